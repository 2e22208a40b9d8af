"""Cost of the lensing potential planes (csrc/planes.hip): 256^3 s_zel, 9 planes (three cut points x three normals) at R = 4096.
(a) the counting pass alone (mpg_dev_plane_counts: zeroing the counters, the one pass over the particles, the per-plane sums and the
read-back of the sums), (b) the whole particle-plane call, (c) the call with the Nmesh = 512 massive-neutrino correction (a synthetic
callback, its own time measured inside it).  Wall clock around synchronised calls, warm-up first, medians.  The numpy restatement
(tests/planes_restated.py) is timed in the same process on ONE plane - (b): its counting and solve; (c): the mesh pass once and one
plane's projection, solve and resampling - because nine of them take minutes.  Prints one JSON line.
    python tools/plane_time.py [n] [R] [nmesh] [calls]
Under `rocprofv3 --kernel-trace --stats -- python tools/plane_time.py 256 4096 512 3 nocpu` the kernel times of the passes."""
import importlib, json, os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

if __name__ == "__main__":
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 256
    R = int(sys.argv[2]) if len(sys.argv) > 2 else 4096
    nmesh = int(sys.argv[3]) if len(sys.argv) > 3 else 512
    calls = int(sys.argv[4]) if len(sys.argv) > 4 else 10
    cpu = not (len(sys.argv) > 5 and sys.argv[5] == "nocpu")
    pkg = importlib.import_module("mp-gadget_amd")
    import torch
    dev = torch.device("cuda", 0)
    pos, mass, box = pkg.ics.s_zel(n)
    eng = pkg.Engine(0)
    eng.use_torch_stream()
    eng.gravpm_init_periodic(box, 1.5, nmesh, 43.0071)
    d_pos, d_mass = torch.from_numpy(pos).to(dev), torch.from_numpy(mass).to(dev)
    eng.dev_bind_particles(d_pos, d_mass, box)
    cosmo = dict(atime=0.5, comoving_distance=2.5e5, HubbleParam=0.7, omega_source=0.27)
    kw = dict(Thickness=box / 3, **cosmo)
    counts = torch.empty((3, 3, R, R), dtype=torch.int32, device=dev)
    planes = torch.empty((3, 3, R, R), dtype=torch.float64, device=dev)
    cb_ms = []

    def fn(kk, dcdm, nm):
        t0 = time.perf_counter()
        r = np.log(kk), 0.3 / (1 + (kk / kk[len(kk) // 3]) ** 2), 0.07, 1.05
        cb_ms.append((time.perf_counter() - t0) * 1e3)
        return r

    def timed(f, k):
        ts = []
        for _ in range(k):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            f()
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3)
        return ts

    fa = lambda: eng.dev_plane_counts(R, [0, 1, 2], out=counts, **kw)
    fb = lambda: eng.dev_potential_planes(R, [0, 1, 2], out=planes, **kw)
    fc = lambda: eng.dev_potential_planes(R, [0, 1, 2], out=planes, nu_response=fn, BoxSize_in_MPC=box / 1000.0, **kw)
    for f in (fa, fb, fc):
        timed(f, 2)                          # warm-up: plans, buffers, the deposit tuner
    cb_ms.clear()
    ta, tb, tc = timed(fa, calls), timed(fb, calls), timed(fc, calls)
    read_bytes = len(pos) * 24               # the bound arrays the pass reads: Pos (no type / flags bound here)
    res = {"n": n, "R": R, "nmesh": nmesh, "planes": 9, "calls": calls,
           "count_ms": float(np.median(ta)), "count_spread_ms": [float(min(ta)), float(max(ta))],
           "planes_ms": float(np.median(tb)), "planes_spread_ms": [float(min(tb)), float(max(tb))],
           "planes_nu_ms": float(np.median(tc)), "planes_nu_spread_ms": [float(min(tc)), float(max(tc))],
           "callback_ms": float(np.median(cb_ms)), "read_bound_ms_at_5p3TBs": read_bytes / 5.3e12 * 1e3,
           "counter_bytes": 9 * R * R * 4}
    if cpu:
        import planes_restated as PR
        t0 = time.perf_counter()
        one = PR.potential_planes(pos, box, R, [2], CutPoints=[box / 2], **kw)
        res["numpy_one_plane_s"] = time.perf_counter() - t0
        t0 = time.perf_counter()
        act = np.ones(len(pos), bool)
        real, tm, _ = PR.correction_mesh(pos, mass, act, box, nmesh, box / 1000.0, fn)
        res["numpy_nu_mesh_s"] = time.perf_counter() - t0
        t0 = time.perf_counter()
        corr = PR.correction_plane(real, tm, box, 2, box / 2, box / 3, cosmo["comoving_distance"], cosmo["atime"], cosmo["HubbleParam"],
                                   cosmo["omega_source"])
        PR.bilinear_add(one["planes"][0, 0], corr)
        res["numpy_nu_one_plane_s"] = time.perf_counter() - t0
    print(json.dumps(res), flush=True)
    eng.close()
