"""Cost of the DM velocity dispersion loop (csrc/veldisp.hip) on the 2 x n^3 DM + gas set of `bench.py --workload hydro`, after the
density loop has converged the smoothing lengths: mpg_dev_find_vel_disp with a threshold that lets (a) all gas and (b) about 10 % of the
gas qualify.  Wall clock around synchronised calls, warm-up first, the median of `calls` calls; the iterations of the radius loop and the
time per iteration (the call less the DM tree build, which is timed alone).  The yardstick, in the same run: one k_density pass
(mpg_dev_density with update_hsml = 0 on the gas tree) over the same number of targets - the same search with one radius instead of
five, against the gas tree.  Prints one JSON line.
    python tools/veldisp_time.py [n] [calls]"""
import importlib, json, os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

if __name__ == "__main__":
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 128
    calls = int(sys.argv[2]) if len(sys.argv) > 2 else 10
    pkg = importlib.import_module("mp-gadget_amd")
    import torch
    dev = torch.device("cuda", 0)
    f8 = torch.float64
    pos, mass, typ, box = pkg.ics.hydro_pair(n)
    N = len(pos)
    eng = pkg.Engine(0)
    eng.use_torch_stream()
    eng.set_gravshort_treepar()
    eng.gravshort_set_softenings(box / n)
    eng.set_densitypar(1.0, 2.0, 2.0, 99999., pkg.engine.DENSITY_KERNEL_QUINTIC_SPLINE, 0.006)
    d_pos, d_mass, d_type = torch.from_numpy(pos).to(dev), torch.from_numpy(mass).to(dev), torch.from_numpy(typ).to(dev)
    eng.dev_bind_particles(d_pos, d_mass, box, type=d_type)
    z1 = lambda: torch.zeros(N, dtype=f8, device=dev)
    z3 = lambda: torch.zeros(N, 3, dtype=f8, device=dev)
    vel = torch.from_numpy(100.0 * np.random.RandomState(1).standard_normal((N, 3))).to(dev)
    a = dict(hsml=z1(), dthsml=z1(), vel=vel, entropy=torch.ones(N, dtype=f8, device=dev), density=z1(), egywtdensity=z1(),
             dhsmlegyfac=z1(), divvel=z1(), curlvel=z1(), hydroacc_out=z3(), dtentropy_out=z1(), maxsignalvel=z1())
    t = pkg.SphTimes()
    t.atime, t.hubble = 0.1, 0.1
    for i in range(47):
        t.dloga_bin[i] = 0.01
    eng.dev_force_tree_rebuild_mask(pkg.engine.GASMASK + pkg.engine.BHMASK, with_moments=True)
    eng.dev_set_init_hsml(a, box / n)
    for _ in range(2):                           # converge Hsml; Density is what the threshold is compared with
        eng.dev_force_tree_rebuild_mask(pkg.engine.GASMASK)
        eng.dev_density(a, t)
    torch.cuda.synchronize()
    gas = torch.nonzero(d_type == 0).flatten()
    dens = a["density"][gas]
    v = dict(vel=a["vel"], hsml=a["hsml"], dthsml=a["dthsml"], density=a["density"], vdisp=z1())

    def timed(f, k):
        ts = []
        for _ in range(k):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            f()
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3)
        return ts

    res = {"n": n, "particles": N, "calls": calls}
    fb = lambda: eng.dev_force_tree_rebuild_mask(pkg.engine.DMMASK)
    timed(fb, 2)
    tb = timed(fb, calls)
    res["dm_tree_build_ms"] = float(np.median(tb))
    for label, frac in (("all_gas", 1.0), ("tenth_of_gas", 0.1)):
        thr = 0.0 if frac >= 1.0 else 10.0 * float(torch.quantile(dens[:: max(1, len(dens) // 1000000)], 1.0 - frac))
        f = lambda: eng.dev_find_vel_disp(v, t, 0.1, 0.1, 0.0, thr)
        timed(f, 2)
        ts = timed(f, calls)
        st = eng.veldisp_stats()
        ql = eng.veldisp_export(N)["queue_lengths"]
        ntar = ql[0]
        med = float(np.median(ts))
        # the yardstick: one density pass over as many targets, on the gas tree
        act = gas if frac >= 1.0 else gas[dens >= 0.1 * thr]
        act = act.to(torch.int32).contiguous()
        eng.dev_force_tree_rebuild_mask(pkg.engine.GASMASK)
        fd = lambda: eng.dev_density(a, t, active=act, update_hsml=0)
        timed(fd, 2)
        td = timed(fd, calls)
        sd = eng.sph_stats()
        res[label] = {"targets": int(ntar), "density_targets": int(len(act)), "call_ms": med, "call_spread_ms": [float(min(ts)), float(max(ts))],
                      "iterations": int(st["iterations"]), "targets_all_iterations": int(st["targets"]), "queue_lengths": ql,
                      "ms_per_iteration": (med - res["dm_tree_build_ms"]) / max(int(st["iterations"]), 1),
                      "neighbours": int(st["neighbours"]), "candidates": int(st["candidates"]), "tight": int(st["tight"]),
                      "density_pass_ms": float(np.median(td)), "density_pass_spread_ms": [float(min(td)), float(max(td))],
                      "density_interactions": int(sd["interactions"]), "density_candidates": int(sd["candidates"])}
    print(json.dumps(res), flush=True)
    eng.close()
