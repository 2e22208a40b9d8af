"""Cost of the helium reionisation call (csrc/heiii.hip) on the 2 x n^3 set of `bench.py --workload hydro`, after the density loop has
converged: K + 2 candidate groups centred on random gas particles, bubbles of 0.02 box (about 70 gas rows each at n = 128, hardly any overlap:
every row is tested against every bubble of its batch, the scan's worst case), a desired fraction that is never reached and no
insufficient-ionisation stop, so that the loop runs K + 1 iterations and lights K bubbles but for the choices of list position 0.
K = 1, 64, 1024, each at batch sizes 1, 8 and the default 64.  Wall clock around synchronised calls, flag and entropy restored before each,
two warm-up calls, the median of `calls` calls; from the engine's own events the scan kernels, the copies of the counts and the apply
passes, summed over the batches.  The yardsticks, in the same run: ONE k_density pass (mpg_dev_density at the prescribed radii,
update_hsml = 0) over K gas targets and over all gas; the fraction count alone.  Prints one JSON line.
    python tools/heiii_time.py [n] [calls]"""
import importlib, json, os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

if __name__ == "__main__":
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 128
    calls = int(sys.argv[2]) if len(sys.argv) > 2 else 10
    pkg = importlib.import_module("mp-gadget_amd")
    import torch
    E = pkg.engine
    dev = torch.device("cuda", 0)
    f8 = torch.float64
    pos, mass, typ, box = pkg.ics.hydro_pair(n)
    N = len(pos)
    res = {"n": n, "particles": N, "calls": calls}
    rs = np.random.RandomState(5)
    gas0 = np.nonzero(typ == 0)[0]
    atime = 0.22
    eng = pkg.Engine(0)
    eng.use_torch_stream()
    eng.set_gravshort_treepar()
    eng.gravshort_set_softenings(box / n)
    eng.set_densitypar(1.0, 2.0, 2.0, 99999., E.DENSITY_KERNEL_QUINTIC_SPLINE, 0.006)
    d_pos, d_mass, d_type = torch.from_numpy(pos).to(dev), torch.from_numpy(mass).to(dev), torch.from_numpy(typ.astype(np.uint8)).to(dev)
    eng.dev_bind_particles(d_pos, d_mass, box, type=d_type)
    z1 = lambda: torch.zeros(N, dtype=f8, device=dev)
    z3 = lambda: torch.zeros(N, 3, dtype=f8, device=dev)
    a = dict(hsml=z1(), dthsml=z1(), vel=z3(), entropy=torch.ones(N, dtype=f8, device=dev), density=z1(), egywtdensity=z1(),
             dhsmlegyfac=z1(), divvel=z1(), curlvel=z1(), hydroacc_out=z3(), dtentropy_out=z1(), maxsignalvel=z1())
    t = pkg.SphTimes()
    t.atime, t.hubble = atime, 0.8
    eng.dev_force_tree_rebuild_mask(E.GASMASK + E.BHMASK, with_moments=True)
    eng.dev_set_init_hsml(a, box / n)
    eng.dev_force_tree_rebuild_mask(E.GASMASK)
    eng.dev_density(a, t, DoEgyDensity=1)
    torch.cuda.synchronize()
    eng.set_random_table(np.clip(rs.random_sample(1 << 20), 1e-12, None))
    eng.set_heiii_params(dict(qso_candidate_min_mass=100.0, qso_candidate_max_mass=1000.0, mean_bubble=0.02 * box, var_bubble=0.0, heIIIreion_finish_frac=2.0))
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    flag0 = torch.zeros(N, dtype=torch.uint8, device=dev)
    ent0 = torch.ones(N, dtype=f8, device=dev)
    st = dict(atime=atime, desired_ion_frac=0.999, qso_inst_heating=2.9e-11, uu_in_cgs=1e10, n_gas_tot=len(gas0), non_overlapping_bubble_number=0, TotNgroups=12345)
    med = lambda v: float(np.median(v))
    tc = []
    for k in range(calls + 2):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        eng.dev_heiii_ionization_fraction(flag0, len(gas0))
        if k >= 2:
            tc.append((time.perf_counter() - t0) * 1e3)
    res["ionization_fraction_call_ms"] = med(tc)
    for K in (1, 64, 1024):
        ng = K + 2
        # candidates among three times as many groups outside the window
        gm = np.full(3 * ng, 5000.0)
        gm[rs.choice(3 * ng, ng, replace=False)] = 500.0
        groups = dict(mass=up(gm), cm=up(pos[rs.choice(gas0, 3 * ng, replace=False)]), minid=up(rs.randint(1, 1 << 48, 3 * ng).astype(np.int64)))
        out = {"bubbles": K}
        for B in (1, 8, 0):
            eng.heiii_set_batch(B)
            ts, ph = [], []
            for k in range(calls + 2):
                flag, ent = flag0.clone(), ent0.clone()
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                r = eng.dev_heiii_reionization(st, a["density"], ent, flag, groups)
                torch.cuda.synchronize()
                if k >= 2:
                    ts.append((time.perf_counter() - t0) * 1e3)
                    ph.append(eng.heiii_times())
            assert r["iterations"] == K + 1 and r["stop_reason"] == E.HEIII_EXHAUSTED, r
            out["B_%s" % (B or "default")] = {"call_ms": med(ts), "call_spread_ms": [float(min(ts)), float(max(ts))], "scan_ms": med([p["scan_ms"] for p in ph]),
                                              "copy_ms": med([p["copy_ms"] for p in ph]), "apply_ms": med([p["apply_ms"] for p in ph]),
                                              "batches": -(-(K + 1) // (B or 64)), "rows_ionised": int(r["tot_n_ionized"])}
        for label, act in (("density_one_pass_K_targets_ms", up(np.sort(rs.choice(gas0, K, replace=False)).astype(np.int32))), ("density_one_pass_all_gas_ms", None)):
            td = []
            for k in range(calls + 2):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                eng.dev_density(a, t, active=act, update_hsml=0, DoEgyDensity=1)
                torch.cuda.synchronize()
                if k >= 2:
                    td.append((time.perf_counter() - t0) * 1e3)
            out[label] = med(td)
        res["bubbles_%d" % K] = out
    eng.close()
    print(json.dumps(res), flush=True)
