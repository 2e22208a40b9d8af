"""Cost of the stellar mass and metal return (csrc/metals.hip) on the 2 x n^3 set of `bench.py --workload hydro`, after the density loop has
converged: a fraction of the gas (1 % and 10 %) is turned into returning stars - type 4 at the gas particle's place, entry Hsml the gas
particle's own, a return of 1 - 5 % of the mass - and mpg_dev_metal_return runs on the tree of the remaining gas.  Wall clock around
synchronised calls, the in/out arrays restored before each, two warm-up calls, the median of `calls` calls; from the engine's own events
the radius loop (and so the time per pass), the return walk and the apply pass.  The yardstick, in the same run: ONE k_density pass
(mpg_dev_density at the prescribed radii, update_hsml = 0) over the same number of gas targets.
Prints one JSON line.
    python tools/metals_time.py [n] [calls]"""
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
    res = {"n": n, "particles": N, "calls": calls, "launch_bound": os.environ.get("MPG_EXTRA_FLAGS") or "source default"}
    rs = np.random.RandomState(5)
    gas0 = np.nonzero(typ == 0)[0]
    for frac in (0.01, 0.1):
        ty = typ.copy()
        stars = np.sort(rs.choice(gas0, int(frac * len(gas0)), replace=False))
        ty[stars] = 4
        eng = pkg.Engine(0)
        eng.use_torch_stream()
        eng.set_gravshort_treepar()
        eng.gravshort_set_softenings(box / n)
        eng.set_densitypar(1.0, 2.0, 2.0, 99999., pkg.engine.DENSITY_KERNEL_QUINTIC_SPLINE, 0.006)
        d_pos, d_mass, d_type = torch.from_numpy(pos).to(dev), torch.from_numpy(mass).to(dev), torch.from_numpy(ty).to(dev)
        eng.dev_bind_particles(d_pos, d_mass, box, type=d_type)
        z1 = lambda: torch.zeros(N, dtype=f8, device=dev)
        z3 = lambda: torch.zeros(N, 3, dtype=f8, device=dev)
        a = dict(hsml=z1(), dthsml=z1(), vel=z3(), entropy=torch.ones(N, dtype=f8, device=dev), density=z1(), egywtdensity=z1(),
                 dhsmlegyfac=z1(), divvel=z1(), curlvel=z1(), hydroacc_out=z3(), dtentropy_out=z1(), maxsignalvel=z1())
        t = pkg.SphTimes()
        t.atime, t.hubble = 0.25, 0.8
        for i in range(47):
            t.dloga_bin[i] = 0.01
        # smoothing lengths for everything that was gas (the stars keep theirs as the entry Hsml), then the loop on the remaining gas
        d_type.copy_(torch.from_numpy(typ).to(dev))
        eng.dev_force_tree_rebuild_mask(pkg.engine.GASMASK + pkg.engine.BHMASK, with_moments=True)
        eng.dev_set_init_hsml(a, box / n)
        eng.dev_force_tree_rebuild_mask(pkg.engine.GASMASK)
        eng.dev_density(a, t)
        torch.cuda.synchronize()
        d_type.copy_(torch.from_numpy(ty).to(dev))
        for _ in range(2):
            eng.dev_force_tree_rebuild_mask(pkg.engine.GASMASK)
            eng.dev_density(a, t)
        torch.cuda.synchronize()
        nstar = len(stars)
        m64 = mass.astype(np.float64)
        massgen = np.zeros(N)
        massgen[stars] = m64[stars] * rs.uniform(0.01, 0.05, nstar)
        metalgen = 0.02 * massgen
        species = metalgen[:, None] * np.full((1, 9), 0.1)
        up = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
        m = dict(massgenerated=up(massgen), metalgenerated=up(metalgen), speciesgenerated=up(species), stellarage=up(np.full(N, 100.0)),
                 mass=d_mass, hsml=a["hsml"], totalmassreturned=z1(), lastenrichment=z1(), density=a["density"], metallicity=z1(),
                 metals=torch.zeros(N, 9, dtype=f8, device=dev), massreturned=z1(), starvolume=z1())
        eng.set_metal_params(1, 2.0, 4.0 * float(m64[gas0].mean()))
        keep = {k: m[k].clone() for k in ("mass", "hsml", "totalmassreturned", "lastenrichment", "density", "metallicity", "metals")}
        ts, ph = [], []
        for k in range(calls + 2):
            for key, v in keep.items():
                m[key].copy_(v)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            eng.dev_metal_return(m)
            torch.cuda.synchronize()
            if k >= 2:
                ts.append((time.perf_counter() - t0) * 1e3)
                ph.append(eng.metals_times())
        st = eng.metals_stats()
        med = lambda key: float(np.median([p[key] for p in ph]))
        out = {"stars": int(nstar), "call_ms": float(np.median(ts)), "call_spread_ms": [float(min(ts)), float(max(ts))],
               "iterations": int(st["iterations"]), "targets_over_iterations": int(st["targets"]), "loop_ms": med("loop_ms"),
               "ms_per_pass": med("loop_ms") / max(int(st["iterations"]), 1), "scatter_ms": med("scatter_ms"), "apply_ms": med("apply_ms"),
               "candidates": int(st["candidates"]), "neighbours": int(st["neighbours"]), "refused": int(st["refused"]), "tight": int(st["tight"])}
        for key, v in keep.items():
            m[key].copy_(v)
        # the yardstick: one k_density pass over as many gas targets
        gas = torch.nonzero(d_type == 0).flatten()
        act = gas[torch.from_numpy(np.sort(rs.choice(len(gas), nstar, replace=False))).to(dev)].to(torch.int32).contiguous()
        td = []
        for k in range(calls + 2):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            eng.dev_density(a, t, active=act, update_hsml=0)
            torch.cuda.synchronize()
            if k >= 2:
                td.append((time.perf_counter() - t0) * 1e3)
        out["density_one_pass_same_targets_ms"] = float(np.median(td))
        out["call_over_density_pass"] = out["call_ms"] / out["density_one_pass_same_targets_ms"]
        res["frac_%g" % frac] = out
        eng.close()
    print(json.dumps(res), flush=True)
