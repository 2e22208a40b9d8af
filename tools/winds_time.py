"""Cost of the wind model (csrc/winds.hip) on the 2 x n^3 set of `bench.py --workload hydro`, after the density loop has converged: 1 000 and
100 000 gas particles are turned into new stars - type 4 at the gas particle's place, Hsml the gas particle's own, Vdisp 10 - 20 - and
mpg_dev_winds_and_feedback (ofjt10, p of about 0.3 per neighbour for a star of typical Vdisp) runs on the gas tree built BEFORE they formed.  Wall clock around synchronised calls,
the in/out arrays restored before each, two warm-up calls, the median of `calls` calls; from the engine's own events the weight walk, the
feedback walk and the resolve + apply passes.  The yardstick, in the same run: ONE k_density pass (mpg_dev_density at the prescribed
radii, update_hsml = 0) over the same number of gas targets.
Then the cost of the decoupling in hydro_force: the hydro loop of the same set without a DelayTime column, with a column of zeros, and
with 1 % of the gas decoupled (the smoothing lengths of decoupled sources are stored negated: no load is added to the pair test).
Prints one JSON line.
    python tools/winds_time.py [n] [calls]"""
import importlib, json, math, os, sys, time
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
    res = {"n": n, "particles": N, "calls": calls, "launch_bound": os.environ.get("MPG_EXTRA_FLAGS") or "source default"}
    rs = np.random.RandomState(5)
    gas0 = np.nonzero(typ == 0)[0]
    atime = 0.25
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
    for i in range(47):
        t.dloga_bin[i] = 0.01
    eng.dev_force_tree_rebuild_mask(E.GASMASK + E.BHMASK, with_moments=True)
    eng.dev_set_init_hsml(a, box / n)
    eng.dev_force_tree_rebuild_mask(E.GASMASK)
    eng.dev_density(a, t, DoEgyDensity=1)
    eng.dev_force_tree_calc_hmax()
    torch.cuda.synchronize()
    ngb = float(eng.lib.mpg_get_numngb(eng.h))
    vphys, wtf = 15.0 / atime, 0.5
    par = dict(WindModel=E.WIND_USE_HALO | E.WIND_DECOUPLE_SPH | E.WIND_ISOTROPIC, WindEfficiency=2.0, WindSigma0=vphys * math.sqrt(0.3 * ngb * (1 + 3 * wtf)),
               WindSpeedFactor=3.7, MinWindVelocity=5.0, WindThermalFactor=wtf, WindFreeTravelLength=20.0, WindSpeed=250.0, MaxWindFreeTravelTime=0.1,
               WindFreeTravelDensThresh=0.0)
    eng.set_wind_params(par)
    eng.set_random_table(rs.random_sample(1 << 20))
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    ids = up(rs.permutation(N).astype(np.int64) + 1)
    for nstar in (1000, 100000):
        if nstar > len(gas0) // 4:
            continue
        stars = np.sort(rs.choice(gas0, nstar, replace=False)).astype(np.int32)
        ty = typ.astype(np.uint8).copy()
        ty[stars] = 4
        d_type.copy_(up(ty))                                   # the gas tree is the one built before they formed
        vdisp = np.zeros(N)
        vdisp[stars] = rs.uniform(10.0, 20.0, nstar)
        w = dict(id=ids, hsml=a["hsml"], vdisp=up(vdisp), density=a["density"], vel=z3(), entropy=torch.ones(N, dtype=f8, device=dev),
                 delaytime=z1(), totalweight=z1())
        keep = {k: w[k].clone() for k in ("vel", "entropy", "delaytime")}
        d_stars = up(stars)
        ts, ph = [], []
        for k in range(calls + 2):
            for key, v in keep.items():
                w[key].copy_(v)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            eng.dev_winds_and_feedback(w, d_stars, atime)
            torch.cuda.synchronize()
            if k >= 2:
                ts.append((time.perf_counter() - t0) * 1e3)
                ph.append(eng.winds_times())
        st = eng.winds_stats()
        med = lambda key: float(np.median([p[key] for p in ph]))
        out = {"stars": int(nstar), "call_ms": float(np.median(ts)), "call_spread_ms": [float(min(ts)), float(max(ts))],
               "weight_ms": med("weight_ms"), "feedback_ms": med("feedback_ms"), "apply_ms": med("apply_ms"),
               "candidates": int(st["candidates"]), "neighbours": int(st["neighbours"]), "potential_kicks": int(st["potential_kicks"]),
               "applied": int(st["applied"]), "discarded": int(st["discarded"])}
        d_type.copy_(up(typ.astype(np.uint8)))
        act = d_stars
        td = []
        for k in range(calls + 2):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            eng.dev_density(a, t, active=act, update_hsml=0, DoEgyDensity=1)
            torch.cuda.synchronize()
            if k >= 2:
                td.append((time.perf_counter() - t0) * 1e3)
        out["density_one_pass_same_targets_ms"] = float(np.median(td))
        out["call_over_density_pass"] = out["call_ms"] / out["density_one_pass_same_targets_ms"]
        res["stars_%d" % nstar] = out
    # ---- the decoupling in hydro_force
    delay = np.zeros(N)
    delay[rs.choice(gas0, len(gas0) // 100, replace=False)] = 0.05
    hyd = {}
    for label, col in (("no_column", None), ("column_of_zeros", z1()), ("one_percent_decoupled", up(delay))):
        eng.dev_set_delaytime(col)
        th = []
        for k in range(calls + 2):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            eng.dev_hydro_force(a, t)
            torch.cuda.synchronize()
            if k >= 2:
                th.append((time.perf_counter() - t0) * 1e3)
        hyd[label] = {"hydro_force_ms": float(np.median(th)), "spread_ms": [float(min(th)), float(max(th))], "pairs": int(eng.sph_stats()["interactions"])}
    eng.dev_set_delaytime(None)
    res["hydro_force"] = hyd
    eng.close()
    print(json.dumps(res), flush=True)
