"""Device time of the black-hole step (mpg_blackhole_get_times) at 2 x 128^3 on one GPU, beside one density pass over as many targets.

    python tools/blackhole_time.py [--n 128] [--nbh 1000 100000] [--calls 10]

Gas of ics.hydro_pair(n); `nbh` gas particles become black holes (Hsml x BlackHoleNgbFactor^(1/3), BHP.Density from the density loop).
Medians of `calls` synchronised calls on fresh copies of the in / out columns; the density pass is k_density at the converged radii
(update_hsml = 0) over `nbh` gas targets.  Prints one JSON line per black-hole count."""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=128)
    ap.add_argument("--nbh", type=int, nargs="+", default=[1000, 100000])
    ap.add_argument("--calls", type=int, default=10)
    args = ap.parse_args()
    import torch
    import blackhole_restated as R
    pkg = importlib.import_module("mp-gadget_amd")
    E = pkg.engine
    pos, mass, typ, box = pkg.ics.hydro_pair(args.n)
    n = len(pos)
    rng = np.random.RandomState(1)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    T = E.SphTimes()
    Td = R.default_times()
    T.FgravkickB, T.atime, T.hubble = Td["FgravkickB"], Td["atime"], Td["hubble"]
    for b in range(47):
        T.gravkicks[b], T.hydrokicks[b], T.dloga_bin[b] = Td["gravkicks"][b], Td["hydrokicks"][b], Td["dloga_bin"][b]
    for nbh in args.nbh:
        t = typ.copy()
        bh = rng.choice(np.nonzero(typ == 0)[0], nbh, replace=False)
        t[bh] = 5
        eng = pkg.Engine(0)
        eng.set_gravshort_treepar()
        eng.gravshort_set_softenings(box / args.n)
        eng.set_densitypar(1.0, 2.0, 2.0, 99999., E.DENSITY_KERNEL_QUINTIC_SPLINE, 0.006)
        par = R.default_params(ForceSoftening=0.0)
        eng.set_blackhole_params(par)
        eng.set_random_table(R.random_table(3, 1 << 16))
        d_pos, d_mass, d_type = up(pos), up(mass.astype(np.float32)), up(t)
        eng.dev_bind_particles(d_pos, d_mass, box, type=d_type)
        z = lambda *s: torch.zeros(*s, dtype=torch.float64, device="cuda")
        a = dict(hsml=z(n), dthsml=z(n), vel=up(0.3 * rng.standard_normal((n, 3))), entropy=torch.ones(n, dtype=torch.float64, device="cuda"), density=z(n),
                 egywtdensity=z(n), dhsmlegyfac=z(n), divvel=z(n), curlvel=z(n))
        eng.dev_force_tree_rebuild_mask(E.GASMASK + E.BHMASK, with_moments=1)
        eng.dev_set_init_hsml(a, box / args.n)
        eng.dev_density(a, T, update_hsml=1, BlackHoleOn=1)
        eng.dev_force_tree_calc_hmax()
        eng.synchronize()
        # one density pass over nbh gas targets at the converged radii
        gas_targets = up(rng.choice(np.nonzero(t == 0)[0], nbh, replace=False).astype(np.int32))
        dens_ms = []
        for _ in range(args.calls):
            eng.synchronize()
            t0 = time.perf_counter()
            eng.dev_density(a, T, active=gas_targets, update_hsml=0, BlackHoleOn=1)
            eng.synchronize()
            dens_ms.append(1e3 * (time.perf_counter() - t0))
        eng.dev_force_tree_calc_hmax()
        u8 = lambda v=0: torch.full((n,), v, dtype=torch.uint8, device="cuda")
        base = dict(id=up(np.arange(1, 2 * n + 1, 2).astype(np.int64)), gacc=z(n, 3), gpm=z(n, 3), hydroacc=z(n, 3), tb_hydro=u8(20), tb_grav=u8(20),
                    hsml=a["hsml"], density=a["density"], delaytime=z(n), dfaccel=z(n, 3), vdisp=z(n) + 0.5)
        bhm = np.zeros(n)
        bhm[bh] = float(mass[typ == 0][0]) * np.exp(rng.standard_normal(nbh))
        times, stats = [], None
        for _ in range(args.calls):
            io = dict(mass=d_mass.clone(), vel=a["vel"].clone(), entropy=a["entropy"].clone(), flags=u8(), bh_mass=up(bhm), mtrack=z(n) + 10.0,
                      kineticfdbkenergy=z(n), countprogs=torch.ones(n, dtype=torch.int32, device="cuda"))
            out = dict(mdot=z(n), dragaccel=z(n, 3), encounter=torch.zeros(n, dtype=torch.int32, device="cuda"),
                       mintimebin=torch.zeros(n, dtype=torch.int32, device="cuda"), swallowid=torch.zeros(n, dtype=torch.int64, device="cuda"),
                       swallowtime=z(n), bhheated=u8())
            eng.synchronize()
            eng.dev_blackhole(dict(base, **io, **out), T)
            eng.synchronize()
            times.append(eng.blackhole_times())
            stats = eng.blackhole_stats()
        med = lambda k: float(np.median([x[k] for x in times]))
        print(json.dumps(dict(n=args.n, nbh=nbh, calls=args.calls, accretion_ms=med("accretion_ms"), feedback_ms=med("feedback_ms"), apply_ms=med("apply_ms"),
                              density_pass_ms_wall=float(np.median(dens_ms)), stats=stats)))
        eng.close()


if __name__ == "__main__":
    main()
