"""Cost of the radiative cooling (csrc/cooling.hip) on the gas of the 2 x n^3 set of `bench.py --workload hydro`, after the density loop has
converged: mpg_dev_cooling over all gas for both kernel forms (MPG_COOLING_FORM 0: one particle per lane to completion, 1: the per-lane
state machine with a wave-aggregated list) and both placements of the six network tables (MPG_COOLING_LDS 0: global memory, 1: LDS), on
two input sets: `igm` (temperatures of 10^3.5 .. 10^4.5 K at the densities the loop found, the mean at 1e-5 protons/cm^3 comoving - a
photo-heated intergalactic medium at z = 3) and `spread` (u = 1 .. 3e6 and a start value of Ne in 0 .. 1.2, the spread of the tests).
Verner96 / Sherwood with self-shielding at z = 3, the UV background of tests/golden/cooling_kat.npz.  Wall clock around synchronised
calls, the inputs restored before each, warm-up first, the median of `calls` calls; the histogram of network evaluations per particle.
The yardstick, in the same run: the restated loop (tests/cooling_restated.py) on 16 host processes over a sample, scaled to all gas.
Prints one JSON line.
    python tools/cooling_time.py [n] [calls] [host sample per process]"""
import importlib, json, os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import cooling_restated as R

TREECOOL = np.load(os.path.join(ROOT, "tests", "golden", "cooling_kat.npz"))["treecool"]
ATIME = 0.25


def setting(**over):
    C = R.Cooling(R.default_params(**over), R.TreeCool(TREECOOL))
    redshift = 1 / ATIME - 1
    step = dict(uvbg=C.get_global_UVBG(redshift), long_mean_free_path_heating=0.0, lastred=redshift + 0.05, redshift=redshift)
    times = dict(atime=ATIME, hubble=0.1 * ATIME ** -1.5, dloga_bin=np.full(47, 0.02 * 0.1 * ATIME ** -1.5))
    return C, times, step


def host_chunk(args):
    density, entropy, ne, unit = args
    C, times, step = setting(density_in_phys_cgs=unit)
    n = len(density)
    d = dict(type=np.zeros(n, np.uint8), mass=np.ones(n, np.float32), density=density, entropy=entropy, ne=ne, sfr=np.zeros(n))
    t0 = time.perf_counter()
    r = R.cool_particles(C, d, times, step)
    return time.perf_counter() - t0, int(r["evals"].sum())


if __name__ == "__main__":
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 128
    calls = int(sys.argv[2]) if len(sys.argv) > 2 else 10
    sample = int(sys.argv[3]) if len(sys.argv) > 3 else 250
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
    a = dict(hsml=z1(), dthsml=z1(), vel=z3(), entropy=torch.ones(N, dtype=f8, device=dev), density=z1(), egywtdensity=z1(),
             dhsmlegyfac=z1(), divvel=z1(), curlvel=z1(), hydroacc_out=z3(), dtentropy_out=z1(), maxsignalvel=z1())
    C, times, step = setting()
    t = pkg.SphTimes()
    t.atime, t.hubble = times["atime"], times["hubble"]
    for i in range(47):
        t.dloga_bin[i] = times["dloga_bin"][i]
    eng.dev_force_tree_rebuild_mask(pkg.engine.GASMASK + pkg.engine.BHMASK, with_moments=True)
    eng.dev_set_init_hsml(a, box / n)
    for _ in range(2):
        eng.dev_force_tree_rebuild_mask(pkg.engine.GASMASK)
        eng.dev_density(a, t)
    torch.cuda.synchronize()
    gas = torch.nonzero(d_type == 0).flatten()
    ngas = len(gas)
    a3inv = 1 / ATIME ** 3
    # the unit of density: the mean gas density is 1e-5 protons / cm^3 comoving
    meanrho = float(mass[typ == 0].sum()) / box ** 3
    par = dict(C.p, density_in_phys_cgs=1e-5 * R.PROTONMASS / meanrho)
    rs = np.random.RandomState(3)
    rho = a["density"].clamp(min=1e-300)
    enttou = (rho * a3inv) ** R.GAMMA_MINUS1 / R.GAMMA_MINUS1
    meanweight_ion = 4 / (8 - 5 * (1 - R.HYDROGEN_MASSFRAC))
    u_igm = par["temp_to_u"] / meanweight_ion * 10 ** rs.uniform(3.5, 4.5, N)
    sets = dict(igm=(torch.from_numpy(u_igm).to(dev) / enttou, torch.ones(N, dtype=f8, device=dev)),
                spread=(torch.from_numpy(np.exp(rs.uniform(0, np.log(3e6), N))).to(dev) / enttou, torch.from_numpy(rs.uniform(0, 1.2, N)).to(dev)))
    res = {"n": n, "gas": int(ngas), "calls": calls}
    for label, (ent0, ne0) in sets.items():
        c = dict(density=a["density"], entropy=ent0.clone(), ne=ne0.clone(), sfr=z1())
        out = {}
        for form in (0, 1):
            for lds in (0, 1):
                os.environ["MPG_COOLING_FORM"], os.environ["MPG_COOLING_LDS"] = str(form), str(lds)
                eng.set_cooling_params(par)
                ts = []
                for k in range(calls + 2):
                    c["entropy"].copy_(ent0)
                    c["ne"].copy_(ne0)
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    eng.dev_cooling(c, t, step)
                    torch.cuda.synchronize()
                    if k >= 2:
                        ts.append((time.perf_counter() - t0) * 1e3)
                st = eng.cooling_stats()
                out["form%d_lds%d" % (form, lds)] = {"call_ms": float(np.median(ts)), "call_spread_ms": [float(min(ts)), float(max(ts))],
                                                     "evaluations": int(st["evaluations"]), "bisections": int(st["bisections"]), "floor": int(st["floor"]),
                                                     "ns_per_evaluation": float(np.median(ts)) * 1e6 / max(int(st["evaluations"]), 1)}
        ev = eng.cooling_export(N)
        ev = ev[ev >= 0]
        edges = [0, 16, 24, 32, 48, 64, 96, 128, 192, 256, 384, 512, 1 << 30]
        out["evaluations_per_particle"] = {"min": int(ev.min()), "median": float(np.median(ev)), "mean": float(ev.mean()), "max": int(ev.max()),
                                           "histogram_edges": edges[:-1], "histogram": [int(x) for x in np.histogram(ev, edges)[0]]}
        # the mean of the per-wave maxima over 64 consecutive particles: what the first form pays per wave against the mean it needs
        w = ev[: len(ev) // 64 * 64].reshape(-1, 64)
        out["wave_max_over_mean"] = float(w.max(1).mean() / w.mean())
        # the yardstick: the restated loop on 16 host processes over a sample, scaled to all gas
        from multiprocessing import get_context
        idx = gas.cpu().numpy()[rs.choice(ngas, 16 * sample, replace=False)]
        dens_h, ent_h, ne_h = a["density"].cpu().numpy()[idx], ent0.cpu().numpy()[idx], ne0.cpu().numpy()[idx]
        with get_context("spawn").Pool(16) as pool:
            t0 = time.perf_counter()
            parts = pool.map(host_chunk, [(dens_h[k::16], ent_h[k::16], ne_h[k::16], par["density_in_phys_cgs"]) for k in range(16)])
            wall = time.perf_counter() - t0
        out["host_restated_16_processes"] = {"sample": int(16 * sample), "slowest_process_s": float(max(p[0] for p in parts)), "pool_wall_s": float(wall),
                                             "all_gas_s": float(max(p[0] for p in parts)) * ngas / (16 * sample),
                                             "evaluations": int(sum(p[1] for p in parts))}
        res[label] = out
    del os.environ["MPG_COOLING_FORM"], os.environ["MPG_COOLING_LDS"]
    print(json.dumps(res), flush=True)
    eng.close()
