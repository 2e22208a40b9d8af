"""Cost of the excursion set's J21 in cooling and star formation (get_local_UVBG_from_J21; csrc/cooling.hip, csrc/sfr.hip) on the gas of
tools/sfr_time.py's set (2 x n^3 particles of `bench.py --workload hydro` after the density loop has converged, the `igm` inputs,
Verner96 / Sherwood at z = 3): mpg_dev_cooling over all gas and mpg_dev_cooling_and_starformation with the densest tenth of the gas on the
effective equation of state, each with the global background (no model: the plain path), with the J21 columns (a third of the rows never
ionised, the others with J21 = 1e-2 .. 1e1 log-uniform, about the global background in the middle) and with a UV-fluctuation table that
leaves half of the gas dark (the form the J21 one is set beside), on the same inputs in the same process.  On a library without
mpg_set_excursion_set only the plain path is timed: that is how an older build is put beside this one.  Wall clock around synchronised
calls, the inputs restored before each, two warm-up calls, the median of `calls`.  Prints one JSON line.
    python tools/excursion_cooling_time.py [n] [calls]"""
import importlib, json, os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import cooling_restated as R
import sfr_restated as SF
from cooling_time import setting, ATIME

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
    gas = (d_type == 0)
    ngas = int(gas.sum())
    a3inv = 1 / ATIME ** 3
    redshift = 1 / ATIME - 1
    meanrho = float(mass[typ == 0].sum()) / box ** 3
    par = dict(C.p, density_in_phys_cgs=1e-5 * R.PROTONMASS / meanrho)
    eng.set_cooling_params(par)
    eng.set_random_table(SF.random_table())
    rs = np.random.RandomState(3)
    rho = a["density"].clamp(min=1e-300)
    enttou = (rho * a3inv) ** R.GAMMA_MINUS1 / R.GAMMA_MINUS1
    meanweight_ion = 4 / (8 - 5 * (1 - R.HYDROGEN_MASSFRAC))
    ent0 = torch.from_numpy(par["temp_to_u"] / meanweight_ion * 10 ** rs.uniform(3.5, 4.5, N)).to(dev) / enttou
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    cols = dict(id=up(np.arange(N, dtype=np.int64) * 7), generation=up(np.zeros(N, np.uint8)), density=a["density"], tb_hydro=up(np.full(N, 3, np.uint8)),
                entropy=ent0.clone(), ne=torch.ones(N, dtype=f8, device=dev), sfr=z1(), metallicity=up(rs.uniform(0, 0.02, N)),
                bhheated=up((np.arange(N) % 5 == 2).astype(np.uint8)))
    cool_cols = {k: cols[k] for k in ("density", "entropy", "ne", "sfr", "metallicity", "tb_hydro")}
    rho_gas = (a["density"][gas] * a3inv).cpu().numpy()
    P0 = SF.init_star_formation(R.Cooling(par, R.TreeCool(np.load(os.path.join(ROOT, "tests", "golden", "cooling_kat.npz"))["treecool"])),
                                BHFeedbackUseTcool=1, avg_baryon_mass=float(mass[typ == 0].mean()))
    sfr_par = dict(P0, PhysDensThresh=float(np.quantile(rho_gas, 0.9)), OverDensThresh=0.0)
    res = {"n": n, "gas": ngas, "calls": calls}

    def timed(call):
        ts = []
        for k in range(calls + 2):
            cols["entropy"].copy_(ent0)
            cols["ne"].fill_(1.0)
            cols["sfr"].zero_()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            call()
            torch.cuda.synchronize()
            if k >= 2:
                ts.append((time.perf_counter() - t0) * 1e3)
        return {"call_ms": float(np.median(ts)), "call_spread_ms": [float(min(ts)), float(max(ts))]}

    def both(label, **flags):
        eng.set_sfr_params(SF.engine_params(dict(sfr_par, **flags)))
        res["cooling_" + label] = dict(timed(lambda: eng.dev_cooling(cool_cols, t, step)), evaluations=int(eng.cooling_stats()["evaluations"]))
        out = timed(lambda: eng.dev_cooling_and_starformation(cols, t, step))
        r = eng.sfr_result()
        out.update(cooled=r["cooled"], starforming=r["sum_sf_part"], sf_evaluations=eng.sfr_stats()["evaluations"],
                   cooling_evaluations=int(eng.cooling_stats()["evaluations"]))
        res["cooling_and_starformation_" + label] = out

    both("plain")
    if hasattr(eng, "set_excursion_set"):
        model = pkg.excursion.params(pkg.excursion.J21Coeffs.load(os.path.join(ROOT, "tests", "golden", "J21_to_rates_test.txt")), 0.7, 1, 2.0)
        kind = rs.randint(0, 3, N)
        J21 = up(np.where(kind == 0, 0.0, 10 ** rs.uniform(-2, 1, N)))
        zre = up(np.where(kind == 0, -1.0, redshift + rs.uniform(0.5, 5.0, N)))
        eng.set_excursion_set(model)
        eng.dev_set_excursion_columns(J21, zre)
        both("J21", ExcursionSetReion=1)
        eng.set_excursion_set(dict(model, ExcursionSetZStop=redshift))     # the model loaded, the redshift not above ZStop: the plain kernels
        both("plain_with_model_below_zstop", ExcursionSetReion=1)
        eng.set_excursion_set()
        eng.dev_set_excursion_columns()
        nside = 64
        g = np.arange(nside) / float(nside)
        table = redshift + 0.9 * np.sin(2 * np.pi * g)[:, None, None] * np.cos(2 * np.pi * g)[None, :, None] + 0.5 * np.sin(2 * np.pi * g)[None, None, :]
        eng.set_uvf_table(table, box)
        both("uvf_table", UVFluctuationOn=1)
        eng.set_uvf_table()
        for k in ("cooling", "cooling_and_starformation"):
            res[k + "_J21_over_uvf"] = res[k + "_J21"]["call_ms"] / res[k + "_uvf_table"]["call_ms"]
            res[k + "_J21_over_plain"] = res[k + "_J21"]["call_ms"] / res[k + "_plain"]["call_ms"]
    print(json.dumps(res), flush=True)
    eng.close()
