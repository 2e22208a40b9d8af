"""Cost of the UV-fluctuation table (patchy reionisation, csrc/cooling.hip) on the gas of tools/cooling_time.py's set (2 x n^3 particles of
`bench.py --workload hydro`, the `igm` inputs, Verner96 / Sherwood at z = 3): the table pass alone (mpg_dev_uvf_zreion on the gas
positions), and mpg_dev_cooling over all gas without a table, with a table of Nside^3 entries whose zreion lies on both sides of the
redshift (half of the gas dark: other physics, other evaluation counts), and with a table that leaves every row lit (the same arithmetic).
Every time is taken from a pair of events on the engine's stream around the call, the inputs restored before each call, two warm-up calls,
the median of `calls`.  Prints one JSON line.
    python tools/uvf_time.py [n] [calls] [Nside]"""
import importlib, json, os, sys
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import cooling_restated as R
from cooling_time import ATIME, setting

if __name__ == "__main__":
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 128
    calls = int(sys.argv[2]) if len(sys.argv) > 2 else 10
    nside = int(sys.argv[3]) if len(sys.argv) > 3 else 400
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
    ngas = int((typ == 0).sum())
    a3inv = 1 / ATIME ** 3
    meanrho = float(mass[typ == 0].sum()) / box ** 3
    par = dict(C.p, density_in_phys_cgs=1e-5 * R.PROTONMASS / meanrho)
    eng.set_cooling_params(par)
    rs = np.random.RandomState(3)
    enttou = (a["density"].clamp(min=1e-300) * a3inv) ** R.GAMMA_MINUS1 / R.GAMMA_MINUS1
    u_igm = par["temp_to_u"] / (4 / (8 - 5 * (1 - R.HYDROGEN_MASSFRAC))) * 10 ** rs.uniform(3.5, 4.5, N)
    ent0, ne0 = torch.from_numpy(u_igm).to(dev) / enttou, torch.ones(N, dtype=f8, device=dev)
    c = dict(density=a["density"], entropy=ent0.clone(), ne=ne0.clone(), sfr=z1())
    # a smooth field around the redshift of the step: about half of the gas is not yet reionised
    g = np.arange(nside) / float(nside)
    table = (1 / ATIME - 1) + 0.9 * np.sin(2 * np.pi * g)[:, None, None] * np.cos(2 * np.pi * g)[None, :, None] + 0.5 * np.sin(2 * np.pi * g)[None, None, :]

    def timed(call):
        ms = []
        for k in range(calls + 2):
            c["entropy"].copy_(ent0)
            c["ne"].copy_(ne0)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            call()
            e1.record()
            torch.cuda.synchronize()
            if k >= 2:
                ms.append(e0.elapsed_time(e1))
        return {"ms": float(np.median(ms)), "spread_ms": [float(min(ms)), float(max(ms))]}

    res = {"n": n, "gas": ngas, "calls": calls, "Nside": nside, "table_MB": table.nbytes / 1e6}
    res["cooling_without_table"] = dict(timed(lambda: eng.dev_cooling(c, t, step)), evaluations=int(eng.cooling_stats()["evaluations"]))
    eng.set_uvf_table(table, box)
    gas_pos, out = d_pos[: ngas].contiguous(), torch.zeros(ngas, dtype=f8, device=dev)      # (the gas comes first in this set)
    res["table_pass_alone"] = timed(lambda: eng.dev_uvf_zreion(gas_pos, out))
    res["dark_fraction"] = float((out < 1 / ATIME - 1).double().mean())
    res["cooling_with_table"] = dict(timed(lambda: eng.dev_cooling(c, t, step)), evaluations=int(eng.cooling_stats()["evaluations"]))
    # ... and with a table of the same size that says "reionised long ago" everywhere: the arithmetic of the call without a table, so the
    # difference to it is what the pass and the per-row choice of the background cost
    eng.set_uvf_table(np.full((nside,) * 3, 100.0), box)
    res["cooling_with_table_all_lit"] = dict(timed(lambda: eng.dev_cooling(c, t, step)), evaluations=int(eng.cooling_stats()["evaluations"]))
    print(json.dumps(res), flush=True)
    eng.close()
