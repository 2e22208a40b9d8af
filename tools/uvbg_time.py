"""Cost of the excursion-set reionisation call (csrc/uvbg.hip) on the 2 x n^3 set of `bench.py --workload hydro`, 2 % of the gas rows turned
into stars with halo masses in their escape fraction, at UVBGdim 128 and 256 with the real-space top hat: wall clock around synchronised
calls of mpg_dev_calculate_uvbg with the columns restored before each, two warm-up calls, the median of `calls` calls.  The radii loop alone
is the difference between a call with all radii (ReionRBubbleMax = 0.3 box down to ReionRBubbleMin = 2 cells at 1.1: about 40 radii) and a
call whose only step is the unfiltered one (ReionRBubbleMax below ReionRBubbleMin), over the number of radii between them.  The yardstick,
in the same run: mpg_dev_gravpm_force (deposit, transforms, read-out of one PM step) on a mesh of UVBGdim.  Prints one JSON line.
    python tools/uvbg_time.py [n] [calls]"""
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
    rs = np.random.RandomState(5)
    typ = typ.astype(np.uint8)
    gas = np.nonzero(typ == 0)[0]
    typ[rs.choice(gas, len(gas) // 50, replace=False)] = 4
    halo = np.where(rs.random_sample(N) < 0.5, 10 ** rs.uniform(-2, 2, N), 0.0)
    sfr = rs.uniform(0, 2e-3, N)
    res = {"n": n, "particles": N, "stars": int((typ == 4).sum()), "calls": calls}
    eng = pkg.Engine(0)
    eng.use_torch_stream()
    d_pos, d_mass, d_type = torch.from_numpy(pos).to(dev), torch.from_numpy(mass).to(dev), torch.from_numpy(typ).to(dev)
    eng.dev_bind_particles(d_pos, d_mass, box, type=d_type)
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    halo0, zre0 = up(halo), up(np.full(N, -1.0))
    cols = dict(sfr=up(sfr), escfrac=halo0.clone(), local_J21=torch.zeros(N, dtype=f8, device=dev), zreion=zre0.clone())
    med = lambda v: float(np.median(v))
    base = dict(ReionFilterType=0, RtoMFilterType=0, ReionDeltaRFactor=1.1, ReionNionPhotPerBary=4000.0, AlphaUV=3.0, EscapeFractionNorm=0.3,
                EscapeFractionScaling=0.5, ReionSFRTimescale=0.5, Time=0.125, Omega0=0.2814, OmegaBaryon=0.0464, RhoCrit=2.77536627e-8,
                HubbleParam=0.697, hubble=1.3e-3, UnitLength_in_cm=3.085678e21, UnitMass_in_g=1.989e43, UnitTime_in_s=3.08568e16, NTask=1)

    def timed(par):
        ts, r = [], None
        for k in range(calls + 2):
            cols["escfrac"].copy_(halo0)
            cols["zreion"].copy_(zre0)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            r = eng.dev_calculate_uvbg(par, cols)
            torch.cuda.synchronize()
            if k >= 2:
                ts.append((time.perf_counter() - t0) * 1e3)
        return ts, r

    for dim in (128, 256):
        cell = box / dim
        out = {}
        for use_sfr in (0, 1):
            par = dict(base, UVBGdim=dim, ReionUseParticleSFR=use_sfr, ReionRBubbleMax=0.3 * box, ReionRBubbleMin=2 * cell)
            ts, r = timed(par)
            t1, r1 = timed(dict(par, ReionRBubbleMax=cell, ReionRBubbleMin=2 * cell))
            assert len(r1["radii"]) == 1
            nr = len(r["radii"])
            out["sfr_%d" % use_sfr] = {"radii": nr, "call_ms": med(ts), "call_spread_ms": [float(min(ts)), float(max(ts))],
                                       "one_step_call_ms": med(t1), "per_radius_ms": (med(ts) - med(t1)) / (nr - 1),
                                       "volume_weighted_global_xHI": r["volume_weighted_global_xHI"]}
        G = 43.0071
        eng.gravshort_fill_ntab(0, 1.5)
        eng.gravpm_init_periodic(box, 1.5, dim, G)
        gpm = torch.zeros(N, 3, dtype=f8, device=dev)
        tp = []
        for k in range(calls + 2):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            eng.dev_gravpm_force(gpm)
            torch.cuda.synchronize()
            if k >= 2:
                tp.append((time.perf_counter() - t0) * 1e3)
        out["gravpm_force_same_mesh_ms"] = med(tp)
        res["dim_%d" % dim] = out
    eng.close()
    print(json.dumps(res), flush=True)
