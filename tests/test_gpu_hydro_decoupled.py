"""GPU tests of the wind model's decoupling in hydro_force (csrc/sph.hip, k_hydro<true>): gas with DelayTime > 0 is no hydro source
(hydra.c:360-363) and, as a target, keeps only MaxSignalVel, rescaled (winds_decoupled_hydro, winds.c:122-136).

Scene: ics.hydro_pair(16) (16^3 gas + 16^3 dark matter) after a density pass on the device.  The decoupled set D (about 200 gas particles):
100 isolated members drawn at random, a clump of one particle and its 60 nearest neighbours, and the 40 gas particles nearest to a face of
the box.  Expected values come from the CPU oracle's hydro loop (the `orc` fixture, unchanged):
  targets outside D   the oracle on the particle set WITHOUT D (their rows carry type 1 there: not in its gas tree), with the device's
                      density-stage fields of the full set.  HydroAccel and DtEntropy to 1e-10, MaxSignalVel to 1e-12 (the tolerances and
                      the norm of test_gpu_sph.py).
  targets in D        HydroAccel == 0 and DtEntropy == 0 exactly; for eight of them (isolated, clump, face) MaxSignalVel against
                      hsml_c max(2 windspeed, M), M the oracle's MaxSignalVel of that target on (set without D) + {target}, to 1e-12.
                      WindSpeed is the median of M / (2 atime fac_mu) over the eight, so both sides of the maximum occur.
With the bit set and every DelayTime zero the outputs equal those of a call without a column; whether bit for bit is printed.
The host setters (mpg_set_delaytime for mpg_hydro_force, mpg_resident_sph_set_delaytime for a resident gas run) give the dev form's result."""
import numpy as np
import pytest

import winds_restated as R
from oracle import oracle as O
from test_gpu_cooling import device_view
from test_gpu_sph import gpu_arrays, make_times, rel

pytestmark = pytest.mark.gpu

GAMMA = 5.0 / 3.0
TK = dict(atime=0.5, hubble=0.3)
PE = 1
OUT = ("hydroacc_out", "dtentropy_out", "maxsignalvel")
STAGE = ("hsml", "density", "egywtdensity", "dhsmlegyfac", "divvel", "curlvel")
_cache = {}


def scene(pkg):
    if "scene" in _cache:
        return _cache["scene"]
    pos, mass, typ, box = pkg.ics.hydro_pair(16)
    typ = typ.astype(np.int32)
    N = len(pos)
    rng = np.random.RandomState(17)
    gas = np.flatnonzero(typ == 0)
    pg = pos[gas]
    face = gas[np.argsort(np.minimum(pg, box - pg).min(1))[:40]]
    centre = gas[rng.randint(len(gas))]
    dist = pos[centre] - pg
    dist -= box * np.rint(dist / box)
    clump = gas[np.argsort((dist ** 2).sum(1))[:61]]
    rest = np.setdiff1d(gas, np.concatenate([face, clump]))
    iso = rng.choice(rest, 100, replace=False)
    D = np.unique(np.concatenate([iso, clump, face]))
    delay = np.zeros(N)
    delay[D] = 0.01 + 0.05 * rng.random_sample(len(D))
    delay[typ != 0] = 0.03                          # DelayTime of rows that are no gas is never read
    eight = np.concatenate([iso[:3], clump[:3], face[:2]])
    s = dict(pos=pos, mass=mass, typ=typ, box=box, N=N, gas=gas, D=D, eight=eight, delay=delay, h0=np.full(N, 2.5 * box / 16),
             vel=100.0 * rng.standard_normal((N, 3)), ent=1.0 + 0.5 * rng.random_sample(N))
    _cache["scene"] = s
    return s


def new_engine(pkg, s, par=None):
    eng = pkg.Engine(0)
    eng.set_gravshort_treepar()
    eng.gravshort_set_softenings(s["box"] / 16)
    eng.set_densitypar(1.0, 2.0, 2.0, 99999., pkg.engine.DENSITY_KERNEL_QUINTIC_SPLINE, 0.006)
    eng.set_hydropar(PE, 100.0, 0.75)
    if par is not None:
        eng.set_wind_params(par)
    return eng


def dev_run(pkg, torch, s, par, delay):
    """density -> hmax -> hydro_force in the dev form; delay: None (no column) or the column.  Returns the outputs and the density-stage fields"""
    eng = new_engine(pkg, s, par)
    a, keep = gpu_arrays(torch, s["pos"], s["mass"], s["typ"], s["h0"], s["vel"], s["ent"])
    eng.dev_bind_particles(keep["pos"], keep["mass"], s["box"], type=keep["type"])
    eng.dev_force_tree_rebuild_mask(pkg.engine.GASMASK)
    t = make_times(pkg, **TK)
    eng.dev_density(a, t, DoEgyDensity=PE)
    eng.dev_force_tree_calc_hmax()
    d = None if delay is None else torch.from_numpy(delay).cuda()
    eng.dev_set_delaytime(d)
    eng.dev_hydro_force(a, t)
    eng.synchronize()
    st = eng.sph_stats()
    eng.close()
    return {k: a[k].cpu().numpy() for k in OUT + STAGE}, st


def wind_par(windspeed, thresh, decouple=True):
    par = R.model("fixed", True)
    par["WindSpeed"], par["WindFreeTravelDensThresh"] = float(windspeed), float(thresh)
    if not decouple:
        par["WindModel"] &= ~R.WIND_DECOUPLE_SPH
    return par


def reference(pkg, orc, torch):
    """the device's density-stage fields (a run without a column), the oracle's hydro loop without D, and per target of the eight with it"""
    if "ref" in _cache:
        return _cache["ref"]
    s = scene(pkg)
    plain, st_plain = dev_run(pkg, torch, s, None, None)
    N, typ = s["N"], s["typ"]
    dp = O.DensityParams(1.0, 2.0, 2.0, 99999., 2, 0.006)
    hp = O.HydroParams(PE, 100.0, 0.75)
    O.sph_set_softening(orc, 2.8 * (s["box"] / 16) / 30.)
    to = O.sph_times(**TK)

    def oracle_hydro(types, active):
        A = O.SphArrays(s["pos"], s["mass"], type=typ.copy(), hsml=s["h0"], vel=s["vel"], entropy=s["ent"])   # (A.type is written below)
        tr = orc.tree(s["pos"], s["mass"], s["box"], type=typ, hsml=A.hsml, hydro_active=np.ones(N, np.uint8), mask=1, moments=False)
        O.sph_density(orc, tr, dp, A, to, active=active[:1], DoEgyDensity=PE)       # fills EntVarPred of all gas (density.c:296-301)
        for k in STAGE:
            getattr(A, k)[:] = plain[k]
        A.type[:] = types
        tr2 = orc.tree(s["pos"], s["mass"], s["box"], type=types, hsml=A.hsml, hydro_active=np.zeros(N, np.uint8), mask=1, moments=False)
        tr2.calc_moments()
        O.sph_hydro_force(orc, tr2, dp, hp, A, to, active=active)
        return A

    without = typ.copy()
    without[s["D"]] = 1
    outside = np.setdiff1d(s["gas"], s["D"]).astype(np.int32)
    A = oracle_hydro(without, outside)
    M = np.zeros(len(s["eight"]))
    for k, i in enumerate(s["eight"]):
        ty = without.copy()
        ty[i] = 0
        M[k] = oracle_hydro(ty, np.array([i], np.int32)).maxsignalvel[i]
    fac_mu = pow(TK["atime"], 3 * (GAMMA - 1) / 2) / TK["atime"]
    windspeed = float(np.median(M)) / (2 * TK["atime"] * fac_mu)
    thresh = 0.1 * float(np.median(plain["density"][s["gas"]]))
    _cache["ref"] = dict(plain=plain, st_plain=st_plain, A=A, outside=outside, M=M, par=wind_par(windspeed, thresh), fac_mu=fac_mu)
    return _cache["ref"]


def check(s, ref, got, label):
    A, outside, D = ref["A"], ref["outside"], s["D"]
    r = dict(acc=rel(got["hydroacc_out"][outside], A.hydroacc_out[outside]), dtent=rel(got["dtentropy_out"][outside], A.dtentropy_out[outside]),
             msv=rel(got["maxsignalvel"][outside], A.maxsignalvel[outside]))
    assert np.abs(A.dtentropy_out[outside]).max() > 0
    assert (got["hydroacc_out"][D] == 0).all() and (got["dtentropy_out"][D] == 0).all()
    par, at = ref["par"], TK["atime"]
    windspeed = par["WindSpeed"] * at
    windspeed *= ref["fac_mu"]
    e = s["eight"]
    hsml_c = np.cbrt(par["WindFreeTravelDensThresh"] / ref["plain"]["density"][e]) * at
    exp = hsml_c * np.maximum(2 * windspeed, ref["M"])
    assert (2 * windspeed > ref["M"]).any() and (2 * windspeed < ref["M"]).any()
    r["msv eight"] = float(np.abs(got["maxsignalvel"][e] / exp - 1).max())
    print("hydro decoupled %s: |D| = %d, relative differences: %s" % (label, len(D), ", ".join("%s %.3g" % kv for kv in r.items())))
    assert r["acc"] <= 1e-10 and r["dtent"] <= 1e-10 and r["msv"] <= 1e-12 and r["msv eight"] <= 1e-12, r
    # every member of D took the target rule: MaxSignalVel is hsml_c times something >= 2 windspeed
    hc = np.cbrt(par["WindFreeTravelDensThresh"] / ref["plain"]["density"][D]) * at
    assert (got["maxsignalvel"][D] >= hc * 2 * windspeed * (1 - 1e-12)).all()


def test_decoupled_sources_and_targets_dev_form(pkg, orc):
    import torch
    s = scene(pkg)
    ref = reference(pkg, orc, torch)
    got, st = dev_run(pkg, torch, s, ref["par"], s["delay"])
    # what D would have contributed is visible: the outputs of their neighbours differ from the run without a column
    assert rel(got["hydroacc_out"][ref["outside"]], ref["plain"]["hydroacc_out"][ref["outside"]]) > 1e-6
    assert st["interactions"] < ref["st_plain"]["interactions"]
    check(s, ref, got, "dev form")
    _cache["dev"] = got


def test_without_the_bit_or_with_zero_delaytime_nothing_changes(pkg, orc):
    """no WIND_DECOUPLE_SPH in the model: the column is ignored, the outputs are those of a call without one, bit for bit (the same kernel);
    the bit and a column of zeros: the same to the tolerances of the loop, and whether bit for bit is printed"""
    import torch
    s = scene(pkg)
    ref = reference(pkg, orc, torch)
    plain = ref["plain"]
    nobit, _ = dev_run(pkg, torch, s, wind_par(ref["par"]["WindSpeed"], ref["par"]["WindFreeTravelDensThresh"], decouple=False), s["delay"])
    for k in OUT:
        assert np.array_equal(nobit[k], plain[k]), k
    zero, st = dev_run(pkg, torch, s, ref["par"], np.zeros(s["N"]))
    g = s["gas"]
    same = all(np.array_equal(zero[k], plain[k]) for k in OUT)
    print("hydro decoupled, all DelayTime zero against no column: bit-identical %s; relative differences %s"
          % (same, ", ".join("%s %.3g" % (k, rel(zero[k][g], plain[k][g])) for k in OUT)))
    assert st == ref["st_plain"]
    assert rel(zero["hydroacc_out"][g], plain["hydroacc_out"][g]) <= 1e-10 and rel(zero["dtentropy_out"][g], plain["dtentropy_out"][g]) <= 1e-10
    assert rel(zero["maxsignalvel"][g], plain["maxsignalvel"][g]) <= 1e-12


@pytest.mark.parametrize("form", ["host", "resident"])
def test_host_setters_give_the_dev_forms_result(pkg, orc, form):
    """mpg_set_delaytime with the staged mpg_hydro_force, and mpg_resident_sph_set_delaytime on a resident gas run"""
    import torch
    s = scene(pkg)
    ref = reference(pkg, orc, torch)
    if "dev" not in _cache:
        _cache["dev"], _ = dev_run(pkg, torch, s, ref["par"], s["delay"])
    dev = _cache["dev"]
    N, box = s["N"], s["box"]
    z = lambda *sh: np.zeros(sh)
    P = pkg.make_particles(s["pos"], s["mass"], type=s["typ"])
    P["Vel"] = s["vel"]
    a = dict(hsml=s["h0"].copy(), dthsml=z(N), vel=s["vel"].copy(), gacc=z(N, 3), gpm=z(N, 3), entropy=s["ent"].copy(), density=z(N), egywtdensity=z(N),
             dhsmlegyfac=z(N), divvel=z(N), curlvel=z(N), hydroacc_out=z(N, 3), dtentropy_out=z(N), maxsignalvel=z(N),
             tb_grav=np.zeros(N, np.uint8), tb_hydro=np.zeros(N, np.uint8))
    eng = new_engine(pkg, s, ref["par"])
    t = make_times(pkg, **TK)
    if form == "resident":
        eng.resident_begin(P, box)
        eng.resident_sph_begin(P, a)
        eng.density(P, box, a, t, DoEgyDensity=PE)
        eng.resident_sph_set_delaytime(s["delay"])
        eng.hydro_force(P, a, t)
        eng.resident_sph_end(a)
        eng.resident_end(P)
    else:
        eng.density(P, box, a, t, DoEgyDensity=PE)
        eng.set_delaytime(s["delay"])
        eng.hydro_force(P, a, t)
    eng.close()
    g = s["gas"]
    assert rel(a["hydroacc_out"][g], dev["hydroacc_out"][g]) <= 1e-10 and rel(a["dtentropy_out"][g], dev["dtentropy_out"][g]) <= 1e-10
    assert rel(a["maxsignalvel"][g], dev["maxsignalvel"][g]) <= 1e-12
    check(s, ref, a, form + " form")


def test_host_column_does_not_disturb_the_resident_one(pkg, orc):
    """both setters in use on a resident gas run: a call with the host column of mpg_set_delaytime (all zeros: nothing decoupled) uses
    that column, and the column of mpg_resident_sph_set_delaytime is in effect again, unchanged, once the host column is unbound"""
    import torch
    s = scene(pkg)
    ref = reference(pkg, orc, torch)
    N, box = s["N"], s["box"]
    z = lambda *sh: np.zeros(sh)
    P = pkg.make_particles(s["pos"], s["mass"], type=s["typ"])
    P["Vel"] = s["vel"]
    a = dict(hsml=s["h0"].copy(), dthsml=z(N), vel=s["vel"].copy(), gacc=z(N, 3), gpm=z(N, 3), entropy=s["ent"].copy(), density=z(N), egywtdensity=z(N),
             dhsmlegyfac=z(N), divvel=z(N), curlvel=z(N), hydroacc_out=z(N, 3), dtentropy_out=z(N), maxsignalvel=z(N),
             tb_grav=np.zeros(N, np.uint8), tb_hydro=np.zeros(N, np.uint8))
    eng = new_engine(pkg, s, ref["par"])
    t = make_times(pkg, **TK)
    eng.resident_begin(P, box)
    eng.resident_sph_begin(P, a)
    eng.density(P, box, a, t, DoEgyDensity=PE)
    eng.resident_sph_set_delaytime(s["delay"])
    eng.set_delaytime(np.zeros(N))
    eng.hydro_force(P, a, t)
    eng.synchronize()
    ptr = eng.resident_sph_arrays()
    first = {"hydroacc_out": device_view(torch, ptr["hydroacc_out"], 3 * N).cpu().numpy().reshape(N, 3),
             "maxsignalvel": device_view(torch, ptr["maxsignalvel"], N).cpu().numpy()}
    eng.set_delaytime(None)
    eng.hydro_force(P, a, t)
    eng.resident_sph_end(a)
    eng.resident_end(P)
    eng.close()
    g, plain = s["gas"], ref["plain"]
    assert rel(first["hydroacc_out"][g], plain["hydroacc_out"][g]) <= 1e-10 and rel(first["maxsignalvel"][g], plain["maxsignalvel"][g]) <= 1e-12
    check(s, ref, a, "resident column after a call with a host column")
