"""GPU tests of the stellar mass and metal return (metal_return, csrc/metals.hip) against the all-pairs numpy restatement
(tests/metals_restated.py: the radius loop with the reference's literal shrinking search radius; the return walk in the defined fp64 form
(b) and in the reference's literal float form (a)): the three entry points mpg_dev_metal_return / mpg_metal_return /
mpg_resident_sph_metal_return, the latter in the call order of run.c (density -> hydro_force -> metal_return inside a resident stretch).

Scenes: 16^3 gas of ics.hydro_pair with 150 stars, and the clustered 4096-gas set of ics.s_clust(16) with 100 stars; in both the stars'
entry Hsml is the mean-density guess times 0.05 (growth), 1 (bisection) or 20 (left == 0, more gas inside the first search radius than one
leaf list holds), one star sits in a corner of the box, a tenth of the stars lie below the 1e-3 work threshold, rows are garbage or
swallowed, black holes sit among the gas, and a few gas particles are so close to MaxGasMass that sizeable contributions to them are refused.

Conditions, asserted from the restatement alone before anything is compared (the seeds are chosen so that they hold with no target left
out): no gas particle within 1e-10 relative of a trial radius used or of a final Hsml; no Ngb that decides a branch within 1e-9 relative of
its threshold; no target ends through the tight bracket; every (star, gas) pair is either refused at the entry mass or fits with all other
contributions added, by 1e-9 - so the reference's thread order cannot matter.

What is compared, per call
  integers    iterations, maxcmpte and close per target, queue lengths, refused contributions: EQUAL.
  Hsml        1e-12 relative (the device pow is not correctly rounded).
  sums        starvolume and massreturned within 4 (n + 8) eps sum|term|; Density, Metallicity, Metals within 4 (k + 8) eps of their sums of
              absolute terms, k the accepted contributions; gas Mass within 1 float ulp of (b).
  against (a) within (k + 2) 2^-23 relative to the largest value on the path: the reference's own float rounding.
  The radius loop (integers, Hsml, starvolume) is held against the restated loop.  The return walk - massreturned and the gas columns - is
  held against (b) twice.  At the restated loop's own Hsml and StarVolumeSPH the bound of a few eps on the SUM is widened by what the
  allowed difference of the radius moves every TERM by, delta * sum |term| (|d ln wk / d ln Hsml| + 1) with delta the observed relative
  difference of Hsml plus that of StarVolumeSPH (2e-14 + 2e-14; the radius differs through ngb_narrow_down's differences of nearly equal
  sums): without that term the bound is 4 (k + 8) eps = 8e-15 for a gas particle whose metal content comes from one contribution, below the
  2e-14 its one term moves by, and the ratio is 1.5 (Metallicity) and 2.3 (Metals).  At the Hsml and StarVolumeSPH the device loop ended
  with, (b) and (a) are held with the bounds of a few eps alone.  The accepted and refused pairs are asserted to be the same at either radius.
  untouched rows bit-identical.
The largest observed ratio to each bound is printed (pytest -s); DESIGN 3.10 records them.

Largest ratios of a run on an MI355X: radius / Hsml 0.023, starvolume 0.17, massreturned 0.013, Mass 0 ulp, Density 0.045, Metallicity 0.072,
Metals 0.068; against (a): Mass 0.33, Metals 0.35, Density and Metallicity 1.4e-9; at the restated Hsml, with the added term: Density 0.036,
Metallicity 0.079, Metals 0.14, massreturned 0.0065."""
import numpy as np
import pytest

import metals_restated as R

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps
KT, ETA, MAXDEV = 2, 1.0, 2.0
GAS_COLS = ("density", "metallicity", "metals")
STAR_COLS = ("hsml", "totalmassreturned", "lastenrichment")
_cache = {}


# ---- inputs and their restatement, computed once per scene --------------------------------------------------------------------------------
def scene(pkg, name):
    if name in _cache:
        return _cache[name]
    if name == "zel":
        pos, _, typ, box = pkg.ics.hydro_pair(16)
        d = R.sample_scene(pos[typ == 0], box, 150, seed=5, ktype=KT, eta=ETA)
        sphw, active = 1, None
    else:
        pg, _, box = pkg.ics.s_clust(16, seed=3)
        d = R.sample_scene(pg, box, 100, seed=8, ktype=KT, eta=ETA)
        # an active sublist: every gas / black-hole row, three quarters of the stars
        s = np.arange(d["s0"], d["n"])
        sphw, active = 0, np.concatenate([np.arange(0, d["s0"]), s[s % 4 != 1]]).astype(np.int32)
    out, res, info = R.metal_return(d, d["box"], KT, ETA, MAXDEV, sphw, d["maxgasmass"], active=active)
    _cache[name] = (d, sphw, active, out, res, info)
    return _cache[name]


def conditions(res, info):
    assert res["min_gap"] > 1e-10 and info["min_gap"] > 1e-10, (res["min_gap"], info["min_gap"])
    assert res["min_margin"] > 1e-9, res["min_margin"]
    assert not any(res["tight"].values())
    assert info["cap_margin"] > 1e-9, info["cap_margin"]


def compare(d, sphw, out, res, info, got, exp, stats, label):
    """got: dict of the arrays after the call (numpy, particle order) plus massreturned / starvolume.  The radius loop is held against the
    restated loop; the return walk is then held against forms (b) and (a) EVALUATED AT the Hsml and StarVolumeSPH the device loop ended
    with: a bound of a few eps on a sum of k terms cannot cover terms that themselves move with the 1e-12 the radius is allowed (the
    restated loop's own Hsml and volume give the same accepted and refused pairs, which is asserted)."""
    conditions(res, info)
    tl = res["targets"]
    t = np.array(tl, np.int64)
    assert set(np.nonzero(exp["iterations"] >= 0)[0].tolist()) == set(tl)
    assert exp["queue_lengths"] == res["queue_lengths"]
    assert stats["iterations"] == len(res["queue_lengths"]) and stats["targets"] == sum(res["queue_lengths"])
    assert stats["tight"] == 0 and stats["refused"] == info["refused"]
    assert stats["candidates"] >= stats["neighbours"] > 0
    for key in ("iterations", "maxcmpte", "close"):
        assert np.array_equal(exp[key][t], [res[key][i] for i in tl]), key
    worst = {}
    worst["radius"] = np.abs(exp["radius"][t] / np.array([res["radius"][i] for i in tl]) - 1).max() / 1e-12
    worst["hsml"] = np.abs(got["hsml"][t] / out["hsml"][t] - 1).max() / 1e-12
    w = 0.0
    for i in tl:
        b = 4 * (res["vol_n"][i] + 8) * EPS * res["vol_abs"][i]
        w = max(w, abs(got["starvolume"][i] - res["volume"][i]) / b)
    worst["starvolume"] = w
    assert worst["radius"] <= 1 and worst["hsml"] <= 1 and worst["starvolume"] <= 1, (label, worst)
    # the return walk against (b) at the RESTATED loop's Hsml and StarVolumeSPH, as the issue words it: 4 (k + 8) eps of the sums of absolute
    # terms, plus what the allowed difference of the radius and the volume moves the terms by to first order, delta * sum |term| (|d ln wk /
    # d ln Hsml| + 1) from the restatement's own kernel, delta = max |dHsml / Hsml| + max |dStarVolumeSPH / StarVolumeSPH| over the targets;
    # the factor 2 covers the second order and the centred difference the lever is taken with
    delta = np.abs(got["hsml"][t] / out["hsml"][t] - 1).max() + max(abs(got["starvolume"][i] / res["volume"][i] - 1) for i in tl)
    g0, k0, tch0, Mn0 = info["gas"], info["k"], info["touched"], info["Mnew"]
    kb0 = 4 * (k0 + 8) * EPS
    M0 = d["mass"][g0].astype(np.float64)
    rat = lambda err, bound: (err / bound)[tch0].max()
    worst["restated-Hsml density"] = rat(np.abs(got["density"][g0] - out["density"][g0]),
                                         kb0 * out["density"][g0] + 2 * delta * d["density"][g0] * info["sens_M"] / M0)
    worst["restated-Hsml metallicity"] = rat(np.abs(got["metallicity"][g0] - out["metallicity"][g0]),
                                             (kb0 * info["abs_Z"] + 2 * delta * (info["sens_Z"] + out["metallicity"][g0] * info["sens_M"])) / Mn0)
    worst["restated-Hsml metals"] = rat(np.abs(got["metals"][g0] - out["metals"][g0]),
                                        (kb0[:, None] * info["abs_S"] + 2 * delta * (info["sens_S"] + out["metals"][g0] * info["sens_M"][:, None])) / Mn0[:, None])
    worst["restated-Hsml massreturned"] = max(abs(got["massreturned"][i] - info["massreturn"][i])
                                              / (4 * (info["nacc"][i] + 8) * EPS * info["massreturn"][i] + 2 * delta * info["sens_star"][i] + 1e-300) for i in tl)
    # ... and, with bounds of a few eps alone, at the device loop's own Hsml and StarVolumeSPH
    k_restated, refused_restated = info["k"], info["refused"]
    vol_dev = {i: float(got["starvolume"][i]) for i in tl}
    out, info = R.return_defined(d, tl, got["hsml"], vol_dev, d["box"], KT, sphw, d["maxgasmass"])
    lit = R.return_literal(d, tl, got["hsml"], vol_dev, d["box"], KT, sphw, d["maxgasmass"])
    out["hsml"] = got["hsml"]
    assert info["min_gap"] > 1e-10 and info["cap_margin"] > 1e-9
    assert np.array_equal(info["k"], k_restated) and info["refused"] == refused_restated == lit["refused"]
    gas, k = info["gas"], info["k"]
    w = 0.0
    for i in tl:
        b = 4 * (info["nacc"][i] + 8) * EPS * info["massreturn"][i]
        if b > 0:
            w = max(w, abs(got["massreturned"][i] - info["massreturn"][i]) / b)
        else:
            assert got["massreturned"][i] == 0
    worst["massreturned"] = w
    # gas against (b)
    Mb = out["mass"][gas]
    ulp = np.spacing(Mb)
    worst["mass ulp"] = (np.abs(got["mass"][gas].astype(np.float64) - Mb.astype(np.float64)) / ulp).max()
    tch = info["touched"]
    kb = 4 * (k + 8) * EPS
    worst["density"] = (np.abs(got["density"][gas] - out["density"][gas]) / (kb * out["density"][gas]))[tch].max()
    worst["metallicity"] = (np.abs(got["metallicity"][gas] - out["metallicity"][gas]) / (kb * info["abs_Z"] / info["Mnew"]))[tch].max()
    worst["metals"] = (np.abs(got["metals"][gas] - out["metals"][gas]) / (kb[:, None] * info["abs_S"] / info["Mnew"][:, None]))[tch].max()
    # the stars' own columns: Mass -= MassReturn in float, TotalMassReturned += MassReturn, LastEnrichmentMyr = StellarAge
    assert (np.abs(got["mass"][t].astype(np.float64) - out["mass"][t]) <= np.spacing(out["mass"][t])).all()
    assert np.allclose(got["totalmassreturned"][t], out["totalmassreturned"][t], rtol=1e-12, atol=0)
    assert np.array_equal(got["lastenrichment"][t], d["stellarage"][t])
    # against (a): the reference's own float rounding
    fb = (k + 2) * 2.0 ** -23
    la = lambda key: lit[key][gas].astype(np.float64)
    worst["(a) mass"] = (np.abs(got["mass"][gas].astype(np.float64) - la("mass")) / (fb * la("mass"))).max()
    worst["(a) density"] = (np.abs(got["density"][gas] - la("density")) / (fb * la("density"))).max()
    zmax = np.maximum(d["metallicity"][gas], out["metallicity"][gas])
    worst["(a) metallicity"] = (np.abs(got["metallicity"][gas] - la("metallicity")) / (fb * zmax)).max()
    smax = np.maximum(d["metals"][gas], out["metals"][gas])
    worst["(a) metals"] = (np.abs(got["metals"][gas] - la("metals")) / (fb[:, None] * smax)).max()
    print("metals %s: %d targets, iterations %s, refused %d, largest ratio to the bound: %s; min gap %.2e, min margin %.2e, cap margin %.2e"
          % (label, len(tl), res["queue_lengths"], info["refused"], ", ".join("%s %.3g" % kv for kv in worst.items()), min(res["min_gap"], info["min_gap"]),
             res["min_margin"], info["cap_margin"]))
    for key, v in worst.items():
        assert v <= 1, (label, key, v)
    # untouched rows are bit-identical
    same = np.ones(d["n"], bool)
    same[t] = False
    same[gas[tch]] = False
    for key in ("mass",) + GAS_COLS + STAR_COLS:
        assert np.array_equal(got[key][same], d[key][same]), key
    return worst


def dev_arrays(torch, d, sentinel=-3.0):
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    a = {key: up(d[key]) for key in ("massgenerated", "metalgenerated", "speciesgenerated", "stellarage", "mass", "hsml", "totalmassreturned",
                                     "lastenrichment", "density", "metallicity", "metals")}
    a["massreturned"] = torch.full((d["n"],), sentinel, dtype=torch.float64, device="cuda")
    a["starvolume"] = torch.full((d["n"],), sentinel, dtype=torch.float64, device="cuda")
    keep = dict(pos=up(d["pos"]), type=up(d["type"]))
    return a, keep


def down(a):
    return {key: v.cpu().numpy() for key, v in a.items()}


def new_engine(pkg, d, sphw):
    eng = pkg.Engine(0)
    eng.set_densitypar(ETA, 2.0, 2.0, 99999., pkg.engine.DENSITY_KERNEL_QUINTIC_SPLINE, 0.006)
    eng.set_metal_params(sphw, MAXDEV, d["maxgasmass"])
    return eng


def host_table(pkg, d):
    """struct particle_data with the types as the table holds them and IsGarbage / Swallowed in the flags byte"""
    P = pkg.make_particles(d["pos"], d["mass"], type=d["type_table"])
    P["Flags"][d["dead"]] = 1
    P["Flags"][d["dead"][-1]] = 2      # a swallowed star
    return P


def host_arrays(d):
    a = {key: d[key].copy() for key in ("massgenerated", "metalgenerated", "speciesgenerated", "stellarage", "hsml", "totalmassreturned",
                                        "lastenrichment", "density", "metallicity", "metals")}
    a["massreturned"] = np.full(d["n"], -3.0)
    a["starvolume"] = np.full(d["n"], -3.0)
    return a


def run_dev(pkg, torch, d, sphw, active, mask):
    eng = new_engine(pkg, d, sphw)
    a, keep = dev_arrays(torch, d)
    eng.dev_bind_particles(keep["pos"], a["mass"], d["box"], type=keep["type"])
    eng.dev_force_tree_rebuild_mask(mask)
    eng.dev_metal_return(a, active=None if active is None else torch.from_numpy(active).cuda())
    eng.synchronize()
    got, exp, stats = down(a), eng.metals_export(d["n"]), eng.metals_stats()
    ntree = eng.tree_stats().NumParticles
    eng.close()
    return got, exp, stats, ntree


# ---- the scenes themselves -----------------------------------------------------------------------------------------------------------------
def test_scenes_reach_what_they_are_for(pkg):
    """from the restatement alone: the branches, the faces and the corner, pause and resume, shared neighbours, refusals, non-targets"""
    for name in ("zel", "clust"):
        d, sphw, active, out, res, info = scene(pkg, name)
        conditions(res, info)
        tl = res["targets"]
        stars = np.arange(d["s0"], d["n"])
        assert len(tl) > 0.6 * d["nstar"] and len(res["queue_lengths"]) >= 4
        grow = [i for i in tl if out["hsml"][i] > 4 * d["hsml"][i]]
        shrink = [i for i in tl if out["hsml"][i] < d["hsml"][i] / 4]
        assert len(grow) >= 5 and len(shrink) >= 3                       # entry Hsml x 0.05 and x 20
        assert max(res["first_count"].values()) > 120 * 8                # more gas than one leaf list can hold: pause and resume
        assert sorted(set(res["maxcmpte"].values()))[0] == 1 and max(res["maxcmpte"].values()) == R.NHSML
        h = np.array([out["hsml"][i] for i in tl])
        p = d["pos"][tl]
        face = ((p < h[:, None]) | (p > d["box"] - h[:, None]))
        assert face.any(1).sum() >= 3 and face.all(1).any()              # faces, and the star in the corner
        assert info["k"].max() >= 2 and info["refused"] > 0              # shared neighbours; pairs refused outright
        assert (info["k"][np.isin(info["gas"], d["heavy"])] == 0).any()
        low = [i for i in stars if d["type"][i] == 4 and d["massgenerated"][i] < 1e-3 * (d["mass"][i] + d["totalmassreturned"][i])]
        assert len(low) >= 3 and not set(low) & set(tl)
        assert (d["type"][stars] == 7).sum() >= 3
        if active is not None:
            assert len(set(stars.tolist()) - set(active.tolist())) > 10 and set(tl) <= set(active.tolist())


def test_dev_form_weighted_with_black_holes_in_the_tree(pkg):
    """mpg_dev_metal_return, NULL active list, SPHWeighting = 1, on a tree of gas AND black holes (the black holes are skipped)"""
    import torch
    d, sphw, active, out, res, info = scene(pkg, "zel")
    got, exp, stats, ntree = run_dev(pkg, torch, d, sphw, active, pkg.engine.GASMASK + pkg.engine.BHMASK)
    assert ntree == int((d["type"] == 0).sum() + (d["type"] == 5).sum()) > len(info["gas"])
    compare(d, sphw, out, res, info, got, exp, stats, "dev / zel / weighted")
    # the optional outputs are written for targets only
    nt = np.ones(d["n"], bool)
    nt[res["targets"]] = False
    assert (got["massreturned"][nt] == -3.0).all() and (got["starvolume"][nt] == -3.0).all()


def test_dev_form_unweighted_active_sublist(pkg):
    """SPHWeighting = 0 on the clustered set, an active sublist that leaves a quarter of the stars out, a gas-only tree"""
    import torch
    d, sphw, active, out, res, info = scene(pkg, "clust")
    got, exp, stats, ntree = run_dev(pkg, torch, d, sphw, active, pkg.engine.GASMASK)
    assert ntree == len(info["gas"])
    compare(d, sphw, out, res, info, got, exp, stats, "dev / clustered / unweighted / sublist")


def test_host_form_equals_the_dev_form(pkg):
    """mpg_metal_return on the 160-byte records (flags: IsGarbage, Swallowed): within the bounds, and bit for bit the dev form's in
    everything that is not an atomic sum"""
    import torch
    d, sphw, active, out, res, info = scene(pkg, "clust")
    P = host_table(pkg, d)
    a = host_arrays(d)
    eng = new_engine(pkg, d, sphw)
    eng.metal_return(P, d["box"], a, ActiveParticle=active)
    got = dict(a, mass=P["Mass"].copy())
    exp, stats = eng.metals_export(d["n"]), eng.metals_stats()
    assert eng.tree_stats().NumParticles == len(info["gas"])             # the gas tree, built by the call
    eng.close()
    assert a["massgenerated"].tobytes() == d["massgenerated"].tobytes()  # an input goes up and does not come back
    compare(d, sphw, out, res, info, got, exp, stats, "host / clustered")
    dev, exp_d, stats_d, _ = run_dev(pkg, torch, d, sphw, active, pkg.engine.GASMASK)
    for key in ("hsml", "starvolume", "lastenrichment", "massreturned", "totalmassreturned"):     # per-target sums in a fixed lane order
        assert np.array_equal(got[key], dev[key]), key
    t = np.array(res["targets"])
    assert np.array_equal(exp["iterations"], exp_d["iterations"])
    for key in ("radius", "maxcmpte", "close"):                      # (defined for the targets only)
        assert np.array_equal(exp[key][t], exp_d[key][t]), key
    assert stats == stats_d


def sph_times(pkg):
    T = pkg.SphTimes()
    T.atime, T.hubble = 0.5, 0.3
    for b in range(47):
        T.dloga_bin[b] = 0.01
    return T


def test_resident_form_in_the_order_of_run_c(pkg):
    """a resident gas stretch: density -> hydro_force -> metal_return (Mass, Hsml and Density are resident columns, the metal columns and
    the per-star inputs travel), then density and hydro_force again.  The entry state of the call is what the same stretch WITHOUT the call
    holds after hydro_force (the loops are deterministic)."""
    pg, _, box = pkg.ics.s_clust(16, seed=3)
    d = R.sample_scene(pg, box, 100, seed=8, ktype=KT, eta=ETA, nheavy=0)
    n = d["n"]
    T = sph_times(pkg)
    rng = np.random.RandomState(2)
    vel = rng.standard_normal((n, 3))
    stars = np.arange(d["s0"], n)
    act = np.concatenate([np.arange(0, d["s0"]), stars[stars % 4 != 1]]).astype(np.int32)
    runs = []
    for with_call in (False, True):
        P = host_table(pkg, d)
        P["Vel"] = vel
        eng = new_engine(pkg, d, 1)
        eng.set_gravshort_treepar()
        eng.gravshort_set_softenings(box / 20)
        eng.set_hydropar(0, 100.0, 0.75)
        z = lambda *s: np.zeros(s)
        a = dict(hsml=z(n), dthsml=z(n), vel=vel.copy(), gacc=z(n, 3), gpm=z(n, 3), entropy=np.ones(n), density=z(n), egywtdensity=z(n), dhsmlegyfac=z(n),
                 divvel=z(n), curlvel=z(n), hydroacc_out=z(n, 3), dtentropy_out=z(n), maxsignalvel=z(n))
        eng.set_init_hsml(P, box, a, box / 16)
        a["hsml"][stars] = d["hsml"][stars]
        a["hsml"][stars[8]] = 0.0                                        # the resident column holds a zero: the caller's value must arrive
        eng.resident_begin(P, box)
        eng.resident_sph_begin(P, a)
        eng.density(P, box, a, T)
        eng.hydro_force(P, a, T)
        m = host_arrays(d)
        if with_call:
            eng.resident_sph_metal_return(P, m, ActiveParticle=act)
            exp, stats = eng.metals_export(n), eng.metals_stats()
            mass_after = P["Mass"].copy()                                # written into the records by the call
        eng.resident_sph_end(a)                                          # Hsml and Density as the call left them
        state = dict(hsml=a["hsml"].copy(), density=a["density"].copy())
        if with_call:                                                    # the stretch goes on, on the new masses
            eng.resident_sph_begin(P, a)
            eng.density(P, box, a, T)
            eng.hydro_force(P, a, T)
            eng.resident_sph_end(a)
            assert np.isfinite(a["density"]).all() and np.isfinite(a["hydroacc_out"]).all()
        eng.resident_end(P)
        eng.close()
        runs.append((state, m))
    entry = dict(d, hsml=runs[0][0]["hsml"].copy(), density=runs[0][0]["density"])
    entry["hsml"][stars] = d["hsml"][stars]                              # the stars' Hsml is the caller's (host_arrays), not the column's zero
    out, res, info = R.metal_return(entry, box, KT, ETA, MAXDEV, 1, d["maxgasmass"], active=act)
    assert len(res["targets"]) > 50 and int(stars[8]) in res["targets"]
    got = dict(runs[1][1], mass=mass_after, hsml=runs[1][0]["hsml"], density=runs[1][0]["density"])
    assert np.array_equal(runs[1][1]["hsml"], runs[1][0]["hsml"])        # the resident column came back through A->hsml
    compare(entry, 1, out, res, info, got, exp, stats, "resident / clustered / sublist")
    # ... and the dev form on the same entry state and the same tree: bit for bit in everything that is not an atomic sum
    import torch
    dev, exp_d, stats_d, ntree = run_dev(pkg, torch, entry, 1, act, pkg.engine.GASMASK)
    assert ntree == len(info["gas"])
    t = np.array(res["targets"])
    for key in ("hsml", "starvolume", "lastenrichment", "massreturned", "totalmassreturned"):
        assert np.array_equal(got[key][t], dev[key][t]), key
    assert np.array_equal(got["mass"][t], dev["mass"][t])                # the stars' masses: Mass - MassReturn
    assert np.array_equal(exp["iterations"], exp_d["iterations"]) and exp["queue_lengths"] == exp_d["queue_lengths"]
    for key in ("radius", "maxcmpte", "close"):
        assert np.array_equal(exp[key][t], exp_d[key][t]), key
    assert stats == stats_d
    gas = info["gas"]
    assert (np.abs(got["mass"][gas].astype(np.float64) - dev["mass"][gas]) <= np.spacing(dev["mass"][gas])).all()
    for key in GAS_COLS:                                                 # atomic sums: within the bounds of compare() of each other, twice
        assert np.allclose(got[key][gas], dev[key][gas], rtol=8 * (info["k"].max() + 8) * EPS, atol=0), key


def test_no_target(pkg):
    """a call without a target: nothing is written and no tree is demanded; the statistics are zero"""
    import torch
    d, sphw, active, *_ = scene(pkg, "clust")
    none = dict(d, massgenerated=np.where(d["type"] == 4, 1e-5, d["massgenerated"]))
    assert R.metal_return(none, d["box"], KT, ETA, MAXDEV, 1, d["maxgasmass"])[0] is None
    eng = new_engine(pkg, d, 1)
    a, keep = dev_arrays(torch, none)
    eng.dev_bind_particles(keep["pos"], a["mass"], d["box"], type=keep["type"])
    eng.dev_metal_return(a)                                              # no tree yet: none demanded
    with pytest.raises(pkg.EngineError, match="no tree"):
        eng.tree_stats()
    eng.synchronize()
    got = down(a)
    for key in ("mass",) + GAS_COLS + STAR_COLS:
        assert np.array_equal(got[key], none[key]), key
    assert (got["massreturned"] == -3.0).all()
    st = eng.metals_stats()
    assert st["iterations"] == 0 and st["targets"] == 0 and st["candidates"] == 0 and st["refused"] == 0
    assert (eng.metals_export(d["n"])["iterations"] == -1).all()
    # ... and an empty active list with returning stars in the table
    a, keep = dev_arrays(torch, d)
    eng.dev_bind_particles(keep["pos"], a["mass"], d["box"], type=keep["type"])
    eng.dev_metal_return(a, active=torch.from_numpy(np.arange(0, d["s0"], dtype=np.int32)).cuda())
    assert eng.metals_stats()["targets"] == 0
    eng.close()


def test_density_and_hydro_after_a_call_equal_a_fresh_engine_on_the_new_masses(pkg):
    """mpg_dev_density + mpg_dev_hydro_force after a call and a tree rebuild equal the same calls on a fresh engine that is given the
    updated masses and arrays, bit for bit: the call leaves nothing behind in the engine"""
    import torch
    d, *_ = scene(pkg, "zel")
    n, box = d["n"], d["box"]
    T = sph_times(pkg)
    rng = np.random.RandomState(7)
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()
    z = lambda *s: torch.zeros(*s, dtype=torch.float64, device="cuda")
    OUT = ("hsml", "dthsml", "density", "dhsmlegyfac", "divvel", "curlvel", "hydroacc_out", "dtentropy_out", "maxsignalvel")

    def loops(eng, a):
        eng.dev_force_tree_rebuild_mask(pkg.engine.GASMASK)
        eng.dev_density(a, T)
        eng.dev_force_tree_calc_hmax()
        eng.dev_hydro_force(a, T)

    def engine():
        eng = new_engine(pkg, d, 1)
        eng.set_gravshort_treepar()
        eng.gravshort_set_softenings(box / 16)
        eng.set_hydropar(0, 100.0, 0.75)
        return eng

    eng = engine()
    pos, typ, mass = up(d["pos"]), up(d["type"]), up(d["mass"])
    a = dict(hsml=z(n), dthsml=z(n), vel=up(rng.standard_normal((n, 3))), entropy=torch.ones(n, dtype=torch.float64, device="cuda"), density=z(n),
             egywtdensity=z(n), dhsmlegyfac=z(n), divvel=z(n), curlvel=z(n), hydroacc_out=z(n, 3), dtentropy_out=z(n), maxsignalvel=z(n))
    eng.dev_bind_particles(pos, mass, box, type=typ)
    eng.dev_force_tree_rebuild_mask(pkg.engine.GASMASK + pkg.engine.BHMASK, with_moments=True)
    eng.dev_set_init_hsml(a, box / 16)
    eng.synchronize()                       # (torch works on another stream than the engine)
    a["hsml"][d["s0"]:] = up(d["hsml"][d["s0"]:])
    torch.cuda.synchronize()
    loops(eng, a)
    m, _ = dev_arrays(torch, d)
    m.update(mass=mass, hsml=a["hsml"], density=a["density"])
    eng.dev_metal_return(m)
    eng.synchronize()
    assert eng.metals_stats()["targets"] > 100 and not torch.equal(mass, up(d["mass"]))
    fresh = {key: v.clone() for key, v in a.items()}
    mass2 = mass.clone()
    torch.cuda.synchronize()
    loops(eng, a)
    eng.synchronize()
    first = {key: a[key].cpu().numpy().copy() for key in OUT}
    eng.close()
    eng = engine()
    eng.dev_bind_particles(pos, mass2, box, type=typ)
    loops(eng, fresh)
    eng.synchronize()
    for key in OUT:
        assert np.array_equal(first[key], fresh[key].cpu().numpy()), key
    eng.close()


def test_errors(pkg):
    """Hsml <= 0 of a target, no gas tree, no parameters and missing arrays are error returns with a message; the engine goes on working"""
    import torch
    d, sphw, active, out, res, info = scene(pkg, "clust")
    eng = pkg.Engine(0)
    eng.set_densitypar(ETA, 2.0, 2.0, 99999., pkg.engine.DENSITY_KERNEL_QUINTIC_SPLINE, 0.006)
    a, keep = dev_arrays(torch, d)
    eng.dev_bind_particles(keep["pos"], a["mass"], d["box"], type=keep["type"])
    with pytest.raises(pkg.EngineError, match="mpg_set_metal_params"):
        eng.dev_metal_return(a)
    eng.set_metal_params(sphw, MAXDEV, d["maxgasmass"])
    with pytest.raises(pkg.EngineError, match="does not contain the gas"):
        eng.dev_metal_return(a)                                          # no tree at all
    eng.dev_force_tree_rebuild_mask(2)                                   # DMMASK
    with pytest.raises(pkg.EngineError, match="does not contain the gas"):
        eng.dev_metal_return(a)
    eng.dev_force_tree_rebuild_mask(pkg.engine.GASMASK)
    for missing in ("massgenerated", "speciesgenerated", "mass", "hsml", "density", "metals"):
        b = dict(a)
        b[missing] = None
        with pytest.raises(pkg.EngineError, match="required"):
            eng.dev_metal_return(b)
    bad = dict(a, hsml=a["hsml"].clone())
    bad["hsml"][res["targets"][3]] = 0.0
    torch.cuda.synchronize()
    with pytest.raises(R.MetalError):
        h = d["hsml"].copy()
        h[res["targets"][3]] = 0.0
        R.stellar_density(d["pos"], d["type"], d["mass"], d["density"], h, res["targets"], d["box"], KT, ETA, MAXDEV, sphw)
    with pytest.raises(pkg.EngineError, match="Hsml <= 0"):
        eng.dev_metal_return(bad)
    eng.synchronize()
    assert np.array_equal(a["mass"].cpu().numpy(), d["mass"]) and np.array_equal(a["density"].cpu().numpy(), d["density"])   # nothing was written
    # the host form names the array that is missing
    P = host_table(pkg, d)
    h = host_arrays(d)
    h["metals"] = None
    with pytest.raises(pkg.EngineError, match="metals is required"):
        eng.metal_return(P, d["box"], h)
    # ... and a good call afterwards
    eng.dev_bind_particles(keep["pos"], a["mass"], d["box"], type=keep["type"])
    eng.dev_force_tree_rebuild_mask(pkg.engine.GASMASK)
    eng.dev_metal_return(a, active=torch.from_numpy(active).cuda())
    eng.synchronize()
    compare(d, sphw, out, res, info, down(a), eng.metals_export(d["n"]), eng.metals_stats(), "dev / after errors")
    eng.close()
