"""GPU tests of the wind model (csrc/winds.hip) against the all-pairs numpy restatement (tests/winds_restated.py, form (b): per gas particle
the minimum over (r, StarID)): mpg_dev_winds_and_feedback and the host form mpg_winds_and_feedback on two scenes and four models, the calls
with nothing to do, the error returns, mpg_dev_winds_subgrid and mpg_dev_winds_evolve.

Scenes (winds_restated.wind_scene): 16^3 gas of ics.hydro_pair(16) with 150 stars and the clustered 4096-gas set ics.s_clust(16) with 100.
Star Hsml is the mean-density guess times 0.05 (TotalWeight == 0), 1 or 20 (pause and resume of the leaf list); one star in a corner of the
box; Vdisp <= 0 and Vdisp below the MinWindVelocity floor; a tenth of the gas with DelayTime > 0; garbage rows, black holes in the tree, rows
of the tree that became stars or were swallowed after the build; IDs above 2^63; one gas particle at dyadic coordinates between two mirrored
stars (r2 exactly equal, both pairs potential kicks).  Models: USE_HALO and FIXED_EFFICIENCY, each with MaxWindFreeTravelTime > 0 and 0.

Conditions (winds_restated.conditions, proven on the CPU by test_winds_restated.py and asserted here again before anything is compared): no
gas within 1e-10 relative of a star's Hsml, |table value - p| > 1e-9 for every pair tested, no two potential kicks of a gas particle within
1e-10 relative in r unless exactly equal, >= 100 kicks applied, >= 20 gas particles with candidates from several stars, for >= 5 of them the
winner is not the first in list order.

Compared, per scene, model and form
  integers    the set of potential kicks as (star, gas) pairs, kick_star of every row, the eligible-neighbour count, the stats: EQUAL
              (maxvel, one product or a parameter times atime, as well).
  TotalWeight within 4 (k + 8) eps of its sum of k positive terms; exactly 0 without a term.
  Vel         within TRANS_DIR v + 2 eps |Vel| per component;  Entropy within (TRANS + 4 eps) (Entropy + therm / enttou);  DelayTime within
              4 eps relative.  TRANS_DIR = 1e-12 and TRANS = 1e-14 as in test_gpu_blackhole.py (the direction formula, the device pow).
  other rows  bit-identical, those with DelayTime > 0 included.
The largest observed ratio to each bound is printed (pytest -s); DESIGN 3.13 records them."""
import numpy as np
import pytest

import winds_restated as R

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps
TRANS, TRANS_DIR = 1e-14, 1e-12
COLS = ("vel", "entropy", "delaytime")
SENT = -3.0


def up(torch, a):
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint64:
        a = a.view(np.int64)          # torch has no uint64: the same bits
    return torch.from_numpy(a).cuda()


def dev_arrays(torch, d):
    a = {k: up(torch, d[k]) for k in ("id", "hsml", "vdisp", "density", "vel", "entropy", "delaytime")}
    a["totalweight"] = torch.full((d["n"],), SENT, dtype=torch.float64, device="cuda")
    a["kick_star"] = torch.full((d["n"],), -3, dtype=torch.int64, device="cuda")
    return a


def down(a):
    g = {k: v.cpu().numpy() for k, v in a.items()}
    g["kick_star"] = g["kick_star"].view(np.uint64)
    return g


def new_engine(pkg, d, par, table=True):
    eng = pkg.Engine(0)
    if par is not None:
        eng.set_wind_params(par)
    if table:
        eng.set_random_table(d["table"])
    return eng


def bound_engine(pkg, torch, d, par, mask, table=True):
    """an engine with the scene bound and the tree of `mask` built from the types as they were at the build; the type column then takes
    the current types (stars formed and gas swallowed since)"""
    eng = new_engine(pkg, d, par, table)
    keep = dict(pos=up(torch, d["pos"]), mass=up(torch, d["mass"]), type=up(torch, d["type_tree"]))
    eng.dev_bind_particles(keep["pos"], keep["mass"], d["box"], type=keep["type"])
    if mask:
        eng.dev_force_tree_rebuild_mask(mask)
        eng.synchronize()
    keep["type"].copy_(up(torch, d["type"]))
    torch.cuda.synchronize()
    return eng, keep


def has_no_tree(pkg, eng):
    with pytest.raises(pkg.EngineError, match="no tree"):
        eng.tree_stats()
    return True


def compare(d, par, out, info, got, stats, pairs, label):
    R.conditions(d, info)
    listed = d["newstars"]
    # integers
    assert pairs == info["pairs"], (label, len(pairs), len(info["pairs"]))
    assert np.array_equal(got["kick_star"], out["kick_star"]), label
    assert stats["stars"] == len(listed) and stats["neighbours"] == int(info["nterm"].sum()) and stats["candidates"] >= stats["neighbours"]
    assert stats["potential_kicks"] == len(info["kicks"]) and stats["applied"] == info["applied"]
    assert stats["discarded"] == len(info["kicks"]) - info["applied"] and stats["maxvel"] == info["maxvel"]
    worst = {}
    # TotalWeight
    w = 0.0
    for q, i in enumerate(listed):
        k, s = int(info["nterm"][q]), float(info["totalweight"][q])
        if k == 0:
            assert got["totalweight"][i] == 0.0
        else:
            w = max(w, abs(got["totalweight"][i] - s) / (4 * (k + 8) * EPS * s))
    worst["totalweight"] = w
    notlisted = np.ones(d["n"], bool)
    notlisted[listed] = False
    assert (got["totalweight"][notlisted] == SENT).all()
    # the kicked rows
    kicked = np.array(sorted(info["best"]), np.int64)
    v = np.array([info["best"][g][3] for g in kicked])
    dent = np.array([info["dent"][g] for g in kicked])
    worst["vel"] = (np.abs(got["vel"][kicked] - out["vel"][kicked]) / (TRANS_DIR * v[:, None] + 2 * EPS * np.abs(out["vel"][kicked]))).max()
    worst["entropy"] = (np.abs(got["entropy"][kicked] - out["entropy"][kicked]) / ((TRANS + 4 * EPS) * (d["entropy"][kicked] + dent))).max()
    if par["MaxWindFreeTravelTime"] > 0:
        worst["delaytime"] = (np.abs(got["delaytime"][kicked] / out["delaytime"][kicked] - 1) / (4 * EPS)).max()
    else:
        assert np.array_equal(got["delaytime"], d["delaytime"])
    # every other row bit-identical
    same = np.ones(d["n"], bool)
    same[kicked] = False
    for key in COLS:
        assert np.array_equal(got[key][same], d[key][same]), (label, key)
    assert (d["delaytime"][same] > 0).sum() > 100
    print("winds %s: %d stars, %d eligible neighbours, %d potential kicks, %d applied, largest ratio to the bound: %s; gaps: Hsml %.2e, p %.2e, r %.2e"
          % (label, len(listed), stats["neighbours"], stats["potential_kicks"], stats["applied"], ", ".join("%s %.3g" % kv for kv in worst.items()),
             info["hsml_gap"], info["p_margin"], info["r_gap"]))
    for key, val in worst.items():
        assert val <= 1, (label, key, val)


CASES = [(name, kind, dec) for name in ("zel", "clust") for kind, dec in R.MODELS]


@pytest.mark.parametrize("name,kind,dec", CASES)
def test_dev_form(pkg, name, kind, dec):
    """mpg_dev_winds_and_feedback; the first scene on a tree of gas AND black holes (the black holes are skipped), the second on the gas tree"""
    import torch
    d, par, out, info = R.restated(pkg.ics, name, kind, dec)
    mask = pkg.engine.GASMASK + (pkg.engine.BHMASK if name == "zel" else 0)
    eng, keep = bound_engine(pkg, torch, d, par, mask)
    ntree = eng.tree_stats().NumParticles
    assert ntree == int(((d["type_tree"] == 0) | ((d["type_tree"] == 5) & (name == "zel"))).sum()) > int((d["type"] == 0).sum())
    a = dev_arrays(torch, d)
    eng.dev_winds_and_feedback(a, up(torch, d["newstars"]), R.ATIME)
    eng.synchronize()
    stats = eng.winds_stats()
    s, g = eng.winds_export()
    t = eng.winds_times()
    assert t["weight_ms"] > 0 and t["feedback_ms"] > 0 and t["apply_ms"] > 0
    eng.close()
    pairs = set(zip(s.tolist(), g.tolist()))
    assert len(pairs) == len(s)
    compare(d, par, out, info, down(a), stats, pairs, "dev / %s / %s%s" % (name, kind, " / decoupling" if dec else ""))


@pytest.mark.parametrize("name,kind,dec", CASES)
def test_host_form(pkg, name, kind, dec):
    """mpg_winds_and_feedback: the table carries the current types and IsGarbage / Swallowed in its flags; the call builds the gas tree"""
    d, par, out, info = R.restated(pkg.ics, name, kind, dec)
    table_type = d["type"].copy()
    table_type[d["dead"]] = np.where(d["dead"] < d["ng"], 0, 4)
    table_type[d["swal"]] = 0
    P = pkg.make_particles(d["pos"], d["mass"], type=table_type)
    P["Flags"][d["dead"]] = 1
    P["Flags"][d["swal"]] = 1            # gas that a black hole swallowed is garbage at once (slots_mark_garbage)
    P["Flags"][d["dead"][-1]] = 2        # a swallowed star: not listed
    a = {k: d[k].copy() for k in ("id", "hsml", "vdisp", "density", "vel", "entropy", "delaytime")}
    a["totalweight"] = np.full(d["n"], SENT)
    a["kick_star"] = np.full(d["n"], 7, np.uint64)
    eng = new_engine(pkg, d, par)
    eng.winds_and_feedback(P, d["box"], a, d["newstars"], R.ATIME)
    stats = eng.winds_stats()
    assert eng.tree_stats().NumParticles == int((d["type"] == 0).sum())
    s, g = eng.winds_export()
    eng.close()
    assert np.array_equal(P["Mass"], d["mass"]) and np.array_equal(P["Type"], table_type)
    assert a["vdisp"].tobytes() == d["vdisp"].tobytes()              # an input goes up and does not come back
    compare(d, par, out, info, a, stats, set(zip(s.tolist(), g.tolist())), "host / %s / %s%s" % (name, kind, " / decoupling" if dec else ""))


def test_calls_with_nothing_to_do(pkg):
    """an empty list, or WIND_SUBGRID set: nothing is written and no tree is demanded or built"""
    import torch
    d = R.scene(pkg.ics, "zel")
    par = R.model("halo", True)
    for p, stars in ((par, None), (par, d["newstars"][:0]), (dict(par, WindModel=par["WindModel"] | R.WIND_SUBGRID), d["newstars"])):
        eng, keep = bound_engine(pkg, torch, d, p, 0)
        a = dev_arrays(torch, d)
        eng.dev_winds_and_feedback(a, None if stars is None else up(torch, stars), R.ATIME)
        eng.synchronize()
        assert has_no_tree(pkg, eng)
        st = eng.winds_stats()
        assert st["stars"] == 0 and st["potential_kicks"] == 0 and st["maxvel"] == 0
        got = down(a)
        for key in COLS:
            assert np.array_equal(got[key], d[key])
        assert (got["totalweight"] == SENT).all() and (got["kick_star"].view(np.int64) == -3).all()
        # ... and the host form: nothing travels, no tree
        h = {k: d[k].copy() for k in ("id", "hsml", "vdisp", "density", "vel", "entropy", "delaytime")}
        eng.winds_and_feedback(pkg.make_particles(d["pos"], d["mass"], type=d["type"]), d["box"], h, stars, R.ATIME)
        assert has_no_tree(pkg, eng)
        for key in COLS:
            assert np.array_equal(h[key], d[key])
        eng.close()


def test_errors(pkg):
    """a listed row that is no star, a missing random table, missing parameters, a tree without the gas, an undefined model"""
    import torch
    d = R.scene(pkg.ics, "zel")
    par = R.model("fixed", True)
    E = pkg.EngineError
    stars = up(torch, d["newstars"])

    def call(eng, rows=stars):
        a = dev_arrays(torch, d)
        eng.dev_winds_and_feedback(a, rows, R.ATIME)
        return a

    eng, keep = bound_engine(pkg, torch, d, par, pkg.engine.GASMASK)
    for bad in (d["tie_gas"], int(d["dead"][-1]), d["n"], -1):  # gas, a garbage star (type 7), rows outside the table
        rows = d["newstars"].copy()
        rows[3] = bad
        a = dev_arrays(torch, d)
        with pytest.raises(E, match="not a star"):
            eng.dev_winds_and_feedback(a, up(torch, rows), R.ATIME)
        got = down(a)
        for key in COLS:                                       # checked before anything is written
            assert np.array_equal(got[key], d[key])
    with pytest.raises(E, match="required"):
        a = dev_arrays(torch, d)
        a["vdisp"] = None
        eng.dev_winds_and_feedback(a, stars, R.ATIME)
    with pytest.raises(E, match="strange"):
        eng.set_wind_params(dict(par, WindModel=R.WIND_DECOUPLE_SPH | R.WIND_ISOTROPIC))
    call(eng)                                                  # the refused parameters changed nothing: the call still runs
    eng.close()
    eng, keep = bound_engine(pkg, torch, d, par, pkg.engine.GASMASK, table=False)
    with pytest.raises(E, match="random table"):
        call(eng)
    eng.close()
    eng, keep = bound_engine(pkg, torch, d, None, pkg.engine.GASMASK)
    with pytest.raises(E, match="no parameters"):
        call(eng)
    with pytest.raises(E, match="no parameters"):
        eng.dev_winds_subgrid(dev_arrays(torch, d), None, up(torch, np.zeros(d["n"])), R.ATIME, n=4)
    eng.close()
    eng, keep = bound_engine(pkg, torch, d, par, pkg.engine.DMMASK)
    with pytest.raises(E, match="does not contain the gas"):
        call(eng)
    eng.close()
    eng, keep = bound_engine(pkg, torch, d, par, 0)
    with pytest.raises(E, match="does not contain the gas"):
        call(eng)
    eng.close()


@pytest.mark.parametrize("kind", ["halo", "fixed"])
def test_subgrid_call(pkg, kind):
    """mpg_dev_winds_subgrid on 512 listed gas particles: the kicked set EQUAL, the kicks within the bounds above, every other row
    bit-identical; without WIND_SUBGRID nothing is written"""
    import torch
    d = R.scene(pkg.ics, "zel")
    rng = np.random.RandomState(21)
    rows = rng.choice(np.nonzero(d["type"] == 0)[0], 512, replace=False).astype(np.int32)
    sm = d["mass"].astype(np.float64) * 0.1 * rng.random_sample(d["n"])
    par = dict(R.model(kind, True), WindEfficiency=7.0)
    par["WindSigma0"] *= (7.0 / (0.3 * R.desnumngb(2, 1.0))) ** 0.5
    par["WindModel"] |= R.WIND_SUBGRID
    out, kicked, margin = R.winds_subgrid(d, rows, sm, par, d["table"], R.ATIME)
    assert margin > 1e-9 and 50 < len(kicked) < 462, (margin, len(kicked))
    eng, keep = bound_engine(pkg, torch, d, par, 0)
    a = dev_arrays(torch, d)
    eng.dev_winds_subgrid(a, up(torch, rows), up(torch, sm), R.ATIME)
    eng.synchronize()
    got = down(a)
    assert eng.winds_stats()["applied"] == len(kicked) and eng.winds_stats()["stars"] == 512
    k = np.array(sorted(kicked), np.int64)
    v = np.array([kicked[i][0] for i in k])
    dent = np.array([kicked[i][1] for i in k])
    same = np.ones(d["n"], bool)
    same[k] = False
    for key in COLS:
        assert np.array_equal(got[key][same], d[key][same]), key
    assert (got["delaytime"][k] > 0).all() and not (d["delaytime"][k] == got["delaytime"][k]).all()
    worst = dict(vel=(np.abs(got["vel"][k] - out["vel"][k]) / (TRANS_DIR * v[:, None] + 2 * EPS * np.abs(out["vel"][k]))).max(),
                 entropy=(np.abs(got["entropy"][k] - out["entropy"][k]) / ((TRANS + 4 * EPS) * (d["entropy"][k] + dent))).max(),
                 delaytime=(np.abs(got["delaytime"][k] / out["delaytime"][k] - 1) / (4 * EPS)).max())
    print("winds subgrid / %s: %d of 512 kicked, margin %.2e, largest ratio to the bound: %s" % (kind, len(k), margin, ", ".join("%s %.3g" % kv for kv in worst.items())))
    assert max(worst.values()) <= 1, worst
    # a listed row that is no gas particle is an error; without the bit the call does nothing
    with pytest.raises(pkg.EngineError, match="not gas"):
        eng.dev_winds_subgrid(dev_arrays(torch, d), up(torch, np.array([int(d["newstars"][0])], np.int32)), up(torch, sm), R.ATIME)
    eng.set_wind_params(dict(par, WindModel=par["WindModel"] & ~R.WIND_SUBGRID))
    b = dev_arrays(torch, d)
    eng.dev_winds_subgrid(b, up(torch, rows), up(torch, sm), R.ATIME)
    eng.synchronize()
    got = down(b)
    for key in COLS:
        assert np.array_equal(got[key], d[key])
    eng.close()


def test_evolve_call(pkg):
    """mpg_dev_winds_evolve: the reset by the density, the clamp to the maximum and the plain reduction, on an active sublist and on every
    row; rows that are not gas or not listed stay as they are.  DelayTime within 2 eps relative of the restatement, exactly 0 where the
    restatement gives 0 (both forms take the same IEEE division and subtraction); whether it is bit-identical is printed"""
    import torch
    d = R.scene(pkg.ics, "zel")
    n = d["n"]
    rng = np.random.RandomState(4)
    par = dict(R.model("halo", True), WindFreeTravelDensThresh=float(np.median(d["density"]) / R.ATIME ** 3 * 0.8), MaxWindFreeTravelTime=0.04)
    dt = np.where(rng.random_sample(n) < 0.7, 0.06 * rng.random_sample(n), 0.0)
    tb = rng.randint(0, 47, n).astype(np.uint8)
    T = pkg.engine.SphTimes()
    dloga = 0.03 * rng.random_sample(47)
    for k in range(47):
        T.dloga_bin[k] = dloga[k]
    T.atime, T.hubble = R.ATIME, 1.3
    eng, keep = bound_engine(pkg, torch, d, par, 0)
    for rows in (np.sort(rng.choice(n, n // 2, replace=False)).astype(np.int32), None):
        exp, branch = R.winds_evolve(dt, d["density"], d["type"], tb, dloga, 1.3, R.ATIME, par, range(n) if rows is None else rows)
        assert all((branch == b).sum() > 50 for b in (1, 2, 3))
        a = dict(density=up(torch, d["density"]), tb_hydro=up(torch, tb), delaytime=up(torch, dt))
        eng.dev_winds_evolve(a, T, None if rows is None else up(torch, rows))
        eng.synchronize()
        got = a["delaytime"].cpu().numpy()
        assert np.array_equal(got[branch == 0], dt[branch == 0]) and (got[branch == 1] == 0).all()
        assert (got[exp == 0] == 0).all()
        nz = exp != 0
        ratio = (np.abs(got[nz] - exp[nz]) / (2 * EPS * np.abs(exp[nz]))).max()
        print("winds evolve (%s): branches %s, largest ratio to the bound %.3g, bit-identical: %s"
              % ("all rows" if rows is None else "sublist", [(int(b), int((branch == b).sum())) for b in (0, 1, 2, 3)], ratio, np.array_equal(got, exp)))
        assert ratio <= 1
    with pytest.raises(pkg.EngineError, match="outside the table"):
        eng.dev_winds_evolve(a, T, up(torch, np.array([0, n], np.int32)))
    eng.close()
