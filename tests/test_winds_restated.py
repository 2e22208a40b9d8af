"""The numpy restatement of the wind model (tests/winds_restated.py) held against itself and against hand-computed cases, on the CPU:
form (a) - the reference's list, sorted with cmp_by_part_id - equals form (b) - the minimum over (r, StarID) - bit for bit under permutations
of the star list; an exact tie goes to the smaller star ID; the conditions that make the GPU comparison one of equal integers hold for the
committed seeds (so test_gpu_winds.py's caps are proven here, not on the GPU); get_wind_params, the delay cap and winds_evolve by hand."""
import math

import numpy as np
import pytest

import winds_restated as R


def test_module_is_part_of_the_package(pkg):
    """the engine mirrors what is restated here: the parameter struct, the array struct and the model bits"""
    E = pkg.engine
    assert [k for k, _ in E.WindParams._fields_] == ["WindModel", "WindEfficiency", "WindSigma0", "WindSpeedFactor", "MinWindVelocity",
                                                     "WindThermalFactor", "WindFreeTravelLength", "WindSpeed", "MaxWindFreeTravelTime",
                                                     "WindFreeTravelDensThresh"]
    assert set(R.model("halo", True)) == set(k for k, _ in E.WindParams._fields_)
    assert (E.WIND_SUBGRID, E.WIND_DECOUPLE_SPH, E.WIND_USE_HALO, E.WIND_FIXED_EFFICIENCY, E.WIND_ISOTROPIC) == (1, 2, 4, 8, 512)
    assert E.WIND_ARRAY_FIELDS == ("id", "hsml", "vdisp", "density", "tb_hydro", "vel", "entropy", "delaytime", "totalweight", "kick_star")


@pytest.mark.parametrize("name", ["zel", "clust"])
def test_literal_equals_defined_under_permutations(pkg, name):
    """(a) == (b) bit for bit for the list as committed and four permutations of it, and every permutation gives the same result"""
    d = R.scene(pkg.ics, name)
    par = R.model("halo", True)
    ref, info = R.winds_and_feedback(d, d["newstars"], par, d["table"], R.ATIME)
    rng = np.random.RandomState(11)
    orders = [d["newstars"], d["newstars"][::-1]] + [d["newstars"][rng.permutation(len(d["newstars"]))] for _ in range(3)]
    for order in orders:
        b, ib = R.winds_and_feedback(d, order, par, d["table"], R.ATIME)
        a, ia = R.winds_and_feedback(d, order, par, d["table"], R.ATIME, literal=True)
        for key in ("vel", "entropy", "delaytime", "kick_star"):
            assert np.array_equal(a[key], b[key]), key
            assert np.array_equal(b[key], ref[key]), key
        assert ia["maxvel"] == ib["maxvel"] == info["maxvel"] and ia["applied"] == ib["applied"]
        assert ib["pairs"] == info["pairs"]


def test_exact_tie_goes_to_the_smaller_star_id():
    box = 8.0
    g = np.array([2.0, 3.0, 2.5])
    dl = np.array([1 / 32, -1 / 64, 1 / 128])
    for ids in ((50, 9), (9, 50), ((1 << 63) + 4, 3)):
        d = dict(pos=np.array([g, g + dl, g - dl]), type=np.array([0, 4, 4], np.uint8), mass=np.ones(3, np.float32), box=box,
                 id=np.array([1000, ids[0], ids[1]], np.uint64), hsml=np.array([0.0, 0.5, 0.5]), vdisp=np.array([0.0, 12.0, 20.0]),
                 delaytime=np.zeros(3), density=np.ones(3), vel=np.zeros((3, 3)), entropy=np.ones(3))
        table = np.zeros(7)                       # every pair is a potential kick
        par = R.model("halo", True)
        for order in ([1, 2], [2, 1]):
            for literal in (False, True):
                out, info = R.winds_and_feedback(d, order, par, table, R.ATIME, literal=literal)
                assert len(info["kicks"]) == 2 and info["kicks"][0][1] == info["kicks"][1][1]
                assert info["applied"] == 1 and int(out["kick_star"][0]) == min(ids) + 1
                v = par["WindSpeedFactor"] * d["vdisp"][1 + ids.index(min(ids))]
                assert info["maxvel"] == v
                assert math.isclose(float(np.linalg.norm(out["vel"][0])), v, rel_tol=1e-14)


@pytest.mark.parametrize("name", ["zel", "clust"])
def test_scene_conditions_hold_for_the_committed_seeds(pkg, name):
    for kind, dec in R.MODELS:
        d, par, out, info = R.restated(pkg.ics, name, kind, dec)
        c = R.conditions(d, info)
        # what the scene is for
        s0 = d["s0"]
        listed = d["newstars"]
        assert (info["totalweight"] == 0).sum() >= 5                                           # Hsml x 0.05: no gas inside
        assert info["nterm"].max() > 120 * 8                                                   # Hsml x 20: more than one leaf list holds
        assert (d["vdisp"][listed] <= 0).sum() >= 5 and (d["vdisp"][listed] == 1e-3).sum() >= 5
        assert int(s0) in listed and set(d["conv"].tolist()) <= set(listed.tolist())           # the corner star; gas that became a star
        assert (d["type"][d["conv"]] == 4).all() and (d["type_tree"][d["conv"]] == 0).all()
        assert (d["type"][d["swal"]] == 7).all() and (d["type_tree"][d["swal"]] == 0).all()
        assert (d["type_tree"] == 5).sum() >= 3 and (d["delaytime"][:d["ng"]] > 0).mean() > 0.05
        big = int(1 << 63)
        assert any(int(d["id"][k[5]]) >= big and int(d["id"][k[0]]) >= big for k in info["kicks"])   # an ID sum that wraps
        kicked = set(info["best"])
        assert not kicked & set(np.nonzero(d["delaytime"] > 0)[0].tolist())
        assert not kicked & set(np.nonzero(d["type"] != 0)[0].tolist())
        if kind == "halo":                                                                     # the floor on v is active for some kicks
            assert any(k[3] == par["MinWindVelocity"] * R.ATIME for k in info["best"].values())
        if dec:                                                                                # both branches of the delay cap
            dt = out["delaytime"][sorted(kicked)]
            assert (dt == par["MaxWindFreeTravelTime"]).any() and ((dt > 0) & (dt < par["MaxWindFreeTravelTime"])).any() or kind == "fixed"
        else:
            assert np.array_equal(out["delaytime"], d["delaytime"])
        assert c["multi"] >= 20 and c["notfirst"] >= 5


def test_get_wind_params_by_hand():
    par = dict(WindModel=R.WIND_USE_HALO, WindEfficiency=2.0, WindSigma0=353.0, WindSpeedFactor=3.7, MinWindVelocity=100.0, WindThermalFactor=0.5,
               WindFreeTravelLength=20.0, WindSpeed=400.0, MaxWindFreeTravelTime=0.06, WindFreeTravelDensThresh=0.0)
    # ofjt10: vphys = 200, utherm = 0.5 * 1.5 * 4e4 = 3e4, windeff = 353^2 / (4e4 + 6e4), v = 3.7 * 100 = 370 > 100 * 0.5
    v, eff, u = R.get_wind_params(par, 100.0, 0.5)
    assert (v, u) == (370.0, 30000.0) and eff == 353.0 ** 2 / 1e5
    # ... below the floor: v = 3.7 * 10 = 37 < MinWindVelocity * time = 50
    v, eff, u = R.get_wind_params(par, 10.0, 0.5)
    assert v == 50.0 and u == 0.75 * 400.0 and eff == 353.0 ** 2 / (400.0 + 600.0)
    # vs08: fixed efficiency and speed; the floor applies there too
    fx = dict(par, WindModel=R.WIND_FIXED_EFFICIENCY)
    assert R.get_wind_params(fx, 100.0, 0.5) == (200.0, 2.0, 30000.0)
    assert R.get_wind_params(dict(fx, MinWindVelocity=500.0), 100.0, 0.5)[0] == 250.0
    with pytest.raises(R.WindError):
        R.get_wind_params(dict(par, WindModel=R.WIND_DECOUPLE_SPH | R.WIND_ISOTROPIC), 100.0, 0.5)


def test_delay_cap_and_kick_by_hand():
    par = R.model("halo", True)
    table = np.full(11, 0.5)                       # theta = acos(0) = pi / 2, phi = pi: dir = (-1, 0, 0) to rounding
    mk = lambda: dict(vel=np.zeros((1, 3)), entropy=np.array([2.0]), delaytime=np.array([0.0]))
    ids, rho = np.array([5], np.uint64), np.array([0.25 ** 3 * 8.0])     # Density / atime^3 = 8: enttou = 8^(2/3) / (2/3) = 6
    out = mk()
    R.wind_do_kick(out, ids, rho, 0, 100.0, 3.0, 0.25, par, table)     # 20 / (100 / 0.25) = 0.05 < 0.1
    assert out["delaytime"][0] == 0.05 and abs(out["vel"][0, 0] + 100.0) < 1e-12 and abs(out["entropy"][0] - 2.5) < 1e-14
    out = mk()
    R.wind_do_kick(out, ids, rho, 0, 10.0, 3.0, 0.25, par, table)      # 20 / (10 / 0.25) = 0.5 > 0.1: capped
    assert out["delaytime"][0] == 0.1
    out = mk()
    R.wind_do_kick(out, ids, rho, 0, 10.0, 3.0, 0.25, dict(par, MaxWindFreeTravelTime=0.0), table)
    assert out["delaytime"][0] == 0.0 and out["entropy"][0] > 2.0     # never decouples: DelayTime is not written
    out = mk()
    R.wind_do_kick(out, ids, rho, 0, 0.0, 3.0, 0.25, par, table)       # v == 0: nothing
    assert out["entropy"][0] == 2.0 and not out["vel"].any()


def test_winds_evolve_three_branches_by_hand():
    par = dict(R.model("halo", True), WindFreeTravelDensThresh=1.0, MaxWindFreeTravelTime=0.1)
    dloga = np.zeros(47)
    dloga[3], dloga[4] = 0.02, 0.5
    a = 0.5                                          # a3inv = 8
    #            reset by density   reduced     clamped then reduced   reduced to 0   no delay   not gas   not listed
    dt = np.array([0.05,            0.05,       0.7,                   0.05,          0.0,       0.05,     0.05])
    rho = np.array([0.1,            1.0,        1.0,                   1.0,           1.0,       1.0,      1.0])
    tb = np.array([3,               3,          3,                     4,             3,         3,        3], np.uint8)
    ty = np.array([0,               0,          0,                     0,             0,         4,        0], np.uint8)
    new, branch = R.winds_evolve(dt, rho, ty, tb, dloga, 2.0, a, par, range(6))
    assert new.tolist() == [0.0, 0.05 - 0.01, 0.1 - 0.01, 0.0, 0.0, 0.05, 0.05]
    assert branch.tolist() == [1, 3, 2, 3, 0, 0, 0]


def test_subgrid_probability_by_hand():
    par = dict(R.model("fixed", True), WindModel=R.WIND_FIXED_EFFICIENCY | R.WIND_SUBGRID, WindEfficiency=2.0)
    d = dict(vel=np.zeros((2, 3)), entropy=np.ones(2), delaytime=np.zeros(2), vdisp=np.array([10.0, 10.0]), mass=np.array([1.0, 1.0], np.float32),
             id=np.array([7, 8], np.uint64), density=np.ones(2))
    prob = 1 - math.exp(-2.0 * 0.25 / 1.0)
    table = np.zeros(16)
    table[(7 + 2) % 16] = prob - 1e-6              # kicked
    table[(8 + 2) % 16] = prob + 1e-6              # not kicked
    out, kicked, margin = R.winds_subgrid(d, [0, 1], np.array([0.25, 0.25]), par, table, 0.5)
    assert list(kicked) == [0] and abs(margin - 1e-6) < 1e-12
    assert out["delaytime"][0] > 0 and out["delaytime"][1] == 0 and not out["vel"][1].any()
    # without WIND_SUBGRID the call does nothing
    out, kicked, _ = R.winds_subgrid(d, [0, 1], np.array([0.25, 0.25]), dict(par, WindModel=R.WIND_FIXED_EFFICIENCY), table, 0.5)
    assert not kicked and not out["vel"].any()
