"""The numpy restatement of metal_return (tests/metals_restated.py) against itself and against hand-worked cases: the final state of the
reference's shrinking stellar-density walk does not depend on the visiting order; the reference's literal return walk - float P.Mass and
Metals rounded per contribution, the cap on the running mass, stars in any order - agrees with the defined fp64 form within the float
rounding of its own path; mass and metal mass are conserved; one star with three gas particles by hand; the branches of ngb_narrow_down
that only ten radii and a fractional neighbour number reach.  No GPU."""
import math

import numpy as np
import pytest

import metals_restated as R

KT, ETA, MAXDEV = 2, 1.0, 2.0      # quintic kernel, DensityResolutionEta = 1: GetNumNgb = 113.097...


def small_scene(seed=3, ng=3000, nstar=40):
    rng = np.random.RandomState(seed)
    box = 1000.0
    a = ng // 2
    pos_gas = np.concatenate([box * rng.random_sample((a, 3)), np.mod(box * 0.5 + box / 10 * rng.standard_normal((ng - a, 3)), box)])
    return R.sample_scene(pos_gas, box, nstar, seed, ktype=KT, eta=ETA)


@pytest.fixture(scope="module")
def scene():
    d = small_scene()
    out, res, info = R.metal_return(d, d["box"], KT, ETA, MAXDEV, 1, d["maxgasmass"])
    return d, out, res, info


def test_shrinking_walk_is_independent_of_the_visiting_order():
    """stellar_density_ngbiter under shuffled visiting orders: the same maxcmpte, the same Ngb and VolumeSPH below it, the same closest
    index - and the closed form maxcmpte = 1 + min{i : complete Ngb_i > desnumngb} (10 if none) with complete sums for every j < maxcmpte"""
    d = small_scene()
    gas = np.nonzero(d["type"] == 0)[0]
    vol = d["mass"][gas].astype(np.float64) / d["density"][gas]
    des = R.desnumngb(KT, ETA)
    rng = np.random.RandomState(1)
    shrunk = 0
    for i in range(d["s0"], d["s0"] + 12):
        dist = R.nearest(d["pos"][i] - d["pos"][gas], d["box"])
        r2 = (dist * dist).sum(1)
        r = np.sqrt(r2)
        h0 = (3 * des / (4 * np.pi * d["ng"])) ** (1. / 3) * d["box"]
        for scale in (0.5, 1.0, 1.6, 3.0):
            radii = [R.effhsml(0.0, d["box"], scale * h0, d["box"], j) for j in range(R.NHSML)]
            wk = [np.where(r2 < rj * rj, R.kernel_wk(r / rj, rj, KT), 0.0) for rj in radii]
            complete = [float((wk[j] * R.kernel_volume(radii[j])).sum()) for j in range(R.NHSML)]
            over = [j for j in range(R.NHSML) if complete[j] > des]
            want_max = 1 + over[0] if over else R.NHSML
            shrunk += want_max < R.NHSML
            for sphw in (0, 1):
                ref = R.literal_walk(r2, wk, vol, radii, des, sphw)
                assert ref[2] == want_max
                assert ref[0][:want_max] == pytest.approx(complete[:want_max], rel=1e-12)
                close_ref = R.ngb_narrow_down(d["box"], 0.0, radii, ref[0], ref[2], int(des), d["box"])
                for _ in range(3):
                    got = R.literal_walk(r2, wk, vol, radii, des, sphw, rng.permutation(len(gas)))
                    assert got[2] == ref[2]
                    assert got[0][:want_max] == pytest.approx(ref[0][:want_max], rel=1e-12)
                    assert got[1][:want_max] == pytest.approx(ref[1][:want_max], rel=1e-12)
                    c = R.ngb_narrow_down(d["box"], 0.0, radii, got[0], got[2], int(des), d["box"])
                    assert c[3] == close_ref[3] and c[0] == pytest.approx(close_ref[0], rel=1e-12)
    assert shrunk > 12      # the shrink was exercised


def test_radius_loop_is_independent_of_the_visiting_order(scene):
    """the whole loop under shuffled neighbour orders: final Hsml, maxcmpte, close and the iteration count of every target"""
    d, out, res, _ = scene
    assert len(res["targets"]) > 25 and max(res["iterations"].values()) >= 4
    assert res["min_gap"] > 1e-10 and res["min_margin"] > 1e-9 and not any(res["tight"].values())
    rng = np.random.RandomState(2)
    for _ in range(2):
        hsml = d["hsml"].copy()
        got = R.stellar_density(d["pos"], d["type"], d["mass"], d["density"], hsml, res["targets"], d["box"], KT, ETA, MAXDEV, 1,
                                order=rng.permutation(int((d["type"] == 0).sum())))
        assert got["queue_lengths"] == res["queue_lengths"]
        for key in ("iterations", "maxcmpte", "close"):
            assert got[key] == res[key]
        t = np.array(res["targets"])
        assert np.abs(hsml[t] / out["hsml"][t] - 1).max() < 1e-12
        assert max(abs(got["volume"][i] / res["volume"][i] - 1) for i in t) < 1e-12


def test_converged_radius_holds_the_wanted_neighbour_number(scene):
    d, out, res, _ = scene
    des = res["des"]
    for i in res["targets"]:
        assert des - MAXDEV <= res["numngb"][i] <= des + MAXDEV
        # the saved volume is the one of trial radius `close`: all gas inside it, kernel weighted
        gas = np.nonzero(d["type"] == 0)[0]
        dist = R.nearest(d["pos"][i] - d["pos"][gas], d["box"])
        r = np.sqrt((dist * dist).sum(1))
        h = res["radius"][i]
        sel = r < h
        v = (d["mass"][gas][sel].astype(np.float64) / d["density"][gas][sel] * R.kernel_wk(r[sel] / h, h, KT)).sum()
        assert res["volume"][i] == pytest.approx(v, rel=1e-12)


def test_literal_order_of_the_stars_agrees_with_the_defined_form(scene):
    """(a) under 20 shuffles of the star order against (b): Mass within 1 float ulp per accepted contribution, Density / Metallicity /
    Metals within (k + 2) 2^-23 relative to the largest value on the path, the stars' own columns within the fp64 sums' error"""
    d, out, res, info = scene
    assert info["cap_margin"] > 1e-9 and info["refused"] > 0 and info["k"].max() >= 3
    gas = info["gas"]
    k = info["k"]
    rng = np.random.RandomState(4)
    u = 2.0 ** -23
    for _ in range(20):
        order = [int(i) for i in rng.permutation(res["targets"])]
        a = R.return_literal(d, order, out["hsml"], res["volume"], d["box"], KT, 1, d["maxgasmass"])
        assert a["refused"] == info["refused"]
        bound = (k + 2) * u
        assert (np.abs(a["mass"][gas].astype(np.float64) - out["mass"][gas]) <= bound * out["mass"][gas]).all()
        assert (np.abs(a["density"][gas] - out["density"][gas]) <= bound * out["density"][gas]).all()
        zmax = np.maximum(d["metallicity"][gas], out["metallicity"][gas])
        assert (np.abs(a["metallicity"][gas] - out["metallicity"][gas]) <= bound * zmax).all()
        smax = np.maximum(d["metals"][gas], out["metals"][gas])
        assert (np.abs(a["metals"][gas].astype(np.float64) - out["metals"][gas]) <= bound[:, None] * smax).all()
        untouched = gas[k == 0]
        assert np.array_equal(a["mass"][untouched], d["mass"][untouched]) and np.array_equal(a["density"][untouched], d["density"][untouched])
        for i in res["targets"]:
            n = info["nacc"][i]
            assert abs(a["massreturn"][i] - info["massreturn"][i]) <= (n + 2) * u * info["massreturn"][i] + 1e-300
        t = np.array(res["targets"])
        assert np.array_equal(a["lastenrichment"][t], d["stellarage"][t])


def test_mass_and_metal_mass_are_conserved(scene):
    d, out, res, info = scene
    gas = info["gas"]
    M0 = d["mass"][gas].astype(np.float64)
    total = sum(info["massreturn"].values())
    assert info["dM"].sum() == pytest.approx(total, rel=1e-13)
    # the float masses carry it to their own rounding
    assert (out["mass"][gas].astype(np.float64) - M0).sum() == pytest.approx(total, rel=1e-5)
    t = np.array(res["targets"])
    assert (d["mass"][t].astype(np.float64) - out["mass"][t]).sum() == pytest.approx(total, rel=1e-5)
    assert (out["totalmassreturned"][t] - d["totalmassreturned"][t]).sum() == pytest.approx(total, rel=1e-12)
    dzm = (out["metallicity"][gas] * info["Mnew"] - d["metallicity"][gas] * M0).sum()
    assert dzm == pytest.approx(info["accepted_metal"], rel=1e-10)
    # Density follows the mass: Mass / Density is unchanged
    assert np.allclose(info["Mnew"] / out["density"][gas], M0 / d["density"][gas], rtol=1e-14)
    # rows that are no target and no touched gas are bit-identical
    same = np.ones(d["n"], bool)
    same[t] = False
    same[gas[info["touched"]]] = False
    for key in ("mass", "density", "metallicity", "metals", "totalmassreturned", "lastenrichment", "hsml"):
        assert np.array_equal(out[key][same], d[key][same]), key


def test_one_star_three_gas_particles_by_hand():
    """a star at the origin of a box of 100 with Hsml = 2 and three gas particles at r = 0.5, 1 and 3 (outside), no SPH weighting:
    returnfraction = volume_j / (volume_1 + volume_2)"""
    pos = np.array([[10.5, 10, 10], [10, 11, 10], [10, 10, 13], [10, 10, 10]], np.float64)
    d = dict(pos=pos, type=np.array([0, 0, 0, 4], np.uint8), mass=np.array([1, 2, 1, 5], np.float32), density=np.array([2.0, 1.0, 1.0, 0.0]),
             metallicity=np.array([0.0, 0.01, 0.0, 0.0]), metals=np.zeros((4, 9)), massgenerated=np.array([0, 0, 0, 0.5]),
             metalgenerated=np.array([0, 0, 0, 0.05]), speciesgenerated=np.zeros((4, 9)), stellarage=np.array([0, 0, 0, 77.0]),
             totalmassreturned=np.zeros(4), lastenrichment=np.zeros(4))
    d["speciesgenerated"][3, 2] = 0.025
    hsml = np.array([0, 0, 0, 2.0])
    volume = {3: 0.5 + 2.0}                                     # 1 / 2 + 2 / 1
    out, info = R.return_defined(d, [3], hsml, volume, 100.0, KT, 0, maxgasmass=4.0)
    # gas 0: rf = 0.2, thismass 0.1; gas 1: rf = 0.8, thismass 0.4; gas 2 is outside
    assert out["mass"][0] == np.float32(1.1) and out["mass"][1] == np.float32(2.4) and out["mass"][2] == 1
    assert out["density"][0] == pytest.approx(2.2) and out["density"][1] == pytest.approx(1.2)
    assert out["metallicity"][0] == pytest.approx(0.2 * 0.05 / 1.1)
    assert out["metallicity"][1] == pytest.approx((0.01 * 2 + 0.8 * 0.05) / 2.4)
    assert out["metals"][1, 2] == pytest.approx(0.8 * 0.025 / 2.4) and out["metals"][1, 3] == 0
    assert out["mass"][3] == np.float32(4.5) and out["totalmassreturned"][3] == pytest.approx(0.5) and out["lastenrichment"][3] == 77.0
    assert info["refused"] == 0
    # a cap of 2.3: gas 1 (2 + 0.4) is refused, the star keeps that mass
    out, info = R.return_defined(d, [3], hsml, volume, 100.0, KT, 0, maxgasmass=2.3)
    assert info["refused"] == 1 and out["mass"][1] == 2 and out["density"][1] == 1.0 and out["metallicity"][1] == 0.01
    assert out["mass"][3] == np.float32(4.9) and info["massreturn"][3] == pytest.approx(0.1)
    # the literal form gives the same here
    a = R.return_literal(d, [3], hsml, volume, 100.0, KT, 0, 2.3)
    assert a["refused"] == 1 and a["mass"][0] == np.float32(1.1) and a["mass"][3] == np.float32(4.9)
    # with SPH weighting the kernel value at r / h weighs the volumes
    w0, w1 = float(R.kernel_wk(0.25, 2.0, KT)), float(R.kernel_wk(0.5, 2.0, KT))
    vol = {3: 0.5 * w0 + 2.0 * w1}
    out, info = R.return_defined(d, [3], hsml, vol, 100.0, KT, 1, maxgasmass=4.0)
    assert out["mass"][0] == np.float32(1 + 0.5 * (0.5 * w0) / vol[3]) and info["massreturn"][3] == pytest.approx(0.5)


def test_trial_radii_and_kernel():
    """effhsml: ten radii evenly split in volume between 0.1 Hsml and 1.1 Hsml on the first pass, between the bracket later; the kernel is
    normalised (sum of wk kernel_volume over a fine uniform lattice is the number of points inside the support's unit density volume)"""
    box = 1000.0
    r = [R.effhsml(0.0, box, 10.0, box, j) for j in range(10)]
    v = np.array(r) ** 3
    assert np.allclose(np.diff(v), (11.0 ** 3 - 1.0) / 11) and v[0] == pytest.approx(1.0 + (11.0 ** 3 - 1.0) / 11)
    r = [R.effhsml(4.0, 8.0, 99.0, box, j) for j in range(10)]
    assert r[0] > 4.0 and r[-1] < 8.0 and np.allclose(np.diff(np.array(r) ** 3), (512.0 - 64.0) / 11)
    g = (np.arange(-20, 20) + 0.5) * 0.25
    x, y, z = np.meshgrid(g, g, g, indexing="ij")
    rr = np.sqrt(x * x + y * y + z * z)
    for kt in (1, 2, 4):
        h = 4.0
        w = np.where(rr < h, R.kernel_wk(rr / h, h, kt), 0.0)
        assert w.sum() * 0.25 ** 3 == pytest.approx(1.0, rel=2e-3)
    assert R.desnumngb(2, 1.0) == pytest.approx(4 * math.pi / 3 * 27, rel=1e-9) and int(R.desnumngb(2, 1.0)) == 113


def test_narrow_down_with_ten_radii():
    """branches of ngb_narrow_down that five radii and integer counts do not reach.  desnumngb arrives truncated (113 for 113.097)."""
    box = 1000.0
    rad = [float(j + 1) for j in range(10)]
    cube = lambda v: v ** (1. / 3)
    # growth with maxcmpt = 10: the slope comes from entries 8 and 9, the volume is extrapolated from radius[close]
    num = [2.0 * j + 0.5 for j in range(10)]             # all below 113: left = radius[9], right stays the box
    h, right, left, close = R.ngb_narrow_down(box, 0.0, rad, num, 10, 113, box)
    dngbdv = (num[9] - num[8]) / (1000.0 - 729.0)
    assert close == 9 and left == 10.0 and right == box
    assert h == pytest.approx(cube(1000.0 + (113 - num[9]) / dngbdv)) and 10.0 < h < 40.0
    num = [0.1 * j + 0.05 for j in range(10)]            # a shallow slope: the extrapolation (67) is capped at four times radius[close]
    h, right, left, close = R.ngb_narrow_down(box, 0.0, rad, num, 10, 113, box)
    assert cube(1000.0 + (113 - num[9]) / (0.1 / 271.0)) > 40.0 and h == 40.0
    num = [100.0 + 1.4 * j for j in range(10)]           # 100 .. 112.6: a steep slope, the extrapolation stays below the cap
    h, right, left, close = R.ngb_narrow_down(box, 0.0, rad, num, 10, 113, box)
    assert h == pytest.approx(cube(1000.0 + (113 - num[9]) / (1.4 / 271.0))) and 10.0 < h < 40.0
    # a fractional sum between the truncated and the full neighbour number: NOT above 113.097 for the walk (maxcmpt stays 10), but above 113
    # inside ngb_narrow_down - it sets the right edge and ends the scan there
    num = [20.0, 60.0, 100.0, 113.05, 113.08, 113.09, 150.0, 200.0, 250.0, 300.0]
    h, right, left, close = R.ngb_narrow_down(box, 0.0, rad, num, 10, 113, box)
    assert close == 3 and right == 4.0 and left == 3.0 and h == 4.0
    # closest index in the upper half (beyond what five radii have), bracketed on both sides: hsml = radius[close] unchanged
    num = [10.0, 20.0, 30.0, 40.0, 60.0, 80.0, 112.0, 140.0, 0.0, 0.0]
    h, right, left, close = R.ngb_narrow_down(50.0, 2.0, rad, num, 8, 113, box)
    assert close == 6 and left == 7.0 and right == 8.0 and h == 7.0
    # an exact hit of the truncated number moves neither edge at that entry
    num = [50.0, 113.0, 180.0] + [0.0] * 7
    h, right, left, close = R.ngb_narrow_down(50.0, 0.5, rad, num, 3, 113, box)
    assert close == 1 and left == 1.0 and right == 3.0 and h == 2.0
    # left == 0 with ten radii and the first entry already above: extrapolation DOWN from radius[0] with the slope of entries 0 and 1
    num = [200.0, 900.0] + [0.0] * 8
    h, right, left, close = R.ngb_narrow_down(box, 0.0, rad, num, 1, 113, box)
    assert close == 0 and right == 1.0 and left == 0.0
    assert h == pytest.approx(cube(1.0 + (113 - 200.0) / (200.0 / 1.0)))        # maxcmpt == 1: dngbdv = num[0] / radius[0]^3
    num = [120.0, 400.0] + [0.0] * 8
    h, right, left, close = R.ngb_narrow_down(box, 0.0, rad, num, 2, 113, box)
    assert right == 1.0 and h == pytest.approx(cube(1.0 + (113 - 120.0) / (280.0 / 7.0)))


def test_error_cases():
    d = small_scene()
    tl = R.targets(d["type"], d["mass"], d["totalmassreturned"], d["massgenerated"])
    bad = d["hsml"].copy()
    bad[tl[0]] = 0.0
    with pytest.raises(R.MetalError):
        R.stellar_density(d["pos"], d["type"], d["mass"], d["density"], bad, tl[:1], d["box"], KT, ETA, MAXDEV, 1)
    # stars below the work threshold, garbage rows and non-active stars are no targets
    s = np.arange(d["s0"], d["n"])
    low = [i for i in s if d["massgenerated"][i] < 1e-3 * (d["mass"][i] + d["totalmassreturned"][i])]
    assert len(low) >= 3 and not set(low) & set(tl) and not set(d["dead"].tolist()) & set(tl)
    assert len(tl) == len(s) - len(set(low) | (set(d["dead"].tolist()) & set(s.tolist())))
    act = s[::2]
    assert set(R.targets(d["type"], d["mass"], d["totalmassreturned"], d["massgenerated"], act)) == set(tl) & set(act.tolist())
