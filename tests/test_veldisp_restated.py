"""The numpy restatement of winds_find_vel_disp (tests/veldisp_restated.py) against itself and against hand-worked cases: the final
state of the reference's shrinking walk does not depend on the visiting order, a converged radius encloses 39-41 DM particles, VDisp is
sqrt(var / 3) of exactly those neighbours, and ngb_narrow_down takes each of its branches as worked out by hand.  No GPU."""
import math

import numpy as np
import pytest

import veldisp_restated as R


def small_set(seed=5, nd=4096, ng=60):
    rng = np.random.RandomState(seed)
    box = 1000.0
    a = nd // 2
    pos_dm = np.concatenate([box * rng.random_sample((a, 3)), np.mod(box * 0.5 + box / 12 * rng.standard_normal((nd - a, 3)), box)])
    pos_gas = np.concatenate([box * rng.random_sample((ng // 2, 3)), np.mod(box * 0.5 + box / 12 * rng.standard_normal((ng - ng // 2, 3)), box)])
    # (some targets right at the faces of the box)
    pos_gas[0] = [0.5, 500.0, 999.7]
    pos_gas[1] = [999.9, 0.2, 300.0]
    return R.sample_inputs(pos_gas, pos_dm, box, seed, nbh=4, ngarbage=10), R.sample_times(seed)


def run(d, t, thr=0.0, active=None, order=None):
    vd = np.full(d["n"], -1.0)
    res = R.find_vel_disp(d["pos"], d["type"], d["vel"], d["gacc"], d["gpm"], d["tb_grav"], d["hsml"], d["dthsml"], d["density"], vd, d["box"],
                          t["Time"], t["hubble"], t["ddrift"], thr, t["gravkicks"], t["FgravkickB"], active=active, order=order)
    return vd, res


def test_shrinking_walk_is_independent_of_the_visiting_order():
    """wind_vdisp_ngbiter under shuffled visiting orders: the same maxcmpte, the same Ngb below it, the same closest index - and the closed
    form maxcmpte = 1 + min{i : complete N_i > 40} (5 if none) with complete counts for every j < maxcmpte."""
    d, t = small_set()
    dm = np.nonzero(d["type"] == 1)[0]
    velpred = R.dm_velpred(d["vel"][dm], d["gacc"][dm], d["gpm"][dm], d["tb_grav"][dm], t["gravkicks"], t["FgravkickB"])
    rng = np.random.RandomState(1)
    shrunk = 0
    for i in range(40):
        dist = R.nearest(d["pos"][i] - d["pos"][dm], d["box"])
        r2 = (dist * dist).sum(1)
        vterm = velpred - d["vel"][i] + t["hubble"] * t["Time"] ** 2 * dist
        for scale in (0.6, 1.0, 1.8, 3.0):          # from too few to several times too many neighbours
            radii = [R.effdmradius(0.0, d["box"], scale * d["hsml"][i], d["box"], j) for j in range(5)]
            complete = [int((np.sqrt(r2) < rj).sum()) for rj in radii]
            over = [j for j in range(5) if complete[j] > 40]
            want_max = 1 + over[0] if over else 5
            ref = R.literal_walk(r2, vterm, radii)
            assert ref[3] == want_max and [int(x) for x in ref[0][:want_max]] == complete[:want_max]
            shrunk += want_max < 5
            close_ref = R.ngb_narrow_down(d["box"], 0.0, radii, ref[0], ref[3], 40, d["box"])[3]
            for _ in range(3):
                order = rng.permutation(len(dm))
                got = R.literal_walk(r2, vterm, radii, order)
                assert got[3] == ref[3] and got[0][:want_max] == ref[0][:want_max]
                assert R.ngb_narrow_down(d["box"], 0.0, radii, got[0], got[3], 40, d["box"])[3] == close_ref
                for j in range(want_max):
                    assert got[2][j] == pytest.approx(ref[2][j], rel=1e-12)
                    assert got[1][j] == pytest.approx(ref[1][j], rel=1e-9, abs=1e-9 * math.sqrt(ref[2][j] + 1))
    assert shrunk > 20      # the shrink was exercised


def test_converged_radius_encloses_40_and_vdisp_is_the_spread_of_those_neighbours():
    d, t = small_set()
    vd, res = run(d, t)
    dm = np.nonzero(d["type"] == 1)[0]
    velpred = R.dm_velpred(d["vel"][dm], d["gacc"][dm], d["gpm"][dm], d["tb_grav"][dm], t["gravkicks"], t["FgravkickB"]).astype(np.longdouble)
    targets = sorted(res["iterations"])
    assert len(targets) == 60 - 5 and res["built"] and max(res["iterations"].values()) > 1
    assert not any(res["tight"].values())
    for i in targets:
        dist = R.nearest(d["pos"][i] - d["pos"][dm], d["box"])
        r = np.sqrt((dist * dist).sum(1))
        sel = r < res["radius"][i]
        n = int(sel.sum())
        assert 39 <= n <= 41 and n == res["numngb"][i]
        v = velpred[sel] - d["vel"][i].astype(np.longdouble) + np.longdouble(t["hubble"] * t["Time"] ** 2) * dist[sel].astype(np.longdouble)
        var = (v * v).sum() / n - ((v.sum(0) / n) ** 2).sum()
        assert var > 0 and vd[i] == pytest.approx(float(np.sqrt(var / 3)), rel=1e-12)
    # black holes: one pass at Hsml; untouched rows keep the sentinel
    for i, numdm in res["bh_numdm"].items():
        dist = R.nearest(d["pos"][i] - d["pos"][dm], d["box"])
        sel = (dist * dist).sum(1) < d["hsml"][i] ** 2
        assert int(sel.sum()) == numdm
        if numdm > 1:
            v = velpred[sel] - d["vel"][i].astype(np.longdouble)
            var = (v * v).sum() / numdm - ((v.sum(0) / numdm) ** 2).sum()
            assert vd[i] == pytest.approx(float(np.sqrt(var / 3)), rel=1e-12)
    written = set(targets) | {i for i, k in res["bh_numdm"].items() if k > 1}
    assert all(vd[i] == -1.0 for i in range(d["n"]) if i not in written)
    assert d["type"][d["n"] - 1] == 7 and (d["n"] - 1) not in res["bh_numdm"]       # the swallowed black hole is no target


def test_threshold_active_list_and_early_exit():
    d, t = small_set()
    thr = 10.0 * np.median(d["density"][:d["ng"]])         # 0.1 * thr = the median: about half of the gas
    vd, res = run(d, t, thr=thr)
    want = R.gas_targets(d["type"], d["hsml"], d["dthsml"], d["density"], t["ddrift"], thr)
    assert sorted(res["iterations"]) == want and 15 < len(want) < 45
    act = np.arange(0, d["n"], 3)
    vd2, res2 = run(d, t, thr=thr, active=act)
    assert sorted(res2["iterations"]) == [i for i in want if i % 3 == 0]
    assert all(vd2[i] == vd[i] for i in res2["iterations"])
    # nothing qualifies and no black hole in the table: nothing built, nothing written
    d3 = dict(d)
    d3["type"] = d["type"].copy()
    d3["type"][d["type"] == 5] = 7
    vd3, res3 = run(d3, t, thr=1e30)
    assert not res3["built"] and (vd3 == -1.0).all() and res3["queue_lengths"] == []
    # black holes but no qualifying gas: the tree is demanded, the black holes are written
    vd4, res4 = run(d, t, thr=1e30)
    assert res4["built"] and res4["queue_lengths"] == [] and len(res4["bh_numdm"]) == 3
    assert all(vd4[i] == vd[i] for i in res4["bh_numdm"])


def test_zero_hsml_does_not_converge():
    """a gas particle with Hsml = 0 keeps DMRadius = 0 for ever: the reference's endrun(1155) after 400 iterations"""
    d, t = small_set()
    live = int(np.nonzero(d["type"] == 0)[0][0])
    d["hsml"][live] = 0.0
    with pytest.raises(R.NoConvergence):
        run(d, t, active=np.array([live]))


BOX = 100.0
NAN = float("nan")


@pytest.mark.parametrize("name, right, left, radius, num, maxcmpt, want", [
    # growth at Right > 0.99 Box from the last two entries: dngbdv = 1 / 61, newvolume = 125 + 35 * 61 = 2260 (< (4 * 5)^3)
    ("growth", BOX, 0.0, [1, 2, 3, 4, 5], [1, 2, 3, 4, 5], 5, (2260 ** (1. / 3), BOX, 5.0, 4)),
    # no gradient: the factor 4 on radius[close = 0] = 1, then the clamp from below at Left = radius[4]
    ("clamp_left", BOX, 0.0, [1, 2, 3, 4, 5], [1, 1, 1, 1, 1], 5, (5.0, BOX, 5.0, 0)),
    # the factor 4 beyond Right: the clamp from above
    ("clamp_right", BOX, 0.0, [26, 27, 28, 29, 30], [1, 1, 1, 1, 1], 5, (BOX, BOX, 30.0, 0)),
    # Left == 0 extrapolation with two entries: dngbdv = 19 / 19, dngb = -4, newvolume = 8 - 4
    ("left0", BOX, 0.0, [2, 3, NAN, NAN, NAN], [44, 63, NAN, NAN, NAN], 2, (4 ** (1. / 3), 2.0, 0.0, 0)),
    # maxcmpt == 1 (treewalk.c:1418-1422): entries 1.. undefined, dngbdv = 80 / 8, newvolume = 8 - 40 / 10
    ("maxcmpt1", BOX, 0.0, [2, NAN, NAN, NAN, NAN], [80, NAN, NAN, NAN, NAN], 1, (4 ** (1. / 3), 2.0, 0.0, 0)),
    # maxcmpt == 1 at Right > 0.99 Box: the growth branch has no gradient (:1400), factor 4, clamp to Right = 99.5, then the Left == 0
    # extrapolation with dngbdv = 80 / 99.5^3: newvolume = 99.5^3 / 2
    ("maxcmpt1_growth", BOX, 0.0, [99.5, NAN, NAN, NAN, NAN], [80, NAN, NAN, NAN, NAN], 1, (99.5 / 2 ** (1. / 3), 99.5, 0.0, 0)),
    # a bracket: Left from the last count below 40, Right from the first above, the closest count wins
    ("bracket", BOX, 0.0, [1, 2, 3, 4, 5], [10, 30, 38, 45, 60], 4, (3.0, 4.0, 3.0, 2)),
])
def test_ngb_narrow_down_hand_worked(name, right, left, radius, num, maxcmpt, want):
    hsml, r, l, close = R.ngb_narrow_down(right, left, [float(x) for x in radius], [float(x) for x in num], maxcmpt, 40, BOX)
    assert (r, l, close) == want[1:]
    assert hsml == pytest.approx(want[0], rel=1e-14)
