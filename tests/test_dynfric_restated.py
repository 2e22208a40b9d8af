"""Closed forms of the dynamical-friction restatement (tests/dynfric_restated.py) that need no device: what the GPU tests compare against
is itself pinned here."""
import math

import numpy as np

import dynfric_restated as R
from blackhole_restated import default_times, velpred
from metals_restated import kernel_wk

EPS = np.finfo(np.float64).eps


def small_scene(method=1, nstar=1, r=0.03, h=0.1, v=None, ktype=1):
    """a black hole in the middle of a unit box and `nstar` stars at distance r from it (on a ring)"""
    ang = 2 * np.pi * np.arange(nstar) / max(nstar, 1)
    stars = 0.5 + r * np.stack([np.cos(ang), np.sin(ang), 0 * ang], 1)
    pos = np.concatenate([[[0.5, 0.5, 0.5]], stars])
    ptype = np.array([5] + [4] * nstar, np.uint8)
    d = R.make_scene(pos, ptype, 3, np.full(len(pos), h), ktype)
    if v is not None:            # a uniform velocity field: no accelerations, every star at v
        d["vel"][1:] = v
        d["gacc"][:], d["gpm"][:], d["hydroacc"][:] = 0, 0, 0
    d["potential"][:] = -np.arange(len(pos)) - 1.0        # every star lower than the black hole, the last the lowest
    return d, R.default_params(BH_DynFrictionMethod=method), default_times()


def test_one_star_at_known_distance():
    d, par, T = small_scene()
    out, info = R.dynfric(d, par, T)
    H, r = 0.1, float(np.linalg.norm(d["pos"][1] - d["pos"][0]))
    wk = float(kernel_wk(r / H, H, 1))
    assert out["df_density"][0] == float(d["mass"][1]) * wk
    vp = velpred(d, T, 1, False)
    assert np.allclose(out["df_vel"][0], vp, rtol=4 * EPS, atol=0)
    assert math.isclose(out["df_rmsvel"][0], math.sqrt(float((vp * vp).sum())), rel_tol=8 * EPS)
    assert info["per"][0]["numngb"] == 2 and info["per"][0]["minidx"] == 1 and info["targets"] == [0] and info["listed"] == [0]
    assert out["minpot"][0] == d["potential"][1] and np.array_equal(out["minpotpos"][0], d["pos"][1]) and np.array_equal(out["minpotvel"][0], d["vel"][1])
    assert out["jumptominpot"][0] == 0          # repositioning is off: the flag takes that value


def test_uniform_velocity_field():
    v = np.array([0.3, -0.2, 0.1])
    d, par, T = small_scene(nstar=12, v=v)
    out, info = R.dynfric(d, par, T)
    assert math.isclose(out["df_rmsvel"][0], float(np.linalg.norm(v)), rel_tol=32 * EPS)
    assert np.allclose(out["df_vel"][0], v, rtol=32 * EPS, atol=0)
    rel = d["vel"][0] - out["df_vel"][0]
    acc = out["dfaccel"][0]
    assert np.linalg.norm(acc) > 0
    cosine = float((acc * rel).sum()) / (np.linalg.norm(acc) * np.linalg.norm(rel))
    assert cosine < -1 + 1e-12                  # antiparallel to Vel - v
    det = info["dfaccel"][0]
    assert det["f"] == max(det["t1"] - det["t2"], 0.0) and det["lam"] > 1


def test_black_hole_at_rest_relative_to_its_surroundings_gives_exactly_zero():
    v = np.array([0.3, -0.2, 0.1])
    d, par, T = small_scene(nstar=1, v=v)
    out0, _ = R.dynfric(d, par, T)
    d["vel"][0] = out0["df_vel"][0]
    out, info = R.dynfric(d, par, T)
    assert info["dfaccel"][0]["bhvel"] == 0 and np.array_equal(out["dfaccel"][0], np.zeros(3))
    assert not np.signbit(out["dfaccel"][0]).any()


def test_no_lower_neighbour_keeps_position_and_flag():
    d, par, T = small_scene(nstar=3)
    d["potential"][0] = -100.0                   # the black hole is the minimum
    d["jumptominpot"][0] = 1
    par["BlackHoleRepositionEnabled"] = 0
    out, info = R.dynfric(d, par, T)
    assert info["per"][0]["minidx"] == -1
    assert out["minpot"][0] == -100.0 and np.array_equal(out["minpotpos"][0], d["pos"][0])
    assert np.all(out["minpotvel"][0] == R.SENTINEL) and out["jumptominpot"][0] == 1      # untouched
    # an equal potential is not strictly lower
    d["potential"][2] = -100.0
    out, info = R.dynfric(d, par, T)
    assert info["per"][0]["minidx"] == -1


def test_tie_takes_the_smaller_index_and_zero_density_is_counted():
    d, par, T = small_scene(nstar=4)
    d["potential"][[2, 4]] = -50.0
    out, info = R.dynfric(d, par, T)
    assert info["per"][0]["minidx"] == 2 and info["margins"]["potgap"] == 0
    d["type"][1:] = 1                            # dark matter only: method 1 sums nothing
    out, info = R.dynfric(d, par, T)
    assert info["zerodf"] == 1 and info["zerodfmass"] == d["bh_mass"][0] and out["df_density"][0] == 0
    assert np.array_equal(out["dfaccel"][0], np.zeros(3)) and info["dfaccel"][0] is None
    assert info["tree"] == 1                     # stars and black holes only


def test_forms_agree_within_the_sum_bound():
    par = R.default_params(BH_DynFrictionMethod=3)
    d = R.scene_a(par)
    T = default_times()
    b, ib = R.dynfric(d, par, T)
    a, ia = R.dynfric(d, par, T, literal=True)
    assert ib["targets"] == ia["targets"] and len(ib["targets"]) == 37
    worst = 0.0
    for i in ib["targets"]:
        assert ib["per"][i]["minidx"] == ia["per"][i]["minidx"] and ib["per"][i]["numngb"] == ia["per"][i]["numngb"]
        for s, name in enumerate(R.SUMS):
            k, ab = ib["per"][i]["sums"][name]
            err = abs(ib["per"][i]["raw"][s] - ia["per"][i]["raw"][s])
            assert err <= k * EPS * ab, (i, name, err, k * EPS * ab)
            worst = max(worst, err / (k * EPS * ab + 1e-300))
    assert 0 < worst <= 1
    b0 = d["b0"]
    assert ib["per"][b0]["numngb"] > 2000 and ib["zerodf"] >= 1 and b0 + 3 not in ib["targets"]
    assert ib["dfaccel"][b0 + 4]["x"] < 0.01 and ib["dfaccel"][b0 + 5]["x"] > 5
    assert np.array_equal(b["df_density"][b0 + 3], d["df_density"][b0 + 3]) and np.any(b["dfaccel"][b0 + 3] != 0)     # stale sums, fresh DFAccel


def test_f_of_x_slope_matches_a_difference_quotient():
    for x in (0.05, 0.4, 1.0, 2.5):
        h = 1e-6 * x
        num = ((lambda t: t[0] - t[1])(R.f_of_x_terms(x + h)) - (lambda t: t[0] - t[1])(R.f_of_x_terms(x - h))) / (2 * h)
        assert math.isclose(R.f_of_x_slope(x), abs(num), rel_tol=1e-5, abs_tol=1e-9)


def test_dynfric_bin_of_hand_picked_velocities():
    from oracle import hiergrav_oracle as H
    tl = H.Timeline(np.log([0.1, 1.0]))
    Ti = 5 << 40
    times = dict(Ti_Current=Ti, PM_length=1 << 43)
    logD = tl.dloga_interval_ti(Ti)
    atime, hubble, errtol = 0.5, 2.0, 0.025
    # relative speed 1, Hsml chosen so that dloga is 1.5 steps of bin 30: bin 30; ten times faster: three bins lower
    hs = 1.5 * (1 << 30) * logD / hubble / (2 * errtol * atime * atime)
    S = dict(type=np.array([5, 5, 5, 1], np.uint8), flags=np.zeros(4, np.uint8), vel=np.array([[1.0, 0, 0], [10.0, 0, 0], [1.0, 0, 0], [1.0, 0, 0]]),
             df_vel=np.zeros((4, 3)), hsml=np.full(4, hs), dthsml=np.zeros(4), tb_grav=np.array([40, 40, 28, 40], np.uint8),
             tb_hydro=np.array([20, 29, 20, 20], np.uint8), tb_dynfric=np.array([30, 30, 30, 9], np.uint8))
    res, margin = R.find_dynfric_timesteps(S, None, times, tl, errtol, 1e-9, 0.15, atime, hubble)
    assert list(S["tb_dynfric"]) == [30, 29, 28, 9]      # the bin; clamped up to the hydro bin (27 -> 29); clamped down to the gravity bin; no black hole
    assert res == dict(dynratio=10 + 0 + 8, maxdyndiff=10, nbh=3) and margin > 0.15    # (0.15 x 2^30 = 1.2 x 2^27: a sixth above its bin)
    # the total velocity counts when it exceeds the relative one
    assert R.dynfric_dloga([3.0, 0, 0], [2.5, 0, 0], hs, 0.0, atime, hubble, errtol, 0.15) == R.dynfric_dloga([3.0, 0, 0], [0, 0, 0], hs, 0.0, atime, hubble, errtol, 0.15)


def test_reposition_and_kick():
    rng = np.random.RandomState(2)
    n = 6
    pos, vel = rng.random_sample((n, 3)), rng.standard_normal((n, 3))
    ptype = np.array([5, 5, 5, 0, 5, 5], np.uint8)
    flags = np.array([0, 0, 2, 0, 0, 0], np.uint8)
    jump = np.array([1, 0, 1, 1, 1, 1], np.int32)
    mpp, mpv = pos + 0.01, vel + 1.0
    mpp[4] = pos[4] - 0.3                         # Pos - MinPotPos = +0.3 box: too far
    mpp[5, 0] = pos[5, 0] + 0.3                   # -0.3: the reference's signed test lets it pass
    p, v, j, far = R.reposition(pos, vel, ptype, flags, jump, mpp, mpv, 1.0)
    assert far == [4]
    assert np.array_equal(p[0], mpp[0]) and np.array_equal(v[0], mpv[0]) and np.array_equal(p[5], mpp[5])
    for i in (1, 2, 3, 4):
        assert np.array_equal(p[i], pos[i]) and np.array_equal(v[i], vel[i])
    assert list(j) == [0, 0, 1, 1, 1, 0]        # cleared for live black holes; swallowed, gas and the refused one keep theirs
    gk = 0.01 * (1 + np.arange(47))
    tb = np.array([3, 4, 5, 6, 7, 8], np.uint8)
    df, dr = rng.standard_normal((n, 3)), rng.standard_normal((n, 3))
    k = R.bh_subgrid_kick(vel, ptype, flags, tb, df, dr, gk, active=[0, 2, 3, 4])
    assert np.array_equal(k[0], (vel[0] + df[0] * gk[3]) + dr[0] * gk[3]) and np.array_equal(k[4], (vel[4] + df[4] * gk[7]) + dr[4] * gk[7])
    for i in (1, 2, 3, 5):
        assert np.array_equal(k[i], vel[i])
