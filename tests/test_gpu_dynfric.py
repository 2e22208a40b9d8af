"""GPU tests of black-hole dynamical friction and the potential minimum (csrc/dynfric.hip) and of the three integrator kernels that consume
their results (csrc/timestep.hip) against the all-pairs restatement (tests/dynfric_restated.py): the entry points
mpg_dev_blackhole_dynfric, mpg_blackhole_dynfric and mpg_resident_sph_blackhole_dynfric, the latter inside a resident gas stretch in the
order of run.c.

Scenes (dynfric_restated.scene_a / scene_b).  A: 16^3 jittered gas + 16^3 dark matter + 512 stars + 40 black holes in a unit box with
distinct random potentials; among the black holes one with Hsml = 0.45 (thousands of neighbours: the search pauses and resumes), one at a
corner of the box (the wrap form), one whose Hsml holds nothing but itself (ZeroDF), one with active_dynfric = 0 and non-zero stale sums,
one swallowed, one garbage, one moving with its surroundings to 1e-3 of their dispersion (f_of_x cancels), one at five dispersions.
B: the clustered 12^3 set of ics.s_clust(12, seed=5) - the generator behind the golden set grav_sclust12 - in a unit box.

Conditions, asserted from the restatement before anything is compared: no candidate within 1e-9 relative of a target's Hsml; every gap
between the two lowest potentials inside a target's radius positive; no dynfric step within 1e-9 relative of a bin boundary.

Compared against the defined form (b).  EQUAL as integers: the queue (targets, listed), ZeroDF, the index of the minimum, JumpToMinPot,
the neighbour count per target and in total, tb_dynfric; ZeroDFMass to 8 eps.  BIT-IDENTICAL: MinPot, MinPotPos, MinPotVel (copies), every
row and array the call does not write (the stale sums of non-targets among them), the velocities after mpg_dev_apply_bh_subgrid_kick and
Pos / Vel after mpg_dev_reposition_blackholes against the numpy restatement.  The three raw sums of k terms within 4 (k + 8) eps sum|term|,
the project's bound for a reordered fp64 sum, one more k eps sum|term| against the literal form (a); the normalised velocity
and rms by first-order propagation of those bounds; DFAccel by first-order propagation through its formula plus an allowance TRANS for the
device's exp, log, sqrt and pow - relative to log lambda, and for f_of_x relative to the sum of the absolute values of its two terms (they
cancel to third order at small x).  No accuracy table of the device math library ships with this ROCm, so TRANS started at 1e-12 (as
DESIGN 3.11 did) and stays no tighter than ten times what a run on an MI355X showed (DESIGN 3.12 holds the ratios seen).  The largest
ratio to every bound is printed (pytest -s)."""
import math

import numpy as np
import pytest

import dynfric_restated as R
from blackhole_restated import default_times

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps
TRANS = 1e-12
_cache = {}


def scene(pkg, name, method, repos, ktype):
    """inputs and both forms of the restatement, computed once per case"""
    key = (name, method, repos, ktype)
    if key in _cache:
        return _cache[key]
    par = R.default_params(BH_DynFrictionMethod=method, BlackHoleRepositionEnabled=repos)
    if name == "A":
        d = R.scene_a(par, ktype)
        keep = np.ones(d["n"], bool)
        keep[[d["b0"] + 9, d["b0"] + 17, 5, 5000]] = False                  # an active sublist: two black holes are not listed
        active = np.nonzero(keep)[0].astype(np.int32)
    else:
        pos, _, box = pkg.ics.s_clust(12, seed=5)
        d = R.scene_b(pos / box, par, ktype)
        active = None
    T = default_times()
    out, info = R.dynfric(d, par, T, active=active)
    lit, linfo = R.dynfric(d, par, T, active=active, literal=True)
    _cache[key] = (d, par, T, active, out, info, lit)
    return _cache[key]


def conditions(info):
    m = info["margins"]
    assert m["hsml"] > 1e-9 and m["potgap"] > 0, m


def sph_times(pkg, T):
    t = pkg.engine.SphTimes()
    t.FgravkickB, t.atime, t.hubble = T["FgravkickB"], T["atime"], T["hubble"]
    for k in ("gravkicks", "hydrokicks", "dloga_bin"):
        for b in range(47):
            getattr(t, k)[b] = T[k][b]
    return t


def fresh_outputs(n):
    return {k: np.full((n, w) if w > 1 else n, float(R.SENTINEL)) for k, w in R.OUT.items()}


def new_engine(pkg, par, ktype):
    eng = pkg.Engine(0)
    eng.set_bh_dynfric_params(par["BH_DynFrictionMethod"], par["BH_DFBoostFactor"], par["BH_DFbmax"], par["BlackHoleRepositionEnabled"],
                              par["GravInternal"], ktype)
    return eng


def run_dev(pkg, torch, d, par, T, active, potential=None):
    eng = new_engine(pkg, par, d["ktype"])
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    a = {k: up(d[k]) for k in R.READ + R.IN_OUT}
    if potential is not None:
        a["potential"] = up(potential)
    a.update({k: up(v) for k, v in fresh_outputs(d["n"]).items()})
    pos, mass, typ = up(d["pos"]), up(d["mass"]), up(d["type"])
    eng.dev_bind_particles(pos, mass, d["box"], type=typ)
    try:
        eng.dev_blackhole_dynfric(a, sph_times(pkg, T), active=None if active is None else torch.from_numpy(active).cuda())
        eng.synchronize()
        got = {k: v.cpu().numpy() for k, v in a.items()}
        stats = eng.bh_dynfric_stats()
        got.update(eng.bh_dynfric_export(d["n"]) if stats["targets"] > 0 else {})
        got["tree"] = eng.tree_stats().NumParticles if stats["targets"] > 0 else None
        return got, stats
    finally:
        eng.close()


def dfaccel_bound(d, par, T, i, exp, det, drho, du, drms):
    """first-order propagation of the errors of the stored sums through blackhole_compute_dfaccel, plus TRANS for exp / log / sqrt / pow"""
    G, M, a = par["GravInternal"], float(d["mass"][i]), T["atime"]
    rho, rms, b = float(exp["df_density"][i]), float(exp["df_rmsvel"][i]), det["bhvel"]
    dv = np.abs(d["vel"][i] - exp["df_vel"][i])
    db = float((dv * du).sum()) / b + 2 * EPS * b
    dx = det["x"] * (db / b + drms / rms + 4 * EPS)
    L, lam = abs(det["loglambda"]), det["lam"]
    dL = (lam - 1) / lam * 2 * db / b + TRANS * L
    df = R.f_of_x_slope(det["x"]) * dx + TRANS * (abs(det["t1"]) + abs(det["t2"]))
    C = 4 * math.pi * G * G * M * a * par["BH_DFBoostFactor"] / b ** 3
    f = det["f"]
    return C * (drho * L * f * dv + rho * dL * f * dv + rho * L * df * dv + rho * L * f * du + rho * L * f * dv * 3 * db / b) + 16 * EPS * np.abs(exp["dfaccel"][i])


def compare(d, par, T, out, info, got, stats, label, lit=None):
    conditions(info)
    method, n = par["BH_DynFrictionMethod"], d["n"]
    worst = {}
    rat = lambda key, err, bound: worst.__setitem__(key, max(worst.get(key, 0.0), float(np.max(np.asarray(err) / (np.asarray(bound) + 1e-300)))))
    tl = info["targets"]
    # integers and copies
    assert stats["targets"] == len(tl) and stats["listed"] == len(info["listed"]) and stats["zerodf"] == info["zerodf"], (label, stats)
    assert stats["neighbours"] == info["neighbours"] and stats["candidates"] >= stats["neighbours"], (label, stats)
    assert abs(stats["zerodfmass"] - info["zerodfmass"]) <= 8 * EPS * info["zerodfmass"]
    if tl:
        assert got["tree"] == info["tree"], (label, got["tree"], info["tree"])
        exp_idx, exp_ngb = np.full(n, -1, np.int32), np.full(n, -1, np.int32)
        for i in tl:
            exp_idx[i], exp_ngb[i] = info["per"][i]["minidx"], info["per"][i]["numngb"]
        assert np.array_equal(got["minidx"], exp_idx), label
        assert np.array_equal(got["numngb"], exp_ngb), label
    for key in ("jumptominpot", "minpot", "minpotpos", "minpotvel"):
        assert np.array_equal(got[key], out[key]), (label, key)
    # what the call does not write is bit-identical
    for key in R.OUT:
        untouched = out[key] == R.SENTINEL
        assert np.array_equal(got[key][untouched], out[key][untouched]), (label, key)
    for key in R.IN_OUT:
        same = out[key] == d[key]
        assert np.array_equal(got[key][same], d[key][same]), (label, key)
    if method > 0:
        nontargets = np.setdiff1d(np.arange(n), np.array(tl, np.int64))
        for key in ("df_density", "df_vel", "df_rmsvel"):
            assert np.array_equal(got[key][nontargets], d[key][nontargets]), (label, key)
        for form, exp, extra in (("", out, 0),) + ((("(a) ", lit, 1),) if lit is not None else ()):
            errs = {}
            for i in tl:
                P = info["per"][i]
                kb = {name: (4 * (P["sums"][name][0] + 8) + extra * P["sums"][name][0]) * EPS * P["sums"][name][1] for name in R.SUMS}
                if not extra:                      # (form (a) keeps no raw sums of its own: its density IS one, compared below)
                    for s, name in enumerate(R.SUMS):
                        rat("raw " + name, abs(got["rawsums"][i][s] - P["raw"][s]), kb[name] + 1e-300)
                rho = float(exp["df_density"][i])
                rat(form + "df_density", abs(got["df_density"][i] - rho), kb["dens"] + 1e-300)
                if not rho > 0:
                    assert got["df_density"][i] == 0 and not got["df_vel"][i].any() and got["df_rmsvel"][i] == 0
                    errs[i] = (0.0, np.zeros(3), 0.0)
                    continue
                u, rms = exp["df_vel"][i], float(exp["df_rmsvel"][i])
                du = np.array([kb["v%d" % k] for k in range(3)]) / rho + np.abs(u) * (kb["dens"] / rho + 2 * EPS)
                drms = rms * (0.5 * (kb["rms"] / (rms * rms * rho) + kb["dens"] / rho) + 2 * EPS)
                rat(form + "df_vel", np.abs(got["df_vel"][i] - u), du)
                rat(form + "df_rmsvel", abs(got["df_rmsvel"][i] - rms), drms)
                errs[i] = (kb["dens"], du, drms)
            for i in info["listed"]:
                det = info["dfaccel"][i]
                if det is None or not det["bhvel"] > 0:
                    assert np.array_equal(got["dfaccel"][i], np.zeros(3)), (label, i)
                    continue
                drho, du, drms = errs.get(i, (0.0, np.zeros(3), 0.0))
                b = dfaccel_bound(d, par, T, i, exp, det, drho, du, drms)
                rat(form + "dfaccel", np.abs(got["dfaccel"][i] - exp["dfaccel"][i]), b)
                if i == d["b0"] + 4 and "bh" not in d:
                    rat(form + "dfaccel at small x", np.abs(got["dfaccel"][i] - exp["dfaccel"][i]), b)
    print("dynfric %s: %d targets of %d listed, %d neighbours of %d candidates, %d ZeroDF; largest ratio to the bound: %s; margins %s"
          % (label, len(tl), len(info["listed"]), stats["neighbours"], stats["candidates"], stats["zerodf"],
             ", ".join("%s %.3g" % kv for kv in sorted(worst.items())), ", ".join("%s %.1e" % kv for kv in info["margins"].items())))
    for key, v in worst.items():
        assert v <= 1, (label, key, v)
    return worst


CASES = [("A", 1, 0, 1), ("A", 2, 0, 1), ("A", 3, 0, 1), ("A", 3, 0, 2), ("A", 0, 1, 1), ("A", 2, 1, 2), ("B", 2, 0, 1), ("B", 3, 0, 2), ("B", 0, 1, 1)]


@pytest.mark.parametrize("name,method,repos,ktype", CASES, ids=["%s-method%d-repos%d-kernel%d" % c for c in CASES])
def test_dev_form(pkg, name, method, repos, ktype):
    """mpg_dev_blackhole_dynfric: methods 1, 2, 3 and method 0 with repositioning, the cubic and the quintic kernel, an active sublist (A)
    and the NULL list (B)"""
    import torch
    d, par, T, active, out, info, lit = scene(pkg, name, method, repos, ktype)
    got, stats = run_dev(pkg, torch, d, par, T, active)
    compare(d, par, T, out, info, got, stats, "dev / %s / method %d repos %d kernel %d" % (name, method, repos, ktype), lit=lit)
    if name == "A":
        b0 = d["b0"]
        assert b0 + 38 not in info["listed"] and b0 + 39 not in info["listed"] and b0 + 9 not in info["listed"]
        if method == 3 or repos:
            assert info["per"][b0]["numngb"] > 2000          # more than one leaf list of SPH_LCAP x 8 candidates
        if method > 0:
            assert info["zerodf"] >= 1 and b0 + 3 not in info["targets"] and b0 + 3 in info["listed"]
            assert info["dfaccel"][b0 + 4]["x"] < 0.01 and info["dfaccel"][b0 + 5]["x"] > 5


def test_tie_takes_the_smaller_index(pkg):
    """two equal lowest potentials inside a target's radius: the smaller particle index wins - the documented rule - whichever the tree
    visits first (the pair is tried in both index orders relative to the tree's order)"""
    import torch
    d, par, T, active, out, info, lit = scene(pkg, "A", 2, 1, 2)
    i = d["b0"] + 6
    dx = R.nearest(d["pos"][i] - d["pos"], d["box"])
    inside = np.nonzero(((dx * dx).sum(1) < d["hsml"][i] ** 2) & (d["type"] != 7))[0]
    inside = inside[inside != i]
    assert len(inside) >= 4
    for lo, hi in ((inside[0], inside[-1]), (inside[1], inside[-2])):
        pot = d["potential"].copy()
        pot[[lo, hi]] = -5.0
        got, stats = run_dev(pkg, torch, d, par, T, np.array([i], np.int32), potential=pot)
        assert got["minidx"][i] == min(lo, hi) and got["minpot"][i] == -5.0
        assert np.array_equal(got["minpotpos"][i], d["pos"][min(lo, hi)]) and got["jumptominpot"][i] == 1


def test_host_form(pkg):
    """mpg_blackhole_dynfric: the arrays travel; nothing of the records is written"""
    d, par, T, active, out, info, lit = scene(pkg, "A", 3, 0, 1)
    P = pkg.make_particles(d["pos"], d["mass"], type=d["type_table"])
    P["Flags"] = d["flags"]
    before = P.copy()
    eng = new_engine(pkg, par, d["ktype"])
    a = {k: d[k].copy() for k in R.READ + R.IN_OUT}
    a.update(fresh_outputs(d["n"]))
    eng.blackhole_dynfric(P, d["box"], a, sph_times(pkg, T), ActiveParticle=active)
    stats = eng.bh_dynfric_stats()
    got = dict(a, **eng.bh_dynfric_export(d["n"]))
    got["tree"] = eng.tree_stats().NumParticles
    eng.close()
    compare(d, par, T, out, info, got, stats, "host / A / method 3")
    assert np.array_equal(P, before)
    for k in R.READ:
        assert np.array_equal(a[k], d[k]), k


def test_nothing_to_do(pkg):
    """method 0 without repositioning, and a list without a black hole: nothing is read or written and no tree is built"""
    import torch
    d, par, T, active, out, info, lit = scene(pkg, "A", 2, 0, 1)
    nobh = np.nonzero(d["type"] != 5)[0].astype(np.int32)
    for p, act in ((dict(par, BH_DynFrictionMethod=0), None), (par, nobh)):
        got, stats = run_dev(pkg, torch, d, p, T, act)
        assert all(v == 0 for v in stats.values()) and got["tree"] is None
        for key, v in fresh_outputs(d["n"]).items():
            assert np.array_equal(got[key], v), key
        for key in R.IN_OUT:
            assert np.array_equal(got[key], d[key]), key
    # no tree was built: a call that needs one says so
    eng = new_engine(pkg, dict(par, BH_DynFrictionMethod=0), d["ktype"])
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    pos, mass, typ = up(d["pos"]), up(d["mass"]), up(d["type"])
    eng.dev_bind_particles(pos, mass, d["box"], type=typ)
    eng.dev_blackhole_dynfric({}, sph_times(pkg, T))
    with pytest.raises(pkg.EngineError, match="no tree"):
        eng.tree_stats()
    # the host form runs its queue pass before anything travels: arrays it would require are not even looked at
    P = pkg.make_particles(d["pos"], d["mass"], type=d["type_table"])
    P["Flags"] = d["flags"]
    eng.set_bh_dynfric_params(2, 2, 10.0, 0, 1.0, 1)
    eng.blackhole_dynfric(P, d["box"], {}, sph_times(pkg, T), ActiveParticle=nobh)
    assert all(v == 0 for v in eng.bh_dynfric_stats().values())
    eng.close()


def test_error_returns(pkg):
    """a call before the parameters; an unknown method; a missing array; a non-finite relative velocity (the reference's endrun(6))"""
    import torch
    d, par, T, active, out, info, lit = scene(pkg, "A", 2, 0, 1)
    eng = pkg.Engine(0)
    with pytest.raises(pkg.EngineError, match="BH_DynFrictionMethod"):
        eng.set_bh_dynfric_params(4)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    pos, mass, typ = up(d["pos"]), up(d["mass"]), up(d["type"])
    eng.dev_bind_particles(pos, mass, d["box"], type=typ)
    with pytest.raises(pkg.EngineError, match="mpg_set_bh_dynfric_params"):
        eng.dev_blackhole_dynfric({}, sph_times(pkg, T))
    eng.set_bh_dynfric_params(2, 2, 10.0, 0, 1.0, 1)
    with pytest.raises(pkg.EngineError, match="required"):
        eng.dev_blackhole_dynfric({}, sph_times(pkg, T))
    eng.close()
    bad = dict(d, vel=d["vel"].copy())
    bad["vel"][d["b0"] + 7, 1] = np.inf
    with pytest.raises(pkg.EngineError, match="not finite"):
        run_dev(pkg, torch, bad, par, T, active)


def test_subgrid_kick_dynfric_bins_and_reposition(pkg):
    """the three integrator kernels against their numpy restatements: the black holes' velocities after a half kick and
    mpg_dev_apply_bh_subgrid_kick BIT-IDENTICAL to do_hydro_kick's two additions; tb_dynfric and the message's figures EQUAL; Pos / Vel and
    the flags after mpg_dev_reposition_blackholes BIT-IDENTICAL; the signed 0.1 BoxSize test an error return"""
    import torch
    from oracle import hiergrav_oracle as H
    d, par, T, active, out, info, lit = scene(pkg, "A", 2, 1, 2)
    n, b0 = d["n"], d["b0"]
    rng = np.random.RandomState(9)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    eng = pkg.Engine(0)
    pos, mass, typ = up(d["pos"]), up(d["mass"]), up(d["type"])
    eng.dev_bind_particles(pos, mass, d["box"], type=typ)
    dfaccel = np.where((d["type"] == 5)[:, None], out["dfaccel"], 0.0)
    dragaccel = np.where((d["type"] == 5)[:, None], 0.1 * rng.standard_normal((n, 3)), 0.0)
    # ---- the kick: after the hydro half kick (which leaves type 5 alone)
    K = pkg.engine.KickFactors()
    for b in range(47):
        K.gravkick[b], K.hydrokick[b], K.dt_entr[b], K.bin_active[b] = 0.004 * (1 + b % 5), 0.003 * (1 + b % 7), 0.001 * b, 1
    K.atime, K.MaxGasVel = T["atime"], 1e30
    gk = np.array([K.gravkick[b] for b in range(47)])
    vel = up(d["vel"])
    flags, tbh = up(d["flags"]), up(d["tb_hydro"])
    act = up(active)
    entropy, dtent = up(np.ones(n)), up(np.zeros(n))
    eng.dev_apply_hydro_half_kick(vel, K, typ, up(d["hydroacc"]), entropy, dtent, active=act, flags=flags, tb_hydro=tbh)
    eng.synchronize()
    v_half = vel.cpu().numpy()
    assert np.array_equal(v_half[d["type"] != 0], d["vel"][d["type"] != 0])
    eng.dev_apply_bh_subgrid_kick(vel, K, typ, up(dfaccel), up(dragaccel), active=act, flags=flags, tb_hydro=tbh)
    eng.synchronize()
    v_exp = R.bh_subgrid_kick(v_half, d["type"], d["flags"], d["tb_hydro"], dfaccel, dragaccel, gk, active=active)
    assert np.array_equal(vel.cpu().numpy(), v_exp)
    moved = np.nonzero((v_exp != v_half).any(1))[0]
    assert set(moved) <= set(info["listed"]) and len(moved) >= 30
    # ---- the dynamic-friction bins, at two points of the timeline
    sync = np.log(np.array([0.1, 0.25, 0.5, 1.0]))
    tl = H.Timeline(sync)
    atime, hubble, courant, errtol = 0.37, 0.21, 0.15, 0.025
    for case, Ti_cur in enumerate(((1 << H.TIMEBINS), (1 << H.TIMEBINS) + (5 << 33))):
        tbg = rng.randint(30, 42, n).astype(np.uint8)
        tbhy = np.minimum(rng.randint(24, 42, n), tbg).astype(np.uint8)
        S = dict(type=d["type"], flags=d["flags"], vel=d["vel"] * 10 ** rng.uniform(-2, 2, (n, 1)), df_vel=out["df_vel"] * (d["type"] == 5)[:, None],
                 hsml=d["hsml"] * 10 ** rng.uniform(-4, 0, n), dthsml=np.where(rng.random_sample(n) < 0.5, 0.0, rng.standard_normal(n)),
                 tb_grav=tbg, tb_hydro=tbhy, tb_dynfric=rng.randint(26, 40, n).astype(np.uint8))
        times = dict(mintimebin=30, maxtimebin=41, mingravtimebin=31, Ti_Current=Ti_cur, PM_length=1 << 41, PM_start=Ti_cur - (1 << 41) * case, PM_kick=0,
                     Ti_kick=[0] * (H.TIMEBINS + 1))
        from test_gpu_hiergrav import to_struct
        dev = {k: up(v) for k, v in S.items()}
        before = S["tb_dynfric"].copy()
        res, margin = R.find_dynfric_timesteps(S, active if case else None, times, tl, errtol, 1e-7, courant, atime, hubble)
        assert margin > 1e-9, margin
        got = eng.dev_find_dynfric_timesteps(dev, act if case else None, to_struct(pkg, times), sync, errtol, 1e-7, courant, atime, hubble)
        eng.synchronize()
        assert np.array_equal(dev["tb_dynfric"].cpu().numpy(), S["tb_dynfric"]), case
        assert got == res and res["nbh"] >= 36 and res["maxdyndiff"] > 0, (got, res)
        ch = S["tb_dynfric"] != before
        assert ch.any() and not ch[d["type"] != 5].any()
        assert len(set(S["tb_dynfric"][ch] - tbhy[ch])) > 3 and (S["tb_dynfric"] <= tbg)[ch].all() and (S["tb_dynfric"] >= tbhy)[ch].all()
    # ---- the jump
    jump = out["jumptominpot"].copy()
    jump[b0 + 38] = 1                                                       # swallowed: stays where it is, keeps its flag
    mpp = np.where((out["minpotpos"] == R.SENTINEL), d["pos"], out["minpotpos"])
    mpv = np.where((out["minpotvel"] == R.SENTINEL), d["vel"], out["minpotvel"])
    far_ok = [i for i in info["targets"] if jump[i] and i != b0]
    assert len(far_ok) > 20
    for i in info["targets"]:                                              # keep every jump inside 0.1 box along every axis
        dx = R.nearest(d["pos"][i] - mpp[i], d["box"])
        if (np.abs(dx) > 0.1).any():
            jump[i] = 0
    p_exp, v_exp, j_exp, far = R.reposition(d["pos"], d["vel"], d["type"], d["flags"], jump, mpp, mpv, d["box"])
    assert not far and (p_exp != d["pos"]).any(1).sum() >= 8
    dp, dvv, dj = up(d["pos"]), up(d["vel"]), up(jump)
    eng.dev_reposition_blackholes(dp, dvv, typ, dj, up(mpp), up(mpv), d["box"], flags=flags)
    eng.synchronize()
    assert np.array_equal(dp.cpu().numpy(), p_exp) and np.array_equal(dvv.cpu().numpy(), v_exp) and np.array_equal(dj.cpu().numpy(), j_exp)
    assert j_exp[b0 + 38] == 1 and not j_exp[info["listed"]].any()
    # too far: Pos - MinPotPos = +0.3 box is an error and moves nothing; -0.3 passes the reference's signed test
    i = b0 + 10
    for sign, fails in ((+1, True), (-1, False)):
        mpp2 = d["pos"].copy()
        mpp2[i, 0] = d["pos"][i, 0] - sign * 0.3
        j2 = np.zeros(n, np.int32)
        j2[i] = 1
        dp, dvv, dj = up(d["pos"]), up(d["vel"]), up(j2)
        if fails:
            with pytest.raises(pkg.EngineError, match="very far"):
                eng.dev_reposition_blackholes(dp, dvv, typ, dj, up(mpp2), up(mpv), d["box"], flags=flags)
            assert np.array_equal(dp.cpu().numpy(), d["pos"])
        else:
            eng.dev_reposition_blackholes(dp, dvv, typ, dj, up(mpp2), up(mpv), d["box"], flags=flags)
            assert dp.cpu().numpy()[i, 0] == mpp2[i, 0]
    eng.close()


def test_resident_form_in_the_order_of_run_c(pkg):
    """a resident gas stretch in the order of run.c: density -> hydro_force -> find_vel_disp -> blackhole_dynfric -> blackhole -> cooling.
    The call reads the resident Vel, accelerations (HydroAccel: what hydro_force has just left), bins, Hsml and Potential, leaves the tree of
    its own mask (stars + black holes + dark matter + gas here) and changes nothing resident; mpg_resident_sph_blackhole then finds another
    tree than its own and builds the tree of gas and black holes again.  The entry state of the call is what the same stretch WITHOUT the
    call holds (the loops are deterministic)."""
    import test_gpu_blackhole as TB
    import test_gpu_cooling as TC
    d0, bpar, T, rnd, active, *_ = TB.scene(pkg, "zel")
    C0, _, step, _, _ = TC.reference("sherwood_z3")
    n, box = d0["n"], d0["box"]
    t = TB.sph_times(pkg, T)
    for k in ("drifts", "dloga_kick"):
        for b in range(47):
            getattr(t, k)[b] = 0.0
    rs = np.random.RandomState(6)
    potential = -(1.0 + rs.permutation(n)) / n
    par = R.default_params(BH_DynFrictionMethod=3)
    bh = d0["type_table"] == 5
    stale = dict(df_density=np.where(bh, 0.7, 0.0), df_vel=np.where(bh[:, None], 0.1 * rs.standard_normal((n, 3)), 0.0), df_rmsvel=np.where(bh, 0.5, 0.0),
                 jumptominpot=np.where(bh, 1, 0).astype(np.int32))
    adf = np.ones(n, np.uint8)
    adf[d0["b0"] + 5] = 0
    z = lambda *s: np.zeros(s)
    runs = []
    for with_call in (False, True):
        P = TB.host_table(pkg, d0)
        P["Vel"], P["Potential"] = d0["vel"], potential
        P["FullTreeGravAccel"], P["GravPM"] = d0["gacc"], d0["gpm"]
        eng = TB.new_engine(pkg, bpar, rnd)
        eng.set_gravshort_treepar()
        eng.gravshort_set_softenings(d0["soft"] / 2.8)
        eng.set_hydropar(0, 100.0, 0.75)
        eng.set_bh_dynfric_params(3, par["BH_DFBoostFactor"], par["BH_DFbmax"], 0, par["GravInternal"], pkg.engine.DENSITY_KERNEL_CUBIC_SPLINE)
        TC.configure(eng, C0)
        a = dict(hsml=d0["hsml"].copy(), dthsml=z(n), vel=d0["vel"].copy(), gacc=d0["gacc"].copy(), gpm=d0["gpm"].copy(), tb_hydro=d0["tb_hydro"].copy(),
                 tb_grav=d0["tb_grav"].copy(), entropy=d0["entropy"].copy(), density=z(n), egywtdensity=z(n), dhsmlegyfac=z(n), divvel=z(n), curlvel=z(n),
                 hydroacc_out=z(n, 3), dtentropy_out=z(n), maxsignalvel=z(n))
        eng.resident_begin(P, box)
        eng.resident_sph_begin(P, a)
        eng.density(P, box, a, t, update_hsml=0, BlackHoleOn=1)
        eng.hydro_force(P, a, t)
        vdisp = d0["vdisp"].copy()
        eng.resident_sph_find_vel_disp(P, t, T["atime"], T["hubble"], 0.0, 1e30, vdisp, ActiveParticle=active)
        assert eng.tree_stats().NumParticles == int((d0["type"] == 1).sum())
        m = TB.host_arrays(d0, skip=("vel", "gacc", "gpm", "hydroacc", "tb_hydro", "tb_grav", "hsml", "density", "entropy"))
        m["vdisp"] = vdisp
        df, stats, export = None, None, None
        if with_call:
            df = dict({k: v.copy() for k, v in stale.items()}, bh_mass=d0["bh_mass"].copy(), active_dynfric=adf, **fresh_outputs(n))
            eng.resident_sph_blackhole_dynfric(P, df, t, ActiveParticle=active)
            stats, export = eng.bh_dynfric_stats(), eng.bh_dynfric_export(n)
            ntree = eng.tree_stats().NumParticles
            assert ntree == int(np.isin(d0["type"], (0, 1, 4, 5)).sum()) and ntree > int(((d0["type"] == 0) | (d0["type"] == 5)).sum())
        eng.resident_sph_blackhole(P, m, t, ActiveParticle=active)
        assert eng.tree_stats().NumParticles == int(((d0["type"] == 0) | (d0["type"] == 5)).sum())       # its own tree, rebuilt
        bstats = eng.blackhole_stats()
        ne = np.ones(n)
        eng.resident_sph_cooling(P, t, step, ne, ActiveParticle=active)
        eng.resident_sph_end(a)
        eng.resident_end(P)
        runs.append((dict(a), m, P, df, stats, export, bstats))
        eng.close()
    a0 = runs[0][0]
    # the black-hole step saw the same state with and without the call in front of it
    assert runs[0][6] == runs[1][6] and runs[1][6]["gas_swallowed"] > 10
    for key in ("sph_swallowid", "bh_swallowid", "flags", "swallowid"):
        assert np.array_equal(runs[0][1][key], runs[1][1][key]), key
    entry = dict(d0, ktype=1, potential=potential, hydroacc=None, active_dynfric=adf, **stale)
    # HydroAccel at the call: the run without the black-hole step's kicks would be needed for the gas it kicked; the call reads it BEFORE
    # blackhole(), where it is hydro_force's output - which blackhole() does not change
    entry["hydroacc"] = a0["hydroacc_out"]
    out, info = R.dynfric(entry, par, T, active=active)
    assert len(info["targets"]) >= 30 and len(info["listed"]) == len(info["targets"]) + 1
    got = dict(runs[1][3], **runs[1][5])
    got["tree"] = info["tree"]
    compare(entry, par, T, out, info, got, runs[1][4], "resident / zel / method 3")
