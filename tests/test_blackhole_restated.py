"""CPU tests of the restated black-hole step (tests/blackhole_restated.py): the literal sequential form (a) equals the defined form (b) within
the rounding of (a)'s running sums on the scenes of the GPU tests; closed forms (Bondi rate with and without the Eddington cap, the three
merger examples of the reference's comment, the Mtrack rule in its three regimes, the energy cap, conservation of mass and momentum through
swallowing); and the conditions of the GPU tests hold on every scene and parameter set they use, with no target left out."""
import math

import numpy as np
import pytest

import blackhole_restated as R
import test_gpu_blackhole as G

EPS = R.EPS


def tiny(pos, typ, box=8.0, hsml=1.0, ktype=1, **cols):
    """a table of a few rows with quiet defaults; cols override"""
    n = len(pos)
    z = lambda *s: np.zeros(s)
    d = dict(pos=np.array(pos, np.float64), type=np.array(typ, np.uint8), box=box, n=n, ktype=ktype, id=(10 + 10 * np.arange(n)).astype(np.uint64),
             mass=np.ones(n, np.float32), hsml=np.full(n, float(hsml)), vel=z(n, 3), gacc=z(n, 3), gpm=z(n, 3), hydroacc=z(n, 3), dfaccel=z(n, 3),
             tb_hydro=np.full(n, 20, np.uint8), tb_grav=np.full(n, 20, np.uint8), entropy=np.ones(n), density=np.ones(n), delaytime=z(n), vdisp=z(n),
             active_hydro=np.ones(n, np.uint8), flags=np.zeros(n, np.uint8), bh_mass=np.ones(n), mtrack=np.full(n, 10.0), kineticfdbkenergy=z(n),
             countprogs=np.ones(n, np.int32))
    for k, v in cols.items():
        d[k] = np.array(v, d[k].dtype) if not np.isscalar(v) else np.full(n, v, d[k].dtype)
    return d


def test_literal_form_equals_defined_form(pkg):
    for name in ("zel", "clust"):
        d, par, T, rnd, active, out, info, lit = G.scene(pkg, name)
        G.conditions(info)
        for key in ("bh_swallowid", "sph_swallowid", "flags", "encounter", "mintimebin", "countprogs", "keflag", "bhheated", "swallowid", "mass"):
            assert np.array_equal(out[key], lit[key]), key
        kmax = max(max(v[0] for v in S.values() if isinstance(v, tuple)) for S in info["sums"].values())
        for key in ("feedbackweightsum", "mgasenc", "accreted_mass", "accreted_bhmass", "mtrack", "entropy", "bh_mass"):
            assert np.allclose(out[key], lit[key], rtol=kmax * EPS, atol=0), key
        for i in info["targets"]:
            S = info["sums"][i]
            if S["density"] > 0:
                assert abs(out["bh_entropy"][i] - lit["bh_entropy"][i]) <= S["ent"][0] * EPS * S["ent"][1] / S["density"]
                for k in range(3):
                    assert abs(out["gasvel"][i][k] - lit["gasvel"][i][k]) <= S["gv%d" % k][0] * EPS * S["gv%d" % k][1] / S["density"]
        for j, e in info["kicks"].items():
            # (the kick's size carries the rounding of the target's sums: KineticFdbkEnergy through Mdot)
            assert (np.abs(out["vel"][j] - lit["vel"][j]) <= (kmax + e["k"] + 1) * EPS * (e["abs"] + np.abs(d["vel"][j]))).all()


@pytest.mark.parametrize("over", [{}, dict(BlackHoleFeedbackMethod=R.FB_SPLINE), dict(BlackHoleFeedbackMethod=R.FB_MASS), dict(BlackHoleFeedbackMethod=0),
                                  dict(BlackHoleKineticOn=0), dict(SeedBHDynMass=0.0), dict(BH_DRAG=2, MergeGravBound=0), dict(BH_DRAG=0, WindDecouple=0)])
def test_conditions_hold_on_every_scene_of_the_gpu_tests(pkg, over):
    for name in ("zel", "clust") if not over else ("zel",):
        *_, info, lit = G.scene(pkg, name, **over)
        G.conditions(info)


def test_scenes_reach_what_they_are_for(pkg):
    """from the restatement alone: every scene of the GPU tests holds what it was built for"""
    for name in ("zel", "clust"):
        d, par, T, rnd, active, out, info, lit = G.scene(pkg, name)
        G.conditions(info)
        b0, tl, st = d["b0"], np.array(info["targets"]), info["stats"]
        assert len(tl) >= 35 and 0 < len(info["feedback_targets"]) < len(tl)
        assert st["gas_swallowed"] >= 30 and st["bh_swallowed"] >= 5
        sw = {j - b0: v for j, v in info["swal"].items() if d["type"][j] == 5}
        assert not (4 in sw or 5 in sw or 6 in sw or 7 in sw) and (0 in sw or 1 in sw) and (2 in sw or 3 in sw)    # unbound / bound pairs
        assert out["encounter"][b0 + 4] == 1 and out["encounter"][b0 + 6] == 1
        assert (20 in sw) != (21 in sw)                                                    # found only through the larger Hsml of the two
        capped = out["mdot"][tl] == par["BlackHoleEddingtonFactor"] * G.C_medd(par, T) * d["bh_mass"][tl]
        assert 3 <= capped.sum() <= len(tl) - 3
        assert all((out["keflag"][tl] == k).sum() >= 1 for k in (0, 2)) and (out["keflag"][tl] >= 1).sum() >= 3
        assert sum(e["capped"] for e in info["energy"].values()) >= 5 and max(e["k"] for e in info["energy"].values()) >= 2
        assert len(info["kicks"]) >= 50 and (out["bhheated"] == 1).sum() >= 20 and (out["bhheated"] == 1).sum() < len(info["energy"])
        assert (d["delaytime"] > 0).sum() >= 50 and (d["type"] == 7).sum() >= 10 and (d["type"] == 4).sum() >= 10
        ft = np.array(info["feedback_targets"])
        acc = out["accreted_mass"][ft] > 0
        assert (out["mtrack"][ft][acc] == par["SeedBHDynMass"]).any() and (out["mtrack"][ft][acc] < par["SeedBHDynMass"]).any()   # the Mtrack rule
        h, p = d["hsml"][tl], d["pos"][tl]
        assert ((p < h[:, None]) | (p > d["box"] - h[:, None])).all(1).any()               # the black hole in the corner
        if name == "clust":
            k_all = info["sums"][b0 + 19]["fws"][0]
            assert k_all > 0.95 * (d["type"] == 0).sum() > 120 * 8                         # pause and resume of the leaf list
            assert (b0 + 16) in info["swal"] and (b0 + 17) in info["swal"]                 # an inactive target and its neighbour mark each other
        else:
            assert set(d["inactive"].tolist()).isdisjoint(tl.tolist())
            # black holes 32-37 are the last wave of the queue: no periodic wrap (ngb_walk.h, interior_wave)
            live = (d["type"] == 0) | (d["type"] == 5)
            root_hmax = (np.abs(d["pos"][live] - d["box"] / 2) + d["hsml"][live, None] - d["box"] / 2).max()
            w = np.arange(b0 + 32, b0 + 38)
            face = np.maximum(d["hsml"][w], root_hmax) + 0.002 * d["box"]
            assert face.max() < 0.25 * d["box"] and (d["pos"][w] > face[:, None]).all() and (d["pos"][w] < d["box"] - face[:, None]).all()
            assert list(tl[-6:]) == list(w)


def uniform_gas(m=6, box=8.0):
    g = (np.arange(m) + 0.5) * box / m
    return np.array(np.meshgrid(g, g, g, indexing="ij")).reshape(3, -1).T


@pytest.mark.parametrize("alpha,capped", [(1e-3, False), (1e3, True)])
def test_lone_black_hole_in_uniform_gas_gives_the_bondi_rate(alpha, capped):
    pg = uniform_gas()
    pos = np.concatenate([pg, [[4.1, 3.9, 4.05]]])
    n = len(pos)
    A, vg, vb, Mbh = 1.7, np.array([0.2, -0.1, 0.05]), np.array([0.5, 0.3, -0.2]), 0.8
    d = tiny(pos, [0] * (n - 1) + [5], hsml=2.5, entropy=A)
    d["vel"][:] = vg
    d["vel"][-1] = vb
    d["bh_mass"][-1] = Mbh
    d["density"][-1] = rho = R.bh_density(d, n - 1)
    par, T = R.default_params(BlackHoleAccretionFactor=alpha, ForceSoftening=0.1, BlackHoleKineticOn=0), R.default_times()
    for b in range(47):
        T["gravkicks"][b] = T["hydrokicks"][b] = 0
    out, info = R.blackhole(d, par, T, R.random_table(1))
    a = T["atime"]
    cs2 = R.GAMMA * A * rho ** R.GAMMA_MINUS1 * a ** (-3 * R.GAMMA_MINUS1)
    v2 = float(((vb - vg) ** 2).sum()) / a ** 2
    bondi = 4 * math.pi * alpha * par["GravInternal"] ** 2 * Mbh ** 2 * rho / a ** 3 / (cs2 + v2) ** 1.5
    edd = par["BlackHoleEddingtonFactor"] * R.constants(par, T)["medd_fac"] * Mbh
    assert (bondi > edd) == capped
    assert math.isclose(out["mdot"][-1], edd if capped else bondi, rel_tol=1e-12)
    assert math.isclose(out["bh_entropy"][-1], A, rel_tol=1e-13) and np.allclose(out["gasvel"][-1], vg, rtol=1e-13)
    dt = T["dloga_bin"][20] / T["hubble"]
    assert math.isclose(out["bh_mass"][-1], Mbh + out["mdot"][-1] * dt, rel_tol=1e-15)
    assert np.allclose(out["dragaccel"][-1], -(vb - vg) * out["mdot"][-1] / 1.0 * a, rtol=1e-12)


@pytest.mark.parametrize("ids,expect", [((10, 20, 30), {1: 2}), ((10, 30, 20), {0: 1, 2: 1}), ((20, 10, 30), {1: 2}), ((30, 10, 20), {1: 0})])
def test_merger_examples(ids, expect):
    """black holes A, B, C in a row, A-B and B-C closer than the merger distance, A-C not (the three examples of the reference's comment;
    the third twice, once for each of A and C as the larger): who is swallowed by whom, who keeps an encounter, whose mass goes where"""
    md = 0.1
    pos = [[4.0, 4, 4], [4.07, 4, 4], [4.14, 4, 4]]
    d = tiny(pos, [5, 5, 5], hsml=0.5, id=ids, bh_mass=[1.0, 2.0, 4.0], countprogs=[1, 2, 4])
    par = R.default_params(ForceSoftening=md * 1.4, MergeGravBound=0, SeedBHDynMass=0.0, BlackHoleKineticOn=0)
    for literal in (False, True):
        out, info = R.blackhole(d, par, R.default_times(), R.random_table(1), literal=literal)
        got = {j: [i for i in range(3) if d["id"][i] == out["swallowid"][j]][0] for j in range(3) if out["flags"][j] == 2}
        assert got == expect
        for j, i in expect.items():
            assert out["flags"][j] == 2 and out["swallowid"][j] == d["id"][i] and out["encounter"][j] == 0
        for i in set(range(3)) - set(expect):
            eaten = [j for j, w in expect.items() if w == i]
            assert out["bh_mass"][i] == d["bh_mass"][i] + sum(d["bh_mass"][j] for j in eaten)
            assert out["countprogs"][i] == d["countprogs"][i] + sum(d["countprogs"][j] for j in eaten)
            assert out["mass"][i] == 1 + len(eaten) and out["flags"][i] == 0
        if ids == (10, 20, 30):        # example 1: A is not swallowed by B, which is itself swallowed; A keeps its encounter
            assert out["encounter"][0] == 1 and out["flags"][0] == 0 and info["feedback_targets"] == [2] and 0 in info["swal"]


@pytest.mark.parametrize("mtrack,seed,newtrack,newmass", [(0.5, 3.0, 1.75, 1.0), (2.5, 3.0, 3.0, 3.75), (3.0, 3.0, 3.0, 2.25), (0.5, 0.0, 0.5, 2.25)])
def test_mtrack_rule(mtrack, seed, newtrack, newmass):
    """a black hole that swallows one gas particle of mass 1.25: still in the seed regime, crossing the seed's dynamic mass, a regular black
    hole, and without a seed mass"""
    d = tiny([[4.0, 4, 4], [4.2, 4, 4]], [5, 0], hsml=1.0, mass=[1.0, 1.25], bh_mass=[1e6, 0], mtrack=[mtrack, 0])
    par = R.default_params(ForceSoftening=0.1, SeedBHDynMass=seed, BlackHoleKineticOn=0)
    out, info = R.blackhole(d, par, R.default_times(), np.full(7, 1e-9))
    assert info["stats"]["gas_swallowed"] == 1 and out["flags"][1] == 1 and out["accreted_mass"][0] == 1.25
    assert out["mtrack"][0] == newtrack and out["mass"][0] == np.float32(newmass)


def test_energy_cap():
    """gas that the feedback would lift over 5e8 K ends exactly on the cap, in both forms; gas already above it is brought down to it"""
    pg = uniform_gas(4)
    pos = np.concatenate([pg, [[4.1, 3.9, 4.05], [4.3, 4.2, 3.8]]])
    n = len(pos)
    d = tiny(pos, [0] * (n - 2) + [5, 5], hsml=3.0)
    par, T = R.default_params(ForceSoftening=0.01, BlackHoleKineticOn=0, BlackHoleFeedbackFactor=3.5), R.default_times()
    d["density"][-2:] = [R.bh_density(d, n - 2), R.bh_density(d, n - 1)]
    R.heat_near_cap(d, par, T, range(0, n - 2, 2), frac=0.999)
    R.heat_near_cap(d, par, T, [22], frac=1.5)
    C = R.constants(par, T)
    for literal in (False, True):
        out, info = R.blackhole(d, par, T, R.random_table(1), literal=literal)
        enttou = np.array([info["energy"][j]["enttou"] for j in sorted(info["energy"])])
        u = out["entropy"][sorted(info["energy"])] * enttou
        capped = np.array([info["energy"][j]["capped"] for j in sorted(info["energy"])])
        assert capped.sum() >= 3 and (~capped).sum() >= 3 and max(e["k"] for e in info["energy"].values()) == 2 and info["energy"][22]["capped"]
        assert np.allclose(u[capped], C["ucap"], rtol=4 * EPS, atol=0) and (u[~capped] < C["ucap"]).all()
        assert (out["entropy"][sorted(info["energy"])][~capped] > d["entropy"][sorted(info["energy"])][~capped]).all()


def test_mass_and_momentum_are_conserved_through_swallowing(pkg):
    """without a seed mass and with velocities predicted at the kick time, the mass and the momentum of gas and black holes that are not
    garbage or swallowed are the same before and after, to the float rounding of P.Mass"""
    d, par, T, rnd, active, *_ = G.scene(pkg, "zel")
    par = dict(par, SeedBHDynMass=0.0, BlackHoleKineticOn=0)
    T = dict(T, FgravkickB=0.0, gravkicks=np.zeros(47), hydrokicks=np.zeros(47))
    out, info = R.blackhole(d, par, T, rnd, active=active)
    assert info["stats"]["gas_swallowed"] > 30 and info["stats"]["bh_swallowed"] > 3
    live0 = (d["type"] == 0) | (d["type"] == 5)
    live1 = live0 & ((out["flags"] & 3) == 0)
    m0, m1 = d["mass"][live0].astype(np.float64), out["mass"][live1].astype(np.float64)
    f32 = float(np.finfo(np.float32).eps)
    assert abs(m0.sum() - m1.sum()) <= 2 * f32 * m1[np.isin(np.nonzero(live1)[0], info["feedback_targets"])].sum()
    p0, p1 = (m0[:, None] * d["vel"][live0]).sum(0), (m1[:, None] * out["vel"][live1]).sum(0)
    scale = np.abs(m1[:, None] * out["vel"][live1])[np.isin(np.nonzero(live1)[0], info["feedback_targets"])].sum(0)
    assert (np.abs(p0 - p1) <= 2 * f32 * scale + 1e-12 * np.abs(m0[:, None] * d["vel"][live0]).sum(0)).all()
