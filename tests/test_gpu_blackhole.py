"""GPU tests of the black-hole step (csrc/blackhole.hip) against the all-pairs restatement (tests/blackhole_restated.py): the entry points
mpg_dev_blackhole, mpg_blackhole and mpg_resident_sph_blackhole, the latter inside a resident gas stretch in the order of run.c.

Scenes: the 16^3 gas of ics.hydro_pair(16) and the clustered 4096-gas set of ics.s_clust(16), both scaled to a box of 8, each with 40 black
holes among the gas (blackhole_restated.sample_scene: bound and unbound pairs and chains of three inside the merger distance, inactive ones
next to active ones, one in a corner of the box, one whose Hsml holds all the gas (clustered set), a pair with Hsml 50 : 1, heavy accretors
that swallow tens of gas particles, a wave of central targets that needs no periodic wrap (16^3 set)), decoupled wind gas, garbage and
swallowed rows, stars and dark matter in the table, every ninth gas particle within 5e-4 of the 5e8 K cap.

Conditions, asserted from the restatement before anything is compared: no particle within 1e-10 relative of a symmetric radius or of a
target's Hsml, no pair within 1e-10 of the merger distance, |PE + KE| > 1e-9 (|PE| + KE), |w - p| > 1e-9, no two candidate swallowers of
one black hole with consecutive IDs, every branch (Eddington cap, the kinetic thresholds, the efficiency cap, the Mtrack rule, the energy
cap) at least 1e-9 relative from its branch point.

Compared, against the defined form (b): integers EQUAL (both swallow-ID arrays, flags, encounter, minTimeBin, CountProgs, KEflag, BHHeated,
SwallowID, the counters); sums of k terms within 4 (k + 8) eps sum|term| (FeedbackWeightSum, BH_Entropy, GasVel, MgasEnc, accreted mass,
BHP.Mass and momentum, energy per gas particle, kicks); P.Mass within 1 float ulp; rows the call does not write bit-identical; the scalars
behind pow / sqrt / acos / sin / cos (Mdot, BHP.Mass, DragAccel, KineticFdbkEnergy, the new entropy, the kicks) within the bound
propagated from their sums plus TRANS relative for the transcendentals.  No accuracy table of the device math library ships with the ROCm
installation this was written on (no document on the math functions under its tree), so the issue's fallback holds: the
allowance started from the 1e-12 the metal-return tests make for the device pow and was tightened to ten times what a run on an MI355X
showed - 1e-14 for the scalars behind pow and sqrt (seen: 1e-15 on Mdot, 4e-16 on the entropy); the kick keeps TRANS_DIR = 1e-12, six
times the 1.5e-13 seen, of the sum of absolute terms: acos(2 w - 1) loses digits towards the poles and a component sin(theta) cos(phi)
can be small against that loss.  Against the literal form (a): the same with one more k eps sum|term| for (a)'s own running sums,
P.Mass within (k + 2) 2^-23.  The largest ratio to every bound is printed (pytest -s)."""
import numpy as np
import pytest

import blackhole_restated as R

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps
TRANS = 1e-14
TRANS_DIR = 1e-12
ETA = 1.0
_cache = {}
ARRAY_IN = ("id", "gacc", "gpm", "hydroacc", "tb_hydro", "tb_grav", "hsml", "density", "delaytime", "dfaccel", "vdisp", "active_hydro")


def scene(pkg, name, **over):
    """inputs and both forms of the restatement, computed once per (scene, parameter set)"""
    key = (name, tuple(sorted(over.items())))
    if key in _cache:
        return _cache[key]
    if name == "zel":
        pos, _, typ, box = pkg.ics.hydro_pair(16)
        pg, seed = pos[typ == 0] * (8.0 / box), 5
    else:
        pg, _, box = pkg.ics.s_clust(16, seed=3)
        pg, seed = pg * (8.0 / box), 8
    box = 8.0
    soft = 0.028 * box
    d = R.sample_scene(pg, box, seed, soft, allgas=(name == "clust"))
    par = R.default_params(ForceSoftening=soft, **over)
    T, rnd = R.default_times(), R.random_table(11)
    R.heat_near_cap(d, par, T, np.arange(0, d["ng"], 9))
    # zel: an active sublist without the inactive black holes and a few more; clust: every row (two black holes then mark each other)
    active = None
    if name == "zel":
        keep = np.ones(d["n"], bool)
        keep[d["inactive"]] = False
        keep[d["b0"] + 30] = False
        active = np.nonzero(keep)[0].astype(np.int32)
    out, info = R.blackhole(d, par, T, rnd, active=active)
    lit, linfo = R.blackhole(d, par, T, rnd, active=active, literal=True)
    _cache[key] = (d, par, T, rnd, active, out, info, lit)
    return _cache[key]


def conditions(info):
    m = info["margins"]
    assert m["hsml"] > 1e-10 and m["merge"] > 1e-10, m
    assert m["bound"] > 1e-9 and m["swallow"] > 1e-9 and m["branch"] > 1e-9 and m["cap"] > 1e-9, m
    assert not info["consecutive"]


def sph_times(pkg, T):
    t = pkg.engine.SphTimes()
    t.FgravkickB, t.atime, t.hubble = T["FgravkickB"], T["atime"], T["hubble"]
    for k in ("gravkicks", "hydrokicks", "dloga_bin"):
        for b in range(47):
            getattr(t, k)[b] = T[k][b]
    return t


def fresh_outputs(n):
    return {k: np.full((n, w) if w > 1 else n, R.SENTINEL, dt) for k, (dt, w) in R.OUT.items()}


def compare(d, par, T, out, info, got, stats, label, lit=None):
    """got: dict of every in / out column and output after the call (numpy, particle order)"""
    conditions(info)
    n, tl, ftl = d["n"], np.array(info["targets"]), np.array(info["feedback_targets"])
    C = R.constants(par, T)
    worst = {}
    rat = lambda key, err, bound: worst.__setitem__(key, max(worst.get(key, 0.0), float(np.max(np.asarray(err) / (np.asarray(bound) + 1e-300)))))
    for form, exp, extra in (("", out, 0),) + ((("(a) ", lit, 1),) if lit is not None else ()):
        # integers
        for key in ("bh_swallowid", "sph_swallowid", "flags", "encounter", "mintimebin", "countprogs", "keflag", "bhheated", "swallowid"):
            assert np.array_equal(got[key], exp[key]), (label, form, key)
        assert np.array_equal(got["swallowtime"], exp["swallowtime"])
        for i in tl:
            S = info["sums"][int(i)]
            kb = lambda name: (4 * (S[name][0] + 8) + extra * S[name][0]) * EPS * S[name][1]
            rho = S["density"]
            rat(form + "fws", abs(got["feedbackweightsum"][i] - exp["feedbackweightsum"][i]), kb("fws"))
            rat(form + "mgasenc", abs(got["mgasenc"][i] - exp["mgasenc"][i]), kb("mgas"))
            if not rho > 0:
                assert got["mdot"][i] == 0 and np.allclose(got["dragaccel"][i], exp["dragaccel"][i], rtol=8 * EPS, atol=0)   # (no sum enters)
                continue
            dent = kb("ent") / rho + 2 * EPS * abs(exp["bh_entropy"][i])
            dgv = np.array([kb("gv%d" % k) for k in range(3)]) / rho + 2 * EPS * np.abs(exp["gasvel"][i])
            rat(form + "bh_entropy", abs(got["bh_entropy"][i] - exp["bh_entropy"][i]), dent)
            rat(form + "gasvel", np.abs(got["gasvel"][i] - exp["gasvel"][i]), dgv)
            # Mdot = const M^2 rho / (cs^2 + v^2)^1.5: first-order propagation of the two sums, plus TRANS for pow / sqrt
            dv = d["vel"][i] - exp["gasvel"][i]
            v2 = float((dv * dv).sum()) / T["atime"] ** 2
            cs2 = R.GAMMA * exp["bh_entropy"][i] * rho ** R.GAMMA_MINUS1 * T["atime"] ** (-3 * R.GAMMA_MINUS1)
            rel_mdot = 1.5 * (cs2 * dent / exp["bh_entropy"][i] + 2 * float((np.abs(dv) * dgv).sum()) / T["atime"] ** 2) / (cs2 + v2) + TRANS
            rat(form + "mdot", abs(got["mdot"][i] - exp["mdot"][i]), rel_mdot * exp["mdot"][i])
            dt = T["dloga_bin"][d["tb_hydro"][i]] / T["hubble"]
            dacc = (4 * (S["bhmass"][0] + 8) + extra * S["bhmass"][0]) * EPS * S["bhmass"][1] if "bhmass" in S else 0.0
            rat(form + "bh_mass", abs(got["bh_mass"][i] - exp["bh_mass"][i]), rel_mdot * exp["mdot"][i] * dt + 4 * EPS * exp["bh_mass"][i] + dacc)
            fac = np.abs(exp["dragaccel"][i]) / (np.abs(dv) + 1e-300)
            rat(form + "dragaccel", np.abs(got["dragaccel"][i] - exp["dragaccel"][i]), fac * dgv + np.abs(exp["dragaccel"][i]) * (rel_mdot + 4 * EPS))
            rat(form + "kineticfdbkenergy", abs(got["kineticfdbkenergy"][i] - exp["kineticfdbkenergy"][i]),
                (rel_mdot + TRANS) * max(exp["kineticfdbkenergy"][i], d["kineticfdbkenergy"][i]) + 1e-300)
        for i in ftl:
            S = info["sums"][int(i)]
            kb = lambda name: (4 * (S[name][0] + 8) + extra * S[name][0]) * EPS * S[name][1]
            rat(form + "accreted_mass", abs(got["accreted_mass"][i] - exp["accreted_mass"][i]), kb("mass") + 1e-300)
            rat(form + "accreted_bhmass", abs(got["accreted_bhmass"][i] - exp["accreted_bhmass"][i]), kb("bhmass") + 1e-300)
            dmom = np.array([kb("mom%d" % k) for k in range(3)])
            rat(form + "accreted_momentum", np.abs(got["accreted_momentum"][i] - exp["accreted_momentum"][i]), dmom + 1e-300)
            if exp["accreted_mass"][i] > 0:
                Mn = float(d["mass"][i]) + exp["accreted_mass"][i]
                rat(form + "vel of the swallower", np.abs(got["vel"][i] - exp["vel"][i]),
                    dmom / Mn + (8 * EPS + kb("mass") / Mn) * (np.abs(exp["vel"][i]) + np.abs(d["vel"][i])))
                k = S["mass"][0]
                m_got, m_exp = float(got["mass"][i]), float(exp["mass"][i])
                if extra:
                    rat(form + "P.Mass", abs(m_got - m_exp), (k + 2) * 2.0 ** -23 * m_exp)
                else:
                    rat("P.Mass ulp", abs(m_got - m_exp), float(np.spacing(np.float32(m_exp))))
                rat(form + "mtrack", abs(got["mtrack"][i] - exp["mtrack"][i]), kb("mass") + 4 * EPS * exp["mtrack"][i])
        for j, e in info["energy"].items():
            # entropy' = min(u0 + sum e / m, cap) / enttou, enttou through pow
            b = ((4 * (e["k"] + 8) + extra * e["k"]) * EPS * e["abs"] / float(d["mass"][j]) / e["enttou"] + (TRANS + 4 * EPS) * exp["entropy"][j])
            rat(form + "entropy", abs(got["entropy"][j] - exp["entropy"][j]), b)
        for j, e in info["kicks"].items():
            b = (4 * (e["k"] + 8) + extra * e["k"]) * EPS * e["abs"] + TRANS_DIR * e["abs"] + 2 * EPS * np.abs(exp["vel"][j])
            rat(form + "kick", np.abs(got["vel"][j] - exp["vel"][j]), b)
    # what the call does not write is bit-identical: outputs keep the sentinel, in / out columns their input
    for key in R.OUT:
        untouched = out[key] == R.SENTINEL
        assert np.array_equal(got[key][untouched], out[key][untouched]), (label, key)
    for key in R.IN_OUT:
        same = out[key] == d[key]
        assert np.array_equal(got[key][same], d[key][same]), (label, key)
    for key in ("gas_swallowed", "bh_swallowed", "accretion_neighbours", "feedback_neighbours", "accretion_targets", "feedback_targets"):
        assert stats[key] == info["stats"][key], (label, key, stats[key], info["stats"][key])
    assert stats["accretion_candidates"] >= stats["accretion_neighbours"] and stats["feedback_candidates"] >= stats["feedback_neighbours"]
    print("blackhole %s: %d / %d targets, %d gas and %d black holes swallowed, %d gas heated, %d kicked; largest ratio to the bound: %s; margins %s"
          % (label, len(tl), len(ftl), stats["gas_swallowed"], stats["bh_swallowed"], len(info["energy"]), len(info["kicks"]),
             ", ".join("%s %.3g" % kv for kv in sorted(worst.items())), ", ".join("%s %.1e" % kv for kv in info["margins"].items())))
    for key, v in worst.items():
        assert v <= 1, (label, key, v)
    return worst


def u64(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).cuda()


def dev_arrays(torch, d):
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    a = {}
    for key in ARRAY_IN + R.IN_OUT:
        a[key] = u64(torch, d[key]) if d[key].dtype == np.uint64 else up(d[key])
    for key, v in fresh_outputs(d["n"]).items():
        a[key] = u64(torch, v) if v.dtype == np.uint64 else up(v)
    keep = dict(pos=up(d["pos"]), type=up(d["type"]))
    return a, keep


def down(a):
    g = {}
    for key, v in a.items():
        h = v.cpu().numpy()
        want = R.OUT[key][0] if key in R.OUT else None
        g[key] = h.view(np.uint64) if want is np.uint64 or key == "id" else h
    return g


def new_engine(pkg, par, rnd):
    eng = pkg.Engine(0)
    eng.set_densitypar(ETA, 2.0, 2.0, 99999., pkg.engine.DENSITY_KERNEL_CUBIC_SPLINE, 0.006)
    eng.set_blackhole_params(par)
    if rnd is not None:
        eng.set_random_table(rnd)
    return eng


def run_dev(pkg, torch, d, par, T, rnd, active, mask=None, hmax=True):
    eng = new_engine(pkg, par, rnd)
    a, keep = dev_arrays(torch, d)
    eng.dev_bind_particles(keep["pos"], a["mass"], d["box"], type=keep["type"])
    eng.dev_force_tree_rebuild_mask(pkg.engine.GASMASK + pkg.engine.BHMASK if mask is None else mask)
    if hmax:
        eng.dev_force_tree_calc_hmax(a["hsml"])
    try:
        eng.dev_blackhole(a, sph_times(pkg, T), active=None if active is None else torch.from_numpy(active).cuda())
        eng.synchronize()
        return down(a), eng.blackhole_stats()
    finally:
        eng.close()


def host_table(pkg, d):
    P = pkg.make_particles(d["pos"], d["mass"], type=d["type_table"])
    P["Flags"] = d["flags"]
    return P


def host_arrays(d, skip=()):
    a = {key: d[key].copy() for key in ARRAY_IN + R.IN_OUT if key not in skip and key != "mass"}
    a.update(fresh_outputs(d["n"]))
    return a


def C_medd(par, T):
    return R.constants(par, T)["medd_fac"]


@pytest.mark.parametrize("name", ["zel", "clust"])
def test_dev_form(pkg, name):
    """mpg_dev_blackhole on a tree of gas and black holes: an active sublist (zel) and the NULL list (clust), kinetic feedback on"""
    import torch
    d, par, T, rnd, active, out, info, lit = scene(pkg, name)
    got, stats = run_dev(pkg, torch, d, par, T, rnd, active)
    compare(d, par, T, out, info, got, stats, "dev / " + name, lit=lit)


@pytest.mark.parametrize("over", [dict(BlackHoleFeedbackMethod=R.FB_SPLINE), dict(BlackHoleFeedbackMethod=R.FB_MASS), dict(BlackHoleFeedbackMethod=0),
                                  dict(BlackHoleKineticOn=0), dict(SeedBHDynMass=0.0), dict(BH_DRAG=2, MergeGravBound=0), dict(BH_DRAG=0, WindDecouple=0)],
                         ids=["volume-spline", "mass-tophat", "volume-tophat", "thermal-only", "no-seed-mass", "drag2-nobound", "nodrag-nodecouple"])
def test_dev_form_parameter_sets(pkg, over):
    """the four weight / spline combinations (mass-spline is the default of the other tests), BlackHoleKineticOn = 0, SeedBHDynMass = 0, the
    other BH_DRAG branches, mergers without the bound check, wind gas that is not decoupled"""
    import torch
    d, par, T, rnd, active, out, info, lit = scene(pkg, "zel", **over)
    got, stats = run_dev(pkg, torch, d, par, T, rnd, active)
    compare(d, par, T, out, info, got, stats, "dev / zel / " + str(over), lit=lit)
    if over.get("BlackHoleKineticOn") == 0:
        assert not info["kicks"] and (got["keflag"][info["targets"]] == 0).all()


def test_host_form(pkg):
    """mpg_blackhole: the arrays travel, Mass and the flags also go into the records"""
    d, par, T, rnd, active, out, info, lit = scene(pkg, "zel")
    P = host_table(pkg, d)
    eng = new_engine(pkg, par, rnd)
    a = host_arrays(d)
    eng.blackhole(P, d["box"], a, sph_times(pkg, T), ActiveParticle=active)
    stats = eng.blackhole_stats()
    ntree = eng.tree_stats().NumParticles
    eng.close()
    assert ntree == int(((d["type"] == 0) | (d["type"] == 5)).sum())
    assert a["id"].tobytes() == d["id"].tobytes()                     # an input goes up and does not come back
    got = dict(a, mass=P["Mass"].copy(), id=d["id"])
    compare(d, par, T, out, info, got, stats, "host / zel")
    assert np.array_equal(P["Flags"] & 3, got["flags"] & 3)


@pytest.mark.parametrize("tree", ["dm-tree", "fitting-tree"])
def test_resident_form_in_the_order_of_run_c(pkg, tree):
    """a resident gas stretch in the order of run.c: density -> hydro_force -> metal_return (stars that return mass: the resident Mass and
    Density columns change) -> find_vel_disp -> blackhole -> cooling.  "dm-tree": find_vel_disp runs (a PM step) and leaves the DM tree, so
    the call builds its own; "fitting-tree": find_vel_disp does not run and the current tree is one of gas and black holes with hmax, which
    the call uses as it is.  The entry state of the call is what the same stretch WITHOUT the call holds (the loops are deterministic);
    cooling afterwards skips the rows that were just swallowed."""
    import torch
    d0, par, T, rnd, active, *_ = scene(pkg, "zel")
    import test_gpu_cooling as TC
    C0, _, step, _, _ = TC.reference("sherwood_z3")
    n, box = d0["n"], d0["box"]
    t = sph_times(pkg, T)
    for k in ("drifts", "dloga_kick"):
        for b in range(47):
            getattr(t, k)[b] = 0.0
    stars = d0["type"] == 4
    rs = np.random.RandomState(4)
    z = lambda *s: np.zeros(s)
    runs = []
    for with_call in (False, True):
        P = host_table(pkg, d0)
        P["Vel"] = d0["vel"]
        P["FullTreeGravAccel"], P["GravPM"] = d0["gacc"], d0["gpm"]
        eng = new_engine(pkg, par, rnd)
        eng.set_gravshort_treepar()
        eng.gravshort_set_softenings(d0["soft"] / 2.8)
        eng.set_hydropar(0, 100.0, 0.75)
        eng.set_metal_params(1, 2.0, 4 * float(d0["mass"][d0["type"] == 0].mean()))
        TC.configure(eng, C0)
        a = dict(hsml=d0["hsml"].copy(), dthsml=z(n), vel=d0["vel"].copy(), gacc=d0["gacc"].copy(), gpm=d0["gpm"].copy(), tb_hydro=d0["tb_hydro"].copy(),
                 tb_grav=d0["tb_grav"].copy(), entropy=d0["entropy"].copy(), density=z(n), egywtdensity=z(n), dhsmlegyfac=z(n), divvel=z(n), curlvel=z(n),
                 hydroacc_out=z(n, 3), dtentropy_out=z(n), maxsignalvel=z(n))
        eng.resident_begin(P, box)
        eng.resident_sph_begin(P, a)
        eng.density(P, box, a, t, update_hsml=0, BlackHoleOn=1)
        eng.hydro_force(P, a, t)
        massgen = np.where(stars, 0.05 * d0["mass"].astype(np.float64), 0.0)
        metals = dict(massgenerated=massgen, metalgenerated=0.02 * massgen, speciesgenerated=np.ascontiguousarray(0.002 * massgen[:, None] * np.ones((1, 9))),
                      stellarage=np.full(n, 100.0), totalmassreturned=z(n), lastenrichment=z(n), metallicity=0.01 * rs.random_sample(n),
                      metals=np.ascontiguousarray(1e-3 * np.ones((n, 9))), massreturned=z(n))
        eng.resident_sph_metal_return(P, metals, ActiveParticle=active)
        assert eng.metals_stats()["targets"] >= 10 and metals["massreturned"][stars].sum() > 0
        vdisp = d0["vdisp"].copy()
        if tree == "dm-tree":
            eng.resident_sph_find_vel_disp(P, t, T["atime"], T["hubble"], 0.0, 1e30, vdisp, ActiveParticle=active)
            assert eng.tree_stats().NumParticles == int((d0["type"] == 1).sum())
        else:
            eng.dev_force_tree_rebuild_mask(pkg.engine.GASMASK + pkg.engine.BHMASK)
            eng.dev_force_tree_calc_hmax(TC.device_view(torch, eng.resident_sph_arrays()["hsml"], n))
        mass_entry = P["Mass"].copy()                                    # metal_return wrote the new masses into the records
        m = host_arrays(d0, skip=("vel", "gacc", "gpm", "hydroacc", "tb_hydro", "tb_grav", "hsml", "density", "entropy"))
        m["vdisp"] = vdisp
        stats, treated, entropy_after = None, None, None
        if with_call:
            eng.resident_sph_blackhole(P, m, t, ActiveParticle=active)
            stats = eng.blackhole_stats()
            entropy_after = TC.device_view(torch, eng.resident_sph_arrays()["entropy"], n).cpu().numpy()
            assert eng.tree_stats().NumParticles == int(((d0["type"] == 0) | (d0["type"] == 5)).sum())
            # cooling_and_starformation comes next in run.c: the gas just swallowed is garbage to it
            ne = np.ones(n)
            eng.resident_sph_cooling(P, t, step, ne, ActiveParticle=active)
            treated = eng.cooling_stats()["treated"]
        eng.resident_sph_end(a)
        eng.resident_end(P)
        runs.append((dict(a), m, P, stats, treated, mass_entry, entropy_after))
        eng.close()
    a0 = runs[0][0]
    assert np.array_equal(runs[0][5], runs[1][5]) and (runs[0][5] != d0["mass"])[d0["type"] == 0].sum() > 100     # the gas took the stars' mass
    entry = dict(d0, mass=runs[0][5], density=a0["density"], hydroacc=a0["hydroacc_out"], vdisp=runs[0][1]["vdisp"], entropy=a0["entropy"], vel=a0["vel"])
    out, info = R.blackhole(entry, par, T, rnd, active=active)
    assert info["stats"]["gas_swallowed"] > 10 and info["stats"]["bh_swallowed"] >= 3
    got = dict(runs[1][1], mass=runs[1][2]["Mass"].copy(), vel=runs[1][2]["Vel"].copy(), entropy=runs[1][6], id=d0["id"])
    compare(entry, par, T, out, info, got, runs[1][3], "resident / zel / " + tree)
    assert np.array_equal(runs[1][2]["Flags"] & 3, got["flags"] & 3)
    act = np.zeros(n, bool)
    act[active] = True
    assert runs[1][4] == int((act & (d0["type"] == 0)).sum()) - info["stats"]["gas_swallowed"]


def test_no_target(pkg):
    """a call without a target: nothing is written and no tree is demanded; the statistics are zero"""
    import torch
    d, par, T, rnd, *_ = scene(pkg, "zel")
    active = np.nonzero(d["type"] == 0)[0].astype(np.int32)
    eng = new_engine(pkg, par, rnd)
    a, keep = dev_arrays(torch, d)
    eng.dev_bind_particles(keep["pos"], a["mass"], d["box"], type=keep["type"])
    eng.dev_blackhole(a, sph_times(pkg, T), active=torch.from_numpy(active).cuda())      # no tree at all
    eng.synchronize()
    assert all(v == 0 for v in eng.blackhole_stats().values()) and all(v == 0 for v in eng.blackhole_times().values())
    got = down(a)
    eng.close()
    for key, v in fresh_outputs(d["n"]).items():
        assert np.array_equal(got[key], v), key
    for key in R.IN_OUT:
        assert np.array_equal(got[key], d[key]), key
    # the host form runs its queue pass before anything travels: arrays it would require are not even looked at
    P = host_table(pkg, d)
    eng = new_engine(pkg, par, rnd)
    eng.blackhole(P, d["box"], {}, sph_times(pkg, T), ActiveParticle=active)
    assert all(v == 0 for v in eng.blackhole_stats().values())
    eng.close()
    assert np.array_equal(P["Mass"], d["mass"]) and np.array_equal(P["Flags"], d["flags"])


def test_error_returns(pkg):
    """the two settings that are not carried; a dev call on a tree without gas, without black holes or without hmax; a call before the table"""
    import torch
    d, par, T, rnd, active, *_ = scene(pkg, "zel")
    eng = pkg.Engine(0)
    with pytest.raises(pkg.EngineError, match="BH_FEEDBACK_OPTTHIN"):
        eng.set_blackhole_params(dict(par, BlackHoleFeedbackMethod=R.FB_OPTTHIN | R.FB_MASS))
    with pytest.raises(pkg.EngineError, match="BHFeedbackUseTcool"):
        eng.set_blackhole_params(dict(par, BHFeedbackUseTcool=2))
    eng.close()
    with pytest.raises(pkg.EngineError, match="random table"):
        run_dev(pkg, torch, d, par, T, None, active)
    with pytest.raises(pkg.EngineError, match="GASMASK"):
        run_dev(pkg, torch, d, par, T, rnd, active, mask=pkg.engine.BHMASK + 2)
    with pytest.raises(pkg.EngineError, match="BHMASK"):
        run_dev(pkg, torch, d, par, T, rnd, active, mask=pkg.engine.GASMASK)
    with pytest.raises(pkg.EngineError, match="hmax"):
        run_dev(pkg, torch, d, par, T, rnd, active, hmax=False)


def test_random_table_decides_a_swallow(pkg):
    """mpg_set_random_table read back through a decision: one table entry changed flips the mark of one gas particle and nothing else"""
    import torch
    d, par, T, rnd, active, out, info, lit = scene(pkg, "zel")
    slots = (d["id"][d["type"] == 0] % np.uint64(len(rnd))).astype(np.int64)
    alone = np.bincount(slots, minlength=len(rnd)) == 1
    j = next(j for j, v in sorted(info["swal"].items()) if d["type"][j] == 0 and alone[int(d["id"][j]) % len(rnd)])
    slot = int(d["id"][j]) % len(rnd)
    rnd2 = rnd.copy()
    rnd2[slot] = 1.0 - 1e-9
    out2, info2 = R.blackhole(d, par, T, rnd2, active=active)
    assert j not in info2["swal"] and {k: v for k, v in info["swal"].items() if k != j} == info2["swal"]
    got, stats = run_dev(pkg, torch, d, par, T, rnd, active)
    got2, stats2 = run_dev(pkg, torch, d, par, T, rnd2, active)
    assert got["sph_swallowid"][j] == info["swal"][j] and got2["sph_swallowid"][j] == 0
    diff = np.nonzero(got["sph_swallowid"] != got2["sph_swallowid"])[0]
    assert list(diff) == [j] and stats2["gas_swallowed"] == stats["gas_swallowed"] - 1
