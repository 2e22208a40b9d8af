"""GPU tests of the DM velocity dispersion (winds_find_vel_disp, csrc/veldisp.hip) against the numpy restatement
(tests/veldisp_restated.py, which walks in a fixed order with the reference's literal shrinking search radius): the three entry points
mpg_dev_find_vel_disp / mpg_find_vel_disp / mpg_resident_sph_find_vel_disp, the latter in the call order of the in-tree shim
(density -> hydro_force -> winds_find_vel_disp inside a resident stretch).

What is compared, per call
  counts   per target the number of iterations, the final closest count and maxcmpte; the queue length of every iteration; which entries of
           vdisp were written (the others keep a sentinel): all EQUAL.
  radii    the final trial radius to 1e-12 relative: an iteration adds a few ulp through the two pow calls (the device pow is not correctly
           rounded), iterations number about 10, and a wrong branch moves a radius by at least the loop's own 5e-6.
  VDisp    |dVDisp| <= B / (6 VDisp), B = 4 (n + 8) eps V2 / n from the restatement's own sums: the first-order summation error of n terms
           plus the flops of the prediction and the Hubble term, with a factor 4 over it.
Conditions, asserted from the restatement alone on the seeds chosen here: no DM particle within 1e-10 relative of any trial radius used
(else a count may legitimately flip), no written target with a variance below ten times its bound, no target ending through the
tight-bracket exit.  The largest observed ratio |dVDisp| / bound is printed (pytest -s); DESIGN 3.8 records it."""
import numpy as np
import pytest

import veldisp_restated as R

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps
SENTINEL = -7.0


# ---- inputs ---------------------------------------------------------------------------------------------------------------------------------
def zel_set(pkg):
    """DM + gas from ics at 32^3 each (the gas run's initial conditions), 6 black holes, garbage / swallowed rows"""
    pos, _, typ, box = pkg.ics.hydro_pair(32)
    return R.sample_inputs(pos[typ == 0], pos[typ == 1], box, seed=11), R.sample_times(11)


def clustered_set(pkg):
    """a clustered set: two thirds of DM and gas in two clumps, smoothing lengths off by factors"""
    pd, _, box = pkg.ics.s_clust(20, seed=2)
    pg, _, _ = pkg.ics.s_clust(20, seed=3)
    return R.sample_inputs(pg, pd, box, seed=12, hsml_scatter=0.9), R.sample_times(12)


def threshold_for(d, fraction):
    """the sfr_density_threshold that lets about `fraction` of the gas qualify (the engine takes a tenth of it)"""
    return 10.0 * float(np.quantile(d["density"][:d["ng"]], 1.0 - fraction))


def restate(d, t, thr, active=None):
    vd = np.full(d["n"], SENTINEL)
    res = R.find_vel_disp(d["pos"], d["type"], d["vel"], d["gacc"], d["gpm"], d["tb_grav"], d["hsml"], d["dthsml"], d["density"], vd, d["box"],
                          t["Time"], t["hubble"], t["ddrift"], thr, t["gravkicks"], t["FgravkickB"], active=active)
    return vd, res


def conditions(res):
    """what the chosen seeds must satisfy, from the restatement alone; returns the per-target VDisp bounds"""
    assert res["min_gap"] > 1e-10, res["min_gap"]
    assert not any(res["tight"].values())
    bound = {}
    for i, var in res["var"].items():
        n = res["numngb"][i]
        b = 4 * (n + 8) * EPS * res["v2n"][i]
        assert var > 10 * b, (i, var, b)
        bound[i] = b / (6 * np.sqrt(var / 3))
    for i, var in res["bh_var"].items():
        n = res["bh_numdm"][i]
        b = 4 * (n + 8) * EPS * res["bh_v2n"][i]
        if var > 0:
            assert var > 10 * b, (i, var, b)
            bound[i] = b / (6 * np.sqrt(var / 3))
    return bound


def sph_times(pkg, t):
    T = pkg.SphTimes()
    T.FgravkickB = t["FgravkickB"]
    for b in range(47):
        T.gravkicks[b] = t["gravkicks"][b]
        T.hydrokicks[b] = 0.123      # (not read by this call)
    T.atime, T.hubble = 99.0, 99.0   # (not read either: Time and hubble come with mpg_veldisp_params)
    return T


def compare(d, res, vd_ref, vd, exp, stats, label):
    bound = conditions(res)
    gas = sorted(res["iterations"])
    bhs = sorted(res["bh_numdm"])
    targets = set(gas) | set(bhs)
    assert set(np.nonzero(exp["iterations"] >= 0)[0].tolist()) == targets
    assert exp["queue_lengths"] == res["queue_lengths"]
    assert stats["iterations"] == len(res["queue_lengths"]) and stats["targets"] == sum(res["queue_lengths"]) and stats["tight"] == 0
    assert stats["candidates"] >= stats["neighbours"] > 0
    g = np.array(gas, np.int64)
    if len(g):
        assert np.array_equal(exp["iterations"][g], [res["iterations"][i] for i in gas])
        assert np.array_equal(exp["numngb"][g], [res["numngb"][i] for i in gas])
        assert np.array_equal(exp["maxcmpte"][g], [res["maxcmpte"][i] for i in gas])
        rr = np.array([res["radius"][i] for i in gas])
        assert np.abs(exp["radius"][g] / rr - 1).max() <= 1e-12
    for i in bhs:
        assert exp["numngb"][i] == res["bh_numdm"][i] and exp["iterations"][i] == 1
    # written and untouched entries
    assert np.array_equal(vd != SENTINEL, vd_ref != SENTINEL)
    assert set(np.nonzero(vd != SENTINEL)[0].tolist()) <= targets
    worst = 0.0
    for i, b in bound.items():
        err = abs(vd[i] - vd_ref[i])
        assert err <= b, (label, i, err, b)
        worst = max(worst, err / b)
    print("veldisp %s: %d gas targets, %d iterations, %d black holes, max |dVDisp| / bound = %.3f, min gap %.2e"
          % (label, len(gas), len(res["queue_lengths"]), len(bhs), worst, res["min_gap"]))
    return worst


def dev_arrays(torch, d, vd):
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    a = {k: up(d[k]) for k in ("vel", "gacc", "gpm", "tb_grav", "hsml", "dthsml", "density")}
    a["vdisp"] = up(vd)
    keep = dict(pos=up(d["pos"]), mass=up(d["mass"]), type=up(d["type"]))
    return a, keep


def host_table(pkg, d):
    """struct particle_data with the types as the table holds them and IsGarbage / Swallowed in the flags byte"""
    P = pkg.make_particles(d["pos"], d["mass"], type=d["type_table"])
    P["Flags"][d["dead"]] = 1
    P["Flags"][d["n"] - 1] = 2       # the last black hole: swallowed
    P["Vel"], P["FullTreeGravAccel"], P["GravPM"] = d["vel"], d["gacc"], d["gpm"]
    P["TimeBinGravity"], P["Hsml"], P["DtHsml"] = d["tb_grav"], d["hsml"], d["dthsml"]
    return P


# ---- the three entry points ---------------------------------------------------------------------------------------------------------------
def test_dev_form_null_list_partial_threshold(pkg):
    """mpg_dev_find_vel_disp, NULL active list, a threshold that excludes most of the gas; targets near the faces of the box"""
    import torch
    d, t = zel_set(pkg)
    thr = threshold_for(d, 0.035)
    vd_ref, res = restate(d, t, thr)
    gas = sorted(res["iterations"])
    assert 800 < len(gas) < 1500 and len(res["bh_numdm"]) == 5 and len(res["queue_lengths"]) > 3
    nb = sorted(res["bh_numdm"].values())
    assert nb[0] < 30 and nb[-1] > 200                        # black holes from a few to a few hundred DM neighbours
    face = [i for i in gas if (d["pos"][i] < res["radius"][i]).any() or (d["pos"][i] > d["box"] - res["radius"][i]).any()]
    assert len(face) > 20                                     # targets whose search crosses a face
    eng = pkg.Engine(0)
    a, keep = dev_arrays(torch, d, np.full(d["n"], SENTINEL))
    eng.dev_bind_particles(keep["pos"], keep["mass"], d["box"], type=keep["type"])
    eng.dev_find_vel_disp(a, sph_times(pkg, t), t["Time"], t["hubble"], t["ddrift"], thr)
    eng.synchronize()
    compare(d, res, vd_ref, a["vdisp"].cpu().numpy(), eng.veldisp_export(d["n"]), eng.veldisp_stats(), "dev / zel")
    # the current tree is the DM tree now
    assert eng.tree_stats().NumParticles == int((d["type"] == 1).sum())
    # an active sublist on the same arrays
    act = np.sort(np.random.RandomState(3).choice(d["n"], d["n"] // 2, replace=False)).astype(np.int32)
    vd_ref2, res2 = restate(d, t, thr, active=act)
    a["vdisp"].fill_(SENTINEL)
    eng.dev_find_vel_disp(a, sph_times(pkg, t), t["Time"], t["hubble"], t["ddrift"], thr, active=torch.from_numpy(act).cuda())
    eng.synchronize()
    compare(d, res2, vd_ref2, a["vdisp"].cpu().numpy(), eng.veldisp_export(d["n"]), eng.veldisp_stats(), "dev / zel / sublist")
    assert all(vd_ref2[i] == vd_ref[i] for i in res2["iterations"])
    eng.close()


def test_host_form_active_sublist(pkg):
    """mpg_find_vel_disp on the 160-byte records (flags: IsGarbage, Swallowed) with an active sublist"""
    d, t = zel_set(pkg)
    thr = threshold_for(d, 0.06)
    act = np.concatenate([np.arange(0, d["n"] - d["nbh"], 2), np.arange(d["n"] - d["nbh"], d["n"])]).astype(np.int32)
    vd_ref, res = restate(d, t, thr, active=act)
    assert 700 < len(res["iterations"]) < 1500 and len(res["bh_numdm"]) == 5
    P = host_table(pkg, d)
    eng = pkg.Engine(0)
    vd = np.full(d["n"], SENTINEL)
    a = dict(vel=d["vel"].copy(), gacc=d["gacc"].copy(), gpm=d["gpm"].copy(), tb_grav=d["tb_grav"].copy(), hsml=d["hsml"].copy(),
             dthsml=d["dthsml"].copy(), density=d["density"].copy(), vdisp=vd)
    eng.find_vel_disp(P, d["box"], a, sph_times(pkg, t), t["Time"], t["hubble"], t["ddrift"], thr, ActiveParticle=act)
    assert a["vel"].tobytes() == d["vel"].tobytes()                   # an input goes up and does not come back
    compare(d, res, vd_ref, vd, eng.veldisp_export(d["n"]), eng.veldisp_stats(), "host / zel / sublist")
    eng.close()


def test_resident_form_in_the_shims_call_order(pkg):
    """a resident gas stretch on the clustered set in the order of run.c: density -> hydro_force -> winds_find_vel_disp
    (mpg_resident_sph_find_vel_disp: only vdisp travels), then density again (the host form rebuilds its gas tree)"""
    d, t = clustered_set(pkg)
    P = host_table(pkg, d)
    n, box = d["n"], d["box"]
    eng = pkg.Engine(0)
    eng.set_gravshort_treepar()
    eng.gravshort_set_softenings(box / 20)
    eng.set_densitypar(1.0, 2.0, 2.0, 99999., pkg.engine.DENSITY_KERNEL_QUINTIC_SPLINE, 0.006)
    eng.set_hydropar(0, 100.0, 0.75)
    z = lambda *s: np.zeros(s)
    a = dict(hsml=z(n), dthsml=z(n), vel=d["vel"].copy(), gacc=d["gacc"].copy(), gpm=d["gpm"].copy(), entropy=np.ones(n), density=z(n), egywtdensity=z(n), dhsmlegyfac=z(n), divvel=z(n), curlvel=z(n),
             hydroacc_out=z(n, 3), dtentropy_out=z(n), maxsignalvel=z(n), tb_grav=d["tb_grav"].copy(), tb_hydro=d["tb_grav"].copy())
    T = sph_times(pkg, t)
    T.atime, T.hubble = t["Time"], t["hubble"]
    for b in range(47):
        T.hydrokicks[b] = 0.0
        T.dloga_bin[b] = 0.01
    eng.set_init_hsml(P, box, a, box / 20)
    eng.resident_begin(P, box)
    eng.resident_sph_begin(P, a)
    eng.density(P, box, a, T)
    eng.hydro_force(P, a, T)
    act = np.concatenate([np.arange(0, n - d["nbh"], 4), np.arange(n - d["nbh"], n)]).astype(np.int32)
    vd = np.full(n, SENTINEL)
    eng.resident_sph_find_vel_disp(P, T, t["Time"], t["hubble"], t["ddrift"], 0.0, vd, ActiveParticle=act)
    exp, stats = eng.veldisp_export(n), eng.veldisp_stats()
    eng.density(P, box, a, T)            # the stretch goes on: the gas tree is rebuilt by the host form
    eng.hydro_force(P, a, T)
    eng.resident_sph_end(a)
    eng.resident_end(P)
    # the restatement on what the stretch held at the call: Hsml / DtHsml / Density of the (converged) density loop
    d2 = dict(d, hsml=a["hsml"].copy(), dthsml=a["dthsml"].copy(), density=a["density"].copy())
    vd_ref, res = restate(d2, t, 0.0, active=act)
    # (fewer than the ~2000 listed gas particles qualify although the threshold is 0: DtHsml of the density loop on random velocities makes
    # densfac negative for many, and Density / densfac^3 < 0 is "below the threshold" in the reference's test, veldisp.c:359-363)
    assert len(res["iterations"]) > 500 and max(res["iterations"].values()) >= 3
    compare(d2, res, vd_ref, vd, exp, stats, "resident / clustered / sublist")
    eng.close()


# ---- early exits --------------------------------------------------------------------------------------------------------------------------
def test_nothing_qualifies(pkg):
    """a threshold that excludes all gas and a table without black holes: nothing is written and no tree is built or demanded; with
    black holes in the table the DM tree is built and the black-hole pass runs"""
    import torch
    d, t = clustered_set(pkg)
    none = dict(d, type=np.where(d["type"] == 5, 7, d["type"]).astype(np.uint8))
    vd_ref, res = restate(none, t, 1e30)
    assert not res["built"]
    eng = pkg.Engine(0)
    a, keep = dev_arrays(torch, none, np.full(d["n"], SENTINEL))
    eng.dev_bind_particles(keep["pos"], keep["mass"], d["box"], type=keep["type"])
    eng.dev_find_vel_disp(a, sph_times(pkg, t), t["Time"], t["hubble"], t["ddrift"], 1e30)     # no tree yet: none demanded
    with pytest.raises(pkg.EngineError, match="no tree"):
        eng.tree_stats()
    eng.dev_force_tree_rebuild_mask(pkg.engine.GASMASK)
    ngas = eng.tree_stats().NumParticles
    eng.dev_find_vel_disp(a, sph_times(pkg, t), t["Time"], t["hubble"], t["ddrift"], 1e30)
    eng.synchronize()
    assert eng.tree_stats().NumParticles == ngas == int((d["type"] == 0).sum())                # the gas tree stays
    assert (a["vdisp"].cpu().numpy() == SENTINEL).all()
    st = eng.veldisp_stats()
    assert st["iterations"] == 0 and st["targets"] == 0 and st["candidates"] == 0
    # black holes, no qualifying gas
    vd_ref, res = restate(d, t, 1e30)
    assert res["built"] and res["queue_lengths"] == [] and len(res["bh_numdm"]) == 5
    a, keep = dev_arrays(torch, d, np.full(d["n"], SENTINEL))
    eng.dev_bind_particles(keep["pos"], keep["mass"], d["box"], type=keep["type"])
    eng.dev_force_tree_rebuild_mask(pkg.engine.GASMASK)
    eng.dev_find_vel_disp(a, sph_times(pkg, t), t["Time"], t["hubble"], t["ddrift"], 1e30)
    eng.synchronize()
    compare(d, res, vd_ref, a["vdisp"].cpu().numpy(), eng.veldisp_export(d["n"]), eng.veldisp_stats(), "dev / black holes only")
    assert eng.tree_stats().NumParticles == int((d["type"] == 1).sum())
    eng.close()


# ---- no side effects ----------------------------------------------------------------------------------------------------------------------
def test_density_and_hydro_after_a_call_are_bit_identical(pkg):
    """mpg_dev_density + mpg_dev_hydro_force after a velocity-dispersion call (the gas tree rebuilt, as the header documents) equal the
    same calls without it, bit for bit"""
    import torch
    pos, mass, typ, box = pkg.ics.hydro_pair(16)
    n = len(pos)
    rng = np.random.RandomState(7)
    vel = rng.standard_normal((n, 3))
    T = pkg.SphTimes()
    T.atime, T.hubble = 0.5, 0.3
    for b in range(47):
        T.dloga_bin[b] = 0.01
    outs = []
    for with_call in (False, True):
        eng = pkg.Engine(0)
        eng.set_gravshort_treepar()
        eng.gravshort_set_softenings(box / 16)
        eng.set_densitypar(1.0, 2.0, 2.0, 99999., pkg.engine.DENSITY_KERNEL_QUINTIC_SPLINE, 0.006)
        eng.set_hydropar(0, 100.0, 0.75)
        up = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()
        keep = dict(pos=up(pos), mass=up(mass), type=up(typ))
        z = lambda *s: torch.zeros(*s, dtype=torch.float64, device="cuda")
        a = dict(hsml=z(n), dthsml=z(n), vel=up(vel), entropy=torch.ones(n, dtype=torch.float64, device="cuda"), density=z(n), egywtdensity=z(n),
                 dhsmlegyfac=z(n), divvel=z(n), curlvel=z(n), hydroacc_out=z(n, 3), dtentropy_out=z(n), maxsignalvel=z(n))
        eng.dev_bind_particles(keep["pos"], keep["mass"], box, type=keep["type"])
        eng.dev_force_tree_rebuild_mask(pkg.engine.GASMASK + pkg.engine.BHMASK, with_moments=True)
        eng.dev_set_init_hsml(a, box / 16)
        eng.dev_force_tree_rebuild_mask(pkg.engine.GASMASK)
        eng.dev_density(a, T)
        eng.dev_force_tree_calc_hmax()
        eng.dev_hydro_force(a, T)
        if with_call:
            v = dict(vel=a["vel"], hsml=a["hsml"], dthsml=a["dthsml"], density=a["density"], vdisp=z(n))
            eng.dev_find_vel_disp(v, T, 0.5, 0.3, 0.2, 0.0)
            assert eng.veldisp_stats()["targets"] >= n // 2 and eng.tree_stats().NumParticles == n // 2
            assert (v["vdisp"][: n // 2] > 0).all() and (v["vdisp"][n // 2:] == 0).all()
        eng.dev_force_tree_rebuild_mask(pkg.engine.GASMASK)
        eng.dev_density(a, T)
        eng.dev_force_tree_calc_hmax()
        eng.dev_hydro_force(a, T)
        eng.synchronize()
        outs.append({k: a[k].cpu().numpy().copy() for k in ("hsml", "dthsml", "density", "dhsmlegyfac", "divvel", "curlvel", "hydroacc_out",
                                                            "dtentropy_out", "maxsignalvel")})
        eng.close()
    for k in outs[0]:
        assert np.array_equal(outs[0][k], outs[1][k]), k


# ---- errors -------------------------------------------------------------------------------------------------------------------------------
def test_errors(pkg):
    """the 400-iteration limit (a gas particle with Hsml = 0 never leaves DMRadius = 0: the reference's endrun(1155)) and a missing required
    array are error returns with a message; the engine goes on working"""
    import torch
    d, t = clustered_set(pkg)
    live = int(np.nonzero(d["type"] == 0)[0][0])
    bad = dict(d, hsml=d["hsml"].copy())
    bad["hsml"][live] = 0.0
    act = np.array([live], np.int32)
    with pytest.raises(R.NoConvergence):
        restate(bad, t, 0.0, active=act)
    eng = pkg.Engine(0)
    a, keep = dev_arrays(torch, bad, np.full(d["n"], SENTINEL))
    eng.dev_bind_particles(keep["pos"], keep["mass"], d["box"], type=keep["type"])
    with pytest.raises(pkg.EngineError, match="failed to converge"):
        eng.dev_find_vel_disp(a, sph_times(pkg, t), t["Time"], t["hubble"], t["ddrift"], 0.0, active=torch.from_numpy(act).cuda())
    assert eng.veldisp_stats()["iterations"] == R.MAXITER + 1
    for missing in ("vel", "hsml", "density", "vdisp"):
        b = dict(a)
        b[missing] = None
        with pytest.raises(pkg.EngineError, match="required"):
            eng.dev_find_vel_disp(b, sph_times(pkg, t), t["Time"], t["hubble"], t["ddrift"], 0.0)
    # ... and a good call afterwards
    a, keep = dev_arrays(torch, d, np.full(d["n"], SENTINEL))
    eng.dev_bind_particles(keep["pos"], keep["mass"], d["box"], type=keep["type"])
    act = np.arange(0, 400, dtype=np.int32)
    vd_ref, res = restate(d, t, 0.0, active=act)
    eng.dev_find_vel_disp(a, sph_times(pkg, t), t["Time"], t["hubble"], t["ddrift"], 0.0, active=torch.from_numpy(act).cuda())
    eng.synchronize()
    compare(d, res, vd_ref, a["vdisp"].cpu().numpy(), eng.veldisp_export(d["n"]), eng.veldisp_stats(), "dev / after errors")
    eng.close()
