"""GPU tests of the helium reionisation by quasar bubbles (csrc/heiii.hip) against the all-pairs numpy restatement (tests/heiii_restated.py,
form (a): the literal sequential loop): mpg_dev_heiii_reionization at batch sizes 1, 3 and the default on two scenes and six cases, the host
form and the form on a resident gas run on the main case, mpg_dev_heiii_ionization_fraction, and the error returns.

Scenes (heiii_restated.heiii_scene): the 16^3 gas of ics.hydro_pair(16) and the clustered 4096-gas set ics.s_clust(16), each with garbage
rows, rows that became stars or black holes since, dark matter and a twentieth of the rows already ionised; 4133 rows (no multiple of 64).
161 groups, about 90 inside the mass window, one exactly on each bound; radii from 0.03 to 0.6 of the box; one centre in a corner, one
bubble that covers nothing, one MinID above 2^63.  Cases: desired reached mid-list with list position 0 chosen at iteration 2; the list
exhausted (the last candidate unlit); the insufficient-ionisation stop after more than 12 iterations; nothing to do; no candidates; flash.

Conditions (heiii_restated.conditions, proven on the CPU by test_heiii_restated.py and asserted here again before anything is compared): no
gas row within 1e-10 relative of ANY candidate's radius, every radius > 0, >= 500 rows ionised in the main case, >= 100 rows covered by two
or more lit bubbles and for >= 5 of them the first cover is not the bubble of lowest group index, every stop reason reached.

Compared, per scene, case, batch size and form
  integers    flags, per-iteration records (position, group, count), result integers, stop reason: EQUAL.
  doubles     initionfrac, curionfrac (per iteration and final) and the radii: BIT-IDENTICAL (the same host operations in the same order).
  Entropy     of newly ionised rows within (TRANS + 4 eps) (Entropy + delta), TRANS = 1e-14 as in test_gpu_winds.py and
              test_gpu_blackhole.py (the device pow); every other row and the density column bit-identical.
  the tree    the engine's tree statistics are unchanged by the call; without a tree none is built.
The largest observed ratio to the entropy bound is printed (pytest -s); DESIGN 3.14 records it."""
import numpy as np
import pytest

import heiii_restated as R

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps
TRANS = 1e-14
BATCHES = (1, 3, 0)          # 0: the default


def up(torch, a):
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint64:
        a = a.view(np.int64)          # torch has no uint64: the same bits
    return torch.from_numpy(a).cuda()


def bound_engine(pkg, torch, d, par, table=True, tree=True):
    eng = pkg.Engine(0)
    if par is not None:
        eng.set_heiii_params(par)
    if table:
        eng.set_random_table(d["table"])
    keep = dict(pos=up(torch, d["pos"]), mass=up(torch, np.ones(d["n"], np.float32)), type=up(torch, d["type"]))
    eng.dev_bind_particles(keep["pos"], keep["mass"], d["box"], type=keep["type"])
    if tree:
        eng.dev_force_tree_rebuild_mask(pkg.engine.GASMASK)
        eng.synchronize()
    return eng, keep


def dev_groups(torch, d):
    return dict(mass=up(torch, d["gmass"]), cm=up(torch, d["gcm"]), minid=up(torch, d["gminid"]))


def host_groups(d):
    return dict(mass=d["gmass"].copy(), cm=d["gcm"].copy(), minid=d["gminid"].copy())


def tree_tuple(eng):
    s = eng.tree_stats()
    return (s.NumParticles, s.numnodes, s.numleaves, s.maxlevel, s.root_mass, tuple(s.root_cofm), s.root_hmax)


def compare(d, par, st, want, cname, got_flag, got_ent, res, exp, label):
    R.conditions(d, par, st, want, cname)
    flag, ent, wres, rec = want
    assert np.array_equal(got_flag, flag), label
    for k in ("n_ionized_before", "flash_ionized", "iterations", "tot_n_ionized", "stop_reason"):
        assert res[k] == wres[k], (label, k, res[k], wres[k])
    for k in ("initionfrac", "curionfrac"):
        assert np.float64(res[k]).tobytes() == np.float64(wres[k]).tobytes(), (label, k, res[k], wres[k])
    assert len(exp["position"]) == len(rec), label
    assert exp["position"].tolist() == [r[0] for r in rec] and exp["group"].tolist() == [r[1] for r in rec], label
    assert exp["count"].tolist() == [r[3] for r in rec], label
    assert exp["radius"].tobytes() == np.array([r[2] for r in rec], np.float64).tobytes(), label
    assert exp["curionfrac"].tobytes() == np.array([r[4] for r in rec], np.float64).tobytes(), label
    new = (flag != 0) & (d["flag"] == 0)
    assert int(new.sum()) == wres["tot_n_ionized"] + wres["flash_ionized"]
    worst = 0.0
    if new.any():
        delta = R.heat(d, st)[new]
        worst = float((np.abs(got_ent[new] - ent[new]) / ((TRANS + 4 * EPS) * (d["entropy"][new] + delta))).max())
        assert (got_ent[new] > d["entropy"][new]).all()
    assert got_ent[~new].tobytes() == d["entropy"][~new].tobytes(), label
    print("heiii %s: %s after %d iterations, %d rows ionised (%d by the flash), curionfrac %.6f, largest ratio to the entropy bound %.3g"
          % (label, R.REASONS[res["stop_reason"]], res["iterations"], wres["tot_n_ionized"], wres["flash_ionized"], res["curionfrac"], worst))
    assert worst <= 1, (label, worst)


@pytest.mark.parametrize("sname", sorted(R.SCENES))
@pytest.mark.parametrize("cname", R.CASES)
def test_dev_form(pkg, sname, cname):
    """mpg_dev_heiii_reionization at B = 1, 3 and the default, with a gas tree in place that the call must leave alone"""
    import torch
    d, par, st, want = R.restated(pkg.ics, sname, cname)
    eng, keep = bound_engine(pkg, torch, d, par)
    before = tree_tuple(eng)
    g = dev_groups(torch, d)
    dens = up(torch, d["density"])
    for B in BATCHES:
        eng.heiii_set_batch(B)
        ent, flag = up(torch, d["entropy"]), up(torch, d["flag"])
        n0, f0 = eng.dev_heiii_ionization_fraction(flag, st["n_gas_tot"])
        res = eng.dev_heiii_reionization(st, dens, ent, flag, g)
        eng.synchronize()
        exp = eng.heiii_export()
        assert tree_tuple(eng) == before
        assert n0 == want[2]["n_ionized_before"] and f0 == n0 / st["n_gas_tot"]
        n1, f1 = eng.dev_heiii_ionization_fraction(flag, st["n_gas_tot"])
        assert n1 == int(((want[0] != 0) & (d["type"] == 0)).sum())
        if res["iterations"] > 0:
            t = eng.heiii_times()
            assert t["scan_ms"] > 0 and t["copy_ms"] > 0 and t["apply_ms"] > 0
        assert np.array_equal(dens.cpu().numpy(), d["density"])
        for k in g:
            assert np.array_equal(g[k].cpu().numpy(), up(torch, d["g" + k]).cpu().numpy())
        compare(d, par, st, want, cname, flag.cpu().numpy(), ent.cpu().numpy(), res, exp, "dev / %s / %s / B %d" % (sname, cname, B))
    eng.close()


@pytest.mark.parametrize("sname", sorted(R.SCENES))
def test_host_form(pkg, sname):
    """mpg_heiii_reionization on the main case: the table carries IsGarbage in its flags (the garbage rows are gas by type); no tree is built"""
    d, par, st, want = R.restated(pkg.ics, sname, "main")
    table_type = d["type"].copy()
    table_type[d["garbage"]] = 0
    P = pkg.make_particles(d["pos"], np.ones(d["n"], np.float32), type=table_type)
    P["Flags"][d["garbage"]] = 1
    for B in BATCHES:
        eng = pkg.Engine(0)
        eng.set_heiii_params(par)
        eng.set_random_table(d["table"])
        eng.heiii_set_batch(B)
        dens, ent, flag, g = d["density"].copy(), d["entropy"].copy(), d["flag"].copy(), host_groups(d)
        res = eng.heiii_reionization(P, d["box"], st, dens, ent, flag, g)
        exp = eng.heiii_export()
        with pytest.raises(pkg.EngineError, match="no tree"):
            eng.tree_stats()
        eng.close()
        assert np.array_equal(dens, d["density"]) and np.array_equal(P["Type"], table_type)
        assert all(np.array_equal(g[k], d["g" + k]) for k in g)
        compare(d, par, st, want, "main", flag, ent, res, exp, "host / %s / main / B %d" % (sname, B))


def device_view(torch, ptr, n):
    class H:
        pass
    h = H()
    h.__cuda_array_interface__ = {"shape": (int(n),), "typestr": "<f8", "data": (int(ptr), False), "version": 2}
    return torch.as_tensor(h, device="cuda")


def test_resident_form(pkg):
    """mpg_resident_sph_heiii_reionization on the main case: Density and Entropy are the resident columns, the flag travels"""
    import torch
    d, par, st, want = R.restated(pkg.ics, "zel", "main")
    n = d["n"]
    table_type = d["type"].copy()
    table_type[d["garbage"]] = 0
    P = pkg.make_particles(d["pos"], np.ones(n, np.float32), type=table_type)
    P["Flags"][d["garbage"]] = 1
    eng = pkg.Engine(0)
    eng.set_heiii_params(par)
    eng.set_random_table(d["table"])
    z = lambda *s: np.zeros(s)
    a = dict(hsml=np.full(n, d["box"] / 16), dthsml=z(n), vel=z(n, 3), gacc=z(n, 3), gpm=z(n, 3), entropy=d["entropy"].copy(), density=d["density"].copy(),
             egywtdensity=z(n), dhsmlegyfac=z(n), divvel=z(n), curlvel=z(n), hydroacc_out=z(n, 3), dtentropy_out=z(n), maxsignalvel=z(n),
             tb_grav=np.ones(n, np.uint8), tb_hydro=np.ones(n, np.uint8))
    eng.resident_begin(P, d["box"])
    eng.resident_sph_begin(P, a)
    ptr = eng.resident_sph_arrays()
    d_ent, d_rho = device_view(torch, ptr["entropy"], n), device_view(torch, ptr["density"], n)
    d_ent.copy_(up(torch, d["entropy"]))
    d_rho.copy_(up(torch, d["density"]))
    torch.cuda.synchronize()
    flag, g = d["flag"].copy(), host_groups(d)
    res = eng.resident_sph_heiii_reionization(P, st, flag, g)
    exp = eng.heiii_export()
    got_ent = d_ent.cpu().numpy()
    assert np.array_equal(d_rho.cpu().numpy(), d["density"])
    eng.resident_sph_end(a)
    eng.resident_end(P)
    eng.close()
    compare(d, par, st, want, "main", flag, got_ent, res, exp, "resident / zel / main")


def test_errors(pkg):
    """no parameters, no random table, n_gas_tot <= 0, a batch size outside 0 .. 64, a radius that is not positive, a table value of
    exactly 0 at a seed used as u1: each an error return, and the columns are as they were"""
    import torch
    d = R.scene(pkg.ics, "zel")
    par, st, _ = R.case(d, "main")
    E = pkg.EngineError
    g = dev_groups(torch, d)
    dens = up(torch, d["density"])

    def call(eng, step=st, groups=g):
        ent, flag = up(torch, d["entropy"]), up(torch, d["flag"])
        try:
            return eng.dev_heiii_reionization(step, dens, ent, flag, groups)
        finally:
            assert np.array_equal(flag.cpu().numpy(), d["flag"]) and np.array_equal(ent.cpu().numpy(), d["entropy"])

    eng, keep = bound_engine(pkg, torch, d, None, tree=False)
    with pytest.raises(E, match="no parameters"):
        call(eng)
    eng.close()
    eng, keep = bound_engine(pkg, torch, d, par, table=False, tree=False)
    with pytest.raises(E, match="random table"):
        call(eng)
    eng.close()
    eng, keep = bound_engine(pkg, torch, d, par, tree=False)
    for bad in (0, -5):
        with pytest.raises(E, match="n_gas_tot"):
            call(eng, dict(st, n_gas_tot=bad))
        with pytest.raises(E, match="n_gas_tot"):
            eng.dev_heiii_ionization_fraction(up(torch, d["flag"]), bad)
    for bad in (-1, 65):
        with pytest.raises(E, match="bubbles per scan"):
            eng.heiii_set_batch(bad)
    with pytest.raises(E, match="required"):
        call(eng, groups=dict(g, cm=None))
    eng.set_heiii_params(dict(par, mean_bubble=0.001 * d["box"]))
    with pytest.raises(E, match="not positive and finite"):
        call(eng)
    eng.set_heiii_params(par)
    t = d["table"].copy()
    for k in R.candidates(d, par):
        t[int(d["gminid"][k]) % len(t)] = 0.0
    eng.set_random_table(t)
    with pytest.raises(E, match="exactly 0"):
        call(eng)
    eng.set_random_table(d["table"])
    ent, flag = up(torch, d["entropy"]), up(torch, d["flag"])
    res = eng.dev_heiii_reionization(st, dens, ent, flag, g)     # the refused calls changed nothing: the call still runs
    assert res["stop_reason"] == R.REACHED
    eng.close()
