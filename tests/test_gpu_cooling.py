"""GPU tests of the radiative cooling (cooling_direct / DoCooling and the ionisation network, csrc/cooling.hip) against the plain-Python
restatement tests/cooling_restated.py, which tests/test_cooling_restated.py pins to the reference's known answers and whose decisions it
shows to be stable on the very input sets used here.

What is compared, per call
  counts    the network evaluations of every particle (mpg_cooling_export), the statistics of the call, Sfr == 0, and that rows outside
            the list, non-gas, garbage and massless rows keep Entropy / Ne / Sfr: EQUAL.
  Entropy   1e-12 relative: with identical decisions the bracket is identical; what remains is a handful of roundings and the device's
            exp / log in entropy_to_u.
  Ne        1e-10 absolute: the sensitivity to a 2e-15 change of the tables is 7e-15; the margin covers the device's exp / log / pow.
  A particle may miss these (or its count) only within 0.1 % of the treated particles, and must then still agree to 3e-6 relative (two final
  brackets).  The worst ratios are printed (pytest -s); DESIGN 3.9 records them.
Both kernel forms (one particle per lane to completion; the per-lane state machine with a wave-aggregated list) and both table placements
are run: MPG_COOLING_FORM / MPG_COOLING_LDS are read by mpg_set_cooling_params."""
import math
import os

import numpy as np
import pytest

import cooling_restated as R
import test_cooling_restated as K

pytestmark = pytest.mark.gpu

G = K.G
_ref = {}


def reference(name):
    """the restatement of a setting's whole input set, computed once: cooling_direct is per particle, so every shape and every active list
    of the tests is a selection of these rows"""
    if name not in _ref:
        C, times, step, make = R.config(name, G["treecool"])
        d = make(K.SIZES[name])
        _ref[name] = (C, times, step, d, R.cool_particles(C, d, times, step))
        assert not _ref[name][4]["failed"]
    return _ref[name]


def sph_times(pkg, times):
    T = pkg.SphTimes()
    T.atime, T.hubble = times["atime"], times["hubble"]
    for b in range(47):
        T.dloga_bin[b] = times["dloga_bin"][b]
        T.gravkicks[b] = T.hydrokicks[b] = T.drifts[b] = T.dloga_kick[b] = 0.123      # (not read by the cooling)
    return T


def configure(eng, C, form=0, lds=0, **over):
    os.environ["MPG_COOLING_FORM"], os.environ["MPG_COOLING_LDS"] = str(form), str(lds)
    try:
        eng.set_cooling_params(dict(C.p, **over))
    finally:
        del os.environ["MPG_COOLING_FORM"], os.environ["MPG_COOLING_LDS"]
    if C.metal is not None:
        eng.set_metal_cooling_table(*R.synthetic_metal_table())
    else:
        eng.set_metal_cooling_table()


def bind(torch, eng, d, n):
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a[:n])).cuda()
    pos = torch.from_numpy(np.random.RandomState(1).uniform(0, 1, (n, 3))).cuda()
    keep = dict(pos=pos, mass=up(d["mass"]), type=up(d["type"]))
    eng.dev_bind_particles(keep["pos"], keep["mass"], 1.0, type=keep["type"])
    a = {k: up(d[k]) for k in ("density", "entropy", "ne", "sfr", "metallicity", "heiii_ionized", "tb_hydro") if d.get(k) is not None}
    return a, keep


def compare(d, res, out, evals, stats, n, rows, label, bad=()):
    """`out`: entropy / ne / sfr after the call (numpy, n rows); `rows`: the listed rows; `bad`: rows expected to hit a limit"""
    listed = np.zeros(n, bool)
    listed[rows] = True
    treated = listed & (res["evals"][:n] >= 0)
    good = treated.copy()
    good[list(bad)] = False
    keep = ~good
    for k in ("entropy", "ne", "sfr"):                      # everything not treated successfully is as it was
        assert np.array_equal(out[k][keep], d[k][:n][keep]), (label, k)
    assert np.array_equal(evals[~treated], np.full(int((~treated).sum()), -1)), label
    assert (out["sfr"][good] == 0).all(), label
    e_ent = np.abs(out["entropy"][good] / res["entropy"][:n][good] - 1)
    e_ne = np.abs(out["ne"][good] - res["ne"][:n][good])
    miss = (e_ent > 1e-12) | (e_ne > 1e-10) | (evals[good] != res["evals"][:n][good])
    ng = int(good.sum())
    print("cooling %s: %d treated, %d miss; max |dEntropy| / 1e-12 = %.3g, max |dNe| / 1e-10 = %.3g; evaluations %d .. %d"
          % (label, ng, miss.sum(), (e_ent[~miss].max() if (~miss).any() else 0) / 1e-12, (e_ne[~miss].max() if (~miss).any() else 0) / 1e-10,
             res["evals"][:n][good].min() if ng else 0, res["evals"][:n][good].max() if ng else 0))
    assert miss.sum() <= 1e-3 * ng, (label, int(miss.sum()), ng)
    assert (e_ent[miss] <= 3e-6).all() and (np.abs(out["ne"][good][miss] / np.maximum(res["ne"][:n][good][miss], 1e-300) - 1) <= 3e-6).all(), label
    info = res["info"]
    g = np.nonzero(good)[0]
    assert stats["treated"] == int(treated.sum()) and stats["errors"] == len(bad)
    assert stats["reion"] == sum(info[i]["reion"] for i in g)
    if not miss.any():
        assert stats["evaluations"] == int(res["evals"][:n][good].sum()) + sum(int(evals[i]) for i in bad)
        assert stats["floor"] == sum(info[i]["floor"] for i in g)
        assert stats["bisections"] >= sum(info[i]["bisections"] for i in g)


def run_dev(torch, eng, d, times, step, n, active=None):
    a, keep = bind(torch, eng, d, n)
    act = None if active is None else torch.from_numpy(np.ascontiguousarray(active, np.int32)).cuda()
    nact = None
    if act is not None and len(active) == 0:
        hold = torch.zeros(1, dtype=torch.int32, device="cuda")          # an empty list with a pointer that is not NULL
        act, nact = hold.data_ptr(), 0
    err = None
    try:
        eng.dev_cooling(a, times, step, active=act, nactive=nact)
    except Exception as e:      # noqa: BLE001 - the caller decides whether an error return was expected
        err = e
    eng.synchronize()
    out = {k: a[k].cpu().numpy() for k in ("entropy", "ne", "sfr")}
    return out, eng.cooling_export(n), eng.cooling_stats(), err


# ---- mpg_dev_cooling against the restatement ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", R.CONFIGS)
def test_dev_form_against_restatement(pkg, name):
    """every setting (Verner96 / Sherwood at z = 3, 15 and 16, Cen92 / KWH92 at z = 0, Badnell06 / Enzo2Nyx at z = 2), NULL list, both kernel
    forms and both table placements"""
    import torch
    C, times, step, d, res = reference(name)
    n = K.SIZES[name]
    eng = pkg.Engine(0)
    T = sph_times(pkg, times)
    outs = []
    for form, lds in ((0, 0), (1, 0), (0, 1), (1, 1)):
        configure(eng, C, form, lds)
        out, evals, stats, err = run_dev(torch, eng, d, T, step, n)
        assert err is None, err
        compare(d, res, out, evals, stats, n, np.arange(n), "%s form %d lds %d" % (name, form, lds))
        outs.append((out, evals))
    for out, evals in outs[1:]:                              # the forms and placements do the same arithmetic
        assert np.array_equal(evals, outs[0][1])
        for k in ("entropy", "ne", "sfr"):
            assert np.array_equal(out[k], outs[0][0][k]), k
    eng.close()


def test_shapes_and_active_lists(pkg):
    """n = 1, 63, 64, 65 and 4099; a list that is NULL, empty, a strided subset and a permutation, with non-gas, garbage and massless rows in it"""
    import torch
    name = "sherwood_z16"
    C, times, step, d, res = reference(name)
    N = K.SIZES[name]
    assert N == 4099
    eng = pkg.Engine(0)
    T = sph_times(pkg, times)
    rs = np.random.RandomState(9)
    for form in (0, 1):
        configure(eng, C, form)
        for n in (1, 63, 64, 65):
            out, evals, stats, err = run_dev(torch, eng, d, T, step, n)
            assert err is None, err
            compare(d, res, out, evals, stats, n, np.arange(n), "n = %d form %d" % (n, form))
        lists = dict(empty=np.zeros(0, np.int32), strided=np.arange(3, N, 7, dtype=np.int32), permutation=rs.permutation(N).astype(np.int32))
        for what, act in lists.items():
            skipped = (d["type"][act] != 0) | ~(d["mass"][act] > 0)
            assert what == "empty" or ((d["type"][act] == 7).any() and (d["type"][act] == 1).any() and (d["mass"][act] <= 0).any() and skipped.sum() > 20)
            out, evals, stats, err = run_dev(torch, eng, d, T, step, N, active=act)
            assert err is None, err
            compare(d, res, out, evals, stats, N, act, "%s list form %d" % (what, form))
            if what == "empty":
                assert stats["treated"] == 0 and stats["evaluations"] == 0
    eng.close()


# ---- the network alone ----------------------------------------------------------------------------------------------------------------------
def test_cooling_state_known_answers(pkg):
    """mpg_dev_cooling_state at the scalar known answers of test_cooling_rates.c, at that file's tolerances"""
    import torch
    tc = R.TreeCool(G["treecool"])
    eng = pkg.Engine(0)
    f8 = lambda *x: torch.tensor(x, dtype=torch.float64, device="cuda")

    def state(C, uvbg, rho, u, ne, redshift, helium=0.0):
        r, uu, x = f8(*rho), f8(*u), f8(*ne)
        lam, temp, nh0 = torch.zeros_like(r), torch.zeros_like(r), torch.zeros_like(r)
        eng.dev_cooling_state(r, uu, x, dict(uvbg=uvbg, redshift=redshift, helium=helium), lambdanet=lam, temp=temp, nh0=nh0)
        eng.synchronize()
        return lam.cpu().numpy(), temp.cpu().numpy(), nh0.cpu().numpy(), x.cpu().numpy()

    # test_rate_network (:119-170): Verner96 / Sherwood, self-shielding, z = 2
    C = R.Cooling(R.default_params(), tc)
    eng.set_cooling_params(C.p)
    uvbg = C.get_global_UVBG(2)
    for dens, helium, tol in G["equilib_ne"]:
        _, _, _, ne = state(C, uvbg, [dens], [200. * 1e10], [1.0], 2, helium)
        assert abs(ne[0] - (1 + 2 * helium / (1 - helium) / 4)) < tol
    _, temp, nh0, ne = state(C, uvbg, [1e-4, 1e-4, 1.0, 1e-4, 1e-5, 1e-6, 1.0, 0.1], [200e10, 400e10, 200e10, 200e10, 200e10, 200e10, 100., 100e10], [1.0] * 8, 2)
    assert G["temp_window"][0] < temp[0] < G["temp_window"][1]
    assert abs(temp[1] / temp[0] - 2.) < 1e-3 and abs(temp[2] - 14700) < 200
    for k, dens in ((3, 1e-4), (4, 1e-5), (5, 1e-6)):
        assert abs(nh0[k] / dens - float(G["nh0_slope"])) < 1e-3
    assert nh0[6] > 0.95 and 0.735 < nh0[7] < 0.75
    # ... and the values agree with the restatement's far below those tolerances
    for k, (dens, u) in enumerate(((1e-4, 200e10), (1e-4, 400e10), (1.0, 200e10))):
        t_ref, ne_ref = C.get_temp(dens, u, 0.24, uvbg, 1.0)
        assert abs(temp[k] / t_ref - 1) < 1e-10 and abs(ne[k] - ne_ref) < 1e-10
    C0 = R.Cooling(R.default_params(SelfShieldingOn=0), tc)
    eng.set_cooling_params(C0.p)
    _, _, nh0, _ = state(C0, uvbg, [1.0, 0.1], [100e10, 100e10], [1.0, 1.0], 2)
    assert nh0[0] < 0.25 and nh0[1] < 0.05
    # test_heatingcooling_rate (:174-253): Cen92 / KWH92; ne carried from one call to the next as the reference does
    U, egyhot, cases = K.heatingcooling_cases()
    ne = 1.0
    for ss, with_uvbg, dens, u, (kind, want) in cases:
        Ck = R.Cooling(R.default_params(recomb=R.Cen92, cooling=R.KWH92, SelfShieldingOn=ss, **U), tc)
        eng.set_cooling_params(Ck.p)
        uv = Ck.get_global_UVBG(0) if with_uvbg else R.zero_uvbg()
        lam, _, _, x = state(Ck, uv, [dens], [u], [ne], 0)
        ne = float(x[0])
        if kind == "tcool":
            assert abs(egyhot / (-lam[0]) / U["tt_in_s"] / want - 1) < 1e-3
        elif kind == "lambda":
            assert abs(lam[0] / want - 1) < 1e-3
        else:
            assert lam[0] > 0
    eng.close()


def test_docooling_grid_through_dev_cooling(pkg):
    """the 400-point grid of test_cooling.c:220-239 through mpg_dev_cooling meets unew_table to 5e-3"""
    import torch
    par = R.default_params(recomb=R.Cen92, cooling=R.KWH92, SelfShieldingOn=0, MinGasTemp=0.0, sfr_MinGasTemp=1.0,
                           rho_crit_baryon=0.045 * 3.0 * math.pow(0.7 * R.HUBBLE, 2.0) / (8.0 * math.pi * R.GRAVITY))
    C = R.Cooling(par, R.TreeCool(G["treecool"]))
    NSTEP = 20
    dens = np.repeat(np.exp(np.log(1e-9) + np.arange(NSTEP) * (np.log(1e-2) - np.log(1e-9)) / 1. / NSTEP), NSTEP)
    uu = np.tile(np.exp(np.log(200) + np.arange(NSTEP) * (np.log(36000) - np.log(200)) / 1. / NSTEP), NSTEP)
    enttou = np.array([C.entropy_to_u(float(x), 1.0) for x in dens])
    n = NSTEP * NSTEP
    d = dict(type=np.zeros(n, np.uint8), mass=np.ones(n, np.float32), density=dens, entropy=uu / enttou, ne=np.ones(n), sfr=np.ones(n),
             heiii_ionized=np.ones(n, np.uint8))
    times = dict(atime=1.0, hubble=0.5, dloga_bin=np.full(47, 0.2 * 0.5))
    step = dict(uvbg=C.get_global_UVBG(0), long_mean_free_path_heating=0.0, lastred=0.0)
    eng = pkg.Engine(0)
    for form in (0, 1):
        configure(eng, C, form)
        out, evals, stats, err = run_dev(torch, eng, d, sph_times(pkg, times), step, n)
        assert err is None, err
        unew = out["entropy"] * enttou
        worst = np.abs(unew / G["unew_table"] - 1).max()
        print("DoCooling grid on the device, form %d: max |unew / unew_table - 1| = %.2e; evaluations %d .. %d" % (form, worst, evals.min(), evals.max()))
        assert worst < 5e-3 and (out["sfr"] == 0).all() and stats["treated"] == n
    eng.close()


# ---- the host form and the resident form ----------------------------------------------------------------------------------------------------
def test_host_form_equals_dev_form(pkg):
    """mpg_cooling on the 160-byte records (IsGarbage in the flags byte) with an active sublist: bit for bit the dev form"""
    import torch
    name = "sherwood_z3"
    C, times, step, d, res = reference(name)
    n = K.SIZES[name]
    act = np.arange(1, n, 2, dtype=np.int32)
    eng = pkg.Engine(0)
    configure(eng, C)
    T = sph_times(pkg, times)
    dev, evals, stats, err = run_dev(torch, eng, d, T, step, n, active=act)
    assert err is None, err
    compare(d, res, dev, evals, stats, n, act, "dev / sublist")
    P = pkg.make_particles(np.random.RandomState(1).uniform(0, 1, (n, 3)), d["mass"], type=np.where(d["type"] == 7, 0, d["type"]))
    P["Flags"][d["type"] == 7] = 1
    a = {k: d[k].copy() for k in ("density", "entropy", "ne", "sfr", "metallicity", "heiii_ionized", "tb_hydro")}
    eng.cooling(P, 1.0, a, T, step, ActiveParticle=act)
    assert np.array_equal(eng.cooling_export(n), evals)
    for k in ("entropy", "ne", "sfr"):
        assert np.array_equal(a[k], dev[k]), k
    for k in ("density", "metallicity", "heiii_ionized", "tb_hydro"):
        assert np.array_equal(a[k], d[k]), k
    eng.close()


def device_view(torch, ptr, n):
    class H:
        pass
    h = H()
    h.__cuda_array_interface__ = {"shape": (int(n),), "typestr": "<f8", "data": (int(ptr), False), "version": 2}
    return torch.as_tensor(h, device="cuda")


def test_resident_form_in_a_gas_stretch(pkg):
    """density -> hydro_force -> cooling inside a resident stretch (mpg_resident_sph_cooling: only ne and the optional inputs travel): the
    resident entropy column holds, bit for bit, what the dev form gives on the same density / entropy / ne; and the stretch goes on - density
    and hydro force after it equal those of a stretch whose entropy column was set to the same values by hand"""
    import torch
    pos, mass, typ, box = pkg.ics.hydro_pair(12)
    n = len(pos)
    C0, times, step, _, _ = reference("sherwood_z3")
    # the unit of density chosen so that the mean gas density of these initial conditions is 1e-3 protons / cm^3 (proper) at this redshift
    a3inv = 1. / times["atime"] ** 3
    meanrho = float(mass[typ == 0].sum()) / box ** 3
    C = R.Cooling(dict(C0.p, density_in_phys_cgs=1e-3 * R.PROTONMASS / (meanrho * a3inv)), R.TreeCool(G["treecool"]), C0.metal)
    rs = np.random.RandomState(21)
    u_target = np.exp(rs.uniform(np.log(1.0), np.log(3e6), n))
    T = sph_times(pkg, times)
    for b in range(47):
        T.hydrokicks[b] = T.gravkicks[b] = T.drifts[b] = T.dloga_kick[b] = 0.0
    T.FgravkickB = 0.0
    gas = typ == 0
    ne0 = rs.uniform(0, 1.2, n)
    Z = np.where(rs.uniform(size=n) < 0.5, rs.uniform(0, 1.5, n), 0.0)
    he = (rs.uniform(size=n) < 0.5).astype(np.uint8)
    tb = rs.randint(1, 47, n).astype(np.uint8)
    act = np.arange(0, n, 3, dtype=np.int32)
    outs = []
    for by_hand in (False, True):
        eng = pkg.Engine(0)
        configure(eng, C)
        eng.set_gravshort_treepar()
        eng.gravshort_set_softenings(box / 12)
        eng.set_densitypar(1.0, 2.0, 2.0, 99999., pkg.engine.DENSITY_KERNEL_QUINTIC_SPLINE, 0.006)
        eng.set_hydropar(0, 100.0, 0.75)
        z = lambda *s: np.zeros(s)
        P = pkg.make_particles(pos, mass, type=typ)
        a = dict(hsml=z(n), dthsml=z(n), vel=z(n, 3), gacc=z(n, 3), gpm=z(n, 3), entropy=np.ones(n),
                 density=z(n), egywtdensity=z(n), dhsmlegyfac=z(n), divvel=z(n), curlvel=z(n), hydroacc_out=z(n, 3), dtentropy_out=z(n), maxsignalvel=z(n),
                 tb_grav=tb.copy(), tb_hydro=tb.copy())
        eng.set_init_hsml(P, box, a, box / 12)
        eng.resident_begin(P, box)
        eng.resident_sph_begin(P, a)
        eng.density(P, box, a, T)
        eng.hydro_force(P, a, T)
        ptr = eng.resident_sph_arrays()
        d_ent, d_rho = device_view(torch, ptr["entropy"], n), device_view(torch, ptr["density"], n)
        # entropies that mean u = 1 .. 3e6 at the densities the loop found (the same values in both runs)
        d_ent.copy_(torch.where(d_rho > 0, torch.from_numpy(u_target).cuda() * R.GAMMA_MINUS1 / (d_rho.clamp(min=1e-300) * a3inv) ** R.GAMMA_MINUS1, d_ent))
        if not by_hand:
            ent0, rho0 = d_ent.clone(), d_rho.clone()
            ne = ne0.copy()
            eng.resident_sph_cooling(P, T, step, ne, metallicity=Z, heiii_ionized=he, ActiveParticle=act)
            evals, stats = eng.cooling_export(n), eng.cooling_stats()
            ent1 = d_ent.clone()
            # the dev form on copies of what the stretch held (the bound table is the resident one)
            up = lambda x: torch.from_numpy(x).cuda()
            c = dict(density=rho0, entropy=ent0.clone(), ne=up(ne0), sfr=torch.ones(n, dtype=torch.float64, device="cuda"), metallicity=up(Z),
                     heiii_ionized=up(he), tb_hydro=up(tb))
            eng.dev_cooling(c, T, step, active=up(act))
            eng.synchronize()
            assert stats["treated"] == int(gas[act].sum()) > 100 and stats["errors"] == 0 and stats["evaluations"] > 20 * stats["treated"]
            assert np.array_equal(eng.cooling_export(n), evals)
            assert torch.equal(c["entropy"], ent1) and np.array_equal(c["ne"].cpu().numpy(), ne)
            changed = (ent1 != ent0).cpu().numpy()
            assert changed[act][gas[act]].sum() > 100 and not changed[np.setdiff1d(np.arange(n), act)].any() and not changed[~gas].any()
            # ... and against the restatement on those columns
            dd = dict(type=typ.astype(np.uint8), mass=mass.astype(np.float32), density=rho0.cpu().numpy(), entropy=ent0.cpu().numpy(), ne=ne0, sfr=np.ones(n),
                      metallicity=Z, heiii_ionized=he, tb_hydro=tb)
            res = R.cool_particles(C, dd, times, step, active=act)
            compare(dd, res, dict(entropy=ent1.cpu().numpy(), ne=ne, sfr=c["sfr"].cpu().numpy()), evals, stats, n, act, "resident / sublist")
            keep_ent = ent1
        else:
            d_ent.copy_(keep_ent)
        eng.density(P, box, a, T)
        eng.hydro_force(P, a, T)
        eng.resident_sph_end(a)
        eng.resident_end(P)
        outs.append({k: a[k].copy() for k in ("entropy", "hsml", "density", "egywtdensity", "dhsmlegyfac", "divvel", "hydroacc_out", "dtentropy_out", "maxsignalvel")})
        eng.close()
    assert np.array_equal(outs[0]["entropy"], keep_ent.cpu().numpy())          # the stretch hands the cooled entropies back
    for k in outs[0]:
        assert np.array_equal(outs[0][k], outs[1][k]), k


# ---- errors ---------------------------------------------------------------------------------------------------------------------------------
def test_iteration_limit_is_an_error_return(pkg):
    """a particle that exhausts the network's iteration limit (finite input; the limit lowered through the test-only member of
    mpg_cooling_params until exactly one particle of the set needs more): a non-zero return, stats errors == 1, that particle untouched,
    every other particle correct; the next call without the limit succeeds"""
    import torch
    name = "sherwood_reion"
    C, times, step, d, res = reference(name)
    n = K.SIZES[name]
    order = np.argsort(res["maxfp"])
    worst, kmax = int(order[-1]), int(res["maxfp"][order[-1]])
    limit = kmax - 1
    assert limit >= 8
    # rows that tie with it are taken out of the list; everybody else needs at most `limit` iterations and never sees the limit
    act = np.array([i for i in range(n) if i == worst or res["maxfp"][i] <= limit], np.int32)
    assert len(act) > n - 10
    Climited = R.Cooling(dict(C.p, test_network_maxiter=limit), R.TreeCool(G["treecool"]))
    r1 = R.cool_particles(Climited, {k: v[[worst]] for k, v in d.items()}, times, step)
    assert r1["failed"] == [0]                                # the restatement fails on it too
    eng = pkg.Engine(0)
    T = sph_times(pkg, times)
    for form in (0, 1):
        configure(eng, C, form, test_network_maxiter=limit)
        out, evals, stats, err = run_dev(torch, eng, d, T, step, n, active=act)
        assert isinstance(err, pkg.EngineError) and "iteration limit" in str(err)
        assert stats["errors"] == 1 and evals[worst] >= 2 * limit      # (it may fail in its very first solve: two evaluations per iteration)
        compare(d, res, out, evals, stats, n, act, "limit %d form %d" % (limit, form), bad=[worst])
        configure(eng, C, form)
        out, evals, stats, err = run_dev(torch, eng, d, T, step, n, active=act)
        assert err is None, err
        compare(d, res, out, evals, stats, n, act, "after the error, form %d" % form)
    # a missing required array and missing parameters are error returns too
    a, keep = bind(torch, eng, d, n)
    for missing in ("density", "entropy", "ne", "sfr"):
        with pytest.raises(pkg.EngineError, match="required"):
            eng.dev_cooling(dict(a, **{missing: None}), T, step)
    e2 = pkg.Engine(0)
    e2.dev_bind_particles(keep["pos"], keep["mass"], 1.0, type=keep["type"])
    with pytest.raises(pkg.EngineError, match="mpg_set_cooling_params"):
        e2.dev_cooling(a, T, step)
    with pytest.raises(pkg.EngineError, match="recomb"):
        e2.set_cooling_params(dict(C.p, recomb=5))
    e2.close()
    eng.close()


# ---- no side effects ------------------------------------------------------------------------------------------------------------------------
def test_gravity_and_sph_unchanged_by_a_cooling_call(pkg):
    """a gravity step (PM force, tree build, walk) and a density -> hydro sequence before and after a cooling call on other arrays: bit-equal"""
    import torch
    pos, mass, typ, box = pkg.ics.hydro_pair(12)
    n = len(pos)
    C, times, step, d, res = reference("kwh_z0")
    T = pkg.SphTimes()
    T.atime, T.hubble = 0.5, 0.3
    for b in range(47):
        T.dloga_bin[b] = 0.01
    eng = pkg.Engine(0)
    eng.gravshort_fill_ntab(0, 1.5)
    eng.gravpm_init_periodic(box, 1.5, 32, 43.0071)
    eng.set_gravshort_treepar(TreeUseBH=1)      # (the Barnes-Hut opening on every walk: a walk does not depend on the one before it)
    eng.gravshort_set_softenings(box / 12)
    eng.set_densitypar(1.0, 2.0, 2.0, 99999., pkg.engine.DENSITY_KERNEL_QUINTIC_SPLINE, 0.006)
    eng.set_hydropar(0, 100.0, 0.75)
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()
    keep = dict(pos=up(pos), mass=up(mass), type=up(typ))
    z = lambda *s: torch.zeros(*s, dtype=torch.float64, device="cuda")

    def gravity_and_sph():
        eng.dev_bind_particles(keep["pos"], keep["mass"], box, type=keep["type"])
        gpm, acc, pot = z(n, 3), z(n, 3), z(n)
        eng.dev_gravpm_force(gpm, None)
        eng.dev_force_tree_build()
        eng.dev_grav_short_tree(acc, potential=pot)
        a = dict(hsml=z(n), dthsml=z(n), vel=z(n, 3), entropy=torch.ones(n, dtype=torch.float64, device="cuda"), density=z(n), egywtdensity=z(n),
                 dhsmlegyfac=z(n), divvel=z(n), curlvel=z(n), hydroacc_out=z(n, 3), dtentropy_out=z(n), maxsignalvel=z(n))
        eng.dev_force_tree_rebuild_mask(pkg.engine.GASMASK + pkg.engine.BHMASK, with_moments=True)
        eng.dev_set_init_hsml(a, box / 12)
        eng.dev_force_tree_rebuild_mask(pkg.engine.GASMASK)
        eng.dev_density(a, T)
        eng.dev_force_tree_calc_hmax()
        eng.dev_hydro_force(a, T)
        eng.synchronize()
        r = {k: a[k].cpu().numpy().copy() for k in ("hsml", "density", "divvel", "hydroacc_out", "dtentropy_out", "maxsignalvel")}
        r.update(acc=acc.cpu().numpy().copy(), pot=pot.cpu().numpy().copy())
        return r

    before = gravity_and_sph()
    configure(eng, C)
    m = K.SIZES["kwh_z0"]
    out, evals, stats, err = run_dev(torch, eng, d, sph_times(pkg, times), step, m)
    assert err is None and stats["treated"] > 300
    compare(d, res, out, evals, stats, m, np.arange(m), "between two gravity steps")
    after = gravity_and_sph()
    for k in before:
        # (the PM force itself sums with atomics and differs in the last bits from run to run; the walk, the tree and the SPH loops do not)
        assert np.array_equal(before[k], after[k]), k
    eng.close()
