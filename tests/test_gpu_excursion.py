"""GPU tests of the excursion set's consumer in cooling and star formation (get_local_UVBG_from_J21 / get_local_UVBG,
cooling_uvfluc.c:199-246, in csrc/cooling.hip and csrc/sfr.hip) against the plain-Python restatement tests/excursion_restated.py, which
tests/test_excursion_restated.py pins and whose input sets it shows to hold every class of row inside every wave.

The background of a point: the four rates, J_UV and zreion are correctly rounded products in the reference's order, so they are held to the
restatement's bits.  self_shield_dens is held to 20 * 2^-53 relative: the device library's pow is within 16 ulp (OpenCL's limit for pow,
which is what it promises), and three products follow it.  Everything downstream is compared as tests/test_gpu_cooling.py and
tests/test_gpu_sfr.py compare it, with their functions imported unchanged; the class of a row cannot differ between the two sides, because
zreion is input data with the same bits on both."""
import numpy as np
import pytest

import cooling_restated as R
import excursion_restated as X
import sfr_restated as SF
import test_cooling_restated as K
import test_gpu_cooling as TC
import test_gpu_sfr as TS
import test_gpu_uvbg as TU
import uvbg_restated as UR
import uvfluc_restated as U

pytestmark = pytest.mark.gpu

G = K.G
COOL_COLUMNS = ("density", "entropy", "ne", "sfr", "metallicity", "heiii_ionized", "tb_hydro")
SSD_BOUND = 20 * 2.0 ** -53
_cool, _sfr = {}, {}


def cooling_reference(name):
    """a cooling set and its restatement, computed once: every list of the tests is a selection of its rows"""
    if name not in _cool:
        C, times, step, d, par, exc, J21, zre, cls = X.cooling_set(name, G["treecool"])
        res = X.cool_particles_j21(C, exc, d, J21, zre, times, step)
        assert not res["failed"]
        _cool[name] = (C, times, step, d, par, exc, J21, zre, cls, res)
    return _cool[name]


def sfr_reference():
    if not _sfr:
        S, times, step, d, par, exc, J21, zre, cls = X.sfr_set(G["treecool"])
        res = X.cooling_and_starformation_j21(S, exc, d, J21, zre, times, step, SF.random_table(), wind=SF.WIND)
        assert not res["failed"]
        _sfr["x"] = (S, times, step, d, par, exc, J21, zre, cls, res)
    return _sfr["x"]


def up(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a).copy()).cuda()


def first_rows(res, n):
    return {k: (v[:n] if isinstance(v, np.ndarray) else v) for k, v in res.items()}


def run_cooling(torch, eng, d, T, step, J21=None, zre=None, active=None, pos=None, box=1.0):
    """bind the table, then the two columns (they are bound for the table bound at that moment), then mpg_dev_cooling"""
    n = len(d["type"])
    keep = dict(pos=up(torch, np.random.RandomState(1).uniform(0, 1, (n, 3)) if pos is None else pos), mass=up(torch, d["mass"]), type=up(torch, d["type"]))
    eng.dev_bind_particles(keep["pos"], keep["mass"], box, type=keep["type"])
    if J21 is not None:
        keep["J21"], keep["zre"] = up(torch, J21), up(torch, zre)
        eng.dev_set_excursion_columns(keep["J21"], keep["zre"])
    a = {k: up(torch, d[k]) for k in COOL_COLUMNS if d.get(k) is not None}
    act, nact = None, None
    if active is not None:
        act = up(torch, np.asarray(active, np.int32))
        if len(active) == 0:
            keep["hold"] = torch.zeros(1, dtype=torch.int32, device="cuda")      # an empty list with a pointer that is not NULL
            act, nact = keep["hold"].data_ptr(), 0
    err = None
    try:
        eng.dev_cooling(a, T, step, active=act, nactive=nact)
    except Exception as e:      # noqa: BLE001 - the caller decides whether an error return was expected
        err = e
    eng.synchronize()
    return {k: a[k].cpu().numpy() for k in ("entropy", "ne", "sfr")}, eng.cooling_export(n), eng.cooling_stats(), err


def same_bits(a, b, label):
    assert a[3] is None and b[3] is None, (label, a[3], b[3])
    assert a[2] == b[2] and np.array_equal(a[1], b[1]), label
    for k in ("entropy", "ne", "sfr"):
        assert np.array_equal(a[0][k], b[0][k]), (label, k)


# ---- 1. the point entry -----------------------------------------------------------------------------------------------------------------------
def test_point_entry(pkg):
    """mpg_dev_excursion_uvbg on 4099 points at z = 3 (grey opacity tabulated), 15 and 16 (clamped), then at and below ExcursionSetZStop and
    with ExcursionSetReionOn = 0"""
    import torch
    C, times, step, d, par, exc, _, _, _ = X.cooling_set("sherwood_z3", G["treecool"])
    n = 4099
    assert n % 64 != 0
    rs = np.random.RandomState(5)
    J21 = np.exp(rs.uniform(np.log(1e-6), np.log(1e3), n))
    J21[:7] = [0.0, 5e-324, 1e-310, 1e-30, 1e3, 1.0, 0.0]
    zre = rs.uniform(2.0, 20.0, n)
    zre[[0, 6]] = -1.0
    eng = pkg.Engine(0)
    TC.configure(eng, C)
    eng.set_excursion_set(par)
    dJ, dz = up(torch, J21), up(torch, zre)
    worst = 0.0
    for redshift in (3.0, 15.0, 16.0):
        out = torch.full((n, 9), -7.0, dtype=torch.float64, device="cuda")
        eng.dev_excursion_uvbg(dJ, dz, redshift, out, uvbg=step["uvbg"])
        eng.synchronize()
        got = out.cpu().numpy()
        want = np.array([[X.get_local_UVBG_from_J21(C, exc, redshift, float(J21[i]), float(zre[i]))[k] for k in X.UVBG_MEMBERS] for i in range(n)])
        for c, k in enumerate(X.UVBG_MEMBERS):
            if k != "self_shield_dens":
                assert np.array_equal(got[:, c], want[:, c]), (redshift, k)
        dark = want[:, X.UVBG_MEMBERS.index("gJH0")] == 0
        s = X.UVBG_MEMBERS.index("self_shield_dens")
        assert dark[:2].all() and not dark[2] and dark[6] and (got[dark, s] == 1e10).all() and (want[dark, s] == 1e10).all()
        rel = np.abs(got[~dark, s] / want[~dark, s] - 1)
        worst = max(worst, rel.max())
        print("self_shield_dens at z = %g: max relative difference %.3g = %.2f of the bound" % (redshift, rel.max(), rel.max() / SSD_BOUND))
        assert (rel <= SSD_BOUND).all()
    print("self_shield_dens: largest relative difference %.3g (%.2f * 2^-53)" % (worst, worst / 2.0 ** -53))
    # at or below ExcursionSetZStop, and with the model switched off: the global background for every point
    g = np.array([step["uvbg"][k] for k in X.UVBG_MEMBERS])
    for over, redshift in ((dict(ExcursionSetZStop=3.0), 3.0), (dict(ExcursionSetZStop=3.0), 2.5), (dict(ExcursionSetReionOn=0), 15.0)):
        eng.set_excursion_set(dict(par, **over))
        out = torch.zeros((n, 9), dtype=torch.float64, device="cuda")
        eng.dev_excursion_uvbg(dJ, dz, redshift, out, uvbg=step["uvbg"])
        eng.synchronize()
        assert (out.cpu().numpy() == g[None, :]).all(), over
    # a point without a background: NaN for it alone, a non-zero return
    eng.set_excursion_set(par)
    bad = J21.copy()
    bad[70], bad[71] = np.nan, -1.0
    zb = zre.copy()
    zb[200] = np.nan
    ref = torch.zeros((n, 9), dtype=torch.float64, device="cuda")
    eng.dev_excursion_uvbg(dJ, dz, 3.0, ref, uvbg=step["uvbg"])
    out = torch.zeros((n, 9), dtype=torch.float64, device="cuda")
    with pytest.raises(pkg.EngineError, match="3 point"):
        eng.dev_excursion_uvbg(up(torch, bad), up(torch, zb), 3.0, out, uvbg=step["uvbg"])
    eng.synchronize()
    got, want = out.cpu().numpy(), ref.cpu().numpy()
    rows = np.zeros(n, bool)
    rows[[70, 71, 200]] = True
    assert np.isnan(got[rows]).all() and np.array_equal(got[~rows], want[~rows])
    # the setter's refusals
    for over, text in ((dict(gJH0=np.nan), "gJH0"), (dict(epsHe0=-1.0), "epsHe0"), (dict(gJHep=np.inf), "gJHep"), (dict(ExcursionSetZStop=np.inf), "ExcursionSetZStop")):
        with pytest.raises(pkg.EngineError, match=text):
            eng.set_excursion_set(dict(par, **over))
    eng.close()


# ---- 2. the cooling ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(X.COOLING_SETS))
def test_cooling_with_the_columns(pkg, name):
    """both kernel forms and both table placements against the restatement and against each other; an active sub-list and an empty list;
    ExcursionSetZStop above the redshift and the model removed are the engine that never had one"""
    import torch
    C, times, step, d, par, exc, J21, zre, cls, res = cooling_reference(name)
    n = len(d["type"])
    redshift = 1. / times["atime"] - 1
    T = TC.sph_times(pkg, times)
    eng = pkg.Engine(0)
    eng.set_excursion_set(par)
    window = int(sum(res["info"][p]["reion"] for p in res["info"]))
    runs = []
    for form, lds in ((0, 0), (1, 0), (0, 1), (1, 1)):
        TC.configure(eng, C, form, lds)
        r = run_cooling(torch, eng, d, T, step, J21, zre)
        assert r[3] is None, r[3]
        assert r[2]["reion"] == window and (window > 50 if name == "sherwood_reion" else window == 0)
        TC.compare(d, res, r[0], r[1], r[2], n, np.arange(n), "%s with J21, form %d lds %d" % (name, form, lds))
        runs.append(r)
    for r in runs[1:]:                                          # the forms and placements do the same arithmetic
        same_bits(r, runs[0], name)
    for form in (0, 1):
        TC.configure(eng, C, form)
        for what, act in (("strided", np.arange(3, n, 7, dtype=np.int32)), ("empty", np.zeros(0, np.int32))):
            out, evals, stats, err = run_cooling(torch, eng, d, T, step, J21, zre, active=act)
            assert err is None, err
            TC.compare(d, res, out, evals, stats, n, act, "%s with J21, %s list form %d" % (name, what, form))
            if what == "empty":
                assert stats["treated"] == 0 and stats["evaluations"] == 0
            else:
                listed = np.zeros(n, bool)
                listed[act] = True
                for k in ("entropy", "ne", "sfr"):
                    assert np.array_equal(out[k][listed], runs[0][0][k][listed]), k
    # an engine that never had a model; then ExcursionSetZStop above the redshift; then the model removed
    TC.configure(eng, C)
    fresh = pkg.Engine(0)
    TC.configure(fresh, C)
    plain = run_cooling(torch, fresh, d, T, step)
    fresh.close()
    treated = res["evals"] >= 0
    differ = (plain[0]["entropy"] != runs[0][0]["entropy"]) | (plain[0]["ne"] != runs[0][0]["ne"])
    print("%s: %d of %d treated rows differ from the engine without a model" % (name, differ[treated].sum(), treated.sum()))
    assert differ[treated].sum() >= 0.10 * treated.sum() and not differ[~treated].any()
    eng.set_excursion_set(dict(par, ExcursionSetZStop=redshift + 1.0))
    same_bits(run_cooling(torch, eng, d, T, step, J21, zre), plain, "ZStop above the redshift")
    eng.set_excursion_set(dict(par, ExcursionSetZStop=redshift))                       # (redshift > ZStop is false at the redshift itself)
    same_bits(run_cooling(torch, eng, d, T, step, J21, zre), plain, "ZStop at the redshift")
    eng.set_excursion_set()
    same_bits(run_cooling(torch, eng, d, T, step, J21, zre), plain, "model removed")
    eng.close()


def test_table_below_zstop_columns_above(pkg):
    """with a UV-fluctuation table loaded as well: the table governs at or below ExcursionSetZStop, the J21 columns above it"""
    import torch
    C, times, step, d, par, exc, J21, zre, cls, res = cooling_reference("sherwood_z3")
    n = 260
    dd = {k: v[:n] for k, v in d.items()}
    pos = U.positions(n)
    uvf = U.UVF(U.synthetic_zreion_table(U.NSIDE, 3.0, 4), U.BOXSIZE)
    by_table = U.cool_particles_local(C, dd, pos, U.OFFSET, uvf, times, step)
    assert not by_table["failed"]
    T = TC.sph_times(pkg, times)
    eng = pkg.Engine(0)
    eng.set_uvf_table(np.array(uvf.Table).reshape((uvf.Nside,) * 3), U.BOXSIZE)
    eng.set_uvf_offset(U.OFFSET)
    for form in (0, 1):
        TC.configure(eng, C, form)
        eng.set_excursion_set(par)                                                     # ZStop = 2 < z = 3
        out, evals, stats, err = run_cooling(torch, eng, dd, T, step, J21[:n], zre[:n], pos=pos, box=U.BOXSIZE)
        assert err is None, err
        TC.compare(dd, first_rows(res, n), out, evals, stats, n, np.arange(n), "table and columns, z above ZStop, form %d" % form)
        eng.set_excursion_set(dict(par, ExcursionSetZStop=3.0))
        out2, evals2, stats2, err = run_cooling(torch, eng, dd, T, step, J21[:n], zre[:n], pos=pos, box=U.BOXSIZE)
        assert err is None, err
        TC.compare(dd, by_table, out2, evals2, stats2, n, np.arange(n), "table and columns, z at ZStop, form %d" % form)
        assert (out2["entropy"] != out["entropy"]).sum() > 50
    eng.close()


# ---- 3. star formation ------------------------------------------------------------------------------------------------------------------------
def configure_sfr(eng, S, par):
    eng.set_cooling_params(S.C.p)
    eng.set_metal_cooling_table(*R.synthetic_metal_table())
    eng.set_random_table(SF.random_table())
    eng.set_wind_params(SF.WIND)
    eng.set_excursion_set(par)
    eng.set_sfr_params(dict(SF.engine_params(S.p), ExcursionSetReion=int(par is not None)))


def sfr_out(eng, columns, n):
    out = {k: columns[k] for k in TS.IO + ("stellarmass",)}
    out["cls"], out["sfevals"] = eng.sfr_export_rows(n)
    out["evals"] = eng.cooling_export(n)
    out.update(eng.sfr_export())
    out["result"], out["stats"], out["cooling_stats"] = eng.sfr_result(), eng.sfr_stats(), eng.cooling_stats()
    return out


def test_star_formation_three_forms(pkg):
    """the `heating` set with BHFeedbackUseTcool = 3 through the device, host and resident forms: columns, both lists in list order and the
    sums against the restatement at the tolerances of tests/test_gpu_sfr.py"""
    import torch
    S, times, step, d, par, exc, J21, zre, cls, res = sfr_reference()
    n = len(d["type"])
    T = TS.sph_times(pkg, times)
    eng = pkg.Engine(0)
    configure_sfr(eng, S, par)
    a, keep = TS.bind(torch, eng, d, n)
    dJ, dz = up(torch, J21), up(torch, zre)
    eng.dev_set_excursion_columns(dJ, dz)
    eng.dev_cooling_and_starformation(a, T, step)
    eng.synchronize()
    dev = sfr_out(eng, {k: a[k].cpu().numpy() for k in TS.IO + ("stellarmass",)}, n)
    TS.compare(d, res, dev, n, "heating with J21, device form")
    assert dev["result"]["sum_sf_part"] == res["sum_sf_part"] > 100 and dev["result"]["cooled"] > 100
    eng.dev_set_excursion_columns()
    # the host form: the columns travel with the call
    pos = np.random.RandomState(1).uniform(0, 1, (n, 3))
    P = pkg.make_particles(pos, d["mass"], type=np.where(d["type"] == 7, 0, d["type"]))
    P["Flags"][d["type"] == 7] = 1
    h = TS.host_columns(d, n)
    eng.set_excursion_columns(J21, zre)
    eng.cooling_and_starformation(P, 1.0, h, T, step)
    host = sfr_out(eng, h, n)
    TS.compare(d, res, host, n, "heating with J21, host form")
    for k in TS.IO + ("stellarmass", "parent", "spawn", "mass_of_star", "maybewind"):
        assert np.array_equal(host[k], dev[k]), k
    eng.set_excursion_columns()
    eng.close()
    # the resident form: a gas stretch whose Density / Entropy / TimeBinHydro / Hsml / DivVel / CurlVel columns hold the table's
    eng = pkg.Engine(0)
    configure_sfr(eng, S, par)
    eng.set_gravshort_treepar()
    eng.gravshort_set_softenings(1.0 / 12)
    eng.set_densitypar(1.0, 2.0, 2.0, 99999., pkg.engine.DENSITY_KERNEL_QUINTIC_SPLINE, 0.006)
    eng.set_hydropar(0, 100.0, 0.75)
    z = lambda *s: np.zeros(s)
    sph = dict(hsml=d["hsml"].copy(), dthsml=z(n), vel=z(n, 3), gacc=z(n, 3), gpm=z(n, 3), entropy=d["entropy"].copy(), density=d["density"].copy(),
               egywtdensity=z(n), dhsmlegyfac=z(n), divvel=d["divvel"].copy(), curlvel=d["curlvel"].copy(), hydroacc_out=z(n, 3), dtentropy_out=z(n),
               maxsignalvel=z(n), tb_grav=d["tb_hydro"].copy(), tb_hydro=d["tb_hydro"].copy())
    eng.resident_begin(P, 1.0)
    eng.resident_sph_begin(P, sph)
    ptr = eng.resident_sph_arrays()
    d_ent, d_rho = TS.device_view(torch, ptr["entropy"], n), TS.device_view(torch, ptr["density"], n)
    d_rho.copy_(torch.from_numpy(d["density"]).cuda())
    d_ent.copy_(torch.from_numpy(d["entropy"]).cuda())
    r = TS.host_columns(d, n)
    for k in ("density", "entropy", "tb_hydro", "hsml", "divvel", "curlvel"):           # the resident columns: not read from the host
        r[k] = None
    eng.resident_sph_set_excursion_columns(J21, zre)
    eng.resident_sph_cooling_and_starformation(P, r, T, step)
    resident = sfr_out(eng, dict(r, entropy=d_ent.cpu().numpy()), n)
    TS.compare(d, res, resident, n, "heating with J21, resident form")
    for k in TS.IO + ("stellarmass", "parent", "spawn", "mass_of_star", "maybewind"):
        assert np.array_equal(resident[k], dev[k]), k
    eng.resident_sph_end(sph)
    eng.resident_end(P)
    # the columns of the stretch ended with it
    with pytest.raises(pkg.EngineError, match="no local_J21 / zreion columns are bound"):
        eng.cooling_and_starformation(P, 1.0, TS.host_columns(d, n), T, step)
    eng.close()


# ---- 4. producer into consumer ----------------------------------------------------------------------------------------------------------------
def test_calculate_uvbg_into_cooling(pkg):
    """mpg_dev_calculate_uvbg at UVBGdim 8 on the 16^3 scene of tests/test_gpu_uvbg.py, its two output tensors bound as they are, then
    mpg_dev_cooling: the result is the restatement's on the exported columns.  No host array is passed."""
    import torch
    C, times, step, make = R.config("sherwood_reion", G["treecool"])
    S = UR.scene("d16", UVBGdim=8, Time=times["atime"])
    n = S["n"]
    d = make(n)
    d["type"], d["mass"] = S["type"].copy(), np.asarray(S["mass"], np.float32)
    par, exc = X.model(5.0)
    eng = pkg.Engine(0)
    TC.configure(eng, C)
    eng.set_excursion_set(par)
    keep = TU.bind(eng, S)
    cols = {k: TU.dev(v) for k, v in TU.columns(S).items()}
    eng.dev_calculate_uvbg(S["par"], cols)
    eng.dev_set_excursion_columns(cols["local_J21"], cols["zreion"])
    a = {k: up(torch, d[k]) for k in COOL_COLUMNS if d.get(k) is not None}
    act = np.arange(0, n, 2, dtype=np.int32)
    eng.dev_cooling(a, TC.sph_times(pkg, times), step, active=up(torch, act))
    eng.synchronize()
    out, evals, stats = {k: a[k].cpu().numpy() for k in ("entropy", "ne", "sfr")}, eng.cooling_export(n), eng.cooling_stats()
    J21, zre = cols["local_J21"].cpu().numpy(), cols["zreion"].cpu().numpy()
    gas = d["type"] == 0
    redshift = 1. / times["atime"] - 1
    assert redshift == 15 and (gas & (J21 > 0)).sum() > 100 and (gas & (J21 == 0)).sum() > 100 and (gas & (zre == redshift)).sum() > 50
    res = X.cool_particles_j21(C, exc, d, J21, zre, times, step, active=act)
    assert not res["failed"]
    TC.compare(d, res, out, evals, stats, n, act, "calculate_uvbg into cooling")
    assert stats["reion"] > 25 and stats["treated"] > 1000
    del keep
    eng.close()


# ---- 5. errors and refusals -------------------------------------------------------------------------------------------------------------------
def test_error_rows_and_refusals(pkg):
    import torch
    C, times, step, d, par, exc, J21, zre, cls, res = cooling_reference("sherwood_reion")
    S = sfr_reference()[0]
    n = 130
    dd = {k: v[:n] for k, v in d.items()}
    T = TC.sph_times(pkg, times)
    eng = pkg.Engine(0)
    TC.configure(eng, C)
    before = run_cooling(torch, eng, dd, T, step)
    # the setting is refused without a model and accepted with one
    eng.set_random_table(SF.random_table())
    with pytest.raises(pkg.EngineError, match="EXCUR_REION.*mpg_set_excursion_set first"):
        eng.set_sfr_params(dict(SF.engine_params(S.p), ExcursionSetReion=1))
    eng.set_excursion_set(par)
    eng.set_sfr_params(dict(SF.engine_params(S.p), ExcursionSetReion=1))
    # no columns bound; columns bound for a table of another size
    out, evals, stats, err = run_cooling(torch, eng, dd, T, step)
    assert isinstance(err, pkg.EngineError) and "no local_J21 / zreion columns are bound" in str(err)
    for k in ("entropy", "ne", "sfr"):
        assert np.array_equal(out[k], dd[k]), k
    good = run_cooling(torch, eng, dd, T, step, J21[:n], zre[:n])
    assert good[3] is None
    TC.compare(dd, first_rows(res, n), good[0], good[1], good[2], n, np.arange(n), "130 rows")
    a, keep = TC.bind(torch, eng, d, n - 1)                                               # (the columns stay bound, for 130 rows)
    with pytest.raises(pkg.EngineError, match="bound for a table of 130 particles, this call is on 129"):
        eng.dev_cooling(a, T, step)
    eng.synchronize()
    for k in ("entropy", "ne", "sfr"):
        assert np.array_equal(a[k].cpu().numpy(), d[k][:n - 1]), k
    # one row with J21 = NaN, one with J21 = -1, one with zreion = NaN: error rows, the rest unchanged
    gas = np.nonzero(res["evals"][:n] >= 0)[0]
    victims = [int(gas[10]), int(gas[40]), int(gas[70])]
    bJ, bz = J21[:n].copy(), zre[:n].copy()
    bJ[victims[0]], bJ[victims[1]], bz[victims[2]] = np.nan, -1.0, np.nan
    for form in (0, 1):
        TC.configure(eng, C, form)
        out, evals, stats, err = run_cooling(torch, eng, dd, T, step, bJ, bz)
        assert isinstance(err, pkg.EngineError) and "local_J21" in str(err) and "3 particle" in str(err)
        assert stats["errors"] == 3 and (evals[victims] == 0).all()
        TC.compare(dd, first_rows(res, n), out, evals, stats, n, np.arange(n), "three rows without a background, form %d" % form, bad=victims)
        for k in ("entropy", "ne", "sfr"):
            keep = np.ones(n, bool)
            keep[victims] = False
            assert np.array_equal(out[k][keep], good[0][k][keep]), k
    # a plain call before and after all of this is bit-equal to itself
    TC.configure(eng, C)
    eng.set_excursion_set()
    eng.dev_set_excursion_columns()
    same_bits(run_cooling(torch, eng, dd, T, step), before, "plain call before and after")
    eng.close()


# ---- 6. the host and resident forms of the cooling --------------------------------------------------------------------------------------------
def test_host_and_resident_cooling_equal_dev_form(pkg):
    """mpg_cooling on the 160-byte records and mpg_resident_sph_cooling inside a resident gas stretch on 520 rows with an active sub-list:
    bit for bit the device form"""
    import torch
    C, times, step, d, par, exc, J21, zre, cls, res = cooling_reference("sherwood_reion")
    n = 520
    dd = {k: np.ascontiguousarray(v[:n]) for k, v in d.items()}
    J, Z = np.ascontiguousarray(J21[:n]), np.ascontiguousarray(zre[:n])
    act = np.arange(1, n, 2, dtype=np.int32)
    T = TC.sph_times(pkg, times)
    eng = pkg.Engine(0)
    TC.configure(eng, C)
    eng.set_excursion_set(par)
    dev, evals, stats, err = run_cooling(torch, eng, dd, T, step, J, Z, active=act)
    assert err is None, err
    TC.compare(dd, first_rows(res, n), dev, evals, stats, n, act, "device form / sublist")
    assert stats["treated"] > 150 and stats["reion"] > 10
    eng.dev_set_excursion_columns()
    pos = np.random.RandomState(1).uniform(0, 1, (n, 3))
    P = pkg.make_particles(pos, dd["mass"], type=np.where(dd["type"] == 7, 0, dd["type"]))
    P["Flags"][dd["type"] == 7] = 1
    a = {k: dd[k].copy() for k in COOL_COLUMNS if dd.get(k) is not None}
    eng.set_excursion_columns(J, Z)
    eng.cooling(P, 1.0, a, T, step, ActiveParticle=act)
    assert np.array_equal(eng.cooling_export(n), evals) and eng.cooling_stats() == stats
    for k in ("entropy", "ne", "sfr"):
        assert np.array_equal(a[k], dev[k]), k
    eng.set_excursion_columns()
    # the resident form
    eng.set_gravshort_treepar()
    eng.gravshort_set_softenings(1.0 / 12)
    eng.set_densitypar(1.0, 2.0, 2.0, 99999., pkg.engine.DENSITY_KERNEL_QUINTIC_SPLINE, 0.006)
    eng.set_hydropar(0, 100.0, 0.75)
    z = lambda *s: np.zeros(s)
    sph = dict(hsml=np.full(n, 0.05), dthsml=z(n), vel=z(n, 3), gacc=z(n, 3), gpm=z(n, 3), entropy=dd["entropy"].copy(), density=dd["density"].copy(),
               egywtdensity=z(n), dhsmlegyfac=z(n), divvel=z(n), curlvel=z(n), hydroacc_out=z(n, 3), dtentropy_out=z(n), maxsignalvel=z(n),
               tb_grav=dd["tb_hydro"].copy(), tb_hydro=dd["tb_hydro"].copy())
    eng.resident_begin(P, 1.0)
    eng.resident_sph_begin(P, sph)
    ptr = eng.resident_sph_arrays()
    d_ent, d_rho = TC.device_view(torch, ptr["entropy"], n), TC.device_view(torch, ptr["density"], n)
    d_rho.copy_(torch.from_numpy(dd["density"]).cuda())
    d_ent.copy_(torch.from_numpy(dd["entropy"]).cuda())
    ne = dd["ne"].copy()
    eng.resident_sph_set_excursion_columns(J, Z)
    eng.resident_sph_cooling(P, T, step, ne, metallicity=dd.get("metallicity"), heiii_ionized=dd["heiii_ionized"].copy(), ActiveParticle=act)
    assert np.array_equal(eng.cooling_export(n), evals) and eng.cooling_stats() == stats
    assert np.array_equal(d_ent.cpu().numpy(), dev["entropy"]) and np.array_equal(ne, dev["ne"])
    eng.resident_sph_end(sph)
    eng.resident_end(P)
    eng.close()
