"""GPU tests of patchy reionisation (the UV-fluctuation table of cooling_uvfluc.c:115-197 in csrc/cooling.hip and csrc/sfr.hip) against the
plain-Python restatement tests/uvfluc_restated.py, which tests/test_uvfluc_restated.py pins to the reference's assertions and whose input
sets it shows to hold every class of row, wrapped cells on both sides and no row on a decision.

The per-point read is held to 16 * 2^-52 * max|table| absolute.  The bound is derived, not measured: the cell and the fraction f are the
same bits on both sides (a subtraction, a division and a floor, each correctly rounded), so what remains is at most 11 roundings of relative
size 2^-53 on terms no larger than max|table| (1 - f, two products per weight, the product with the entry, seven additions whose partial sums
stay below max|table| because the weights are positive and sum to one); FMA contraction on the device only removes some.  At grid points
f = 0 and the result is the entry itself.  Everything downstream of the read is compared as tests/test_gpu_cooling.py and
tests/test_gpu_sfr.py compare it, with their functions imported unchanged."""
import numpy as np
import pytest

import cooling_restated as R
import sfr_restated as SF
import test_cooling_restated as K
import test_gpu_cooling as TC
import test_gpu_sfr as TS
import uvfluc_restated as U

pytestmark = pytest.mark.gpu

G = K.G
EPS = 2.0 ** -52
COOL_COLUMNS = ("density", "entropy", "ne", "sfr", "metallicity", "heiii_ionized", "tb_hydro")
_cool, _sfr = {}, {}


def cooling_reference(name):
    """a cooling set and its restatement, computed once: every list of the tests is a selection of its rows"""
    if name not in _cool:
        C, times, step, d, pos, uvf = U.cooling_set(name, G["treecool"])
        res = U.cool_particles_local(C, d, pos, U.OFFSET, uvf, times, step)
        assert not res["failed"]
        _cool[name] = (C, times, step, d, pos, uvf, res)
    return _cool[name]


def sfr_reference():
    if not _sfr:
        S, times, step, d, pos, uvf = U.sfr_set(G["treecool"])
        res = U.cooling_and_starformation_local(S, d, pos, U.OFFSET, uvf, times, step, SF.random_table(), wind=SF.WIND)
        assert not res["failed"]
        _sfr["x"] = (S, times, step, d, pos, uvf, res)
    return _sfr["x"]


def table_of(uvf):
    return np.array(uvf.Table).reshape((uvf.Nside,) * 3)


def bind_cooling(torch, eng, d, pos):
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    keep = dict(pos=up(pos), mass=up(d["mass"]), type=up(d["type"]))
    eng.dev_bind_particles(keep["pos"], keep["mass"], U.BOXSIZE, type=keep["type"])
    return {k: up(d[k]) for k in COOL_COLUMNS if d.get(k) is not None}, keep


def run_cooling(torch, eng, d, pos, T, step, active=None):
    a, keep = bind_cooling(torch, eng, d, pos)
    act, nact = None, None
    if active is not None:
        act = torch.from_numpy(np.ascontiguousarray(active, np.int32)).cuda()
        if len(active) == 0:
            hold = torch.zeros(1, dtype=torch.int32, device="cuda")      # an empty list with a pointer that is not NULL
            act, nact = hold.data_ptr(), 0
    err = None
    try:
        eng.dev_cooling(a, T, step, active=act, nactive=nact)
    except Exception as e:      # noqa: BLE001 - the caller decides whether an error return was expected
        err = e
    eng.synchronize()
    n = len(d["type"])
    return {k: a[k].cpu().numpy() for k in ("entropy", "ne", "sfr")}, eng.cooling_export(n), eng.cooling_stats(), err


def check_export(z, res, rows, redshift, lastred, d, bound, label):
    """uvf_export against the restatement: NaN exactly where no row was treated, the value within the bound, the class equal"""
    n = len(z)
    listed = np.zeros(n, bool)
    listed[rows] = True
    treated = listed & (res["cls"] >= 0)
    assert np.isnan(z[~treated]).all() and not np.isnan(z[treated]).any(), label
    err = np.abs(z[treated] - res["zreion"][treated])
    print("uvf_export %s: %d rows, max |dzreion| = %.2g of the bound" % (label, treated.sum(), err.max() / bound if treated.any() else 0))
    assert (err <= bound).all(), label
    cls = np.array([U.row_class(z[p], redshift, float(lastred[d["tb_hydro"][p]])) for p in np.nonzero(treated)[0]])
    assert np.array_equal(cls, res["cls"][treated]), label


# ---- 1. the per-point read --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Nside", (2, 5, 16))
def test_per_point_read(pkg, Nside):
    """mpg_dev_uvf_zreion on 4099 points: grid points, x == BoxSize, x == 0, negative coordinates, coordinates beyond two periods, with two
    offsets; then one NaN and one 1e300 coordinate"""
    import torch
    box = 0.25 * (Nside - 1)                                          # cells of exactly 0.25
    table = U.synthetic_zreion_table(Nside, 7.0, 10 + Nside)
    uvf = U.UVF(table, box)
    assert uvf.interp.Step == [0.25] * 3
    bound = 16 * EPS * np.abs(table).max()
    rs = np.random.RandomState(Nside)
    period = 0.25 * Nside
    gi = rs.randint(-2 * Nside, 3 * Nside, (600, 3))                  # grid points, up to two periods away on either side
    gi[:8] = [[a, b, c] for a in (0, Nside - 1) for b in (0, Nside - 1) for c in (0, Nside - 1)]
    special = np.array([[box, 0.1, 0.2], [0.1, box, box], [0.0, 0.0, 0.0], [0.0, 0.3, box], [-0.01, -0.3, 0.4], [-1e-300, 0.5, -box], [period, 2 * period, -period]])
    near = rs.uniform(-0.25 * box, 1.25 * box, (2000, 3))
    far = rs.uniform(-3.5 * period, 4.5 * period, (4099 - 600 - len(special) - 2000, 3))
    assert (np.abs(far) > 2 * period).any(axis=1).sum() > 300
    eng = pkg.Engine(0)
    eng.set_uvf_table(table, box)
    first = None
    for offset in ((0.5, -0.25, 0.125), U.OFFSET):                    # the first is exact in binary: grid points stay grid points
        pts = np.concatenate([0.25 * gi + np.array(offset), special, near, far])
        assert pts.shape == (4099, 3) and 4099 % 64 != 0
        want = np.array([uvf.zreion(x, offset) for x in pts])
        eng.set_uvf_offset(offset)
        pos, out = torch.from_numpy(pts).cuda(), torch.zeros(4099, dtype=torch.float64, device="cuda")
        eng.dev_uvf_zreion(pos, out)
        eng.synchronize()
        got = out.cpu().numpy()
        err = np.abs(got - want)
        print("zreion Nside %d offset %s: max error %.2g of the bound" % (Nside, offset, err.max() / bound))
        assert (err <= bound).all()
        if first is None:
            first = (pts, got)
            entries = table[gi[:, 0] % Nside, gi[:, 1] % Nside, gi[:, 2] % Nside]
            assert np.array_equal(got[:600], entries) and np.array_equal(want[:600], entries)
    # a coordinate that is not finite, and one beyond 2^31 cells: NaN for those points alone, a non-zero return, the others unchanged
    eng.set_uvf_offset((0.5, -0.25, 0.125))
    pts, good = first[0].copy(), first[1]
    pts[7, 0], pts[1000, 1] = np.nan, 1e300
    pos, out = torch.from_numpy(pts).cuda(), torch.zeros(4099, dtype=torch.float64, device="cuda")
    with pytest.raises(pkg.EngineError, match="2 point"):
        eng.dev_uvf_zreion(pos, out)
    eng.synchronize()
    got = out.cpu().numpy()
    bad = np.zeros(4099, bool)
    bad[[7, 1000]] = True
    assert np.isnan(got[bad]).all() and np.array_equal(got[~bad], good[~bad])
    eng.close()


# ---- 2. the setters ---------------------------------------------------------------------------------------------------------------------------
def test_setters(pkg):
    """what mpg_set_uvf_table refuses, by name; and removing the table gives back the call without one, bit for bit"""
    import torch
    C, times, step, d, pos, uvf, res = cooling_reference("sherwood_reion")
    table = table_of(uvf)
    eng = pkg.Engine(0)
    with pytest.raises(pkg.EngineError, match="Nside"):
        eng.set_uvf_table(np.full((1, 1, 1), 7.0), 1.0)
    bad = table.copy()
    bad[0, 0, 0] = 200.0
    with pytest.raises(pkg.EngineError, match=r"table\[0\]"):
        eng.set_uvf_table(bad, 1.0)
    bad = table.copy()
    bad[2, 3, 1] = np.nan
    with pytest.raises(pkg.EngineError, match="table"):
        eng.set_uvf_table(bad, 1.0)
    with pytest.raises(pkg.EngineError, match="BoxSize"):
        eng.set_uvf_table(table, 0.0)
    with pytest.raises(pkg.EngineError, match="no table"):
        eng.dev_uvf_zreion(torch.zeros(4, 3, dtype=torch.float64, device="cuda"), torch.zeros(4, dtype=torch.float64, device="cuda"))
    T = TC.sph_times(pkg, times)
    TC.configure(eng, C)
    plain = run_cooling(torch, eng, d, pos, T, step)
    assert plain[3] is None
    eng.set_uvf_table(table, U.BOXSIZE)
    eng.set_uvf_offset(U.OFFSET)
    with_table = run_cooling(torch, eng, d, pos, T, step)
    assert with_table[3] is None and (with_table[0]["entropy"] != plain[0]["entropy"]).sum() > 50
    eng.set_uvf_table()
    again = run_cooling(torch, eng, d, pos, T, step)
    assert again[3] is None and again[2] == plain[2] and np.array_equal(again[1], plain[1])
    for k in plain[0]:
        assert np.array_equal(again[0][k], plain[0][k]), k
    eng.close()


# ---- 3. the cooling ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(U.COOLING_SETS))
def test_cooling_with_the_table(pkg, name):
    """both kernel forms and both table placements against the restatement; the table is read; a table of 100s is the call without one
    except in the HIReionTemp window; an active sub-list and an empty list"""
    import torch
    C, times, step, d, pos, uvf, res = cooling_reference(name)
    n = len(d["type"])
    redshift = 1. / times["atime"] - 1
    table = table_of(uvf)
    bound = 16 * EPS * np.abs(table).max()
    eng = pkg.Engine(0)
    T = TC.sph_times(pkg, times)
    eng.set_uvf_table(table, U.BOXSIZE)
    eng.set_uvf_offset(U.OFFSET)
    outs = []
    for form, lds in ((0, 0), (1, 0), (0, 1), (1, 1)):
        TC.configure(eng, C, form, lds)
        out, evals, stats, err = run_cooling(torch, eng, d, pos, T, step)
        assert err is None, err
        label = "%s with a table, form %d lds %d" % (name, form, lds)
        z = eng.uvf_export(n)
        check_export(z, res, np.arange(n), redshift, step["lastred"], d, bound, label)
        window = int(sum(res["info"][p]["reion"] for p in res["info"]))
        assert stats["reion"] == window and (window > 50 if C.p["HIReionTemp"] > 0 else window == 0)
        TC.compare(d, res, out, evals, stats, n, np.arange(n), label)
        outs.append((out, evals, z))
    for out, evals, z in outs[1:]:                              # the forms and placements do the same arithmetic
        assert np.array_equal(evals, outs[0][1]) and np.array_equal(z, outs[0][2], equal_nan=True)
        for k in ("entropy", "ne", "sfr"):
            assert np.array_equal(out[k], outs[0][0][k]), k
    # an active sub-list and an empty list
    for form in (0, 1):
        TC.configure(eng, C, form)
        for what, act in (("strided", np.arange(3, n, 7, dtype=np.int32)), ("empty", np.zeros(0, np.int32))):
            out, evals, stats, err = run_cooling(torch, eng, d, pos, T, step, active=act)
            assert err is None, err
            label = "%s with a table, %s list form %d" % (name, what, form)
            TC.compare(d, res, out, evals, stats, n, act, label)
            check_export(eng.uvf_export(n), res, act, redshift, step["lastred"], d, bound, label)
            if what == "empty":
                assert stats["treated"] == 0 and stats["evaluations"] == 0
    # the global background alone gives something else: the table is read
    TC.configure(eng, C)
    eng.set_uvf_table()
    plain, pevals, pstats, err = run_cooling(torch, eng, d, pos, T, step)
    assert err is None, err
    treated = res["cls"] >= 0
    differ = (plain["entropy"] != outs[0][0]["entropy"]) | (plain["ne"] != outs[0][0]["ne"])
    print("%s: %d of %d treated rows differ from the call without a table" % (name, differ[treated].sum(), treated.sum()))
    assert differ[treated].sum() >= 0.10 * treated.sum() and not differ[~treated].any()
    # reionised long before: the global background for every row, and a zreion of 100 in the window test
    eng.set_uvf_table(np.full((3, 3, 3), 100.0), U.BOXSIZE)
    early, eevals, estats, err = run_cooling(torch, eng, d, pos, T, step)
    assert err is None, err
    assert (np.abs(eng.uvf_export(n)[treated] - 100.0) <= 16 * EPS * 100.0).all()
    zg = step["uvbg"]["zreion"]
    window = treated & (C.p["HIReionTemp"] > 0) & (zg >= redshift) & (zg < step["lastred"][d["tb_hydro"]])
    assert estats["reion"] == 0 and pstats["reion"] == int(window.sum()) and (window.sum() > 50 if C.p["HIReionTemp"] > 0 else True)
    for k in ("entropy", "ne", "sfr"):
        assert np.array_equal(early[k][~window], plain[k][~window]), k
    assert np.array_equal(eevals[~window], pevals[~window])
    if window.any():                                            # ... whose rows are cooled instead of set to HIReionTemp
        assert (eevals[window] > 0).all() and (pevals[window] == 0).all()
    eng.close()


def test_a_position_that_cannot_be_read_is_an_error_row(pkg):
    """one gas row with a NaN coordinate: the call returns non-zero, the row keeps Entropy / Ne / Sfr and counts in the errors, its zreion is
    NaN, every other row is as without it"""
    import torch
    C, times, step, d, pos, uvf, res = cooling_reference("sherwood_reion")
    n = 130
    dd = {k: v[:n] for k, v in d.items()}
    victim = int(np.nonzero(res["cls"][:n] >= 0)[0][40])
    broken = pos[:n].copy()
    broken[victim, 1] = np.nan
    eng = pkg.Engine(0)
    T = TC.sph_times(pkg, times)
    eng.set_uvf_table(table_of(uvf), U.BOXSIZE)
    eng.set_uvf_offset(U.OFFSET)
    sub = {k: (v[:n] if isinstance(v, np.ndarray) else v) for k, v in res.items()}
    for form in (0, 1):
        TC.configure(eng, C, form)
        out, evals, stats, err = run_cooling(torch, eng, dd, broken, T, step)
        assert isinstance(err, pkg.EngineError) and "position" in str(err)
        assert stats["errors"] == 1 and evals[victim] == 0 and np.isnan(eng.uvf_export(n)[victim])
        TC.compare(dd, sub, out, evals, stats, n, np.arange(n), "a NaN position, form %d" % form, bad=[victim])
    eng.close()


# ---- 4. the host form -------------------------------------------------------------------------------------------------------------------------
def test_host_form_equals_dev_form(pkg):
    """mpg_cooling on the 160-byte records with an active sub-list: bit for bit the dev form, the zreion column included"""
    import torch
    C, times, step, d, pos, uvf, res = cooling_reference("sherwood_z3")
    n = len(d["type"])
    act = np.arange(1, n, 2, dtype=np.int32)
    eng = pkg.Engine(0)
    TC.configure(eng, C)
    eng.set_uvf_table(table_of(uvf), U.BOXSIZE)
    eng.set_uvf_offset(U.OFFSET)
    T = TC.sph_times(pkg, times)
    dev, evals, stats, err = run_cooling(torch, eng, d, pos, T, step, active=act)
    assert err is None, err
    z = eng.uvf_export(n)
    TC.compare(d, res, dev, evals, stats, n, act, "dev / sublist with a table")
    P = pkg.make_particles(pos, d["mass"], type=np.where(d["type"] == 7, 0, d["type"]))
    P["Flags"][d["type"] == 7] = 1
    a = {k: d[k].copy() for k in COOL_COLUMNS}
    eng.cooling(P, U.BOXSIZE, a, T, step, ActiveParticle=act)
    assert np.array_equal(eng.cooling_export(n), evals) and np.array_equal(eng.uvf_export(n), z, equal_nan=True)
    assert np.isfinite(z).sum() == stats["treated"] > 300
    for k in ("entropy", "ne", "sfr"):
        assert np.array_equal(a[k], dev[k]), k
    eng.close()


# ---- 5. star formation ------------------------------------------------------------------------------------------------------------------------
def configure_sfr(eng, S, uvf=None):
    eng.set_cooling_params(S.C.p)
    eng.set_metal_cooling_table(*R.synthetic_metal_table())
    eng.set_random_table(SF.random_table())
    eng.set_wind_params(SF.WIND)
    if uvf is None:
        eng.set_uvf_table()
    else:
        eng.set_uvf_table(table_of(uvf), U.BOXSIZE)
        eng.set_uvf_offset(U.OFFSET)
    eng.set_sfr_params(dict(SF.engine_params(S.p), UVFluctuationOn=int(uvf is not None)))


def run_sfr(torch, eng, d, pos, T, step):
    n = len(d["type"])
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    keep = dict(pos=up(pos), mass=up(d["mass"]), type=up(d["type"]))
    eng.dev_bind_particles(keep["pos"], keep["mass"], U.BOXSIZE, type=keep["type"])
    a = {k: up(d[k].view(np.int64) if k == "id" else d[k]) for k in TS.READ + TS.IO}
    a["stellarmass"] = torch.zeros(n, dtype=torch.float64, device="cuda")
    eng.dev_cooling_and_starformation(a, T, step)
    eng.synchronize()
    out = {k: a[k].cpu().numpy() for k in TS.IO + ("stellarmass",)}
    out["cls"], out["sfevals"] = eng.sfr_export_rows(n)
    out["evals"] = eng.cooling_export(n)
    out.update(eng.sfr_export())
    out["result"], out["stats"], out["cooling_stats"] = eng.sfr_result(), eng.sfr_stats(), eng.cooling_stats()
    return out


def test_star_formation_with_the_table(pkg):
    """the `heating` set through mpg_dev_cooling_and_starformation: every column, both lists, the sums and the counts against the
    restatement at the tolerances of tests/test_gpu_sfr.py; without the table the dark star-forming rows come out differently"""
    import torch
    S, times, step, d, pos, uvf, res = sfr_reference()
    n = len(d["type"])
    T = TS.sph_times(pkg, times)
    eng = pkg.Engine(0)
    configure_sfr(eng, S, uvf)
    out = run_sfr(torch, eng, d, pos, T, step)
    TS.compare(d, res, out, n, "heating with a table")
    assert out["result"]["sum_sf_part"] == res["sum_sf_part"] and out["result"]["newstars"] == len(res["parent"])
    z = eng.uvf_export(n)
    treated = res["cls"] != 0
    assert np.isnan(z[~treated]).all() and (np.abs(z[treated] - res["zreion"][treated]) <= 16 * EPS * np.abs(table_of(uvf)).max()).all()
    assert np.array_equal(z[treated] < 1. / times["atime"] - 1, res["dark"][treated])
    configure_sfr(eng, S, None)
    plain = run_sfr(torch, eng, d, pos, T, step)
    sf_dark = (res["cls"] == SF.ROW_STARFORMING) & res["dark"]
    sf_lit = (res["cls"] == SF.ROW_STARFORMING) & ~res["dark"]
    differ = (plain["entropy"] != out["entropy"]) | (plain["sfr"] != out["sfr"])
    print("star formation: %d of %d dark star-forming rows differ from the call without a table" % (differ[sf_dark].sum(), sf_dark.sum()))
    assert differ[sf_dark].sum() >= 50 and not differ[sf_lit].any()
    eng.close()


# ---- 6. the flag ------------------------------------------------------------------------------------------------------------------------------
def test_the_flag_and_the_table_go_together(pkg):
    import torch
    S, times, step, d, pos, uvf, res = sfr_reference()
    n = 130
    dd = {k: v[:n] for k, v in d.items()}
    T = TS.sph_times(pkg, times)
    eng = pkg.Engine(0)
    with pytest.raises(pkg.EngineError, match="UVFluctuationOn"):
        eng.set_sfr_params(dict(SF.engine_params(S.p), UVFluctuationOn=1))
    configure_sfr(eng, S, uvf)                                  # accepted once the table is there
    run_sfr(torch, eng, dd, pos[:n], T, step)
    eng.set_uvf_table()                                         # the flag stays set, the table is gone
    with pytest.raises(pkg.EngineError, match="UVFluctuationOn"):
        run_sfr(torch, eng, dd, pos[:n], T, step)
    configure_sfr(eng, S, None)
    run_sfr(torch, eng, dd, pos[:n], T, step)
    eng.set_uvf_table(table_of(uvf), U.BOXSIZE)                 # a table, and the flag 0
    with pytest.raises(pkg.EngineError, match="UVFluctuationOn"):
        run_sfr(torch, eng, dd, pos[:n], T, step)
    for over, text in ((dict(ExcursionSetReion=1), "EXCUR_REION"), (dict(BHFeedbackUseTcool=2), "BHFeedbackUseTcool == 2"), (dict(NTask=2), "NTask")):
        with pytest.raises(pkg.EngineError, match=text):
            eng.set_sfr_params(dict(SF.engine_params(S.p), UVFluctuationOn=1, **over))
    eng.close()


# ---- 7. the resident form ---------------------------------------------------------------------------------------------------------------------
def test_resident_form_in_a_gas_stretch(pkg):
    """density -> hydro_force -> cooling inside a resident stretch with a table (the pattern, box and gas count of
    tests/test_gpu_cooling.py::test_resident_form_in_a_gas_stretch): the resident entropy column, ne and the zreion column equal, bit for bit,
    what the dev form gives on the same positions and columns"""
    import torch
    pos, mass, typ, box = pkg.ics.hydro_pair(12)
    n = len(pos)
    C0, times, step, _ = R.config("sherwood_z3", G["treecool"])
    a3inv = 1. / times["atime"] ** 3
    meanrho = float(mass[typ == 0].sum()) / box ** 3
    C = R.Cooling(dict(C0.p, density_in_phys_cgs=1e-3 * R.PROTONMASS / (meanrho * a3inv)), R.TreeCool(G["treecool"]), C0.metal)
    table = U.synthetic_zreion_table(5, 3.0, 4)
    offset = tuple(box * x for x in U.OFFSET)
    rs = np.random.RandomState(21)
    u_target = np.exp(rs.uniform(np.log(1.0), np.log(3e6), n))
    T = TC.sph_times(pkg, times)
    for b in range(47):
        T.hydrokicks[b] = T.gravkicks[b] = T.drifts[b] = T.dloga_kick[b] = 0.0
    T.FgravkickB = 0.0
    gas = typ == 0
    ne0 = rs.uniform(0, 1.2, n)
    Z = np.where(rs.uniform(size=n) < 0.5, rs.uniform(0, 1.5, n), 0.0)
    he = (rs.uniform(size=n) < 0.5).astype(np.uint8)
    tb = rs.randint(1, 47, n).astype(np.uint8)
    act = np.arange(0, n, 3, dtype=np.int32)
    eng = pkg.Engine(0)
    TC.configure(eng, C)
    eng.set_uvf_table(table, box)
    eng.set_uvf_offset(offset)
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
    d_ent, d_rho = TC.device_view(torch, ptr["entropy"], n), TC.device_view(torch, ptr["density"], n)
    d_ent.copy_(torch.where(d_rho > 0, torch.from_numpy(u_target).cuda() * R.GAMMA_MINUS1 / (d_rho.clamp(min=1e-300) * a3inv) ** R.GAMMA_MINUS1, d_ent))
    ent0, rho0 = d_ent.clone(), d_rho.clone()
    ne = ne0.copy()
    eng.resident_sph_cooling(P, T, step, ne, metallicity=Z, heiii_ionized=he, ActiveParticle=act)
    evals, stats, zres = eng.cooling_export(n), eng.cooling_stats(), eng.uvf_export(n)
    ent1 = d_ent.clone()
    # the dev form on copies of what the stretch held (the bound table is the resident one)
    up = lambda x: torch.from_numpy(x).cuda()
    c = dict(density=rho0, entropy=ent0.clone(), ne=up(ne0), sfr=torch.ones(n, dtype=torch.float64, device="cuda"), metallicity=up(Z),
             heiii_ionized=up(he), tb_hydro=up(tb))
    eng.dev_cooling(c, T, step, active=up(act))
    eng.synchronize()
    assert stats["treated"] == int(gas[act].sum()) > 100 and stats["errors"] == 0 and stats["evaluations"] > 20 * stats["treated"]
    assert np.array_equal(eng.cooling_export(n), evals) and np.array_equal(eng.uvf_export(n), zres, equal_nan=True)
    assert torch.equal(c["entropy"], ent1) and np.array_equal(c["ne"].cpu().numpy(), ne)
    # ... and the zreion column is the restatement's at the resident positions, with dark and lit rows among them
    uvf = U.UVF(table, box)
    listed = np.zeros(n, bool)
    listed[act] = True
    treated = listed & gas
    want = np.array([uvf.zreion(pos[p], offset) for p in np.nonzero(treated)[0]])
    assert np.isnan(zres[~treated]).all() and (np.abs(zres[treated] - want) <= 16 * EPS * np.abs(table).max()).all()
    redshift = 1. / times["atime"] - 1
    assert (want < redshift).sum() > 100 and (want >= redshift).sum() > 100
    eng.resident_sph_end(a)
    eng.resident_end(P)
    eng.close()
