"""GPU tests of the star formation (csrc/sfr.hip: the loop of cooling_and_starformation without the spawning) against the plain-Python
restatement tests/sfr_restated.py, which tests/test_sfr_restated.py holds to identities, holds the host build of csrc/sfr.h to bit for bit,
and whose decisions it shows to be stable on the very input sets used here.

What is compared, per call
  EQUAL     the class of every row, the new-star list (parent, mass_of_star, convert / spawn) and the MaybeWind list in the order of the
            active list, the counts and sum_sf_part, DelayTime (winds_evolve) and BHHeated of every row, Sfr == 0 on the cooled rows, and every
            column of every row that is not treated (outside the list, non-gas, garbage, massless), bit for bit.
  cooled    the tolerances of tests/test_gpu_cooling.py: 1e-12 relative entropy, 1e-10 Ne, equal evaluation counts; within its cap of 0.1 %
            a row may miss and must then agree to 3e-6.  A TimeBinHydro beyond 46 is read as 46 (a case of its own).
  star-forming rows
            every output column to 100 x the sensitivity tests/test_sfr_restated.py recorded for it, floor 1e-13 (sfr_restated.TOLERANCE;
            the error is sfr_restated.column_error's): Entropy 1.6e-12, Ne 1e-13, Sfr 8.5e-11 (the cancellation of 1 - exp(-p)), Metallicity
            1e-13, StellarMass 1e-13.  A row may miss only if its network evaluation count differs from the restatement's, at most 0.1 % of
            the star-forming rows may, and such a row still agrees to 1e-6 / (1 - cloudfrac) with equal decisions.
  sums      sum_sm, localsfr, sum_dtime to 1e-12 relative, and bit-equal between two calls.
The worst ratios are printed (pytest -s); DESIGN 3.15 records them."""
import numpy as np
import pytest

import cooling_restated as R
import sfr_restated as SF
import test_cooling_restated as K
import test_sfr_restated as KS
from test_gpu_cooling import sph_times

pytestmark = pytest.mark.gpu

G = K.G
IO = ("entropy", "ne", "sfr", "metallicity", "delaytime", "bhheated", "vel")
READ = ("id", "generation", "density", "hsml", "divvel", "curlvel", "gradrho_mag", "tb_hydro", "heiii_ionized", "vdisp")
_tables, _cache, _ref = {}, {}, {}


def table(name, mode):
    """the input table of a case, computed once (the cases of equal size share it: the generator does not depend on the setting)"""
    S, times, step, make = SF.config(name, G["treecool"], mode)
    n = KS.size_of(name, mode)
    if n not in _tables:
        _tables[n] = make(n)
    return S, times, step, _tables[n]


def restate(name, mode, S, times, step, d, n=None, active=None):
    """the restatement on the first n rows; cooling_direct of a row is computed once per (table, UV background) whatever the setting"""
    n = len(d["type"]) if n is None else n
    dd = {k: v[:n] for k, v in d.items()}
    cache = _cache.setdefault((len(d["type"]), name == "heating"), {})
    return dd, SF.cooling_and_starformation(S, dd, times, step, SF.random_table(), active=active, wind=SF.WIND, cool_cache=cache)


def reference(name, mode):
    if (name, mode) not in _ref:
        S, times, step, d = table(name, mode)
        _ref[(name, mode)] = (S, times, step, d, restate(name, mode, S, times, step, d)[1])
        assert not _ref[(name, mode)][4]["failed"]
    return _ref[(name, mode)]


def configure(eng, S, wind_on=0, model=SF.WIND["WindModel"], **over):
    eng.set_cooling_params(dict(S.C.p, **over))
    eng.set_metal_cooling_table(*R.synthetic_metal_table())
    eng.set_random_table(SF.random_table())
    eng.set_wind_params(dict(SF.WIND, WindModel=model))
    eng.set_sfr_params(dict(SF.engine_params(S.p), WindOn=wind_on))


def bind(torch, eng, d, n):
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a[:n])).cuda()
    pos = torch.from_numpy(np.random.RandomState(1).uniform(0, 1, (n, 3))).cuda()
    keep = dict(pos=pos, mass=up(d["mass"]), type=up(d["type"]))
    eng.dev_bind_particles(keep["pos"], keep["mass"], 1.0, type=keep["type"])
    a = {k: up(d[k].view(np.int64) if k == "id" else d[k]) for k in READ + IO}
    a["stellarmass"] = torch.zeros(n, dtype=torch.float64, device="cuda")
    return a, keep


def run_dev(torch, eng, d, T, step, n, active=None):
    a, keep = bind(torch, eng, d, n)
    act, nact = None, None
    if active is not None:
        act = torch.from_numpy(np.ascontiguousarray(active, np.int32)).cuda()
        if len(active) == 0:
            act, nact = torch.zeros(1, dtype=torch.int32, device="cuda"), 0            # an empty list with a pointer that is not NULL
    err = None
    try:
        eng.dev_cooling_and_starformation(a, T, step, active=act, nactive=nact)
    except Exception as e:      # noqa: BLE001 - the caller decides whether an error return was expected
        err = e
    eng.synchronize()
    out = {k: a[k].cpu().numpy() for k in IO + ("stellarmass",)}
    out["cls"], out["sfevals"] = eng.sfr_export_rows(n)
    out["evals"] = eng.cooling_export(n)
    out.update(eng.sfr_export())
    out["result"], out["stats"], out["cooling_stats"] = eng.sfr_result(), eng.sfr_stats(), eng.cooling_stats()
    return out, err


def compare(d, res, out, n, label, bad=()):
    """`d`: the n input rows; `res`: the restatement; `out`: run_dev's; `bad`: rows expected to hit a limit"""
    bad = list(bad)
    assert np.array_equal(out["cls"], res["cls"]), label
    cooled, sf = res["cls"] == SF.ROW_COOLED, res["cls"] == SF.ROW_STARFORMING
    ok = np.ones(n, bool)
    ok[bad] = False
    # the lists, in order
    for k in ("parent", "spawn", "mass_of_star", "maybewind"):
        assert np.array_equal(out[k], res[k]), (label, k)
    r = out["result"]
    assert (r["treated"], r["cooled"], r["sum_sf_part"], r["newstars"], r["maybewind"]) == \
        (int((res["cls"] != 0).sum()), int(cooled.sum()), res["sum_sf_part"], len(res["parent"]), len(res["maybewind"])), (label, r)
    assert r["spawned"] == int(res["spawn"].sum()) and r["converted"] == len(res["parent"]) - r["spawned"] and r["errors"] == len(bad)
    st = out["stats"]
    assert (st["treated"], st["cooled"], st["starforming"], st["newstars"], st["maybewind"]) == (r["treated"], r["cooled"], r["sum_sf_part"], r["newstars"], r["maybewind"])
    for k in ("sum_sm", "localsfr", "sum_dtime"):
        assert abs(r[k] - res[k]) <= 1e-12 * abs(res[k]), (label, k, r[k], res[k])
    # what no arithmetic touches: winds_evolve's DelayTime and BHHeated everywhere, every column of the rows that are not treated, and what
    # a class does not write
    assert np.array_equal(out["delaytime"], res["delaytime"]) and np.array_equal(out["bhheated"], res["bhheated"]), label
    assert np.array_equal(out["vel"], d["vel"]), label
    keep = (res["cls"] == 0) | ~ok
    for k in ("entropy", "ne", "sfr", "metallicity"):
        assert np.array_equal(out[k][keep], d[k][keep]), (label, k)
    assert np.array_equal(out["metallicity"][cooled], d["metallicity"][cooled]) and (out["sfr"][cooled & ok] == 0).all(), label
    assert np.array_equal(out["stellarmass"] != 0, res["stellarmass"] != 0), label
    assert np.array_equal(out["sfevals"][~sf], np.full(int((~sf).sum()), -1)) and np.array_equal(out["evals"][~cooled], np.full(int((~cooled).sum()), -1)), label
    # the cooled rows at the tolerances of tests/test_gpu_cooling.py
    c = cooled & ok
    e_ent = np.abs(out["entropy"][c] / res["entropy"][c] - 1)
    e_ne = np.abs(out["ne"][c] - res["ne"][c])
    miss = (e_ent > 1e-12) | (e_ne > 1e-10) | (out["evals"][c] != res["evals"][c])
    assert miss.sum() <= 1e-3 * c.sum(), (label, int(miss.sum()), int(c.sum()))
    assert (e_ent[miss] <= 3e-6).all() and (np.abs(out["ne"][c][miss] / np.maximum(res["ne"][c][miss], 1e-300) - 1) <= 3e-6).all(), label
    # the star-forming rows
    s = np.nonzero(sf & ok)[0]
    line = "sfr %s: %d cooled (%d miss), %d star-forming" % (label, c.sum(), miss.sum(), len(s))
    if len(s) and res["info"]:
        same = out["sfevals"][s] == res["sfevals"][s]
        missed = ~same
        cf = np.array([res["info"][i]["cloudfrac"] for i in s])
        loose = 1e-6 / np.maximum(1 - cf, 1e-300)
        for k in ("entropy", "ne", "sfr", "metallicity", "stellarmass"):
            err = SF.column_error(k, out[k][s], res[k][s])
            line += "; %s %.2g" % (k, (err[same].max() if same.any() else 0) / SF.TOLERANCE[k])
            assert (err[same] <= SF.TOLERANCE[k]).all(), (label, k, float(err[same].max()), SF.TOLERANCE[k])
            assert (err[missed] <= loose[missed]).all(), (label, k)
        assert missed.sum() <= 1e-3 * len(s), (label, int(missed.sum()), len(s))
        line += " of the tolerance; %d with another evaluation count; evaluations %d .. %d" % (missed.sum(), res["sfevals"][s].min(), res["sfevals"][s].max())
        if not missed.any():
            assert st["evaluations"] == int(res["sfevals"][s].sum()) + sum(int(out["sfevals"][i]) for i in bad if sf[i])
    else:                                                     # Quick Lyman alpha: a star-forming row keeps every column
        for k in ("entropy", "ne", "sfr", "metallicity"):
            assert np.array_equal(out[k][sf], d[k][sf]), (label, k)
    print(line)


def subgrid_on_equals_chain(torch, eng, S, d, T, step, n, atime):
    """with WindOn and WIND_SUBGRID the call equals the call without WindOn followed by mpg_dev_winds_subgrid on the exported MaybeWind list,
    bit for bit in every column; returns the kicks applied"""
    configure(eng, S, wind_on=1)
    a1, keep1 = bind(torch, eng, d, n)
    eng.dev_cooling_and_starformation(a1, T, step)
    applied = eng.winds_stats()["applied"]
    lists1 = eng.sfr_export()
    configure(eng, S, wind_on=0)
    a2, keep2 = bind(torch, eng, d, n)
    eng.dev_cooling_and_starformation(a2, T, step)
    lists2 = eng.sfr_export()
    for k in lists1:
        assert np.array_equal(lists1[k], lists2[k]), k
    if len(lists2["maybewind"]):
        eng.dev_winds_subgrid(a2, torch.from_numpy(lists2["maybewind"]).cuda(), a2["stellarmass"], atime)
        assert eng.winds_stats()["applied"] == applied
    eng.synchronize()
    for k in IO + ("stellarmass",):
        assert torch.equal(a1[k], a2[k]), k
    return applied


# ---- mpg_dev_cooling_and_starformation against the restatement ------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(SF.SETTINGS))
def test_dev_form_against_restatement(pkg, name):
    """every setting (the density criterion, + H2, + self-gravity with and without its two modifiers, BoostSFDenseGas, Quick Lyman alpha, the
    synthetic heating case) at z = 3, Verner96 / Sherwood with metals, with BHFeedbackUseTcool 0, 1 and 3; NULL list.  WIND_SUBGRID off:
    against the restatement; on: against the call without it followed by the subgrid kernel on the exported list"""
    import torch
    eng = pkg.Engine(0)
    for mode in KS.MODES:
        S, times, step, d, res = reference(name, mode)
        n = len(d["type"])
        configure(eng, S)
        out, err = run_dev(torch, eng, d, sph_times(pkg, times), step, n)
        assert err is None, err
        compare(d, res, out, n, "%s / %d" % (name, mode))
        applied = subgrid_on_equals_chain(torch, eng, S, d, sph_times(pkg, times), step, n, times["atime"])
        assert applied > 0 or len(res["maybewind"]) == 0, (name, mode)
    eng.close()


def test_time_bins_beyond_46_are_read_as_46(pkg):
    """a TimeBinHydro of 47 .. 249 (every ninth row, cooled, star-forming and in the wind among them) is handled as the cooling kernel handles
    it: read as bin 46, by winds_evolve, by the cooled rows and by the star-forming rows alike"""
    import torch
    S, times, step, d0, _ = reference("density", 3)
    n = len(d0["type"])
    d = dict(d0, tb_hydro=d0["tb_hydro"].copy())
    high = np.arange(n) % 9 == 4
    d["tb_hydro"][high] = (47 + np.arange(n) % 209)[high].astype(np.uint8)
    assert d["tb_hydro"][high].min() >= 47 and d["tb_hydro"].max() > 200
    res = SF.cooling_and_starformation(S, d, times, step, SF.random_table(), wind=SF.WIND)          # (no cache: the rows differ from the table's)
    assert not res["failed"]
    assert (res["cls"][high] == SF.ROW_COOLED).sum() > 10 and (res["cls"][high] == SF.ROW_STARFORMING).sum() > 10
    assert (high & (d["delaytime"] > 0) & (res["delaytime"] != d["delaytime"])).sum() > 3
    eng = pkg.Engine(0)
    configure(eng, S)
    out, err = run_dev(torch, eng, d, sph_times(pkg, times), step, n)
    assert err is None, err
    compare(d, res, out, n, "time bins beyond 46")
    eng.close()


def test_shapes_and_active_lists(pkg):
    """n = 1, 63, 64, 65 and 4099; a list that is NULL, empty, a strided subset and a permutation (with non-gas, garbage and massless rows and
    entries outside the table in it): both lists come out in the order of the list"""
    import torch
    S, times, step, d, res = reference("density", 1)
    N = len(d["type"])
    assert N == 4099
    eng = pkg.Engine(0)
    configure(eng, S)
    T = sph_times(pkg, times)
    for n in (1, 63, 64, 65):
        dd, r = restate("density", 1, S, times, step, d, n)
        out, err = run_dev(torch, eng, d, T, step, n)
        assert err is None, err
        compare(dd, r, out, n, "n = %d" % n)
    rs = np.random.RandomState(9)
    perm = rs.permutation(N).astype(np.int32)
    lists = dict(empty=np.zeros(0, np.int32), strided=np.arange(3, N, 7, dtype=np.int32),
                 permutation=np.concatenate([perm[:2000], np.array([-1, N, N + 5, 2 ** 31 - 1], np.int32), perm[2000:]]))
    for what, act in lists.items():
        dd, r = restate("density", 1, S, times, step, d, N, active=act)
        out, err = run_dev(torch, eng, d, T, step, N, active=act)
        assert err is None, err
        compare(dd, r, out, N, "%s list" % what)
        if what == "empty":
            assert out["result"]["treated"] == 0 and out["stats"]["listed"] == 0 and len(out["parent"]) == 0
        if what == "permutation":
            assert len(out["parent"]) > 100 and (np.diff(out["parent"]) < 0).any() and (np.diff(out["maybewind"]) < 0).any()
    eng.close()


def test_two_calls_give_the_same_bits(pkg):
    """the four sums, the lists and every column of two calls on the same input are bit-equal"""
    import torch
    S, times, step, d, res = reference("density", 1)
    n = len(d["type"])
    eng = pkg.Engine(0)
    configure(eng, S)
    T = sph_times(pkg, times)
    a, _ = run_dev(torch, eng, d, T, step, n)
    b, _ = run_dev(torch, eng, d, T, step, n)
    assert a["result"] == b["result"] and a["result"]["sum_sm"] > 0 and a["result"]["localsfr"] > 0 and a["result"]["sum_dtime"] > 0
    for k in IO + ("stellarmass", "cls", "sfevals", "evals", "parent", "spawn", "mass_of_star", "maybewind"):
        assert np.array_equal(a[k], b[k]), k
    eng.close()


# ---- the host form and the resident form ----------------------------------------------------------------------------------------------------
def host_columns(d, n):
    a = {k: np.ascontiguousarray(d[k][:n]).copy() for k in READ + IO}
    a["stellarmass"] = np.zeros(n)
    return a


def device_view(torch, ptr, n, typestr="<f8"):
    class H:
        pass
    h = H()
    h.__cuda_array_interface__ = {"shape": (int(n),), "typestr": typestr, "data": (int(ptr), False), "version": 2}
    return torch.as_tensor(h, device="cuda")


def test_host_and_resident_forms_equal_dev_form(pkg):
    """mpg_cooling_and_starformation on the 160-byte records (IsGarbage in the flags byte) and mpg_resident_sph_cooling_and_starformation
    inside a resident gas stretch (Density, Entropy, TimeBinHydro, Hsml, DivVel and CurlVel resident - the H2 criterion reads Hsml from the
    stretch -, the rest travels), with an active sublist: every column and
    both lists bit for bit the dev form's"""
    import torch
    name, mode = "h2", 1
    S, times, step, d, res = reference(name, mode)
    n = len(d["type"])
    act = np.arange(1, n, 2, dtype=np.int32)
    eng = pkg.Engine(0)
    configure(eng, S)
    T = sph_times(pkg, times)
    dev, err = run_dev(torch, eng, d, T, step, n, active=act)
    assert err is None, err
    compare(d, restate(name, mode, S, times, step, d, n, active=act)[1], dev, n, "dev / sublist")
    pos = np.random.RandomState(1).uniform(0, 1, (n, 3))
    P = pkg.make_particles(pos, d["mass"], type=np.where(d["type"] == 7, 0, d["type"]))
    P["Flags"][d["type"] == 7] = 1
    a = host_columns(d, n)
    eng.cooling_and_starformation(P, 1.0, a, T, step, ActiveParticle=act)
    host = dict(a, **eng.sfr_export())
    assert eng.sfr_result() == dev["result"]
    for k in IO + ("stellarmass", "parent", "spawn", "mass_of_star", "maybewind"):
        assert np.array_equal(host[k], dev[k]), k
    for k in READ:
        assert np.array_equal(a[k], d[k]), k
    assert np.array_equal(eng.cooling_export(n), dev["evals"]) and np.array_equal(eng.sfr_export_rows(n)[1], dev["sfevals"])
    eng.close()
    # the resident form: a gas stretch whose Density / Entropy / TimeBinHydro columns hold the table's
    eng = pkg.Engine(0)
    configure(eng, S)
    eng.set_gravshort_treepar()
    eng.gravshort_set_softenings(1.0 / 12)
    eng.set_densitypar(1.0, 2.0, 2.0, 99999., pkg.engine.DENSITY_KERNEL_QUINTIC_SPLINE, 0.006)
    eng.set_hydropar(0, 100.0, 0.75)
    z = lambda *s: np.zeros(s)
    sph = dict(hsml=d["hsml"].copy(), dthsml=z(n), vel=z(n, 3), gacc=z(n, 3), gpm=z(n, 3), entropy=d["entropy"].copy(), density=d["density"].copy(),
               egywtdensity=z(n), dhsmlegyfac=z(n), divvel=d["divvel"].copy(), curlvel=d["curlvel"].copy(), hydroacc_out=z(n, 3), dtentropy_out=z(n), maxsignalvel=z(n),
               tb_grav=d["tb_hydro"].copy(), tb_hydro=d["tb_hydro"].copy())
    eng.resident_begin(P, 1.0)
    eng.resident_sph_begin(P, sph)
    ptr = eng.resident_sph_arrays()
    d_ent, d_rho = device_view(torch, ptr["entropy"], n), device_view(torch, ptr["density"], n)
    d_rho.copy_(torch.from_numpy(d["density"]).cuda())              # (the upload of begin holds them already; written again to be sure of the columns)
    d_ent.copy_(torch.from_numpy(d["entropy"]).cuda())
    a = host_columns(d, n)
    for k in ("density", "entropy", "tb_hydro", "hsml", "divvel", "curlvel"):           # the resident columns: not read from the host
        a[k] = None
    eng.resident_sph_cooling_and_starformation(P, a, T, step, ActiveParticle=act)
    resident = dict(a, **eng.sfr_export())
    assert eng.sfr_result() == dev["result"]
    assert np.array_equal(d_ent.cpu().numpy(), dev["entropy"])
    for k in ("ne", "sfr", "metallicity", "delaytime", "bhheated", "vel", "stellarmass", "parent", "spawn", "mass_of_star", "maybewind"):
        assert np.array_equal(resident[k], dev[k]), k
    # the one refusal that belongs to this form: WindOn with WIND_SUBGRID (the kicks would have to reach the resident Vel); nothing is written
    eng.set_sfr_params(dict(SF.engine_params(S.p), WindOn=1))
    b = host_columns(d, n)
    for k in ("density", "entropy", "tb_hydro", "hsml", "divvel", "curlvel"):
        b[k] = None
    with pytest.raises(pkg.EngineError, match="WIND_SUBGRID is not carried on a resident gas run"):
        eng.resident_sph_cooling_and_starformation(P, b, T, step, ActiveParticle=act)
    assert np.array_equal(d_ent.cpu().numpy(), dev["entropy"]) and np.array_equal(b["ne"], d["ne"]) and np.array_equal(b["vel"], d["vel"])
    eng.resident_sph_end(sph)
    eng.resident_end(P)
    assert np.array_equal(sph["entropy"], dev["entropy"])          # the stretch hands the new entropies back
    eng.close()


# ---- the subgrid winds at the end of the call -------------------------------------------------------------------------------------------------
def test_wind_subgrid_chain(pkg):
    """with WindOn and WIND_SUBGRID the call equals the call without WindOn followed by mpg_dev_winds_subgrid on the exported list, bit for bit
    (also when that list is taken from the device without a host trip); kicks are applied"""
    import torch
    S, times, step, d, res = reference("density", 1)
    n = len(d["type"])
    eng = pkg.Engine(0)
    T = sph_times(pkg, times)
    configure(eng, S, wind_on=1)
    a1, keep1 = bind(torch, eng, d, n)
    eng.dev_cooling_and_starformation(a1, T, step)
    stats = eng.winds_stats()
    assert stats["stars"] == len(res["maybewind"]) > 500 and stats["applied"] > 20
    lists1 = eng.sfr_export()
    outs = []
    for from_device in (False, True):
        configure(eng, S, wind_on=0)
        a2, keep2 = bind(torch, eng, d, n)
        eng.dev_cooling_and_starformation(a2, T, step)
        lists2 = eng.sfr_export()
        for k in lists1:
            assert np.array_equal(lists1[k], lists2[k]), k
        assert torch.equal(a2["vel"], torch.from_numpy(d["vel"]).cuda())              # no kick yet
        if from_device:
            mw = eng.sfr_dev_lists()["maybewind"]
            W = pkg.engine.WindArraysC()
            for k in ("id", "vdisp", "density", "vel", "entropy", "delaytime"):
                setattr(W, k, a2[k].data_ptr())
            import ctypes as C
            eng._ck(eng.lib.mpg_dev_winds_subgrid(eng.h, C.byref(W), C.c_void_p(mw), C.c_int64(len(lists2["maybewind"])), C.c_void_p(a2["stellarmass"].data_ptr()),
                                                  C.c_double(times["atime"])))
        else:
            eng.dev_winds_subgrid(a2, torch.from_numpy(lists2["maybewind"]).cuda(), a2["stellarmass"], times["atime"])
        eng.synchronize()
        assert eng.winds_stats()["applied"] == stats["applied"]
        for k in IO + ("stellarmass",):
            assert torch.equal(a1[k], a2[k]), k
        outs.append(a2)
    kicked = (a1["vel"].cpu().numpy() != d["vel"]).any(axis=1)
    assert kicked.sum() == stats["applied"] and np.isin(np.nonzero(kicked)[0], res["maybewind"]).all()
    assert (a1["delaytime"].cpu().numpy()[kicked] > 0).all()
    # a model without WIND_SUBGRID: WindOn changes nothing
    configure(eng, S, wind_on=1, model=SF.WIND_USE_HALO)
    out, err = run_dev(torch, eng, d, T, step, n)
    assert err is None, err
    compare(d, res, out, n, "WindOn without WIND_SUBGRID")
    eng.close()


# ---- errors -----------------------------------------------------------------------------------------------------------------------------------
def test_iteration_limit_is_an_error_return(pkg):
    """a star-forming row that exhausts the test-only network limit (finite input; the limit lowered until exactly one star-forming row of the
    list needs more): a non-zero return, that row untouched, in no list and no sum, every other row correct; the next call succeeds"""
    import torch
    name, mode = "density", 3
    S, times, step, d, res = reference(name, mode)
    n = len(d["type"])
    maxfp = np.zeros(n, np.int64)
    for i, o in res["info"].items():
        maxfp[i] = o["maxfp"]
    worst = int(np.argmax(maxfp))
    limit = int(maxfp[worst]) - 1
    assert limit >= 2
    # the cooled rows need more iterations than any star-forming row: they stay out of the list, as do the rows that tie with the worst
    act = np.array([i for i in range(n) if res["cls"][i] != SF.ROW_COOLED and (i == worst or maxfp[i] <= limit)], np.int32)
    assert (res["cls"][act] == SF.ROW_STARFORMING).sum() > 150
    Cl = R.Cooling(dict(S.C.p, test_network_maxiter=limit), S.C.tc, S.C.metal)
    dd = SF.cooling_and_starformation(SF.Sfr(Cl, S.p), d, times, step, SF.random_table(), active=act, wind=SF.WIND)
    assert dd["failed"] == [worst]                             # the restatement fails on it too, and on it alone
    eng = pkg.Engine(0)
    T = sph_times(pkg, times)
    configure(eng, S, test_network_maxiter=limit)
    out, err = run_dev(torch, eng, d, T, step, n, active=act)
    assert isinstance(err, pkg.EngineError) and "iteration limit" in str(err)
    assert out["result"]["errors"] == 1 and out["stats"]["errors"] == 1 and out["sfevals"][worst] >= 2 * limit
    assert worst not in out["parent"] and worst not in out["maybewind"]
    compare(d, dd, out, n, "limit %d" % limit, bad=[worst])
    configure(eng, S)
    out, err = run_dev(torch, eng, d, T, step, n, active=act)
    assert err is None, err
    compare(d, restate(name, mode, S, times, step, d, n, active=act)[1], out, n, "after the error")
    # missing columns and parameters are error returns too
    a, keep = bind(torch, eng, d, n)
    for missing in ("id", "density", "entropy", "ne", "sfr", "metallicity"):
        with pytest.raises(pkg.EngineError, match="required"):
            eng.dev_cooling_and_starformation(dict(a, **{missing: None}), T, step)
    eng.set_sfr_params(dict(SF.engine_params(S.p), StarformationCriterion=SF.CRIT_MOLECULAR_H2))
    with pytest.raises(pkg.EngineError, match="gradrho_mag"):
        eng.dev_cooling_and_starformation(dict(a, gradrho_mag=None), T, step)
    eng.set_sfr_params(dict(SF.engine_params(S.p), StarformationCriterion=SF.CRIT_SELFGRAVITY))
    with pytest.raises(pkg.EngineError, match="divvel"):
        eng.dev_cooling_and_starformation(dict(a, divvel=None), T, step)
    eng.set_sfr_params(dict(SF.engine_params(S.p), WindOn=1))
    with pytest.raises(pkg.EngineError, match="WIND_SUBGRID"):
        eng.dev_cooling_and_starformation(dict(a, stellarmass=None), T, step)
    e2 = pkg.Engine(0)
    e2.dev_bind_particles(keep["pos"], keep["mass"], 1.0, type=keep["type"])
    with pytest.raises(pkg.EngineError, match="mpg_set_sfr_params"):
        e2.dev_cooling_and_starformation(a, T, step)
    e2.close()
    eng.close()


def test_refused_settings(pkg):
    """mpg_set_sfr_params names the setting it refuses: BHFeedbackUseTcool == 2, a UV-fluctuation table, EXCUR_REION, several ranks"""
    S = reference("density", 1)[0]
    eng = pkg.Engine(0)
    for over, text in ((dict(BHFeedbackUseTcool=2), "BHFeedbackUseTcool == 2"), (dict(UVFluctuationOn=1), "UVFluctuationOn"),
                       (dict(ExcursionSetReion=1), "EXCUR_REION"), (dict(NTask=2), "NTask")):
        with pytest.raises(pkg.EngineError, match=text):
            eng.set_sfr_params(dict(SF.engine_params(S.p), **over))
    eng.set_sfr_params(SF.engine_params(S.p))
    eng.close()


# ---- no side effects --------------------------------------------------------------------------------------------------------------------------
def test_dev_cooling_unchanged_by_a_star_formation_call(pkg):
    """mpg_dev_cooling on the same table before and after a star-formation call: bit-equal columns, counts and statistics"""
    import torch
    S, times, step, d, res = reference("density", 1)
    n = 520
    eng = pkg.Engine(0)
    configure(eng, S)
    T = sph_times(pkg, times)

    def cool():
        a, keep = bind(torch, eng, d, n)
        eng.dev_cooling({k: a[k] for k in ("density", "entropy", "ne", "sfr", "metallicity", "heiii_ionized", "tb_hydro")}, T, step)
        eng.synchronize()
        return {k: a[k].cpu().numpy() for k in ("entropy", "ne", "sfr")}, eng.cooling_export(n), eng.cooling_stats()

    before = cool()
    out, err = run_dev(torch, eng, d, T, step, n)
    assert err is None and out["result"]["sum_sf_part"] > 100
    after = cool()
    assert before[2] == after[2] and np.array_equal(before[1], after[1]) and before[2]["treated"] > 300
    for k in before[0]:
        assert np.array_equal(before[0][k], after[0][k]), k
    eng.close()
