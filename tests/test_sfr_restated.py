"""tests/sfr_restated.py (the restatement of cooling_and_starformation the GPU tests compare csrc/sfr.hip with) held to identities that need no
second implementation, the host build of csrc/sfr.h held to it bit for bit, and the conditions under which tests/test_gpu_sfr.py may ask
for equal decisions, shown on the very inputs those tests use:
  - with every table lookup perturbed by +-2e-15 the network evaluation count of no star-forming row changes;
  - for every star-forming row |rnd - prob| > 1e-9;
  - for every row Density a3inv is not within 1e-12 relative of a threshold.
It also measures, per output column, the largest change those perturbations and a +-1-ulp perturbation of every pow / exp / sqrt / log
result of the model cause, and holds them below sfr_restated.SENSITIVITY, from which the GPU tests take their tolerances."""
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

import cooling_restated as R
import sfr_restated as SF
import test_cooling_restated as K

G = K.G
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODES = (0, 1, 3)                                   # BHFeedbackUseTcool
# the cases of the GPU tests (tests/test_gpu_sfr.py imports them): every setting with every mode; one large table, the others two blocks and a bit
CASES = [(name, mode) for name in SF.SETTINGS for mode in MODES]


def size_of(name, mode):
    return SF.SIZE if (name, mode) == ("density", 1) else 520


_base = {}


def base_run(name, mode):
    """the unperturbed restatement of a case's star-forming rows (the cooled rows are test_cooling_restated's subject)"""
    if (name, mode) not in _base:
        S, times, step, make = SF.config(name, G["treecool"], mode)
        d = make(size_of(name, mode))
        rnd = SF.random_table()
        _base[(name, mode)] = (S, times, step, d, rnd, SF.cooling_and_starformation(S, d, times, step, rnd, wind=SF.WIND, cool=False))
    return _base[(name, mode)]


def sf_rows(res):
    return np.array(sorted(res["info"]), np.int64)


# ---- identities -----------------------------------------------------------------------------------------------------------------------------
def test_cloudfrac_solves_its_quadratic():
    """(a) x = cloudfrac solves y (1 - x)^2 = x, for the y of every star-forming row of the main case and for synthetic y over 15 decades"""
    S, times, step, d, rnd, res = base_run("density", 1)
    ys = [res["info"][i]["y"] for i in sf_rows(res)] + list(np.exp(np.linspace(np.log(1e-3), np.log(1e12), 400)))
    assert len(ys) > 1500
    eps = 2.0 ** -52
    for y in ys:
        x = 1 + 1 / (2 * y) - math.sqrt(1 / y + 1 / (4 * y * y))
        # x is a difference of terms of size 1 + 1 / (2 y), so it carries an absolute error of a few eps of that; the residual
        # y (1 - x)^2 - x moves by (2 y (1 - x) + 1) times the error of x
        assert abs(y * (1 - x) ** 2 - x) <= 8 * eps * (1 + 1 / (2 * y)) * (2 * y * (1 - x) + 1), y
        assert 0 <= x <= 1
    # net heating: tcool = 0 gives y = inf, x = 1, trelax = 0
    y = SF.div(1.5, 0.0) * 3.0
    assert y == math.inf and 1 + SF.div(1, 2 * y) - math.sqrt(SF.div(1, y) + SF.div(1, 4 * y * y)) == 1.0


def test_cooling_relaxed_limits():
    """(b) cooling_relaxed returns the input at dtime -> 0 and egyeff at dtime >> trelax"""
    S, times, step, d, rnd, res = base_run("density", 0)
    a3inv = 1. / times["atime"] ** 3
    redshift = 1. / times["atime"] - 1
    seen = 0
    for i in sf_rows(res)[:200]:
        o = res["info"][i]
        if not (o["trelax"] > 0):
            continue
        r = dict(density=float(d["density"][i]), entropy=float(d["entropy"][i]))
        dd = dict(cloudfrac=o["cloudfrac"], trelax=o["trelax"], egyhot=S.p["EgySpecSN"] / (1 + R.pow_(r["density"] * a3inv / S.p["PhysDensThresh"], -0.8)
                                                                                            * S.p["FactorEVP"]) + S.p["EgySpecCold"])
        e0, _ = S.cooling_relaxed(r, dd, 0.0, step["uvbg"], redshift, a3inv, 1.0, 0.0, 0)
        assert abs(e0 / r["entropy"] - 1) < 1e-13
        e1, _ = S.cooling_relaxed(r, dd, 1e4 * o["trelax"], step["uvbg"], redshift, a3inv, 1.0, 0.0, 0)
        egyeff = S.p["EgySpecCold"] * dd["cloudfrac"] + (1 - dd["cloudfrac"]) * dd["egyhot"]
        assert e1 == egyeff / S.entropy_to_u(r["density"], a3inv)
        seen += 1
    assert seen > 100


def test_threshold_closure():
    """(c) with the threshold computed as sfr_eff.c:932-958 does, the effective energy at the threshold at z = 0 without a UV background is the
    1e4 K energy u4 (Verner96 / Sherwood in the unit system of test_cooling.c: PhysDensThresh = 7.2534e-4, egyeff / u4 = 1.0067)"""
    C = R.Cooling(R.default_params(), R.TreeCool(G["treecool"]))
    P = SF.init_star_formation(C)
    S = SF.Sfr(C, P)
    ratio = SF.get_egyeff(S, 0, P["PhysDensThresh"], SF.no_uvbg()) / P["u4"]
    print("PhysDensThresh = %.5g, egyeff / u4 = %.5f" % (P["PhysDensThresh"], ratio))
    assert abs(P["PhysDensThresh"] / 7.2534e-4 - 1) < 1e-3
    assert abs(ratio - 1) < 1e-2


def test_mass_and_metal_bookkeeping():
    """(d) the three outcomes: no star and a spawned star leave the particle both metallicity increments, a converted particle only the
    first; mass_of_star never exceeds the mass, a spawn leaves at least a tenth of a star behind, a conversion takes the whole particle"""
    seen = {SF.OUT_NOSTAR: 0, SF.OUT_CONVERT: 0, SF.OUT_SPAWN: 0}
    for name, mode in (("density", 1), ("boost", 0)):
        S, times, step, d, rnd, res = base_run(name, mode)
        Gen = S.p["Generations"]
        for i in sf_rows(res):
            o = res["info"][i]
            m, Z0 = float(d["mass"][i]), float(d["metallicity"][i])
            seen[o["outcome"]] += 1
            full = SF.METAL_YIELD * o["frac"] / Gen
            part = o["w"] * SF.METAL_YIELD * o["frac"] / Gen
            want = Z0 + (part if o["outcome"] == SF.OUT_CONVERT else full)
            assert abs(o["metallicity"] - want) <= 4e-16 * max(want, 1e-300) + 1e-18, (i, o["outcome"])
            assert 0 <= o["dM"] <= m and o["mass_of_star"] <= m and abs(o["prob"] * o["mass_of_star"] - o["dM"]) <= 1e-15 * m
            if o["outcome"] == SF.OUT_SPAWN:
                assert m - o["mass_of_star"] >= 0.1 * o["mass_of_star"] * (1 - 1e-7) and o["mass_of_star"] == S.p["avg_baryon_mass"] / Gen
                assert int(d["generation"][i]) <= Gen
            if o["outcome"] == SF.OUT_CONVERT:
                assert o["mass_of_star"] == m
        # the lists: parents in list order, the MaybeWind list the star-forming rows without a star, StellarMass theirs alone
        stars = [i for i in sf_rows(res) if res["info"][i]["outcome"] != SF.OUT_NOSTAR]
        assert list(res["parent"]) == stars and list(res["maybewind"]) == [i for i in sf_rows(res) if res["info"][i]["outcome"] == SF.OUT_NOSTAR]
        other = np.ones(len(d["type"]), bool)
        other[res["maybewind"]] = False
        assert (res["stellarmass"][res["maybewind"]] >= 0).all() and (res["stellarmass"][res["maybewind"]] > 0).sum() > 100 and not res["stellarmass"][other].any()
        assert res["sum_sf_part"] == len(sf_rows(res)) + len(res["failed"])
    print("outcomes:", seen)
    assert min(seen.values()) > 30


def test_input_sets_cover_the_branches():
    """what the issue asks the input tables to mix, read off the restatement's record"""
    S, times, step, d, rnd, res = base_run("density", 1)
    n = len(d["type"])
    a3inv = 1. / times["atime"] ** 3
    gas = (d["type"] == 0) & (d["mass"] > 0)
    assert (d["type"] == 7).any() and (d["type"] == 1).any() and (d["mass"] <= 0).any()
    sf = res["cls"] == SF.ROW_STARFORMING
    assert sf.sum() > 1500 and (res["cls"] == SF.ROW_COOLED).sum() > 800 and not (sf & ~gas).any()
    above = d["density"] * a3inv >= S.p["PhysDensThresh"]
    assert (gas & above & (d["delaytime"] > 0) & ~sf).sum() > 50          # in the wind: cooled although dense
    assert (sf & (d["bhheated"] == 1)).sum() > 50 and (sf & (d["tb_hydro"] == 0)).sum() > 10 and set(d["tb_hydro"][sf]) == set(range(47))
    u = d["entropy"] * np.array([R.Cooling.entropy_to_u(float(x), a3inv) for x in d["density"]])
    assert (sf & (u > 5e6)).sum() > 50
    assert (sf & (d["generation"] > S.p["Generations"])).sum() > 100
    mos = S.p["avg_baryon_mass"] / S.p["Generations"]
    assert (sf & (d["mass"] < 2 * mos)).sum() > 100 and (sf & (d["mass"] == np.float32(2 * mos))).sum() > 5 and (sf & (d["mass"] == np.float32(1.1 * mos))).sum() > 5
    assert (d["ne"][sf] == 0).sum() > 50 and (d["metallicity"][sf] > 0).sum() > 500 and (d["metallicity"][sf] == 0).sum() > 100
    ev = res["sfevals"][sf_rows(res)]
    print("evaluations per star-forming row: %d .. %d; y %.3g .. %.3g; cloudfrac %.3g .. %.4g" % (
        ev.min(), ev.max(), min(o["y"] for o in res["info"].values()), max(o["y"] for o in res["info"].values()),
        min(o["cloudfrac"] for o in res["info"].values()), max(o["cloudfrac"] for o in res["info"].values())))
    # the second cooling time of cooling_relaxed is taken in modes 1 and 3, never in mode 0
    ev0 = base_run("density", 0)[5]["sfevals"]
    ev3 = base_run("density", 3)[5]["sfevals"]
    common = sf_rows(base_run("density", 0)[5])
    assert (ev3[common] > ev0[common]).sum() > 50
    # the synthetic heating case: every cooling time is 0
    Sh, th, sh, dh, rh, resh = base_run("heating", 1)
    assert all(o["tcool"] == 0 and o["cloudfrac"] == 1 and o["trelax"] == 0 for o in resh["info"].values()) and len(resh["info"]) > 200
    # Quick Lyman alpha: conversions only, no column of a star-forming row changes
    Sq, tq, sq, dq, rq, resq = base_run("quicklya", 0)
    qsf = resq["cls"] == SF.ROW_STARFORMING
    assert qsf.sum() > 50 and (resq["cls"] == SF.ROW_COOLED).sum() > 100 and len(resq["parent"]) == qsf.sum() and not resq["spawn"].any()
    assert np.array_equal(resq["mass_of_star"], dq["mass"][resq["parent"]].astype(np.float64)) and len(resq["maybewind"]) == 0


# ---- what the GPU tests may demand ----------------------------------------------------------------------------------------------------------
measured = {}


@pytest.mark.parametrize("name,mode", CASES)
def test_decisions_are_stable_on_the_gpu_tests_inputs(name, mode):
    S, times, step, d, rnd, base = base_run(name, mode)
    assert not base["failed"]
    rows = sf_rows(base)
    a3inv = 1. / times["atime"] ** 3
    # no density on a threshold
    gas = (d["type"] == 0) & (d["mass"] > 0)
    for thr, x in ((S.p["PhysDensThresh"], d["density"] * a3inv), (S.p["OverDensThresh"], d["density"]), (100 * S.p["PhysDensThresh"], d["density"] * a3inv),
                   (S.p["BoostSFOverDenseFactor"] * S.p["PhysDensThresh"], d["density"] * a3inv)):
        assert (np.abs(x[gas] / thr - 1) > 1e-12).all()
    if name == "quicklya":
        assert all(abs(float(rnd[((int(d["id"][i]) + 1) % (1 << 64)) % len(rnd)]) - S.p["QuickLymanAlphaProbability"]) > 1e-9 for i in np.nonzero(gas)[0])
        return
    # no draw near its probability
    gap = min(abs(float(rnd[((int(d["id"][i]) + 1) % (1 << 64)) % len(rnd)]) - base["info"][i]["prob"]) for i in rows)
    assert gap > 1e-9, gap
    worst = dict.fromkeys(SF.SENSITIVITY, 0.0)
    worst.update(sum_sm=0.0, localsfr=0.0, sum_dtime=0.0)
    for perturb, ulp in ((2e-15, 0), (-2e-15, 0), (0.0, 1), (0.0, -1)):
        Sp = SF.config(name, G["treecool"], mode, perturb=perturb, ulp=ulp)[0]
        Sp.p = S.p                                 # (the threshold is the caller's, computed once)
        r = SF.cooling_and_starformation(Sp, d, times, step, rnd, wind=SF.WIND, cool=False)
        assert not r["failed"]
        if ulp == 0:
            assert np.array_equal(r["sfevals"], base["sfevals"])               # the evaluation count of no row changes
        same = rows[r["sfevals"][rows] == base["sfevals"][rows]]
        assert len(same) >= 0.999 * len(rows)
        assert np.array_equal(r["cls"], base["cls"]) and np.array_equal(r["parent"], base["parent"]) and np.array_equal(r["spawn"], base["spawn"])
        assert np.array_equal(r["maybewind"], base["maybewind"]) and np.array_equal(r["mass_of_star"], base["mass_of_star"])
        for k in ("entropy", "ne", "sfr", "metallicity"):
            worst[k] = max(worst[k], float(SF.column_error(k, r[k][same], base[k][same]).max()))
        mw = np.intersect1d(base["maybewind"], same)
        if len(mw):
            worst["stellarmass"] = max(worst["stellarmass"], float(SF.column_error("stellarmass", r["stellarmass"][mw], base["stellarmass"][mw]).max()))
        for k in ("sum_sm", "localsfr", "sum_dtime"):
            worst[k] = max(worst[k], abs(r[k] / base[k] - 1) if base[k] else 0.0)
    measured[(name, mode)] = worst
    print("sensitivity %s / %d (%d rows): %s" % (name, mode, len(rows), ", ".join("%s %.1e" % kv for kv in worst.items())))
    for k, lim in SF.SENSITIVITY.items():
        assert worst[k] <= lim, (k, worst[k], lim)
    assert max(worst["sum_sm"], worst["localsfr"], worst["sum_dtime"]) < 1e-13


# ---- the host build of csrc/sfr.h -------------------------------------------------------------------------------------------------------------
COOLING_KEYS = ("recomb", "cooling", "SelfShieldingOn", "HeliumHeatOn", "CoolingOn", "test_network_maxiter", "CMBTemperature", "MinGasTemp",
                "HeliumHeatThresh", "HeliumHeatAmp", "HeliumHeatExp", "rho_crit_baryon", "density_in_phys_cgs", "uu_in_cgs", "tt_in_s",
                "units_rho_crit_baryon", "sfr_MinGasTemp", "temp_to_u", "HIReionTemp")
UVBG_KEYS = ("J_UV", "gJH0", "gJHep", "gJHe0", "epsH0", "epsHep", "epsHe0", "self_shield_dens", "zreion")
ROW_KEYS = ("density", "entropy", "ne", "metallicity", "delaytime", "hsml", "divvel", "curlvel", "gradrho_mag", "mass", "generation", "bhheated")


@pytest.fixture(scope="module")
def sfr_host(tmp_path_factory):
    """csrc/sfr.h compiled for the host with its own main (tests/c/sfr_host.cpp); the HIP headers are needed for the types only"""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    inc = os.path.join(os.path.dirname(os.path.dirname(hipcc)), "include")
    if not shutil.which("g++") or not os.path.isdir(inc):
        pytest.fail("no g++ or no HIP headers: the host build of csrc/sfr.h cannot be checked")
    exe = str(tmp_path_factory.mktemp("sfr_host") / "sfr_host")
    r = subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Wno-unused-function", "-Wno-unused-result", "-D__HIP_PLATFORM_AMD__", "-I", inc,
                        os.path.join(ROOT, "tests", "c", "sfr_host.cpp"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


@pytest.mark.parametrize("name,mode", [("density", 1), ("h2", 3), ("selfgravity", 0), ("selfgravity_plain", 1), ("boost", 3), ("heating", 1)])
def test_host_build_of_sfr_h_equals_the_restatement(sfr_host, tmp_path, name, mode):
    """(e) sfr::starformation of csrc/sfr.h, built for the host, on the star-forming rows of a case: every result bit for bit the restatement's"""
    S, times, step, d, rnd, base = base_run(name, mode)
    rows = sf_rows(base)
    C = S.C
    maxiter = C.p.get("test_network_maxiter", 0) or R.MAXITER
    head = [float(len(rows))] + [float(maxiter if k == "test_network_maxiter" else C.p[k]) for k in COOLING_KEYS] + [step["uvbg"][k] for k in UVBG_KEYS]
    head += [1. / times["atime"] - 1, step["long_mean_free_path_heating"]]
    head += [float(S.p[k]) for k in SF.ENGINE_KEYS[:18]] + [times["hubble"], times["atime"]]
    M = C.metal
    head += [float(x) for x in M.dims] + M.Min + M.Max + M.data
    body = []
    for i in rows:
        ID = int(d["id"][i])
        b = min(int(d["tb_hydro"][i]), 46)
        body += [float(base["delaytime"][i] if k == "delaytime" else d[k][i]) for k in ROW_KEYS] + [float(b), float(times["dloga_bin"][b]), float(rnd[ID % len(rnd)]), float(rnd[((ID + 1) % (1 << 64)) % len(rnd)])]
    fin, fout = str(tmp_path / "in.f64"), str(tmp_path / "out.f64")
    np.array(head + body, np.float64).tofile(fin)
    r = subprocess.run([sfr_host, fin, fout], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    out = np.fromfile(fout, np.float64).reshape(len(rows), 12)
    # delaytime as the loop left it (winds_evolve): the star-forming rows have none
    assert (base["delaytime"][rows] <= 0).all()
    cols = dict(entropy=0, ne=1, sfr=2, metallicity=3, bhheated=4)
    for k, c in cols.items():
        assert np.array_equal(out[:, c], base[k][rows].astype(np.float64)), k
    info = [base["info"][i] for i in rows]
    for c, k in ((5, "sm"), (6, "dM"), (7, "mass_of_star"), (8, "outcome"), (10, "cloudfrac"), (11, "dtime")):
        assert np.array_equal(out[:, c], np.array([float(o[k]) for o in info])), k
    assert np.array_equal(out[:, 9], base["sfevals"][rows].astype(np.float64))
