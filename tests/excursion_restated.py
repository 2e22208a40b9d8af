"""Plain-Python restatement of the excursion set's consumer in MP-Gadget's cooling and star formation (libgadget/cooling_uvfluc.c:199-246),
statement by statement: get_local_UVBG_from_J21 with get_self_shield_dens (cooling_rates.c:345-361, cooling_restated's), the switch
get_local_UVBG, and the loops of cooling_direct and cooling_and_starformation with the background of every row taken from it.  The loops are
those of cooling_restated and sfr_restated, imported and not edited, wrapped as uvfluc_restated wraps them around
get_local_UVBG_from_global: every listed row runs through them alone with its own background and the sums are added in list order.
Test infrastructure: tests/test_excursion_restated.py pins it, tests/test_gpu_excursion.py compares the engine with it."""
import os

import numpy as np

import cooling_restated as R
import sfr_restated as SF
import uvfluc_restated as U

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "J21_to_rates_test.txt")
UVBG_MEMBERS = ("J_UV", "gJH0", "gJHep", "gJHe0", "epsH0", "epsHep", "epsHe0", "self_shield_dens", "zreion")   # struct UVBG, cooling.h:9-19


# ---- cooling_uvfluc.c -------------------------------------------------------------------------------------------------------------------------
def get_local_UVBG_from_J21(C, exc, redshift, J21, zreion):           # :199-231; exc["coeffs"] is get_J21_coeffs(AlphaUV)
    uvbg = R.zero_uvbg()
    uvbg["J_UV"] = J21
    uvbg["zreion"] = zreion
    J21toUV = exc["coeffs"]
    uvbg["gJH0"] = J21toUV["gJH0"] * J21
    uvbg["epsH0"] = J21toUV["epsH0"] * J21 * 1.60218e-12
    uvbg["gJHe0"] = J21toUV["gJHe0"] * J21
    uvbg["epsHe0"] = J21toUV["epsHe0"] * J21 * 1.60218e-12
    uvbg["gJHep"] = 0.
    uvbg["epsHep"] = 0.
    uvbg["self_shield_dens"] = C.get_self_shield_dens(redshift, uvbg)
    return uvbg


def j21_mode(exc, redshift):                                          # :238
    return bool(exc is not None and exc["ExcursionSetReionOn"] and redshift > exc["ExcursionSetZStop"])


def get_local_UVBG(C, exc, redshift, GlobalUVBG, Pos, PosOffset, uvf, J21, zreion):   # :236-246
    if j21_mode(exc, redshift):
        return get_local_UVBG_from_J21(C, exc, redshift, J21, zreion)
    return U.get_local_UVBG_from_global(redshift, GlobalUVBG, Pos, PosOffset, uvf)


# the classes of a row of the two columns
NEVER, WINDOW, LIT = 0, 1, 2


# ---- the loops --------------------------------------------------------------------------------------------------------------------------------
def cool_particles_j21(C, exc, d, J21, zreion, times, step, active=None, pos=None, offset=None, uvf=None):
    """cooling_restated.cool_particles with the background of every row from get_local_UVBG (sfr_eff.c:477-478).  Returns its dict."""
    n = len(d["type"])
    out = dict(entropy=d["entropy"].copy(), ne=d["ne"].copy(), sfr=d["sfr"].copy(), evals=np.full(n, -1, np.int32), maxfp=np.zeros(n, np.int32),
               info={}, failed=[], cls=np.full(n, -1, np.int32))
    redshift = 1. / times["atime"] - 1
    for p in U._rows(d, active):
        if d["type"][p] != 0 or not d["mass"][p] > 0:
            continue
        uvbg = get_local_UVBG(C, exc, redshift, step["uvbg"], None if pos is None else pos[p], offset, uvf, float(J21[p]), float(zreion[p]))
        out["cls"][p] = 0
        r = R.cool_particles(C, U._one(d, p), times, dict(step, uvbg=uvbg))
        for k in ("entropy", "ne", "sfr", "evals", "maxfp"):
            out[k][p] = r[k][0]
        if r["failed"]:
            out["failed"].append(p)
        else:
            out["info"][p] = r["info"][0]
    return out


def cooling_and_starformation_j21(S, exc, d, J21, zreion, times, step, rnd, active=None, wind=None):
    """sfr_restated.cooling_and_starformation with the background of every row from get_local_UVBG (sfr_eff.c:745 for the star-forming
    rows, :477-478 for the cooled ones).  The lists and the three sums are put together in the order of the active list."""
    n = len(d["type"])
    out = {k: d[k].copy() for k in SF.COLUMNS_IO if d.get(k) is not None}
    out.update(stellarmass=np.zeros(n), cls=np.zeros(n, np.uint8), evals=np.full(n, -1, np.int32), sfevals=np.full(n, -1, np.int32))
    lists = dict(parent=[], mass_of_star=[], spawn=[], maybewind=[])
    sums = dict(sum_sm=0.0, localsfr=0.0, sum_dtime=0.0, sum_sf_part=0)
    failed, info = [], {}
    redshift = 1. / times["atime"] - 1
    for p in U._rows(d, active):
        if d["type"][p] != 0 or not d["mass"][p] > 0:
            continue
        uvbg = get_local_UVBG(S.C, exc, redshift, step["uvbg"], None, None, None, float(J21[p]), float(zreion[p]))
        r = SF.cooling_and_starformation(S, U._one(d, p), times, dict(step, uvbg=uvbg), rnd, wind=wind)
        for k in list(SF.COLUMNS_IO) + ["stellarmass", "cls", "evals", "sfevals"]:
            if k in out:
                out[k][p] = r[k][0]
        lists["parent"] += [p] * len(r["parent"])
        lists["maybewind"] += [p] * len(r["maybewind"])
        lists["mass_of_star"] += list(r["mass_of_star"])
        lists["spawn"] += list(r["spawn"])
        for k in sums:
            sums[k] += r[k]
        if r["failed"]:
            failed.append(p)
        if 0 in r["info"]:
            info[p] = r["info"][0]
    out.update(parent=np.array(lists["parent"], np.int32), mass_of_star=np.array(lists["mass_of_star"], np.float64),
               spawn=np.array(lists["spawn"], np.uint8), maybewind=np.array(lists["maybewind"], np.int32), failed=failed, info=info, **sums)
    return out


# ---- the input sets of the tests (tests/test_excursion_restated.py checks what they cover, tests/test_gpu_excursion.py runs them on the GPU) --
ALPHA_UV = 0.7                                                        # between two entries of the fixture
# ExcursionSetZStop per set: 2 on the z = 3 sets, so that the grey opacity of the self-shield density is interpolated there, not clamped
COOLING_SETS = dict(sherwood_reion=dict(n=1000, zstop=5.0, seed=31), sherwood_z3=dict(n=1000, zstop=2.0, seed=32))
SFR_SET = dict(name="heating", mode=3, n=1200, zstop=2.0, seed=33)


def model(zstop, on=1):
    """(the members of mpg_excursion_set_params, the same with the coefficients under "coeffs" for the restatement) from the fixture"""
    import importlib
    exc = importlib.import_module("mp-gadget_amd.excursion")
    par = exc.params(exc.J21Coeffs.load(GOLDEN), ALPHA_UV, on, zstop)
    return par, dict(par, coeffs={k: par[k] for k in exc.COLUMNS})


def columns(d, redshift, lastred, seed):
    """(local_J21, zreion, class) per row, drawn per row so that the classes mix inside every wave: a third never ionised (J21 = 0,
    zreion = -1); a third ionised this step (zreion inside [redshift, lastred[bin]) for even bins; for odd bins, and wherever the bin's
    step began at the redshift itself, lit just before the step began); a third lit earlier.  Lit rows: J21 = 1e-6 .. 1e3 log-uniform."""
    rs = np.random.RandomState(seed)
    n = len(d["type"])
    cls = rs.randint(0, 3, n)
    J21 = np.exp(rs.uniform(np.log(1e-6), np.log(1e3), n))
    last = np.asarray(lastred, np.float64)[d["tb_hydro"]]
    inside = redshift + rs.uniform(0.0, 1.0, n) * (last - redshift)                  # in [redshift, lastred) where lastred > redshift
    zre = np.where(cls == WINDOW, inside, last + rs.uniform(0.1, 3.0, n))
    odd = (d["tb_hydro"] % 2 == 1) | ~(inside < last)
    zre = np.where((cls == WINDOW) & odd, last + rs.uniform(0.1, 3.0, n), zre)
    cls = np.where((cls == WINDOW) & odd, LIT, cls)
    J21 = np.where(cls == NEVER, 0.0, J21)
    zre = np.where(cls == NEVER, -1.0, zre)
    return np.ascontiguousarray(J21), np.ascontiguousarray(zre), cls


def cooling_set(name, treecool_columns):
    """(Cooling, times, step, table of n rows, model for the engine, model for the restatement, J21, zreion, class) of a cooling set"""
    s = COOLING_SETS[name]
    C, times, step, make = R.config(name, treecool_columns)
    d = make(s["n"])
    par, exc = model(s["zstop"])
    J21, zre, cls = columns(d, 1. / times["atime"] - 1, step["lastred"], s["seed"])
    return C, times, step, d, par, exc, J21, zre, cls


def sfr_set(treecool_columns):
    """... of the star-formation set: the `heating` setting with BHFeedbackUseTcool = 3 (uvfluc_restated.sfr_set)"""
    s = SFR_SET
    S, times, step, make = SF.config(s["name"], treecool_columns, s["mode"])
    d = make(s["n"])
    par, exc = model(s["zstop"])
    J21, zre, cls = columns(d, 1. / times["atime"] - 1, step["lastred"], s["seed"])
    return S, times, step, d, par, exc, J21, zre, cls
