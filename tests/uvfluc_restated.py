"""Plain-Python restatement of MP-Gadget's patchy reionisation (libgadget/cooling_uvfluc.c:115-197 on libgadget/utils/interp.c), statement by
statement: the periodic multilinear read of Zreion_Table with the reference's `while` wraps, get_local_UVBG_from_global, and the loops of
cooling_direct and cooling_and_starformation with the background of every row taken from it.  The loops are those of cooling_restated and
sfr_restated, imported and not edited: they take the background as an argument, so every listed row is run through them alone with its own
background and the sums are added in the order of the active list, which is the order the one loop of the reference adds them in.
Test infrastructure: tests/test_uvfluc_restated.py pins it, tests/test_gpu_uvfluc.py compares the engine with it."""
import math

import numpy as np

import cooling_restated as R
import sfr_restated as SF


# ---- utils/interp.c ---------------------------------------------------------------------------------------------------------------------------
class Interp:
    """interp_init (:9-43) and interp_init_dim (:50-54)"""

    def __init__(self, dims):
        self.Ndim = len(dims)
        self.dims = [int(x) for x in dims]
        self.strides = [0] * self.Ndim
        N = 1
        for d in range(self.Ndim - 1, -1, -1):                        # column first, C ordering
            self.strides[d] = N
            N *= self.dims[d]
        self.fsize = 1
        for d in range(self.Ndim):
            self.fsize *= 2
        self.Min, self.Max, self.Step = [0.0] * self.Ndim, [0.0] * self.Ndim, [0.0] * self.Ndim

    def init_dim(self, d, Min, Max):
        self.Min[d] = Min
        self.Max[d] = Max
        self.Step[d] = (Max - Min) / (self.dims[d] - 1)


def linearindex(strides, xi, Ndim):                                   # :57-64
    rt = 0
    for d in range(Ndim):
        rt += strides[d] * xi[d]
    return rt


def interp_cells(obj, x):
    """the first loop of interp_eval_periodic (:140-144): (xi, f) per axis"""
    xi, f = [0] * obj.Ndim, [0.0] * obj.Ndim
    for d in range(obj.Ndim):
        xd = (x[d] - obj.Min[d]) / obj.Step[d]
        xi[d] = int(math.floor(xd))
        f[d] = xd - xi[d]
    return xi, f


def interp_eval_periodic(obj, x, ydata, modulo=False):
    """:134-170 on the flat array ydata.  modulo: the wrap as one integer modulo that handles negative cells (what the engine does) in place
    of the two `while` loops"""
    xi, f = interp_cells(obj, x)
    xi1 = [0] * obj.Ndim
    ret = 0.0
    for i in range(obj.fsize):
        filter = 1.0
        for d in range(obj.Ndim):
            foffset = 1 if (i & (1 << d)) else 0
            xi1[d] = xi[d] + foffset
            if modulo:
                xi1[d] = xi1[d] % obj.dims[d]                         # (Python's %: the sign of the divisor)
            else:
                while xi1[d] >= obj.dims[d]:
                    xi1[d] -= obj.dims[d]
                while xi1[d] < 0:
                    xi1[d] += obj.dims[d]
            filter *= f[d] if foffset else (1 - f[d])
        l = linearindex(obj.strides, xi1, obj.Ndim)
        ret += ydata[l] * filter
    return ret


# ---- cooling_uvfluc.c -------------------------------------------------------------------------------------------------------------------------
class UVF:
    """init_uvf_table (:115-167) without the file: Table[Nside][Nside][Nside] in C order, interp_init_dim(d, 0, BoxSize)"""

    def __init__(self, table, BoxSize):
        table = np.ascontiguousarray(table, np.float64)
        self.Nside = table.shape[0]
        assert table.shape == (self.Nside,) * 3
        self.Table = [float(v) for v in table.ravel()]
        self.interp = Interp([self.Nside] * 3)
        for d in range(3):
            self.interp.init_dim(d, 0, BoxSize)
        assert not (self.Table[0] < 0.01 or self.Table[0] > 100.0)     # :164
        self.enabled = 1

    def zreion(self, Pos, PosOffset):                                 # :185-189
        corrpos = [float(Pos[i]) - float(PosOffset[i]) for i in range(3)]
        return interp_eval_periodic(self.interp, corrpos, self.Table)


def get_local_UVBG_from_global(redshift, GlobalUVBG, Pos, PosOffset, uvf):   # :174-197
    if uvf is None or not uvf.enabled:
        return dict(GlobalUVBG)
    uvbg = R.zero_uvbg()
    uvbg["self_shield_dens"] = GlobalUVBG["self_shield_dens"]
    zreion = uvf.zreion(Pos, PosOffset)
    if zreion < redshift:
        uvbg["zreion"] = zreion
        return uvbg
    uvbg = dict(GlobalUVBG)
    uvbg["zreion"] = zreion
    return uvbg


DARK, WINDOW, LIT = 0, 1, 2


def row_class(zreion, redshift, lastred):
    """what a row's result depends on: dark (zreion < redshift), in the window [redshift, lastred of its bin) that the HIReionTemp test of
    sfr_eff.c:488 asks for, or after it"""
    if zreion < redshift:
        return DARK
    return WINDOW if zreion < lastred else LIT


def synthetic_zreion_table(Nside, zmid, seed):
    """a smooth field plus 5 % noise around zmid: zmid + 0.15 + 0.9 sin cos + 0.5 sin + 0.05 noise on the grid i / Nside"""
    rs = np.random.RandomState(seed)
    g = np.arange(Nside) / float(Nside)
    x, y, z = np.meshgrid(g, g, g, indexing="ij")
    t = zmid + 0.15 + 0.9 * np.sin(2 * np.pi * x) * np.cos(2 * np.pi * y) + 0.5 * np.sin(2 * np.pi * (z + 0.3 * x)) + 0.05 * rs.normal(size=(Nside,) * 3)
    return np.ascontiguousarray(t)


# ---- the loops --------------------------------------------------------------------------------------------------------------------------------
def _rows(d, active):
    n = len(d["type"])
    return range(n) if active is None else [int(x) for x in active if 0 <= int(x) < n]


def _one(d, p):
    return {k: (None if v is None else v[p:p + 1]) for k, v in d.items()}


def cool_particles_local(C, d, pos, offset, uvf, times, step, active=None):
    """cooling_restated.cool_particles with the background of every row from get_local_UVBG (sfr_eff.c:477-478).  Returns its dict, with
    zreion (NaN: row not treated) and cls (DARK / WINDOW / LIT, -1: not treated) per particle besides."""
    n = len(d["type"])
    out = dict(entropy=d["entropy"].copy(), ne=d["ne"].copy(), sfr=d["sfr"].copy(), evals=np.full(n, -1, np.int32), maxfp=np.zeros(n, np.int32),
               info={}, failed=[], zreion=np.full(n, np.nan), cls=np.full(n, -1, np.int32))
    redshift = 1. / times["atime"] - 1
    lastred = np.broadcast_to(np.asarray(step.get("lastred", 0.0), np.float64), (47,))
    for p in _rows(d, active):
        if d["type"][p] != 0 or not d["mass"][p] > 0:
            continue
        uvbg = get_local_UVBG_from_global(redshift, step["uvbg"], pos[p], offset, uvf)
        b = int(d["tb_hydro"][p]) if d.get("tb_hydro") is not None else 0
        out["zreion"][p] = uvbg["zreion"]
        out["cls"][p] = row_class(uvbg["zreion"], redshift, float(lastred[b]))
        r = R.cool_particles(C, _one(d, p), times, dict(step, uvbg=uvbg))
        for k in ("entropy", "ne", "sfr", "evals", "maxfp"):
            out[k][p] = r[k][0]
        if r["failed"]:
            out["failed"].append(p)
        else:
            out["info"][p] = r["info"][0]
    return out


def cooling_and_starformation_local(S, d, pos, offset, uvf, times, step, rnd, active=None, wind=None):
    """sfr_restated.cooling_and_starformation with the background of every row from get_local_UVBG (sfr_eff.c:745 for the star-forming
    rows, :477-478 for the cooled ones).  The lists and the three sums are put together in the order of the active list."""
    n = len(d["type"])
    out = {k: d[k].copy() for k in SF.COLUMNS_IO if d.get(k) is not None}
    out.update(stellarmass=np.zeros(n), cls=np.zeros(n, np.uint8), evals=np.full(n, -1, np.int32), sfevals=np.full(n, -1, np.int32),
               zreion=np.full(n, np.nan), dark=np.zeros(n, bool))
    lists = dict(parent=[], mass_of_star=[], spawn=[], maybewind=[])
    sums = dict(sum_sm=0.0, localsfr=0.0, sum_dtime=0.0, sum_sf_part=0)
    failed, info = [], {}
    redshift = 1. / times["atime"] - 1
    for p in _rows(d, active):
        if d["type"][p] != 0 or not d["mass"][p] > 0:
            continue
        uvbg = get_local_UVBG_from_global(redshift, step["uvbg"], pos[p], offset, uvf)
        out["zreion"][p] = uvbg["zreion"]
        out["dark"][p] = uvbg["zreion"] < redshift
        r = SF.cooling_and_starformation(S, _one(d, p), times, dict(step, uvbg=uvbg), rnd, wind=wind)
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


# ---- the input sets of the tests (tests/test_uvfluc_restated.py checks what they cover, tests/test_gpu_uvfluc.py runs them on the GPU) ------
NSIDE, BOXSIZE, OFFSET = 5, 1.0, (0.11, -0.07, 0.2)
COOLING_SETS = dict(sherwood_reion=dict(n=1000, zmid=15.0, seed=3), sherwood_z3=dict(n=1000, zmid=3.0, seed=4))
SFR_SET = dict(name="heating", mode=3, n=1200, zmid=3.0, seed=4)
POS_SEED = 77


def positions(n):
    """uniform in [-0.25, 1.25)^3: a quarter box beyond both faces"""
    return np.random.RandomState(POS_SEED).uniform(-0.25, 1.25, (n, 3))


def cooling_set(name, treecool_columns):
    """(Cooling, times, step, table of n rows, positions, UVF) of a cooling set"""
    s = COOLING_SETS[name]
    C, times, step, make = R.config(name, treecool_columns)
    return C, times, step, make(s["n"]), positions(s["n"]), UVF(synthetic_zreion_table(NSIDE, s["zmid"], s["seed"]), BOXSIZE)


def sfr_set(treecool_columns):
    """(Sfr, times, step, table, positions, UVF) of the star-formation set: the `heating` setting, whose global background forces
    tcool = 0, with BHFeedbackUseTcool = 3, under which cooling_relaxed calls GetCoolingTime a second time for every hot row"""
    s = SFR_SET
    S, times, step, make = SF.config(s["name"], treecool_columns, s["mode"])
    return S, times, step, make(s["n"]), positions(s["n"]), UVF(synthetic_zreion_table(NSIDE, s["zmid"], s["seed"]), BOXSIZE)
