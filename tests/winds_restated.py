"""numpy restatement of the wind model (libgadget/winds.c), written from the cited lines, over ALL pairs (no tree): get_wind_params :493-511,
sfr_wind_weight_ngbiter :414-450, sfr_wind_feedback_ngbiter :513-569, cmp_by_part_id :207-224 with the loop of :338-356, wind_do_kick and
get_wind_dir :453-490, winds_make_after_sf :571-589 with winds_subgrid :275-295, winds_evolve :374-391.

Two forms of the nearest-star rule:
  (a) literal   the kick list filled star by star in list order, sorted with cmp_by_part_id, the first entry of every particle applied.
  (b) defined   per gas particle the minimum over (r, StarID) of its potential kicks (include/mpgadget_hip.h).
IDs are unsigned 64-bit: sums wrap (Python integers masked to 64 bits).  The random table is data: get_random_number(id) = table[id % size].
Not a test module: imported by test_winds_restated.py (runs anywhere) and test_gpu_winds.py (the HIP path)."""
import functools
import math

import numpy as np

from metals_restated import desnumngb
from veldisp_restated import nearest

WIND_SUBGRID, WIND_DECOUPLE_SPH, WIND_USE_HALO, WIND_FIXED_EFFICIENCY, WIND_ISOTROPIC = 1, 2, 4, 8, 512   # winds.h:13-20
GAMMA_MINUS1 = 5.0 / 3.0 - 1                                                                          # physconst.h:35-36
M64 = (1 << 64) - 1
EPS = float(np.finfo(np.float64).eps)


class WindError(RuntimeError):
    """endrun: an undefined model (:506), a listed row that is no star (:406-407), an odd kick (:350-355)"""


def rnd(table, ident):
    """get_random_number, system.c:55-61, of an id that has already wrapped"""
    return float(table[(int(ident) & M64) % len(table)])


def get_wind_params(par, vdisp, time):
    """:493-511 -> (vel, windeff, utherm)"""
    vphys = vdisp / time
    utherm = par["WindThermalFactor"] * 1.5 * vphys * vphys
    if par["WindModel"] & WIND_FIXED_EFFICIENCY:
        windeff = par["WindEfficiency"]
        vel = par["WindSpeed"] * time
    elif par["WindModel"] & WIND_USE_HALO:
        with np.errstate(divide="ignore"):
            windeff = float(np.float64(par["WindSigma0"]) ** 2 / np.float64(vphys * vphys + 2 * utherm))
        vel = par["WindSpeedFactor"] * vdisp
    else:
        raise WindError("WindModel = 0x%X is strange. This shall not happen." % par["WindModel"])
    if vel < par["MinWindVelocity"] * time:
        vel = par["MinWindVelocity"] * time
    return vel, windeff, utherm


def wind_dir(table, ident):
    """get_wind_dir, :477-490"""
    theta = math.acos(2 * rnd(table, int(ident) + 3) - 1)
    phi = 2 * math.pi * rnd(table, int(ident) + 4)
    return np.array([math.sin(theta) * math.cos(phi), math.sin(theta) * math.sin(phi), math.cos(theta)])


def wind_do_kick(out, ids, density, other, vel, therm, atime, par, table):
    """:453-475 on row `other` of out["vel"], out["entropy"], out["delaytime"]; returns therm / enttou (0 when nothing was done)"""
    d = wind_dir(table, ids[other])
    if vel > 0 and atime > 0:
        for j in range(3):
            out["vel"][other, j] += vel * d[j]
        enttou = math.pow(density[other] / math.pow(atime, 3), GAMMA_MINUS1) / GAMMA_MINUS1
        out["entropy"][other] += therm / enttou
        if par["MaxWindFreeTravelTime"] > 0:
            delay = par["WindFreeTravelLength"] / (vel / atime)
            if delay > par["MaxWindFreeTravelTime"]:
                delay = par["MaxWindFreeTravelTime"]
            out["delaytime"][other] = delay
        return therm / enttou
    return 0.0


def cmp_by_part_id(a, b):
    """:207-224 on tuples (part_index, StarDistance, StarID, ...)"""
    for k in range(3):
        if a[k] > b[k]:
            return 1
        if a[k] < b[k]:
            return -1
    return 0


def walks(d, newstars, par, table, atime):
    """both walks over all pairs.  d: pos, type (CURRENT), mass float32, id uint64, hsml, vdisp, delaytime, box.  Returns per list row the
    TotalWeight with its number of terms, the eligible-neighbour count, and the potential kicks in the order the reference fills its list
    when it takes the stars in list order (each star's neighbours by row): tuples (gas row, r, StarID, v, utherm, star row); and the margins
    hsml_gap (smallest |r - Hsml| / Hsml over all candidates) and p_margin (smallest |table value - p| over the pairs tested)."""
    pos = np.asarray(d["pos"], np.float64)
    gas = np.nonzero(d["type"] == 0)[0]
    gpos = pos[gas]
    M = d["mass"][gas].astype(np.float64)
    free = ~(d["delaytime"][gas] > 0)
    tw, nterm, kicks = [], [], []
    tested = 0
    hsml_gap, p_margin = float("inf"), float("inf")
    for i in newstars:
        i = int(i)
        if d["type"][i] != 4:
            raise WindError("Particle %d has type %d not a star" % (i, d["type"][i]))
        h = float(d["hsml"][i])
        dist = nearest(pos[i] - gpos, d["box"])
        r2 = dist[:, 0] * dist[:, 0] + dist[:, 1] * dist[:, 1] + dist[:, 2] * dist[:, 2]
        r = np.sqrt(r2)
        if len(r):
            hsml_gap = min(hsml_gap, float(np.abs(r - h).min() / abs(h)))
        inside = ~(r2 > h * h) & ~(r > h) & free
        sel = np.nonzero(inside)[0]
        w = math.fsum(M[sel])
        tw.append(w)
        nterm.append(len(sel))
        vd = float(d["vdisp"][i])
        if w == 0 or vd <= 0:
            continue
        v, windeff, utherm = get_wind_params(par, vd, atime)
        p = windeff * float(d["mass"][i]) / w
        sid = int(d["id"][i])
        for j in sel:
            t = rnd(table, sid + int(d["id"][gas[j]]))
            tested += 1
            p_margin = min(p_margin, abs(t - p))
            if t < p and v > 0:
                kicks.append((int(gas[j]), float(r[j]), sid, v, utherm, i))
    return dict(totalweight=np.array(tw), nterm=np.array(nterm, np.int64), kicks=kicks, tested=tested, hsml_gap=hsml_gap, p_margin=p_margin)


def resolve_defined(kicks):
    """form (b): {gas row: winning entry}, the minimum over (r, StarID)"""
    best = {}
    for k in kicks:
        b = best.get(k[0])
        if b is None or (k[1], k[2]) < (b[1], b[2]):
            best[k[0]] = k
    return best


def resolve_literal(kicks):
    """form (a): sort with cmp_by_part_id, the first entry per particle (:338-348); returns ({gas row: entry}, maxvel = the kick velocity
    of the first sorted entry, what the reference prints; 0 for an empty list (:323))"""
    s = sorted(kicks, key=functools.cmp_to_key(cmp_by_part_id))
    best, last = {}, -1
    for k in s:
        if k[0] == last:
            continue
        last = k[0]
        best[k[0]] = k
    return best, (s[0][3] if s else 0.0)


def r_gap(kicks):
    """the smallest relative difference of r between two potential kicks of one gas particle that are not exactly equal"""
    by = {}
    for k in kicks:
        by.setdefault(k[0], []).append(k[1])
    gap = float("inf")
    for rs in by.values():
        rs = np.unique(np.array(rs))
        if len(rs) > 1:
            gap = min(gap, float((np.diff(rs) / rs[1:]).min()))
    return gap


def winds_and_feedback(d, newstars, par, table, atime, literal=False):
    """the whole call; returns out (vel, entropy, delaytime, kick_star uint64: ID + 1) and info"""
    out = dict(vel=d["vel"].copy(), entropy=d["entropy"].copy(), delaytime=d["delaytime"].copy(), kick_star=np.zeros(len(d["type"]), np.uint64))
    if par["WindModel"] & WIND_SUBGRID or len(newstars) == 0:                    # :302-306
        return out, None
    W = walks(d, newstars, par, table, atime)
    if literal:
        best, maxvel = resolve_literal(W["kicks"])
    else:
        best = resolve_defined(W["kicks"])
        maxvel = best[min(best)][3] if best else 0.0
    dent = {}
    for g in sorted(best):
        k = best[g]
        dent[g] = wind_do_kick(out, d["id"], d["density"], g, k[3], k[4], atime, par, table)
        out["kick_star"][g] = np.uint64((k[2] + 1) & M64)
        if k[3] <= 0 or not math.isfinite(k[3]) or not math.isfinite(out["delaytime"][g]):
            raise WindError("Odd v: other = %d" % g)
    info = dict(W, best=best, dent=dent, maxvel=maxvel, applied=len(best), pairs=set((k[5], k[0]) for k in W["kicks"]), r_gap=r_gap(W["kicks"]))
    return out, info


def winds_subgrid(d, rows, stellarmass, par, table, atime):
    """:275-295 with winds_make_after_sf :571-589; stellarmass by particle.  Returns out, the kicked rows {row: (v, therm / enttou)} and
    the smallest |table value - prob|"""
    out = dict(vel=d["vel"].copy(), entropy=d["entropy"].copy(), delaytime=d["delaytime"].copy())
    kicked, margin = {}, float("inf")
    if not par["WindModel"] & WIND_SUBGRID:
        return out, kicked, margin
    for i in rows:
        i = int(i)
        vel, windeff, utherm = get_wind_params(par, float(d["vdisp"][i]), atime)
        pw = windeff * float(stellarmass[i]) / float(d["mass"][i])
        prob = 1 - math.exp(-pw)
        t = rnd(table, int(d["id"][i]) + 2)
        margin = min(margin, abs(t - prob))
        if t < prob:
            kicked[i] = (vel, wind_do_kick(out, d["id"], d["density"], i, vel, utherm, atime, par, table))
    return out, kicked, margin


def winds_evolve(delaytime, density, ptype, tb_hydro, dloga_bin, hubble, atime, par, rows):
    """:374-391 for the listed rows of type 0, a3inv = 1 / atime^3 (sfr_eff.c:211); returns the new DelayTime and the branch every row took:
    0 untouched, 1 reset by the density, 2 clamped to the maximum, 3 reduced only"""
    dt = delaytime.copy()
    branch = np.zeros(len(dt), np.int8)
    a3inv = 1 / (atime * atime * atime)
    for i in rows:
        i = int(i)
        if ptype[i] != 0:
            continue
        if dt[i] > 0 and density[i] * a3inv < par["WindFreeTravelDensThresh"]:
            dt[i] = 0
            branch[i] = 1
        if dt[i] > 0:
            branch[i] = 3
            if dt[i] > par["MaxWindFreeTravelTime"]:
                dt[i] = par["MaxWindFreeTravelTime"]
                branch[i] = 2
            dtime = dloga_bin[tb_hydro[i]] / hubble
            dt[i] = max(dt[i] - dtime, 0)
    return dt, branch


# ---- inputs shared by the two test modules ---------------------------------------------------------------------------------------------
ATIME = 0.25
TABLE_SIZE = 10007


def model(kind, decouple_time, ngb=None):
    """struct WindParams after init_winds for the four models the tests run: kind "halo" (ofjt10) or "fixed" (vs08), with
    MaxWindFreeTravelTime > 0 or 0.  WindSigma0 / WindEfficiency give p of about 0.3 for a star of typical Vdisp with `ngb` free gas
    particles of its own mass inside Hsml."""
    ngb = desnumngb(2, 1.0) if ngb is None else ngb
    wtf = 0.5
    vphys = 15.0 / ATIME
    par = dict(WindModel=(WIND_USE_HALO if kind == "halo" else WIND_FIXED_EFFICIENCY) | WIND_DECOUPLE_SPH | WIND_ISOTROPIC,
               WindEfficiency=0.3 * ngb, WindSigma0=vphys * math.sqrt(0.3 * ngb * (1 + 3 * wtf)), WindSpeedFactor=3.7, MinWindVelocity=5.0,
               WindThermalFactor=wtf, WindFreeTravelLength=20.0, WindSpeed=250.0, MaxWindFreeTravelTime=0.1 if decouple_time else 0.0,
               WindFreeTravelDensThresh=0.0)
    return par


def wind_scene(pos_gas, box, nstar, seed, nbh=4, ndm=50, nconv=5, nswal=4):
    """A particle table: gas (type 0), `nbh` black holes (type 5) at gas-like places, `ndm` dark matter rows, then `nstar` stars (type 4) drawn
    near gas positions - one of them in a corner of the box -, with garbage / swallowed rows (type 7) among gas and stars, and `nconv` gas
    rows that became stars and `nswal` that were swallowed after the tree was built (type_tree 0, type 4 / 7).  The new-star list is every live star and the converted rows,
    shuffled.  Star Hsml is the radius of desnumngb gas particles at mean density times 0.05 (a fifth), 20 (a tenth) or 1; a tenth of the
    stars have Vdisp <= 0, a tenth a Vdisp below the MinWindVelocity floor; a tenth of the gas has DelayTime > 0; a tenth of all IDs lie
    above 2^63.  One gas particle sits at dyadic coordinates with two stars mirrored about it (r2 exactly equal), and the random table
    makes both pairs potential kicks; of those two stars the LATER in the list has the smaller ID."""
    rng = np.random.RandomState(seed)
    ng = len(pos_gas)
    at = rng.choice(ng, nstar + nbh, replace=False)
    spread = 0.3 * box / ng ** (1. / 3)
    pos_bh = pos_gas[at[:nbh]] + spread * rng.standard_normal((nbh, 3))
    pos_st = pos_gas[at[nbh:]] + spread * rng.standard_normal((nstar, 3))
    pos_st[0] = box * np.array([3e-4, 0.9998, 2e-4])                       # a search that crosses a corner
    pos_gas = np.array(pos_gas, np.float64)
    u = 2.0 ** math.floor(math.log2(box / 16))
    tie_gas = int(rng.randint(ng))
    pos_gas[tie_gas] = u * np.array([4.0, 6.0, 5.0])
    delta = u * np.array([1 / 16, -1 / 32, 1 / 64])
    pos_st[1] = pos_gas[tie_gas] + delta
    pos_st[2] = pos_gas[tie_gas] - delta
    pos = np.mod(np.concatenate([pos_gas, pos_bh, box * rng.random_sample((ndm, 3)), pos_st]), box)
    pos[pos <= 0] += box
    pos = np.ascontiguousarray(pos)
    n = len(pos)
    s0 = ng + nbh + ndm
    type_tree = np.concatenate([np.zeros(ng, np.uint8), np.full(nbh, 5, np.uint8), np.ones(ndm, np.uint8), np.full(nstar, 4, np.uint8)])
    mass = (1.0 + 0.2 * rng.random_sample(n)).astype(np.float32)
    density = ng * float(mass[:ng].mean()) / box ** 3 * np.exp(0.3 * rng.standard_normal(n))
    h0 = (3 * desnumngb(2, 1.0) / (4 * np.pi * ng)) ** (1. / 3) * box
    hsml = h0 * np.exp(0.2 * rng.standard_normal(n))
    kind = rng.random_sample(n)
    kind[[s0 + 1, s0 + 2]] = 0.5
    hsml[s0:][kind[s0:] < 0.2] *= 0.05
    hsml[s0:][kind[s0:] > 0.9] *= 20.0
    vdisp = 10.0 * (1 + rng.random_sample(n))
    vk = rng.random_sample(n)
    vk[[s0 + 1, s0 + 2]] = 0.5
    vdisp[vk < 0.05] = 0.0
    vdisp[(vk >= 0.05) & (vk < 0.1)] = -3.0
    vdisp[(vk >= 0.1) & (vk < 0.2)] = 1e-3
    delaytime = np.where(rng.random_sample(n) < 0.1, 0.05 * rng.random_sample(n), 0.0)
    delaytime[tie_gas] = 0.0
    ids = rng.randint(1, 1 << 48, n).astype(np.uint64)
    ids[rng.random_sample(n) < 0.1] += np.uint64(1 << 63)
    ids[s0 + 1], ids[s0 + 2] = np.uint64((1 << 63) + 77), np.uint64((1 << 63) + 5)   # both above 2^63: their sums with a large gas ID wrap
    assert len(np.unique(ids)) == n
    ptype = type_tree.copy()
    live_gas = np.setdiff1d(np.arange(ng), [tie_gas])
    dead = np.concatenate([rng.choice(live_gas, 12, replace=False), s0 + 3 + rng.choice(nstar - 3, 6, replace=False)])
    ptype[dead] = 7
    type_tree_alive = type_tree.copy()
    type_tree_alive[dead] = 7                                               # garbage before the build: such rows are not in the tree
    conv = rng.choice(np.setdiff1d(live_gas, dead), nconv, replace=False)
    ptype[conv] = 4                                                         # formed a star since the tree was built
    swal = rng.choice(np.setdiff1d(live_gas, np.concatenate([dead, conv])), nswal, replace=False)
    ptype[swal] = 7                                                         # swallowed by a black hole since the tree was built
    stars = np.concatenate([s0 + np.nonzero(ptype[s0:] == 4)[0], conv])
    newstars = stars[rng.permutation(len(stars))].astype(np.int32)
    a, b = int(np.nonzero(newstars == s0 + 1)[0][0]), int(np.nonzero(newstars == s0 + 2)[0][0])
    if b < a:                                                               # the smaller ID (s0 + 2) later in the list
        newstars[a], newstars[b] = newstars[b], newstars[a]
    table = rng.random_sample(TABLE_SIZE)
    for s in (s0 + 1, s0 + 2):
        table[((int(ids[s]) + int(ids[tie_gas])) & M64) % TABLE_SIZE] = 0.0
    return dict(pos=pos, type=ptype, type_tree=type_tree_alive, box=float(box), n=n, ng=ng, nstar=nstar, s0=s0, mass=mass, density=density, hsml=hsml,
                vdisp=vdisp, delaytime=delaytime, id=ids, vel=np.ascontiguousarray(100.0 * rng.standard_normal((n, 3))),
                entropy=1.0 + rng.random_sample(n), newstars=newstars, table=table, tie_gas=tie_gas, tie_stars=(s0 + 1, s0 + 2), conv=conv, dead=dead, swal=swal)


SCENES = dict(zel=(150, 5), clust=(100, 8))     # stars, seed
MODELS = (("halo", True), ("halo", False), ("fixed", True), ("fixed", False))
_cache = {}


def scene(ics, name):
    """the two scenes of the metals tests: 16^3 gas of ics.hydro_pair(16), the clustered 4096-gas set ics.s_clust(16)"""
    if name not in _cache:
        nstar, seed = SCENES[name]
        if name == "zel":
            pos, _, typ, box = ics.hydro_pair(16)
            pg = pos[typ == 0]
        else:
            pg, _, box = ics.s_clust(16, seed=3)
        _cache[name] = wind_scene(pg, box, nstar, seed)
    return _cache[name]


def restated(ics, name, kind, decouple_time):
    """(scene, parameters, out, info) of form (b), computed once"""
    key = (name, kind, decouple_time)
    if key not in _cache:
        d = scene(ics, name)
        par = model(kind, decouple_time)
        out, info = winds_and_feedback(d, d["newstars"], par, d["table"], ATIME)
        _cache[key] = (d, par, out, info)
    return _cache[key]


def conditions(d, info):
    """what the committed seeds must satisfy for the GPU comparison to be one of equal integers (asserted, no target left out)"""
    assert info["hsml_gap"] > 1e-10, info["hsml_gap"]
    assert info["p_margin"] > 1e-9, info["p_margin"]
    assert info["r_gap"] > 1e-10, info["r_gap"]
    assert info["applied"] >= 100, info["applied"]
    order = {int(s): q for q, s in enumerate(d["newstars"])}
    by = {}
    for k in info["kicks"]:
        by.setdefault(k[0], set()).add(k[5])
    multi = [g for g, s in by.items() if len(s) >= 2]
    notfirst = [g for g in multi if order[info["best"][g][5]] != min(order[s] for s in by[g])]
    assert len(multi) >= 20 and len(notfirst) >= 5, (len(multi), len(notfirst))
    # the exact tie: both mirrored stars are potential kicks of the dyadic particle at the same r, no other star is nearer, the smaller ID wins
    t = [k for k in info["kicks"] if k[0] == d["tie_gas"] and k[5] in d["tie_stars"]]
    assert len(t) == 2 and t[0][1] == t[1][1] and t[0][2] != t[1][2]
    w = info["best"][d["tie_gas"]]
    assert w[1] == t[0][1] and w[2] == min(t[0][2], t[1][2]) and order[w[5]] > min(order[s] for s in d["tie_stars"])
    return dict(multi=len(multi), notfirst=len(notfirst))
