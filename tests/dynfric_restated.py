"""Black-hole dynamical friction and the potential minimum of repositioning - the walk, its post-process and DFAccel - restated in numpy and
plain Python over ALL PAIRS, with no tree, from the description of the model (bhdynfric.c of the reference is cited for orientation only):

  the tree of a call holds the particles of its type mask (stars and black holes; the dark matter when the method is above 1; the gas when
  it is 3; every type when repositioning is on; garbage and swallowed rows carry type 7 and are in no tree); a target visits every particle
  of the tree with r^2 < Hsml^2 on the nearest periodic image (its own Hsml: the asymmetric search), itself included.
  The potential minimum starts from the target's own Potential and position; a neighbour wins only when strictly lower; among neighbours
  of EQUAL lowest potential the smaller particle index wins (the engine's documented rule; the reference: the first visited).
  The friction sums run over the stars, the dark matter (method > 1) and the gas (method 3): sum m wk, sum m wk v[k], sum m wk v[k]^2.

Two forms, selected by `literal`: (b) every sum is the exactly rounded sum of its terms (math.fsum); (a) literal and sequential, in
particle order.  With every result come the number of terms and the sum of absolute terms of every sum, the two terms of f_of_x separately,
the smallest relative distance of any candidate from a target's Hsml and the gap between the lowest and the second-lowest potential inside
each target's radius.  The module also holds numpy restatements of the three integrator kernels that consume the results (the sub-grid kick
of the black holes, the dynamic-friction time bin, the jump to the potential minimum) and builds the scenes of the two test modules."""
import math

import numpy as np

from blackhole_restated import Sum, default_times, nearest, rel, velpred
from metals_restated import kernel_wk

EPS = float(np.finfo(np.float64).eps)
SENTINEL = 3          # what the tests fill the outputs with before a call (exact in every element type)
A_ERF = 8 * (math.pi - 3) / (3 * math.pi * (4. - math.pi))
IN_OUT = ("df_density", "df_vel", "df_rmsvel", "jumptominpot")
OUT = dict(minpot=1, minpotpos=3, minpotvel=3, dfaccel=3)
READ = ("vel", "gacc", "gpm", "hydroacc", "tb_grav", "tb_hydro", "hsml", "potential", "bh_mass", "active_dynfric")
SUMS = ("dens", "v0", "v1", "v2", "rms")


def default_params(**over):
    p = dict(BH_DynFrictionMethod=2, BH_DFBoostFactor=2, BH_DFbmax=10.0, BlackHoleRepositionEnabled=0, GravInternal=1.0)
    p.update(over)
    return p


def treemask(par):
    mask = 16 + 32
    if par["BH_DynFrictionMethod"] > 1:
        mask += 2
    if par["BH_DynFrictionMethod"] > 2:
        mask += 1
    if par["BlackHoleRepositionEnabled"]:
        mask = 63
    return mask


def f_of_x_terms(x):
    """the two terms of f_of_x = x / |x| sqrt(1 - exp(-x^2 (4 / pi + a x^2) / (1 + a x^2))) - 2 x / sqrt(pi) exp(-x^2)"""
    t1 = x / abs(x) * math.sqrt(1 - math.exp(-x * x * (4 / math.pi + A_ERF * x * x) / (1 + A_ERF * x * x)))
    t2 = 2 * x / math.sqrt(math.pi) * math.exp(-x * x)
    return t1, t2


def f_of_x_slope(x):
    """|d f_of_x / dx|, for the first-order propagation of an error of x"""
    g = x * x * (4 / math.pi + A_ERF * x * x) / (1 + A_ERF * x * x)
    dg = ((8 / math.pi * x + 4 * A_ERF * x ** 3) * (1 + A_ERF * x * x) - x * x * (4 / math.pi + A_ERF * x * x) * 2 * A_ERF * x) / (1 + A_ERF * x * x) ** 2
    t1 = math.sqrt(1 - math.exp(-g))
    d1 = math.exp(-g) * dg / (2 * t1) if t1 > 0 else 0.0
    d2 = 2 / math.sqrt(math.pi) * math.exp(-x * x) * (1 - 2 * x * x)
    return abs(d1 - d2)


def compute_dfaccel(vel, mass, density, dfvel, rms, par, atime):
    """DFAccel of one black hole from its stored sums; returns (accel[3], detail) - detail None when the density is not positive, else
    bhvel, x, the two terms of f_of_x, f_of_x (floored at zero), log lambda, lambda"""
    acc = np.zeros(3)
    if not density > 0:
        return acc, None
    G = par["GravInternal"]
    dv = np.asarray(vel, np.float64) - np.asarray(dfvel, np.float64)
    bhvel = 0.0
    for j in range(3):
        bhvel += float(dv[j]) * float(dv[j])
    bhvel = math.sqrt(bhvel)
    if not math.isfinite(bhvel):
        raise FloatingPointError("bhvel is not finite")
    det = dict(bhvel=bhvel, x=0.0, t1=0.0, t2=0.0, f=0.0, loglambda=0.0, lam=1.0)
    if not bhvel > 0:
        return acc, det
    x = bhvel / math.sqrt(2) / (rms / 3) if rms > 0 else math.inf
    if math.isfinite(x):
        t1, t2 = f_of_x_terms(x)
    else:
        t1, t2 = 1.0, 0.0
    f = max(t1 - t2, 0.0)
    lam = 1. + par["BH_DFbmax"] * (bhvel / atime) ** 2 / G / mass
    L = math.log(lam)
    for j in range(3):
        a = -4. * math.pi * G * G * mass * density * L * f * float(dv[j]) / bhvel ** 3
        a *= atime
        a *= par["BH_DFBoostFactor"]
        acc[j] = a
    det.update(x=x, t1=t1, t2=t2, f=f, loglambda=L, lam=lam)
    return acc, det


def dynfric(d, par, T, active=None, literal=False):
    """the whole call on the scene `d`.  Returns (out, info): out holds the in / out columns and every output in particle order (inputs /
    SENTINEL where the call writes nothing); info the listed black holes and the targets, per target the raw sums with their (k, sum |term|),
    the index of the potential minimum (-1: none lower), the neighbour count, the margins, and per listed black hole the detail of DFAccel."""
    n, box, ktype, typ = d["n"], d["box"], d["ktype"], d["type"]
    method, repos = par["BH_DynFrictionMethod"], par["BlackHoleRepositionEnabled"]
    out = {k: d[k].copy() for k in IN_OUT}
    for k, w in OUT.items():
        out[k] = np.full((n, w) if w > 1 else n, float(SENTINEL))
    idx = np.arange(n) if active is None else np.asarray(active, np.int64)
    listed = [int(i) for i in idx if typ[i] == 5]
    info = dict(listed=listed, targets=[], per={}, dfaccel={}, margins=dict(hsml=np.inf, potgap=np.inf), zerodf=0, zerodfmass=0.0, neighbours=0,
                tree=0)
    if method == 0 and not repos:
        info["listed"] = []
        return out, info
    if method > 0:
        ad = d.get("active_dynfric")
        targets = [i for i in listed if ad is None or ad[i]]
    else:
        targets = list(listed)
    info["targets"] = targets
    mask = treemask(par)
    intree = np.nonzero((typ < 6) & (((1 << typ.astype(np.int64)) & mask) != 0))[0]
    info["tree"] = len(intree)
    zmass = []
    for i in targets:
        H = float(d["hsml"][i])
        dx = nearest(d["pos"][i] - d["pos"][intree], box)
        r2 = (dx * dx).sum(1)
        info["margins"]["hsml"] = min(info["margins"]["hsml"], float(np.abs(np.sqrt(r2) / H - 1).min()))
        keep = r2 < H * H
        cj, cr = intree[keep], np.sqrt(r2[keep])
        pots = np.sort(d["potential"][cj])
        gap = float(pots[1] - pots[0]) if len(pots) > 1 else np.inf
        info["margins"]["potgap"] = min(info["margins"]["potgap"], gap)
        # the potential minimum: strictly lower than the target's own; equal lowest: the smaller index (particle order IS index order)
        ipot, bpot, bidx = float(d["potential"][i]), 0.0, -1
        for j in cj.tolist():
            p = float(d["potential"][j])
            if p < ipot and (bidx < 0 or p < bpot):
                bpot, bidx = p, j
        if bidx >= 0:
            out["minpot"][i], out["minpotpos"][i], out["minpotvel"][i], out["jumptominpot"][i] = bpot, d["pos"][bidx], d["vel"][bidx], repos
        else:
            out["minpot"][i], out["minpotpos"][i] = ipot, d["pos"][i]
        P = dict(minidx=bidx, numngb=len(cj), potgap=gap)
        info["neighbours"] += len(cj)
        if method > 0:
            S = {k: Sum(literal) for k in SUMS}
            for j, r in zip(cj.tolist(), cr.tolist()):
                ty = int(typ[j])
                if not (ty == 4 or (ty == 1 and method > 1) or (ty == 0 and method == 3)):
                    continue
                wk = float(kernel_wk(r / H, H, ktype))
                mw = float(d["mass"][j]) * wk
                v = velpred(d, T, j, ty == 0)
                S["dens"].add(mw)
                for k in range(3):
                    S["v%d" % k].add(mw * float(v[k]))
                    S["rms"].add(mw * (float(v[k]) * float(v[k])))
            raw = np.array([S[k].value for k in SUMS])
            P["raw"], P["sums"] = raw, {k: (S[k].k, S[k].abs) for k in SUMS}
            dens = raw[0]
            if dens > 0:
                out["df_rmsvel"][i] = math.sqrt(raw[4] / dens)
                out["df_vel"][i] = raw[1:4] / dens
            else:
                info["zerodf"] += 1
                zmass.append(float(d["bh_mass"][i]))
                out["df_rmsvel"][i], out["df_vel"][i] = raw[4], raw[1:4]
            out["df_density"][i] = dens
        info["per"][i] = P
    info["zerodfmass"] = math.fsum(zmass)
    if method > 0:
        for i in listed:
            acc, det = compute_dfaccel(d["vel"][i], float(d["mass"][i]), float(out["df_density"][i]), out["df_vel"][i], float(out["df_rmsvel"][i]), par,
                                       T["atime"])
            out["dfaccel"][i] = acc
            info["dfaccel"][i] = det
    return out, info


# ---- the three integrator kernels ----------------------------------------------------------------------------------------------------------
def listed_rows(n, active, flags):
    idx = np.arange(n) if active is None else np.asarray(active, np.int64)
    if flags is not None:
        idx = idx[(flags[idx] & 3) == 0]
    return idx


def bh_subgrid_kick(vel, ptype, flags, tb_hydro, dfaccel, dragaccel, gravkick, active=None):
    """Vel += DFAccel * gravkick[TimeBinHydro], then Vel += DragAccel * gravkick[TimeBinHydro] for the listed live type-5 rows: two additions"""
    v = vel.copy()
    idx = listed_rows(len(vel), active, flags)
    idx = idx[ptype[idx] == 5]
    F = np.asarray(gravkick, np.float64)[tb_hydro[idx]][:, None]
    v[idx] = v[idx] + dfaccel[idx] * F
    v[idx] = v[idx] + dragaccel[idx] * F
    return v


def dynfric_dloga(vel, dfvel, hsml, dthsml, atime, hubble, errtol, courant):
    bhvel, bhvel2 = 0.0, 0.0
    for j in range(3):
        dlt = float(vel[j]) - float(dfvel[j])
        bhvel += dlt * dlt
        bhvel2 += float(vel[j]) * float(vel[j])
    if bhvel2 > bhvel:
        bhvel = bhvel2
    bhvel = math.sqrt(bhvel)
    dt = 2 * errtol * atime * atime * hsml / (bhvel + 1e-20)
    dt_hsml = courant * atime * atime * abs(hsml / (dthsml + 1e-20))
    if dt_hsml < dt:
        dt = dt_hsml
    return dt * hubble


def find_dynfric_timesteps(S, active, times, tl, errtol, minsize, courant, atime, hubble):
    """S: dict with type, flags, vel, df_vel, hsml, dthsml, tb_grav, tb_hydro, tb_dynfric (updated in place).  Returns dict(dynratio,
    maxdyndiff, nbh) and the smallest relative distance of any step from a bin boundary (a power of two of the integer timeline)."""
    from oracle import hiergrav_oracle as H
    idx = listed_rows(len(S["type"]), active, S.get("flags"))
    idx = idx[S["type"][idx] == 5]
    res, margin = dict(dynratio=0, maxdyndiff=0, nbh=0), np.inf
    for i in idx.tolist():
        dloga = dynfric_dloga(S["vel"][i], S["df_vel"][i], float(S["hsml"][i]), float(S["dthsml"][i]), atime, hubble, errtol, courant)
        dti = int(H.convert_timestep_to_ti(np.array([dloga]), times["PM_length"], times["Ti_Current"], tl, minsize)[0])
        if dti > 1:
            b = dti.bit_length() - 1
            margin = min(margin, abs(dti - (1 << b)) / dti if dti != (1 << b) else 0.0, abs((1 << (b + 1)) - dti) / dti)
        b = H.get_timebin_from_dti(dti, int(S["tb_dynfric"][i]), times["Ti_Current"])
        b = min(b, int(S["tb_grav"][i]))
        b = max(b, int(S["tb_hydro"][i]))
        S["tb_dynfric"][i] = b
        diff = b - int(S["tb_hydro"][i])
        res["dynratio"] += diff
        res["maxdyndiff"] = max(res["maxdyndiff"], diff)
        res["nbh"] += 1
    return res, margin


def reposition(pos, vel, ptype, flags, jump, minpotpos, minpotvel, box):
    """a live flagged black hole takes MinPotPos / MinPotVel; the flag of every live black hole is cleared.  Returns (pos, vel, jump, far):
    far lists the black holes whose signed NEAREST(Pos - MinPotPos) exceeds 0.1 box along an axis (they are not moved, the call is an error)"""
    p, v, jmp, far = pos.copy(), vel.copy(), jump.copy(), []
    for i in np.nonzero((ptype == 5) & ((flags & 3) == 0))[0].tolist():
        if jmp[i]:
            dx = p[i] - minpotpos[i]
            dx = np.where(dx > 0.5 * box, dx - box, np.where(dx < -0.5 * box, dx + box, dx))
            if (dx > 0.1 * box).any():
                far.append(i)
                continue
            p[i], v[i] = minpotpos[i], minpotvel[i]
        jmp[i] = 0
    return p, v, jmp, far


# ---- scenes ----------------------------------------------------------------------------------------------------------------------------------
def make_scene(pos, ptype, seed, hsml, ktype=1, box=1.0):
    """a particle table with everything the call reads, from positions and types: distinct random potentials, random velocities,
    accelerations and bins, float masses, stale non-zero friction sums and flags of the black holes"""
    rng = np.random.RandomState(seed)
    n = len(pos)
    d = dict(pos=np.ascontiguousarray(pos), type=ptype.astype(np.uint8), type_table=ptype.astype(np.uint8).copy(), box=float(box), n=n, ktype=ktype)
    d["mass"] = (1.0 + 0.2 * rng.random_sample(n)).astype(np.float32)
    d["vel"] = 0.3 * rng.standard_normal((n, 3))
    d["gacc"], d["gpm"], d["hydroacc"] = (rng.standard_normal((n, 3)) for _ in range(3))
    d["tb_grav"] = rng.randint(17, 23, n).astype(np.uint8)
    d["tb_hydro"] = rng.randint(17, 23, n).astype(np.uint8)
    d["hsml"] = np.asarray(hsml, np.float64).copy()
    d["potential"] = -(1.0 + rng.permutation(n)) / n                    # distinct
    bh = ptype == 5
    d["bh_mass"] = np.where(bh, np.exp(rng.standard_normal(n)), 0.0)
    d["active_dynfric"] = np.ones(n, np.uint8)
    d["df_density"] = np.where(bh, 0.5 + rng.random_sample(n), 0.0)       # stale, non-zero
    d["df_vel"] = np.where(bh[:, None], 0.2 * rng.standard_normal((n, 3)), 0.0)
    d["df_rmsvel"] = np.where(bh, 0.4 + 0.2 * rng.random_sample(n), 0.0)
    d["jumptominpot"] = np.where(bh, rng.randint(0, 2, n), 0).astype(np.int32)
    d["flags"] = np.zeros(n, np.uint8)
    return d


def place_relative_to_surroundings(d, par, T, i, nsigma, seed):
    """the velocity of black hole i at `nsigma` dispersions from the mean velocity of its surroundings (neither enters any sum)"""
    out, _ = dynfric(d, par, T, active=[i])
    if not out["df_density"][i] > 0:
        return
    u = np.random.RandomState(seed).standard_normal(3)
    d["vel"][i] = out["df_vel"][i] + nsigma * out["df_rmsvel"][i] * u / np.linalg.norm(u)


def scene_a(par, ktype=1, seed=21):
    """16^3 jittered gas + 40 black holes + 16^3 jittered dark matter + 512 stars in a unit box.  Black holes (relative to b0): 0 with
    Hsml = 0.45 (thousands of neighbours: more than one leaf list), 1 at a corner of the box, 2 with an Hsml that holds nothing but itself
    (ZeroDF), 3 with active_dynfric = 0 (its stale sums stay), 4 moving with its surroundings to 1e-3 of their dispersion, 5 at five
    dispersions, 38 swallowed, 39 garbage."""
    rng = np.random.RandomState(seed)
    g = (np.stack(np.meshgrid(*[np.arange(16)] * 3, indexing="ij"), -1).reshape(-1, 3) + 0.5) / 16.0
    gas = np.mod(g + 0.02 * rng.standard_normal(g.shape), 1.0)
    dm = np.mod(g + 0.03 + 0.02 * rng.standard_normal(g.shape), 1.0)
    stars = rng.random_sample((512, 3))
    nbh = 40
    bh = 0.1 + 0.8 * rng.random_sample((nbh, 3))
    bh[1] = (0.002, 0.998, 0.003)
    pos = np.concatenate([gas, bh, dm, stars])
    pos[pos <= 0] += 1.0
    ptype = np.concatenate([np.zeros(len(gas)), np.full(nbh, 5), np.ones(len(dm)), np.full(512, 4)]).astype(np.uint8)
    hsml = np.full(len(pos), 0.05)
    b0 = len(gas)
    hsml[b0:b0 + nbh] = rng.uniform(0.10, 0.22, nbh)
    hsml[b0], hsml[b0 + 1], hsml[b0 + 2] = 0.45, 0.08, 1e-4
    d = make_scene(pos, ptype, seed + 1, hsml, ktype)
    d["b0"], d["nbh"] = b0, nbh
    d["active_dynfric"][b0 + 3] = 0
    d["flags"][b0 + 38], d["flags"][b0 + 39] = 2, 1
    d["type"][b0 + 38] = d["type"][b0 + 39] = 7
    if par["BH_DynFrictionMethod"] > 0:
        T = default_times()
        place_relative_to_surroundings(d, par, T, b0 + 4, 1e-3, seed + 2)
        place_relative_to_surroundings(d, par, T, b0 + 5, 5.0, seed + 3)
    return d


def scene_b(pos, par, ktype=1, seed=31):
    """a clustered set (positions in a unit box): 40 black holes drawn among the particles, the rest gas, dark matter and stars at random"""
    rng = np.random.RandomState(seed)
    n = len(pos)
    pos = np.mod(np.asarray(pos, np.float64), 1.0)
    pos[pos <= 0] += 1.0
    ptype = rng.choice([0, 0, 1, 1, 4], n).astype(np.uint8)
    bh = np.sort(rng.choice(n, 40, replace=False))
    ptype[bh] = 5
    hsml = rng.uniform(0.03, 0.10, n)
    d = make_scene(pos, ptype, seed + 1, hsml, ktype)
    d["b0"], d["nbh"], d["bh"] = int(bh[0]), 40, bh
    d["active_dynfric"][bh[::7]] = 0
    return d
