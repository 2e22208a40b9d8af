"""The black-hole step - accretion walk, its post-process, feedback walk, its post-process - restated in numpy and plain Python over ALL
PAIRS, with no tree, from the description of the model (blackhole.c:373-990 of the reference is cited for orientation only):

  a pair (target i, candidate j) interacts when j is gas or a black hole of the table (not garbage, not swallowed) and
  r_ij <= max(Hsml_i, Hsml_j) on the nearest periodic image (the symmetric search); gas contributes to a target's sums only inside
  the target's own Hsml.

Two forms of every walk, selected by `literal`:
  (b) the defined form: every sum is the exactly rounded sum of its terms (math.fsum), a gas particle receives ONE energy sum and ONE
      cap, a mark is the largest ID + 1 over the candidates that may mark.
  (a) the reference's literal sequential form in a fixed order (targets in queue order, candidates in particle order): running sums,
      the compare-and-swap rules of the marks as the reference words them (the stored ID + 1 compared with the newcomer's ID), the cap
      after every addition of energy, velocity kicks added one by one.
Both round P.Mass through a float where the reference does.  The module also builds the random table, the parameter sets and the scenes
of the two test modules, and returns, with the results, everything the tests' bounds and conditions need: the number of terms and the sum
of absolute terms of every sum, and the distance of every decision from its branch point."""
import math

import numpy as np

from metals_restated import KERNELS, desnumngb, kernel_wk

EPS = float(np.finfo(np.float64).eps)
TIMEBINS = 46
GAMMA = 5.0 / 3.0
GAMMA_MINUS1 = GAMMA - 1
# cgs constants of the model
GRAVITY, BOLTZMANN, LIGHTCGS, PROTONMASS, THOMPSON, HYDROGEN_MASSFRAC = 6.672e-8, 1.38066e-16, 2.99792458e10, 1.6726e-24, 6.65245e-25, 0.76
FB_SPLINE, FB_MASS, FB_OPTTHIN = 0x4, 0x8, 0x20

IN_OUT = ("mass", "vel", "entropy", "flags", "bh_mass", "mtrack", "kineticfdbkenergy", "countprogs")
OUT = dict(mdot=(np.float64, 1), dragaccel=(np.float64, 3), encounter=(np.int32, 1), mintimebin=(np.int32, 1), swallowid=(np.uint64, 1),
           swallowtime=(np.float64, 1), bhheated=(np.uint8, 1), feedbackweightsum=(np.float64, 1), bh_entropy=(np.float64, 1),
           gasvel=(np.float64, 3), mgasenc=(np.float64, 1), keflag=(np.int32, 1), accreted_mass=(np.float64, 1), accreted_bhmass=(np.float64, 1),
           accreted_momentum=(np.float64, 3), sph_swallowid=(np.uint64, 1), bh_swallowid=(np.uint64, 1))
SENTINEL = 3          # what the tests fill the outputs with before a call (exact in every element type)


def default_params(**over):
    """mpg_blackhole_params in a unit system in which the quantities of the scenes are of order one"""
    p = dict(BlackHoleAccretionFactor=0.1, BlackHoleFeedbackFactor=0.05, BlackHoleEddingtonFactor=2.0, BlackHoleFeedbackMethod=FB_SPLINE | FB_MASS,
             BlackHoleKineticOn=1, BHKE_EddingtonThrFactor=0.6, BHKE_EddingtonMFactor=0.5, BHKE_EddingtonMPivot=1.0, BHKE_EddingtonMIndex=2.0,
             BHKE_EffRhoFactor=0.05, BHKE_EffCap=0.2, BHKE_InjEnergyThr=0.02, BHKE_SfrCritOverDensity=57.7, MergeGravBound=1, BH_DRAG=1,
             SeedBHDynMass=3.0, BlackHoleRepositionEnabled=0, WindDecouple=1, StarformationOn=1, BHFeedbackUseTcool=0, PhysDensThresh=70.0,
             OverDensThresh=0.5, ForceSoftening=0.0, GravInternal=1.0, HubbleParam=0.7, OmegaBaryon=0.045, Hubble=0.1, UnitTime_in_s=1.0e15,
             UnitVelocity_in_cm_per_s=LIGHTCGS / 100.0, uu_in_cgs=2.0e15)
    p.update(over)
    return p


def default_times(atime=0.5, hubble=2.0):
    """the members of mpg_sph_times the call reads: kick factors per bin, dloga per bin, atime, hubble"""
    b = np.arange(47, dtype=np.float64)
    return dict(FgravkickB=0.013, gravkicks=0.004 * (1 + b % 5), hydrokicks=0.003 * (1 + b % 7), dloga_bin=0.02 * 2.0 ** (b - 20), atime=atime,
                hubble=hubble)


def random_table(seed, size=4099):
    return np.random.RandomState(seed).random_sample(size)


def nearest(dx, box):
    return dx - box * np.rint(dx / box)


def constants(par, T):
    a = T["atime"]
    c = dict(a3inv=1. / (a * a * a))
    c["medd_fac"] = (4 * math.pi * GRAVITY * LIGHTCGS * PROTONMASS / (0.1 * LIGHTCGS * LIGHTCGS * THOMPSON)) * par["UnitTime_in_s"] / par["HubbleParam"]
    c["c2"] = (LIGHTCGS / par["UnitVelocity_in_cm_per_s"]) ** 2
    rho_crit_baryon = par["OmegaBaryon"] * 3 * par["Hubble"] ** 2 / (8 * math.pi * par["GravInternal"])
    c["rho_sfr"] = par["BHKE_SfrCritOverDensity"] * rho_crit_baryon
    u_to_temp = (4 / (8 - 5 * (1 - HYDROGEN_MASSFRAC))) * PROTONMASS / BOLTZMANN * GAMMA_MINUS1 * par["uu_in_cgs"]
    c["ucap"] = 5.0e8 / u_to_temp
    return c


def velpred(d, T, j, hydro):
    v = d["vel"][j] + T["gravkicks"][d["tb_grav"][j]] * d["gacc"][j] + d["gpm"][j] * T["FgravkickB"]
    if hydro:
        v = v + T["hydrokicks"][d["tb_hydro"][j]] * d["hydroacc"][j]
    return v


def rel(x, y):
    """relative distance of x from the branch point y"""
    return abs(x - y) / max(abs(x), abs(y), 1e-300)


class Sum:
    """a sum of terms: exactly rounded (defined form) or running in the order of arrival (literal form), with the bookkeeping of its bound"""

    def __init__(self, literal):
        self.literal, self.terms, self.run = literal, [], 0.0

    def add(self, t):
        t = float(t)
        self.terms.append(t)
        self.run += t

    @property
    def value(self):
        return self.run if self.literal else math.fsum(self.terms)

    @property
    def k(self):
        return len(self.terms)

    @property
    def abs(self):
        return math.fsum(abs(t) for t in self.terms)


def candidates(d, i, live):
    """the pairs of target i under the symmetric search, in particle order: (index, dx[3], r2), and the smallest relative distance of
    any particle from the symmetric radius and from the target's own Hsml"""
    dx = nearest(d["pos"][i] - d["pos"][live], d["box"])
    r2 = (dx * dx).sum(1)
    dist = np.maximum(d["hsml"][live], d["hsml"][i])
    keep = ~(r2 > dist * dist)
    r = np.sqrt(r2)
    return live[keep], dx[keep], r2[keep], min(np.abs(r / dist - 1).min(), np.abs(r / d["hsml"][i] - 1).min())


def blackhole(d, par, T, rnd, active=None, literal=False, merge_dist=None):
    """the whole step on the scene `d`.  Returns (out, info): out holds the in / out columns and every output, in particle order, with
    SENTINEL where the call writes nothing; info the targets, the marks, the counters, per sum its k and its sum of absolute terms, and
    the margins of the conditions."""
    n, box, ktype = d["n"], d["box"], d["ktype"]
    C = constants(par, T)
    md = merge_dist if merge_dist is not None else 2 * par["ForceSoftening"] / 2.8
    atime = T["atime"]
    typ, ids, hs = d["type"], d["id"], d["hsml"]
    out = {k: d[k].copy() for k in IN_OUT}
    for k, (dt, w) in OUT.items():
        out[k] = np.full((n, w) if w > 1 else n, SENTINEL, dt)
    listed = np.arange(n) if active is None else np.asarray(active, np.int64)
    targets = [int(i) for i in listed if typ[i] == 5]
    info = dict(targets=targets, margins=dict(hsml=np.inf, merge=np.inf, bound=np.inf, swallow=np.inf, branch=np.inf, cap=np.inf),
                consecutive=False, sums={}, stats=dict(gas_swallowed=0, bh_swallowed=0, accretion_neighbours=0, feedback_neighbours=0,
                                                        accretion_targets=len(targets), feedback_targets=0))
    if not targets:
        return out, info
    M = info["margins"]
    live = np.nonzero((typ == 0) | (typ == 5))[0]
    swal = {}                       # particle -> ID + 1 of its swallower
    markers = {}                    # black hole -> IDs of all candidates that may mark it
    out["sph_swallowid"][live[typ[live] == 0]] = 0
    out["bh_swallowid"][live[typ[live] == 5]] = 0
    spline, bymass = bool(par["BlackHoleFeedbackMethod"] & FB_SPLINE), bool(par["BlackHoleFeedbackMethod"] & FB_MASS)
    seed = par["SeedBHDynMass"]
    weight = lambda j: float(d["mass"][j]) if bymass else float(hs[j]) ** 3
    decoupled = lambda j: par["WindDecouple"] and typ[j] == 0 and d["delaytime"][j] > 0
    dtime = lambda i: T["dloga_bin"][d["tb_hydro"][i]] / T["hubble"]
    fws, keflag, mdot_of = {}, {}, {}

    # ---- the accretion walk and its post-process --------------------------------------------------------------------------------------
    for i in targets:
        cj, cdx, cr2, gaps = candidates(d, i, live)
        M["hsml"] = min(M["hsml"], gaps)
        H, idi = float(hs[i]), int(ids[i])
        S = {k: Sum(literal) for k in ("ent", "gv0", "gv1", "gv2", "fws", "mgas")}
        partmass = float(d["mass"][i])
        if seed > 0 and d["mtrack"][i] < seed:
            partmass = float(d["mtrack"][i])
        bhm, rho_i = float(d["bh_mass"][i]), float(d["density"][i])
        iacc = d["gacc"][i] + d["gpm"][i] + d["dfaccel"][i]
        enc = 0
        for j, dx, r2 in zip(cj.tolist(), cdx, cr2.tolist()):
            if d["mass"][j] < 0 or decoupled(j) or int(ids[j]) == idi:
                continue
            info["stats"]["accretion_neighbours"] += 1
            r = math.sqrt(r2)
            mass_j = float(d["mass"][j])
            if typ[j] == 5:
                M["merge"] = min(M["merge"], rel(r, md))
                if r < md:
                    enc = 1
                    flag = par["BlackHoleRepositionEnabled"] == 1 or par["MergeGravBound"] == 0
                    if par["MergeGravBound"] == 1 and par["BlackHoleRepositionEnabled"] == 0:
                        dv = d["vel"][i] - velpred(d, T, j, False)
                        da = iacc - d["gacc"][j] - d["gpm"][j] - d["dfaccel"][j]
                        KE = float((0.5 * dv * dv).sum()) / (atime * atime)
                        PE = float((da * dx).sum()) / atime
                        M["bound"] = min(M["bound"], abs(PE + KE) / (abs(PE) + KE))
                        flag = PE + KE <= 0
                    if flag:
                        other_active = bool(d["active_hydro"][j])
                        if literal:
                            readid = swal.get(j, 0)
                            if (readid != 0 and readid < idi) or (readid == 0 and (int(ids[j]) < idi or not other_active)):
                                swal[j] = idi + 1
                        elif int(ids[j]) < idi or not other_active:
                            swal[j] = max(swal.get(j, 0), idi + 1)
                        if int(ids[j]) < idi or not other_active:
                            markers.setdefault(j, []).append(idi)
            if typ[j] == 0 and r2 < H * H:
                wk = float(kernel_wk(r / H, H, ktype))
                S["ent"].add(mass_j * wk * d["entropy"][j])
                vp = velpred(d, T, j, True)
                for k in range(3):
                    S["gv%d" % k].add(mass_j * wk * vp[k])
                p = (bhm - partmass) * wk / rho_i if (bhm - partmass) > 0 and rho_i > 0 else 0.0
                w = float(rnd[int(ids[j]) % len(rnd)])
                M["swallow"] = min(M["swallow"], abs(w - p))
                if w < p and swal.get(j, 0) < idi + 1:
                    swal[j] = idi + 1
                S["fws"].add(weight(j) * wk if spline else weight(j))
                if par["BlackHoleKineticOn"] == 1:
                    S["mgas"].add(mass_j)
        # post-process
        ent, gv = S["ent"].value, np.array([S["gv%d" % k].value for k in range(3)])
        mdot, medd = 0.0, C["medd_fac"] * bhm
        if rho_i > 0:
            ent /= rho_i
            gv = gv / rho_i
            bhvel = math.sqrt(float(((d["vel"][i] - gv) ** 2).sum())) / atime
            cs = math.sqrt(GAMMA * ent * math.pow(rho_i, GAMMA_MINUS1)) * math.pow(atime, -1.5 * GAMMA_MINUS1)
            norm = math.pow(cs * cs + bhvel * bhvel, 1.5)
            if norm > 0:
                mdot = 4. * math.pi * par["BlackHoleAccretionFactor"] * par["GravInternal"] ** 2 * bhm * bhm * rho_i * C["a3inv"] / norm
        if par["BlackHoleEddingtonFactor"] > 0:
            M["branch"] = min(M["branch"], rel(mdot, par["BlackHoleEddingtonFactor"] * medd))
            if mdot > par["BlackHoleEddingtonFactor"] * medd:
                mdot = par["BlackHoleEddingtonFactor"] * medd
        dt = dtime(i)
        newmass = bhm + mdot * dt
        out["mdot"][i], out["bh_mass"][i], mdot_of[i] = mdot, newmass, mdot
        fac = 0.0
        if par["BH_DRAG"] == 1:
            fac = mdot / float(d["mass"][i])
        if par["BH_DRAG"] == 2:
            fac = par["BlackHoleEddingtonFactor"] * medd / newmass
        fac *= atime
        out["dragaccel"][i] = -(d["vel"][i] - gv) * fac if par["BH_DRAG"] > 0 else 0.0
        kf = 0
        if par["BlackHoleKineticOn"] == 1:
            lam = par["BHKE_EddingtonThrFactor"]
            x = par["BHKE_EddingtonMFactor"] * math.pow(newmass / par["BHKE_EddingtonMPivot"], par["BHKE_EddingtonMIndex"])
            M["branch"] = min(M["branch"], rel(lam, x))
            lam = min(lam, x)
            ke = float(d["kineticfdbkenergy"][i])
            M["branch"] = min(M["branch"], rel(mdot / medd, lam))
            if mdot / medd < lam:
                kf = 1
                eps_ = (rho_i / C["rho_sfr"]) / par["BHKE_EffRhoFactor"]
                M["branch"] = min(M["branch"], rel(eps_, par["BHKE_EffCap"]))
                eps_ = min(eps_, par["BHKE_EffCap"])
                ke += eps_ * (mdot * dt * C["c2"])
                out["kineticfdbkenergy"][i] = ke
            vd = float(d["vdisp"][i])
            thresh = 0.5 * vd * vd * S["mgas"].value * par["BHKE_InjEnergyThr"]
            if vd > 0:
                M["branch"] = min(M["branch"], rel(ke, thresh))
                if ke > thresh:
                    kf = 2
        out["encounter"][i], out["feedbackweightsum"][i], out["bh_entropy"][i] = enc, S["fws"].value, ent
        out["gasvel"][i], out["mgasenc"][i], out["keflag"][i] = gv, S["mgas"].value, kf
        fws[i], keflag[i] = S["fws"].value, kf
        info["sums"][i] = {k: (s.k, s.abs) for k, s in S.items()}
        info["sums"][i]["density"] = rho_i

    for j, who in markers.items():
        w = sorted(set(who))
        if any(b - a == 1 for a, b in zip(w, w[1:])):
            info["consecutive"] = True
    for j, v in swal.items():
        out["sph_swallowid" if typ[j] == 0 else "bh_swallowid"][j] = v
    info["swal"] = dict(swal)

    # ---- the feedback walk and its post-process ---------------------------------------------------------------------------------------
    ftargets = [i for i in targets if swal.get(i, 0) == 0]
    info["feedback_targets"] = ftargets
    info["stats"]["feedback_targets"] = len(ftargets)
    energy, kicks = {}, {}           # per gas particle: the terms of the injected energy, of the velocity kick
    new_entropy = {}                 # literal form: the running entropy
    new_vel = {}
    enttou = lambda j: math.pow(float(d["density"][j]) * C["a3inv"], GAMMA_MINUS1) / GAMMA_MINUS1
    for i in ftargets:
        cj, cdx, cr2, _ = candidates(d, i, live)
        H, idi, rho_i, mtrack = float(hs[i]), int(ids[i]), float(d["density"][i]), float(d["mtrack"][i])
        fenergy = par["BlackHoleFeedbackFactor"] * 0.1 * mdot_of[i] * dtime(i) * C["c2"]
        channel, kenergy = 0, 0.0
        if par["BlackHoleKineticOn"] == 1 and keflag[i] > 0:
            channel = 1
            if keflag[i] == 2:
                kenergy = float(out["kineticfdbkenergy"][i])
        S = {k: Sum(literal) for k in ("mass", "bhmass", "mom0", "mom1", "mom2")}
        progs, mintb = 0, TIMEBINS
        for j, dx, r2 in zip(cj.tolist(), cdx, cr2.tolist()):
            if int(ids[j]) == idi or decoupled(j):
                continue
            info["stats"]["feedback_neighbours"] += 1
            mark = swal.get(j, 0)
            mass_j = float(d["mass"][j])
            if typ[j] == 5 and mark != 0:
                if mark != idi + 1:
                    continue
                out["swallowid"][j], out["swallowtime"][j], out["encounter"][j] = idi, atime, 0
                out["flags"][j] |= 2
                progs += int(d["countprogs"][j])
                S["bhmass"].add(out["bh_mass"][j])
                other = mass_j
                if seed > 0 and mtrack > 0 and d["mtrack"][j] < seed:
                    other = float(d["mtrack"][j])
                S["mass"].add(other)
                vp = velpred(d, T, j, False)
                for k in range(3):
                    S["mom%d" % k].add(other * vp[k])
                info["stats"]["bh_swallowed"] += 1
                continue
            if typ[j] != 0:
                continue
            if mark == 0 and r2 < H * H:
                mintb = min(mintb, int(d["tb_hydro"][j]))
                wk = float(kernel_wk(math.sqrt(r2) / H, H, ktype)) if spline else 1.0
                if fws[i] > 0 and fenergy > 0 and channel == 0 and mass_j > 0:
                    e = fenergy * weight(j) * wk / fws[i]
                    energy.setdefault(j, []).append(e)
                    rho = float(d["density"][j])
                    if par["StarformationOn"] and rho * C["a3inv"] >= par["PhysDensThresh"] and not rho < par["OverDensThresh"] and not d["delaytime"][j] > 0:
                        out["bhheated"][j] = 1
                    if literal:
                        u = new_entropy.get(j, float(d["entropy"][j])) * enttou(j) + e / mass_j
                        new_entropy[j] = min(u, C["ucap"]) / enttou(j)
                if kenergy > 0 and channel == 1 and rho_i > 0:
                    dvel = math.sqrt(2 * kenergy * wk / rho_i)
                    theta = math.acos(2 * float(rnd[(int(ids[j]) + 3) % len(rnd)]) - 1)
                    phi = 2 * math.pi * float(rnd[(int(ids[j]) + 4) % len(rnd)])
                    kick = dvel * np.array([math.sin(theta) * math.cos(phi), math.sin(theta) * math.sin(phi), math.cos(theta)])
                    kicks.setdefault(j, []).append(kick)
                    if literal:
                        new_vel[j] = new_vel.get(j, d["vel"][j].copy()) + kick
            if mark == idi + 1:
                S["mass"].add(mass_j)
                vp = velpred(d, T, j, True)
                for k in range(3):
                    S["mom%d" % k].add(mass_j * vp[k])
                out["flags"][j] |= 1
                info["stats"]["gas_swallowed"] += 1
        # post-process
        accmass, accbh = S["mass"].value, S["bhmass"].value
        mom = np.array([S["mom%d" % k].value for k in range(3)])
        out["mintimebin"][i] = mintb
        out["countprogs"][i] += progs
        if accbh > 0:
            out["bh_mass"][i] += accbh
        if accmass > 0:
            Mi = float(d["mass"][i])
            out["vel"][i] = (d["vel"][i] * Mi + mom) / (Mi + accmass)
            M["branch"] = min(M["branch"], rel(mtrack + accmass, seed) if seed > 0 else np.inf)
            if seed > 0 and mtrack + accmass < seed:
                out["mtrack"][i] = mtrack + accmass
            elif mtrack < seed:
                out["mass"][i] = np.float32(mtrack + accmass)
                out["mtrack"][i] = seed
            else:
                out["mass"][i] = np.float32(Mi + accmass)
        if keflag[i] == 2:
            out["kineticfdbkenergy"][i] = 0
        out["accreted_mass"][i], out["accreted_bhmass"][i], out["accreted_momentum"][i] = accmass, accbh, mom
        info["sums"][i].update({k: (s.k, s.abs) for k, s in S.items()})
    # the gas that received energy or kicks
    info["energy"], info["kicks"] = {}, {}
    for j, terms in energy.items():
        tot = math.fsum(terms)
        u0 = float(d["entropy"][j]) * enttou(j)
        u = u0 + tot / float(d["mass"][j])
        M["cap"] = min(M["cap"], rel(u, C["ucap"]))
        out["entropy"][j] = new_entropy[j] if literal else min(u, C["ucap"]) / enttou(j)
        info["energy"][j] = dict(k=len(terms), sum=tot, abs=tot, u0=u0, u=u, capped=u > C["ucap"], enttou=enttou(j))
    for j, terms in kicks.items():
        t = np.array(terms)
        tot = np.array([math.fsum(t[:, k]) for k in range(3)])
        out["vel"][j] = new_vel[j] if literal else d["vel"][j] + tot
        info["kicks"][j] = dict(k=len(terms), sum=tot, abs=np.abs(t).sum(0))
    return out, info


# ---- inputs shared by the two test modules ---------------------------------------------------------------------------------------------
def bh_density(d, i):
    """the kernel-weighted gas density at black hole i inside its Hsml (what density() leaves in BHP.Density)"""
    g = np.nonzero(d["type"] == 0)[0]
    dx = nearest(d["pos"][i] - d["pos"][g], d["box"])
    r = np.sqrt((dx * dx).sum(1))
    H = d["hsml"][i]
    m = r < H
    return float((d["mass"][g][m].astype(np.float64) * kernel_wk(r[m] / H, H, d["ktype"])).sum())


def sample_scene(pos_gas, box, seed, soft, nbh=40, ndm=30, nstar=20, ktype=1, eta=1.0, ngbfactor=2.0, allgas=True):
    """A particle table: gas (type 0), `nbh` black holes (type 5) placed among the gas, dark matter and stars, garbage and swallowed rows
    (type 7).  Among the black holes (indices relative to the first, b0): 0-1, 2-3 bound pairs and 4-5, 6-7 unbound pairs inside the merger
    distance 2 soft / 2.8; 8-9-10 and 11-12-13 chains of three (neighbours inside the distance, the ends not); 14-15 and 16-17 an inactive one
    next to an active one; 18 in a corner of the box; 19 (with `allgas`) with an Hsml that holds all the gas; 20-21 a pair whose Hsml differ by a
    factor 50; 22-25 with BH_Mass - Mass of tens of gas masses; 32-37 in the middle of the box with a moderate Hsml (without `allgas` they are
    a wave of targets that needs no periodic wrap); the rest single.  `soft` is FORCE_SOFTENING.  Returns a dict of arrays in particle order."""
    rng = np.random.RandomState(seed)
    ng = len(pos_gas)
    md = 2 * soft / 2.8
    at = rng.choice(ng, nbh, replace=False)
    spread = 0.3 * box / ng ** (1. / 3)
    pos_bh = pos_gas[at] + spread * rng.standard_normal((nbh, 3))
    unit = lambda: (lambda v: v / np.linalg.norm(v))(rng.standard_normal(3))
    for a, b in ((0, 1), (2, 3), (4, 5), (6, 7), (14, 15), (16, 17), (20, 21)):
        pos_bh[b] = pos_bh[a] + (0.3 + 0.4 * rng.random_sample()) * md * unit()
    for a in (8, 11):
        u = unit()
        pos_bh[a + 1] = pos_bh[a] + 0.7 * md * u
        pos_bh[a + 2] = pos_bh[a] + 1.4 * md * u
    pos_bh[18] = box * np.array([2e-4, 0.9997, 3e-4])
    pos_bh[32:38] = box * (0.4 + 0.2 * rng.random_sample((6, 3)))
    pos = np.mod(np.concatenate([pos_gas, pos_bh, box * rng.random_sample((ndm + nstar, 3))]), box)
    pos[pos <= 0] += box
    pos = np.ascontiguousarray(pos)
    n, b0 = len(pos), ng
    ptype = np.concatenate([np.zeros(ng, np.uint8), np.full(nbh, 5, np.uint8), np.ones(ndm, np.uint8), np.full(nstar, 4, np.uint8)])
    ids = (1000 + 7 * rng.permutation(n)).astype(np.uint64)        # spaced: no two consecutive
    ids[rng.random_sample(n) < 0.2] += np.uint64(1) << np.uint64(40)   # beyond 32 bits
    mass = (1.0 + 0.2 * rng.random_sample(n)).astype(np.float32)
    h0 = (3 * desnumngb(ktype, eta) / (4 * np.pi * ng)) ** (1. / 3) * box
    hsml = h0 * np.exp(0.2 * rng.standard_normal(n))
    hsml[b0:b0 + nbh] *= ngbfactor ** (1. / 3)
    if allgas:
        hsml[b0 + 19] = 0.9 * box
    hsml[b0 + 32:b0 + 38] = np.minimum(hsml[b0 + 32:b0 + 38], 0.18 * box)
    hsml[b0 + 20] = max(hsml[b0 + 20], 2.5 * md)
    hsml[b0 + 21] = hsml[b0 + 20] / 50.0
    for a, b in ((0, 1), (2, 3), (4, 5), (6, 7), (8, 9), (9, 10), (11, 12), (12, 13), (14, 15), (16, 17)):   # both inside the other's Hsml
        hsml[b0 + a], hsml[b0 + b] = max(hsml[b0 + a], 2.5 * md), max(hsml[b0 + b], 2.5 * md)
    d = dict(pos=pos, type=ptype, box=float(box), n=n, ng=ng, b0=b0, nbh=nbh, ktype=ktype, eta=eta, soft=float(soft), id=ids, mass=mass, hsml=hsml)
    v0 = 0.3
    d["vel"] = v0 * rng.standard_normal((n, 3))
    d["gacc"], d["gpm"], d["hydroacc"] = (rng.standard_normal((n, 3)) for _ in range(3))
    d["dfaccel"] = 0.1 * rng.standard_normal((n, 3))
    d["dfaccel"][ptype != 5] = 0
    d["tb_hydro"] = rng.randint(17, 23, n).astype(np.uint8)
    d["tb_grav"] = rng.randint(17, 23, n).astype(np.uint8)
    d["entropy"] = np.exp(0.5 * rng.standard_normal(n))
    d["density"] = ng * float(mass[:ng].mean()) / box ** 3 * np.exp(0.3 * rng.standard_normal(n))
    d["delaytime"] = np.zeros(n)
    d["delaytime"][rng.choice(ng, ng // 50, replace=False)] = 0.3          # decoupled wind gas
    d["vdisp"] = np.zeros(n)
    d["vdisp"][b0:b0 + nbh] = 0.5 * np.exp(0.5 * rng.standard_normal(nbh))
    d["vdisp"][b0 + 26] = 0.0
    d["active_hydro"] = np.ones(n, np.uint8)
    d["flags"] = np.zeros(n, np.uint8)
    d["bh_mass"], d["mtrack"], d["kineticfdbkenergy"] = np.zeros(n), np.zeros(n), np.zeros(n)
    B = slice(b0, b0 + nbh)
    d["bh_mass"][B] = np.exp(1.2 * rng.standard_normal(nbh))
    d["bh_mass"][b0 + 22:b0 + 26] = mass[b0 + 22:b0 + 26] + np.array([12.0, 25.0, 40.0, 60.0])
    d["mtrack"][B] = np.where(rng.random_sample(nbh) < 0.5, 0.3 + 2.5 * rng.random_sample(nbh), 3.0 + rng.random_sample(nbh))
    d["kineticfdbkenergy"][B] = np.exp(2.0 * rng.standard_normal(nbh) - 1.0)
    d["countprogs"] = np.zeros(n, np.int32)
    d["countprogs"][B] = 1 + rng.randint(0, 4, nbh)
    # pairs: bound (at rest relative to each other, attracted) and unbound (fast)
    for a, b, bound in ((0, 1, 1), (2, 3, 1), (4, 5, 0), (6, 7, 0), (8, 9, 1), (9, 10, 1), (11, 12, 1), (12, 13, 1), (14, 15, 1), (16, 17, 1), (20, 21, 1)):
        ia, ib = b0 + a, b0 + b
        dx = nearest(pos[ia] - pos[ib], box)
        for k in ("gacc", "gpm", "dfaccel"):
            d[k][ib] = d[k][ia] + (dx / md if k == "gacc" else 0.0)
        d["tb_grav"][ib] = d["tb_grav"][ia]
        d["vel"][ib] = d["vel"][ia] + (0.01 if bound else 3.0) * rng.standard_normal(3)
    d["inactive"] = np.array([b0 + 15, b0 + 16])
    d["active_hydro"][d["inactive"]] = 0
    # the black holes' density: the kernel sum of the gas around them, as density() leaves it
    for i in range(b0, b0 + nbh):
        d["density"][i] = bh_density(d, i) * (0.9 + 0.2 * rng.random_sample())
    d["density"][b0 + 27] = 0.0                                             # no gas density: no accretion, no kicks
    dead = np.concatenate([rng.choice(ng, 12, replace=False), [b0 + nbh - 1, b0 + nbh - 2], n - 1 - rng.choice(nstar, 3, replace=False)])
    d["dead"] = dead
    d["type_table"] = ptype.copy()
    d["flags"][dead] = 1
    d["flags"][b0 + nbh - 1] = 2                                            # a black hole swallowed on an earlier step
    d["type"][dead] = 7
    return d


def heat_near_cap(d, par, T, gas, frac=0.9995):
    """entropy of the listed gas particles so that their internal energy is `frac` of the 5e8 K cap"""
    C = constants(par, T)
    for j in gas:
        d["entropy"][j] = frac * C["ucap"] / (math.pow(float(d["density"][j]) * C["a3inv"], GAMMA_MINUS1) / GAMMA_MINUS1)
