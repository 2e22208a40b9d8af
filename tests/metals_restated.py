"""numpy restatement of metal_return (libgadget/metal_return.c), written from the cited lines, over ALL pairs (no tree): metals_haswork
:714-724, stellar_density :930-1006 (effhsml :778-804, stellar_density_ngbiter :879-928, stellar_density_check_neighbours :827-877, with
ngb_narrow_down of treewalk.c:1371-1434 from veldisp_restated), metal_return_ngbiter :637-709 and metal_return_postprocess :623-631.  The
yields (metal_yield) are inputs: MassGenerated, MetalGenerated, MetalSpeciesGenerated per star.

Two forms of the return walk:
  (a) return_literal   the reference's own arithmetic, stars one after another in a given order: P.Mass and SphP.Metals are float and are
                       rounded after every contribution, the cap is tested on the RUNNING mass, Mass / Density is taken from the running
                       values.
  (b) return_defined   what the engine defines (include/mpgadget_hip.h): every contribution tested against the mass at call entry, the
                       accepted ones summed per gas particle in fp64 and applied once.
The radius loop is one function; its neighbour walk is the literal one (per neighbour, with the shrinking search radius) in a visiting
order the caller may permute.
Not a test module: imported by test_metals_restated.py (runs anywhere) and test_gpu_metals.py (the HIP path)."""
import math

import numpy as np

from veldisp_restated import MAXITER, NoConvergence, nearest, ngb_narrow_down

NHSML = 10           # metal_return.c:733
NMETALS = 9          # slotsmanager.h
NORM_COEFF = 4.188790204786   # densitykernel.h:6
EPS = float(np.finfo(np.float64).eps)

# enum DensityKernelType -> (support, sigma[3D]) of densitykernel.c:92-122
KERNELS = {1: (2.0, 1 / math.pi), 2: (3.0, 1 / (120 * math.pi)), 4: (2.5, 1 / (20 * math.pi))}


class MetalError(RuntimeError):
    """a target with Hsml <= 0 on entry, or one that ends with StarVolumeSPH == 0 (endrun(3), metal_return.c:988-989)"""


def desnumngb(ktype, eta):
    """GetNumNgb -> density_kernel_desnumngb, densitykernel.c:124-131"""
    return NORM_COEFF * math.pow(KERNELS[ktype][0] * eta, 3)


def _poly(ktype, q):
    """the kernel polynomials of densitykernel.c:24-90 (scalar or array q)"""
    q = np.asarray(q, np.float64)
    p = lambda c: np.maximum(c - q, 0.0)
    if ktype == 1:
        return 0.25 * p(2.) ** 3 - p(1.) ** 3
    if ktype == 2:
        return p(3.) ** 5 - 6 * p(2.) ** 5 + 15 * p(1.) ** 5
    return p(2.5) ** 4 - 5 * p(1.5) ** 4 + 10 * p(.5) ** 4


def wknorm(H, ktype):
    """density_kernel_init, densitykernel.c:139-153"""
    support, sigma = KERNELS[ktype]
    hinv = (1. / H) * support
    return sigma * hinv * hinv * hinv


def kernel_wk(u, H, ktype):
    """density_kernel_wk: Wknorm * wk(u * support)"""
    return wknorm(H, ktype) * _poly(ktype, np.asarray(u) * KERNELS[ktype][0])


def kernel_volume(H):
    return NORM_COEFF * math.pow(H, 3)


def effhsml(left, right, hsml, box, i):
    """effhsml, metal_return.c:778-804 (without the zero-Hsml repair: Hsml <= 0 is an error of the call)"""
    if right > 0.99 * box:
        right = hsml * ((1. + NHSML) / NHSML)
    if left == 0:
        left = 0.1 * hsml
    rvol = math.pow(right, 3)
    lvol = math.pow(left, 3)
    return math.pow((1. * i + 1) / (1. * NHSML + 1) * (rvol - lvol) + lvol, 1. / 3)


def targets(ptype, mass, totalmassreturned, massgenerated, active=None):
    """metals_haswork (:714-724) over the active list, in particle order; garbage and swallowed rows carry type 7"""
    idx = np.arange(len(ptype)) if active is None else np.sort(np.asarray(active))
    return [int(i) for i in idx
            if ptype[i] == 4 and not massgenerated[i] < 1e-3 * (np.float64(mass[i]) + totalmassreturned[i])]


def literal_walk(r2, wk, vol, radii, des, sphweight, order=None):
    """treewalk_visit_nolist_ngbiter + stellar_density_ngbiter (:879-928) for one target: the gas particles in `order` (default: index
    order), the search radius starting at radii[9] and shrinking to radii[i], maxcmpte to i + 1, as soon as the running Ngb[i] exceeds
    desnumngb.  wk[i][k]: the kernel value of gas k at radius i.  Returns (Ngb[10], VolumeSPH[10], maxcmpte, visited)."""
    Ngb = [0.0] * NHSML
    Vol = [0.0] * NHSML
    HH = [h * h for h in radii]
    kvol = [kernel_volume(h) for h in radii]
    maxcmpte = NHSML
    hs = radii[NHSML - 1]
    first = r2 <= hs * hs           # (candidates beyond the FIRST search radius can never pass a later, smaller one)
    cand = np.nonzero(first)[0] if order is None else np.asarray(order)[first[np.asarray(order)]]
    visited = 0
    for k in cand:
        r2k = r2[k]
        if r2k > hs * hs:           # treewalk.c:1226-1233
            continue
        visited += 1
        for i in range(maxcmpte):
            if r2k < HH[i]:
                w = wk[i][k]
                Ngb[i] += w * kvol[i]                          # :908
                Vol[i] += vol[k] * w if sphweight else vol[k]  # :910-913
        for i in range(NHSML):
            if Ngb[i] > des:
                maxcmpte = i + 1
                hs = radii[i]
                break
    return Ngb, Vol, maxcmpte, visited


def stellar_density(pos, ptype, mass, density, hsml, tlist, box, ktype, eta, maxdev, sphweight, order=None, maxiter=MAXITER):
    """stellar_density.  hsml is updated in place (assigned on every pass).  Returns a dict of what the loop did: queue_lengths per iteration
    and, keyed by target, iterations, maxcmpte, close, radius (the trial radius of the final sums), volume (StarVolumeSPH), numngb, tight,
    vol_n / vol_abs (terms and sum of absolute terms of the final volume), first_count (gas inside the first search radius); min_gap (the
    smallest relative distance of a gas particle from a trial radius used) and min_margin (the smallest relative distance of a deciding Ngb
    from desnumngb and from desnumngb +- MaxNgbDeviation)."""
    pos = np.asarray(pos, np.float64)
    gas = np.nonzero(ptype == 0)[0]
    gpos = pos[gas]
    vol = mass[gas].astype(np.float64) / density[gas]
    des = desnumngb(ktype, eta)
    support = KERNELS[ktype][0]
    res = dict(queue_lengths=[], iterations={}, maxcmpte={}, close={}, radius={}, volume={}, numngb={}, tight={}, vol_n={}, vol_abs={},
               first_count={}, trial_radii={}, min_gap=float("inf"), min_margin=float("inf"), des=des)
    for i in tlist:
        if not hsml[i] > 0:
            raise MetalError("Hsml <= 0 for star %d" % i)
        res["iterations"][i] = 0
        res["trial_radii"][i] = []
    Left = {i: 0.0 for i in tlist}
    Right = {i: float(box) for i in tlist}
    queue = list(tlist)
    niter = 0
    while queue:
        niter += 1
        res["queue_lengths"].append(len(queue))
        redo = []
        for i in queue:
            radii = [effhsml(Left[i], Right[i], float(hsml[i]), box, j) for j in range(NHSML)]
            res["trial_radii"][i].extend(radii)
            dist = nearest(pos[i] - gpos, box)
            r2 = (dist * dist).sum(1)
            r = np.sqrt(r2)
            if res["iterations"][i] == 0:
                res["first_count"][i] = int((r2 <= radii[-1] ** 2).sum())
            near = r2 <= radii[-1] ** 2
            w = []
            for rj in radii:
                res["min_gap"] = min(res["min_gap"], float(np.abs(r - rj).min() / rj))
                wj = np.zeros(len(gas))
                wj[near] = kernel_wk(r[near] * (1. / rj), rj, ktype)
                w.append(wj)
            Ngb, Vol, maxcmpt, _ = literal_walk(r2, w, vol, radii, des, sphweight, order)
            for j in range(maxcmpt):       # the values that decide maxcmpte and the bracket
                res["min_margin"] = min(res["min_margin"], abs(Ngb[j] - des) / des, abs(Ngb[j] - int(des)) / des)
            newh, Right[i], Left[i], close = ngb_narrow_down(Right[i], Left[i], radii, Ngb, maxcmpt, int(des), box)
            hsml[i] = newh
            numngb = Ngb[close]
            for edge in (des - maxdev, des + maxdev):
                res["min_margin"] = min(res["min_margin"], abs(numngb - edge) / des)
            res["iterations"][i] += 1
            res["maxcmpte"][i] = maxcmpt
            res["close"][i] = close
            res["radius"][i] = radii[close]
            res["volume"][i] = Vol[close]
            res["numngb"][i] = numngb
            inside = r2 < radii[close] ** 2
            res["vol_n"][i] = int(inside.sum())
            res["vol_abs"][i] = Vol[close]          # all terms are non-negative
            off = numngb < des - maxdev or numngb > des + maxdev
            if off and not (Right[i] - Left[i]) < 1.0e-4 * Left[i]:
                redo.append(i)
                continue
            res["tight"][i] = bool(off)
        queue = redo
        if queue and niter > maxiter:
            raise NoConvergence("failed to converge density for %d particles" % len(queue))
    for i in tlist:
        if res["volume"][i] == 0:
            raise MetalError("StarVolumeSPH == 0 for star %d" % i)
    return res


def _pairs(pos, gas, gpos, i, hsml_i, box, ktype, sphweight):
    """the gas inside a star's final radius (r2 > 0 && r2 < HH, :660), their kernel values, the closest any gas comes to the radius, and
    |d ln wk / d ln Hsml| per pair (a centred difference of 1e-6; 0 without SPHWeighting)"""
    dist = nearest(pos[i] - gpos, box)
    r2 = (dist * dist).sum(1)
    sel = np.nonzero((r2 > 0) & (r2 < hsml_i * hsml_i))[0]
    r = np.sqrt(r2[sel])
    wk = kernel_wk(r * (1. / hsml_i), hsml_i, ktype) if sphweight else np.ones(len(sel))
    gap = float(np.abs(np.sqrt(r2) - hsml_i).min() / hsml_i)
    sens = np.zeros(len(sel))
    if sphweight and len(sel):
        e = 1e-6
        hp, hm = hsml_i * (1 + e), hsml_i * (1 - e)
        wp, wm = kernel_wk(r * (1. / hp), hp, ktype), kernel_wk(r * (1. / hm), hm, ktype)
        sens = np.abs(wp - wm) / (2 * e * wk)
    return sel, wk, gap, sens


def return_defined(d, tlist, hsml, volume, box, ktype, sphweight, maxgasmass):
    """form (b).  d: dict of the arrays in particle order (pos, type, mass float32, density, metallicity, metals, massgenerated,
    metalgenerated, speciesgenerated, stellarage, totalmassreturned, lastenrichment).  Returns the new arrays and the bookkeeping the bounds
    are made of: per gas particle k (accepted contributions), the sums of absolute terms; per star n accepted and massreturn; refused;
    sens_M / sens_Z / sens_S per gas particle and sens_star per star: sum of |term| (|d ln wk / d ln Hsml| + 1), what a relative change of
    the stars' Hsml and StarVolumeSPH moves the sums by to first order; cap_margin: the smallest relative distance from MaxGasMass of (entry mass + one contribution) over the refused and of (entry mass + ALL
    accepted contributions) over the accepted - positive iff the reference's thread order cannot matter; min_gap as in stellar_density."""
    pos = np.asarray(d["pos"], np.float64)
    gas = np.nonzero(d["type"] == 0)[0]
    gpos = pos[gas]
    M = d["mass"][gas].astype(np.float64)
    vol = M / d["density"][gas]
    ng = len(gas)
    dM = np.zeros(ng)
    dZ = np.zeros(ng)
    dS = np.zeros((ng, NMETALS))
    k = np.zeros(ng, np.int64)
    out = {key: d[key].copy() for key in ("mass", "density", "metallicity", "metals", "totalmassreturned", "lastenrichment")}
    massreturn, nacc, accepted_metal = {}, {}, 0.0
    refused = 0
    margin = float("inf")
    min_gap = float("inf")
    largest_single = np.zeros(ng)
    sens_M, sens_Z, sens_S, sens_star = np.zeros(ng), np.zeros(ng), np.zeros((ng, NMETALS)), {}
    for i in tlist:
        sel, wk, gap, sens = _pairs(pos, gas, gpos, i, float(hsml[i]), box, ktype, sphweight)
        min_gap = min(min_gap, gap)
        rf = wk * vol[sel] / volume[i]
        tm = rf * d["massgenerated"][i]
        ok = ~(M[sel] + tm > maxgasmass)
        refused += int((~ok).sum())
        if (~ok).any():
            margin = min(margin, float(((M[sel] + tm)[~ok] / maxgasmass - 1).min()))
        a = sel[ok]
        dM[a] += tm[ok]
        dZ[a] += rf[ok] * d["metalgenerated"][i]
        dS[a] += rf[ok][:, None] * d["speciesgenerated"][i][None, :]
        k[a] += 1
        largest_single[a] = np.maximum(largest_single[a], tm[ok])
        # first-order reach of a relative change of this star's Hsml and StarVolumeSPH: |term| (|d ln wk / d ln h| + 1)
        lever = sens[ok] + 1
        sens_M[a] += tm[ok] * lever
        sens_Z[a] += rf[ok] * d["metalgenerated"][i] * lever
        sens_S[a] += (rf[ok] * lever)[:, None] * d["speciesgenerated"][i][None, :]
        sens_star[i] = float((tm[ok] * lever).sum())
        mr = float(tm[ok].sum())
        massreturn[i] = mr
        nacc[i] = int(ok.sum())
        accepted_metal += float((rf[ok] * d["metalgenerated"][i]).sum())
        out["mass"][i] = np.float32(np.float64(d["mass"][i]) - mr)
        out["totalmassreturned"][i] = d["totalmassreturned"][i] + mr
        out["lastenrichment"][i] = d["stellarage"][i]
    touched = dM > 0
    if touched.any():
        margin = min(margin, float((1 - (M + dM)[touched] / maxgasmass).min()))
    Mnew = M + dM
    g = gas[touched]
    Zold = d["metallicity"][gas]
    Sold = d["metals"][gas]
    out["metals"][g] = ((Sold * M[:, None] + dS) / Mnew[:, None])[touched]
    out["metallicity"][g] = ((Zold * M + dZ) / Mnew)[touched]
    out["density"][g] = (d["density"][gas] * (Mnew / M))[touched]
    out["mass"][g] = Mnew[touched].astype(np.float32)
    info = dict(gas=gas, k=k, dM=dM, dZ=dZ, dS=dS, Mnew=Mnew, massreturn=massreturn, nacc=nacc, refused=refused, cap_margin=margin, min_gap=min_gap,
                abs_Z=np.abs(Zold) * M + dZ, abs_S=np.abs(Sold) * M[:, None] + dS, accepted_metal=accepted_metal, touched=touched,
                sens_M=sens_M, sens_Z=sens_Z, sens_S=sens_S, sens_star=sens_star)
    return out, info


def return_literal(d, star_order, hsml, volume, box, ktype, sphweight, maxgasmass):
    """form (a): metal_return_ngbiter as written, the stars in `star_order`, each star's neighbours in index order (they are distinct gas
    particles, so the order inside one star cannot matter).  P.Mass is float, SphP.Metals is float[9], everything else double."""
    pos = np.asarray(d["pos"], np.float64)
    gas = np.nonzero(d["type"] == 0)[0]
    gpos = pos[gas]
    mass = d["mass"].astype(np.float32).copy()
    density = d["density"].copy()
    metallicity = d["metallicity"].copy()
    metals = d["metals"].astype(np.float32)
    tmr = d["totalmassreturned"].copy()
    last = d["lastenrichment"].copy()
    massreturn = {}
    refused = 0
    for i in star_order:
        sel, wk, _, _ = _pairs(pos, gas, gpos, i, float(hsml[i]), box, ktype, sphweight)
        g = gas[sel]
        Mj = mass[g].astype(np.float64)
        rf = wk * (Mj / density[g]) / volume[i]                 # :674-675
        tm = rf * d["massgenerated"][i]
        ok = ~(Mj + tm > maxgasmass)                            # :680
        refused += int((~ok).sum())
        g, Mj, rf, tm = g[ok], Mj[ok], rf[ok], tm[ok]
        this = rf[:, None] * d["speciesgenerated"][i][None, :]
        metals[g] = ((metals[g].astype(np.float64) * Mj[:, None] + this) / (Mj + tm)[:, None]).astype(np.float32)   # :691
        metallicity[g] = (metallicity[g] * Mj + rf * d["metalgenerated"][i]) / (Mj + tm)                               # :693
        massfrac = (Mj + tm) / Mj
        mass[g] = (Mj * massfrac).astype(np.float32)                                                                   # :696
        density[g] = density[g] * massfrac                                                                             # :700
        mr = float(tm.sum())
        massreturn[i] = mr
        mass[i] = np.float32(np.float64(mass[i]) - mr)
        tmr[i] += mr
        last[i] = d["stellarage"][i]
    return dict(mass=mass, density=density, metallicity=metallicity, metals=metals, totalmassreturned=tmr, lastenrichment=last,
                massreturn=massreturn, refused=refused)


def metal_return(d, box, ktype, eta, maxdev, sphweight, maxgasmass, active=None, order=None):
    """the whole call in form (b): returns (out arrays incl. hsml, loop results, return info); no target: (None, None, None)"""
    tl = targets(d["type"], d["mass"], d["totalmassreturned"], d["massgenerated"], active)
    if not tl:
        return None, None, None
    hsml = d["hsml"].copy()
    res = stellar_density(d["pos"], d["type"], d["mass"], d["density"], hsml, tl, box, ktype, eta, maxdev, sphweight, order)
    out, info = return_defined(d, tl, hsml, res["volume"], box, ktype, sphweight, maxgasmass)
    out["hsml"] = hsml
    res["targets"] = tl
    return out, res, info


# ---- inputs shared by the two test modules ---------------------------------------------------------------------------------------------
def sample_scene(pos_gas, box, nstar, seed, ktype=2, eta=1.0, nbh=4, ndm=50, nheavy=8):
    """A particle table: gas (type 0), `nbh` black holes (type 5) at gas-like places, `ndm` dark matter rows, then `nstar` stars (type 4) drawn
    near gas positions - one of them in the corner of the box -, with garbage / swallowed rows (type 7) among gas and stars.  Entry Hsml of the
    stars is the radius of desnumngb gas particles at mean density times 0.05 (a fifth of them), 20 (a tenth) or 1; a tenth of the stars lie
    below the 1e-3 work threshold; `nheavy` gas particles sit just below MaxGasMass = 4 <m> so that every sizeable contribution to them is
    refused.  Returns a dict of arrays in particle order."""
    rng = np.random.RandomState(seed)
    ng = len(pos_gas)
    at = rng.choice(ng, nstar + nbh, replace=False)
    spread = 0.3 * box / ng ** (1. / 3)
    pos_bh = pos_gas[at[:nbh]] + spread * rng.standard_normal((nbh, 3))
    pos_st = pos_gas[at[nbh:]] + spread * rng.standard_normal((nstar, 3))
    pos_st[0] = box * np.array([3e-4, 0.9998, 2e-4])                       # a search that crosses a corner
    pos = np.mod(np.concatenate([pos_gas, pos_bh, box * rng.random_sample((ndm, 3)), pos_st]), box)
    pos[pos <= 0] += box
    pos = np.ascontiguousarray(pos)
    n = len(pos)
    s0 = ng + nbh + ndm
    ptype = np.concatenate([np.zeros(ng, np.uint8), np.full(nbh, 5, np.uint8), np.ones(ndm, np.uint8), np.full(nstar, 4, np.uint8)])
    mass = (1.0 + 0.2 * rng.random_sample(n)).astype(np.float32)
    avg = float(mass[:ng].astype(np.float64).mean())
    maxgasmass = 4 * avg
    heavy = rng.choice(ng, nheavy, replace=False)
    mass[heavy] = np.float32(maxgasmass * (1 - 3e-7))
    density = ng * avg / box ** 3 * np.exp(0.3 * rng.standard_normal(n))
    h0 = (3 * desnumngb(ktype, eta) / (4 * np.pi * ng)) ** (1. / 3) * box
    hsml = h0 * np.exp(0.2 * rng.standard_normal(n))
    kind = rng.random_sample(nstar)
    hsml[s0:][kind < 0.2] *= 0.05
    hsml[s0:][kind > 0.9] *= 20.0
    massgen = np.zeros(n)
    massgen[s0:] = mass[s0:] * (0.004 + 0.06 * rng.random_sample(nstar))
    massgen[s0:][::7] *= 8.0                                               # some large returns: refusals by the cap
    low = s0 + rng.choice(nstar, nstar // 10, replace=False)
    massgen[low] = 5e-4 * mass[low]                                        # below the 1e-3 work threshold
    tmr = np.zeros(n)
    tmr[s0:] = 0.05 * rng.random_sample(nstar)
    metalgen = massgen * 0.02 * rng.random_sample(n)
    species = metalgen[:, None] * rng.dirichlet(np.ones(NMETALS), n) * 0.9
    d = dict(pos=pos, type=ptype, box=float(box), n=n, ng=ng, nstar=nstar, s0=s0, mass=mass, density=density, hsml=hsml,
             massgenerated=massgen, metalgenerated=metalgen, speciesgenerated=np.ascontiguousarray(species),
             stellarage=100.0 + 50.0 * rng.random_sample(n), totalmassreturned=tmr, lastenrichment=10.0 * rng.random_sample(n),
             metallicity=0.01 * rng.random_sample(n), metals=np.ascontiguousarray(1e-3 * rng.random_sample((n, NMETALS))),
             maxgasmass=maxgasmass, ktype=ktype, eta=eta, heavy=heavy)
    dead = np.concatenate([rng.choice(ng, 12, replace=False), s0 + 1 + rng.choice(nstar - 1, 6, replace=False)])
    d["dead"] = dead
    d["type_table"] = ptype.copy()      # the types as the table holds them; the dead rows carry IsGarbage (the last one: Swallowed)
    d["type"][dead] = 7
    return d
