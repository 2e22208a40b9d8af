"""numpy restatement of winds_find_vel_disp (libgadget/veldisp.c:375-466), written from the cited lines: the DM velocity dispersion of
star-forming gas (the radius loop of treewalk_do_hsml_loop with wind_vdisp_ngbiter / wind_vdisp_postprocess / ngb_narrow_down) and of
black holes (blackhole_veldisp).  Distances are brute force over every DM particle with the periodic wrap; the neighbours of a target are
visited in a fixed order (DM index, or a permutation the caller passes) with the reference's literal shrinking search radius.
Not a test module: imported by test_veldisp_restated.py (runs anywhere) and test_gpu_veldisp.py (the HIP path)."""
import math

import numpy as np

NWINDHSML = 5        # veldisp.c:16
NUMDMNGB = 40        # veldisp.c:17
MAXDMDEVIATION = 1   # veldisp.c:18
MAXITER = 400        # treewalk.h:214


class NoConvergence(RuntimeError):
    """endrun(1155, "failed to converge density ..."), treewalk.c:1361-1363"""


def nearest(x, box):
    """NEAREST, partmanager.h:99"""
    x = np.asarray(x, np.float64)
    return np.where(x > 0.5 * box, x - box, np.where(x < -0.5 * box, x + box, x))


def dm_velpred(vel, gacc, gpm, tb_grav, gravkicks, FgravkickB):
    """DM_VelPred, density.c:106-112"""
    return vel + np.asarray(gravkicks, np.float64)[tb_grav][:, None] * gacc + gpm * FgravkickB


def effdmradius(left, right, dmradius, box, i):
    """vdispeffdmradius, veldisp.c:204-219"""
    if right > 0.99 * box:
        right = dmradius
    if left == 0:
        left = 0.1 * dmradius
    rvol = math.pow(right, 3)
    lvol = math.pow(left, 3)
    return math.pow((1.0 * i + 1) / (1.0 * NWINDHSML + 1) * (rvol - lvol) + lvol, 1. / 3)


def _cbrt(v):
    """pow(v, 1./3) of C: NaN for a negative argument (Python's math.pow raises instead)"""
    return math.pow(v, 1. / 3) if v >= 0 else float("nan")


def ngb_narrow_down(right, left, radius, numNgb, maxcmpt, desnumngb, box):
    """ngb_narrow_down, treewalk.c:1371-1434.  Returns (hsml, right, left, close).
    maxcmpt == 1: the reference reads radius[1] and numNgb[1] (:1418-1419), which nothing defines, and the line after (:1421-1422)
    overwrites what it computed from them; the defined outcome, dngbdv = numNgb[0] / radius[0]^3, is what stands here.  The growth branch
    (:1400) uses the last two entries only when maxcmpt > 1."""
    close = 0
    ngbdist = abs(numNgb[0] - desnumngb)
    for j in range(1, maxcmpt):
        newdist = abs(numNgb[j] - desnumngb)
        if newdist < ngbdist:
            ngbdist = newdist
            close = j
    for j in range(maxcmpt):
        if numNgb[j] < desnumngb:
            left = radius[j]
        if numNgb[j] > desnumngb:
            right = radius[j]
            break
    hsml = radius[close]
    if right > 0.99 * box:
        dngbdv = 0.0
        if maxcmpt > 1 and radius[maxcmpt - 1] > radius[maxcmpt - 2]:
            dngbdv = (numNgb[maxcmpt - 1] - numNgb[maxcmpt - 2]) / (math.pow(radius[maxcmpt - 1], 3) - math.pow(radius[maxcmpt - 2], 3))
        newhsml = 4 * hsml
        if dngbdv > 0:
            dngb = desnumngb - numNgb[maxcmpt - 1]
            newvolume = math.pow(hsml, 3) + dngb / dngbdv
            if _cbrt(newvolume) < newhsml:
                newhsml = _cbrt(newvolume)
        hsml = newhsml
    if hsml > right:
        hsml = right
    if left == 0:
        dngbdv = 0.0
        if maxcmpt > 1:
            if radius[1] > radius[0]:
                dngbdv = (numNgb[1] - numNgb[0]) / (math.pow(radius[1], 3) - math.pow(radius[0], 3))
        elif radius[0] > 0:
            dngbdv = numNgb[0] / math.pow(radius[0], 3)
        if dngbdv > 0:
            dngb = desnumngb - numNgb[0]
            newvolume = math.pow(hsml, 3) + dngb / dngbdv
            hsml = _cbrt(newvolume)
    if hsml < left:
        hsml = left
    return hsml, right, left, close


def literal_walk(r2, vterm, radii, order=None):
    """treewalk_visit_nolist_ngbiter (treewalk.c:1212-1241) + wind_vdisp_ngbiter (veldisp.c:233-284) for one target: the DM particles in
    `order` (default: index order), the search radius starting at radii[4] and shrinking to radii[i], maxcmpte to i + 1, as soon as the
    running Ngb[i] exceeds 40 (the scan for i restarts from 0 at every neighbour).  r2[k]: squared distance of DM particle k (r = sqrt(r2),
    treewalk.c:1238), vterm[k][3]: its velocity term.  Returns (Ngb[5], V1sum[5][3], V2sum[5], maxcmpte, visited); entries at and beyond maxcmpte are what the walk left."""
    Ngb = [0.0] * NWINDHSML
    V1 = [[0.0, 0.0, 0.0] for _ in range(NWINDHSML)]
    V2 = [0.0] * NWINDHSML
    maxcmpte = NWINDHSML
    hsml = radii[NWINDHSML - 1]
    visited = 0
    r = np.sqrt(r2)
    # (candidates beyond the FIRST search radius can never pass a later, smaller one: leave them out of the Python loop)
    cand = np.nonzero(r2 <= hsml * hsml)[0] if order is None else np.asarray(order)[(r2 <= hsml * hsml)[np.asarray(order)]]
    for k in cand:
        rk = r[k]
        if r2[k] > hsml * hsml:            # treewalk.c:1226-1233 (r2 > h2)
            continue
        visited += 1
        for i in range(maxcmpte):
            if rk < radii[i]:
                Ngb[i] += 1
                for d in range(3):
                    vel = vterm[k][d]
                    V1[i][d] += vel
                    V2[i] += vel * vel
        for i in range(NWINDHSML):
            if Ngb[i] > NUMDMNGB:
                maxcmpte = i + 1
                hsml = radii[i]
                break
    return Ngb, V1, V2, maxcmpte, visited


def gas_targets(ptype, hsml, dthsml, density, ddrift, sfr_density_threshold, active=None):
    """winds_veldisp_haswork (veldisp.c:348-371) over the active list; garbage and swallowed particles carry type 7"""
    n = len(ptype)
    idx = np.arange(n) if active is None else np.asarray(active)
    out = []
    for i in idx:
        if ptype[i] != 0:
            continue
        with np.errstate(all="ignore"):
            densfac = (hsml[i] + dthsml[i] * ddrift) / hsml[i]
            if densfac > 1:
                densfac = 1
            if density[i] / (densfac * densfac * densfac) < 0.1 * sfr_density_threshold:
                continue
        out.append(int(i))
    return out


def find_vel_disp(pos, ptype, vel, gacc, gpm, tb_grav, hsml, dthsml, density, vdisp, box, Time, hubble, ddrift, sfr_density_threshold,
                  gravkicks, FgravkickB, active=None, order=None, maxiter=MAXITER):
    """winds_find_vel_disp.  vdisp is updated in place where the reference writes it.  Returns a dict of what the loop did:
    built (the DM tree was demanded), queue_lengths per iteration, and per target (dicts keyed by particle index) iterations, numngb
    (the final closest count), maxcmpte, radius (the trial radius of the final sums), trial_radii (every trial radius used, all
    iterations), var (the final variance), V2 / n of the final sums, tight (ended through the narrow bracket with a count outside 39..41);
    min_gap: the smallest relative distance between a DM particle and a trial radius (or a black hole's Hsml) over the whole call."""
    pos = np.asarray(pos, np.float64)
    dm = np.nonzero(ptype == 1)[0]
    idx = np.arange(len(ptype)) if active is None else np.asarray(active)
    bhs = [int(i) for i in idx if ptype[i] == 5]                       # blackhole_dynfric_haswork, veldisp.c:53-57
    gas = gas_targets(ptype, hsml, dthsml, density, ddrift, sfr_density_threshold, active)
    res = dict(built=False, queue_lengths=[], iterations={}, numngb={}, maxcmpte={}, radius={}, trial_radii={}, var={}, v2n={}, tight={},
               bh_numdm={}, bh_var={}, bh_v2n={}, min_gap=float("inf"))
    totbh = int((ptype == 5).sum())
    if len(gas) == 0 and totbh == 0:                                   # veldisp.c:413
        return res
    res["built"] = True
    velpred = dm_velpred(vel[dm], gacc[dm], gpm[dm], tb_grav[dm], gravkicks, FgravkickB)
    dmpos = pos[dm]
    for i in bhs:                                                      # blackhole_veldisp_ngbiter / _postprocess, veldisp.c:59-107
        dist = nearest(pos[i] - dmpos, box)
        r2 = (dist * dist).sum(1)
        sel = np.nonzero(r2 < hsml[i] * hsml[i])[0]
        if hsml[i] > 0:
            res["min_gap"] = min(res["min_gap"], float(np.abs(np.sqrt(r2) - hsml[i]).min() / hsml[i]))
        numdm = float(len(sel))
        V1 = [0.0, 0.0, 0.0]
        V2 = 0.0
        for k in sel:
            for d in range(3):
                v = velpred[k][d] - vel[i][d]
                V1[d] += v
                V2 += v * v
        res["bh_numdm"][i] = int(numdm)
        if numdm > 0:
            var = V2 / numdm
            for d in range(3):
                var -= math.pow(V1[d] / numdm, 2)
            res["bh_var"][i] = var
            res["bh_v2n"][i] = V2 / numdm
            if var > 0:
                vdisp[i] = math.sqrt(var / 3)
    if len(gas) == 0:
        return res
    Left = {i: 0.0 for i in gas}
    Right = {i: float(box) for i in gas}
    DMRadius = {i: float(hsml[i]) for i in gas}
    for i in gas:
        res["iterations"][i] = 0
        res["trial_radii"][i] = []
    ha2 = hubble * Time * Time
    queue = list(gas)
    niter = 0
    while queue:                                                       # treewalk_do_hsml_loop, treewalk.c:1292-1364
        niter += 1
        res["queue_lengths"].append(len(queue))
        redo = []
        for i in queue:
            radii = [effdmradius(Left[i], Right[i], DMRadius[i], box, j) for j in range(NWINDHSML)]
            res["trial_radii"][i].extend(radii)
            dist = nearest(pos[i] - dmpos, box)
            r2 = (dist * dist).sum(1)
            vterm = velpred - vel[i] + ha2 * dist                      # veldisp.c:265
            with np.errstate(all="ignore"):
                for rj in radii:                                       # how close a DM particle comes to a trial radius (relative)
                    if rj > 0:
                        res["min_gap"] = min(res["min_gap"], float(np.abs(np.sqrt(r2) - rj).min() / rj))
            Ngb, V1, V2, maxcmpt, _ = literal_walk(r2, vterm, radii, order)
            newr, Right[i], Left[i], close = ngb_narrow_down(Right[i], Left[i], radii, Ngb, maxcmpt, NUMDMNGB, box)
            DMRadius[i] = newr
            numngb = Ngb[close]
            res["iterations"][i] += 1
            res["numngb"][i] = int(numngb)
            res["maxcmpte"][i] = maxcmpt
            res["radius"][i] = radii[close]
            off = numngb < NUMDMNGB - MAXDMDEVIATION or numngb > NUMDMNGB + MAXDMDEVIATION
            if off and Right[i] - Left[i] > 5e-6 * Left[i]:
                redo.append(i)
                continue
            res["tight"][i] = bool(off)
            with np.errstate(all="ignore"):
                var = np.float64(V2[close]) / numngb
                for d in range(3):
                    var -= (np.float64(V1[close][d]) / numngb) ** 2
            res["var"][i] = float(var)
            res["v2n"][i] = float(np.float64(V2[close]) / numngb) if numngb > 0 else 0.0
            if var > 0:
                vdisp[i] = math.sqrt(var / 3)
        queue = redo
        if queue and niter > maxiter:
            raise NoConvergence("failed to converge density for %d particles" % len(queue))
    return res


# ---- inputs shared by the two test modules ---------------------------------------------------------------------------------------------
def sample_inputs(pos_gas, pos_dm, box, seed, nbh=6, hsml_scatter=0.5, ngarbage=40):
    """A particle table for the tests: gas (type 0) first, then DM (type 1), then `nbh` black holes (type 5) at DM-like places; random
    velocities and accelerations, mixed gravity time bins, smoothing lengths scattered around the value that encloses ~40 DM particles
    at mean density, black-hole Hsml from a few to a few hundred DM neighbours, lognormal gas densities, and `ngarbage` garbage /
    swallowed rows (type 7) spread over gas, DM and black holes.  Returns a dict of arrays in particle order."""
    rng = np.random.RandomState(seed)
    ng, nd = len(pos_gas), len(pos_dm)
    bh_at = rng.choice(nd, nbh, replace=False)
    pos_bh = np.mod(pos_dm[bh_at] + 1e-3 * box * rng.standard_normal((nbh, 3)), box)
    pos = np.ascontiguousarray(np.concatenate([pos_gas, pos_dm, pos_bh]))
    pos[pos <= 0] += box
    n = len(pos)
    ptype = np.concatenate([np.zeros(ng, np.uint8), np.ones(nd, np.uint8), np.full(nbh, 5, np.uint8)])
    h40 = (3 * 40 / (4 * np.pi * nd)) ** (1. / 3) * box
    hsml = h40 * np.exp(hsml_scatter * rng.standard_normal(n))
    hsml[ng + nd:] = h40 * np.array([0.6, 0.9, 1.3, 1.7, 2.0, 2.2, 0.5, 1.1][:nbh])       # ~9 .. ~430 neighbours at mean density
    d = dict(pos=pos, type=ptype, box=float(box), n=n, ng=ng, nd=nd, nbh=nbh,
             vel=100.0 * rng.standard_normal((n, 3)), gacc=30.0 * rng.standard_normal((n, 3)), gpm=20.0 * rng.standard_normal((n, 3)),
             tb_grav=rng.randint(20, 27, n).astype(np.uint8), hsml=hsml, dthsml=0.05 * hsml * rng.standard_normal(n),
             density=np.exp(rng.standard_normal(n)), mass=np.ones(n, np.float32))
    dead = np.concatenate([rng.choice(ng, ngarbage // 2, replace=False), ng + rng.choice(nd, ngarbage // 2, replace=False), [n - 1]])
    d["dead"] = dead
    d["type_table"] = ptype.copy()     # the types as the particle table holds them; the dead rows carry IsGarbage (the last one: Swallowed)
    d["type"][dead] = 7
    return d


def sample_times(seed):
    """kick factors per gravity bin (DM_VelPred) and the scalars of a call"""
    rng = np.random.RandomState(seed + 1000)
    return dict(gravkicks=0.01 * rng.random_sample(47), FgravkickB=0.004, Time=0.25, hubble=0.8, ddrift=0.3)
