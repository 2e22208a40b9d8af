"""Extended-precision restatement of the excursion-set reionisation model - calculate_uvbg (libgadget/uvbg.c:471-594) through petapm_reion
(petapm.c:381-577) - for one rank that holds the whole mesh, and the scenes its tests share.  Not a test module: imported by
test_uvbg_restated.py (the conditions the scenes must meet, the host-side rules) and test_gpu_uvbg.py (the HIP path against it).

Written from uvbg.c / petapm.c line by line; it shares no code with the engine.  Cells, corners and the deposit are pm_restated.py's (the
cell of a row is the one fp64 decision, as there); everything else is numpy.longdouble, the transforms included, except what the reference
itself keeps in float: the grids J21 / xHI and J21_aux.  `float_filter=True` evaluates the real-space top hat the reference's way
(sinf / cosf / powf of the double kR), which is the one defined numerical difference of the engine (fp64 there).

Besides the results, run() returns per cell the smallest |f_coll eff - 1| over the radii (`margin`: a decision nearer to the barrier than
the arithmetic resolves is no decision) and the cells whose clamped mass falls below 1e-9 of the mean cell mass at some radius
(`degenerate`: the quotient star / mass is rounding noise there, in the reference as well)."""
import functools

import numpy as np

import pm_restated as PM

LD = np.longdouble
PI = PM.PI
# physconst.h
SOLAR_MASS, PLANCK, PROTONMASS, SEC_PER_YEAR, HYDROGEN_MASSFRAC = 1.989e33, 6.6262e-27, 1.6726e-24, 3.155e7, 0.76
FLOAT_REL_TOL = np.float32(1e-5)          # uvbg.c:30
MAX_R_ITERATIONS = 10000                  # petapm.c:410
M_E = 2.718281828459045                   # math.h's double

PAR = dict(ReionFilterType=0, RtoMFilterType=0, ReionRBubbleMax=3000.0, ReionRBubbleMin=100.0, ReionDeltaRFactor=1.1,
           ReionNionPhotPerBary=4000.0, AlphaUV=3.0, EscapeFractionNorm=0.3, EscapeFractionScaling=0.5, ReionUseParticleSFR=0,
           ReionSFRTimescale=0.5, UVBGdim=16, Time=0.125, Omega0=0.2814, OmegaBaryon=0.0464, RhoCrit=2.77536627e-8, HubbleParam=0.697,
           hubble=1.3e-3, UnitLength_in_cm=3.085678e21, UnitMass_in_g=1.989e43, UnitTime_in_s=3.08568e16, NTask=1)


def radii(R_max, R_min, R_delta, box, dim):
    """the loop of petapm_reion_c2r (petapm.c:426-499) in its own fp64 operations -> the radii, the last one the unfiltered step"""
    R_max, R_min, R_delta, box = float(R_max), float(R_min), float(R_delta), float(box)
    cell = box / dim                                                      # petapm.c:112
    R, last, count, out = min(R_max, box), False, 0, []
    while not last:
        count += 1
        if R / R_delta < R_min or R / R_delta < cell or count > MAX_R_ITERATIONS:
            last, R = True, cell
        out.append(R)
        R = R / R_delta
    return out


def init_particles(ptype, escfrac, par):
    """init_particle_uvbg (uvbg.c:471-504) -> escfrac in long double; gas rows keep the halo mass unless ReionUseParticleSFR (the continue)"""
    conv = LD(par["UnitMass_in_g"]) / LD(SOLAR_MASS) / LD(1e10) / LD(par["HubbleParam"])
    out = np.asarray(escfrac, np.float64).astype(LD)
    for i in range(len(out)):
        if ptype[i] == 0:
            if not par["ReionUseParticleSFR"] or out[i] == 0:
                continue
        elif ptype[i] == 4:
            if out[i] == 0:
                continue
        else:
            continue
        f = LD(par["EscapeFractionNorm"]) * np.power(out[i] * conv, LD(par["EscapeFractionScaling"]))
        if f > 1:
            f = LD(1)
        if f < 0:
            raise ValueError("negative escape fraction?")
        out[i] = f
    return out


def zreion_rule(zreion, took, time):
    """readout_J21 (uvbg.c:462-468): 1 / Time - 1 where the row took a value and zreion was -1"""
    z = np.array(zreion, np.float64)
    z[took & (z == -1)] = 1 / float(time) - 1
    return z


def _filter(k2, box, dim, R, ftype, float_filter):
    """filter_pm (uvbg.c:215-248) as a factor on the rfft mesh; None where the k-space top hat zeroes the mode"""
    k_mag64 = np.sqrt(k2.astype(np.float64)) * (2 * np.pi / dim) * (dim / float(box))     # the reference's fp64 operations ...
    kR64 = k_mag64 * float(R)
    kR = np.sqrt(k2.astype(LD)) * (2 * PI / LD(dim)) * (LD(dim) / LD(box)) * LD(R)
    if ftype == 0:
        W = np.ones(k2.shape, LD)
        on = kR64 > 1e-4
        if float_filter:
            k = kR64[on].astype(np.float32)                                                # sinf(double) converts its argument
            W[on] = LD(3) * (np.sin(k) / np.power(k, np.float32(3)) - np.cos(k) / np.power(k, np.float32(2))).astype(LD)
        else:
            k = kR[on]
            W[on] = LD(3) * (np.sin(k) / k ** 3 - np.cos(k) / k ** 2)
        return W
    if ftype == 1:
        return np.where(kR64 * 0.413566994 > 1, LD(0), LD(1))                              # ... decide the cut
    if ftype == 2:
        k = kR * LD(0.643)
        return np.power(LD(M_E), -k * k / LD(2))
    raise ValueError("ReionFilterType type %d is undefined!" % ftype)


def _rtom(R, par):
    R = LD(R)
    if par["RtoMFilterType"] == 0:
        return LD(4) / LD(3) * PI * R ** 3 * (LD(par["Omega0"]) * LD(par["RhoCrit"]))
    if par["RtoMFilterType"] == 1:
        return np.power(2 * PI, LD(1.5)) * LD(par["Omega0"]) * LD(par["RhoCrit"]) * R ** 3
    raise ValueError("Unrecognised RtoM filter (%d)." % par["RtoMFilterType"])


def max_of_corners(J21, pos, box, dim):
    """the largest J21 among the 8 CIC corners of every row, whatever the weights (J21: float32 [dim, dim, dim]) -> float64"""
    ic, res = PM.cells(pos, box, dim)
    flat = np.asarray(J21).reshape(-1)
    best = np.full(len(ic), -np.inf)
    for lin, _ in PM._corners(ic, res, dim):
        best = np.maximum(best, flat[lin].astype(np.float64))
    return best


def run(S, float_filter=False, precision="ld"):
    """steps 1 - 6 of calculate_uvbg on the scene S (dict: pos, mass, type, sfr, escfrac, zreion, box, par).  precision "f64" runs the same
    statements in fp64 (what a line-by-line fp64 implementation decides)."""
    T = LD if precision == "ld" else np.float64
    par, box = S["par"], S["box"]
    dim, use_sfr = par["UVBGdim"], bool(par["ReionUseParticleSFR"])
    ptype = np.asarray(S["type"])
    n = len(ptype)
    out = dict(radii=radii(par["ReionRBubbleMax"], par["ReionRBubbleMin"], par["ReionDeltaRFactor"], box, dim))
    # 1. init_particle_uvbg
    fesc = init_particles(ptype, S["escfrac"], par)
    out["escfrac"] = fesc
    # 2. the deposits (rows of type 7 deposit nothing: the engine's convention)
    live = ptype != 7
    mass = np.asarray(S["mass"]).astype(LD)
    dep = [PM.cic_deposit_ld(S["pos"], mass, box, dim, live),
           PM.cic_deposit_ld(S["pos"], np.where(ptype == 4, mass * fesc, LD(0)), box, dim, live)]
    if use_sfr:
        dep.append(PM.cic_deposit_ld(S["pos"], np.where(ptype == 0, np.asarray(S["sfr"], np.float64).astype(LD) * fesc, LD(0)), box, dim, live))
    out["deposit"] = dep
    # 3. forward transforms, divided by the number of cells
    ncell = T(dim) ** 3
    spec = [np.fft.rfftn(g.astype(T)) / ncell for g in dep]
    KX, KY, KZ = PM._mode_numbers(dim)
    k2 = KX * KX + KY * KY + KZ * KZ
    # constants of reion_loop_pm (uvbg.c:330-371)
    redshift = T(1) / T(par["Time"]) - 1
    Y_He = T(1) - T(HYDROGEN_MASSFRAC)
    eff = T(1) / (T(par["OmegaBaryon"]) / T(par["Omega0"])) * T(par["ReionNionPhotPerBary"]) / (T(1) - T(0.75) * Y_He)
    cell = T(box) / T(dim)
    pixel_volume = cell ** 3
    deltax_conv = ncell / (T(par["RhoCrit"]) * T(par["Omega0"]) * T(box) ** 3)
    hubble_time = 1 / (T(par["hubble"]) * T(par["HubbleParam"]))
    UL, UM, UT = T(par["UnitLength_in_cm"]), T(par["UnitMass_in_g"]), T(par["UnitTime_in_s"])
    pi = T(PI)
    J21 = np.zeros((dim,) * 3, np.float32)
    xHI = np.ones((dim,) * 3, np.float32)
    margin = np.full((dim,) * 3, np.inf)
    degenerate = np.zeros((dim,) * 3, bool)
    first = np.full((dim,) * 3, -1)
    mean_mass = float(dep[0].sum()) / dim ** 3
    # 4. the radius loop
    for step, R in enumerate(out["radii"]):
        last = step + 1 == len(out["radii"])
        W = None if last else _filter(k2, box, dim, R, par["ReionFilterType"], float_filter).astype(T)
        real = [np.fft.irfftn(s if last else s * W, s=(dim,) * 3, axes=(0, 1, 2)) * ncell for s in spec]
        assert real[0].dtype == T
        m, st = np.maximum(real[0], 0), np.maximum(real[1], 0)
        Rt = T(R)
        J21c = (1 + redshift) * (1 + redshift) / (4 * pi) * T(par["AlphaUV"]) * T(PLANCK) * T(1e21) * Rt * UL * T(par["ReionNionPhotPerBary"]) \
            / T(PROTONMASS) * UM / UL ** 3 / UT
        with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
            dom = m * deltax_conv
            fcoll = st / (T(_rtom(R, par)) * dom) * (T(4) / T(3)) * pi * Rt * Rt * Rt / pixel_volume
            if use_sfr:
                sfrd = np.maximum(real[2], 0) / pixel_volume / (UM / T(SOLAR_MASS)) * (UT / T(SEC_PER_YEAR))
            else:
                sfrd = st / (T(par["ReionSFRTimescale"]) * hubble_time) / pixel_volume
            J21_aux = (sfrd * J21c).astype(np.float32)
            ion = fcoll > 1 / eff                                          # (a NaN does not ionise, an infinity does)
            dist = np.abs((fcoll * eff).astype(np.float64) - 1)
        margin = np.where(np.isnan(dist), margin, np.minimum(margin, dist))
        degenerate |= ~(m.astype(np.float64) >= 1e-9 * mean_mass)
        crossing = ion & (xHI > FLOAT_REL_TOL)
        J21[crossing] = J21_aux[crossing]
        first[crossing] = step
        xHI[ion] = 0
        if last:
            part = ~ion & (xHI > FLOAT_REL_TOL)
            with np.errstate(invalid="ignore", over="ignore"):
                xHI[part] = (1 - fcoll * eff)[part].astype(np.float32)
            # 5. the neutral fractions (uvbg.c:423-448)
            x = xHI.astype(T)
            out["volume_weighted_global_xHI"] = x.sum() / dim ** 3
            out["mass_weighted_global_xHI"] = (x * dom).sum() / dom.sum()
    out.update(J21=J21, xHI=xHI, margin=margin, degenerate=degenerate, first_crossing=first)
    # 6. readout_J21
    gas = ptype == 0
    lj = np.zeros(n)
    best = max_of_corners(J21, S["pos"], box, dim)
    took = gas & (best > 0)
    lj[took] = best[took]
    out["local_J21"] = lj
    out["zreion"] = zreion_rule(S["zreion"], took, par["Time"])
    return out


# ------------------------------------------------------------------------------------------------------------------ scenes
SCENES = ("d16", "d24", "void")


def scene(name, **over):
    """A seeded scene: a jittered grid of dim^3 rows of types 1 and 0, about 300 stars in four clumps with halo masses in their escfrac
    (some 0: outside every group; some large: the clamp at 1), rows up to 3 boxes outside [0, Box), rows exactly on cell faces, rows of type
    7 (heavy: they would show if deposited), gas with zreion already set.  "void" empties one octant.  `over`: members of par replaced."""
    dim = dict(d16=16, d24=24, void=16)[name]
    rng = np.random.RandomState(dict(d16=3, d24=5, void=7)[name])
    box = 10000.0
    cell = box / dim
    g = (np.indices((dim,) * 3).reshape(3, -1).T + 0.5) * cell
    pos = (g + rng.normal(0, 0.3 * cell, g.shape)) % box
    ptype = np.where(rng.random_sample(len(pos)) < 0.75, 0, 1).astype(np.uint8)
    if name == "void":
        keep = ~np.all(pos < 0.5 * box, axis=1)
        pos, ptype = pos[keep], ptype[keep]
    mass = 0.5 * rng.uniform(0.9, 1.1, len(pos))
    nstar = 300
    centres = rng.uniform(0.55 * box, 0.95 * box, (4, 3)) if name == "void" else rng.uniform(0, box, (4, 3))
    sp = (centres[rng.randint(0, 4, nstar)] + rng.normal(0, 1.2 * cell, (nstar, 3))) % box
    sm = rng.uniform(0.5, 1.5, nstar) * dict(d16=1e-4, d24=2e-4, void=1e-4)[name]   # (3 - 10 % of the cells ionise with the default filters)
    pos = np.concatenate([pos, sp])
    ptype = np.concatenate([ptype, np.full(nstar, 4, np.uint8)])
    mass = np.concatenate([mass, sm])
    n = len(pos)
    # rows exactly on cell faces; rows outside the box by up to 3 boxes
    face = rng.choice(n, 40, replace=False)
    pos[face] = np.round(pos[face] / cell) * cell
    out = rng.choice(n, 60, replace=False)
    pos[out] += rng.randint(-3, 4, (60, 3)) * box
    # rows of type 7: heavy stale rows
    ndead = 25
    pos = np.concatenate([pos, rng.uniform(0, box, (ndead, 3))])
    ptype = np.concatenate([ptype, np.full(ndead, 7, np.uint8)])
    mass = np.concatenate([mass, np.full(ndead, 50.0)])
    n = len(pos)
    perm = rng.permutation(n)
    pos, ptype, mass = pos[perm], ptype[perm], mass[perm].astype(np.float32)
    # the halo mass of fof_set_escapefraction: 0 outside every group, else log-uniform in [1e-2, 1e2] (the upper end clamps at 1)
    halo = np.where(rng.random_sample(n) < 0.15, 0.0, 10 ** rng.uniform(-2, 2, n))
    halo[(ptype != 0) & (ptype != 4)] = 123.25          # never read nor written
    # every gas row forms stars: a cell without any SFR deposit would hold rounding noise of the transforms after the unfiltered step, and
    # its J21 nothing to compare (test_uvbg_restated.py holds the fp64 statements to a float ulp of these J21 to show there is none)
    sfr = np.where(ptype == 0, rng.uniform(2e-4, 2e-3, n), 7.5)
    gas = np.nonzero(ptype == 0)[0]
    zreion = np.full(n, -1.0)
    zreion[gas[::7]] = 9.5                               # gas reionised earlier
    zreion[ptype != 0] = -3.0                            # never read nor written
    par = dict(PAR, UVBGdim=dim)
    par.update(over)
    return dict(name=name, pos=pos, mass=mass, type=ptype, sfr=sfr, escfrac=halo, zreion=zreion, box=box, par=par, n=n)


@functools.lru_cache(maxsize=None)
def reference(name, ftype=0, rtom=0, use_sfr=0, float_filter=False, precision="ld"):
    """run() of a named scene under the given filter types, computed once and shared (do not modify the result)"""
    return run(scene(name, ReionFilterType=ftype, RtoMFilterType=rtom, ReionUseParticleSFR=use_sfr), float_filter, precision)
