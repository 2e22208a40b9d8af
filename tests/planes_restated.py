"""numpy restatement of the lensing potential planes (write_plane, libgadget/plane.c:572-683), written from the cited lines; the
reference's arithmetic in its order of operations wherever an integer (a pixel, a count) depends on it.  Not a test module: imported by
test_planes_host.py (closed forms) and test_gpu_planes.py (the HIP path)."""
import numpy as np

LIGHTCGS = 2.99792458e10     # physconst.h
CM_PER_KPC = 3.085678e21


# ---- the particle plane: cutPlaneGaussianGrid, lenstools.c:233-319 ---------------------------------------------------------------------
def linspace_ends(start, stop, num):
    """linspace, lenstools.c:39-44: step = (stop - start) / (num - 1), result[i] = start + i * step.  Returns what find_bin reads of it:
    bins[0] and width = bins[num - 1] - bins[0] (lenstools.c:69)."""
    start, stop = np.float64(start), np.float64(stop)
    step = (stop - start) / np.float64(num - 1)
    first = start + np.float64(0) * step
    last = start + np.float64(num - 1) * step
    return first, last - first


def wrap_particle(p, box):
    """lenstools.c:108-109: while(p > Box) p -= Box; while(p <= 0) p += Box (so 0 becomes Box and Box stays)"""
    p = np.array(p, np.float64)
    while True:
        m = p > box
        if not m.any():
            break
        p[m] -= box
    while True:
        m = p <= 0
        if not m.any():
            break
        p[m] += box
    return p


def find_bin(value, b0, width, resolution, L):
    """find_bin, lenstools.c:68-95; -1 where the reference returns -1"""
    rel = np.array(value, np.float64) - b0
    while True:
        m = rel < 0
        if not m.any():
            break
        rel[m] += L
    while True:
        m = rel >= L
        if not m.any():
            break
        rel[m] -= L
    iflt = rel / width * np.float64(resolution)
    idx = np.floor(iflt).astype(np.int64)
    ok = (rel < width) & (idx >= 0) & (idx < resolution)
    return np.where(ok, idx, -1)


def particle_is_active(flags, ptype, tracer):
    """lenstools_particle_is_active, lenstools.c:18-26 (Swallowed: bit 1 of the flags byte), and IsGarbage (bit 0), which the engine skips"""
    act = (np.asarray(flags) & 3) == 0
    if tracer:
        act &= np.asarray(ptype) != 2
    return act


def image_axes(normal):
    """projectDensity, lenstools.c:126-166: (row axis, column axis) of the particle plane"""
    return {0: (1, 2), 1: (0, 2), 2: (0, 1)}[normal]


def plane_pixels(pos, box, R, normal, center, thickness, left_corner=(0., 0., 0.), offset=(0., 0., 0.)):
    """grid3d_ngb, lenstools.c:97-124, for one plane: the flat pixel index row * R + col of every particle, -1 if it is not counted"""
    pos = np.asarray(pos, np.float64)
    p = np.empty_like(pos)
    for d in range(3):
        p[:, d] = wrap_particle(pos[:, d] - np.float64(offset[d]), box)              # :107-109
    idx = []
    for d in range(3):
        if d == normal:                                                              # lenstools.c:256-260, thickness_resolution = 1
            b0, w = linspace_ends(np.float64(center) - np.float64(thickness) / 2, np.float64(center) + np.float64(thickness) / 2, 2)
            idx.append(find_bin(p[:, d], b0, w, 1, box))
        else:
            b0, w = linspace_ends(left_corner[d], np.float64(left_corner[d]) + box, R + 1)
            idx.append(find_bin(p[:, d], b0, w, R, box))
    ok = (idx[0] >= 0) & (idx[1] >= 0) & (idx[2] >= 0)                                  # :116
    r, c = image_axes(normal)
    return np.where(ok, idx[r] * R + idx[c], -1)


def plane_counts(pos, box, R, normal, center, thickness, active=None, **kw):
    pix = plane_pixels(pos, box, R, normal, center, thickness, **kw)
    if active is not None:
        pix = pix[active]
    return np.bincount(pix[pix >= 0], minlength=R * R).reshape(R, R)


def lensing_potential(density, b0, b1, chi, smooth=1.0):
    """calculate_lensing_potential, lenstools.c:168-231, on a square image"""
    R = density.shape[0]
    i = np.arange(R)
    lx = np.where(i < R // 2, i, -(R - i)).astype(np.float64) / R                      # :186-187
    ly = np.arange(R // 2 + 1, dtype=np.float64) / R                                  # :188-189
    l2 = lx[:, None] ** 2 + ly[None, :] ** 2
    l2[0, 0] = 1.0                                                                    # :194
    ft = np.fft.rfft2(density)
    ft[0, 0] = 0.0                                                                    # :200-201
    factor = -2.0 * (b0 * b1 / (chi * chi)) / (l2 * 4 * np.pi * np.pi)                  # :207
    ft = ft * (factor * np.exp(-0.5 * ((2.0 * np.pi * smooth) * (2.0 * np.pi * smooth)) * l2))
    return np.fft.irfft2(ft, s=(R, R))           # (numpy's inverse divides by R^2: lenstools.c:217-221)


def normalisations(box, thickness, chi, atime, HubbleParam, omega_source):
    """cosmo_normalization * density_normalization, lenstools.c:248-249, 271"""
    H0 = 100 * HubbleParam * 3.2407793e-20
    cosmo = 1.5 * H0 ** 2 * omega_source / LIGHTCGS ** 2
    dens = thickness * chi * (CM_PER_KPC / HubbleParam) ** 2 / atime
    return cosmo * dens


def potential_from_counts(counts, n_active_total, box, thickness, chi, atime, HubbleParam, omega_source):
    """lenstools.c:287-311: counts -> density contrast -> potential; a plane without particles stays zero"""
    R = counts.shape[0]
    b = box / R
    if counts.sum() <= 0:
        return np.zeros((R, R))
    f = 1. / n_active_total * (box ** 3 / (b * b * thickness))                         # :292
    return lensing_potential(counts.astype(np.float64) * f, b, b, chi) * normalisations(box, thickness, chi, atime, HubbleParam, omega_source)


def resolve(box, Thickness, CutPoints):
    """plane.c:581-591"""
    th = Thickness if Thickness > 0 else box
    if CutPoints is None or len(CutPoints) == 0:
        CutPoints = [(.5 + i) * th for i in range(int(box / th))]
    return th, list(CutPoints)


# ---- the massive-neutrino correction: plane.c:313-478 -----------------------------------------------------------------------------------
def wrap_position(x, L):
    """plane_wrap_position, plane.c:57-63"""
    x = np.array(x, np.float64)
    while (x < 0).any():
        x[x < 0] += L
    while (x >= L).any():
        x[x >= L] -= L
    return x


def correction_mesh(pos, mass, active, box, nmesh, bmpc, response, offset=(0., 0., 0.)):
    """plane_pm_grid_init_neutrino_correction, plane.c:313-351: (the unnormalised c2r output, total mass, what the callback received)"""
    from oracle import oracle as O
    from test_gpu_nu_response import _nufac, _spectrum
    p = wrap_position(np.asarray(pos, np.float64)[active] - np.asarray(offset, np.float64)[None, :], box)     # plane.c:103
    m = np.asarray(mass)[active]
    rho_k = np.fft.rfftn(O.pm_cic_deposit(p, m, box, nmesh))
    kk, P, N = _spectrum(rho_k, nmesh, bmpc)
    inputs = (kk, np.sqrt(P), N)                                                       # plane.c:279-283
    lk, rt, pf, _ = response(*inputs)
    fac = _nufac(nmesh, bmpc, np.asarray(lk), np.asarray(rt), pf) - 1                  # plane.c:301-310
    fac[0, 0, 0] = 0.0                                                                # plane.c:294-298
    real = np.fft.irfftn(rho_k * fac, s=(nmesh,) * 3, axes=(0, 1, 2)) * float(nmesh) ** 3
    return real, m.astype(np.float64).sum(), inputs


def slab_overlap(cell_start, cellsize, center, thickness, L):
    """plane_periodic_slab_overlap, plane.c:369-387"""
    if thickness >= L:
        return cellsize
    c = float(wrap_position([center], L)[0])
    slab_start = c - 0.5 * thickness
    slab_end = slab_start + thickness
    cell_end = cell_start + cellsize
    overlap = 0.0
    for shift in (-1, 0, 1):
        off = shift * L
        lo, hi = max(cell_start, slab_start + off), min(cell_end, slab_end + off)
        overlap += hi - lo if hi > lo else 0.0
    return overlap


def correction_plane(real, total_mass, box, normal, center, thickness, chi, atime, HubbleParam, omega_source):
    """cutPlanePMNeutrinoCorrection, plane.c:389-445: an Nmesh^2 image with the axes plane_directions[] = (normal + 1) % 3,
    (normal + 2) % 3 - for normal 1 that is (z, x), not the particle plane's (x, z)"""
    nmesh = real.shape[0]
    cellsize = box / nmesh
    ov = np.array([slab_overlap(k * cellsize, cellsize, center, thickness, box) for k in range(nmesh)])
    w = np.where(ov > 0, ov, 0.0) / thickness
    delta = real * (1.0 / float(nmesh) ** 3) / (total_mass / float(nmesh) ** 3)        # plane.c:420
    shape = [1, 1, 1]
    shape[normal] = nmesh
    proj = (delta * w.reshape(shape)).sum(axis=normal)       # axes left in increasing order
    if normal == 1:
        proj = proj.T                                        # (x, z) -> (z, x), plane.c:399, 421-425
    return lensing_potential(proj, cellsize, cellsize, chi) * normalisations(box, thickness, chi, atime, HubbleParam, omega_source)


def bilinear_add(dst, src):
    """plane_add_periodic_bilinear, plane.c:447-478 (returns dst + the resampled src)"""
    dn, sn = dst.shape[0], src.shape[0]
    x = ((np.arange(dn) + 0.5) * sn / dn) - 0.5
    i0 = np.floor(x).astype(np.int64)
    t = x - i0
    i0 = i0 % sn
    i1 = (i0 + 1) % sn
    tx, ty = t[:, None], t[None, :]
    I0, I1, J0, J1 = i0[:, None], i1[:, None], i0[None, :], i1[None, :]
    return dst + ((1 - tx) * (1 - ty) * src[I0, J0] + tx * (1 - ty) * src[I1, J0] + (1 - tx) * ty * src[I0, J1] + tx * ty * src[I1, J1])


# ---- write_plane's loop, plane.c:576-668 --------------------------------------------------------------------------------------------------
def potential_planes(pos, box, Resolution, Normals, atime, comoving_distance, HubbleParam, omega_source, Thickness=0.0, CutPoints=None,
                     left_corner=(0., 0., 0.), CurrentParticleOffset=(0., 0., 0.), flags=None, ptype=None, tracer=False, mass=None,
                     nu_response=None, nmesh=0, BoxSize_in_MPC=0.0, ranks=1, parts=None):
    """Returns a dict: planes[ncuts][nnormals][R][R], npart, counts (int64, same shape as planes), n_active, and with a correction
    `correction` (the resampled correction alone, same shape) and `inputs` (what the callback received).  ranks > 1: the rows are dealt
    to `ranks` ranks, each counts its own, and the integer counts are summed before the one solve (the rank sum of the several-GPU
    form; the reference sums the ranks' finished potentials, plane.c:654, which is the same plane because the solve is linear)."""
    pos = np.asarray(pos, np.float64)
    n = len(pos)
    flags = np.zeros(n, np.uint8) if flags is None else np.asarray(flags)
    ptype = np.ones(n, np.uint8) if ptype is None else np.asarray(ptype)
    act = particle_is_active(flags, ptype, tracer)
    th, cuts = resolve(box, Thickness, CutPoints)
    R = Resolution
    shape = (len(cuts), len(Normals), R, R)
    out = dict(planes=np.zeros(shape), counts=np.zeros(shape, np.int64), npart=np.zeros(shape[:2], np.int64), n_active=int(act.sum()))
    if parts is None:
        parts = [np.arange(n)[r::ranks] for r in range(ranks)]
    if nu_response is not None:
        real, total_mass, out["inputs"] = correction_mesh(pos, mass, act, box, nmesh, BoxSize_in_MPC, nu_response, CurrentParticleOffset)
        out["correction"] = np.zeros(shape)
    for i, cut in enumerate(cuts):
        for j, normal in enumerate(Normals):
            c = np.zeros((R, R), np.int64)
            for rows in parts:
                c += plane_counts(pos[rows], box, R, normal, cut, th, active=act[rows], left_corner=left_corner, offset=CurrentParticleOffset)
            out["counts"][i, j] = c
            out["npart"][i, j] = c.sum()
            out["planes"][i, j] = potential_from_counts(c, out["n_active"], box, th, comoving_distance, atime, HubbleParam, omega_source)
            if nu_response is not None:
                corr = correction_plane(real, total_mass, box, normal, cut, th, comoving_distance, atime, HubbleParam, omega_source)
                out["correction"][i, j] = bilinear_add(np.zeros((R, R)), corr)
                out["planes"][i, j] = bilinear_add(out["planes"][i, j], corr)
    return out
