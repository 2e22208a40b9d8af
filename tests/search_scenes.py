"""Scenes that force the shared neighbour search (csrc/ngb_walk.h) through the control paths the gentle sets of the parity tests never
provably reach, and the all-pairs references they are judged against.  Test infrastructure (tests/test_search_scenes.py asserts, on the
reference side only, the conditions that make each scene mean what it claims; tests/test_gpu_search_edges.py runs the kernels).

Every scene is deterministic and small (<= 4159 particles); Box = 8 (a power of two: the cells of the tree are dyadic).  Builders are
cached: a scene and its references are computed once per process and shared, and nobody writes into them.

  A  clump          1280 particles Gaussian (sigma 0.03 Box) about the centre + 765 uniform, N = 2045 (a ragged last wave), Hsml = 0.2 Box
                    for all: a clump target has > 8 x SPH_LCAP = 960 neighbours, so its leaf list MUST fill and the walk pause and resume;
                    the box holds waves on both sides of interior_wave's geometry.
  B  mixed radii    A's positions, Hsml = 1.0001 x the distance to the k-th neighbour, k log-uniform in [12, 400], capped at 0.24 Box; then
                    4 particles at 0.45 Box and 2 at 0.7 Box: radii of ratio >= 30, hydro pairs that exist only through the neighbour's
                    radius, radii >= Box / 4 and >= Box / 2.
  C  starved gas    40 gas + 500 dark matter, uniform: no radius gives the desired neighbour number, the iteration runs Hsml to Box.
  FOF (i)           A's clump as primaries, the background inert, 64 gas particles 0.1 - 0.3 Box from the centre with Hsml = 0.4 Box.
  FOF (ii)          serpentine chain: every link is the only one between its two sides; IDs on both sides of 2^63.
  FOF (iii)         lattice whose six nearest neighbours sit at r^2 == LL^2 exactly.
"""
import functools

import numpy as np

from sph_paper import paper_density, paper_hydro

BOX = 8.0
SPH_LCAP = 120          # csrc/ngb_walk.h: leaf entries per group; one entry holds at most 8 particles
CHUNK = 256             # targets per block of the all-pairs references (256 x 2045 x 3 doubles = 12.6 MB per array)
ATIME, HUBBLE, DLOGA, ALPHA = 0.5, 0.3, 0.02, 0.75


def _frozen(d):
    for v in d.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return d


def all_pairs_r(pos, box):
    """|x_i - x_j| on the nearest image, dense [N, N]"""
    r2 = np.zeros((len(pos), len(pos)))
    for k in range(3):
        d = pos[:, None, k] - pos[None, :, k]
        d -= box * np.rint(d / box)
        r2 += d * d
    return np.sqrt(r2)


def interior_geometry(pos, radius, box):
    """interior_wave's condition (ngb_walk.h) for one target: radius < Box / 4 and farther than radius + Box / 500 from every face"""
    face = radius + 0.002 * box
    return (radius < 0.25 * box) & (pos.min(1) >= face) & (pos.max(1) <= box - face)


def _gas_fields(N, seed):
    """random velocities, entropies in [1, 1.5], masses scattered by 20 % (as gas_state of test_hydro_physics.py)"""
    rng = np.random.RandomState(seed)
    mass = ((BOX ** 3 / N) * (1.0 + 0.2 * rng.random_sample(N))).astype(np.float32)
    vel = 0.6 * rng.standard_normal((N, 3))
    ent = 1.0 + 0.5 * rng.random_sample(N)
    return mass, vel, ent


@functools.lru_cache(None)
def scene_a():
    rng = np.random.RandomState(11)
    nclump, nback = 1280, 765
    clump = 0.5 * BOX + 0.03 * BOX * rng.standard_normal((nclump, 3))
    back = BOX * rng.random_sample((nback, 3))
    pos = np.ascontiguousarray(np.vstack([clump, back]))
    N = len(pos)
    isclump = np.arange(N) < nclump
    # interleave clump and background in caller order (the tree sorts them anyway; the caller's order must not matter)
    perm = rng.permutation(N)
    pos, isclump = np.ascontiguousarray(pos[perm]), isclump[perm]
    mass, vel, ent = _gas_fields(N, 12)
    return _frozen(dict(name="A", pos=pos, box=BOX, hsml=np.full(N, 0.2 * BOX), clump=isclump, mass=mass, vel=vel, ent=ent,
                        r=all_pairs_r(pos, BOX)))


@functools.lru_cache(None)
def scene_b():
    A = scene_a()
    pos, r = A["pos"], A["r"]
    N = len(pos)
    rng = np.random.RandomState(13)
    k = np.exp(rng.uniform(np.log(12.0), np.log(400.0), N)).astype(np.int64)
    rk = np.sort(r, axis=1)[np.arange(N), k]            # column 0 is the particle itself: column k is its k-th neighbour
    hsml = np.minimum(1.0001 * rk, 0.24 * BOX)
    big = rng.choice(N, 6, replace=False)
    hsml[big[:4]] = 0.45 * BOX
    hsml[big[4:]] = 0.7 * BOX
    mass, vel, ent = _gas_fields(N, 14)
    return _frozen(dict(name="B", pos=pos, box=BOX, hsml=hsml, clump=A["clump"], mass=mass, vel=vel, ent=ent, r=r, big=big))


@functools.lru_cache(None)
def scene_c():
    rng = np.random.RandomState(17)
    ngas, ndm = 40, 500
    N = ngas + ndm
    pos = np.ascontiguousarray(BOX * rng.random_sample((N, 3)))
    typ = np.ones(N, np.int32)
    typ[rng.choice(N, ngas, replace=False)] = 0
    mass, vel, ent = _gas_fields(N, 18)
    return _frozen(dict(name="C", pos=pos, box=BOX, typ=typ, mass=mass, vel=vel, ent=ent, hsml0=np.full(N, 0.3 * BOX)))


_C_ORACLE = {}


def scene_c_oracle(orc):
    """The CPU restatement's density() on scene C from Hsml = 0.3 Box, quintic spline: (SphArrays, (passes, targets, interactions,
    candidates)).  Computed once per oracle."""
    if id(orc) not in _C_ORACLE:
        from oracle import oracle as O
        Cs = scene_c()
        N = len(Cs["pos"])
        dp = O.DensityParams(1.0, 2.0, 2.0, 99999., 2, 0.006)
        O.sph_set_softening(orc, 1e-3)
        A = O.SphArrays(Cs["pos"].copy(), Cs["mass"].copy(), type=Cs["typ"].copy(), hsml=Cs["hsml0"], vel=Cs["vel"].copy(),
                        entropy=Cs["ent"].copy())
        to = O.sph_times(atime=ATIME, hubble=HUBBLE, dloga_bin=[DLOGA] + [0.0] * 46)
        tr = orc.tree(A.pos, A.mass, BOX, type=A.type, hsml=A.hsml, hydro_active=np.ones(N, np.uint8), mask=1, moments=False)
        so = O.sph_density(orc, tr, dp, A, to)
        _C_ORACLE[id(orc)] = (A, tuple(int(x) for x in so))
    return _C_ORACLE[id(orc)]


KERNEL_NAMES = {1: "cubic", 2: "quintic", 4: "quartic"}
# (scene, kernel of sph_paper's numbering, formulation): the cases of the GPU test
SPH_CASES = [("A", 2, "density"), ("A", 1, "pressure"), ("B", 4, "density"), ("B", 2, "pressure")]


def scene(name):
    return {"A": scene_a, "B": scene_b, "C": scene_c}[name]()


@functools.lru_cache(None)
def reference(name, kernel, formulation):
    """paper_density then paper_hydro of the scene at its prescribed radii, every particle a target, in blocks of CHUNK targets"""
    S = scene(name)
    N = len(S["pos"])
    ref = paper_density(S["pos"], S["mass"], S["vel"], S["ent"], S["hsml"], S["box"], kernel, formulation, chunk=CHUNK)
    ref.update(paper_hydro(S["pos"], S["mass"], S["vel"], S["ent"], S["hsml"], S["box"], ref, ATIME, HUBBLE, ALPHA, kernel, formulation,
                           dlna=np.full(N, DLOGA), chunk=CHUNK))
    return _frozen(ref)


def radius_margin(r, radii):
    """The smallest | r_ij / R - 1 | over all pairs i != j and the radii R given per particle (tested as R_i and as R_j) or as scalars"""
    off = ~np.eye(len(r), dtype=bool)
    worst = np.inf
    for R in radii:
        R = np.asarray(R, float)
        if R.ndim == 0:
            worst = min(worst, np.abs(r[off] / R - 1).min())
        else:
            worst = min(worst, np.abs(r / R[:, None] - 1)[off].min(), np.abs(r / R[None, :] - 1)[off].min())
    return worst


# ---- friends of friends --------------------------------------------------------------------------------------------------------------
def link_pairs(pos, box, LL, sel=None):
    """Brute force: the pairs i < j (indices into pos) with r^2 <= LL^2 on the nearest image among the particles `sel` (None: all)."""
    idx = np.arange(len(pos)) if sel is None else np.flatnonzero(sel)
    p = pos[idx]
    ii, jj = [], []
    for a in range(0, len(p), 512):
        r2 = np.zeros((len(p[a:a + 512]), len(p)))
        for k in range(3):
            d = p[a:a + 512, None, k] - p[None, :, k]
            d -= box * np.rint(d / box)
            r2 += d * d
        i, j = np.nonzero(r2 <= LL * LL)
        keep = i + a < j
        ii.append(idx[i[keep] + a])
        jj.append(idx[j[keep]])
    return np.concatenate(ii), np.concatenate(jj)


def components(n, i, j):
    """Labels of the connected components of the graph with edges (i, j) on n vertices, no tree and no union-find of ours involved"""
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    g = coo_matrix((np.ones(len(i), np.int8), (i, j)), shape=(n, n))
    return connected_components(g, directed=False)[1]


def same_partition(a, b):
    """Do two label arrays describe the same partition?"""
    pairs = np.unique(np.stack([np.asarray(a, np.int64), np.unique(b, return_inverse=True)[1]], 1), axis=0)
    return len(np.unique(pairs[:, 0])) == len(pairs) == len(np.unique(pairs[:, 1]))


def secondary_radius(LL, hsml):
    """The radius at which a secondary particle's search for its nearest primary ends when nothing is found earlier (fof.c:1228-1250,
    1285-1293, float arithmetic as there): max(0.4 LL, Hsml / 2), doubled until it reaches 4 LL."""
    h = np.float32(0.4 * LL)
    if float(h) < 0.5 * hsml:
        h = np.float32(0.5 * hsml)
    while float(h) < 4 * LL:
        h = np.float32(h * np.float32(2.0))
    return float(h)


@functools.lru_cache(None)
def fof_scene_i(llfrac=0.2):
    """A's clump as type 1 (primary), its background type 2 (neither primary nor secondary: the clump is the tree), and 64 gas particles
    0.1 - 0.3 Box from the centre with Hsml = 0.4 Box.
    LL = 0.2 Box: every primary sees the whole clump (> 960 in its radius), and so does every gas particle - the first radius of its
    search is Hsml / 2 = 0.2 Box, the last 4 LL = 0.8 Box >= Box / 2.  One group: which primary a gas particle attaches to cannot show.
    LL = 0.02 Box (added to give the attachment teeth): the clump breaks into a core and many small groups and singles, the secondary
    search runs at Hsml / 2 = 0.2 Box (>= 4 LL) and the label a gas particle receives depends on WHICH primary is its nearest."""
    A = scene_a()
    rng = np.random.RandomState(19)
    ngas = 64
    u = rng.standard_normal((ngas, 3))
    u /= np.sqrt((u ** 2).sum(1))[:, None]
    gas = 0.5 * BOX + u * (BOX * rng.uniform(0.1, 0.3, ngas))[:, None]
    pos = np.ascontiguousarray(np.vstack([A["pos"], gas]))
    N = len(pos)
    typ = np.r_[np.where(A["clump"], 1, 2), np.zeros(ngas, np.int64)].astype(np.uint8)
    hsml = np.r_[np.zeros(len(A["pos"])), np.full(ngas, 0.4 * BOX)]
    ids = (rng.permutation(N) + 1000).astype(np.uint64)
    mass = np.where(typ == 0, 0.19, 0.81).astype(np.float32)
    vel = 30.0 * rng.standard_normal((N, 3))
    return _frozen(dict(pos=pos, box=BOX, LL=llfrac * BOX, typ=typ, hsml=hsml, ids=ids, mass=mass, vel=vel))


def nearest_primary(S):
    """Brute force: for every gas particle of a FOF scene the index of its nearest primary, the distance to it and to the second nearest"""
    prim, gas = np.flatnonzero(S["typ"] == 1), np.flatnonzero(S["typ"] == 0)
    d = S["pos"][gas][:, None, :] - S["pos"][prim][None, :, :]
    d -= S["box"] * np.rint(d / S["box"])
    r = np.sqrt((d ** 2).sum(-1))
    o = np.argsort(r, axis=1)
    k = np.arange(len(gas))
    return gas, prim[o[:, 0]], r[k, o[:, 0]], r[k, o[:, 1]]


CHAIN_ROWS, CHAIN_LEN = 64, 64


@functools.lru_cache(None)
def fof_scene_ii():
    """One polyline: 64 rows of 64 points at spacing 0.98 LL along x, consecutive rows 1.96 LL apart in y and joined at alternating ends
    through ONE joint particle half way (two steps of 0.98 LL).  Every link is the only connection between the two sides of the chain, so
    one lost union splits the group.  With the 63 joints flagged as garbage the rows are 64 groups of the same length 64 (one full wave of
    k_fof_accumulate), numbered by MinID alone.  N = 64 x 64 + 63 = 4159.  IDs: a random permutation shifted (mod 2^64) so that half of them
    are >= 2^63, one is 2^64 - 1 and the smallest is 0 - the signed minimum would be 2^64 - ceil(N / 2)."""
    LL = 2.0 ** -5
    s = 0.98 * LL
    rng = np.random.RandomState(23)
    pts, joint, row = [], [], []
    for k in range(CHAIN_ROWS):
        xs = np.arange(CHAIN_LEN) * s
        if k % 2:
            xs = xs[::-1]
        for x in xs:
            pts.append((x, 2 * k * s))
            joint.append(0)
            row.append(k)
        if k + 1 < CHAIN_ROWS:
            pts.append((xs[-1], (2 * k + 1) * s))
            joint.append(1)
            row.append(-1)
    xy = np.array(pts)
    N = len(xy)
    pos = np.empty((N, 3))
    pos[:, :2] = xy + 1.0          # away from the faces; extent 1.93 x 3.86 < Box / 2
    pos[:, 2] = 0.5 * BOX
    perm = rng.permutation(N)      # caller order unrelated to the order along the chain
    pos, joint, row = np.ascontiguousarray(pos[perm]), np.array(joint, np.uint8)[perm], np.array(row)[perm]
    half = (N + 1) // 2
    ids = rng.permutation(N).astype(np.uint64) + np.uint64(2 ** 64 - half)     # wraps mod 2^64
    return _frozen(dict(pos=pos, box=BOX, LL=LL, ids=ids, joint=joint, row=row, mass=np.full(N, 0.37, np.float32)))


@functools.lru_cache(None)
def fof_scene_iii():
    """16^3 particles at spacing exactly 0.5 in a box of 8 (the lattice fills the periodic box): with LL = 0.5 the six nearest neighbours
    of every particle sit at r^2 == LL^2 in exact arithmetic - linked by the inclusive test r2 <= h2 (treewalk.c:984-991), not by r2 < h2."""
    g = np.arange(16) * 0.5
    pos = np.ascontiguousarray(np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3))
    rng = np.random.RandomState(29)
    N = len(pos)
    return _frozen(dict(pos=pos, box=BOX, LL=0.5, ids=(rng.permutation(N) + 7).astype(np.uint64), mass=np.full(N, 0.37, np.float32)))
