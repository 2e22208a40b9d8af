"""The bucket oct-tree of libgadget/forcetree.c restated from its definition, in plain numpy, and the scenes that put the GPU build
(csrc/tree_build.hip) at the edges of its kernels.  Test infrastructure: no GPU, no oracle, and nothing of the kernels' method - no
sorted keys, no common-prefix lengths, no scans.  The tree is built by recursion over index sets.

What is taken in the code's own precision is the octant decision alone (as tests/pm_restated.py takes the CIC cell): the reference's
descent (forcetree.c:278-320) replayed for 21 levels in fp64, centre = Box / 2, len = 1.001 Box, bit = Pos > centre, centre +- 0.25 len,
len *= 0.5.  Everything else follows from the definition:
  node set   the root is a node; a non-empty cell is a node iff its parent is internal; a node at level l is internal iff it holds more
             than 8 particles or l < minlevel, else a leaf; more than 8 particles in a level-21 cell is the refusal (TreeRefusal)
  order      pre-order, children in octant order; `sibling` = the first node after the sub-tree, -1 when there is none
  moments    numpy.longdouble sums over the node's OWN particles (never over its children); the mass is a float32 widened
  hmax       fp64, as the reference writes it: fabs(Pos - centre) + Hsml - len / 2. against the faces of the particle's LEAF
             (forcetree.c:963), types 0 and 5 that are not hydro-active only, maximum with 0, carried up as a maximum (:1090).
             Additions only: the gate on it is bit-equality.
  level order  a stable sort of the pre-order nodes by level; per internal node its occupied octants (contiguous children), per leaf the
             three merge counts of NodeLinkB::firstchild (csrc/mpg_common.h), per leaf the padded block of 8 source records

The bound on the moments (gate_moments).  k_leaf_moments / k_internal_moments (and the reference, in another order) compute
    cofm = fl(sum m x) / fl(sum m).
A child's quotient is multiplied by the child's computed mass again one level up, so the mass roundings below a node cancel in the
numerator, and to first order  cofm_computed = [sum_i m_i x_i (1 + e_i)] / [sum_i m_i (1 + d_i)] (1 + one division), where e_i counts
the roundings the term m_i x_i meets on its way up and d_i those the mass m_i meets.  With u = 2^-53 per rounding and every partial sum
bounded by the sum of the absolute terms:
    leaf of p particles       numerator: 1 product + (p - 1) additions; mass: p - 1 additions; 1 division          -> 2 p
                              (p = 1: the reference divides m x by m, two roundings; the GPU build stores the position itself, which
                              gate_moments(exact_single=True) asserts to the bit on top of the bound)
    internal, c children      numerator: the child's division, 1 product, c - 1 additions; mass: c - 1 additions  -> + 2 c
so  kc(leaf) = 2 p,  kc(node) = max over children kc(child) + 2 c,  and  |cofm - ref| <= (kc + 1) u  sum m|x| / sum m  per component
(the + 1 covers the long-double reference and the second-order terms).  For the mass  km(leaf) = p - 1,  km(node) = max km(child) +
c - 1,  |M - ref| <= (km + 1) u ref.  At most 16 per level: 352 at the root of a 21-level tree; the counts are taken per node from the
tree itself, so a chain of one-child nodes costs 2 per level.
"""
import numpy as np

MAXLEVEL = 21
NMAXCHILD = 8
BOX = 10.0
U = 2.0 ** -53
FAULTS = ("ge", "direct_centre", "leaf9", "hmax_own_faces", "hmax_active", "sibling_last", "merge_one")


class TreeRefusal(Exception):
    """more than 8 particles in one level-21 cell (forcetree.c:393-412: the reference exhausts its node pool)"""


# ------------------------------------------------------------------------------------------------------------ octant paths
def octant_digits(pos, box, fault=None):
    """digits[i, l] = octant (x | y << 1 | z << 2) particle i takes at level l, l = 0 .. 20, by the reference's own descent in fp64"""
    pos = np.asarray(pos, np.float64).reshape(-1, 3)
    n = len(pos)
    c = np.full((n, 3), box / 2.)
    ln = box * 1.001
    ix = np.zeros((n, 3), np.int64)
    digits = np.zeros((n, MAXLEVEL), np.uint8)
    for l in range(MAXLEVEL):
        bit = (pos >= c) if fault == "ge" else (pos > c)
        digits[:, l] = bit[:, 0] | (bit[:, 1] << 1) | (bit[:, 2] << 2)
        if fault == "direct_centre":
            ix = 2 * ix + bit
            c = box / 2. + ((2 * ix + 1 - 2 ** (l + 1)) / 2.) * (0.5 * ln)
        else:
            c = c + np.where(bit, 0.25 * ln, -(0.25 * ln))
        ln = ln * 0.5
    return digits


def cell_of(p, box, level):
    """(centre[3], len) of the level-`level` cell around the point p, by the same accumulation"""
    c = np.full(3, box / 2.)
    ln = box * 1.001
    for _ in range(level):
        bit = np.asarray(p, np.float64) > c
        c = c + np.where(bit, 0.25 * ln, -(0.25 * ln))
        ln = ln * 0.5
    return c, ln


# ------------------------------------------------------------------------------------------------------------ the tree
def restate(pos, mass, box, members=None, minlevel=0, type=None, hsml=None, hact=None, fault=None):
    """The tree of the particles `members` (caller indices; None = all).  Returns a dict of arrays in pre-order (see below)."""
    assert fault is None or fault in FAULTS
    pos = np.ascontiguousarray(pos, np.float64).reshape(-1, 3)
    mass32 = np.asarray(mass, np.float32)
    members = np.arange(len(pos)) if members is None else np.sort(np.asarray(members, np.int64))
    digits = octant_digits(pos, box, fault)
    thr = 9 if fault == "leaf9" else NMAXCHILD
    direct = fault == "direct_centre"
    level, centre, lens, pcount, nbelow, parent, leafmem, allmem, children = [], [], [], [], [], [], [], [], []

    def rec(idx, l, c, ln, ixyz, par):
        j = len(level)
        internal = len(idx) > 0 and (len(idx) > thr or l < minlevel)
        level.append(l), centre.append(c), lens.append(ln), parent.append(par), nbelow.append(len(idx)), allmem.append(idx)
        pcount.append(0 if internal else len(idx)), leafmem.append(None if internal else idx), children.append([])
        if internal:
            if l >= MAXLEVEL:
                raise TreeRefusal("%d particles in one level-%d cell" % (len(idx), MAXLEVEL))
            d = digits[idx, l]
            for o in range(8):
                sub = idx[d == o]
                if len(sub) == 0:
                    continue
                sgn = np.array([1. if o & 1 else -1., 1. if o & 2 else -1., 1. if o & 4 else -1.])
                ic = 2 * ixyz + np.array([o & 1, (o >> 1) & 1, (o >> 2) & 1])
                cc = (box / 2. + ((2 * ic + 1 - 2 ** (l + 1)) / 2.) * (0.5 * ln)) if direct else c + sgn * (0.25 * ln)
                children[j].append(rec(sub, l + 1, cc, 0.5 * ln, ic, j))
        return j

    rec(members, 0, np.full(3, box / 2.), np.float64(box * 1.001), np.zeros(3, np.int64), -1)
    M = len(level)
    T = dict(box=float(box), n=len(members), level=np.array(level, np.int32), center=np.array(centre, np.float64).reshape(M, 3),
             len=np.array(lens, np.float64), pcount=np.array(pcount, np.int32), nbelow=np.array(nbelow, np.int64), parent=np.array(parent, np.int64),
             leafmem=leafmem, allmem=allmem, children=children, digits=digits, members=members)
    # particle ranges in tree order (the leaves' particles in pre-order) and `sibling`
    pstart = np.zeros(M, np.int32)
    run = 0
    for j in range(M):
        pstart[j] = run
        run += pcount[j]
    T["pstart"] = pstart
    sib = np.full(M, -1, np.int32)
    for j in range(M):
        ch = children[j]
        for a, c in enumerate(ch):
            sib[c] = ch[a + 1] if a + 1 < len(ch) else (ch[0] if fault == "sibling_last" else sib[j])
    T["sibling"] = sib
    T["nchild"] = np.array([len(c) for c in children], np.int32)
    # leaf of every particle (caller index -> pre-order node; -1: not in the tree)
    leaf_of = np.full(len(pos), -1, np.int64)
    for j in range(M):
        if leafmem[j] is not None:
            leaf_of[leafmem[j]] = j
    T["leaf_of"] = leaf_of
    # moments: long-double sums over the node's own particles; the rounding counts of the module docstring
    LD = np.longdouble
    pl, ml = pos.astype(LD), mass32.astype(np.float64).astype(LD)
    Mn, cof, absx = np.zeros(M, LD), np.zeros((M, 3), LD), np.zeros((M, 3), LD)
    kc, km = np.zeros(M, np.int64), np.zeros(M, np.int64)
    for j in range(M - 1, -1, -1):
        idx = allmem[j]
        if len(idx) == 0:
            cof[j] = T["center"][j].astype(LD)
            continue
        m = ml[idx]
        Mn[j] = m.sum()
        cof[j] = (m[:, None] * pl[idx]).sum(0) / Mn[j]
        absx[j] = (m[:, None] * np.abs(pl[idx])).sum(0) / Mn[j]
        if pcount[j] > 0:
            kc[j], km[j] = 2 * pcount[j], pcount[j] - 1
        else:
            ch = children[j]
            kc[j], km[j] = max(kc[c] for c in ch) + 2 * len(ch), max(km[c] for c in ch) + len(ch) - 1
    T.update(mass=Mn, cofm=cof, absx=absx, kc=kc, km=km)
    # hmax
    if hsml is not None:
        hs = np.asarray(hsml, np.float64)
        ty = np.ones(len(pos), np.int64) if type is None else (np.asarray(type).astype(np.int64) & 7)
        counts = (ty == 0) | (ty == 5)
        if hact is not None and fault != "hmax_active":
            counts &= ~np.asarray(hact).astype(bool)

        def excess(idx, j):                                # fabs(Pos - centre) + Hsml - len / 2., the largest of the three axes
            return (np.abs(pos[idx] - T["center"][j]) + hs[idx, None] - T["len"][j] / 2.).max(1)
        hm = np.zeros(M)
        for j in range(M - 1, -1, -1):
            if fault == "hmax_own_faces" or pcount[j] > 0:
                idx = allmem[j][counts[allmem[j]]]
                hm[j] = max(0.0, excess(idx, j).max()) if len(idx) else 0.0
            else:
                hm[j] = max([0.0] + [hm[c] for c in children[j]])
        T["hmax"] = hm
    # level order: stable by level; children contiguous; the merge counts of sibling leaves
    bfs = np.argsort(T["level"], kind="stable")
    inv = np.empty(M, np.int64)
    inv[bfs] = np.arange(M)
    first = np.full(M, -1, np.int64)                       # (pre-order index -> firstchild word)
    need = 1 if fault == "merge_one" else 2
    if M == 1 and pcount[0] > 0:
        first[0] = 0
    for j in range(M):
        ch = children[j]
        if not ch:
            continue
        first[j] = inv[ch[0]]
        assert np.array_equal(inv[ch], inv[ch[0]] + np.arange(len(ch)))
        pc = [pcount[c] for c in ch]

        def joined(c0, c1):
            s = pc[c0:min(c1, len(ch))]
            return sum(s) if (all(v > 0 for v in s) and len(s) >= need and sum(s) <= 8) else 0
        for k, c in enumerate(ch):
            if pc[k] > 0:
                first[c] = joined(k & 6, (k & 6) + 2) | (joined(k & 4, (k & 4) + 4) << 4) | (joined(0, 8) << 8)
    T.update(dfs_of_bfs=bfs.astype(np.int64), bfs_of_dfs=inv, firstchild=first)
    return T


def leaf_blocks(T, pos, mass, order):
    """srcL: per level-order node 8 records (x, y, z, m); a leaf's particles in the tree order given, slots beyond its count the first
    particle's position with mass 0; the block behind the last node all zero.  Returns (blocks [M + 1, 8, 4], is_leaf [M])."""
    M = len(T["level"])
    out = np.zeros((M + 1, 8, 4))
    m64 = np.asarray(mass, np.float32).astype(np.float64)
    leaf = np.zeros(M, bool)
    for i, j in enumerate(T["dfs_of_bfs"]):
        pc, ps = T["pcount"][j], T["pstart"][j]
        if pc <= 0:
            continue
        leaf[i] = True
        for s in range(8):
            ci = order[ps + (s if s < pc else 0)]
            out[i, s, :3] = pos[ci]
            out[i, s, 3] = m64[ci] if s < pc else 0.0
    return out, leaf


def level_cell_sums(pos, mass, box, La, own):
    """per level-(La - 1) cell (index = its octant digits, most significant first) the long-double sums (m, m x, m y, m z), the sums of the
    absolute terms and the number of particles, over the particles `own`"""
    LD = np.longdouble
    own = np.asarray(own, np.int64)
    digits = octant_digits(pos, box)
    cell = np.zeros(len(pos), np.int64)
    for l in range(La - 1):
        cell = cell * 8 + digits[:, l]
    nc = 8 ** (La - 1)
    s, a, cnt = np.zeros((nc, 4), LD), np.zeros((nc, 4), LD), np.zeros(nc, np.int64)
    ml, pl = np.asarray(mass, np.float32).astype(np.float64).astype(LD), np.asarray(pos, np.float64).astype(LD)
    for c in np.unique(cell[own]):
        i = own[cell[own] == c]
        t = np.c_[ml[i], ml[i, None] * pl[i]]
        s[c], a[c], cnt[c] = t.sum(0), np.abs(t).sum(0), len(i)
    return s, a, cnt


# ------------------------------------------------------------------------------------------------------------ comparisons
STRUCT_FIELDS = ("level", "center", "len", "pcount", "pstart", "sibling", "nchild", "firstchild", "leaf_of", "hmax")


def differences(A, B):
    """names of the structural fields (bit-equal or integer-equal ones) in which two restated trees differ"""
    out = []
    for k in STRUCT_FIELDS:
        if (k in A) != (k in B) or (k in A and not (A[k].shape == B[k].shape and np.array_equal(A[k], B[k]))):
            out.append(k)
    return out


def moment_ratios(T, mass, cofm, sel=None):
    """(worst |M - ref| / bound, worst |cofm - ref| / bound) of moments given in pre-order against the long-double ones"""
    sel = np.arange(len(T["level"])) if sel is None else np.asarray(sel)
    LD = np.longdouble
    dm = np.abs(np.asarray(mass, np.float64)[sel].astype(LD) - T["mass"][sel])
    bm = (T["km"][sel] + 1) * LD(U) * T["mass"][sel]
    dc = np.abs(np.asarray(cofm, np.float64)[sel].astype(LD) - T["cofm"][sel])
    bc = ((T["kc"][sel] + 1) * LD(U))[:, None] * T["absx"][sel]

    def worst(d, b):
        d, b = np.asarray(d, np.float64), np.asarray(b, np.float64)
        with np.errstate(divide="ignore", invalid="ignore"):
            r = np.where(b > 0, d / b, np.where(d > 0, np.inf, 0.0))
        return float(r.max()) if r.size else 0.0
    return worst(dm, bm), worst(dc, bc)


def gate_moments(T, mass, cofm, label="", sel=None, exact_single=False):
    """the derived bound of the module docstring; exact_single: a single-particle leaf's centre of mass is the position to the bit"""
    rm, rc = moment_ratios(T, mass, cofm, sel)
    print("%s moments: mass worst %.3g of its bound, cofm worst %.3g of its bound (root: kc = %d, km = %d)" % (label, rm, rc, T["kc"][0], T["km"][0]))
    assert rm <= 1 and rc <= 1, (label, rm, rc)
    one = np.flatnonzero(T["pcount"] == 1) if sel is None else np.asarray(sel)[T["pcount"][sel] == 1]
    assert not exact_single or np.array_equal(np.asarray(cofm, np.float64)[one], T["cofm"][one].astype(np.float64)), label
    return rm, rc


def match_by_cell(level, center, T):
    """perm with (level, center)[perm[j]] == the restated node j, bit for bit; asserts that the two node sets are the same"""
    a = np.lexsort((center[:, 2], center[:, 1], center[:, 0], level))
    b = np.lexsort((T["center"][:, 2], T["center"][:, 1], T["center"][:, 0], T["level"]))
    assert len(a) == len(b), (len(a), len(b))
    assert np.array_equal(level[a], T["level"][b]) and np.array_equal(center[a], T["center"][b])
    perm = np.empty(len(b), np.int64)
    perm[b] = a
    return perm


# ------------------------------------------------------------------------------------------------------------ scenes
def _masses(rng, n):
    return (10.0 ** rng.uniform(-3, 3, n)).astype(np.float32)


def _jittered(rng, n, box):
    g = (np.stack(np.meshgrid(*[np.arange(n)] * 3, indexing="ij"), -1).reshape(-1, 3) + 0.5 + rng.uniform(-0.4, 0.4, (n ** 3, 3))) * (box / n)
    return g


PILE = np.array([3.3, 7.1, 4.9])
CENTRE_LEVELS = range(7)


def _deep(piles=True):
    rng = np.random.RandomState(1771)
    box = BOX
    parts, marks = [_jittered(rng, 12, box)], {}

    def add(name, p):
        p = np.atleast_2d(np.asarray(p, np.float64))
        start = sum(len(q) for q in parts)
        parts.append(p)
        marks[name] = np.arange(start, start + len(p))
    if piles:
        # eight in one spot, and a ninth in the other x-half of their level-20 cell: the position comes from the replayed descent
        add("pile", np.tile(PILE, (8, 1)))
        c20, l20 = cell_of(PILE, box, 20)
        ninth = PILE.copy()
        ninth[0] = c20[0] + (-0.25 if PILE[0] > c20[0] else 0.25) * l20
        add("ninth", ninth)
        o = rng.uniform(0, 4e-6 * box, (10, 3))
        o[0] = 0.0
        add("origin", o)
        f = box - rng.uniform(0, 4e-6 * box, (10, 3))
        f[0] = np.nextafter(box, 0)
        add("corner", f)
        # along the pile's path (every cell of it is internal down to level 20): exactly on the cell's centre, and one unit in the last
        # place above it
        on = np.array([cell_of(PILE, box, l)[0] for l in CENTRE_LEVELS])
        add("on_centre", on)
        add("above_centre", np.nextafter(on, np.inf))
    pos = np.concatenate(parts)
    return dict(pos=pos, mass=_masses(rng, len(pos)), box=box, marks=marks)


def _level(nshare):
    """a shallow background and nine particles that share `nshare` octant digits and separate at the next: deepest leaf at nshare + 1"""
    rng = np.random.RandomState(100 + nshare)
    box = BOX
    bg = _jittered(rng, 6, box)
    c, ln = cell_of(np.array([6.2, 2.9, 8.3]), box, nshare)
    oct_ = np.array([[(o & 1), (o >> 1) & 1, (o >> 2) & 1] for o in range(8)]) * 2.0 - 1.0
    nine = np.concatenate([c + oct_[:1] * 0.0625 * ln,      # octant 0, near the cell's centre: the LARGER key of the two in octant 0 ...
                           c + oct_ * 0.25 * ln])          # ... comes FIRST in caller order; then one per octant
    pos = np.concatenate([bg, nine])
    return dict(pos=pos, mass=_masses(rng, len(pos)), box=box, marks=dict(nine=np.arange(len(bg), len(pos))))


def straddles(T):
    """does a leaf hold particles on both sides of a multiple of 256 in tree order?"""
    lf = T["pcount"] > 0
    return any(np.any((T["pstart"][lf] < b) & (T["pstart"][lf] + T["pcount"][lf] > b)) for b in range(256, T["n"], 256))


def _blocks(n, seed):
    """uniform points; the first seed from `seed` on whose tree has a leaf across a block boundary (a property of the scene's own tree)"""
    while True:
        rng = np.random.RandomState(seed)
        S = dict(pos=rng.uniform(0, BOX, (n, 3)), mass=_masses(rng, n), box=BOX, marks={})
        if n <= 256 or straddles(restate(S["pos"], S["mass"], BOX)):
            return S
        seed += 100


def _types():
    S = _deep()
    rng = np.random.RandomState(5)
    n = len(S["pos"])
    S["type"] = rng.choice(np.array([0, 1, 5], np.uint8), n)
    S["hsml"] = 0.01 * 200.0 ** rng.uniform(0, 1, n)
    S["hsml"][:2] = (0.01, 2.0)
    S["hsml2"] = 0.01 * 200.0 ** rng.uniform(0, 1, n)
    S["hact"] = (rng.uniform(0, 1, n) < 0.3).astype(np.uint8)
    S["garbage"] = np.array([3, 700, int(S["marks"]["pile"][2]), int(S["marks"]["origin"][4]), n - 1])
    return S


def _tiny(n):
    rng = np.random.RandomState(40 + n)
    m = n if n else 3
    S = dict(pos=rng.uniform(0, BOX, (m, 3)), mass=_masses(rng, m), box=BOX, marks={})
    if n == 0:                                              # a mask that selects nothing
        S["type"], S["mask"] = np.ones(m, np.uint8), 1
    return S


SCENES = {"deep": _deep, "deep_nopiles": lambda: _deep(False), "level10": lambda: _level(9), "level11": lambda: _level(10),
          "blocks200": lambda: _blocks(200, 7), "blocks512": lambda: _blocks(512, 8), "blocks700": lambda: _blocks(700, 9), "types": _types,
          "tiny0": lambda: _tiny(0), "tiny1": lambda: _tiny(1), "tiny8": lambda: _tiny(8), "tiny9": lambda: _tiny(9)}
_cache = {}


def scene(name):
    """dict(pos, mass, box, marks[, type, hsml, hsml2, hact, garbage, mask]); computed once, never to be modified"""
    if name not in _cache:
        S = SCENES[name]()
        for v in S.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _cache[name] = S
    return _cache[name]


def scene_members(S, mask=None, garbage=False):
    """caller indices of the particles of the scene's tree for a type mask (None: the scene's own, default all), without the garbage"""
    n = len(S["pos"])
    mask = S.get("mask", 63) if mask is None else mask
    ty = S["type"].astype(np.int64) if "type" in S else np.ones(n, np.int64)
    keep = ((1 << ty) & mask) != 0
    if garbage and "garbage" in S:
        keep[S["garbage"]] = False
    return np.flatnonzero(keep)


def reference(name, mask=None, garbage=False, minlevel=0):
    """the restated tree of a scene (shared among the tests, never to be modified)"""
    key = ("ref", name, mask, garbage, minlevel)
    if key not in _cache:
        S = scene(name)
        _cache[key] = restate(S["pos"], S["mass"], S["box"], scene_members(S, mask, garbage), minlevel, S.get("type"), S.get("hsml"), S.get("hact"))
    return _cache[key]
