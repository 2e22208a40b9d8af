"""The particle sets of the sub-grid group sums and of black-hole seeding (test_fof_subgrid_restated.py, test_gpu_fof_subgrid.py): each the
smallest shape at which k_fof_subgrid / k_fof_seed_index / k_blackhole_make_one (csrc/fof.hip) can go wrong.

A set is a list of CLUSTERS on a coarse grid, 20 linking lengths apart: the members of a cluster lie within 0.35 LL of its centre, so its dark
matter links into one group and its gas, stars and black holes attach to it (their search ends at 6.4 LL); a cluster of one row is a
particle on its own.  IDs rise cluster by cluster, so the label order of the catalogue (rows sorted by MinID) is the order the clusters are
listed in, and the place of every group among the 64-row waves and 256-row blocks of the kernel is chosen here.  The particle order is a
permutation of that, so every column is gathered.  Membership comes from the FOF oracle (oracle/fof_oracle.py); nothing here finds groups.
Not a test module."""
import functools

import numpy as np

LL = 1.0
GRID = 16                 # clusters per side
BOX = 20.0 * GRID * LL
ID_HIGH = (1 << 63) + 12345
MIXED = (1, 0, 1, 4, 0, 5, 1, 0)          # the types a cluster of mixed rows cycles through (its first row is dark matter)


def cluster(n, kinds=MIXED):
    return [kinds[k % len(kinds)] for k in range(n)]


def layout(name):
    """-> (clusters: list of lists of types, FOFHaloMinLength)"""
    singles = lambda n, t=1: [[t] for _ in range(n)]
    if name in ("minlen1", "minlen2"):
        # one wave holds >= 8 groups; with minlen 2 the single rows between them belong to no group
        cl = []
        for k in range(60):
            cl += [cluster(2 + k % 7)] + singles(k % 3, 0 if k % 2 else 1)
        return cl, 1 if name == "minlen1" else 2
    if name == "wave64":
        # a group of exactly 64 rows that starts on a wave boundary (64 rows of no group before it), and one that ends on the last row
        return singles(64) + [cluster(64)] + singles(5) + [cluster(9)] + singles(3) + [cluster(70)], 2
    if name == "big700":
        # one group of 700 rows across waves and 256-row blocks, starting off a boundary; a group of dark matter only; a group that ends on
        # the last row of all
        return singles(37) + [cluster(700)] + singles(11, 0) + [[1] * 40] + [cluster(130)] + singles(2) + [cluster(33)], 2
    if name == "seeds":
        # groups for the marks of fof_seed: with and without stars, with and without a black hole
        return [[1, 1, 0, 0, 4, 4], [1, 1, 0, 0, 4, 4, 5], [1, 0, 0, 4], [1, 1, 0, 0, 0], [1, 1, 4, 4], [1, 1, 0, 0, 4, 4, 0, 0],
                [1, 1, 0, 4, 0, 4, 1, 1, 0, 0]] + singles(3) + [cluster(100, (1, 0, 4, 0)), cluster(300, (1, 0, 4, 1, 0))], 2
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def particles(name, order="shuffle", high_ids=False, seed=0):
    """The particle table of a layout, made ONCE per argument set and never changed (copy what you change).
    order: "label" (particle order = label order), "reverse", "shuffle".  high_ids: every ID above 2^63, and the densest gas row of the first
    kept group gets ID 2^64 - 10, so that ID + 23 wraps."""
    clusters, minlen = layout(name)
    rng = np.random.RandomState(1000 + seed)
    n = sum(len(c) for c in clusters)
    assert len(clusters) <= GRID ** 3
    cells = rng.permutation(GRID ** 3)[:len(clusters)]
    pos = np.zeros((n, 3))
    typ = np.zeros(n, np.uint8)
    cl_of = np.zeros(n, np.int64)
    k = 0
    for c, cell in zip(range(len(clusters)), cells):
        centre = (np.array([cell % GRID, (cell // GRID) % GRID, cell // GRID ** 2]) + 0.5) * 20.0 * LL
        m = len(clusters[c])
        d = rng.standard_normal((m, 3))
        d *= (0.35 * LL * rng.random_sample((m, 1)) ** (1 / 3.)) / np.linalg.norm(d, axis=1)[:, None]
        pos[k:k + m] = centre + d
        typ[k:k + m] = clusters[c]
        cl_of[k:k + m] = c
        k += m
    ids = np.arange(n, dtype=np.uint64) * np.uint64(3) + np.uint64(7)
    P = dict(sfr=rng.random_sample(n) * 2.5, metallicity=rng.random_sample(n) * 0.04, metals=(rng.random_sample((n, 9)) * 0.01).astype(np.float32),
             heiii_ionized=(rng.random_sample(n) < 0.4).astype(np.uint8), bh_mass=rng.random_sample(n) * 1e-3 + 5e-5,
             bh_mdot=rng.random_sample(n) * 1e-2, density=np.exp(rng.standard_normal(n) * 3.0),
             delaytime=np.where(rng.random_sample(n) < 0.3, rng.random_sample(n), 0.0))
    # masses with few bits (sums of them are exact in any order: the marks of fof_seed compare group masses with thresholds)
    mass = rng.choice(np.array([0.25, 0.5, 0.75, 1.0], np.float32), n)
    tb_hydro = rng.randint(20, 40, n).astype(np.uint8)
    if high_ids:
        ids = ids + np.uint64(ID_HIGH)
        first = next(c for c in range(len(clusters)) if len(clusters[c]) >= max(minlen, 2) and 0 in clusters[c])
        rows = np.nonzero((cl_of == first) & (typ == 0))[0]
        P["delaytime"][rows[0]] = 0.0
        P["density"][rows[0]] = 1e9
        ids[rows[0]] = np.uint64((1 << 64) - 10)
    perm = {"label": np.arange(n), "reverse": np.arange(n)[::-1], "shuffle": rng.permutation(n)}[order]
    out = dict(name=name, n=n, minlen=minlen, box=BOX, LL=LL, pos=pos[perm], type=typ[perm], ids=ids[perm], mass=mass[perm], tb_hydro=tb_hydro[perm],
               cluster=cl_of[perm], P={k: np.ascontiguousarray(v[perm]) for k, v in P.items()}, flags=None)
    for v in list(out.values()) + list(out["P"].values()):
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


def variant(S, **changes):
    """a copy of the set S with columns of P (or flags / type) replaced; the arrays of S itself stay as they are"""
    T = dict(S)
    T["P"] = dict(S["P"])
    for k, v in changes.items():
        if k in T["P"]:
            T["P"][k] = v
        else:
            T[k] = v
    return T


def with_ties(S, far):
    """S with two gas rows of its largest cluster sharing that group's largest density (nothing decoupled): `far` = False puts them next to
    each other in label order (one wave), True at the 10th and the 10th-last gas row (different 256-row blocks in a group of 700).
    -> (set, (row a, row b))"""
    big = np.bincount(S["cluster"]).argmax()
    rows = np.nonzero((S["cluster"] == big) & (S["type"] == 0))[0]
    # the row of the catalogue every member lands on: the rows of the clusters listed before, then the members in particle order (the
    # catalogue's sort by label is stable)
    members = np.sort(np.nonzero(S["cluster"] == big)[0])
    start = int((S["cluster"] < big).sum())
    row_of = {int(i): start + r for r, i in enumerate(members)}
    by_index = np.sort(rows)
    if far:
        a, b = by_index[10], by_index[-10]
        assert row_of[int(a)] // 256 != row_of[int(b)] // 256
    else:
        a, b = next((x, y) for x, y in zip(by_index[10:], by_index[11:]) if row_of[int(x)] // 64 == row_of[int(y)] // 64)
    dens = S["P"]["density"].copy()
    dens[rows] = np.minimum(dens[rows], 50.0)
    dens[[a, b]] = 77.25
    return variant(S, density=dens, delaytime=np.zeros(S["n"])), (int(a), int(b))


def with_flags(S):
    """S with garbage (bit 0) and swallowed (bit 1) rows: they are in no tree and attach to nothing, so each stays on its own"""
    rng = np.random.RandomState(5)
    f = np.zeros(S["n"], np.uint8)
    f[rng.choice(S["n"], S["n"] // 12, replace=False)] = 1
    f[rng.choice(S["n"], S["n"] // 12, replace=False)] |= 2
    return variant(S, flags=f)


_CACHE = {}


def membership(orc, S, minlen=None):
    """(grnr, group table, group[i]) of the set from the FOF oracle, computed once per (set, flags, minlen)"""
    from oracle import fof_oracle as F
    from fof_subgrid_restated import group_index
    minlen = S["minlen"] if minlen is None else minlen
    key = (S["name"], S["pos"].tobytes()[:64], S["ids"].tobytes()[:64], None if S["flags"] is None else S["flags"].tobytes(), S["type"].tobytes(), minlen)
    if key not in _CACHE:
        grnr, G = F.fof_fof(orc, np.array(S["pos"]), np.array(S["mass"]), np.array(S["ids"]), S["box"], S["LL"], minlen, type=np.array(S["type"]),
                            flags=None if S["flags"] is None else np.array(S["flags"]))
        _CACHE[key] = (grnr, G, group_index(grnr, G["GrNr"]))
    return _CACHE[key]


# the sets every sum is checked on: (layout, order, high_ids)
SUM_SCENES = [("minlen1", "shuffle", False), ("minlen2", "shuffle", False), ("wave64", "label", False), ("wave64", "shuffle", False),
              ("big700", "label", False), ("big700", "shuffle", True), ("seeds", "shuffle", False)]
