"""The frontier of the list kernel (k_walk_lists8, walk variant 6): packed entries, positions of the pushed children from one prefix sum,
unpredicated child writes, the target passes taken from the top bit of a frontier word down.

None of this may change a decision: every case runs the two-kernel walk and compares it with the lane-per-target kernel (variant 1), which
has no frontier at all.  The three interaction counters must be EQUAL; accelerations and potentials differ by the order of summation only
and must agree to 1e-13 of the largest value.  The packed frontier and the two-array one (MPG_LISTS_PACKQ=0, what trees beyond 2^24 nodes
take) must produce the same lists entry for entry: their results are compared bit for bit.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
G = 43.0071
TOL = 1e-13


def _setup(eng, box, mean_sep, nmesh, use_bh):
    eng.gravshort_fill_ntab(0, 1.5)
    eng.gravpm_init_periodic(box, 1.5, nmesh, G)
    eng.set_gravshort_treepar(TreeUseBH=use_bh, Rcut=6.0)
    eng.gravshort_set_softenings(mean_sep)


def _make_set(pkg, name):
    """(pos, mass, box, grid size of the mean separation, Nmesh)"""
    if name in ("zel16", "zel32", "ragged"):
        n = 32 if name == "zel32" else 16
        pos, mass, box = pkg.ics.s_zel(n)
        if name == "ragged":        # 4093 targets: the last wave holds 5
            pos, mass = pos[:-3], mass[:-3]
        return pos, mass, box, n, 2 * n
    if name == "chains":
        # a 16^3 lattice and, in the corner at the origin, 10 particles within 1e-6 of the box: the cell that holds them is split about
        # 14 more times before they separate, every split leaving ONE occupied octant
        pos, mass, box = pkg.ics.s_grid(16)
        pile = 1e-6 * box * np.random.RandomState(7).random_sample((10, 3))
        pos = np.concatenate([pos, pile])
        return pos, np.ones(len(pos), np.float32), box, 16, 32
    if name == "clust":
        pos, mass, box = pkg.ics.s_clust(20, box=8.0, seed=3)
        return pos, mass, box, 20, 40
    raise KeyError(name)


def _nchild(t):
    """occupied octants per node of an exported tree (depth-first pre-order: the parent of a node is the last node before it one level up)"""
    level = t["level"]
    nch = np.zeros(len(level), np.int64)
    path = []
    for i, lv in enumerate(level):
        del path[lv:]
        if lv > 0:
            nch[path[lv - 1]] += 1
        path.append(i)
    return nch


def _walk(pkg, eng, s, variant, walks, monkeypatch=None, packq=True, capacity=512, check_tree=None, count=True):
    """The walks of one set with one kernel: per walk (acceleration, potential, counters).  `walks`: per walk (TreeUseBH, GravPM, previous
    acceleration), identical inputs for every kernel.  count=False: the kernels without the interaction counters, as a simulation runs them."""
    pos, mass, box, n, nmesh = s
    out = []
    if monkeypatch is not None:
        monkeypatch.setenv("MPG_LISTS_PACKQ", "1" if packq else "0")
    try:
        eng.set_walk_variant(variant)
        eng.set_walk_list_capacity(capacity)
        eng.set_instrumentation(False, count)
        for use_bh, gpm, prev in walks:
            _setup(eng, box, box / n, nmesh, use_bh)
            P = pkg.make_particles(pos, mass)
            P["GravPM"] = gpm
            P["FullTreeGravAccel"] = prev
            eng.force_tree_full(P, box)
            if check_tree is not None:
                check_tree(eng.tree_export())
            eng.grav_short_tree(P)
            c = eng.walk_counters() if count else dict(pp=0, nodes_visited=0, nodes_used=0)
            out.append((P["FullTreeGravAccel"].copy(), P["Potential"].copy(), (c["pp"], c["nodes_visited"], c["nodes_used"]), eng.walk_choice()))
    finally:
        eng.set_walk_variant(0)
        eng.set_walk_list_capacity(512)
        eng.set_instrumentation(False, False)
    return out


_cache = {}


def _reference(pkg, eng, name):
    """The set, the inputs of its two walks (Barnes-Hut opening first, then the relative criterion with the first walk's accelerations)
    and what the lane-per-target kernel makes of them; computed once per session."""
    if name not in _cache:
        s = _make_set(pkg, name)
        pos, mass, box, n, nmesh = s
        _setup(eng, box, box / n, nmesh, 1)
        P = pkg.make_particles(pos, mass)
        eng.gravpm_force(P)
        gpm = P["GravPM"].copy()
        zero = np.zeros_like(gpm)
        if name == "clust":     # a zero old acceleration: "mass l^2 > r^4 aold" holds for every node with mass
            walks = [(0, zero, zero)]
            ref = _walk(pkg, eng, s, 1, walks)
        else:
            first = _walk(pkg, eng, s, 1, [(1, gpm, zero)])
            walks = [(1, gpm, zero), (0, gpm, first[0][0])]
            ref = first + _walk(pkg, eng, s, 1, walks[1:])
        for a, p, c, _ in ref:
            assert np.isfinite(a).all() and np.isfinite(p).all() and c[0] > 0 and c[1] > 0
            a.setflags(write=False)
            p.setflags(write=False)
        _cache[name] = (s, walks, ref)
    return _cache[name]


def _compare(name, got, ref):
    for k, ((a, p, c, _), (a0, p0, c0, _)) in enumerate(zip(got, ref)):
        ea = np.abs(a - a0).max() / np.abs(a0).max()
        ep = np.abs(p - p0).max() / np.abs(p0).max()
        print("%s walk %d: counters %s / %s, acceleration %.2e, potential %.2e" % (name, k, c, c0, ea, ep))
        assert c == c0
        assert ea <= TOL and ep <= TOL, (ea, ep)


def _assert_chains(t):
    nch = _nchild(t)
    internal = t["pcount"] == 0
    assert np.array_equal(nch > 0, internal)
    hist = np.bincount(nch[internal], minlength=9)
    print("nchild histogram of the internal nodes:", hist[1:])
    single = np.nonzero(internal & (nch == 1))[0]
    # (pre-order: the only child of node i is node i + 1) single-child nodes that follow each other, beside nodes with 8 children
    assert hist[1] >= 8 and hist[8] >= 64
    assert np.count_nonzero(nch[single + 1] == 1) >= 6


@pytest.mark.parametrize("name", ["zel16", "zel32", "chains", "ragged"])
def test_frontier_against_lane_per_target(pkg, engine, name):
    """Barnes-Hut first walk and relative criterion on Zel'dovich sets of 16^3 and 32^3; single-child chains beside nodes with 8 children
    (a lane that pushes one child writes 7 dead slots into the entries of the lanes above it); a target count that is no multiple of 8."""
    s, walks, ref = _reference(pkg, engine, name)
    assert name != "ragged" or len(s[0]) % 8 != 0
    got = _walk(pkg, engine, s, 6, walks, check_tree=_assert_chains if name == "chains" else None)
    _compare(name, got, ref)
    for r in got:
        assert r[3][0] == 6


def test_frontier_growing_until_the_fallback(pkg, engine):
    """A zero old acceleration on a clustered set of 8000 particles: every node with mass is opened, frontier and lists grow until targets
    are handed to the fallback kernel, and the results are still those of the lane-per-target kernel."""
    s, walks, ref = _reference(pkg, engine, "clust")
    got = _walk(pkg, engine, s, 6, walks)
    variant, cap, handed_on = got[0][3]
    print("walk_choice:", got[0][3])
    assert variant == 6 and handed_on > 0
    _compare("clust", got, ref)


@pytest.mark.parametrize("name", ["zel16", "zel32", "chains"])
def test_packed_against_two_array_frontier(pkg, engine, name, monkeypatch):
    """One word per entry against node index and mask in two arrays (MPG_LISTS_PACKQ=0): the same lists, so the same bits - from the
    counting kernels and from the plain ones."""
    s, walks, ref = _reference(pkg, engine, name)
    packed = _walk(pkg, engine, s, 6, walks, monkeypatch, packq=True)
    two = _walk(pkg, engine, s, 6, walks, monkeypatch, packq=False)
    _compare(name + " (two arrays)", two, ref)
    for (a, p, c, _), (a2, p2, c2, _) in zip(packed, two):
        assert c == c2
        assert np.array_equal(a, a2) and np.array_equal(p, p2)
    # (without the counters a walk whose lists overflow for many targets is repeated with longer lists, with them the fallback kernel takes
    # those targets: plain and counting walks may sum in another order, the two frontiers of either kind may not)
    plain = [_walk(pkg, engine, s, 6, walks, monkeypatch, packq=packq, count=False) for packq in (True, False)]
    for (a, p, _, choice), (a2, p2, _, choice2), (a0, p0, _, _) in zip(plain[0], plain[1], ref):
        assert choice == choice2
        assert np.array_equal(a, a2) and np.array_equal(p, p2)
        assert np.abs(a - a0).max() <= TOL * np.abs(a0).max() and np.abs(p - p0).max() <= TOL * np.abs(p0).max()
