"""The GPU tree build (csrc/tree_build.hip) against the tree restated from its definition (tests/tree_restated.py; tests/test_tree_restated.py
holds the CPU oracle to the same restatement, asserts what each scene forces and shows which one-line faults the comparison catches).

  node table   level, centre and len bit-identical, pcount, pstart and sibling as integers, entry for entry in pre-order; the set of caller
               indices of every leaf; host and device forms identical bytes
  moments      the derived bound of tree_restated (a count of roundings per node, nothing fitted); a single-particle leaf's centre of mass
               is the position to the bit
  hmax         bit-equal per node.  The library takes a particle out of hmax by a negative smoothing length (k_only_hmax_leaf: "< 0: does
               not contribute"): that is how the scene's hydro-active particles are handed over.  calc_moments with smoothing lengths (hmax
               "built with the moments") has no caller in the library and no entry point, so that route cannot be run.
  level order, search geometry, leaf blocks   through mpg_tree_export_derived
  top of a decomposed tree   k_top_partial against long-double cell sums (n roundings for n own particles), k_top_set against the bound above
"""
import numpy as np
import pytest

import tree_restated as TR

pytestmark = pytest.mark.gpu
G = 43.0071
TABLE = ("level", "center", "len", "pcount", "pstart", "sibling")
EXPORTED = TABLE + ("cofm", "mass", "hmax", "order")


def particles(pkg, S, garbage=False):
    P = pkg.make_particles(S["pos"], S["mass"], type=S["type"] if "type" in S else 1)
    if garbage and "garbage" in S:
        P["Flags"][S["garbage"]] = 1                       # IsGarbage
    return P


def host_build(pkg, engine, S, mask=None, garbage=False):
    mask = S.get("mask", 63) if mask is None else mask
    P = particles(pkg, S, garbage)
    if mask == 63:
        engine.force_tree_full(P, S["box"])
    else:
        engine.force_tree_rebuild_mask(P, S["box"], mask)
    return engine.tree_export()


def bind(engine, S, garbage=False, pos=None, mass=None):
    import torch
    ty = S["type"].copy() if "type" in S else np.ones(len(S["pos"]), np.uint8)
    if garbage and "garbage" in S:
        ty[S["garbage"]] = 7                               # (what the host forms make of a garbage flag: no mask has that bit)
    keep = dict(pos=torch.from_numpy(np.array(S["pos"] if pos is None else pos)).cuda(),
                mass=torch.from_numpy(np.array(S["mass"] if mass is None else mass)).cuda(), type=torch.from_numpy(ty.astype(np.uint8)).cuda())
    engine.dev_bind_particles(keep["pos"], keep["mass"], S["box"], type=keep["type"])
    return keep


def dev_build(engine, S, mask=None, garbage=False, moments=True):
    mask = S.get("mask", 63) if mask is None else mask
    keep = bind(engine, S, garbage)
    if mask == 63 and moments:
        engine.dev_force_tree_build(63)
    else:
        engine.dev_force_tree_rebuild_mask(mask, with_moments=moments)
    engine.synchronize()
    return keep


def check_table(t, T, label):
    assert len(t["level"]) == len(T["level"]), (label, len(t["level"]), len(T["level"]))
    for k in TABLE:
        assert np.array_equal(t[k], T[k]), (label, k)
    assert len(t["order"]) == T["n"]
    for j in np.flatnonzero(T["pcount"] > 0):
        got = np.sort(t["order"][T["pstart"][j]:T["pstart"][j] + T["pcount"][j]])
        assert np.array_equal(got, T["leafmem"][j]), (label, "members of leaf", j)


def same_bytes(a, b, label):
    for k in EXPORTED:
        assert a[k].dtype == b[k].dtype and a[k].tobytes() == b[k].tobytes(), (label, k)


# ------------------------------------------------------------------------------------------- a, c: node set, geometry, moments
@pytest.mark.parametrize("name", list(TR.SCENES))
def test_node_table_and_moments(pkg, engine, name):
    S = TR.scene(name)
    garbage = "garbage" in S
    T = TR.reference(name, garbage=garbage)
    th = host_build(pkg, engine, S, garbage=garbage)
    check_table(th, T, name + " host form")
    TR.gate_moments(T, th["mass"], th["cofm"], name + " GPU", exact_single=True)
    keep = dev_build(engine, S, garbage=garbage)
    td = engine.tree_export()
    check_table(td, T, name + " device form")
    same_bytes(th, td, name)
    if T["n"] == 0:
        assert th["mass"][0] == 0 and np.array_equal(th["center"][0], th["cofm"][0])
    del keep


# ------------------------------------------------------------------------------------------- b: order
def test_particle_order_is_a_function_of_the_set(pkg, engine):
    first = host_build(pkg, engine, TR.scene("deep"))
    S10, T10 = TR.scene("level10"), TR.reference("level10")
    t10 = host_build(pkg, engine, S10)
    again = host_build(pkg, engine, TR.scene("deep"))
    same_bytes(first, again, "deep, level10, deep")
    # A tree no deeper than level 10 keeps the stable sort of the top 30 key bits: the order is the caller order sorted by the first ten
    # octant digits, so particles of a leaf that agree in those stay in caller order - the two of the nine in octant 0, which lie in one
    # level-10 leaf with the LARGER key first.  (Particles of a shallower leaf differ within the ten digits and come in key order.)
    d10 = T10["digits"][:, :10]
    assert np.array_equal(t10["order"], np.lexsort(d10.T[::-1]))
    a, b = S10["marks"]["nine"][:2]
    k = list(t10["order"]).index(a)
    assert t10["order"][k + 1] == b and T10["level"][T10["leaf_of"][a]] == 10
    # the full sort: by all 21 digits, equal keys in caller order - the eight coincident particles
    S, T = TR.scene("deep"), TR.reference("deep")
    assert np.array_equal(first["order"], np.lexsort(T["digits"].T[::-1]))
    j = T["leaf_of"][S["marks"]["pile"][0]]
    assert np.array_equal(first["order"][T["pstart"][j]:T["pstart"][j] + 8], S["marks"]["pile"])
    t11 = host_build(pkg, engine, TR.scene("level11"))          # one level deeper: the build must notice and sort all bits
    assert np.array_equal(t11["order"], np.lexsort(TR.reference("level11")["digits"].T[::-1]))


# ------------------------------------------------------------------------------------------- d: hmax, masks, include lists
def excluded(S, hsml):
    return np.where(S["hact"] != 0, -1.0, hsml)


def test_hmax_per_node(pkg, engine):
    import torch
    S, T = TR.scene("types"), TR.reference("types")
    H = torch.from_numpy(excluded(S, S["hsml"])).cuda()
    for moments in (False, True):
        keep = dev_build(engine, S, mask=63, moments=moments)
        engine.dev_force_tree_calc_hmax(hsml=H)
        engine.synchronize()
        t = engine.tree_export()
        check_table(t, T, "types, moments %s" % moments)
        assert np.array_equal(t["hmax"], T["hmax"]), ("moments", moments, np.flatnonzero(t["hmax"] != T["hmax"])[:5])
    # the level-ordered copy exists: a second set of smoothing lengths refreshes both
    D = engine.tree_export_derived()
    assert np.array_equal(D["hmaxB"], T["hmax"][D["dfs_of_bfs"]])
    T2 = TR.restate(S["pos"], S["mass"], S["box"], None, 0, S["type"], S["hsml2"], S["hact"])
    H2 = torch.from_numpy(excluded(S, S["hsml2"])).cuda()
    engine.dev_force_tree_calc_hmax(hsml=H2)
    engine.synchronize()
    t, D = engine.tree_export(), engine.tree_export_derived()
    assert not np.array_equal(T2["hmax"], T["hmax"])
    assert np.array_equal(t["hmax"], T2["hmax"])
    assert np.array_equal(D["hmaxB"], t["hmax"][D["dfs_of_bfs"]])
    assert D["geoS"] is None and D["hsmaxS"] is None and D["srcL"] is None       # the read-out creates neither
    del keep


@pytest.mark.parametrize("mask", [1, 1 + 32, 2])
def test_tree_of_a_type_mask(pkg, engine, mask):
    S, T = TR.scene("types"), TR.reference("types", mask=mask, garbage=True)
    th = host_build(pkg, engine, S, mask=mask, garbage=True)
    check_table(th, T, "types mask %d" % mask)
    TR.gate_moments(T, th["mass"], th["cofm"], "types mask %d GPU" % mask, exact_single=True)
    keep = dev_build(engine, S, mask=mask, garbage=True)
    same_bytes(th, engine.tree_export(), "types mask %d" % mask)
    del keep


def test_tree_of_an_include_list(pkg, engine):
    S = TR.scene("types")
    rng = np.random.RandomState(3)
    act = np.sort(rng.choice(len(S["pos"]), 600, replace=False)).astype(np.int32)
    act = np.union1d(act, np.r_[S["marks"]["pile"], S["marks"]["ninth"]]).astype(np.int32)
    T = TR.restate(S["pos"], S["mass"], S["box"], act)
    engine.force_tree_active_moments(particles(pkg, S), S["box"], ActiveParticle=act)
    t = engine.tree_export()
    check_table(t, T, "include list")
    TR.gate_moments(T, t["mass"], t["cofm"], "include list GPU", exact_single=True)


# ------------------------------------------------------------------------------------------- e: level order, search geometry, leaf blocks
def check_level_order(t, D, T, label):
    bfs = D["dfs_of_bfs"].astype(np.int64)
    assert np.array_equal(bfs, T["dfs_of_bfs"]), label
    lv = t["level"][bfs]
    assert np.all(np.diff(lv) >= 0)
    L = D["linkB"]
    internal = T["pcount"][bfs] == 0
    if T["n"] == 0:
        internal[:] = False
    assert np.array_equal(L[:, 1], np.where(internal, T["nchild"][bfs], 0)), label
    assert np.array_equal(L[:, 0], T["firstchild"][bfs]), (label, "firstchild / merge counts", np.flatnonzero(L[:, 0] != T["firstchild"][bfs])[:5])
    for i in np.flatnonzero(internal):                       # the children are contiguous from firstchild, in pre-order's octant order
        assert np.array_equal(bfs[L[i, 0]:L[i, 0] + L[i, 1]], T["children"][bfs[i]]), (label, i)
    assert np.array_equal(L[:, 2], t["pstart"][bfs]) and np.array_equal(L[:, 3], t["pcount"][bfs])
    assert np.array_equal(D["geoB"], np.c_[t["center"], t["len"]][bfs])
    assert np.array_equal(D["momB"], np.c_[t["cofm"], t["mass"]][bfs])


def test_level_order_and_search_geometry(pkg):
    import torch
    from test_gpu_sph import gpu_arrays, make_times
    import search_scenes as SC
    S, T = TR.scene("types"), TR.reference("types", mask=1)
    N = len(S["pos"])
    rng = np.random.RandomState(8)
    eng = pkg.Engine(0)
    try:
        eng.set_gravshort_treepar(FractionalGravitySoftening=1.0)
        eng.gravshort_set_softenings(1e-3 / 2.8)
        eng.set_densitypar(1.0, 2.0, 2.0, 99999., pkg.engine.DENSITY_KERNEL_CUBIC_SPLINE, 0.006)
        eng.set_hydropar(0, 100.0, SC.ALPHA)
        tm = make_times(pkg, atime=SC.ATIME, hubble=SC.HUBBLE, dloga_bin=[SC.DLOGA] + [0.0] * 46)
        a, keep = gpu_arrays(torch, np.array(S["pos"]), np.array(S["mass"]), np.array(S["type"]), np.array(S["hsml"]), rng.normal(0, 1, (N, 3)), np.ones(N))
        eng.dev_bind_particles(keep["pos"], keep["mass"], S["box"], type=keep["type"])
        eng.dev_force_tree_rebuild_mask(pkg.engine.GASMASK, with_moments=True)
        eng.dev_density(a, tm, update_hsml=0)
        eng.dev_force_tree_calc_hmax()
        eng.dev_hydro_force(a, tm)
        eng.synchronize()
        t, D = eng.tree_export(), eng.tree_export_derived()
    finally:
        eng.close()
    check_table(t, T, "types gas tree")
    check_level_order(t, D, T, "types gas tree")
    # hmax of the gas tree from the caller's radii: every gas particle counts (nothing was handed over as hydro-active)
    Tall = TR.restate(S["pos"], S["mass"], S["box"], TR.scene_members(S, 1), 0, S["type"], S["hsml"], None)
    assert np.array_equal(t["hmax"], Tall["hmax"]) and np.array_equal(D["hmaxB"], t["hmax"][D["dfs_of_bfs"]])
    assert D["geoS"] is not None and D["hsmaxS"] is not None
    pad = 1e-13 * S["box"]
    FACT1 = 0.366025403785
    for i, j in enumerate(D["dfs_of_bfs"]):
        p = S["pos"][T["allmem"][j]]
        c, ln = D["geoS"][i, :3], D["geoS"][i, 3]
        # cull_mask with a target ON the particle and radius 0: dist = 0.5 len, culled if max |c - p| > dist or r2 > (dist + FACT1 len)^2
        d = c - p
        dist = 0.0 + 0.5 * ln
        d2 = dist + FACT1 * ln
        assert not np.any(np.abs(d).max(1) > dist) and not np.any((d * d).sum(1) > d2 * d2), ("geoS does not hold its particles", i)
        assert ln <= (p.max(0) - p.min(0)).max() + 2 * pad, ("geoS wider than its particles", i)
        assert D["hsmaxS"][i] == max(0.0, S["hsml"][T["allmem"][j]].max()), ("hsmaxS", i)


def test_leaf_blocks_after_a_split_walk(pkg, engine):
    S, T = TR.scene("deep"), TR.reference("deep")
    box = S["box"]
    engine.gravshort_fill_ntab(0, 1.5)
    engine.gravpm_init_periodic(box, 1.5, 32, G)
    engine.set_gravshort_treepar(TreeUseBH=2, Rcut=6.0)
    engine.gravshort_set_softenings(box / 12)
    engine.set_walk_variant(6)
    try:
        P = particles(pkg, S)
        engine.force_tree_full(P, box)
        engine.grav_short_tree(P)
        t, D = engine.tree_export(), engine.tree_export_derived()
    finally:
        engine.set_walk_variant(0)
    check_table(t, T, "deep")
    check_level_order(t, D, T, "deep")
    assert D["srcL"] is not None
    want, leaf = TR.leaf_blocks(T, S["pos"], S["mass"], t["order"])
    assert np.array_equal(D["srcL"][:-1][leaf], want[:-1][leaf])
    for i in np.flatnonzero(leaf):
        assert np.all(D["srcL"][i, T["pcount"][D["dfs_of_bfs"][i]]:, 3] == 0)
    assert np.all(D["srcL"][-1] == 0)


# ------------------------------------------------------------------------------------------- f: the top of a decomposed tree
def cell_sums_all_levels(pos, mass, box, La):
    """levels 0 .. La - 1 concatenated, 4 doubles per cell: the long-double sums of ALL particles, rounded once"""
    allp = np.arange(len(pos))
    return np.concatenate([TR.level_cell_sums(pos, mass, box, l + 1, allp)[0].astype(np.float64) for l in range(La)])


@pytest.mark.parametrize("La", [2, 3])
def test_top_of_a_decomposed_tree(pkg, engine, La):
    import torch
    S = TR.scene("deep_nopiles")
    N, box = len(S["pos"]), S["box"]
    n_own = N // 2
    T = TR.reference("deep_nopiles", minlevel=La)
    assert T["level"][T["pcount"] > 0].min() >= La and T["kc"][T["level"] < La].min() >= 3
    rng = np.random.RandomState(La)
    digits = TR.octant_digits(S["pos"], box)
    along_keys = np.lexsort(digits.T[::-1])                   # caller order along the keys: whole waves are own or not
    scattered = rng.permutation(N)                           # own and ghost particles mixed in every wave
    engine.dev_force_tree_set_min_leaf_level(La)
    try:
        for label, perm in (("own particles a prefix along the keys", along_keys), ("own and ghost interleaved", scattered)):
            pos, mass = np.ascontiguousarray(S["pos"][perm]), np.ascontiguousarray(S["mass"][perm])
            keep = bind(engine, S, pos=pos, mass=mass)
            engine.dev_force_tree_build(63)
            engine.synchronize()
            t = engine.tree_export()
            Tp = TR.restate(pos, mass, box, None, La)
            check_table(t, Tp, "La %d, %s" % (La, label))
            for k in ("level", "center", "len", "pcount", "sibling"):
                assert np.array_equal(Tp[k], T[k])            # (the same tree whatever the caller order)
            out = torch.full((8 ** (La - 1), 4), -1.0, dtype=torch.float64, device="cuda")
            engine.dev_tree_top_partial(La, n_own, out)
            engine.synchronize()
            ref, ab, cnt = TR.level_cell_sums(pos, mass, box, La, np.arange(n_own))
            err = np.abs(out.cpu().numpy().astype(np.longdouble) - ref)
            bound = cnt[:, None] * np.longdouble(TR.U) * ab   # n particles: one product and n - 1 additions per component
            print("La %d, %s: worst %.3g of the sum bound" % (La, label, float(np.max(np.where(bound > 0, err / np.where(bound > 0, bound, 1), 0)))))
            assert np.all(err <= bound), (La, label)
            assert cnt.sum() == n_own and (cnt > 0).sum() > 1
            # top_set with the sums of all particles
            sums = torch.from_numpy(cell_sums_all_levels(pos, mass, box, La)).cuda()
            engine.dev_tree_top_set(La, sums)
            engine.synchronize()
            t2 = engine.tree_export()
            above = np.flatnonzero(Tp["level"] < La)
            below = np.flatnonzero(Tp["level"] >= La)
            TR.gate_moments(Tp, t2["mass"], t2["cofm"], "La %d top_set" % La, sel=above)
            assert np.array_equal(t2["mass"][below], t["mass"][below]) and np.array_equal(t2["cofm"][below], t["cofm"][below])
            TR.gate_moments(Tp, t["mass"], t["cofm"], "La %d local moments" % La, exact_single=True)
            del keep
        # a natural leaf above the decomposition level: the particle set of that cell may be incomplete on a rank
        engine.dev_force_tree_set_min_leaf_level(0)
        S9 = TR.scene("tiny9")
        keep = dev_build(engine, S9)
        assert engine.tree_export()["level"].max() < La
        with pytest.raises(pkg.EngineError, match="coarser level"):
            engine.dev_tree_top_set(La, torch.from_numpy(cell_sums_all_levels(S9["pos"], S9["mass"], box, La)).cuda())
    finally:
        engine.dev_force_tree_set_min_leaf_level(0)


# ------------------------------------------------------------------------------------------- g: refusals
def test_refusals_and_the_build_after_them(pkg, engine):
    S = TR.scene("deep")
    box = S["box"]
    c, ln = TR.cell_of(TR.PILE, box, 21)
    eight = np.tile(TR.PILE, (8, 1))
    ones = np.ones(9, np.float32)
    nine_distinct = c + np.linspace(-0.4, 0.4, 9)[:, None] * ln
    assert len(np.unique(TR.octant_digits(nine_distinct, box), axis=0)) == 1
    with pytest.raises(pkg.EngineError, match="coincident"):
        engine.force_tree_full(pkg.make_particles(nine_distinct, ones), box)
    with pytest.raises(pkg.EngineError, match="coincident"):
        engine.force_tree_full(pkg.make_particles(np.concatenate([eight, c[None] + 0.1 * ln]), ones), box)
    legal = np.concatenate([eight, S["pos"][S["marks"]["ninth"]]])
    engine.force_tree_full(pkg.make_particles(legal, ones), box)
    check_table(engine.tree_export(), TR.restate(legal, ones, box), "eight and the ninth")
    with pytest.raises(pkg.EngineError, match="coincident"):
        engine.force_tree_full(pkg.make_particles(nine_distinct, ones), box)
    check_table(host_build(pkg, engine, TR.scene("blocks700")), TR.reference("blocks700"), "the build after a refusal")
