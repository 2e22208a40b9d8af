"""The CPU oracle's short-range walk (oracle/gravtree_oracle.c) against the tree-free extended-precision sums of tests/walk_restated.py,
and what those sums catch.  No GPU: this file says that the references and the scenes mean what tests/test_gpu_walk_restated.py takes
them to mean, and records the oracle's own distance from them - the figure the GPU bound is taken from (walk_restated.ORACLE_RATIO).

Measured here (largest |delta| / (G S) of the fp64 oracle over the compared targets, accelerations / potential):
  all pairs, every node open, TreeRcut 10     jitter  Nmesh 128  2.01e-15 / 7.3e-16    Nmesh 40  3.14e-15 / 2.57e-15   (Nmesh 24: 6.74e-15 / 4.97e-15)
                                              random  Nmesh 128  2.34e-15 / 6.9e-16    Nmesh 40  4.13e-15 / 2.85e-15
  sets, TreeRcut 6, relative and Barnes-Hut   jitter  <= 3.06e-15 / 2.71e-15           random  <= 2.71e-15 / 2.09e-15
  recorded: ORACLE_RATIO = 3.2e-15 (jitter), 4.2e-15 (random); tol = 8 x that = 2.56e-14, 3.36e-14; worst case of K = 1127 / 1151 terms 1.27e-13 / 1.30e-13
With S taken WITHOUT the conditioning of the window interpolation (walk_restated's docstring) the same oracle shows 9.0e-14 (jitter) and
8.3e-14 (random) at Nmesh 128, above the worst case (K + 16) 2^-53 = 1.3e-14 of a sum of its K = 97 terms: a particle a thousand times
heavier than the rest, near the table's end, is most of such a target's sum, and one rounding of r moves its window value by 150 roundings.
"""
import os
import shutil
import subprocess

import numpy as np
import pytest

import walk_restated as W
from oracle import oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCENES = sorted(W.SCENE_SEEDS)


def oracle_params(par):
    op = O.make_grav_params(par["box"], par["nmesh"], mean_sep=W.MEAN_SEP, TreeRcut=par["rcut"] / (1.5 * par["cellsize"]),
                            TreeUseBH=par["use_bh"], G=par["G"], rho0=par["rho0"])
    op.Rcut = par["rcut"]
    assert op.h == par["h"] and op.cellsize == par["cellsize"]
    return op


_TREES = {}


def oracle_tree(o, name):
    if (id(o), name) not in _TREES:
        S = W.scene(name)
        tr = o.tree(S["pos"], S["mass"], W.BOX)
        _TREES[(id(o), name)] = (tr, W.export_from_oracle(tr.export()))
    return _TREES[(id(o), name)]


def oracle_all_open(o, name, nmesh, rho0=0.0, nback=1024):
    par, ref = W.pairs_reference(name, nmesh, rho0, nback)
    tr, _ = oracle_tree(o, name)
    a, p, c, _ = tr.grav_short_tree(oracle_params(par), oldacc=np.zeros(tr.N), want_pot=True)
    return a, p, c, ref, W.compared_targets(name, nback)


def oracle_sets(o, name, nmesh, use_bh, export=None):
    """export: the node table the restatement works on (default: this oracle's own; a mutant is judged on the unmutated oracle's)"""
    tr, ex = oracle_tree(o, name)
    par, old, ref = W.sets_reference(ex if export is None else export, name, nmesh, use_bh, "oracle")
    a, p, c, _ = tr.grav_short_tree(oracle_params(par), oldacc=old, want_pot=True)
    return a, p, c, ref, W.compared_targets(name)


# ---- the scenes mean what they claim --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SCENES)
def test_scene_conditions(orc, name):
    S = W.scene(name)
    pos, mass, tags = S["pos"], S["mass"], S["tags"]
    N = len(pos)
    assert 4000 <= N <= 5000 and N % 8 != 0
    assert mass.dtype == np.float32 and (mass[S["heavy"]] >= 1000).all() and len(S["heavy"]) == 64
    light = np.setdiff1d(np.arange(N), S["heavy"])
    assert mass[light].min() >= 1 and mass[light].max() < 2
    _, ex = oracle_tree(orc, name)
    # FASTWRAP's conditions at Nmesh 128 (engine.hip: Rcut + 1.5 maxleaf < 0.49 Box, Rcut < 0.2 Box), from the exported tree
    minleaf = int(ex["level"][ex["pcount"] > 0].min())
    assert minleaf >= 3
    maxleaf = 1.001 * W.BOX / (1 << minleaf)
    for nmesh, fast in ((128, True), (40, False)):
        rcut = W.make_par(nmesh, W.TREE_RCUT_OPEN)["rcut"]
        assert ((rcut + 1.5 * maxleaf < 0.49 * W.BOX) and (rcut < 0.2 * W.BOX)) == fast
    assert (W.make_par(40, W.TREE_RCUT_OPEN)["rcut"] + ex["len"] >= 0.5 * W.BOX).sum() > 8       # nodes with Rcut + len >= Box / 2
    # interior (plain differences) and face-layer targets both exist among the compared ones, the layer at least half of the background
    tg = W.compared_targets(name)
    layer = W.near_face(pos[tg], W.RCUT_FAST + W.FACE_MARGIN * W.BOX)
    back = ~S["deco"][tg]
    assert back.sum() == 1024 and (layer & back).sum() >= 512 and (~layer & back).sum() >= 256
    assert S["deco"][tg].sum() == S["deco"].sum() == N - W.NGRID ** 3
    # decorations: what each is there for
    h = W.H_SOFT
    for tag in ("clump_centre", "clump_corner", "clump_face", "clump_edge"):
        p = pos[tags[tag]]
        d = p[:, None, :] - p[None, :, :]
        d -= np.rint(d)
        r = np.sqrt((d ** 2).sum(-1))[np.triu_indices(len(p), 1)]
        assert (r < h).sum() > 200 and (r < 0.5 * h).sum() > 50, (tag, (r < h).sum(), (r < 0.5 * h).sum())
    assert near_both_sides(pos[tags["clump_corner"]], 3) and near_both_sides(pos[tags["clump_face"]], 1)
    assert len(np.unique(pos[tags["group8"]], axis=0)) == 1 and len(tags["group8"]) == 8
    a, b = pos[tags["close_pair"]]
    assert 0 < abs(b[0] - a[0]) < 2e-12 * h and (a[1:] == b[1:]).all()
    for tag, r in (("r_h", h), ("r_h_below", np.nextafter(h, 0)), ("r_h_above", np.nextafter(h, 1)), ("r_half", 0.5 * h),
                   ("r_half_below", np.nextafter(0.5 * h, 0)), ("r_half_above", np.nextafter(0.5 * h, 1))):
        a, b = pos[tags[tag]]
        assert a[0] == 0.0 and b[0] - a[0] == r and (a[1:] == b[1:]).all()
    assert (0.5 * h) / h == 0.5
    for nmesh in W.PAIR_MESHES:
        rend = W.table_end(W.make_par(nmesh, W.TREE_RCUT_OPEN))
        a, b = pos[tags["end%d_in" % nmesh]]
        assert 1 - 2e-9 < (b[1] - a[1]) / rend < 1 - 5e-10
        a, b = pos[tags["end%d_out" % nmesh]]
        assert 1 + 5e-10 < (b[1] - a[1]) / rend < 1 + 2e-9
    assert pos[tags["top"]][0, 0] == np.nextafter(W.BOX, 0) and (pos[:, 0] == 0.0).sum() >= 7
    a, b = pos[tags["half_box"]]
    assert b[0] - a[0] == 0.5 * W.BOX


def near_both_sides(p, naxes):
    """the clump has particles on both sides of the face x = 0 (naxes = 1) or of all three faces through the corner (naxes = 3)"""
    return all((p[:, k] < 0.1).any() and (p[:, k] > 0.9).any() for k in range(naxes))


# ---- the oracle against the references ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rho0", [0.0, W.RHO0])
@pytest.mark.parametrize("nmesh", W.PAIR_MESHES)
@pytest.mark.parametrize("name", SCENES)
def test_all_pairs_vs_oracle(orc, name, nmesh, rho0):
    """Every node open (zero old acceleration), TreeRcut = 10: the walk's result is the sum over all pairs inside the table, no tree in it."""
    a, p, c, ref, tg = oracle_all_open(orc, name, nmesh, rho0)
    assert c[2] == 0 and c[0] >= ref["partners"].sum()        # no node used unopened; every partner is among the particles met
    if rho0:
        assert np.abs(p - oracle_all_open(orc, name, nmesh, 0.0)[1]).min() > 1.0      # the cbrt(rho0) term is there
    W.check(a[tg], p[tg], ref, W.ORACLE_RATIO[name], "%s Nmesh %d rho0 %g oracle:" % (name, nmesh, rho0))


def test_all_pairs_half_box_pair(orc):
    """Nmesh 24: the table ends at 0.625 Box, so a pair exactly Box / 2 apart contributes and NEAREST()'s behaviour there shows (x = +Box/2
    stays, seen from the other side x = -Box/2 stays: the two pull each other in opposite directions).  Decorations + 128 of the background."""
    a, p, c, ref, tg = oracle_all_open(orc, "jitter", 24, 0.0, nback=128)
    S = W.scene("jitter")
    i, j = S["tags"]["half_box"]
    par = W.make_par(24, W.TREE_RCUT_OPEN)
    term = W.pair_terms(np.array([[0.5, 0, 0]], W.LD), S["mass"][[j]], par["h"], par["cellsize"], par["tab_dx"], par["tab_force"], par["tab_pot"])[0]
    assert float(term[0, 0]) * par["G"] > 100 * W.TOL["jitter"] * float(ref["S"][np.searchsorted(tg, i), 0])
    W.check(a[tg], p[tg], ref, W.ORACLE_RATIO_HALF_BOX, "jitter Nmesh 24 oracle:")


@pytest.mark.parametrize("use_bh", [0, 1])
@pytest.mark.parametrize("nmesh", W.SET_MESHES)
@pytest.mark.parametrize("name", SCENES)
def test_tree_sets_vs_oracle(orc, name, nmesh, use_bh):
    """Production settings (TreeRcut = 6, given old accelerations), relative and Barnes-Hut criterion: the three counters EQUAL, the sums per
    target within the oracle's figure, every predicate of every target at least 1e-9 from its threshold, nothing excluded."""
    a, p, c, ref, tg = oracle_sets(orc, name, nmesh, use_bh)
    print("counters oracle", tuple(c), "sets", tuple(ref["totals"]), "margin %.2e" % ref["margin_all"])
    assert tuple(c) == tuple(ref["totals"])
    assert ref["margin_all"] >= W.MIN_MARGIN and ref["margin"].min() >= W.MIN_MARGIN
    if use_bh:
        assert c[2] > 100
    else:
        assert 4 * c[2] >= c[0], c          # nodes used unopened: at least a quarter of the pair interactions
    W.check(a[tg], p[tg], ref, W.ORACLE_RATIO[name], "%s Nmesh %d %s oracle:" % (name, nmesh, "Barnes-Hut" if use_bh else "relative"))


def test_tree_sets_single_target(orc):
    """tree_sets, the per-target form: the same counts as the oracle's per-particle interaction number, sets consistent with them"""
    name, nmesh = "random", 96
    tr, ex = oracle_tree(orc, name)
    par, old, ref = W.sets_reference(ex, name, nmesh, 0, "oracle")
    _, _, _, nin = tr.grav_short_tree(oracle_params(par), oldacc=old, per_particle=True)
    S = W.scene(name)
    for t in (int(S["tags"]["clump_face"][0]), int(S["tags"]["top"][0]), int(W.compared_targets(name)[5])):
        used, parts, counts, margin = W.tree_sets(ex, S["pos"], par, old, t)
        assert counts[0] == nin[t] == len(parts) and counts[2] == len(used) and len(np.unique(parts)) == len(parts) and margin >= W.MIN_MARGIN
        k = np.searchsorted(W.compared_targets(name), t)
        assert tuple(ref["counts"][k]) == counts


@pytest.mark.parametrize("name", SCENES)
def test_tol_below_rounding_bound(name):
    """tol = 8 x the oracle's figure stays below the worst case (K + 16) 2^-53 of a sum of K terms, K the scene's largest partner count"""
    K = max(int(W.pairs_reference(name, nmesh)[1]["partners"].max()) for nmesh in W.PAIR_MESHES)
    print(name, "K", K, "tol %.3e" % W.TOL[name], "bound %.3e" % W.rounding_bound(K))
    assert K > 1000 and W.TOL[name] < W.rounding_bound(K)


# ---- what the bound catches -----------------------------------------------------------------------------------------------------------
MUTATIONS = {   # name: (file, old text, new text, the case that must show it: ("pairs", Nmesh) or ("sets", Nmesh))
    "inner_branch_at_half": ("gravtree_oracle.c", "const double u = r / h;\n        if(u < 0.5)", "const double u = r / h;\n        if(u <= 0.5)", ("pairs", 128)),
    "spline_at_h": ("gravtree_oracle.c", "if(r2 < h * h) {", "if(r2 <= h * h) {", ("pairs", 128)),
    "last_interval_dropped": ("gravtree_oracle.c", "if(tabindex >= NTAB - 1)", "if(tabindex >= NTAB - 2)", ("pairs", 40)),
    "exact_third": ("gravtree_oracle.c", "fac = mass * h3_inv * (10.666666666667 + u * u", "fac = mass * h3_inv * (32.0 / 3 + u * u", ("pairs", 128)),
    "nearest_ge": ("oracle_tree.h", "(((x) > 0.5 * (B)) ?", "(((x) >= 0.5 * (B)) ?", ("pairs", 24)),
    "node_at_centre": ("gravtree_oracle.c", "dx[i] = NEAREST(nop->cofm[i] - inpos[i], Box);", "dx[i] = NEAREST(nop->center[i] - inpos[i], Box);", ("sets", 96)),
    "discard_without_len": ("gravtree_oracle.c", "const double eff_dist = rcut + 0.5 * len;", "const double eff_dist = rcut;", ("pairs", 128)),
}


def mutated_oracle(tmp_path, name):
    """A build of the oracle's sources with one text replacement (None: none), as tests/test_hydro_physics.py::mutated_oracle makes them"""
    d = tmp_path / ("mut_%s" % name)
    d.mkdir()
    srcs = ["gravtree_oracle.c", "sph_oracle.c", "timestep_oracle.c", "fof_oracle.c", "oracle_tree.h"]
    for f in srcs:
        shutil.copy(os.path.join(ROOT, "oracle", f), str(d / f))
    if name is not None:
        fname, old, new, _ = MUTATIONS[name]
        txt = (d / fname).read_text()
        assert txt.count(old) == 1, ("mutation target not found exactly once", name)
        (d / fname).write_text(txt.replace(old, new))
    lib = str(d / "liboracle_mut.so")
    subprocess.check_call(["gcc", "-O2", "-fopenmp", "-std=gnu11", "-fPIC", "-shared", "-Wno-unused-function", "-o", lib] +
                          [str(d / f) for f in srcs if f.endswith(".c")] + ["-lm"])
    o = O.Oracle(lib_path=lib)
    o.fill_ntab(0, 1.5)
    return o


def run_case(o, orc, case, name="jitter"):
    kind, nmesh = case
    if kind == "pairs":
        a, p, _, ref, tg = oracle_all_open(o, name, nmesh, 0.0, nback=128 if nmesh == 24 else 1024)
    else:
        a, p, _, ref, tg = oracle_sets(o, name, nmesh, 0, export=oracle_tree(orc, name)[1])
    return W.ratios(a[tg], p[tg], ref)


@pytest.mark.parametrize("mutant", sorted(MUTATIONS))
def test_mutants_exceed_the_bound(orc, tmp_path, mutant):
    """One changed line of the oracle each: the GPU bound (tol = 8 x the oracle's figure) is exceeded on at least one compared target"""
    o = mutated_oracle(tmp_path, mutant)
    ra, rp = run_case(o, orc, MUTATIONS[mutant][3])
    print(mutant, "largest ratio acc %.3e pot %.3e  tol %.3e" % (ra, rp, W.TOL["jitter"]))
    assert max(ra, rp) > max(W.TOL["jitter"], 8 * W.ORACLE_RATIO_HALF_BOX if MUTATIONS[mutant][3][1] == 24 else 0)


def test_unmutated_build_passes(orc, tmp_path):
    """The same build path without a replacement stays within the oracle's figure on every case the mutants are judged on"""
    o = mutated_oracle(tmp_path, None)
    for case in sorted(set(m[3] for m in MUTATIONS.values())):
        ra, rp = run_case(o, orc, case)
        assert max(ra, rp) <= (W.ORACLE_RATIO_HALF_BOX if case[1] == 24 else W.ORACLE_RATIO["jitter"]), (case, ra, rp)


@pytest.mark.parametrize("mutant", ["inner_branch_at_half", "spline_at_h", "exact_third"])
def test_existing_gate_passes_what_the_bound_rejects(orc, tmp_path, mutant):
    """The gap this file closes: assert_accel_parity of tests/test_gpu_gravity.py (median |da| / |a| <= 1e-12, 99.9 % <= 1e-9, maximum
    <= 2 ErrTolForceAcc <|a|>), given the mutant's accelerations of ALL targets against the unmutated oracle's, passes; the bound does not."""
    from test_gpu_gravity import assert_accel_parity
    case = MUTATIONS[mutant][3]
    o = mutated_oracle(tmp_path, mutant)
    a_mut, p_mut, _, ref, tg = oracle_all_open(o, "jitter", case[1])
    a_ref = oracle_all_open(orc, "jitter", case[1])[0]
    assert not np.array_equal(a_mut, a_ref)
    assert_accel_parity(a_mut, a_ref)
    assert max(W.ratios(a_mut[tg], p_mut[tg], ref)) > W.TOL["jitter"]
