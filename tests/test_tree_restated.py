"""tests/tree_restated.py without a GPU: every scene forces what it claims, oracle/gravtree_oracle.c builds the restated tree on every
scene (node set and geometry bit for bit, leaf membership, the sibling chain, hmax bit-equal, moments within the derived bound), and the
comparison catches one-line faults - each on a scene that is named here."""
import numpy as np
import pytest

import tree_restated as TR

ALL = [n for n in TR.SCENES]


def leaf_levels(T):
    return T["level"][(T["pcount"] > 0) | (T["n"] == 0)]


def test_deep_forces_its_edges():
    S, T = TR.scene("deep"), TR.reference("deep")
    assert len(S["pos"]) == 1771 and len(S["pos"]) <= 5000
    lv = leaf_levels(T)
    assert lv.max() == TR.MAXLEVEL and lv.min() <= 3
    # a run of >= 10 one-child internal nodes: the way down to the pile
    run = best = 0
    j = T["leaf_of"][S["marks"]["pile"][0]]
    assert T["level"][j] == 21 and T["pcount"][j] == 8 and T["pcount"][T["leaf_of"][S["marks"]["ninth"][0]]] == 1
    assert T["parent"][j] == T["parent"][T["leaf_of"][S["marks"]["ninth"][0]]]
    while j >= 0:
        run = run + 1 if (T["pcount"][j] == 0 and T["nchild"][j] == 1) else 0
        best = max(best, run)
        j = T["parent"][j]
    assert best >= 10, best
    # on a cell's centre: the low octant; one unit in the last place above it: the high one; and the tree USES that decision (the cell
    # is internal, the two particles lie in different children of it)
    for a, (p, q) in enumerate(zip(S["marks"]["on_centre"], S["marks"]["above_centre"])):
        l = list(TR.CENTRE_LEVELS)[a]
        assert T["digits"][p, l] == 0 and T["digits"][q, l] == 7
        assert np.array_equal(T["digits"][p, :l], T["digits"][S["marks"]["pile"][0], :l])
        assert T["level"][T["leaf_of"][p]] > l and T["level"][T["leaf_of"][q]] > l
    assert np.all(S["pos"][S["marks"]["origin"][0]] == 0.0) and np.all(S["pos"][S["marks"]["corner"][0]] == np.nextafter(S["box"], 0))
    assert S["pos"].min() == 0.0 and S["pos"].max() < S["box"]
    for name in ALL:
        assert TR.scene(name)["mass"].min() >= 1e-3 * (1 - 1e-6) and TR.scene(name)["mass"].max() <= 1e3 * (1 + 1e-6)


def test_level_scenes_sit_on_the_short_sort_boundary():
    assert leaf_levels(TR.reference("level10")).max() == 10
    assert leaf_levels(TR.reference("level11")).max() == 11
    # the two particles of octant 0 come in caller order against their key order
    S, T = TR.scene("level10"), TR.reference("level10")
    a, b = S["marks"]["nine"][:2]
    assert T["leaf_of"][a] == T["leaf_of"][b] and a < b
    assert tuple(T["digits"][a]) > tuple(T["digits"][b])


def test_blocks_straddle_a_block_of_256():
    for name, n in (("blocks200", 200), ("blocks512", 512), ("blocks700", 700)):
        T = TR.reference(name)
        assert T["n"] == n
    assert 200 < 256 and 512 % 256 == 0 and 700 > 512 and 700 % 256 not in (0, 1)
    for name in ("blocks512", "blocks700"):
        assert TR.straddles(TR.reference(name)), name
    for name in ("deep", "types"):                            # (and the halo of the leaf-level kernel is crossed in the deep scenes too)
        assert TR.reference(name)["n"] > 6 * 256


def test_types_scene():
    S = TR.scene("types")
    assert set(np.unique(S["type"])) == {0, 1, 5}
    assert S["hsml"].max() / S["hsml"].min() >= 100
    assert 0.25 < S["hact"].mean() < 0.35
    T = TR.reference("types")
    assert T["hmax"][0] > 0 and (T["hmax"] > 0).sum() > 100


def test_refusal():
    S = TR.scene("deep")
    c, ln = TR.cell_of(TR.PILE, S["box"], 21)
    nine = c + np.linspace(-0.4, 0.4, 9)[:, None] * ln
    with pytest.raises(TR.TreeRefusal):
        TR.restate(np.concatenate([S["pos"], nine]), np.ones(len(S["pos"]) + 9, np.float32), S["box"])
    eight = np.tile(TR.PILE, (8, 1))
    TR.restate(np.concatenate([eight, S["pos"][S["marks"]["ninth"]]]), np.ones(9, np.float32), S["box"])
    with pytest.raises(TR.TreeRefusal):
        TR.restate(np.concatenate([eight, c[None] + 0.1 * ln]), np.ones(9, np.float32), S["box"])


def oracle_against_restatement(orc, S, T, mask, label):
    """the comparison of the module docstring; returns the worst ratios of the oracle's moments to the derived bound"""
    typ = S["type"].astype(np.int32) if "type" in S else None
    ot = orc.tree(S["pos"], S["mass"], S["box"], type=typ, hsml=S.get("hsml"), hydro_active=S.get("hact"), mask=mask)
    d = ot.export()
    live = np.flatnonzero(d["live"])
    perm = live[TR.match_by_cell(d["level"][live], d["center"][live], T)]          # restated node j <-> oracle node perm[j]
    assert np.array_equal(d["len"][perm], T["len"])
    assert np.array_equal(np.where(d["childtype"][perm] == 0, d["noccupied"][perm], 0), T["pcount"])
    back = np.full(len(d["live"]) + 1, -1, np.int64)
    back[perm] = np.arange(len(perm))
    fn = d["firstnode"]
    assert np.array_equal(np.where(d["sibling"][perm] >= 0, back[np.maximum(d["sibling"][perm] - fn, 0)], -1), T["sibling"])
    fa = ot.father()
    memb = T["members"]
    assert np.array_equal(back[fa[memb] - fn], T["leaf_of"][memb])
    assert ot.ninserted == T["n"]
    if "hmax" in T:
        assert np.array_equal(d["hmax"][perm], T["hmax"]), label
    return TR.gate_moments(T, d["mass"][perm], d["cofm"][perm], label + " oracle")


@pytest.mark.parametrize("name", ALL)
def test_oracle_builds_the_restated_tree(orc, name):
    S = TR.scene(name)
    oracle_against_restatement(orc, S, TR.reference(name), S.get("mask", 63), name)
    if name == "types":
        for mask in (1, 1 + 32, 2):
            oracle_against_restatement(orc, S, TR.reference(name, mask=mask), mask, "%s mask %d" % (name, mask))


# which scene shows which one-line fault (asserted: each fault changes the restated tree of its scene; none goes unnoticed)
CAUGHT_ON = {"ge": "deep", "direct_centre": "deep", "leaf9": "tiny9", "hmax_own_faces": "types", "hmax_active": "types",
             "sibling_last": "blocks200", "merge_one": "blocks200"}


@pytest.mark.parametrize("fault", TR.FAULTS)
def test_one_line_faults_are_caught(fault):
    name = CAUGHT_ON[fault]
    S, T = TR.scene(name), TR.reference(name)
    try:
        F = TR.restate(S["pos"], S["mass"], S["box"], TR.scene_members(S), 0, S.get("type"), S.get("hsml"), S.get("hact"), fault=fault)
    except TR.TreeRefusal:
        return                                                 # (a fault that makes the scene unbuildable is caught as well)
    diff = TR.differences(T, F)
    print("fault %s on scene %s: differs in %s" % (fault, name, ", ".join(diff)))
    assert diff, (fault, name)
    expect = {"ge": "leaf_of", "direct_centre": "center", "leaf9": "pcount", "hmax_own_faces": "hmax", "hmax_active": "hmax",
              "sibling_last": "sibling", "merge_one": "firstchild"}[fault]
    assert expect in diff, (fault, diff)
    assert not TR.differences(T, TR.restate(S["pos"], S["mass"], S["box"], TR.scene_members(S), 0, S.get("type"), S.get("hsml"), S.get("hact")))
