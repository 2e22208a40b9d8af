"""The scenes of tests/search_scenes.py mean what they claim: every condition is asserted here on the reference side alone (numpy over all
pairs, the CPU oracle for scene C), without a GPU.  A scene whose condition fails is a failure, not a skip: the GPU tests of
test_gpu_search_edges.py would then pass without having exercised the path they are named after.  Also here: the blocked (targets= /
chunk=) forms of the all-pairs references equal the dense ones bit for bit."""
import numpy as np
import pytest

import search_scenes as SC
from sph_paper import paper_density, paper_hydro, sph_paper
from test_hydro_physics import gas_state


# ---- the references -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("formulation,kernel", [("density", 2), ("pressure", 1), ("density", 4)])
def test_blocked_references_equal_the_dense_ones(pkg, formulation, kernel):
    pos, mass, vel, ent, box = gas_state(pkg)                 # the 9^3 state of test_hydro_physics.py
    N = len(pos)
    rng = np.random.RandomState(2)
    H = 2.2 * box / 9 * (1 + 0.3 * rng.random_sample(N))
    dl = np.full(N, 0.02)
    dense = sph_paper(pos, mass, vel, ent, H, box, 0.5, 0.3, 0.75, kernel, formulation, dlna=dl)
    # every particle, in ragged blocks
    blk = paper_density(pos, mass, vel, ent, H, box, kernel, formulation, chunk=100)
    blk.update(paper_hydro(pos, mass, vel, ent, H, box, blk, 0.5, 0.3, 0.75, kernel, formulation, dlna=dl, chunk=100))
    assert set(blk) == set(dense)
    for k in dense:
        assert np.array_equal(blk[k], dense[k]), k
    # a subset of the targets, in another order
    t = rng.permutation(N)[:250]
    sub = paper_density(pos, mass, vel, ent, H, box, kernel, formulation, targets=t, chunk=64)
    sub.update(paper_hydro(pos, mass, vel, ent, H, box, dense, 0.5, 0.3, 0.75, kernel, formulation, dlna=dl, targets=t, chunk=64))
    for k in dense:
        assert sub[k].shape[0] == len(t) and np.array_equal(sub[k], dense[k][t]), k


def test_reference_counts_and_absolute_sums(pkg):
    pos, mass, vel, ent, box = gas_state(pkg)
    N = len(pos)
    H = 2.2 * box / 9 * (1 + 0.3 * np.random.RandomState(3).random_sample(N))
    ref = sph_paper(pos, mass, vel, ent, H, box, 0.5, 0.3, 0.75, 2, "pressure", dlna=np.full(N, 0.02))
    r = SC.all_pairs_r(pos, box)
    off = ~np.eye(N, dtype=bool)
    assert np.array_equal(ref["nngb"], (r <= H[:, None]).sum(1)) and ref["nngb"].min() >= 2          # the target itself is one of them
    assert np.array_equal(ref["npairs"], (off & ((r < H[:, None]) | (r < H[None, :]))).sum(1))
    assert np.array_equal(ref["graddenom"], 1.0 / ref["dhsml"]) or np.allclose(ref["graddenom"] * ref["dhsml"], 1.0, rtol=1e-15, atol=0)
    # an absolute sum bounds its signed sum, and by a margin in a disordered state (the terms do cancel)
    assert np.all(ref["abs_divvel"] >= np.abs(ref["divvel"])) and np.median(ref["abs_divvel"] / np.abs(ref["divvel"])) > 2
    assert np.all(np.linalg.norm(ref["abs_curlvel"], axis=1) >= ref["curlvel"])
    assert np.all(ref["abs_hydroacc"] >= np.abs(ref["hydroacc"])) and np.all(ref["abs_dtentropy"] >= np.abs(ref["dtentropy"]))
    assert np.all(ref["abs_dhsmlegy"] >= np.abs(ref["dhsmlegy"]) * (1 - 1e-14))


# ---- scenes A and B -------------------------------------------------------------------------------------------------------------------
def test_scene_a_forces_pause_and_resume_and_both_wrap_forms():
    A = SC.scene_a()
    N = len(A["pos"])
    assert N == 2045 and N % 8 != 0 and N % 64 != 0 and A["clump"].sum() == 1280
    inside = (A["r"] <= A["hsml"][:, None]).sum(1) - 1            # neighbours without the target itself
    # one list entry holds at most 8 particles: a target with more than 8 x SPH_LCAP neighbours cannot finish on one list
    assert inside[A["clump"]].min() > 8 * SC.SPH_LCAP, inside[A["clump"]].min()
    print("scene A: clump targets have >= %d neighbours, background targets %d .. %d" %
          (inside[A["clump"]].min(), inside[~A["clump"]].min(), inside[~A["clump"]].max()))
    geo = SC.interior_geometry(A["pos"], A["hsml"], A["box"])
    print("scene A: interior_wave geometry holds for %d targets, not for %d" % (geo.sum(), (~geo).sum()))
    assert geo.sum() >= 500 and (~geo).sum() >= 500
    assert (~geo & ~A["clump"]).sum() >= 500                       # the wrapped form is the background's


def test_scene_b_mixes_radii_and_has_one_sided_pairs():
    B = SC.scene_b()
    H, r = B["hsml"], B["r"]
    print("scene B: Hsml %.4g .. %.4g, ratio %.1f" % (H.min(), H.max(), H.max() / H.min()))
    assert H.max() / H.min() >= 30
    assert (H == 0.45 * SC.BOX).sum() == 4 and (H == 0.7 * SC.BOX).sum() == 2        # >= Box / 4 and >= Box / 2
    assert np.all((H <= 0.24 * SC.BOX) | (H >= 0.45 * SC.BOX))
    off = ~np.eye(len(H), dtype=bool)
    pair = off & ((r < H[:, None]) | (r < H[None, :]))
    foreign = pair & (r >= H[:, None])                             # [target, neighbour]: a pair only through the neighbour's radius
    print("scene B: %d of %d (target, neighbour) hydro pairs lie outside the target's own radius" % (foreign.sum(), pair.sum()))
    assert foreign.sum() >= 0.2 * pair.sum()
    # ... and not through the six large radii alone
    small = H <= 0.24 * SC.BOX
    assert (foreign & small[None, :]).sum() >= 0.05 * pair.sum()


@pytest.mark.parametrize("name", ["A", "B"])
def test_no_pair_on_a_radius(name):
    """No pair within 1e-9 (relative) of a radius it is tested against - its own Hsml, the neighbour's, the linking length: the neighbour
    and pair COUNTS of the references are then the same integers in any arithmetic that is good to 1e-9, and may be compared exactly."""
    S = SC.scene(name)
    m = SC.radius_margin(S["r"], [S["hsml"], 0.2 * SC.BOX])
    print("scene %s: smallest |r / R - 1| = %.3g" % (name, m))
    assert m >= 1e-9


@pytest.mark.parametrize("name,kernel,formulation", SC.SPH_CASES)
def test_grad_h_denominator_is_bounded_below(name, kernel, formulation):
    """1 + (H / 3 rho) d rho / dH >= 0.02 for every target and every kernel run on the scene: its inverse scales the tolerance of the
    grad-h factor, and a denominator near zero would make that gate meaningless."""
    ref = SC.reference(name, kernel, formulation)
    S = SC.scene(name)
    print("scene %s %s: smallest grad-h denominator %.4g (clump %.4g, background %.4g)" %
          (name, SC.KERNEL_NAMES[kernel], ref["graddenom"].min(), ref["graddenom"][S["clump"]].min(), ref["graddenom"][~S["clump"]].min()))
    assert ref["graddenom"].min() >= 0.02
    # the references are live: viscous pairs, pressure forces, total counts beyond the gentle scenes'
    assert (ref["dtentropy"] > 0).mean() > 0.5 and np.abs(ref["hydroacc"]).max() > 0
    assert ref["nngb"].sum() > 1280 * 8 * SC.SPH_LCAP or name == "B"
    assert np.all(ref["npairs"] >= ref["nngb"] - 1)


def test_scene_c_starves_the_iteration(orc):
    """40 gas particles cannot supply ~113 kernel-weighted neighbours at any radius: density_check_neighbours (density.c:589-689) runs every
    Hsml up until the bracket closes at the box size."""
    Cs = SC.scene_c()
    gas = Cs["typ"] == 0
    assert gas.sum() == 40 and (~gas).sum() == 500
    A, so = SC.scene_c_oracle(orc)
    h = A.hsml[gas]
    print("scene C: %d passes, Hsml %.6g .. %.6g of Box" % (so[0], h.min() / SC.BOX, h.max() / SC.BOX))
    assert np.all(h > 0.5 * SC.BOX) and np.all(h <= SC.BOX)
    assert so[0] >= 5                                               # an iteration, not one pass
    # the counts of a pass at the final radii are exact integers: no gas pair on a radius
    m = SC.radius_margin(SC.all_pairs_r(Cs["pos"][gas], SC.BOX), [h])
    print("scene C: smallest |r / R - 1| at the final radii = %.3g" % m)
    assert m >= 1e-9


# ---- friends of friends ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("llfrac", [0.2, 0.02])
def test_fof_scene_i_conditions(llfrac):
    S = SC.fof_scene_i(llfrac)
    prim, gas = S["typ"] == 1, S["typ"] == 0
    assert prim.sum() == 1280 and gas.sum() == 64 and (S["typ"] == 2).sum() == 765
    r = SC.all_pairs_r(S["pos"], S["box"])
    rpp = r[prim][:, prim]
    # the linking length is on nobody's distance
    assert np.abs(rpp[~np.eye(1280, dtype=bool)] / S["LL"] - 1).min() >= 1e-9
    d = np.sqrt(((S["pos"][gas] - 0.5 * SC.BOX) ** 2).sum(1)) / SC.BOX
    assert d.min() >= 0.1 and d.max() <= 0.3
    rad = SC.secondary_radius(S["LL"], 0.4 * SC.BOX)
    _, _, r1, r2 = SC.nearest_primary(S)
    gap = (r2 / r1 - 1).min()
    print("FOF (i), LL = %g Box: final secondary radius %.4g Box; nearest / second nearest primary differ by >= %.3g" % (llfrac, rad / SC.BOX, gap))
    assert gap > 1e-9 and np.abs(r1 / rad - 1).min() > 1e-9
    if llfrac == 0.2:
        # every primary links to more than 8 x SPH_LCAP primaries; the secondary search runs at a radius >= Box / 2 with as many inside
        assert ((rpp <= S["LL"]).sum(1) - 1).min() > 8 * SC.SPH_LCAP
        assert rad >= 0.5 * SC.BOX
        assert (r[gas][:, prim] <= rad).sum(1).min() > 8 * SC.SPH_LCAP
    else:
        assert abs(rad / (0.2 * SC.BOX) - 1) < 1e-6
        i, j = SC.link_pairs(S["pos"], S["box"], S["LL"], sel=prim)
        lab = SC.components(len(S["pos"]), i, j)[prim]
        size = np.bincount(np.unique(lab, return_inverse=True)[1])
        print("FOF (i), LL = 0.02 Box: %d groups of primaries, the largest %d, %d singles" % (len(size), size.max(), (size == 1).sum()))
        assert len(size) >= 20 and size.max() >= 200
        # gas particles that do find a primary, attached to at least 5 different groups; and some that find none
        found = r1 <= rad
        gidx, near, _, _ = SC.nearest_primary(S)
        full = SC.components(len(S["pos"]), i, j)
        assert found.sum() >= 10 and (~found).sum() >= 1 and len(np.unique(full[near[found]])) >= 5


def test_fof_scene_ii_every_link_is_a_bridge():
    S = SC.fof_scene_ii()
    N = len(S["pos"])
    assert N == SC.CHAIN_ROWS * SC.CHAIN_LEN + SC.CHAIN_ROWS - 1 and S["joint"].sum() == SC.CHAIN_ROWS - 1
    assert np.all(np.ptp(S["pos"], axis=0) < 0.5 * SC.BOX)
    i, j = SC.link_pairs(S["pos"], S["box"], S["LL"])
    assert len(i) == N - 1                                                      # a tree on N vertices ...
    lab = SC.components(N, i, j)
    assert lab.max() == 0                                                       # ... that is connected: every edge is a bridge
    deg = np.bincount(np.r_[i, j], minlength=N)
    assert deg.max() == 2 and (deg == 1).sum() == 2                             # a path
    # without the joints: the 64 rows
    keep = S["joint"] == 0
    i2, j2 = SC.link_pairs(S["pos"], S["box"], S["LL"], sel=keep)
    lab2 = SC.components(N, i2, j2)[keep]
    assert np.array_equal(np.sort(np.bincount(np.unique(lab2, return_inverse=True)[1])), np.full(SC.CHAIN_ROWS, SC.CHAIN_LEN))
    assert SC.same_partition(lab2, S["row"][keep])
    # the IDs
    ids = S["ids"]
    assert len(np.unique(ids)) == N and ids.dtype == np.uint64
    assert abs(int((ids >= np.uint64(2 ** 63)).sum()) - N / 2) <= 1
    assert ids.min() < np.uint64(2 ** 63) and ids.max() == np.uint64(2 ** 64 - 1)
    assert ids.view(np.int64).min() < 0 and np.uint64(ids.view(np.int64).min()) != ids.min()     # the signed minimum is another particle
    # ... in every row: the order of the rows by unsigned MinID differs from the order by signed MinID
    rows = [ids[keep & (S["row"] == k)] for k in range(SC.CHAIN_ROWS)]
    umin = np.array([x.min() for x in rows])
    smin = np.array([x.view(np.int64).min() for x in rows])
    assert not np.array_equal(np.argsort(umin), np.argsort(smin))


def test_fof_scene_iii_neighbours_sit_on_the_linking_length():
    S = SC.fof_scene_iii()
    N = len(S["pos"])
    assert N == 4096 and S["LL"] == 0.5
    i, j = SC.link_pairs(S["pos"], S["box"], S["LL"])
    assert len(i) == 3 * N                                                      # six neighbours each, every one at r2 == LL^2 exactly
    d = S["pos"][i] - S["pos"][j]
    d -= S["box"] * np.rint(d / S["box"])
    assert np.all((d ** 2).sum(1) == S["LL"] ** 2)
    assert SC.components(N, i, j).max() == 0
    below = np.nextafter(0.5, 0)
    assert below < 0.5 and len(SC.link_pairs(S["pos"], S["box"], below)[0]) == 0
