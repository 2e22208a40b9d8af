"""The short-range walk kernels against tree-free extended-precision sums (tests/walk_restated.py; tests/test_walk_restated.py holds the
CPU oracle to the same references and shows which one-line faults they catch).

Two kinds of case, on the scenes of walk_restated (4385 particles, Box 1: a background with 64 particles of a thousand times the mass, clumps
one softening length across at the centre, over the corner, over a face and at the edge of the face layer, 8 particles in one spot, pairs at
r = h, h / 2 and the table's end to the bit and one unit in the last place beside them):
  pairs  every node open (zero old acceleration) and TreeRcut = 10, where Rcut is the end of the window table: the result is the sum over
         all pairs inside the table, no tree in it.  Nmesh 128 (the periodic wrap hoisted out of the pair loops: interior and face-layer
         targets), the same with MPG_NO_FASTWRAP=1, and Nmesh 40 (Rcut = 0.375 Box, NEAREST() per pair, nodes with Rcut + len >= Box / 2).
  sets   TreeRcut = 6 and given old accelerations, relative and Barnes-Hut criterion, against the set restatement on the engine's OWN
         exported tree; the totals of pair interactions, nodes visited and nodes used unopened over ALL targets must be EQUAL.
The GPU walks every target; accelerations and Potential are compared on the 1313 targets of walk_restated.compared_targets, per target
and component: |a - a_ref| <= tol G S_k, |pot - pot_ref| <= tol G S_pot, tol = 8 x the fp64 oracle's own largest ratio on the scene
(2.56e-14 jitter, 3.36e-14 random; the worst case of a sum of the scene's K = 1127 / 1151 terms is 1.27e-13 / 1.30e-13).
"""
import numpy as np
import pytest

import walk_restated as W

pytestmark = pytest.mark.gpu

SLICE = 1463            # MPG_SPLIT_SLICE: not a multiple of 8, three slices of the 4385 targets


def form(variant, cap=512, off64=False, overlap=False, cpw=1, slice_=None):
    return dict(variant=variant, cap=cap, off64=off64, overlap=overlap, cpw=cpw, slice=slice_)


FORMS = {
    "k1": form(1), "k4": form(4), "k6": form(6),
    "k6_cap40": form(6, cap=40),                          # more than a fifth of the targets overflow: the retry and the cooperative fallback
    "k6_off64": form(6, off64=True),
    "k6_slices": form(6, slice_=SLICE),
    "k6_ov0_cpw0": form(6, overlap=False, cpw=0, slice_=SLICE), "k6_ov0_cpw2": form(6, overlap=False, cpw=2, slice_=SLICE),
    "k6_ov1_cpw0": form(6, overlap=True, cpw=0, slice_=SLICE), "k6_ov1_cpw1": form(6, overlap=True, cpw=1, slice_=SLICE),
    "k6_ov1_cpw2": form(6, overlap=True, cpw=2, slice_=SLICE),
}
# kind: (pairs | sets, Nmesh, Barnes-Hut?, MPG_NO_FASTWRAP?)
KINDS = {
    "pairs128": ("pairs", 128, 0, False), "pairs128_nofastwrap": ("pairs", 128, 0, True), "pairs40": ("pairs", 40, 0, False),
    "sets96_rel": ("sets", 96, 0, False), "sets96_bh": ("sets", 96, 1, False), "sets40_rel": ("sets", 40, 0, False), "sets40_bh": ("sets", 40, 1, False),
}
CASES = [("jitter", f, k) for f in FORMS for k in KINDS] + [("random", f, k) for f in ("k1", "k4", "k6") for k in KINDS]

_EXPORT = {}


def setup_engine(engine, par):
    engine.gravshort_fill_ntab(0, 1.5)
    engine.gravpm_init_periodic(par["box"], 1.5, par["nmesh"], par["G"])
    engine.set_gravshort_treepar(TreeUseBH=par["use_bh"], Rcut=par["rcut"] / (1.5 * par["cellsize"]))
    engine.gravshort_set_softenings(W.MEAN_SEP)
    assert engine.FORCE_SOFTENING() == par["h"]


def particles(pkg, name, old=None):
    S = W.scene(name)
    P = pkg.make_particles(S["pos"], S["mass"])
    if old is not None:
        P["FullTreeGravAccel"][:, 0] = W.G * old          # |FullTreeGravAccel + GravPM| / G is the opening input (gravshort.h:70-80)
    return P


def engine_export(pkg, engine, name):
    """The engine's own tree of the scene, exported once (the tree of the same particles is the same tree every time)"""
    if name not in _EXPORT:
        P = particles(pkg, name)
        engine.force_tree_full(P, W.BOX)
        _EXPORT[name] = engine.tree_export()
    return _EXPORT[name]


class Settings:
    """One kernel form on the engine, every setting put back on the way out"""

    def __init__(self, engine, monkeypatch, f, nofastwrap=False):
        self.engine, self.mp, self.f, self.nofastwrap = engine, monkeypatch, f, nofastwrap

    def __enter__(self):
        e, f = self.engine, self.f
        e.set_walk_variant(f["variant"])
        e.set_walk_list_capacity(f["cap"])
        e.set_walk_offsets64(f["off64"])
        e.set_walk_split_mode(f["overlap"], f["cpw"])
        if f["slice"]:
            self.mp.setenv("MPG_SPLIT_SLICE", str(f["slice"]))
        if self.nofastwrap:
            self.mp.setenv("MPG_NO_FASTWRAP", "1")
        return self

    def __exit__(self, *exc):
        e = self.engine
        e.set_walk_variant(0)
        e.set_walk_list_capacity(512)
        e.set_walk_offsets64(False)
        e.set_walk_split_mode(False, 1)
        e.set_instrumentation(False, False)
        self.mp.delenv("MPG_SPLIT_SLICE", raising=False)
        self.mp.delenv("MPG_NO_FASTWRAP", raising=False)
        return False


def reference(pkg, engine, name, kind, rho0=0.0):
    """(par, old accelerations or None, reference) of a kind of case"""
    what, nmesh, use_bh, _ = KINDS[kind]
    if what == "pairs":
        par, ref = W.pairs_reference(name, nmesh, rho0)
        return par, None, ref
    par, old, ref = W.sets_reference(engine_export(pkg, engine, name), name, nmesh, use_bh, "engine")
    assert ref["margin_all"] >= W.MIN_MARGIN        # every predicate of every target is at least 1e-9 from its threshold on this tree too
    return par, old, ref


def host_walk(pkg, engine, name, par, old, count=False):
    """grav_short_tree, the host-pointer form: (accelerations, Potential, counters or None)"""
    setup_engine(engine, par)
    P = particles(pkg, name, old)
    P["Potential"] = 0.5
    engine.set_instrumentation(False, count)
    engine.force_tree_full(P, W.BOX)
    engine.grav_short_tree(P, rho0=par["rho0"])
    c = engine.walk_counters() if count else None
    return P["FullTreeGravAccel"], P["Potential"], c


def totals(c):
    return (c["pp"], c["nodes_visited"], c["nodes_used"])


@pytest.mark.parametrize("name,fname,kind", CASES)
def test_walk_forms(pkg, engine, monkeypatch, name, fname, kind):
    """Every kernel form (lane per target 1, cooperative 4, list + evaluation 6 with short lists, 64-bit offsets, three slices, overlap on
    and off, 0 / 1 / 2 chunks per wave) on every wrap form, through the host-pointer entry."""
    what, nmesh, use_bh, nofastwrap = KINDS[kind]
    par, old, ref = reference(pkg, engine, name, kind)
    tg = W.compared_targets(name)
    f = FORMS[fname]
    with Settings(engine, monkeypatch, f, nofastwrap):
        a, p, _ = host_walk(pkg, engine, name, par, old)
        choice = engine.walk_choice()
        if what == "sets":
            engine.set_walk_list_capacity(f["cap"])
            _, _, c = host_walk(pkg, engine, name, par, old, count=True)
    if fname == "k6_cap40" and what == "pairs":
        # more than a fifth of the targets did not fit 40 entries (test_cap40_overflow_runs_the_fallback counts them): the list pass ran again
        assert choice[1] > 40
    if what == "sets":
        assert totals(c) == tuple(ref["totals"])
    else:
        assert np.isfinite(a).all() and np.isfinite(p).all()
    W.check(a[tg], p[tg], ref, W.TOL[name], "%s %s %s:" % (name, fname, kind))


@pytest.mark.parametrize("kind", ["pairs128", "pairs40"])
def test_cap40_overflow_runs_the_fallback(pkg, engine, monkeypatch, kind):
    """With the counters on the list pass is not repeated: every target whose lists overflow 40 entries goes to the cooperative kernel -
    more than a fifth of them - and the results hold the same bound."""
    name = "jitter"
    par, old, ref = reference(pkg, engine, name, kind)
    tg = W.compared_targets(name)
    with Settings(engine, monkeypatch, FORMS["k6_cap40"]):
        a, p, c = host_walk(pkg, engine, name, par, old, count=True)
        overflowed = engine.walk_choice()[2]
    assert 5 * overflowed > len(a), overflowed
    assert c["nodes_used"] == 0
    W.check(a[tg], p[tg], ref, W.TOL[name], "%s k6_cap40 counting %s:" % (name, kind))


@pytest.mark.parametrize("kind", ["pairs128", "pairs40"])
@pytest.mark.parametrize("variant", [1, 4, 6])
def test_rho0(pkg, engine, monkeypatch, variant, kind):
    """rho0 != 0: the - 2.8372975 m^(2/3) cbrt(rho0) term of the potential's post-process, in every kernel's epilogue"""
    name = "random"
    par, old, ref = reference(pkg, engine, name, kind, rho0=W.RHO0)
    par0, _, ref0 = reference(pkg, engine, name, kind)
    assert float(np.abs(ref["pot"] - ref0["pot"]).min()) > 1.0
    tg = W.compared_targets(name)
    with Settings(engine, monkeypatch, form(variant)):
        a, p, _ = host_walk(pkg, engine, name, par, old)
    W.check(a[tg], p[tg], ref, W.TOL[name], "%s k%d rho0 %s:" % (name, variant, kind))


@pytest.mark.parametrize("kind,rho0", [("pairs128", W.RHO0), ("pairs40", 0.0), ("sets96_rel", 0.0), ("sets40_bh", 0.0)])
@pytest.mark.parametrize("variant", [1, 6])
def test_device_entry(pkg, engine, monkeypatch, variant, kind, rho0):
    """dev_grav_short_tree: device arrays, the old accelerations handed over as they are"""
    import torch
    name = "jitter"
    what = KINDS[kind][0]
    par, old, ref = reference(pkg, engine, name, kind, rho0=rho0)
    tg = W.compared_targets(name)
    S = W.scene(name)
    N = len(S["pos"])
    dev = torch.device("cuda", 0)
    d_pos, d_mass = torch.from_numpy(S["pos"].copy()).to(dev), torch.from_numpy(S["mass"].copy()).to(dev)
    d_old = torch.from_numpy(np.zeros(N) if old is None else old.copy()).to(dev)
    acc = torch.full((N, 3), float("nan"), dtype=torch.float64, device=dev)
    pot = torch.full((N,), float("nan"), dtype=torch.float64, device=dev)
    with Settings(engine, monkeypatch, form(variant)):
        setup_engine(engine, par)
        engine.dev_bind_particles(d_pos, d_mass, W.BOX)
        engine.dev_force_tree_build()
        engine.dev_grav_short_tree(acc, oldacc=d_old, potential=pot, rho0=rho0)
        torch.cuda.synchronize()
        a, p = acc.cpu().numpy(), pot.cpu().numpy()
        if what == "sets":
            setup_engine(engine, par)
            engine.set_instrumentation(False, True)
            engine.dev_grav_short_tree(acc, oldacc=d_old, potential=pot, rho0=rho0)
            torch.cuda.synchronize()
            assert totals(engine.walk_counters()) == tuple(ref["totals"])
    W.check(a[tg], p[tg], ref, W.TOL[name], "%s k%d device entry %s:" % (name, variant, kind))


def target_list(name, n):
    """n targets, the first chunk of 8 holding a clump target over the corner, an interior target and a face-layer target; the compared
    targets come first (a seeded order), the rest of the particles fill up"""
    S = W.scene(name)
    tg = W.compared_targets(name)
    pos = S["pos"]
    layer = W.near_face(pos, W.RCUT_FAST + W.FACE_MARGIN * W.BOX)
    back = tg[~S["deco"][tg]]
    head = [int(S["tags"]["clump_corner"][0]), int(back[~layer[back]][0]), int(back[layer[back]][0])]
    rng = np.random.RandomState(5)
    rest = np.setdiff1d(tg, head)
    others = np.setdiff1d(np.arange(len(pos)), tg)
    order = np.r_[head, rng.permutation(rest), rng.permutation(others)]
    assert len(np.unique(order)) == len(pos)
    return order[:n].astype(np.int32)


@pytest.mark.parametrize("n", [1, 7, 8, 9, 63, 64, 65, 4095, 4096])
def test_target_lists(pkg, engine, monkeypatch, n):
    """ActiveParticle + AccelStore with the default kernel choice: the lane-per-target kernel below 4096 targets, the two-kernel walk from
    4096 on; ragged last chunks and waves; a chunk of 8 that mixes an interior, a face-layer and a clump target (one `wrapped` flag per
    wave of 8).  Rows of the store that are no targets stay as they were."""
    name = "jitter"
    par, old, ref = reference(pkg, engine, name, "pairs128")
    tg = W.compared_targets(name)
    act = target_list(name, n)
    with Settings(engine, monkeypatch, form(0)):
        setup_engine(engine, par)
        P = particles(pkg, name)
        before = np.random.RandomState(9).standard_normal((len(P), 3))
        P["FullTreeGravAccel"] = 0.0
        P["Potential"] = 0.5
        store = before.copy()
        engine.force_tree_full(P, W.BOX)
        engine.grav_short_tree(P, ActiveParticle=act, AccelStore=store)
        assert engine.walk_choice()[0] == (1 if n < 4096 else 6)
    inactive = np.setdiff1d(np.arange(len(P)), act)
    assert np.array_equal(store[inactive], before[inactive])
    assert np.all(P["FullTreeGravAccel"][inactive] == 0.0)
    cmp_ = np.intersect1d(act, tg)
    assert len(cmp_) == min(n, len(tg))
    rows = np.searchsorted(tg, cmp_)
    sub = {k: ref[k][rows] for k in ("acc", "pot", "S", "S_pot")}
    assert np.isfinite(store[act]).all()
    W.check(store[cmp_], P["Potential"][cmp_], sub, W.TOL[name], "%s %d targets:" % (name, n))
    W.check(P["FullTreeGravAccel"][cmp_], P["Potential"][cmp_], sub, W.TOL[name], "%s %d targets, P:" % (name, n))
