"""The shared neighbour search (csrc/ngb_walk.h: walk_stepk, cull_mask, interior_wave) behind SPH density, SPH hydro, FOF linking, FOF
secondary attachment and the pair-wise gravity check, at its edges, against all-pairs evaluations that contain no tree at all
(tests/sph_paper.py, brute-force pair graphs).  The scenes and what each forces are in tests/search_scenes.py; the conditions that make
them mean it are asserted without a GPU in tests/test_search_scenes.py.

The pin on the search itself is a pair of INTEGERS: the number of neighbours the density loop found and the number of pairs the hydro loop
found, summed over the targets, equal the all-pairs counts (no pair of a scene lies within 1e-9 of a radius, so the counts do not depend
on rounding).  A dropped leaf, a range lost at a pause, a node culled on the wrong image or on the wrong radius changes them.

Tolerances of the fields (none is fitted to the kernels' output).  2e-10 is the project's gate on the published equations (gate_paper),
applied here PER TARGET - relative to a global maximum the clump of scene A, ~600 x denser than its background, would hide an error in a
background target:
  Density, EgyWtDensity       |err_i| <= 2e-10 ref_i                 (sums of positive terms)
  DivVel, CurlVel, HydroAccel, DtEntropy
                              |err_i| <= 2e-10 x (sum of the absolute pair terms)_i, scaled like the sum itself; CurlVel is the norm of a
                              vector of three such sums: the norm of the three bounds
  grad-h factor f = 1 / D     |err_i| <= (2e-10 / D_i) f_i, D = 1 + (H / 3 rho) d rho / dH >= 0.02 (test_search_scenes.py)
  pressure-entropy factor     -E f with E = (H / 3 y) dy / dH a signed sum: 2e-10 x (|E f| / D + sum|terms of E| f), the two rules combined
  MaxSignalVel                1e-12 relative (a maximum, not a sum)
Expected from the arithmetic: (n + 50) 2^-53 of the absolute sums, ~3e-13 at n = 2000 neighbours; the worst measured ratios error / bound
per field and scene are in DESIGN.md (section "The neighbour search at its edges")."""
import numpy as np
import pytest

import search_scenes as SC
from oracle import fof_oracle as F
from oracle import oracle as O
from sph_paper import paper_density
from test_gpu_fof import compare, run_engine
from test_gpu_sph import gpu_arrays, make_times

pytestmark = pytest.mark.gpu

TOL = 2e-10
FIELDS = ("hsml", "density", "egywtdensity", "dhsmlegyfac", "divvel", "curlvel", "hydroacc_out", "dtentropy_out", "maxsignalvel")


def _times(pkg):
    return make_times(pkg, atime=SC.ATIME, hubble=SC.HUBBLE, dloga_bin=[SC.DLOGA] + [0.0] * 46)


def _new_engine(pkg, kernel, pe):
    eng = pkg.Engine(0)
    eng.set_gravshort_treepar(FractionalGravitySoftening=1.0)
    eng.gravshort_set_softenings(1e-3 / 2.8)
    eng.set_densitypar(1.0, 2.0, 2.0, 99999., kernel, 0.006)
    eng.set_hydropar(pe, 100.0, SC.ALPHA)
    return eng


def run_prescribed(pkg, S, kernel, formulation, host=False):
    """density (update_hsml = 0, the scene's radii) -> hmax -> hydro_force on the GPU.  Returns (fields, density stats, hydro stats)."""
    import torch
    pe = 1 if formulation == "pressure" else 0
    N = len(S["pos"])
    eng = _new_engine(pkg, kernel, pe)
    try:
        t = _times(pkg)
        if host:
            z = lambda *s: np.zeros(s)
            a = dict(hsml=S["hsml"].copy(), dthsml=z(N), vel=S["vel"].copy(), entropy=S["ent"].copy(), density=z(N), egywtdensity=z(N),
                     dhsmlegyfac=z(N), divvel=z(N), curlvel=z(N), hydroacc_out=z(N, 3), dtentropy_out=z(N), maxsignalvel=z(N))
            P = pkg.make_particles(S["pos"].copy(), S["mass"].copy(), type=0)
            eng.density(P, S["box"], a, t, update_hsml=0, DoEgyDensity=pe)
            sd = eng.sph_stats()
            eng.hydro_force(P, a, t)
            sh = eng.sph_stats()
            return {k: a[k] for k in FIELDS}, sd, sh
        a, keep = gpu_arrays(torch, S["pos"].copy(), S["mass"].copy(), np.zeros(N, np.int32), S["hsml"], S["vel"].copy(), S["ent"].copy())
        eng.dev_bind_particles(keep["pos"], keep["mass"], S["box"], type=keep["type"])
        eng.dev_force_tree_rebuild_mask(pkg.engine.GASMASK)
        eng.dev_density(a, t, update_hsml=0, DoEgyDensity=pe)
        sd = eng.sph_stats()
        eng.dev_force_tree_calc_hmax()
        eng.dev_hydro_force(a, t)
        sh = eng.sph_stats()
        eng.synchronize()
        return {k: a[k].cpu().numpy() for k in FIELDS}, sd, sh
    finally:
        eng.close()


class Gate:
    """Collects error / bound per field and target; clump and background targets are reported apart."""

    def __init__(self, label, clump):
        self.label, self.clump, self.lines, self.bad = label, clump, [], []

    def field(self, name, err, bound):
        err, bound = np.abs(np.asarray(err, float)), np.asarray(bound, float)
        with np.errstate(divide="ignore", invalid="ignore"):
            ratio = np.where(bound > 0, err / bound, np.where(err > 0, np.inf, 0.0))
        if ratio.ndim > 1:                                   # vectors: the worst component of each target
            ratio = ratio.max(1)
        part = []
        for what, m in (("clump", self.clump), ("background", ~self.clump)):
            if m.any():
                i = np.flatnonzero(m)[np.argmax(ratio[m])]
                part.append("%s worst %.3g of the bound (target %d), %d of %d beyond it" % (what, ratio[i], i, (ratio[m] > 1).sum(), m.sum()))
        line = "%s %s: %s" % (self.label, name, "; ".join(part))
        print(line)
        self.lines.append(line)
        if not np.all(ratio <= 1):
            self.bad.append(line)

    def finish(self):
        assert not self.bad, "\n" + "\n".join(self.bad)


def gate_density_fields(g, Fd, ref, formulation):
    g.field("Density", Fd["density"] - ref["density"], TOL * ref["density"])
    g.field("DivVel", Fd["divvel"] - ref["divvel"], TOL * ref["abs_divvel"])
    g.field("CurlVel", Fd["curlvel"] - ref["curlvel"], TOL * np.linalg.norm(ref["abs_curlvel"], axis=1))
    if formulation == "pressure":
        g.field("EgyWtDensity", Fd["egywtdensity"] - ref["egywtdensity"], TOL * ref["egywtdensity"])
        g.field("DhsmlEgyDensityFactor", Fd["dhsmlegyfac"] - ref["dhsmlegy"],
                TOL * (np.abs(ref["dhsmlegy"]) / ref["graddenom"] + ref["abs_dhsmlegy"]))
    else:
        g.field("DhsmlDensityFactor", Fd["dhsmlegyfac"] - ref["dhsml"], TOL / ref["graddenom"] * np.abs(ref["dhsml"]))


def gate_hydro_fields(g, Fd, ref):
    g.field("HydroAccel", Fd["hydroacc_out"] - ref["hydroacc"], TOL * ref["abs_hydroacc"])
    g.field("DtEntropy", Fd["dtentropy_out"] - ref["dtentropy"], TOL * ref["abs_dtentropy"])
    g.field("MaxSignalVel", Fd["maxsignalvel"] - ref["maxsignalvel"], 1e-12 * ref["maxsignalvel"])


def check_prescribed(pkg, name, kernel, formulation, host=False):
    S = SC.scene(name)
    ref = SC.reference(name, kernel, formulation)
    Fd, sd, sh = run_prescribed(pkg, S, kernel, formulation, host)
    label = "scene %s %s %s-entropy%s" % (name, SC.KERNEL_NAMES[kernel], formulation, " (host forms)" if host else "")
    # ---- the search: the neighbour and pair counts are the all-pairs ones, as integers
    N = len(S["pos"])
    print("%s: density found %d neighbours among %d candidates (all pairs: %d); hydro %d pairs among %d candidates (all pairs: %d)" %
          (label, sd["interactions"], sd["candidates"], ref["nngb"].sum(), sh["interactions"], sh["candidates"], ref["npairs"].sum()))
    assert (sd["iterations"], sd["targets"]) == (1, N), sd
    assert sd["interactions"] == int(ref["nngb"].sum()), (label, "neighbours of the density loop", sd["interactions"], int(ref["nngb"].sum()))
    assert sd["candidates"] >= sd["interactions"]
    assert sh["interactions"] == int(ref["npairs"].sum()), (label, "pairs of the hydro loop", sh["interactions"], int(ref["npairs"].sum()))
    assert sh["candidates"] >= sh["interactions"]
    assert np.array_equal(Fd["hsml"], S["hsml"]), "update_hsml = 0 changed a smoothing length"
    # ---- the sums
    g = Gate(label, S["clump"])
    gate_density_fields(g, Fd, ref, formulation)
    gate_hydro_fields(g, Fd, ref)
    g.finish()


@pytest.mark.parametrize("name,kernel,formulation", SC.SPH_CASES)
def test_density_and_hydro_at_prescribed_radii(pkg, name, kernel, formulation):
    """Scene A: every clump target has > 8 x SPH_LCAP neighbours - phase A must pause on a full leaf list and the walk resume from the LIFO
    - next to background targets with a dozen, in waves on both sides of interior_wave, the last one ragged.  Scene B: radii of ratio 74,
    a third of the hydro pairs outside the target's own radius (found through the symmetric cull on the node's largest Hsml alone), radii
    of 0.45 and 0.7 Box (no interior form; at >= Box / 2 nothing may be culled on one image)."""
    check_prescribed(pkg, name, kernel, formulation)


def test_prescribed_radii_through_the_host_pointer_forms(pkg):
    """Scene A, quintic, through density() / hydro_force() on host arrays: density at prescribed radii (update_hsml = 0) must leave the
    hmax moments hydro_force() needs."""
    check_prescribed(pkg, "A", 2, "density", host=True)


def test_starved_gas_runs_hsml_to_the_box(pkg, orc):
    """Scene C: the Hsml iteration with too few gas particles for any radius against the CPU restatement - pass for pass - and then one
    pass at the final radii (0.65 .. 1 Box: every search on the wrapped form, most at a radius >= Box / 2) against all pairs."""
    import torch
    Cs = SC.scene_c()
    gas = Cs["typ"] == 0
    A, so = SC.scene_c_oracle(orc)
    eng = _new_engine(pkg, 2, 0)
    try:
        a, keep = gpu_arrays(torch, Cs["pos"].copy(), Cs["mass"].copy(), Cs["typ"].copy(), Cs["hsml0"], Cs["vel"].copy(), Cs["ent"].copy())
        eng.dev_bind_particles(keep["pos"], keep["mass"], SC.BOX, type=keep["type"])
        eng.dev_force_tree_rebuild_mask(pkg.engine.GASMASK)
        t = _times(pkg)
        eng.dev_density(a, t, update_hsml=1)
        sd = eng.sph_stats()
        eng.synchronize()
        h = a["hsml"].cpu().numpy()
        rho_iter = a["density"].cpu().numpy()
        assert (sd["iterations"], sd["targets"], sd["interactions"]) == so[:3], (sd, so)
        assert np.abs(h[gas] / A.hsml[gas] - 1).max() <= 1e-12
        assert np.all(h[gas] > 0.5 * SC.BOX) and np.all(h[gas] <= SC.BOX)
        assert np.array_equal(h[~gas], Cs["hsml0"][~gas])
        assert np.abs(rho_iter[gas] / A.density[gas] - 1).max() <= 1e-10
        # one pass at the final radii (a target that ended on a closed bracket was last summed at the radius before it)
        eng.dev_density(a, t, update_hsml=0)
        s0 = eng.sph_stats()
        eng.synchronize()
        Fd = {k: a[k].cpu().numpy()[gas] for k in FIELDS}
    finally:
        eng.close()
    ref = paper_density(Cs["pos"][gas], Cs["mass"][gas], Cs["vel"][gas], Cs["ent"][gas], h[gas], SC.BOX, 2, "density")
    assert np.array_equal(Fd["hsml"], h[gas])
    assert (s0["iterations"], s0["targets"]) == (1, int(gas.sum()))
    assert s0["interactions"] == int(ref["nngb"].sum()) and s0["candidates"] >= s0["interactions"], (s0, int(ref["nngb"].sum()))
    g = Gate("scene C quintic density-entropy", np.zeros(int(gas.sum()), bool))
    gate_density_fields(g, Fd, ref, "density")
    g.finish()


# ---- friends of friends ---------------------------------------------------------------------------------------------------------------
def _link_alone(engine, S, minlen=1):
    """the primaries' linking without the secondary attachment; every particle numbered (min_length 1)"""
    import torch
    from test_gpu_fof import dev
    d = dict(pos=dev(torch, S["pos"].copy()), mass=dev(torch, S["mass"].copy()), ids=dev(torch, S["ids"].copy().view(np.int64)),
             typ=dev(torch, S["typ"].copy()))
    engine.dev_bind_particles(d["pos"], d["mass"], S["box"], type=d["typ"])
    grnr = torch.zeros(len(S["pos"]), dtype=torch.int64, device="cuda")
    engine.dev_fof_fof(d["ids"], S["LL"], minlen, grnr=grnr, secondary=0)
    engine.synchronize()
    return grnr.cpu().numpy()


@pytest.mark.parametrize("llfrac", [0.2, 0.02])
def test_fof_dense_clump_and_gas_attachment(engine, orc, llfrac):
    """FOF scene (i).  LL = 0.2 Box: every primary has > 960 primaries within the linking length (the leaf list fills, the walk resumes), and
    the secondary search of the gas runs at 0.8 Box >= Box / 2.  LL = 0.02 Box: the clump is a core and many fragments, and the label of a
    gas particle shows which primary the search took for its nearest."""
    S = SC.fof_scene_i(llfrac)
    N = len(S["pos"])
    kw = dict(vel=S["vel"].copy(), typ=S["typ"].copy(), hsml=S["hsml"].copy())
    g, G = run_engine(engine, S["pos"].copy(), S["mass"].copy(), S["ids"].copy(), S["box"], S["LL"], 1, **kw)
    go, Go = F.fof_fof(orc, S["pos"], S["mass"], S["ids"], S["box"], S["LL"], 1, vel=S["vel"], type=S["typ"], hsml=S["hsml"])
    compare(g, G, go, Go, S["box"])
    prim = S["typ"] == 1
    # linking alone against the connected components of the brute-force graph
    i, j = SC.link_pairs(S["pos"], S["box"], S["LL"], sel=prim)
    lab = SC.components(N, i, j)
    gl = _link_alone(engine, S)
    assert gl.min() >= 1 and SC.same_partition(gl, lab)
    if llfrac == 0.2:
        assert len(np.unique(lab[prim])) == 1 and len(np.unique(g[prim])) == 1          # the clump is one group
    # every gas particle carries the label of its brute-force nearest primary (none within the last radius: it stays alone)
    gas, near, r1, _ = SC.nearest_primary(S)
    found = r1 <= SC.secondary_radius(S["LL"], 0.4 * SC.BOX)
    assert np.array_equal(g[gas[found]], g[near[found]])
    assert SC.same_partition(g[prim], lab[prim])
    alone = gas[~found]
    assert np.all(_by_grnr(G)["Length"][g[alone] - 1] == 1)
    if llfrac == 0.02:
        assert len(alone) >= 1 and len(np.unique(g[gas[found]])) >= 5                   # several groups receive gas, some gas finds nobody


def _by_grnr(G):
    """The group table (MinID order) indexed by GrNr - 1"""
    o = np.argsort(G["GrNr"])
    assert np.array_equal(G["GrNr"][o], np.arange(1, len(o) + 1))
    return {k: v[o] for k, v in G.items()}


def test_fof_chain_of_bridges_and_unsigned_ids(engine, orc):
    """FOF scene (ii): a chain in which every link is the only connection between its two sides - one lost union splits the group - with
    IDs on both sides of 2^63: MinID is the UNSIGNED minimum and orders the group table."""
    S = SC.fof_scene_ii()
    N = len(S["pos"])
    m = float(S["mass"][0])
    g, G = run_engine(engine, S["pos"].copy(), S["mass"].copy(), S["ids"].copy(), S["box"], S["LL"], 2)
    assert G["Length"].tolist() == [N] and np.all(g == 1)
    assert G["MinID"].dtype == np.uint64 and G["MinID"][0] == S["ids"].min() and G["MinID"][0] < np.uint64(2 ** 63)
    assert abs(G["Mass"][0] / (N * m) - 1) <= 1e-12
    compare(g, G, *F.fof_fof(orc, S["pos"], S["mass"], S["ids"], S["box"], S["LL"], 2), S["box"])
    # the joints are garbage: the 64 rows, all of length 64, numbered by MinID alone
    flags = S["joint"].copy()
    g, G = run_engine(engine, S["pos"].copy(), S["mass"].copy(), S["ids"].copy(), S["box"], S["LL"], 2, flags=flags)
    rows = SC.CHAIN_ROWS
    assert G["Length"].tolist() == [SC.CHAIN_LEN] * rows
    assert np.all(G["MinID"][1:] > G["MinID"][:-1])                                     # unsigned order
    assert np.all(G["MinID"] < np.uint64(2 ** 63))        # every row holds IDs on both sides of 2^63: its signed minimum would be >= 2^63
    assert np.array_equal(G["GrNr"], np.arange(1, rows + 1))                            # ties in Length broken by MinID
    assert np.all(g[flags == 1] == -1) and np.all(g[flags == 0] >= 1)
    assert np.abs(G["Mass"] / (SC.CHAIN_LEN * m) - 1).max() <= 1e-12
    keep = flags == 0
    assert SC.same_partition(g[keep], S["row"][keep])
    umin = np.array([S["ids"][keep & (S["row"] == k)].min() for k in range(rows)])
    assert np.array_equal(np.sort(umin), G["MinID"])
    compare(g, G, *F.fof_fof(orc, S["pos"], S["mass"], S["ids"], S["box"], S["LL"], 2, flags=flags), S["box"])


def test_fof_links_at_exactly_the_linking_length(engine, orc):
    """FOF scene (iii): the link test is inclusive, r2 <= LL^2 (treewalk.c:984-991).  On a lattice whose spacing IS the linking length every
    link sits on the boundary: one group of all; one ulp less and nobody links.  Integer outputs and Mass only - the moments of a group that
    percolates through the periodic box are a convention, not a number to pin."""
    S = SC.fof_scene_iii()
    N = len(S["pos"])
    m = float(S["mass"][0])

    def ints(LL, minlen):
        g, G = run_engine(engine, S["pos"].copy(), S["mass"].copy(), S["ids"].copy(), S["box"], LL, minlen)
        go, Go = F.fof_fof(orc, S["pos"], S["mass"], S["ids"], S["box"], LL, minlen)
        assert np.array_equal(g, go)
        for k in ("MinID", "Length", "GrNr", "LenType"):
            assert np.array_equal(G[k], Go[k]), k
        return g, G

    g, G = ints(S["LL"], 2)
    assert G["Length"].tolist() == [N] and np.all(g == 1) and G["MinID"][0] == S["ids"].min()
    assert abs(G["Mass"][0] / (N * m) - 1) <= 1e-12
    below = np.nextafter(S["LL"], 0)
    g, G = ints(below, 2)
    assert len(G["Length"]) == 0 and np.all(g == -1)
    g, G = ints(below, 1)
    assert len(G["Length"]) == N and np.all(G["Length"] == 1) and np.array_equal(G["MinID"], np.sort(S["ids"]))
    assert np.array_equal(g, np.argsort(np.argsort(S["ids"])) + 1)                      # numbered by MinID
    assert np.abs(G["Mass"] / m - 1).max() <= 1e-12


# ---- the pair-wise short-range gravity check --------------------------------------------------------------------------------------------
def test_grav_short_pair_on_the_clump(pkg, orc):
    """Scene A through grav_short_pair with a cut-off of 0.2 Box: the same search, the same > 960 partners per clump target."""
    from test_gpu_gravity import G as GRAV, assert_accel_parity, setup_engine
    S = SC.scene_a()
    nmesh, n = 32, 13
    rcut = 0.2 * nmesh / 1.5                                # Rcut x Asmth x Box / Nmesh = 0.2 Box
    par = O.make_grav_params(S["box"], nmesh, npart_cbrt=n, G=GRAV, TreeRcut=rcut)
    assert abs(par.Rcut / (0.2 * S["box"]) - 1) <= 1e-15
    a_ref = orc.grav_short_pair(S["pos"], S["mass"], S["box"], par, par.Rcut)
    eng = pkg.Engine(0)
    try:
        setup_engine(eng, S["box"], n, nmesh, TreeUseBH=0, Rcut=rcut)
        P = pkg.make_particles(S["pos"].copy(), S["mass"].copy())
        P["GravPM"] = 0.0
        eng.force_tree_full(P, S["box"])
        eng.grav_short_pair(P, rcut)
        a = P["FullTreeGravAccel"].copy()
    finally:
        eng.close()
    assert_accel_parity(a, a_ref)
    assert_accel_parity(a[S["clump"]], a_ref[S["clump"]])
    assert_accel_parity(a[~S["clump"]], a_ref[~S["clump"]])
