"""The lensing potential planes on the GPU (csrc/planes.hip through the Python binding) against the numpy restatement of write_plane
(planes_restated.py): the integer counts and npart for equality, the potential to 1e-11 of the mean |psi| of each plane - the form and
the number test_pm_parity applies to rocFFT against pocketfft."""
import os
import sys

import numpy as np
import pytest

from conftest import keep_artifacts_on_failure, phase_clock, run_ranks
import planes_restated as R_

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from mgpu_nu_check import synthetic_response, tracer_types  # noqa: E402
from mgpu_planes_check import COSMO, particle_set, plane_args  # noqa: E402

pytestmark = pytest.mark.gpu
G = 43.0071
BOUND = 1e-11


def _dev(pkg, engine, pos, mass, box, ptype=None):
    import torch
    dev = torch.device("cuda", 0)
    t = (torch.from_numpy(np.ascontiguousarray(pos)).to(dev), torch.from_numpy(np.ascontiguousarray(mass)).to(dev),
         None if ptype is None else torch.from_numpy(np.ascontiguousarray(ptype)).to(dev))
    engine.dev_bind_particles(t[0], t[1], box, type=t[2])
    return t


def _np(engine, t):
    engine.synchronize()
    return t.cpu().numpy()


def _assert_planes(got, want, label="", bound=BOUND):
    """max |got - want| over each plane against bound * mean |want| of that plane; prints the largest ratio to the bound"""
    worst = 0.0
    for idx in np.ndindex(want.shape[:2]):
        m = np.abs(want[idx]).mean()
        d = np.abs(got[idx] - want[idx]).max()
        if m == 0:
            assert d == 0, (label, idx)
            continue
        worst = max(worst, d / m)
        assert d <= bound * m, "%s plane %s: max diff %.3g of mean |psi| (bound %.1g)" % (label, idx, d / m, bound)
    print("%s: largest difference %.3g of mean |psi| (bound %.1g)" % (label, worst, bound))
    return worst


def _edge_set(pkg, name, n=32):
    pos, mass, box = getattr(pkg.ics, name)(n)
    edge = np.array([[0.0, 0.3 * box, 0.6 * box], [box, 0.3 * box, 0.6 * box], [0.2 * box, 0.0, box], [0.7 * box, box, 0.0], [0.0, 0.0, 0.0],
                     [box, box, box]])
    return np.concatenate([pos, edge]), np.concatenate([mass, np.ones(len(edge), np.float32)]), box


@pytest.mark.parametrize("ics", ["s_zel", "s_clust"])
@pytest.mark.parametrize("R", [64, 96, 250])
def test_particle_plane_parity(pkg, engine, R, ics):
    pos, mass, box = _edge_set(pkg, ics)
    _dev(pkg, engine, pos, mass, box)
    calls = [("thin", dict(Thickness=0.07 * box, CutPoints=[0.35 * box, 0.02 * box, 0.98 * box],          # inside, across 0, across Box
                           CurrentParticleOffset=(0.1 * box, 0.0, -0.25 * box))),
             ("edges", dict(Thickness=0.25 * box, CutPoints=[0.125 * box, 0.875 * box, box])),             # slabs that start / end at 0 and Box
             ("thick", dict(Thickness=1.25 * box, CutPoints=[0.5 * box, 0.1 * box, 0.9 * box]))]           # thickness >= Box
    for label, kw in calls:
        want = R_.potential_planes(pos, box, R, [0, 1, 2], **COSMO, **kw)
        counts, nact = engine.dev_plane_counts(R, [0, 1, 2], **COSMO, **kw)
        counts = _np(engine, counts).astype(np.int64)
        assert nact == want["n_active"] == len(pos)
        assert counts.shape == want["counts"].shape and np.array_equal(counts, want["counts"]), label     # every pixel of every plane
        planes, npart = engine.dev_potential_planes(R, [0, 1, 2], **COSMO, **kw)
        assert np.array_equal(npart, want["npart"]) and np.array_equal(npart, counts.sum(axis=(2, 3)))
        assert (npart > 0).all()
        if label == "thick":
            assert (npart == len(pos)).all()
        _assert_planes(_np(engine, planes), want["planes"], "%s R %d %s" % (ics, R, label))


def test_activity(pkg, engine):
    """swallowed and garbage rows, and with the tracer switch on type-2 rows, change neither the counts nor the normalisation"""
    import torch
    pos, mass, box = pkg.ics.s_zel(20)
    n = len(pos)
    kw = dict(Thickness=0.3 * box, CutPoints=[0.2 * box, 0.7 * box], **COSMO)
    R = 64
    rng = np.random.RandomState(4)
    extra = box * rng.random_sample((300, 3))
    xpos = np.concatenate([pos, extra])
    xmass = np.concatenate([mass, np.full(300, 7.0, np.float32)])
    flags = np.zeros(len(xpos), np.uint8)
    flags[n:n + 100] = 2          # Swallowed
    flags[n + 100:n + 200] = 1    # IsGarbage
    types = np.ones(len(xpos), np.uint8)
    types[n + 200:] = 2           # hybrid-neutrino tracers
    _dev(pkg, engine, pos, mass, box)
    base, base_n = engine.dev_potential_planes(R, [0, 2], **kw)
    base = _np(engine, base)
    c0 = _np(engine, engine.dev_plane_counts(R, [0, 2], **kw)[0])
    t = _dev(pkg, engine, xpos, xmass, box, types)
    d_flags = torch.from_numpy(flags).to(t[0].device)
    engine.gravpm_set_hybrid_nu_tracer(True)
    try:
        c, nact = engine.dev_plane_counts(R, [0, 2], flags=d_flags, **kw)
        p, npart = engine.dev_potential_planes(R, [0, 2], flags=d_flags, **kw)
        assert nact == n and np.array_equal(npart, base_n) and np.array_equal(_np(engine, p), base)
        assert np.array_equal(_np(engine, c), c0)        # every counter, not only their sums
    finally:
        engine.gravpm_set_hybrid_nu_tracer(False)
    # switch off: type 2 counts
    c2, nact2 = engine.dev_plane_counts(R, [0, 2], flags=d_flags, **kw)
    want = R_.potential_planes(xpos, box, R, [0, 2], flags=flags, ptype=types, tracer=False, **kw)
    assert nact2 == n + 100 == want["n_active"] and np.array_equal(_np(engine, c2).astype(np.int64), want["counts"])
    p2, npart2 = engine.dev_potential_planes(R, [0, 2], flags=d_flags, **kw)
    assert np.array_equal(npart2, want["npart"]) and (npart2 >= base_n).all() and npart2.sum() > base_n.sum()
    _assert_planes(_np(engine, p2), want["planes"], "tracers counted")
    # the host form reads the same two bits from the records
    P = pkg.make_particles(xpos, xmass, type=types)
    P["Flags"] = flags
    ph, nh = engine.potential_planes(P, box, R, [0, 2], **kw)
    assert np.array_equal(nh, want["npart"])
    _assert_planes(ph, want["planes"], "host records with flags")


def test_overlapping_slabs(pkg, engine):
    pos, mass, box = pkg.ics.s_zel(20)
    _dev(pkg, engine, pos, mass, box)
    th = 0.2 * box
    kw = dict(Thickness=th, CutPoints=[0.40 * box, 0.45 * box], **COSMO)
    counts, _ = engine.dev_plane_counts(64, [1], **kw)
    counts = _np(engine, counts).astype(np.int64)
    want = R_.potential_planes(pos, box, 64, [1], **kw)
    assert np.array_equal(counts, want["counts"])
    y = pos[:, 1]
    shared = ((y >= 0.35 * box) & (y < 0.5 * box)).sum()                 # [0.30, 0.50) and [0.35, 0.55)
    union = ((y >= 0.30 * box) & (y < 0.55 * box)).sum()
    assert shared > 0 and counts.sum() == union + shared                 # the shared particles are in both planes


@pytest.mark.parametrize("R", [64, 100])
@pytest.mark.parametrize("nmesh", [32, 48])
def test_neutrino_correction(pkg, engine, nmesh, R):
    pos, mass, box = particle_set(16)
    bmpc = box / 1000.0
    engine.gravpm_init_periodic(box, 1.5, nmesh, G)
    engine.gravpm_set_nu_response(None)
    engine.gravpm_set_hybrid_nu_tracer(False)
    _dev(pkg, engine, pos, mass, box)
    kw = dict(Thickness=0.3 * box, CutPoints=[0.35 * box, 0.05 * box], **COSMO)
    want = R_.potential_planes(pos, box, R, [0, 1, 2], mass=mass, nu_response=synthetic_response([]), nmesh=nmesh, BoxSize_in_MPC=bmpc, **kw)
    plain = want["planes"] - want["correction"]
    # a condition on the input: the restated correction is at least 1e3 times the bound, so the test cannot pass without it
    for idx in np.ndindex(want["planes"].shape[:2]):
        assert np.abs(want["correction"][idx]).max() >= 1e3 * BOUND * np.abs(want["planes"][idx]).mean()
    calls = []
    with_nu, npart = engine.dev_potential_planes(R, [0, 1, 2], nu_response=synthetic_response(calls), BoxSize_in_MPC=bmpc, **kw)
    with_nu = _np(engine, with_nu)
    without, npart0 = engine.dev_potential_planes(R, [0, 1, 2], **kw)
    without = _np(engine, without)
    assert len(calls) == 1 and np.array_equal(npart, want["npart"]) and np.array_equal(npart0, npart)
    for got, ref in zip(calls[0], want["inputs"]):            # the tolerance test_nu_response_parity asks of the same inputs
        assert got.shape == ref.shape and np.abs(got - ref).max() <= 1e-12 * np.abs(ref).max()
    _assert_planes(with_nu, want["planes"], "nmesh %d R %d with correction" % (nmesh, R))
    # the difference of the two GPU calls against the restated correction, to twice the bound (two planes each within it)
    for idx in np.ndindex(want["planes"].shape[:2]):
        d = np.abs((with_nu[idx] - without[idx]) - want["correction"][idx]).max()
        assert d <= 2 * BOUND * np.abs(want["planes"][idx]).mean(), idx
    # a zero ratio gives the uncorrected plane
    zero, _ = engine.dev_potential_planes(R, [0, 1, 2], nu_response=lambda k, d, m: (np.log(k), np.zeros_like(k), 0.07, 1.05), BoxSize_in_MPC=bmpc,
                                          **kw)
    _assert_planes(_np(engine, zero), plain, "zero ratio")
    # a non-zero CurrentParticleOffset shifts the mesh deposit as well (plane.c:103)
    kw2 = dict(kw, CurrentParticleOffset=(0.1 * box, 0.0, -0.25 * box))
    want2 = R_.potential_planes(pos, box, R, [1], mass=mass, nu_response=synthetic_response([]), nmesh=nmesh, BoxSize_in_MPC=bmpc, **kw2)
    off, _ = engine.dev_potential_planes(R, [1], nu_response=synthetic_response([]), BoxSize_in_MPC=bmpc, **kw2)
    _assert_planes(_np(engine, off), want2["planes"], "offset with correction")


@pytest.mark.parametrize("n,nmesh", [(16, 32), (20, 48)])
def test_pm_force_after_planes(pkg, engine, n, nmesh):
    """the PM meshes are scratch during a planes call: the next gravpm_force meets test_pm_parity's assertion against the oracle, and
    gravpm_get_powerspectrum returns the spectrum of that step"""
    from oracle import oracle as O
    pos, mass, box = pkg.ics.s_grid(n)
    pos[0] = [0.0, box, box / 2]
    engine.gravpm_init_periodic(box, 1.5, nmesh, G)
    engine.set_gravshort_treepar(TreeUseBH=0)
    engine.gravshort_set_softenings(box / n)
    engine.gravpm_set_nu_response(None)
    engine.gravpm_set_hybrid_nu_tracer(False)
    P = pkg.make_particles(pos, mass)
    engine.gravpm_force(P)
    spec0 = engine.gravpm_get_powerspectrum(nmesh, box / 1000.0)
    engine.potential_planes(P, box, 64, [0, 1, 2], Thickness=0.3 * box, nu_response=synthetic_response([]), BoxSize_in_MPC=box / 1000.0, **COSMO)
    # the spectrum of the last PM step is still the one a caller gets
    spec1 = engine.gravpm_get_powerspectrum(nmesh, box / 1000.0)
    for a, b in zip(spec0, spec1):
        assert np.array_equal(a, b)
    P = pkg.make_particles(pos, mass)
    P["Potential"] = 0.25
    engine.gravpm_force(P)
    gpm, pot = O.gravpm_force(pos, mass, box, nmesh, 1.5, G)
    assert np.abs(P["GravPM"] - gpm).max() <= 1e-11 * np.abs(gpm).mean()
    assert np.abs(P["Potential"] - (pot + 0.25)).max() <= 1e-11 * np.abs(pot).mean()
    kk, Pk, N = O.pm_power_spectrum(pos, mass, box, nmesh, box / 1000.0)
    k2, P2, N2 = engine.gravpm_get_powerspectrum(nmesh, box / 1000.0)
    assert np.array_equal(N2, N) and np.abs(k2 - kk).max() <= 1e-12 * kk.max() and np.abs(P2 - Pk).max() <= 1e-12 * Pk.max()


def test_correction_after_mesh_change(pkg, engine):
    """a PM step on a small mesh, a new gravpm_init_periodic with a larger one and no PM step on it: the correction must not take the old
    mesh's spectrum accumulators for the new one's"""
    pos, mass, box = particle_set(16)
    bmpc = box / 1000.0
    engine.gravpm_set_nu_response(None)
    # (a step on a larger mesh first: the engine's buffers only grow, and the case must not depend on what ran before in the session)
    for nm in (128, 32):
        engine.gravpm_init_periodic(box, 1.5, nm, G)
        engine.gravpm_force(pkg.make_particles(pos, mass))
    engine.gravpm_init_periodic(box, 1.5, 96, G)
    _dev(pkg, engine, pos, mass, box)
    kw = dict(Thickness=0.3 * box, CutPoints=[0.35 * box], **COSMO)
    got, _ = engine.dev_potential_planes(64, [2], nu_response=synthetic_response([]), BoxSize_in_MPC=bmpc, **kw)
    want = R_.potential_planes(pos, box, 64, [2], mass=mass, nu_response=synthetic_response([]), nmesh=96, BoxSize_in_MPC=bmpc, **kw)
    _assert_planes(_np(engine, got), want["planes"], "after a mesh change")
    with pytest.raises(pkg.EngineError, match="no PM step"):
        engine.gravpm_get_powerspectrum(96, bmpc)


def test_batched_counting(pkg, engine):
    """a counter budget of two planes: nine planes in five passes, the correction made once; the same planes as in one pass"""
    pos, mass, box = particle_set(16)
    bmpc, R = box / 1000.0, 64
    engine.gravpm_init_periodic(box, 1.5, 32, G)
    engine.gravpm_set_nu_response(None)
    _dev(pkg, engine, pos, mass, box)
    kw = plane_args(box)
    nu = dict(nu_response=synthetic_response([]), BoxSize_in_MPC=bmpc)
    one, one_n = engine.dev_potential_planes(R, [0, 1, 2], **kw)
    one = _np(engine, one)
    one_nu, _ = engine.dev_potential_planes(R, [0, 1, 2], **kw, **nu)
    one_nu = _np(engine, one_nu)
    engine.set_plane_counter_budget(2 * R * R * 4)
    try:
        calls = []
        got, got_n = engine.dev_potential_planes(R, [0, 1, 2], **kw)
        got = _np(engine, got)
        got_nu, got_nu_n = engine.dev_potential_planes(R, [0, 1, 2], nu_response=synthetic_response(calls), BoxSize_in_MPC=bmpc, **kw)
        got_nu = _np(engine, got_nu)
        engine.set_plane_counter_budget(1)                       # less than one plane: one plane per pass
        single, single_n = engine.dev_potential_planes(R, [0, 1, 2], **kw)
        single = _np(engine, single)
    finally:
        engine.set_plane_counter_budget(0)
    assert len(calls) == 1
    assert np.array_equal(got_n, one_n) and np.array_equal(got_nu_n, one_n) and np.array_equal(single_n, one_n)
    want = R_.potential_planes(pos, box, R, [0, 1, 2], mass=mass, nu_response=synthetic_response([]), nmesh=32, BoxSize_in_MPC=bmpc, **kw)
    assert np.array_equal(one_n, want["npart"])
    _assert_planes(got, one, "two planes per pass against one pass")
    _assert_planes(single, one, "one plane per pass against one pass")
    _assert_planes(got_nu, one_nu, "two planes per pass, correction")
    _assert_planes(got_nu, want["planes"], "two planes per pass, correction, against the restatement")


def test_planes_inside_an_epoch(pkg, engine):
    """a planes call between gravpm_force and the walk of one declared epoch, on a table with dead rows: the walk's write-back reads the
    live flags the epoch's staging left on the host, which the planes call must not touch"""
    n, nmesh = 16, 32
    pos, mass, box = pkg.ics.s_zel(n)
    rng = np.random.RandomState(3)
    dead = np.sort(rng.choice(len(pos), len(pos) // 33, replace=False))
    engine.gravpm_init_periodic(box, 1.5, nmesh, G)
    engine.set_gravshort_treepar(TreeUseBH=0)
    engine.gravshort_set_softenings(box / n)
    engine.gravpm_set_nu_response(None)
    engine.gravpm_set_hybrid_nu_tracer(False)
    results = []
    for epoch, with_planes in ((11, False), (12, True)):
        P = pkg.make_particles(pos, mass)
        P["Flags"][dead[0::2]] = 1            # IsGarbage
        P["Flags"][dead[1::2]] = 2            # Swallowed
        P["Type"][dead[1::2]] = 5
        P["FullTreeGravAccel"] = 1e-7
        engine.set_particle_epoch(epoch)
        try:
            engine.gravpm_force(P)
            if with_planes:
                planes, npart = engine.potential_planes(P, box, 64, [0, 1, 2], Thickness=0.3 * box, **COSMO)
            engine.force_tree_full(P, box)
            engine.grav_short_tree(P)
        finally:
            engine.set_particle_epoch(0)
        results.append((P["GravPM"].copy(), P["FullTreeGravAccel"].copy(), P["Potential"].copy()))
    live = np.ones(len(pos), bool)
    live[dead] = False
    want = R_.potential_planes(pos, box, 64, [0, 1, 2], Thickness=0.3 * box, flags=np.where(live, 0, 1).astype(np.uint8), **COSMO)
    assert np.array_equal(npart, want["npart"])
    _assert_planes(planes, want["planes"], "inside an epoch")
    (g0, a0, p0), (g1, a1, p1) = results
    for a in (a0, a1):          # the walk wrote every live row and no dead one
        assert np.all(a[~live] == 1e-7) and np.all(np.abs(a[live]).max(axis=1) != 1e-7) and np.abs(a[live]).mean() > 1e-6
    # the two walks open their nodes with |FullTreeGravAccel + GravPM|, so a last-digit difference of GravPM may move one opening decision:
    # such a row differs by at most the force tolerance (ErrTolForceAcc = 0.002 of its acceleration), an unwritten row by all of it
    assert np.abs(a1 - a0).max() <= 0.002 * np.abs(a0[live]).max()
    # (GravPM and with it Potential carry the last digits of the deposit's atomics)
    assert np.abs(g1 - g0).max() <= 1e-11 * np.abs(g0).mean() and np.abs(p1 - p0).max() <= 1e-11 * np.abs(p0).mean()


def test_entry_points_agree(pkg, engine):
    pos, mass, box = _edge_set(pkg, "s_zel", 20)
    R = 96
    kw = dict(Thickness=0.3 * box, CutPoints=[0.35 * box, 0.05 * box, 0.9 * box], CurrentParticleOffset=(0.1 * box, 0.0, -0.25 * box), **COSMO)
    _dev(pkg, engine, pos, mass, box)
    d_planes, d_npart = engine.dev_potential_planes(R, [0, 1, 2], **kw)
    d_planes = _np(engine, d_planes)
    want = R_.potential_planes(pos, box, R, [0, 1, 2], **kw)
    assert np.array_equal(d_npart, want["npart"])
    P = pkg.make_particles(pos, mass)
    h_planes, h_npart = engine.potential_planes(P, box, R, [0, 1, 2], **kw)
    engine.resident_begin(P, box)
    try:
        r_planes, r_npart = engine.resident_potential_planes(P, R, [0, 1, 2], **kw)
        c, nact = engine.dev_plane_counts(R, [0, 1, 2], **kw)      # (the binding is the resident table's)
        assert nact == len(pos) and np.array_equal(_np(engine, c).astype(np.int64), want["counts"])
    finally:
        engine.resident_end(P)
    assert np.array_equal(h_npart, d_npart) and np.array_equal(r_npart, d_npart)
    _assert_planes(h_planes, d_planes, "host against device")
    _assert_planes(r_planes, d_planes, "resident against device")
    # integer counts into the same plans: recorded, not asserted
    print("host == device bit for bit: %s; resident == device: %s" % (np.array_equal(h_planes, d_planes), np.array_equal(r_planes, d_planes)))


def _run_helper(tmp_path, name, n, R, env_extra, nproc=1, port=29591):
    out = str(tmp_path / name)
    env = dict(os.environ, MPG_DIST_BACKEND="gloo", MASTER_ADDR="127.0.0.1", **env_extra)
    script = os.path.join(ROOT, "tools", "mgpu_planes_check.py")
    if nproc == 1:
        cmd = [sys.executable, script, out, str(n), str(R)]
    else:
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(nproc), "--master-addr", "127.0.0.1",
               "--master-port", str(port), script, out, str(n), str(R)]
    run_ranks(cmd, env, out, timeout=600)
    return [dict(np.load(out + ".rank%d.npz" % r)) for r in range(nproc)]


@pytest.mark.parametrize("nproc", [2, 4])
@keep_artifacts_on_failure
def test_planes_ranks(pkg, engine, tmp_path, nproc):
    n, R = 20, 96
    pos, mass, box = particle_set(n)
    _dev(pkg, engine, pos, mass, box)
    kw = plane_args(box)
    one, one_npart = engine.dev_potential_planes(R, [0, 1, 2], **kw)
    one = _np(engine, one)
    counts, nact = engine.dev_plane_counts(R, [0, 1, 2], **kw)
    counts = _np(engine, counts).astype(np.int64)
    ranks = _run_helper(tmp_path, "dist", n, R, {}, nproc=nproc, port=29591 + nproc)
    for r in ranks:
        assert np.array_equal(r["counts"], counts) and int(r["n_active"][0]) == nact == len(pos)
        assert np.array_equal(r["npart"], one_npart)
        _assert_planes(r["planes"], one, "%d ranks" % nproc)
    # the restated rank sum says the same
    want = R_.potential_planes(pos, box, R, [0, 1, 2], ranks=nproc, **kw)
    assert np.array_equal(want["counts"], counts)
    _assert_planes(ranks[0]["planes"], want["planes"], "%d ranks against the restatement" % nproc)


@keep_artifacts_on_failure
def test_planes_ranks_batched(pkg, engine, tmp_path):
    """every rank with another counter budget (2, 3, 4 planes): the ranks agree on the smallest batch and make the same collectives"""
    n, R = 16, 64
    pos, mass, box = particle_set(n)
    _dev(pkg, engine, pos, mass, box)
    one, one_npart = engine.dev_potential_planes(R, [0, 1, 2], **plane_args(box))
    one = _np(engine, one)
    for r in _run_helper(tmp_path, "batched", n, R, {"MPG_PLANES_BUDGET": "1"}, nproc=3, port=29607):
        assert np.array_equal(r["npart"], one_npart)
        _assert_planes(r["planes"], one, "3 ranks, batched")


@keep_artifacts_on_failure
def test_planes_ranks_refuse_together(pkg, tmp_path):
    """a position one rank cannot wrap: every rank returns the refusal, nobody waits in a collective"""
    for r in _run_helper(tmp_path, "bad", 16, 64, {"MPG_PLANES_BAD_ROW": "1"}, nproc=2, port=29609):
        assert "not finite or far outside the box" in str(r["error"])


@keep_artifacts_on_failure
def test_planes_ranks_refuse_correction(pkg, tmp_path):
    ranks = _run_helper(tmp_path, "nu", 16, 64, {"MPG_PLANES_NU": "1"}, nproc=2, port=29599)
    for r in ranks:
        assert "the massive-neutrino correction on several ranks is not implemented" in str(r["error"])


def test_errors(pkg, engine):
    pos, mass, box = pkg.ics.s_zel(16)
    _dev(pkg, engine, pos, mass, box)
    ok = dict(Thickness=0.3 * box, **COSMO)
    nu = dict(nu_response=synthetic_response([]), BoxSize_in_MPC=box / 1000.0)
    engine.petapm_destroy()
    cases = [(dict(ok), dict(Normals=[0, 3]), "normal direction beyond 0, 1 and 2"),
             (dict(ok), dict(Normals=[-1]), "normal direction beyond 0, 1 and 2"),
             (dict(ok), dict(Resolution=0), "Resolution must be at least 1"),
             (dict(ok, CutPoints=np.linspace(0, box, 1025)), {}, "ncuts > 1024"),
             (dict(ok, Thickness=box / 2000.0), {}, "ncuts > 1024"),
             (dict(ok, omega_source=0.0), {}, "omega_source <= 0"),
             (dict(ok, omega_source=-0.1), {}, "omega_source <= 0"),
             (dict(ok, **nu), {}, "needs the PM mesh")]
    for kw, over, msg in cases:
        args = dict(Resolution=32, Normals=[0, 1])
        args.update(over)
        with pytest.raises(pkg.EngineError, match=msg):
            engine.dev_potential_planes(args["Resolution"], args["Normals"], **kw)
    engine.gravpm_init_periodic(box, 1.5, 32, G)
    with pytest.raises(pkg.EngineError, match="Resolution must be at least 2"):
        engine.dev_potential_planes(1, [0], **dict(ok, **nu))

    def boom(k, d, m):
        raise RuntimeError("no table")
    for fn, msg in ((boom, "potential planes: the neutrino response callback"),
                    (lambda k, d, m: (np.log(k)[::-1].copy(), np.zeros_like(k), 0.07, 1.05), "potential planes: .*not strictly increasing"),
                    (lambda k, d, m: (np.log(k), np.full_like(k, np.nan), 0.07, 1.05), "potential planes: .*not finite")):
        with pytest.raises(pkg.EngineError, match=msg):
            engine.dev_potential_planes(32, [0], **dict(ok, nu_response=fn, BoxSize_in_MPC=box / 1000.0))
    # no active particle; no active mass
    import torch
    dead = torch.full((len(pos),), 2, dtype=torch.uint8, device="cuda")
    with pytest.raises(pkg.EngineError, match="zero active particle count"):
        engine.dev_potential_planes(32, [0], flags=dead, **ok)
    _dev(pkg, engine, pos, np.zeros_like(mass), box)
    with pytest.raises(pkg.EngineError, match="zero active particle mass"):
        engine.dev_potential_planes(32, [0], **dict(ok, **nu))
    # a position the wrap cannot bring home is refused, not spun on
    bad = pos.copy()
    bad[5, 1] = np.inf
    _dev(pkg, engine, bad, mass, box)
    with pytest.raises(pkg.EngineError, match="not finite or far outside the box"):
        engine.dev_potential_planes(32, [0], **ok)
    # the engine is usable afterwards
    _dev(pkg, engine, pos, mass, box)
    planes, npart = engine.dev_potential_planes(32, [0, 1], **ok)
    want = R_.potential_planes(pos, box, 32, [0, 1], **ok)
    assert np.array_equal(npart, want["npart"])
    _assert_planes(_np(engine, planes), want["planes"], "after the errors")
    assert R_.potential_planes(pos, box, 1, [2], **ok)["planes"].shape == (3, 1, 1, 1)
    one, n1 = engine.dev_potential_planes(1, [2], **ok)                     # Resolution 1: only the uniform mode, which is dropped
    assert np.array_equal(_np(engine, one), np.zeros((3, 1, 1, 1))) and (n1 > 0).all()


def test_full_size_particle_planes(pkg, engine):
    """s_zel(256), R = 4096, three normals, default cut points for Thickness = Box / 3"""
    import torch
    clock = phase_clock("test_full_size_particle_planes")
    pos, mass, box = pkg.ics.s_zel(256)
    clock.mark("ics")
    R, th = 4096, box / 3
    _dev(pkg, engine, pos, mass, box)
    counts, nact = engine.dev_plane_counts(R, [0, 1, 2], Thickness=th, **COSMO)
    planes, npart = engine.dev_potential_planes(R, [0, 1, 2], Thickness=th, **COSMO)
    engine.synchronize()
    clock.mark("gpu")
    assert nact == len(pos) and planes.shape == (3, 3, R, R)
    norm = R_.normalisations(box, th, COSMO["comoving_distance"], COSMO["atime"], COSMO["HubbleParam"], COSMO["omega_source"])
    worst = 0.0
    for i, cut in enumerate(R_.resolve(box, th, None)[1]):
        for j, normal in enumerate([0, 1, 2]):
            pix = R_.plane_pixels(pos, box, R, normal, cut, th)
            c = np.bincount(pix[pix >= 0], minlength=R * R).reshape(R, R)
            assert np.array_equal(counts[i, j].cpu().numpy().astype(np.int64), c) and npart[i, j] == c.sum()
            want = R_.potential_from_counts(c, len(pos), box, th, COSMO["comoving_distance"], COSMO["atime"], COSMO["HubbleParam"],
                                            COSMO["omega_source"])
            got = planes[i, j].cpu().numpy()
            d, m = np.abs(got - want).max(), np.abs(want).mean()
            worst = max(worst, d / m)
            assert d <= BOUND * m, (i, j, d / m)
    assert norm > 0
    clock.mark("restated")
    clock.write()
    print("full size: largest difference %.3g of mean |psi| (bound %.1g)" % (worst, BOUND))
    del counts, planes
    torch.cuda.empty_cache()


def test_full_size_correction(pkg, engine):
    """one Nmesh = 512 correction at R = 2048 against the composition"""
    import torch
    clock = phase_clock("test_full_size_correction")
    pos, mass, box = pkg.ics.s_zel(256)
    clock.mark("ics")
    R, nmesh, bmpc = 2048, 512, box / 1000.0
    engine.gravpm_init_periodic(box, 1.5, nmesh, G)
    engine.gravpm_set_nu_response(None)
    _dev(pkg, engine, pos, mass, box)
    kw = dict(Thickness=box / 3, CutPoints=[box / 2], **COSMO)
    calls = []
    planes, npart = engine.dev_potential_planes(R, [1], nu_response=synthetic_response(calls), BoxSize_in_MPC=bmpc, **kw)
    got = _np(engine, planes)
    clock.mark("gpu")
    want = R_.potential_planes(pos, box, R, [1], mass=mass, nu_response=synthetic_response([]), nmesh=nmesh, BoxSize_in_MPC=bmpc, **kw)
    clock.mark("restated")
    clock.write()
    assert np.array_equal(npart, want["npart"]) and len(calls) == 1
    assert np.abs(want["correction"]).max() >= 1e3 * BOUND * np.abs(want["planes"]).mean()
    _assert_planes(got, want["planes"], "full size correction")
    engine.petapm_destroy()
    torch.cuda.empty_cache()
