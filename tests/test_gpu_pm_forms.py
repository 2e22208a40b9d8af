"""Every form of the long-range PM step on the GPU (csrc/pm.hip) against the long-double restatement of tests/pm_restated.py.

What a PM call runs is decided by three switches and, left alone, by a stopwatch: the deposit is the plain atomic kernel or the
cell-sorted, wave-aggregated one (k_cell_keys + radix sort + k_cic_deposit_sorted), whichever PMesh::deposit timed faster on the first
call and every 64th (MPG_PM_DEPOSIT pins it; read on every call); the forces come from one inverse transform and the stencil read-out
or from four inverse transforms (MPG_PM_KSPACE_FORCE, read by gravpm_init_periodic); the potential transfer runs fused into the
power-spectrum pass or alone (gravpm_measure_power).  Each is pinned here and compared with the same reference, on input sets whose
fp64 error is known to be a tenth of the tolerance (test_pm_extended_precision.py).  The slab stage calls (mpg_dev_pm_slab_*) are
driven in one process, W engines standing for W ranks, down to the thinnest slab slab_init admits.

Tolerance, SURVEY 8(d): max |dGravPM| <= 1e-11 mean |GravPM|, the same for the potential; for one particle alone see
pm_restated.force_scale.  Every test makes its own engines: pinning a deposit form leaves an engine in that form."""
import contextlib

import numpy as np
import pytest

import pm_restated as R

pytestmark = pytest.mark.gpu
TOL = 1e-11
POT0 = 0.25                                               # readout_potential accumulates (gravpm.c:499-501)
DEPOSITS = ("plain", "sorted", "auto")


def _pin(monkeypatch, deposit, kspace=False):
    if deposit == "auto":
        monkeypatch.delenv("MPG_PM_DEPOSIT", raising=False)
    else:
        monkeypatch.setenv("MPG_PM_DEPOSIT", deposit)
    if kspace:
        monkeypatch.setenv("MPG_PM_KSPACE_FORCE", "1")
    else:
        monkeypatch.delenv("MPG_PM_KSPACE_FORCE", raising=False)


@contextlib.contextmanager
def own_engines(pkg, box, nmesh, count=1):
    """`count` engines of this test alone with the PM mesh set up (the force form is read from the environment here), closed on exit"""
    engs = []
    try:
        for _ in range(count):
            e = pkg.Engine(0)
            engs.append(e)
            e.gravpm_init_periodic(box, 1.5, nmesh, R.G)
        yield engs
    finally:
        for e in engs:
            e.close()


def _upload(pos, mass, types=None):
    import torch
    d = (torch.from_numpy(np.ascontiguousarray(pos)).cuda(), torch.from_numpy(np.ascontiguousarray(mass, np.float32)).cuda(),
         None if types is None else torch.from_numpy(np.ascontiguousarray(types, np.uint8)).cuda())
    torch.cuda.synchronize()
    return d


def _outputs(n):
    import torch
    gpm = torch.full((max(n, 1), 3), 7.0, dtype=torch.float64, device="cuda")
    pot = torch.full((max(n, 1),), POT0, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()                              # (the engine runs on a stream of its own)
    return gpm, pot


def dev_step(eng, d_pos, d_mass, box, d_type=None):
    eng.dev_bind_particles(d_pos, d_mass, box, d_type)
    gpm, pot = _outputs(d_pos.shape[0])
    eng.dev_gravpm_force(gpm, pot)
    eng.synchronize()
    return gpm.cpu().numpy(), pot.cpu().numpy()


def host_step(pkg, eng, pos, mass):
    P = pkg.make_particles(pos, mass)
    P["Potential"] = POT0
    P["GravPM"] = 7.0
    eng.gravpm_force(P)
    return P["GravPM"].copy(), P["Potential"].copy()


def check(name, gpm, pot, what=""):
    """the bound of the module docstring against the long-double result of the named set; the figures are printed first (pytest -s)"""
    g_ld, p_ld = R.reference(name)
    fs, ps = R.force_scale(name)
    dg = float(np.abs(gpm - g_ld).max() / fs)
    dp = float(np.abs(pot - (p_ld + POT0)).max() / ps)
    print("%s %s: GravPM %.2e  Potential %.2e (of the mean)" % (name, what, dg, dp))
    assert dg <= TOL and dp <= TOL, (name, what, dg, dp)
    return dg, dp


# ------------------------------------------------------------------------------------------------ deposit x force x transfer forms
@pytest.mark.parametrize("name", R.MAIN_SETS)
@pytest.mark.parametrize("measure", [True, False], ids=["fused_ps", "transfer_alone"])
@pytest.mark.parametrize("kspace", [False, True], ids=["stencil", "kspace"])
@pytest.mark.parametrize("deposit", DEPOSITS)
def test_pm_forms_host_entry(pkg, monkeypatch, deposit, kspace, measure, name):
    """mpg_gravpm_force on a particle table: each deposit form, both force forms, both transfer forms, five input sets (Nmesh 32 .. 72)"""
    pos, mass, box, nmesh = R.input_set(name)
    _pin(monkeypatch, deposit, kspace)
    with own_engines(pkg, box, nmesh) as (eng,):
        eng.gravpm_measure_power(measure)
        check(name, *host_step(pkg, eng, pos, mass), what="%s/%s/%s" % (deposit, "kspace" if kspace else "stencil", measure))


# ------------------------------------------------------------------------------------------------ the sorted kernel's scan boundaries
@pytest.mark.parametrize("name", R.SWEEP_SETS)
@pytest.mark.parametrize("deposit", ["plain", "sorted"])
def test_pm_scan_boundaries(pkg, monkeypatch, deposit, name):
    """N = 1, 63, 64, 65, 255, 256, 257, 3001 - all in one cell, and in runs that end on lanes 63 and 0 and cross waves and blocks
    (pm_restated.sweep) - at Nmesh 8 and 40 through the device entry: a wrong carry of the segmented scan at a run, wave or block
    boundary changes which weights are summed"""
    pos, mass, box, nmesh = R.input_set(name)
    _pin(monkeypatch, deposit)
    with own_engines(pkg, box, nmesh) as (eng,):
        d_pos, d_mass, _ = _upload(pos, mass)
        check(name, *dev_step(eng, d_pos, d_mass, box), what=deposit)


def test_pm_no_particles_touches_nothing(pkg, monkeypatch):
    import torch
    _pin(monkeypatch, "auto")
    with own_engines(pkg, 100.0, 8) as (eng,):
        d_pos = torch.zeros((0, 3), dtype=torch.float64, device="cuda")
        d_mass = torch.zeros((0,), dtype=torch.float32, device="cuda")
        gpm, pot = dev_step(eng, d_pos, d_mass, 100.0)
        assert np.all(gpm == 7.0) and np.all(pot == POT0)


def test_pm_retune_calls(pkg, monkeypatch):
    """deposit form left to the stopwatch: call 1 and call 65 time both kernels (the mesh is cleared twice and deposited a third
    time), the calls around them run whichever won.  Calls 1, 64, 65 and 66 on one engine against the reference."""
    name = "pile"
    pos, mass, box, nmesh = R.input_set(name)
    _pin(monkeypatch, "auto")
    with own_engines(pkg, box, nmesh) as (eng,):
        d_pos, d_mass, _ = _upload(pos, mass)
        for call in range(1, 67):
            res = dev_step(eng, d_pos, d_mass, box)
            if call in (1, 64, 65, 66):
                check(name, *res, what="call %d" % call)


# ------------------------------------------------------------------------------------------------ inactive records, zero-weight members
@pytest.mark.parametrize("deposit", DEPOSITS)
def test_pm_dead_records_host_entry(pkg, monkeypatch, deposit):
    """a third of the table garbage or swallowed black holes, heavy, inside the densest cell (the 64-bit-key branch of the sort when the
    deposit is the sorted one): the live records get the result of the live set alone, the dead come back with GravPM = 0 and their
    Potential untouched (gravpm.c:88-92, 176-179)"""
    pos, mass, box, dead = R.pile_with_dead()
    nmesh = 40
    _pin(monkeypatch, deposit)
    with own_engines(pkg, box, nmesh) as (eng,):
        P = pkg.make_particles(pos, mass)
        di = np.flatnonzero(dead)
        assert 0.3 < len(di) / len(P) < 0.37
        P["Flags"][di[0::2]] = 1                          # IsGarbage
        P["Flags"][di[1::2]] = 2                          # Swallowed ...
        P["Type"][di[1::2]] = 5                           # ... black holes
        P["Potential"] = POT0
        P["GravPM"] = 7.0
        eng.gravpm_force(P)
        check("pile-live", P["GravPM"][~dead], P["Potential"][~dead], what=deposit + "/dead records")
        assert np.all(P["GravPM"][di] == 0.0) and np.all(P["Potential"][di] == POT0)


@pytest.mark.parametrize("deposit", DEPOSITS)
def test_pm_tracer_particles_device_entry(pkg, monkeypatch, deposit):
    """hybrid-neutrino tracers through the device entry: a third of the particles are type 2, deposit zero mass (k_tracer_mass) and are
    read out all the same - sorted runs carry zero-weight members"""
    pos, mass, box = R.pile()
    types = R.pile_tracer_types(len(pos))
    _pin(monkeypatch, deposit)
    with own_engines(pkg, box, 40) as (eng,):
        eng.gravpm_set_hybrid_nu_tracer(True)
        d_pos, d_mass, d_type = _upload(pos, mass, types)
        check("pile-tracer", *dev_step(eng, d_pos, d_mass, box, d_type), what=deposit + "/tracers")


# ------------------------------------------------------------------------------------------------ P(k)
@pytest.mark.parametrize("name", ["clust", "pile"])
@pytest.mark.parametrize("deposit", DEPOSITS)
def test_pm_power_spectrum_forms(pkg, monkeypatch, deposit, name):
    """the spectrum of the deposited field under each deposit form against the long-double accumulators: the tolerances of
    test_gpu_gravity.py::test_pm_power_spectrum"""
    pos, mass, box, nmesh = R.input_set(name)
    mpc = box / 1000.0
    _pin(monkeypatch, deposit)
    with own_engines(pkg, box, nmesh) as (eng,):
        d_pos, d_mass, _ = _upload(pos, mass)
        dev_step(eng, d_pos, d_mass, box)
        k, P, N = eng.gravpm_get_powerspectrum(nmesh, mpc)
    kl, Pl, Nl, _ = R.power_spectrum_ld(pos, mass, box, nmesh, mpc)
    assert np.array_equal(N, Nl) and N.sum() == nmesh ** 3 - 1
    dk, dP = float(np.abs(k / kl - 1).max()), float(np.abs(P / Pl - 1).max())
    print("%s %s: k %.2e  P %.2e" % (name, deposit, dk, dP))
    assert dk <= 1e-12 and dP <= 1e-9


# ------------------------------------------------------------------------------------------------ positions outside the box
@pytest.mark.parametrize("entry", ["host", "device"])
@pytest.mark.parametrize("kspace", [False, True], ids=["stencil", "kspace"])
@pytest.mark.parametrize("deposit", DEPOSITS)
def test_pm_positions_whole_boxes_outside(pkg, monkeypatch, deposit, kspace, entry):
    """a fifth of the pile moved by -3, -1, +1, +2 and +5 boxes per axis: the base cell folds by any number of boxes, as the
    reference's while loops do (petapm.c:905-906, 917-918), in the deposit, the cell keys and both read-outs"""
    name = "pile-shift"
    pos, mass, box, nmesh = R.input_set(name)
    assert pos.min() < -2 * box and pos.max() > 5 * box
    _pin(monkeypatch, deposit, kspace)
    with own_engines(pkg, box, nmesh) as (eng,):
        if entry == "host":
            res = host_step(pkg, eng, pos, mass)
        else:
            d_pos, d_mass, _ = _upload(pos, mass)
            res = dev_step(eng, d_pos, d_mass, box)
        check(name, *res, what="%s/%s/%s" % (deposit, "kspace" if kspace else "stencil", entry))


# ------------------------------------------------------------------------------------------------ the slab stage calls
def slab_step(engs, d_pos, d_mass, pos, box, nmesh):
    """One PM step by the slab stage calls, engs[r] standing for rank r of W = len(engs); the collectives between the stages are done
    here with torch indexing.  Returns (GravPM, Potential, targets per rank, ghost_recv per rank)."""
    import torch
    W, n = len(engs), len(pos)
    P = nmesh // W
    f8 = dict(dtype=torch.float64, device="cuda")
    sizes = []
    for r, e in enumerate(engs):
        e.dev_bind_particles(d_pos, d_mass, box)
        sizes.append(e.dev_pm_slab_init(r, W))
    cpp, plane = sizes[0]
    assert all(s == (cpp, plane) for s in sizes) and cpp == P * P * (nmesh // 2 + 1) and plane == nmesh * nmesh

    def stage(call, ins):
        outs = [torch.zeros((W, cpp, 2), **f8) for _ in engs]
        torch.cuda.synchronize()
        for r, e in enumerate(engs):
            call(e, ins[r], outs[r])
            e.synchronize()
        # all-to-all: what rank r receives is, over the senders s, block r of what s sent
        return [torch.stack([outs[s][r] for s in range(W)]).contiguous() for r in range(W)]
    recvA = stage(lambda e, _, out: e.dev_pm_slab_forward_a(out), [None] * W)
    recvB = stage(lambda e, inp, out: e.dev_pm_slab_forward_b(inp, out), recvA)
    ghost_send = [torch.zeros((5, plane), **f8) for _ in engs]
    torch.cuda.synchronize()
    for r, e in enumerate(engs):
        e.dev_pm_slab_inverse_c(recvB[r], ghost_send[r])
        e.synchronize()
    # the next rank's first three planes, then the previous rank's last two
    ghost_recv = [torch.cat([ghost_send[(r + 1) % W][:3], ghost_send[(r - 1) % W][3:5]]).contiguous() for r in range(W)]
    owner = R.cells(pos, box, nmesh)[0][:, 0] // P
    targets = [torch.from_numpy(np.flatnonzero(owner == r).astype(np.int32)).cuda() for r in range(W)]
    gpm = torch.full((n, 3), float("nan"), **f8)
    pot = torch.full((n,), POT0, **f8)
    torch.cuda.synchronize()
    for r, e in enumerate(engs):
        e.dev_pm_slab_readout(ghost_recv[r], targets[r], gpm, pot)
        e.synchronize()
    return gpm.cpu().numpy(), pot.cpu().numpy(), targets, ghost_recv


@pytest.mark.parametrize("kind", ["pileslab", "clust"])
@pytest.mark.parametrize("nmesh,W", R.SLAB_CASES)
@pytest.mark.parametrize("deposit", ["plain", "sorted"])
def test_pm_slab_stages(pkg, monkeypatch, deposit, nmesh, W, kind):
    """forward_a / forward_b / inverse_c / readout with W = 1, 3, 4, 4, 2 ranks: slabs of 32, 16, 5, 3 (the thinnest admitted: the three
    "first" and two "last" ghost planes of a slab overlap) and 4 planes.  The pile's dense cell straddles two ranks' planes - the last
    and the first rank's for W = 4.  Every particle is read out by exactly one rank (a row read twice would hold twice the potential, a
    row never read keeps its NaN) and the union is the long-double result."""
    name = "pileslab-%d-%d" % (nmesh, W) if kind == "pileslab" else "clust-%d" % nmesh
    pos, mass, box, nm = R.input_set(name)
    assert nm == nmesh
    _pin(monkeypatch, deposit)
    with own_engines(pkg, box, nmesh, W) as engs:
        d_pos, d_mass, _ = _upload(pos, mass)
        gpm, pot, targets, _ = slab_step(engs, d_pos, d_mass, pos, box, nmesh)
    allt = np.concatenate([t.cpu().numpy() for t in targets])
    assert len(allt) == len(pos) and np.array_equal(np.sort(allt), np.arange(len(pos)))
    if kind == "pileslab":                                # the dense cell's planes: two ranks deposit its particles
        ix = R.slab_dense_cell(nmesh, W)[0]
        assert W == 1 or ix // (nmesh // W) != ((ix + 1) % nmesh) // (nmesh // W)
    assert np.all(np.isfinite(gpm))
    check(name, gpm, pot, what="slab W=%d/%s" % (W, deposit))


@pytest.mark.parametrize("deposit", ["plain", "sorted"])
def test_pm_slab_positions_whole_boxes_outside(pkg, monkeypatch, deposit):
    """the slab deposit and read-out fold the base cell like the single-mesh kernels: the shifted pile on 4 ranks of 5 planes"""
    name = "pileslab-20-4-shift"
    pos, mass, box, nmesh = R.input_set(name)
    assert pos.min() < -2 * box and pos.max() > 5 * box
    _pin(monkeypatch, deposit)
    with own_engines(pkg, box, nmesh, 4) as engs:
        d_pos, d_mass, _ = _upload(pos, mass)
        gpm, pot, _, _ = slab_step(engs, d_pos, d_mass, pos, box, nmesh)
    check(name, gpm, pot, what="slab W=4/" + deposit)


def test_pm_slab_one_rank_is_the_single_mesh_step(pkg, monkeypatch):
    """include/mpgadget_hip.h: "world == 1 reproduces mpg_dev_gravpm_force to FFT round-off".  Direct difference of the two, the
    project's 1e-11 of the mean asserted.  Measured on an MI355X (pile set, Nmesh 32, plain deposit): GravPM 1.8e-14, Potential 1.9e-15 of
    the mean - both are fp64 transforms of the same mesh, the 3-D plan against the 2-D + 1-D plans and two transposes."""
    name = "pileslab-32-1"
    pos, mass, box, nmesh = R.input_set(name)
    _pin(monkeypatch, "plain")
    with own_engines(pkg, box, nmesh, 2) as (slab, single):
        d_pos, d_mass, _ = _upload(pos, mass)
        g1, p1 = dev_step(single, d_pos, d_mass, box)
        g2, p2, _, _ = slab_step([slab], d_pos, d_mass, pos, box, nmesh)
    fs, ps = R.force_scale(name)
    dg, dp = float(np.abs(g2 - g1).max() / fs), float(np.abs(p2 - p1).max() / ps)
    print("slab W=1 against dev_gravpm_force: GravPM %.2e  Potential %.2e (of the mean)" % (dg, dp))
    assert dg <= TOL and dp <= TOL, (dg, dp)


def test_pm_slab_refusals(pkg, monkeypatch):
    """a target of another rank's slab is an error, not a read beside the slab; slab_init refuses Nmesh % W != 0 and slabs thinner than
    3 planes; the single-mesh step refuses while the mesh is in slab form"""
    import torch
    name = "pileslab-20-4"
    pos, mass, box, nmesh = R.input_set(name)
    _pin(monkeypatch, "plain")
    with own_engines(pkg, box, nmesh, 4) as engs:
        d_pos, d_mass, _ = _upload(pos, mass)
        _, _, targets, ghost_recv = slab_step(engs, d_pos, d_mass, pos, box, nmesh)
        gpm, pot = _outputs(len(pos))
        bad = torch.cat([targets[0][:10], targets[1][:1]]).contiguous()
        torch.cuda.synchronize()
        with pytest.raises(pkg.EngineError, match="outside this rank's slab"):
            engs[0].dev_pm_slab_readout(ghost_recv[0], bad, gpm, pot)
        with pytest.raises(pkg.EngineError, match="slab-decomposed form"):
            engs[0].dev_gravpm_force(gpm, pot)
        with pytest.raises(pkg.EngineError, match="multiple of the number of GPUs"):
            engs[1].dev_pm_slab_init(0, 3)
        with pytest.raises(pkg.EngineError, match="at least 3 mesh planes"):
            engs[2].dev_pm_slab_init(0, 10)
