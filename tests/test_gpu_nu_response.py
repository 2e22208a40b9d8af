"""The massive-neutrino linear response in the PM solve (MassiveNuLinRespOn: gravpm.c:72-79, 303-326, 418-446) and the hybrid-neutrino
deposit mask (gravpm.c:84-85, 469-474), against a composition of the unchanged oracle building blocks: pm_cic_deposit, numpy rfftn,
nufac(k) of gravpm.c:418-436 with np.interp, pm_transfer_arrays, irfftn, pm_readout."""
import os
import sys

import numpy as np
import pytest

from conftest import keep_artifacts_on_failure, run_ranks
from oracle import oracle as O

G = 43.0071
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from mgpu_nu_check import synthetic_response, tracer_types  # noqa: E402


def _kgrid(nmesh):
    kx = np.fft.fftfreq(nmesh, 1.0 / nmesh).astype(np.int64)
    kx[nmesh // 2] = nmesh // 2
    kz = np.arange(nmesh // 2 + 1, dtype=np.int64)
    return np.broadcast_arrays(kx[:, None, None], kx[None, :, None], kz[None, None, :])


def _spectrum(rho_k, nmesh, bmpc, normfac=1.0):
    """measure_power_spectrum + powerspectrum_sum on a Fourier mesh (the arithmetic of O.pm_power_spectrum)"""
    KX, KY, KZ = _kgrid(nmesh)
    k2 = KX * KX + KY * KY + KZ * KZ
    f = np.ones(k2.shape)
    for K in (KX, KY, KZ):
        t = O._sinc_unnormed(K * np.pi / nmesh)
        f = f * (1.0 / (t * t))
    m = rho_k.real ** 2 + rho_k.imag ** 2
    norm = m[0, 0, 0] * normfac
    binsperunit = (nmesh - 1) / np.log(np.sqrt(3) * nmesh / 2.0)
    sel = k2 > 0
    kint = np.floor(binsperunit * np.log(k2[sel].astype(np.float64)) / 2.).astype(np.int64)
    w = np.where((KZ[sel] == 0) | (KZ[sel] == nmesh // 2), 1, 2)
    power = np.bincount(kint, weights=w * m[sel] * f[sel] ** 2, minlength=nmesh)
    kk = np.bincount(kint, weights=w * np.sqrt(k2[sel].astype(np.float64)), minlength=nmesh)
    nm = np.bincount(kint, weights=w, minlength=nmesh).astype(np.int64)
    nz = nm > 0
    return kk[nz] / nm[nz] * 2 * np.pi / bmpc, power[nz] / nm[nz] / norm * bmpc ** 3, nm[nz]


def _nufac(nmesh, bmpc, logknu, ratio, prefac):
    """gravpm.c:418-436: the two clamps, then 1 + nu_prefac * (linear interpolation of delta_nu_ratio in logknu)"""
    KX, KY, KZ = _kgrid(nmesh)
    k2 = (KX * KX + KY * KY + KZ * KZ).astype(np.float64)
    with np.errstate(divide="ignore"):
        logk = np.log(np.sqrt(k2) * 2 * np.pi / bmpc)
    logk = np.where((logk < logknu[0]) & (logk > logknu[0] - np.log(2)), logknu[0], logk)
    logk = np.where(logk > logknu[-1], logknu[-1], logk)
    nf = 1 + prefac * np.interp(logk, logknu, ratio)
    nf[0, 0, 0] = 1.0
    return nf


def composed(pos, mass, box, nmesh, response=None, deposit=None):
    """(GravPM, Potential, (kk, P, N) of the measured spectrum, callback inputs) of the PM step with the response `response` (a
    callable as Engine.gravpm_set_nu_response takes, or None) and only the particles `deposit` (mask) in the mesh"""
    dep = np.ones(len(pos), bool) if deposit is None else deposit
    bmpc = box / 1000.0
    rho_k = np.fft.rfftn(O.pm_cic_deposit(pos[dep], mass[dep], box, nmesh))
    normfac, inputs = 1.0, None
    if response is not None:
        kk, P, N = _spectrum(rho_k, nmesh, bmpc)
        inputs = (kk, np.sqrt(P), N)
        lk, rt, pf, mt = response(*inputs)
        rho_k = rho_k * _nufac(nmesh, bmpc, np.asarray(lk), np.asarray(rt), pf)
        normfac = mt * mt
    spec = _spectrum(rho_k, nmesh, bmpc, normfac)
    fac, diffs = O.pm_transfer_arrays(box, nmesh, 1.5, G)
    pot_k = rho_k * fac
    n3 = float(nmesh) ** 3
    gpm = np.zeros((len(pos), 3))
    for d in range(3):
        gpm[:, d] = O.pm_readout(np.fft.irfftn(pot_k * (1j * diffs[d]), s=(nmesh,) * 3, axes=(0, 1, 2)) * n3, pos, box, nmesh)
    pot = O.pm_readout(np.fft.irfftn(pot_k, s=(nmesh,) * 3, axes=(0, 1, 2)) * n3, pos, box, nmesh)
    return gpm, pot, spec, inputs


def _setup(eng, box, n, nmesh):
    eng.gravpm_init_periodic(box, 1.5, nmesh, G)
    eng.set_gravshort_treepar(TreeUseBH=0)
    eng.gravshort_set_softenings(box / n)
    eng.gravpm_set_hybrid_nu_tracer(False)
    eng.gravpm_set_nu_response(None)


def _close(a, b, rel):
    return np.abs(a - b).max() <= rel * np.abs(b).mean()


def test_composition_reproduces_oracle(pkg):
    """the composition with nufac = 1 is O.gravpm_force"""
    pos, mass, box = pkg.ics.s_zel(16)
    gpm, pot, _, _ = composed(pos, mass, box, 32, response=lambda k, d, m: (np.log(k), np.zeros_like(k), 0.0, 1.0))
    g0, p0 = O.gravpm_force(pos, mass, box, 32, 1.5, G)
    assert _close(gpm, g0, 1e-13) and _close(pot, p0, 1e-13)


@pytest.mark.gpu
@pytest.mark.parametrize("n,nmesh", [(16, 32), (20, 48)])
def test_nu_response_parity(pkg, engine, n, nmesh):
    pos, mass, box = pkg.ics.s_zel(n)
    _setup(engine, box, n, nmesh)
    calls = []
    engine.gravpm_set_nu_response(synthetic_response(calls), box / 1000.0)
    P = pkg.make_particles(pos, mass)
    P["Potential"] = 0.25
    engine.gravpm_force(P)
    gpm, pot, spec, inputs = composed(pos, mass, box, nmesh, synthetic_response([]))
    assert len(calls) == 1
    for got, want in zip(calls[0], inputs):
        assert got.shape == want.shape
        assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max()
    # the bins the callback sees are O.pm_power_spectrum's, square-rooted
    kk, Pk, N = O.pm_power_spectrum(pos, mass, box, nmesh, box / 1000.0)
    assert np.array_equal(calls[0][2], N)
    assert np.abs(calls[0][0] - kk).max() <= 1e-12 * kk.max() and np.abs(calls[0][1] - np.sqrt(Pk)).max() <= 1e-12 * np.sqrt(Pk).max()
    assert _close(P["GravPM"], gpm, 1e-11)
    assert _close(P["Potential"], pot + 0.25, 1e-11)
    # the correction is not a no-op at this tolerance
    g0, _ = O.gravpm_force(pos, mass, box, nmesh, 1.5, G)
    assert np.abs(g0 - gpm).max() > 1e-6 * np.abs(gpm).mean()
    # 2. the saved spectrum is the total matter one: rho_k * nufac, Norm * MtotbyMcdm^2
    k2, P2, N2 = engine.gravpm_get_powerspectrum(nmesh, box / 1000.0)
    assert np.array_equal(N2, spec[2])
    assert np.abs(k2 - spec[0]).max() <= 1e-12 * spec[0].max()
    assert np.abs(P2 - spec[1]).max() <= 1e-12 * spec[1].max()
    engine.gravpm_set_nu_response(None)


@pytest.mark.gpu
def test_nu_response_identity_and_removal(pkg, engine):
    n, nmesh = 16, 32
    pos, mass, box = pkg.ics.s_zel(n)
    _setup(engine, box, n, nmesh)
    runs = []
    for fn in (None, None, lambda k, d, m: (np.log(k), 0.3 / (1 + k), 0.0, 1.0), None):
        engine.gravpm_set_nu_response(fn, box / 1000.0)
        P = pkg.make_particles(pos, mass)
        engine.gravpm_force(P)
        runs.append((P["GravPM"].copy(), P["Potential"].copy()))
    base, again, ident, removed = runs
    # the deposit sums with atomics: bit-equality with the response is asked where two plain runs are bit-equal themselves
    tol = max(np.abs(again[0] - base[0]).max(), 0.0)
    if tol == 0.0:
        assert np.array_equal(ident[0], base[0]) and np.array_equal(ident[1], base[1])
        assert np.array_equal(removed[0], base[0]) and np.array_equal(removed[1], base[1])
    else:
        assert np.abs(ident[0] - base[0]).max() <= 4 * tol and np.abs(removed[0] - base[0]).max() <= 4 * tol
    # the measurement is part of the response: made with mpg_gravpm_measure_power(eng, 0) as well
    engine.gravpm_measure_power(False)
    try:
        calls = []
        engine.gravpm_set_nu_response(synthetic_response(calls), box / 1000.0)
        P = pkg.make_particles(pos, mass)
        engine.gravpm_force(P)
        gpm, _, spec, _ = composed(pos, mass, box, nmesh, synthetic_response([]))
        assert len(calls) == 1 and _close(P["GravPM"], gpm, 1e-11)
        assert np.abs(engine.gravpm_get_powerspectrum(nmesh, box / 1000.0)[1] - spec[1]).max() <= 1e-12 * spec[1].max()
    finally:
        engine.gravpm_measure_power(True)
        engine.gravpm_set_nu_response(None)


@pytest.mark.gpu
def test_nu_response_device_entry(pkg, engine):
    import torch
    n, nmesh = 16, 32
    pos, mass, box = pkg.ics.s_zel(n)
    _setup(engine, box, n, nmesh)
    engine.gravpm_set_nu_response(synthetic_response([]), box / 1000.0)
    dev = torch.device("cuda", 0)
    d_pos, d_mass = torch.from_numpy(pos).to(dev), torch.from_numpy(mass).to(dev)
    engine.dev_bind_particles(d_pos, d_mass, box)
    g = torch.zeros(len(pos), 3, dtype=torch.float64, device=dev)
    p = torch.zeros(len(pos), dtype=torch.float64, device=dev)
    engine.dev_gravpm_force(g, p)
    engine.synchronize()
    gpm, pot, _, _ = composed(pos, mass, box, nmesh, synthetic_response([]))
    assert _close(g.cpu().numpy(), gpm, 1e-11) and _close(p.cpu().numpy(), pot, 1e-11)
    engine.gravpm_set_nu_response(None)


@pytest.mark.gpu
def test_hybrid_tracer_mask(pkg, engine):
    n, nmesh = 16, 32
    pos, mass, box = pkg.ics.s_zel(n)
    types = tracer_types(len(pos))
    _setup(engine, box, n, nmesh)
    engine.gravpm_set_hybrid_nu_tracer(True)
    try:
        for resp in (None, synthetic_response([])):
            engine.gravpm_set_nu_response(resp, box / 1000.0)
            P = pkg.make_particles(pos, mass, type=types)
            engine.gravpm_force(P)
            gpm, pot, _, _ = composed(pos, mass, box, nmesh, None if resp is None else synthetic_response([]), deposit=types != 2)
            assert _close(P["GravPM"], gpm, 1e-11) and _close(P["Potential"], pot, 1e-11)
            assert np.abs(P["GravPM"][types == 2]).max() > 0     # the tracers are read out
    finally:
        engine.gravpm_set_hybrid_nu_tracer(False)
        engine.gravpm_set_nu_response(None)
    P = pkg.make_particles(pos, mass, type=types)
    engine.gravpm_force(P)
    g0, p0 = O.gravpm_force(pos, mass, box, nmesh, 1.5, G)
    assert _close(P["GravPM"], g0, 1e-11) and _close(P["Potential"], p0, 1e-11)


@pytest.mark.gpu
def test_nu_response_errors(pkg, engine):
    n, nmesh = 16, 32
    pos, mass, box = pkg.ics.s_zel(n)
    _setup(engine, box, n, nmesh)

    def boom(k, d, m):
        raise RuntimeError("no table")
    bad = [boom,
           lambda k, d, m: (np.log(k)[::-1].copy(), np.zeros_like(k), 0.07, 1.05),          # logknu not increasing
           lambda k, d, m: (np.log(k), np.full_like(k, np.nan), 0.07, 1.05)]               # not finite
    for fn in bad:
        engine.gravpm_set_nu_response(fn, box / 1000.0)
        P = pkg.make_particles(pos, mass)
        with pytest.raises(pkg.EngineError, match="neutrino response"):
            engine.gravpm_force(P)
        if fn is boom:
            assert isinstance(engine.gravpm_nu_response_error(), RuntimeError)
        engine.gravpm_set_nu_response(synthetic_response([]), box / 1000.0)
        P = pkg.make_particles(pos, mass)
        engine.gravpm_force(P)
        gpm, _, _, _ = composed(pos, mass, box, nmesh, synthetic_response([]))
        assert _close(P["GravPM"], gpm, 1e-11)
    engine.gravpm_set_nu_response(None)


def _run_helper(tmp_path, name, n, nmesh, env_extra, nproc=1, port=29571):
    out = str(tmp_path / name)
    env = dict(os.environ, MPG_DIST_BACKEND="gloo", MASTER_ADDR="127.0.0.1", **env_extra)
    script = os.path.join(ROOT, "tools", "mgpu_nu_check.py")
    if nproc == 1:
        cmd = [sys.executable, script, out, str(n), str(nmesh)]
    else:
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(nproc), "--master-addr", "127.0.0.1",
               "--master-port", str(port), script, out, str(n), str(nmesh)]
    run_ranks(cmd, env, out, timeout=600)
    return [dict(np.load(out + ".rank%d.npz" % r)) for r in range(nproc)]


@pytest.mark.gpu
@pytest.mark.parametrize("var", ["MPG_PM_FUSE_PS=0", "MPG_PM_KSPACE_FORCE=1"])
@keep_artifacts_on_failure
def test_nu_response_transfer_variants(pkg, tmp_path, var):
    n, nmesh = 16, 32
    pos, mass, box = pkg.ics.s_zel(n)
    k, v = var.split("=")
    r = _run_helper(tmp_path, "var", n, nmesh, {k: v, "MPG_NU_MODE": "single", "MPG_NU_HYBRID": "0"})[0]
    gpm, pot, spec, _ = composed(pos, mass, box, nmesh, synthetic_response([]))
    assert int(r["ncalls"]) == 2      # the host form and the device entry
    for g, p in (("gravpm_host", "pot_host"), ("gravpm_dev", "pot_dev")):
        assert _close(r[g], gpm, 1e-11) and _close(r[p], pot, 1e-11)
    assert np.abs(r["ps_P"] - spec[1]).max() <= 1e-12 * spec[1].max()


@pytest.mark.gpu
@pytest.mark.parametrize("nproc", [2, 4])
@keep_artifacts_on_failure
def test_nu_response_ranks(pkg, tmp_path, nproc):
    n, nmesh = 16, 32
    one = _run_helper(tmp_path, "one", n, nmesh, {"MPG_NU_MODE": "single", "MPG_NU_HYBRID": "1"})[0]
    ranks = _run_helper(tmp_path, "dist", n, nmesh, {"MPG_NU_MODE": "dist", "MPG_NU_HYBRID": "1"}, nproc=nproc, port=29571 + nproc)
    # the one-GPU run itself is the composition with the tracers left out of the deposit
    pos, mass, box = pkg.ics.s_zel(n)
    gpm, pot, _, _ = composed(pos, mass, box, nmesh, synthetic_response([]), deposit=tracer_types(len(pos)) != 2)
    assert _close(one["gravpm_host"], gpm, 1e-11) and _close(one["pot_host"], pot, 1e-11)
    for r in ranks:
        assert int(r["ncalls"]) == 2      # mpg_dist_gravpm_force and mpg_dist_gravity_step
        for c in range(2):
            for f in ("kk", "dcdm"):
                want = one["call0_%s" % f]
                assert np.abs(r["call%d_%s" % (c, f)] - want).max() <= 1e-12 * np.abs(want).max()
            assert np.array_equal(r["call%d_nmodes" % c], one["call0_nmodes"])
    r0 = ranks[0]
    for got, want in (("gravpm_host", "gravpm_host"), ("pot_host", "pot_host"), ("gravpm_step", "gravpm_host")):
        assert _close(r0[got], one[want], 1e-12), got
    assert np.array_equal(r0["ps_N"], one["ps_N"])
    assert np.abs(r0["ps_P"] - one["ps_P"]).max() <= 1e-12 * one["ps_P"].max()
