"""The two kernels of the PM step that were rebuilt for fewer memory requests (csrc/pm.hip), each against the long-double restatement
of tests/pm_restated.py at the sizes where its new indexing can go wrong (pm_requests_sets.py lists the sets and why):

  k_cic_deposit           two lanes per particle, the corners with z-bit 0 and 1: half a pair-wave, a whole one, one over, the block edge,
                          the z wrap between the two lanes of a pair (Nmesh 8), dead records, positions whole boxes outside
  k_xpass_solve           2-D transforms over (y, z) around one fused pass along x (transform, P(k), potential factor, transform back)
                          at Nmesh 64 and 128 (every shift of a row against the 128-byte lines, ragged first and last tiles): forces,
                          potential and the bins of P(k); MPG_PM_XPASS=0 and the cases that keep the 3-D plans

Tolerance, SURVEY 8(d): max |dGravPM| <= 1e-11 mean |GravPM|, the same for the potential; P(k) as test_gpu_pm_forms.py: the mode counts
equal, k to 1e-12, P to 1e-9.  The fp64 conditioning of every set: test_pm_requests_inputs.py."""
import numpy as np
import pytest

import pm_requests_sets as S
import pm_restated as R
from test_gpu_pm_forms import POT0, TOL, _pin, _upload, dev_step, host_step, own_engines

pytestmark = pytest.mark.gpu


def check(name, gpm, pot, what=""):
    """the bound of the module docstring against the long-double result of the named set; the figures are printed first (pytest -s)"""
    g_ld, p_ld = S.reference(name)
    fs, ps = S.force_scale(name)
    dg = float(np.abs(gpm - g_ld).max() / fs)
    dp = float(np.abs(pot - (p_ld + POT0)).max() / ps)
    print("%s %s: GravPM %.2e  Potential %.2e (of the mean)" % (name, what, dg, dp))
    assert dg <= TOL and dp <= TOL, (name, what, dg, dp)


def _xpass(monkeypatch, on):
    if on:
        monkeypatch.delenv("MPG_PM_XPASS", raising=False)
    else:
        monkeypatch.setenv("MPG_PM_XPASS", "0")


# ------------------------------------------------------------------------------------------------ deposit: two lanes per particle
@pytest.mark.parametrize("name", S.PAIR_SETS)
def test_deposit_pairs(pkg, monkeypatch, name):
    """N = 1 .. 129 and 3001, all in one cell and in runs, Nmesh 8 (z wrap inside a pair for an eighth of the particles) and 40"""
    pos, mass, box, nmesh = S.input_set(name)
    _pin(monkeypatch, "plain")
    with own_engines(pkg, box, nmesh) as (eng,):
        d_pos, d_mass, _ = _upload(pos, mass)
        check(name, *dev_step(eng, d_pos, d_mass, box), what="pairs")


def test_deposit_pairs_z_wrap_is_exercised():
    """at Nmesh 8 the sets do hold particles in the last z-plane, whose pair of lanes writes cells iz = 7 and 0"""
    for name in ("runs-3001-8", "runs-129-8", "runs-64-8"):
        pos, _, box, nmesh = S.input_set(name)
        iz = R.cells(pos, box, nmesh)[0][:, 2]
        assert np.any(iz == nmesh - 1), name


def test_deposit_pairs_dead_records(pkg, monkeypatch):
    """a third of the table dead (both lanes of a dead record's pair leave): the live records get the result of the live set alone"""
    pos, mass, box, dead = R.pile_with_dead()
    _pin(monkeypatch, "plain")
    with own_engines(pkg, box, 40) as (eng,):
        P = pkg.make_particles(pos, mass)
        di = np.flatnonzero(dead)
        P["Flags"][di[0::2]] = 1                          # IsGarbage
        P["Flags"][di[1::2]] = 2                          # Swallowed ...
        P["Type"][di[1::2]] = 5                           # ... black holes
        P["Potential"] = POT0
        P["GravPM"] = 7.0
        eng.gravpm_force(P)
        check("pile-live", P["GravPM"][~dead], P["Potential"][~dead], what="pairs/dead records")
        assert np.all(P["GravPM"][di] == 0.0) and np.all(P["Potential"][di] == POT0)


def test_deposit_pairs_positions_whole_boxes_outside(pkg, monkeypatch):
    name = "pile-shift"
    pos, mass, box, nmesh = S.input_set(name)
    _pin(monkeypatch, "plain")
    with own_engines(pkg, box, nmesh) as (eng,):
        d_pos, d_mass, _ = _upload(pos, mass)
        check(name, *dev_step(eng, d_pos, d_mass, box), what="pairs/shifted")


# ------------------------------------------------------------------------------------------------ the fused x-pass
@pytest.mark.parametrize("xpass", [True, False], ids=["xpass", "plans3d"])
@pytest.mark.parametrize("name", S.XPASS_SETS)
def test_xpass_forces_potential_spectrum(pkg, monkeypatch, name, xpass):
    """Nmesh 64 and 128, clustered and Zel'dovich-like: the default path (k_xpass_solve) and, with MPG_PM_XPASS=0, the 3-D plans on the
    same inputs under the same bounds"""
    pos, mass, box, nmesh = S.input_set(name)
    _pin(monkeypatch, "plain")
    _xpass(monkeypatch, xpass)
    with own_engines(pkg, box, nmesh) as (eng,):
        d_pos, d_mass, _ = _upload(pos, mass)
        res = dev_step(eng, d_pos, d_mass, box)
        k, P, N = eng.gravpm_get_powerspectrum(nmesh, box / 1000.0)
    check(name, *res, what="xpass" if xpass else "3-D plans")
    kl, Pl, Nl, _ = S.spectrum(name)
    assert np.array_equal(N, Nl) and N.sum() == nmesh ** 3 - 1
    dk, dP = float(np.abs(k / kl - 1).max()), float(np.abs(P / Pl - 1).max())
    print("%s %s: k %.2e  P %.2e" % (name, "xpass" if xpass else "3-D plans", dk, dP))
    assert dk <= 1e-12 and dP <= 1e-9


def test_xpass_repeats_on_one_engine(pkg, monkeypatch):
    """the same engine, three steps, the x-pass switched off for the second: plans of both forms side by side, P(k) zeroed every step"""
    name = "xclust-64"
    pos, mass, box, nmesh = S.input_set(name)
    _pin(monkeypatch, "plain")
    with own_engines(pkg, box, nmesh) as (eng,):
        d_pos, d_mass, _ = _upload(pos, mass)
        for on in (True, False, True):
            _xpass(monkeypatch, on)
            check(name, *dev_step(eng, d_pos, d_mass, box), what="step with xpass=%s" % on)
            N = eng.gravpm_get_powerspectrum(nmesh, box / 1000.0)[2]
            assert N.sum() == nmesh ** 3 - 1


@pytest.mark.parametrize("case", ["transfer_alone", "kspace", "nmesh72"])
def test_xpass_cases_that_keep_the_3d_plans(pkg, monkeypatch, case):
    """gravpm_measure_power(False), MPG_PM_KSPACE_FORCE=1 and a mesh the kernel is not built for (72): the step passes as before"""
    name = "clust-72" if case == "nmesh72" else "xclust-64"
    pos, mass, box, nmesh = S.input_set(name)
    _pin(monkeypatch, "plain", kspace=case == "kspace")
    _xpass(monkeypatch, True)
    with own_engines(pkg, box, nmesh) as (eng,):
        if case == "transfer_alone":
            eng.gravpm_measure_power(False)
        check(name, *host_step(pkg, eng, pos, mass), what=case)
