"""The fp64 PM oracle against the long-double restatement on the input sets of test_gpu_pm_requests.py (pm_requests_sets.py).  No GPU.

As test_pm_extended_precision.py does for the sets of test_gpu_pm_forms.py: the GPU bound, 1e-11 of the mean force / potential, tests a
kernel only on an input that fp64 itself - CIC in double, pocketfft in double - holds to a tenth of it.  A set that fp64 cannot hold to
1e-12 is caught here and has to be replaced."""
import numpy as np
import pytest

import pm_requests_sets as S
import pm_restated as R
from oracle import oracle as O

COND = 1e-12


@pytest.mark.parametrize("name", S.ALL_SETS)
def test_fp64_oracle_within_a_tenth_of_the_gpu_tolerance(name):
    pos, mass, box, nmesh = S.input_set(name)
    g_ld, p_ld = S.reference(name)
    fs, ps = S.force_scale(name)
    g, p = O.gravpm_force(pos, mass, box, nmesh, 1.5, R.G)
    dg, dp = float(np.abs(g - g_ld).max() / fs), float(np.abs(p - p_ld).max() / ps)
    print("%s: N %d Nmesh %d  GravPM %.1e  Potential %.1e" % (name, len(pos), nmesh, dg, dp))
    assert max(dg, dp) <= COND, (name, dg, dp)


@pytest.mark.parametrize("name", S.XPASS_SETS)
def test_power_spectrum_oracle_against_long_double(name):
    """oracle.pm_power_spectrum (fp64) on the x-pass sets, as test_pm_extended_precision.py holds it on its sets: the mode counts equal and
    the tolerances the GPU test asserts (k is a sum of ~1e4 square roots per bin in fp64: 1e-13 at Nmesh 128)"""
    pos, mass, box, nmesh = S.input_set(name)
    k, P, N = O.pm_power_spectrum(pos, mass, box, nmesh, box / 1000.0)
    kl, Pl, Nl, _ = S.spectrum(name)
    assert np.array_equal(N, Nl) and N.sum() == nmesh ** 3 - 1
    dk, dP = float(np.abs(k / kl - 1).max()), float(np.abs(P / Pl - 1).max())
    print("%s: k %.1e  P %.1e" % (name, dk, dP))
    assert dk <= 1e-12 and dP <= 1e-9
