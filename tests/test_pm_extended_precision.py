"""The fp64 PM oracles against the long-double restatement (tests/pm_restated.py), on every input set the GPU tests of
test_gpu_pm_forms.py feed.  No GPU.

The GPU tolerance of the PM is 1e-11 of the mean force / potential.  It only means something on an input where fp64
itself - CIC in double, pocketfft in double, the Fourier-space force_transfer - stays well inside it.  The condition here is a tenth
of it, 1e-12 of the mean, for oracle.gravpm_force (numpy) and gravpm_force_c (pm_oracle.c + scipy.fft): an input that fp64 cannot
hold to that is caught here and has to be replaced, instead of showing up as a flaky GPU test.  Since the long-double forces come from
the real-space 4-point stencil and the oracles' from force_transfer in Fourier space, the same comparison is the independent check
that the two are one operator.

Measured (max deviation over the particles, relative to the mean; numpy oracle / C oracle - the C oracle's deposit is threaded, its
last digit moves from run to run), the four sets of the table:

    set     N      Nmesh   GravPM               Potential
    grid    4096   32      3.3e-14 / 3.9e-14    3.0e-14 / 3.6e-14
    clust   8000   48      1.2e-14 / 1.2e-14    2.1e-15 / 2.2e-15
    zel     13824  48      6.0e-15 / 5.6e-15    3.6e-15 / 3.3e-15
    pile    12000  40      2.8e-14 / 2.8e-14    2.9e-15 / 3.2e-15

(test_table_sets prints them: pytest -s.)  Every other set is below 3.3e-14 but the shifted pile - positions up to 5 boxes out, whose
pos / cell carries the rounding of a number six times as large: oracle(shifted) against long double(shifted) 9.0e-14, long
double(shifted) against long double(unshifted) 1.7e-13, oracle(shifted) against long double(unshifted) 2.5e-13 in the force (potential
below 1e-14).  That margin of 4 is the thinnest: shifts stay at or below 5 boxes."""
import numpy as np
import pytest

import pm_restated as R
from oracle import oracle as O

COND = 1e-12


def _deviation(name, orc=None):
    pos, mass, box, nmesh = R.input_set(name)
    g_ld, p_ld = R.reference(name)
    fs, ps = R.force_scale(name)
    if orc is None:
        g, p = O.gravpm_force(pos, mass, box, nmesh, 1.5, R.G)
    else:
        g, p = O.gravpm_force_c(orc, pos, mass, box, nmesh, 1.5, R.G)
    return float(np.abs(g - g_ld).max() / fs), float(np.abs(p - p_ld).max() / ps)


def test_long_double_is_long_double():
    """what pm_restated asserts on import, stated as a test: 80-bit long double, transforms that keep it"""
    assert np.finfo(np.longdouble).eps < 1.1e-19
    x = np.linspace(np.longdouble(0), np.longdouble(1), 4 ** 3).reshape(4, 4, 4)
    assert np.fft.rfftn(x).dtype == np.clongdouble


def test_cells_are_the_fp64_decision_and_fold_any_number_of_boxes():
    box, nmesh = 100.0, 40
    pos = np.array([[0.0, box, np.nextafter(box, 0.0)], [-1e-13, box + 1e-13, 2.5], [5 * box + 2.6, -3 * box + 2.4, -box]])
    ic, res = R.cells(pos, box, nmesh)
    assert np.array_equal(ic, [[0, 0, int(np.floor(np.nextafter(box, 0.0) / 2.5)) % nmesh], [nmesh - 1, 0, 1], [1, 0, 0]])
    assert res.dtype == np.longdouble and np.all(res > -1e-15) and np.all(res < 1 + 1e-15)
    w = sum(w for _, w in R._corners(ic, res, nmesh))
    assert np.abs(w - 1).max() < 1e-18                    # the 8 weights of a particle sum to 1


def test_deposit_conserves_mass_and_honours_the_live_mask():
    pos, mass, box, dead = R.pile_with_dead()
    rho = R.cic_deposit_ld(pos, mass, box, 40, live=~dead)
    want = mass[~dead].astype(np.longdouble).sum()
    assert abs(rho.sum() - want) <= 1e-17 * want
    rho2 = R.cic_deposit_ld(pos[~dead], mass[~dead], box, 40)
    assert np.abs(rho - rho2).max() <= 1e-17 * np.abs(rho2).max()


@pytest.mark.parametrize("name", ["clust", "pile"])
def test_stencil_is_force_transfer_in_long_double(name):
    """the real-space 4-point stencil and the Fourier-space force_transfer agree to long-double rounding: they are one operator"""
    g_s, p_s = R.reference(name)
    g_k, p_k = R.reference(name, kspace=True)
    d = float(np.abs(g_s - g_k).max() / np.abs(g_s).mean())
    print("%s: stencil against k-space forces in long double: %.2e of the mean" % (name, d))
    assert d <= 1e-15                                     # four more long-double transforms: ~1e3 eps at most
    assert np.array_equal(p_s, p_k)


def test_table_sets(orc):
    """the four sets of the docstring's table, printed"""
    for name in R.TABLE_SETS:
        pos, _, _, nmesh = R.input_set(name)
        dn, dc = _deviation(name), _deviation(name, orc)
        print("%-6s N %5d Nmesh %2d  GravPM %.1e / %.1e  Potential %.1e / %.1e" % (name, len(pos), nmesh, dn[0], dc[0], dn[1], dc[1]))
        assert max(dn + dc) <= COND, (name, dn, dc)


@pytest.mark.parametrize("name", [n for n in R.ALL_SETS if n not in R.TABLE_SETS])
def test_fp64_oracles_within_a_tenth_of_the_gpu_tolerance(orc, name):
    dn, dc = _deviation(name), _deviation(name, orc)
    print("%s: GravPM %.1e / %.1e  Potential %.1e / %.1e" % (name, dn[0], dc[0], dn[1], dc[1]))
    assert max(dn + dc) <= COND, (name, dn, dc)


def test_whole_box_shifts_change_nothing_but_rounding():
    """a fifth of the pile moved by -3 .. +5 whole boxes: the oracle and the long-double result of the shifted set equal the results of
    the unshifted one to 1e-12 of the mean (not exactly: pos / cell of a shifted position rounds differently)"""
    pos, mass, box, nmesh = R.input_set("pile")
    spos, _, _, _ = R.input_set("pile-shift")
    moved = np.any(spos != pos, axis=1)
    assert abs(moved.mean() - 0.2) < 0.01 and np.abs(np.round((spos - pos) / box)).max() == 5 and np.array_equal((spos - pos)[~moved], 0 * pos[~moved])
    assert spos.min() < -2 * box and spos.max() > 5 * box
    g0, p0 = R.reference("pile")
    g1, p1 = R.reference("pile-shift")
    go, po = O.gravpm_force(spos, mass, box, nmesh, 1.5, R.G)
    fs, ps = R.force_scale("pile")
    fig = [float(np.abs(a - b).max() / s) for a, b, s in ((go, g1, fs), (g1, g0, fs), (go, g0, fs), (po, p1, ps), (p1, p0, ps), (po, p0, ps))]
    print("shifted pile, forces: oracle-ld(shifted) %.1e  ld(shifted)-ld %.1e  oracle(shifted)-ld %.1e;  potential %.1e %.1e %.1e" % tuple(fig))
    assert max(fig) <= COND, fig


@pytest.mark.parametrize("name", ["clust", "pile"])
def test_power_spectrum_oracle_against_long_double(name):
    """oracle.pm_power_spectrum (fp64) against the long-double accumulators: the tolerances of test_pm_power_spectrum"""
    pos, mass, box, nmesh = R.input_set(name)
    mpc = box / 1000.0
    k, P, N = O.pm_power_spectrum(pos, mass, box, nmesh, mpc)
    kl, Pl, Nl, raw = R.power_spectrum_ld(pos, mass, box, nmesh, mpc)
    assert np.array_equal(N, Nl) and N.sum() == nmesh ** 3 - 1
    assert np.abs(k / kl - 1).max() <= 1e-12 and np.abs(P / Pl - 1).max() <= 1e-9
    m = mass.astype(np.longdouble).sum()
    assert abs(raw[3] / (m * m) - 1) < 1e-17             # Norm = |rho_0|^2 = (total mass)^2
