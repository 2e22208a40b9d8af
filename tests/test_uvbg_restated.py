"""The restatement of the excursion-set reionisation model (tests/uvbg_restated.py) on its own, without a GPU: the conditions its scenes must
meet for the GPU test (tests/test_gpu_uvbg.py) to be a test of decisions, and the host-side rules.

A cell whose f_coll eff lies within rounding of the barrier 1, or whose filtered mass is rounding noise, has no decision to compare.  The
GPU test leaves such cells out; HERE the scenes are held to having (next to) none, so that leaving them out cannot hide an error: 0
degenerate cells and at most 0.1 % of the cells with a margin below 1e-9 in every scene but "void".  A scene that fails this is to be
changed, never the cap."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import uvbg_restated as U

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONFIGS = ((0, 0, 0), (1, 0, 0), (2, 0, 0), (0, 1, 0), (0, 0, 1))      # (ReionFilterType, RtoMFilterType, ReionUseParticleSFR)
MARGIN, CAP = 1e-9, 1e-3


@pytest.mark.parametrize("cfg", CONFIGS, ids=lambda c: "f%d-m%d-sfr%d" % c)
@pytest.mark.parametrize("name", ["d16", "d24"])
def test_scenes_have_decisions(name, cfg):
    r = U.reference(name, *cfg)
    ion = r["xHI"] == 0
    nrad = np.unique(r["first_crossing"][ion]).size
    print("%s %s: %d radii, %.2f %% ionised over %d first-crossing radii, smallest margin %.3g" % (name, cfg, len(r["radii"]), 100 * ion.mean(), nrad,
                                                                                                 r["margin"].min()))
    assert r["degenerate"].sum() == 0
    assert (r["margin"] < MARGIN).sum() <= CAP * ion.size
    assert nrad >= 10 and ion.mean() >= 0.01
    if cfg == (0, 0, 0):
        assert 0.03 <= ion.mean() <= 0.10
    assert not np.isnan(r["xHI"]).any() and not np.isnan(r["J21"]).any()
    part = (r["xHI"] > 0) & (r["xHI"] < 1)
    assert part.sum() >= 20                                             # the partial ionisation of the last step is exercised
    assert 0 < float(r["volume_weighted_global_xHI"]) < 1 and 0 < float(r["mass_weighted_global_xHI"]) < 1


def test_void_has_degenerate_cells():
    r = U.reference("void")
    assert r["degenerate"].sum() >= 100 and (~r["degenerate"]).sum() >= 1000
    assert np.isfinite(r["J21"]).all()


@pytest.mark.parametrize("cfg", CONFIGS, ids=lambda c: "f%d-m%d-sfr%d" % c)
@pytest.mark.parametrize("name", ["d16", "d24"])
def test_fp64_makes_the_same_decisions(name, cfg):
    """the same statements in fp64 decide every cell as the long-double ones do, and the float grids agree to a float ulp"""
    a, b = U.reference(name, *cfg), U.reference(name, *cfg, precision="f64")
    assert np.array_equal(a["xHI"] == 0, b["xHI"] == 0)
    assert np.array_equal(a["first_crossing"], b["first_crossing"])
    assert np.all(np.abs(a["J21"].astype(np.float64) - b["J21"]) <= 1.2e-7 * np.abs(a["J21"]))
    assert np.abs(a["xHI"].astype(np.float64) - b["xHI"]).max() <= 1.2e-7


@pytest.mark.parametrize("name", ["d16", "d24"])
def test_float_filter_is_the_defined_difference(name):
    """the real-space top hat the reference's way (sinf / cosf / powf): how far it moves the result (printed), and that it stays a matter of
    cells at the barrier: no more decisions flip than the cap on undecided cells allows"""
    a, b = U.reference(name), U.reference(name, float_filter=True)
    flips = ((a["xHI"] == 0) != (b["xHI"] == 0)).sum()
    both = (a["J21"] > 0) & (b["J21"] > 0) & (a["first_crossing"] == b["first_crossing"])
    dj = np.abs(a["J21"].astype(np.float64) - b["J21"])[both] / a["J21"][both]
    dx = np.abs(a["xHI"].astype(np.float64) - b["xHI"])
    print("%s float filter: %d of %d decisions flip, J21 moves by %.3g relative, xHI by %.3g" % (name, flips, a["xHI"].size, dj.max(), dx.max()))
    assert flips <= CAP * a["xHI"].size
    assert dj.max() < 1e-4 and dx.max() < 1e-2


RADII_CASES = ((3000.0, 100.0, 1.1, 10000.0, 16),      # stops by the cell size (625 > Rmin)
               (3000.0, 100.0, 1.1, 10000.0, 256),     # stops by Rmin
               (20000.0, 100.0, 1.1, 10000.0, 24),     # Rmax > Box: starts at the box
               (30.0, 0.5, 1.1, 400.0, 128),           # the reference's comment: 30 Mpc to 0.5 Mpc at 1.1
               (3000.0, 2999.0, 1.0000001, 10000.0, 64),  # MAX_R_ITERATIONS ends the loop
               (50.0, 100.0, 1.3, 10000.0, 32),        # Rmax < Rmin: the unfiltered step alone
               (1000.0, 1.0, 3.0, 999.0, 27))


@pytest.mark.parametrize("case", RADII_CASES, ids=lambda c: "-".join("%g" % x for x in c))
def test_radii_follow_the_c_loop(case, tmp_path):
    if not shutil.which("gcc"):
        pytest.skip("no gcc")
    exe = str(tmp_path / "uvbg_radii")
    r = subprocess.run(["gcc", "-O0", "-std=gnu11", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off", os.path.join(ROOT, "tests", "c", "uvbg_radii.c"),
                        "-o", exe, "-lm"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe] + [repr(x) for x in case], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0
    want = [float.fromhex(s) for s in r.stdout.split()]
    got = U.radii(*case)
    assert got == want
    assert got[-1] == case[3] / case[4] and len(got) <= U.MAX_R_ITERATIONS + 1


def test_gas_escape_fraction_continue():
    """uvbg.c:483: without ReionUseParticleSFR a gas row keeps the halo mass in its EscapeFraction; stars are always converted; 0 stays 0;
    the clamp at 1 is exact"""
    ptype = np.array([0, 0, 4, 4, 4, 1, 0, 5], np.uint8)
    halo = np.array([2.0, 0.0, 2.0, 0.0, 1e4, 3.0, 1e4, 4.0])
    conv = np.longdouble(U.PAR["UnitMass_in_g"]) / np.longdouble(U.SOLAR_MASS) / np.longdouble(1e10) / np.longdouble(U.PAR["HubbleParam"])
    want2 = np.longdouble(0.3) * np.sqrt(np.longdouble(2.0) * conv)
    off = U.init_particles(ptype, halo, dict(U.PAR, ReionUseParticleSFR=0))
    assert off[0] == 2.0 and off[6] == 1e4 and off[1] == 0            # gas: untouched
    assert abs(off[2] - want2) < 1e-18 and off[3] == 0 and off[4] == 1
    assert off[5] == 3.0 and off[7] == 4.0
    on = U.init_particles(ptype, halo, dict(U.PAR, ReionUseParticleSFR=1))
    assert abs(on[0] - want2) < 1e-18 and on[1] == 0 and on[6] == 1
    assert np.array_equal(on[2:6], off[2:6]) and on[7] == 4.0
    with pytest.raises(ValueError, match="negative escape fraction"):
        U.init_particles(ptype, halo, dict(U.PAR, EscapeFractionNorm=-0.3))


def test_zreion_rule():
    z = U.zreion_rule(np.array([-1.0, -1.0, 9.5, 9.5, -3.0]), np.array([True, False, True, False, True]), 0.125)
    assert np.array_equal(z, [7.0, -1.0, 9.5, 9.5, -3.0])
    r, S = U.reference("d16"), U.scene("d16")
    gas = S["type"] == 0
    took = r["local_J21"] > 0
    assert took[gas].sum() >= 100 and not took[~gas].any()
    assert np.all(r["zreion"][took & (S["zreion"] == -1)] == 7.0) and (took & (S["zreion"] == 9.5)).sum() >= 10
    assert np.array_equal(r["zreion"][~took], S["zreion"][~took]) and np.all(r["zreion"][took & (S["zreion"] == 9.5)] == 9.5)
