"""tests/uvfluc_restated.py against the reference's own assertions on its interpolator (libgadget/tests/test_interp.c:40-70, restated with
its grid and function), and the conditions tests/test_gpu_uvfluc.py rests on, asserted on the restatement alone so that the GPU tests
cannot hide behind them: every class of row is there in numbers, the cells wrap on both sides, no row sits on a decision, and the dark
background is visible in what a star-forming row gets."""
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

import cooling_restated as R
import sfr_restated as SF
import test_cooling_restated as K
import uvfluc_restated as U

G = K.G
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the interpolator -------------------------------------------------------------------------------------------------------------------------
def modulus(x, mod):                                                  # test_interp.c:15-20
    if x >= 0:
        return math.fmod(x, mod)
    return math.fmod(x + mod, mod)


def test_interp_periodic_passes_the_reference_assertions():
    """test_interp.c:24-75 as far as it concerns interp_eval_periodic: DSIZE = 3, two dimensions, ydata = |(1 - j)(1 - i)| and i + j"""
    DSIZE = 3
    ip = U.Interp([DSIZE, DSIZE])
    ip.init_dim(0, 0, DSIZE - 1)
    ip.init_dim(1, 0, DSIZE - 1)
    ydata = [abs((1. - j) * (1. - i)) for i in range(DSIZE) for j in range(DSIZE)]
    ydata_sum = [float(i + j) for i in range(DSIZE) for j in range(DSIZE)]
    clamp = lambda v: max(min(v, DSIZE - 1), 0)
    checked = 0
    i = -0.4
    while i <= DSIZE:                                                 # :44-60
        j = -0.4
        while j <= DSIZE:
            yp = U.interp_eval_periodic(ip, [i, j], ydata)
            y_truth = abs((1. - clamp(i)) * (1. - clamp(j)))
            assert abs(yp - y_truth) <= 1e-5 * yp, (i, j, yp, y_truth)
            checked += 1
            j += 0.4
        i += 0.4
    i = -0.4
    while i <= 3.0:                                                   # :62-75
        j = -0.4
        while j <= 3.0:
            yp = U.interp_eval_periodic(ip, [i, j], ydata_sum)
            yp_truth = modulus(i, DSIZE) + modulus(j, DSIZE)
            if i >= 0 and j >= 0 and i <= DSIZE - 1 and j <= DSIZE - 1:
                assert abs(yp - yp_truth) <= 1e-5 * yp, (i, j, yp, yp_truth)
                checked += 1
            j += 0.4
        i += 0.4
    assert checked > 100


def test_grid_points_and_wraps():
    """the table entry exactly at grid points; between -3 and +4 box lengths the `while` wrap and the integer modulo give the same bits; the
    period is Nside cells of BoxSize / (Nside - 1), not BoxSize"""
    for Nside, box in ((2, 1.0), (5, 1.0), (16, 8.0)):
        table = U.synthetic_zreion_table(Nside, 7.0, Nside)
        uvf = U.UVF(table, box)
        step = box / (Nside - 1)
        for (a, b, c) in [(0, 0, 0), (Nside - 1, 0, 1), (1, Nside - 1, Nside - 1), (Nside - 1,) * 3]:
            assert uvf.zreion((a * step, b * step, c * step), (0.0, 0.0, 0.0)) == table[a, b, c]
        # one cell beyond the last point is the first again: x = Nside * step reads entry 0
        assert uvf.zreion((Nside * step, 0.0, 0.0), (0.0, 0.0, 0.0)) == table[0, 0, 0]
        assert uvf.zreion((-step, 0.0, 0.0), (0.0, 0.0, 0.0)) == table[Nside - 1, 0, 0]
        rs = np.random.RandomState(Nside)
        pts = rs.uniform(-3 * box, 4 * box, (600, 3))
        wrapped = 0
        for x in pts:
            w = U.interp_eval_periodic(uvf.interp, list(x), uvf.Table)
            m = U.interp_eval_periodic(uvf.interp, list(x), uvf.Table, modulo=True)
            assert w == m and table.min() <= w <= table.max()
            xi, _ = U.interp_cells(uvf.interp, list(x))
            wrapped += any(c < -Nside or c >= 2 * Nside for c in xi)
        assert wrapped > 100                                          # cells more than one period away on either side


# ---- the input sets ---------------------------------------------------------------------------------------------------------------------------
def zreion_of_rows(d, pos, uvf):
    gas = np.nonzero((d["type"] == 0) & (d["mass"] > 0))[0]
    z = np.array([uvf.zreion(pos[p], U.OFFSET) for p in gas])
    cells = np.array([U.interp_cells(uvf.interp, [pos[p][k] - U.OFFSET[k] for k in range(3)])[0] for p in gas])
    return gas, z, cells


def test_cooling_set_at_reionisation():
    """sherwood_reion (z = 15, HIReionTemp = 2e4, even bins lastred = 15.3, odd bins 15.05): the three classes, the wraps, the margins"""
    C, times, step, d, pos, uvf = U.cooling_set("sherwood_reion", G["treecool"])
    assert len(d["type"]) == 1000 and uvf.Nside == 5 and U.BOXSIZE == 1.0 and U.OFFSET == (0.11, -0.07, 0.2)
    redshift = 1. / times["atime"] - 1
    assert redshift == 15 and C.p["HIReionTemp"] == 2e4
    assert (step["lastred"][0::2] == 15.3).all() and (step["lastred"][1::2] == 15.05).all()
    assert pos.min() >= -0.25 and pos.max() < 1.25 and pos.min() < -0.24 and pos.max() > 1.24
    gas, z, cells = zreion_of_rows(d, pos, uvf)
    last = step["lastred"][d["tb_hydro"][gas]]
    cls = np.array([U.row_class(z[k], redshift, last[k]) for k in range(len(gas))])
    frac = [float((cls == c).mean()) for c in (U.DARK, U.WINDOW, U.LIT)]
    outside = ((cells < 0) | (cells >= uvf.Nside - 1)).any(axis=1).mean()
    margin = min(np.abs(z - redshift).min(), np.abs(z - last).min())
    print("cooling set at z = 15: dark %.0f %%, window %.0f %%, lit %.0f %% of %d treated rows; %.0f %% with a cell outside [0, Nside - 1); "
          "nearest decision %.1e" % (100 * frac[0], 100 * frac[1], 100 * frac[2], len(gas), 100 * outside, margin))
    assert min(frac) >= 0.10
    assert outside >= 0.20 and (cells < 0).any() and (cells >= uvf.Nside - 1).any()
    assert margin >= 1e-9
    assert step["uvbg"]["gJH0"] > 0                                   # the global background is on: dark rows differ from lit ones


def test_cooling_set_with_metals():
    """sherwood_z3 (metals, helium heating, HIReionTemp = 0) with a table around z = 3 and the same positions: dark and lit rows"""
    C, times, step, d, pos, uvf = U.cooling_set("sherwood_z3", G["treecool"])
    assert len(d["type"]) == 1000 and C.p["HIReionTemp"] == 0 and C.metal is not None and C.p["HeliumHeatOn"] == 1
    assert np.array_equal(pos, U.positions(1000))
    redshift = 1. / times["atime"] - 1
    gas, z, cells = zreion_of_rows(d, pos, uvf)
    dark = float((z < redshift).mean())
    print("cooling set at z = 3: dark %.0f %%, lit %.0f %% of %d treated rows; nearest decision %.1e" % (100 * dark, 100 * (1 - dark), len(gas), np.abs(z - redshift).min()))
    assert dark >= 0.25 and 1 - dark >= 0.25
    assert np.abs(z - redshift).min() >= 1e-9


def test_star_formation_set():
    """the `heating` setting with the z = 3 table: dark and lit star-forming rows, and the dark background shows in what they get"""
    S, times, step, d, pos, uvf = U.sfr_set(G["treecool"])
    n = len(d["type"])
    assert n == 1200 and U.SFR_SET["name"] == "heating"
    redshift = 1. / times["atime"] - 1
    a3inv = 1. / times["atime"] ** 3
    rnd = SF.random_table()
    base = SF.cooling_and_starformation(S, d, times, step, rnd, wind=SF.WIND, cool=False)      # the classes do not depend on the background
    sf = np.nonzero(base["cls"] == SF.ROW_STARFORMING)[0]
    z = np.array([uvf.zreion(pos[p], U.OFFSET) for p in sf])
    dark = z < redshift
    print("star-formation set: %d star-forming rows, %.0f %% dark, %.0f %% lit; nearest decision %.1e" % (len(sf), 100 * dark.mean(), 100 * (1 - dark.mean()),
                                                                                                       np.abs(z - redshift).min()))
    assert len(sf) > 300 and dark.mean() >= 0.10 and 1 - dark.mean() >= 0.10
    assert np.abs(z - redshift).min() >= 1e-9
    told_apart = 0
    for p, zr in zip(sf[dark], z[dark]):
        local = U.get_local_UVBG_from_global(redshift, step["uvbg"], pos[p], U.OFFSET, uvf)
        assert local["gJH0"] == 0 and local["epsH0"] == 0 and local["self_shield_dens"] == step["uvbg"]["self_shield_dens"] and local["zreion"] == zr
        one = U._one(d, p)
        a = SF.cooling_and_starformation(S, one, times, dict(step, uvbg=local), rnd, wind=SF.WIND)
        b = SF.cooling_and_starformation(S, one, times, step, rnd, wind=SF.WIND)
        assert not a["failed"] and not b["failed"]
        rel = lambda k: abs(a[k][0] - b[k][0]) > 1e-6 * max(abs(a[k][0]), abs(b[k][0]))
        told_apart += bool(rel("entropy") or rel("sfr"))
    print("star-formation set: %d of %d dark star-forming rows get another Entropy or Sfr under the dark background" % (told_apart, int(dark.sum())))
    assert told_apart >= 50


def test_local_background_is_the_global_one_without_a_table():
    uv = dict(R.zero_uvbg(), gJH0=1e-12, zreion=7.5, self_shield_dens=0.01)
    assert U.get_local_UVBG_from_global(3.0, uv, (0.1, 0.2, 0.3), (0.0, 0.0, 0.0), None) == uv


# ---- the engine's own statement of the read, built for the host ----------------------------------------------------------------------------------
@pytest.mark.parametrize("Nside", (2, 5, 16))
def test_host_build_of_the_read_equals_the_restatement(tmp_path, Nside):
    """cool::uvf_zreion and cool::local_setup of csrc/cooling.h, built for the host with their own main (tests/c/uvfluc_host.cpp): zreion and
    every member of the local struct UVBG bit for bit the restatement's, on grid points, points many periods away on both sides and both
    sides of the redshift; a coordinate that is not finite or beyond 2^31 cells gives NaN"""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    inc = os.path.join(os.path.dirname(os.path.dirname(hipcc)), "include")
    if not shutil.which("g++") or not os.path.isdir(inc):
        pytest.fail("no g++ or no HIP headers: the host build of csrc/cooling.h cannot be checked")
    exe = str(tmp_path / "uvfluc_host")
    r = subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Wno-unused-function", "-Wno-unused-result", "-D__HIP_PLATFORM_AMD__", "-I", inc,
                        os.path.join(ROOT, "tests", "c", "uvfluc_host.cpp"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    box, redshift = 0.25 * (Nside - 1), 7.1
    table = U.synthetic_zreion_table(Nside, 7.0, 10 + Nside)
    uvf = U.UVF(table, box)
    rs = np.random.RandomState(Nside)
    period = 0.25 * Nside
    grid = 0.25 * rs.randint(-2 * Nside, 3 * Nside, (200, 3)) + np.array(U.OFFSET)
    pts = np.concatenate([grid, rs.uniform(-0.25 * box, 1.25 * box, (800, 3)), rs.uniform(-40 * period, 40 * period, (800, 3)),
                          [[box, 0.0, -box], [2000 * period + 0.1, -2000 * period - 0.1, 3.0]]])
    glob = dict(J_UV=1.5, gJH0=1e-12, gJHep=2e-14, gJHe0=3e-13, epsH0=4e-24, epsHep=5e-25, epsHe0=6e-24, self_shield_dens=0.007, zreion=9.25)
    keys = ("J_UV", "gJH0", "gJHep", "gJHe0", "epsH0", "epsHep", "epsHe0", "self_shield_dens", "zreion")
    want = []
    for x in pts:
        local = U.get_local_UVBG_from_global(redshift, glob, x, U.OFFSET, uvf)
        want.append([local["zreion"]] + [local[k] for k in keys])
    want = np.array(want)
    assert (want[:, 0] < redshift).sum() > 300 and (want[:, 0] >= redshift).sum() > 300
    broken = np.array([[np.nan, 0.1, 0.1], [0.1, np.inf, 0.1], [0.1, 0.1, -1e300], [0.25 * 2.0 ** 31 + U.OFFSET[0] + 1.0, 0.1, 0.1]])
    head = [float(len(pts) + len(broken)), float(Nside), box] + list(U.OFFSET) + [redshift] + [glob[k] for k in keys]
    fin, fout = str(tmp_path / "in.f64"), str(tmp_path / "out.f64")
    np.concatenate([head, table.ravel(), pts.ravel(), broken.ravel()]).astype(np.float64).tofile(fin)
    r = subprocess.run([exe, fin, fout], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    out = np.fromfile(fout, np.float64).reshape(len(pts) + len(broken), 10)
    assert np.array_equal(out[:len(pts)], want)
    assert np.isnan(out[len(pts):, 0]).all()
