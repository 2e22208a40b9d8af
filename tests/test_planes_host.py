"""The restatement of the lensing potential planes (planes_restated.py) against closed forms nobody computed with the code under test,
and the host-only Python layer (mp-gadget_amd/planes.py).  No GPU."""
import os

import numpy as np
import pytest

import planes_restated as R_

CHI, ATIME, HUBBLE, OMEGA = 2.5e5, 0.5, 0.7, 0.27


@pytest.mark.parametrize("R", [64, 96, 250])
@pytest.mark.parametrize("m", [1, 3, 7])
def test_solve_closed_form(R, m):
    """a projected density 1 + A cos(2 pi m i / R) along one index is an eigenfunction of the solve (lenstools.c:184-211):
    psi = -2 (b^2 / chi^2) / (4 pi^2 (m/R)^2) exp(-(2 pi)^2 (m/R)^2 / 2) A cos(2 pi m i / R), times the two normalisations, constant along
    the other index; a uniform density gives zero"""
    A, box, th = 0.3, 1000.0, 200.0
    b = box / R
    i = np.arange(R)
    wave = A * np.cos(2 * np.pi * m * i / R)
    l2 = (m / R) ** 2
    norm = R_.normalisations(box, th, CHI, ATIME, HUBBLE, OMEGA)
    want1 = -2 * (b * b / CHI ** 2) / (4 * np.pi ** 2 * l2) * np.exp(-0.5 * (2 * np.pi) ** 2 * l2) * wave * norm
    tol = 1e-13 * np.abs(want1).max()
    for axis in (0, 1):
        dens = 1 + (wave[:, None] if axis == 0 else wave[None, :]) * np.ones((R, R))
        got = R_.lensing_potential(dens, b, b, CHI) * norm
        want = want1[:, None] * np.ones((R, R)) if axis == 0 else want1[None, :] * np.ones((R, R))
        d = np.abs(got - want).max()
        print("R %d m %d axis %d: max diff %.3g of max|psi|" % (R, m, axis, d / np.abs(want1).max()))
        assert d <= tol
    # uniform: only what the transform's rounding leaves of the mean, held to the same 1e-13 of the response to a unit wave at m = 1
    unit = 2 * (b * b / CHI ** 2) / (4 * np.pi ** 2 * (1 / R) ** 2)
    assert np.abs(R_.lensing_potential(np.ones((R, R)), b, b, CHI)).max() <= 1e-13 * unit


def _lattice(n, box):
    """n^3 points, spacing box / n, shifted by half a spacing"""
    g = (np.arange(n) + 0.5) * (box / n)
    return np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)


@pytest.mark.parametrize("normal", [0, 1, 2])
def test_lattice_counts(normal):
    box, n, R = 64.0, 32, 8          # spacing 2, pixel 8: 4 x 4 points per pixel and layer, none on an edge
    pos = _lattice(n, box)
    full = R_.plane_counts(pos, box, R, normal, box / 2, box)         # thickness >= Box: every layer
    assert (full == 4 * 4 * n).all() and full.sum() == n ** 3
    thin = R_.plane_counts(pos, box, R, normal, 20.0, 8.0)            # [16, 24): the layers at 17, 19, 21, 23
    assert (thin == 4 * 4 * 4).all()
    across = R_.plane_counts(pos, box, R, normal, 1.0, 6.0)           # [-2, 4) = [62, 64) + [0, 4): the layers at 63, 1, 3
    assert (across == 4 * 4 * 3).all()
    out = R_.potential_planes(pos, box, R, [normal], ATIME, CHI, HUBBLE, OMEGA, Thickness=8.0, CutPoints=[20.0, 1.0])
    # [16, 24) and [-3, 5) = [61, 64) + [0, 5): the layers at 61, 63, 1, 3
    assert out["npart"].ravel().tolist() == [n * n * 4, n * n * 4] and out["n_active"] == n ** 3
    # uniform counts: no potential beyond the transform's rounding (1e-13 of the response to a unit density wave at m = 1)
    unit = 2 * ((box / R) ** 2 / CHI ** 2) / (4 * np.pi ** 2 * (1 / R) ** 2) * R_.normalisations(box, 8.0, CHI, ATIME, HUBBLE, OMEGA)
    assert np.abs(out["planes"]).max() <= 1e-13 * unit * (box / 8.0)      # (the density contrast of a thin slab is Box / thickness)
    # default cut points (plane.c:587-591) for Thickness = Box / 4: four slabs that tile the box
    out = R_.potential_planes(pos, box, R, [normal], ATIME, CHI, HUBBLE, OMEGA, Thickness=box / 4)
    assert out["npart"].ravel().tolist() == [n ** 3 // 4] * 4


def test_wrap_rule_at_zero_and_box():
    """lenstools.c:108-109: `while(p > Box) p -= Box; while(p <= 0) p += Box`.  A coordinate of exactly 0 is <= 0 and becomes Box; one of
    exactly Box is not > Box and stays Box.  find_bin (lenstools.c:74-76) then takes rel = Box - bins[0] = Box - 0, which is >= L and is
    brought to 0 by its own loop: pixel 0 in an image direction.  Along the normal, for the slab [cut - t/2, cut + t/2) with cut = t/2,
    rel = Box - 0 -> 0 < t: inside; for cut = Box - t/2, bins[0] = Box - t and rel = t, which is not < width = t: OUTSIDE (the slab's upper
    end is open); and for the slab [t/4, 5t/4) that starts above 0, rel = Box - t/4 >= width: outside.  Both particles behave alike."""
    box, R, t = 100.0, 10, 20.0
    pos = np.array([[0.0, 35.0, 35.0], [box, 35.0, 35.0], [35.0, 0.0, box]])
    # image direction: x = 0 and x = Box -> row 0 (normal 2: rows are x)
    pix = R_.plane_pixels(pos, box, R, 2, box / 2, box)
    assert pix.tolist() == [0 * R + 3, 0 * R + 3, 3 * R + 0]
    # normal 1 on the third particle (y = 0 -> Box -> rel 0 against the slab that starts at 0): counted; columns are z = Box -> 0
    assert R_.plane_pixels(pos[2:], box, R, 1, t / 2, t).tolist() == [3 * R + 0]
    # along the normal 0
    assert R_.plane_pixels(pos[:2], box, R, 0, t / 2, t).tolist() == [3 * R + 3] * 2           # [0, t)
    assert R_.plane_pixels(pos[:2], box, R, 0, box - t / 2, t).tolist() == [-1, -1]            # [Box - t, Box): the end is open
    assert R_.plane_pixels(pos[:2], box, R, 0, t / 4 + t / 2, t).tolist() == [-1, -1]          # [t/4, 5t/4)
    assert R_.plane_pixels(pos[:2], box, R, 0, 0.0, t).tolist() == [3 * R + 3] * 2             # [-t/2, t/2): rel = Box + t/2 -> t/2


def test_activity_rule():
    fl = np.array([0, 1, 2, 3, 0, 0], np.uint8)
    ty = np.array([1, 1, 1, 1, 2, 0], np.uint8)
    assert R_.particle_is_active(fl, ty, False).tolist() == [True, False, False, False, True, True]
    assert R_.particle_is_active(fl, ty, True).tolist() == [True, False, False, False, False, True]


@pytest.mark.parametrize("center,thickness", [(30.0, 17.0), (2.0, 9.0), (97.5, 11.0), (50.0, 100.0), (50.0, 130.0)])
def test_overlap_weights_sum_to_thickness(center, thickness):
    """plane.c:369-387: over a column of cells the overlaps add up to the slab's thickness (inside the box and across the boundary);
    thickness >= Box gives every cell its own size"""
    L, n = 100.0, 16
    cs = L / n
    ov = np.array([R_.slab_overlap(k * cs, cs, center, thickness, L) for k in range(n)])
    if thickness >= L:
        assert (ov == cs).all()
    else:
        assert abs(ov.sum() - thickness) <= 1e-12 * L and (ov >= 0).all() and (ov <= cs).all()


def test_bilinear_resampling():
    rng = np.random.default_rng(5)
    src = rng.standard_normal((12, 12))
    assert np.array_equal(R_.bilinear_add(np.zeros((12, 12)), src), src)                   # src_n == dst_n: the identity
    for dn in (5, 12, 31):
        got = R_.bilinear_add(np.full((dn, dn), 1.5), np.full((12, 12), 2.25))
        assert np.abs(got - 3.75).max() <= 1e-15 * 4                                       # a constant stays that constant
    # a plane wave at twice the sampling keeps its mean
    up = R_.bilinear_add(np.zeros((24, 24)), src)
    assert abs(up.mean() - src.mean()) <= 1e-14


# ---- mp-gadget_amd/planes.py ---------------------------------------------------------------------------------------------------------------
def _read_fits(path):
    """a minimal reader of a FITS primary image: (cards as (key, value text, comment), the data array)"""
    raw = open(path, "rb").read()
    assert len(raw) % 2880 == 0
    cards, pos, end = [], 0, False
    while not end:
        block = raw[pos:pos + 2880].decode("ascii")
        pos += 2880
        for k in range(36):
            c = block[80 * k:80 * k + 80]
            key = c[:8].rstrip()
            if key == "END":
                end = True
                assert c[8:].strip() == ""
                break
            if c[8:10] == "= ":
                body = c[10:]
                if body.lstrip().startswith("'"):
                    q = body.index("'")
                    e = body.index("'", q + 1)
                    val, rest = body[q:e + 1], body[e + 1:]
                else:
                    val, _, rest = body.partition("/")
                    rest = "/" + rest if _ else ""
                    assert len(val.rstrip()) <= 20 and val[:20].rstrip() == val.rstrip()    # fixed format: ends in column 30
                cards.append((key, val.strip(), rest.partition("/")[2].strip()))
            else:
                cards.append((key, None, c[8:].strip()))
    assert pos % 2880 == 0
    kv = {k: v for k, v, _ in cards}
    bitpix, n1, n2 = int(kv["BITPIX"]), int(kv["NAXIS1"]), int(kv["NAXIS2"])
    nbytes = abs(bitpix) // 8 * n1 * n2
    assert len(raw) - pos == -(-nbytes // 2880) * 2880 and raw[pos + nbytes:] == b"\0" * (len(raw) - pos - nbytes)
    data = np.frombuffer(raw[pos:pos + nbytes], ">f8" if bitpix == -64 else ">f4").reshape(n2, n1)
    return cards, data


@pytest.mark.parametrize("double_out", [False, True])
def test_save_potential_plane(pkg, tmp_path, double_out):
    PL = pkg.planes
    rng = np.random.default_rng(11)
    rows, cols = 37, 52          # (not square: NAXIS1 is the column count)
    data = rng.standard_normal((rows, cols)) * 1e-9
    box, ulcm, chi, h = 250000.0, 3.085678e21, 1.2345e6, 0.6774
    name = str(tmp_path / "p.fits")
    PL.save_potential_plane(data, name, box, h, 0.3089, 0.6911, 0.75, chi, 123456789012, ulcm, double_out=double_out, w0_fld=-0.9, wa_fld=0.1)
    cards, got = _read_fits(name)
    assert [c[0] for c in cards[:5]] == ["SIMPLE", "BITPIX", "NAXIS", "NAXIS1", "NAXIS2"]
    kv = {k: (v, c) for k, v, c in cards}
    assert kv["SIMPLE"][0] == "T" and int(kv["BITPIX"][0]) == (-64 if double_out else -32) and int(kv["NAXIS"][0]) == 2
    assert int(kv["NAXIS1"][0]) == cols and int(kv["NAXIS2"][0]) == rows
    want = [("H0", h * 100, "Hubble constant in km/s*Mpc"), ("H", h, "Dimensionless Hubble constant"), ("OMEGA_M", 0.3089, "Dark Matter density"),
            ("OMEGA_L", 0.6911, "Dark Energy density"), ("W0", -0.9, "Dark Energy equation of state"),
            ("WA", 0.1, "Dark Energy running equation of state"), ("Z", 0.75, "Redshift of the lens plane"),
            ("CHI", chi * ulcm / 3.085678e24, "Comoving distance in Mpc/h"), ("SIDE", box * ulcm / 3.085678e24, "Side length in Mpc/h")]
    for key, val, comment in want:
        assert key in kv, key
        assert abs(float(kv[key][0]) - val) <= 1e-14 * abs(val) and kv[key][1] == comment, key
    assert int(kv["NPART"][0]) == 123456789012 and kv["NPART"][1] == "Number of particles on the plane"
    assert kv["UNIT"] == ("'rad2    '", "Pixel value unit")
    assert all(k == k.upper() for k, _, _ in cards)
    if double_out:
        assert np.array_equal(got, data)
    else:
        assert np.array_equal(got, data.astype(np.float32))
    # overwriting (the reference's '!' prefix)
    PL.save_potential_plane(data[:5, :7], name, box, h, 0.3089, 0.0, 0.75, chi, 1, ulcm, double_out=double_out, Omega_fld=0.65)
    cards, got = _read_fits(name)
    assert got.shape == (5, 7) and float({k: v for k, v, _ in cards}["OMEGA_L"]) == 0.65     # lenstools.c:342


def test_names_cut_points_and_info(pkg, tmp_path):
    PL = pkg.planes
    assert PL.plane_output_name(12, 3, 1) == "snap12_potentialPlane3_normal1.fits"
    assert PL.default_cut_points(100.0, 30.0).tolist() == [15.0, 45.0, 75.0]
    assert PL.default_cut_points(100.0, 0.0).tolist() == [50.0] and PL.default_cut_points(100.0, 250.0).tolist() == []
    assert PL.default_cut_points(100.0, 25.0).tolist() == R_.resolve(100.0, 25.0, None)[1]
    planes = np.arange(2 * 2 * 4 * 4, dtype=np.float64).reshape(2, 2, 4, 4)
    npart = np.array([[5, 6], [7, 8]])
    out = str(tmp_path / "o")
    for snap in (3, 4):
        names = PL.write_planes(out, snap, planes, npart, [2, 0], 0.5, 1.5e6, 250000.0, 0.7, 0.3, 0.7, 3.085678e21, double_out=True)
    assert [os.path.basename(x) for x in names] == ["snap4_potentialPlane0_normal2.fits", "snap4_potentialPlane0_normal0.fits",
                                                    "snap4_potentialPlane1_normal2.fits", "snap4_potentialPlane1_normal0.fits"]
    cards, got = _read_fits(names[3])
    assert np.array_equal(got, planes[1, 1]) and int({k: v for k, v, _ in cards}["NPART"]) == 8
    assert open(os.path.join(out, "info.txt")).read() == "s=3,d=1500.000000 Mpc/h,z=1.000000\ns=4,d=1500.000000 Mpc/h,z=1.000000\n"
