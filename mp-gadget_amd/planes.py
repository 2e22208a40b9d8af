"""Host side of the lensing potential planes (write_plane, libgadget/plane.c:572-683): default cut points, output names, the FITS
primary image the reference writes through CFITSIO (savePotentialPlane, lenstools.c:322-393) and the info.txt line.  No GPU, no FITS
library: the file is written by hand as the FITS standard lays it out (2880-byte blocks of 80-character cards, big-endian data).  Card
formatting follows the standard; byte identity with CFITSIO's output is not claimed."""
import os

import numpy as np

CM_PER_MPC = 3.085678e24    # physconst.h
BLOCK = 2880


def default_cut_points(BoxSize, Thickness):
    """plane.c:581-591: Thickness <= 0 means BoxSize; CutPoints[i] = (i + 1/2) Thickness for i < (int64) (BoxSize / Thickness)"""
    th = float(Thickness) if Thickness > 0 else float(BoxSize)
    n = int(float(BoxSize) / th)
    return np.array([(.5 + i) * th for i in range(n)], np.float64)


def plane_output_name(snapnum, cut, normal):
    """plane_get_output_fname, plane.c:481-486, without the directory and CFITSIO's leading '!' (overwrite)"""
    return "snap%d_potentialPlane%d_normal%d.fits" % (snapnum, cut, normal)


def _card(key, value=None, comment=None):
    """one 80-character header card: fixed format, the value right-justified to column 30 (strings from column 11, at least 8
    characters between the quotes), ' / comment' behind it"""
    if value is None:
        s = "%-8s" % key
        if comment:
            s += " " + comment
        return s[:80].ljust(80)
    if isinstance(value, bool):
        v = "%20s" % ("T" if value else "F")
    elif isinstance(value, (int, np.integer)):
        v = "%20d" % int(value)
    elif isinstance(value, str):
        v = ("'%-8s'" % value.replace("'", "''")).ljust(20)
    else:
        t = "%.15G" % float(value)
        if "." not in t and "E" not in t and "N" not in t and "I" not in t:
            t += "."
        v = "%20s" % t
    s = "%-8s= %s" % (key, v)
    if comment:
        s += " / " + comment
    return s[:80].ljust(80)


def plane_header_cards(rows, cols, BoxSize, HubbleParam, Omega0, OmegaLambda, Omega_fld, w0_fld, wa_fld, redshift, comoving_distance,
                       num_particles, UnitLength_in_cm, double_out):
    """the cards of savePotentialPlane (lenstools.c:334-359) behind the mandatory ones.  NAXIS1 = cols, NAXIS2 = rows (naxes, :325).  FITS
    keywords are upper case, so the reference's "h" is the card H."""
    Ode0 = OmegaLambda if OmegaLambda > 0 else Omega_fld
    return [
        _card("SIMPLE", True, "file does conform to FITS standard"),
        _card("BITPIX", -64 if double_out else -32, "number of bits per data pixel"),
        _card("NAXIS", 2, "number of data axes"),
        _card("NAXIS1", int(cols), "length of data axis 1"),
        _card("NAXIS2", int(rows), "length of data axis 2"),
        _card("EXTEND", True, "FITS dataset may contain extensions"),
        _card(""),
        _card("H0", HubbleParam * 100, "Hubble constant in km/s*Mpc"),
        _card("H", HubbleParam, "Dimensionless Hubble constant"),
        _card("OMEGA_M", Omega0, "Dark Matter density"),
        _card("OMEGA_L", Ode0, "Dark Energy density"),
        _card("W0", w0_fld, "Dark Energy equation of state"),
        _card("WA", wa_fld, "Dark Energy running equation of state"),
        _card("Z", redshift, "Redshift of the lens plane"),
        _card("CHI", comoving_distance * UnitLength_in_cm / CM_PER_MPC, "Comoving distance in Mpc/h"),
        _card("SIDE", BoxSize * UnitLength_in_cm / CM_PER_MPC, "Side length in Mpc/h"),
        _card("NPART", int(num_particles), "Number of particles on the plane"),
        _card("UNIT", "rad2", "Pixel value unit"),
        _card("END"),
    ]


def save_potential_plane(data, filename, BoxSize, HubbleParam, Omega0, OmegaLambda, redshift, comoving_distance, num_particles, UnitLength_in_cm,
                         double_out=False, Omega_fld=0.0, w0_fld=-1.0, wa_fld=0.0):
    """savePotentialPlane (lenstools.c:322-393): data[rows][cols] doubles as a FITS primary image, BITPIX -64 (double_out) or -32.
    An existing file is overwritten, as the reference's '!' prefix asks of CFITSIO."""
    data = np.asarray(data, np.float64)
    if data.ndim != 2:
        raise ValueError("save_potential_plane: a 2-D image is needed")
    rows, cols = data.shape
    cards = plane_header_cards(rows, cols, BoxSize, HubbleParam, Omega0, OmegaLambda, Omega_fld, w0_fld, wa_fld, redshift, comoving_distance,
                               num_particles, UnitLength_in_cm, double_out)
    head = "".join(cards).encode("ascii")
    head += b" " * (-len(head) % BLOCK)
    body = np.ascontiguousarray(data, ">f8" if double_out else ">f4").tobytes()
    body += b"\0" * (-len(body) % BLOCK)
    with open(filename, "wb") as f:
        f.write(head)
        f.write(body)


def info_line(snapnum, comoving_distance, UnitLength_in_cm, redshift):
    """plane.c:676-679"""
    return "s=%d,d=%f Mpc/h,z=%f\n" % (snapnum, comoving_distance * UnitLength_in_cm / CM_PER_MPC, redshift)


def write_planes(OutputDir, snapnum, planes, npart, Normals, atime, comoving_distance, BoxSize, HubbleParam, Omega0, OmegaLambda, UnitLength_in_cm,
                 double_out=False, Omega_fld=0.0, w0_fld=-1.0, wa_fld=0.0):
    """The output half of write_plane (plane.c:633-682) for the result of a planes call: planes[ncuts][nnormals][R][R] (numpy or a
    torch tensor), npart[ncuts][nnormals].  One file per cut and normal, then the line appended to OutputDir/info.txt.  Returns the
    file names."""
    if hasattr(planes, "cpu"):
        planes = planes.cpu().numpy()
    planes, npart = np.asarray(planes), np.asarray(npart)
    redshift = 1. / atime - 1.
    names = []
    os.makedirs(OutputDir, exist_ok=True)
    for i in range(planes.shape[0]):
        for j, normal in enumerate(Normals):
            name = os.path.join(OutputDir, plane_output_name(snapnum, i, int(normal)))
            save_potential_plane(planes[i, j], name, BoxSize, HubbleParam, Omega0, OmegaLambda, redshift, comoving_distance, int(npart[i, j]),
                                 UnitLength_in_cm, double_out, Omega_fld, w0_fld, wa_fld)
            names.append(name)
    with open(os.path.join(OutputDir, "info.txt"), "a") as f:
        f.write(info_line(snapnum, comoving_distance, UnitLength_in_cm, redshift))
    return names
