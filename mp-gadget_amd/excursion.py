"""The data side of the excursion set's J21 in cooling and star formation (libgadget/cooling_rates.c:226-313, :399-430): the rate
coefficients per unit J21 as a function of the spectral slope alpha, and what the caller of Engine.set_excursion_set computes from them.
The engine reads no file; this module is load_J21coeffs and get_J21_coeffs.

A J21CoeffFile: comment lines (first token starts with '#') anywhere; rows of seven columns: alpha, Gamma_HI, Gamma_HeI, Gamma_HeII in 1/s
and Qdot_HI, Qdot_HeI, Qdot_HeII in eV/s, each for J21 = 1.  The table keeps log10 of the six (load_tree_value, :128-134: -9000 for a value
that is not positive), with HydrogenHeatAmp added to the fourth."""
import math

COLUMNS = ("gJH0", "gJHe0", "gJHep", "epsH0", "epsHe0", "epsHep")     # the order of the file's columns 1 .. 6


def _interp_linear(xa, ya, x):
    """gsl_interp_eval of gsl_interp_linear for xa[0] <= x <= xa[-1]: the interval by bisection (xa[i] <= x < xa[i+1], the last interval
    closed), then y_lo + (x - x_lo) / (x_hi - x_lo) * (y_hi - y_lo)"""
    lo, hi = 0, len(xa) - 1
    while hi > lo + 1:
        i = (hi + lo) // 2
        if xa[i] > x:
            hi = i
        else:
            lo = i
    dx = xa[lo + 1] - xa[lo]
    return ya[lo] + (x - xa[lo]) / dx * (ya[lo + 1] - ya[lo])


def _tree_value(tok):
    data = float(tok)
    return math.log10(data) if data > 0 else -9000.0


class J21Coeffs:
    """The table of a J21CoeffFile: alpha (increasing) and log10 of the six columns by name."""

    def __init__(self, alpha, columns, HydrogenHeatAmp=0.0):
        if len(alpha) <= 2:
            raise ValueError("Photon background contains: %d entries, not enough." % len(alpha))                     # :260-261
        self.alpha = [float(a) for a in alpha]
        self.log = {k: [_tree_value(v) for v in columns[k]] for k in COLUMNS}
        self.log["epsH0"] = [v + HydrogenHeatAmp for v in self.log["epsH0"]]                                         # :293

    @classmethod
    def parse(cls, text, HydrogenHeatAmp=0.0):
        """:242-297 on the text of a file"""
        rows = []
        for line in text.splitlines():
            tok = line.split()
            if not tok or tok[0].startswith("#"):
                continue
            if len(tok) < 7:
                raise ValueError("J21 coefficients: line %r has fewer than seven columns" % line)
            rows.append(tok[:7])
        return cls([r[0] for r in rows], {k: [r[1 + i] for r in rows] for i, k in enumerate(COLUMNS)}, HydrogenHeatAmp)

    @classmethod
    def load(cls, path, HydrogenHeatAmp=0.0):
        with open(path) as f:
            return cls.parse(f.read(), HydrogenHeatAmp)

    def photorate_coeff(self, alpha, name, PhotoIonizeFactor=1.0):
        """get_photorate_coeff, :402-415: 0 at or above the last alpha, the first entry below the first, gsl's linear interpolation of the
        log between; pow(10, .) * PhotoIonizeFactor"""
        if alpha >= self.alpha[-1]:
            return 0.0
        if alpha < self.alpha[0]:
            photo_rate = self.log[name][0]
        else:
            photo_rate = _interp_linear(self.alpha, self.log[name], alpha)
        return math.pow(10, photo_rate) * PhotoIonizeFactor

    def coeffs(self, alpha, PhotoIonizeFactor=1.0):
        """get_J21_coeffs, :419-430: the six members by name, the eps in eV/s"""
        return {k: self.photorate_coeff(alpha, k, PhotoIonizeFactor) for k in COLUMNS}


def params(table, AlphaUV, ExcursionSetReionOn=1, ExcursionSetZStop=0.0, PhotoIonizeFactor=1.0):
    """the members of mpg_excursion_set_params from a J21Coeffs table"""
    return dict(ExcursionSetReionOn=int(ExcursionSetReionOn), ExcursionSetZStop=float(ExcursionSetZStop), AlphaUV=float(AlphaUV),
                **table.coeffs(AlphaUV, PhotoIonizeFactor))
