"""The data side of the helium reionisation model (libgadget/cooling_qso_lightup.c): the history table and what the caller of
Engine.dev_heiii_reionization computes from it.  The engine reads no file; this module is load_heii_reion_hist (:137-244) and its helpers.

A history file: comment lines (first token starts with '#') anywhere; then the quasar spectral index, the instantaneous absorption threshold
energy in eV, and rows of three columns: redshift, HeIII fraction, long-mean-free-path heating in erg/s/cm^3.  Redshifts become scale factors,
so the table is increasing (:208)."""
import math

import numpy as np

E0_HeII = 54.4              # cooling_qso_lightup.c:45, eV
eVinergs = 1.60218e-12      # physconst.h:15
HUBBLE = 3.2407789e-18      # physconst.h:26, h/s
GRAVITY = 6.672e-8          # physconst.h:5


def Q_inst(Emax, alpha_q):
    """:113-121: instantaneous heat injection per helium atom in erg from the photons below Emax (eV)"""
    intflux = (math.pow(Emax, -alpha_q + 1.) - math.pow(E0_HeII, -alpha_q + 1.)) / (math.pow(Emax, -alpha_q) - math.pow(E0_HeII, -alpha_q))
    q = (alpha_q / (alpha_q - 1.0)) * intflux - E0_HeII
    return eVinergs * q


def _interp_linear(xa, ya, x):
    """gsl_interp_eval of gsl_interp_linear: the interval by bisection (xa[i] <= x < xa[i+1], the last interval closed), then
    y_lo + (x - x_lo) / (x_hi - x_lo) * (y_hi - y_lo)"""
    if not (xa[0] <= x <= xa[-1]):
        raise ValueError("interpolation point %r outside the table [%r, %r]" % (x, xa[0], xa[-1]))
    lo, hi = 0, len(xa) - 1
    while hi > lo + 1:
        i = (hi + lo) // 2
        if xa[i] > x:
            hi = i
        else:
            lo = i
    dx = xa[lo + 1] - xa[lo]
    return ya[lo] + (x - xa[lo]) / dx * (ya[lo + 1] - ya[lo])


class ReionHistory:
    """The table of a history file: a (increasing), XHeIII, LMFP; qso_inst_heating = Q_inst of its header; heIIIreion_start = 1 / a[0] - 1."""

    def __init__(self, spectral_index, threshold_energy, redshift, xheiii, lmfp):
        if len(redshift) <= 2:
            raise ValueError("HeII: Reionization history contains: %d entries, not enough." % len(redshift))         # :172-173
        self.spectral_index, self.threshold_energy = float(spectral_index), float(threshold_energy)
        self.a = [1. / (1 + float(z)) for z in redshift]                                                             # :208
        self.xheiii = [float(v) for v in xheiii]
        self.lmfp = [float(v) for v in lmfp]
        self.qso_inst_heating = Q_inst(self.threshold_energy, self.spectral_index)                                  # :222
        self.heIIIreion_start = 1 / self.a[0] - 1                                                                   # :233

    @classmethod
    def parse(cls, text):
        """:150-221 on the text of a file"""
        head, rows = [], []
        for line in text.splitlines():
            tok = line.split()
            if not tok or tok[0].startswith("#"):
                continue
            if len(head) < 2:
                head.append(float(tok[0]))
                continue
            if len(tok) < 3:
                raise ValueError("HeII: Line %s of reionization table was incomplete!" % line)                      # :211-217
            rows.append((float(tok[0]), float(tok[1]), float(tok[2])))
        if len(head) < 2:
            raise ValueError("HeII: the history has no spectral index and threshold energy")
        return cls(head[0], head[1], [r[0] for r in rows], [r[1] for r in rows], [r[2] for r in rows])

    @classmethod
    def load(cls, path):
        with open(path) as f:
            return cls.parse(f.read())

    def desired_fraction(self, atime):
        """XHeIII(atime), :530, :664; an error outside the table, where the reference's guards (:646-651) never ask"""
        return _interp_linear(self.a, self.xheiii, atime)

    def long_mfp_heating(self, redshift):
        """get_long_mean_free_path_heating, :257-277, in erg/s/cm^3: what mpg_set_cooling_params takes; 0 before the start and past the end"""
        if redshift > self.heIIIreion_start:
            return 0.0
        atime = 1 / (1 + redshift)
        if atime > self.a[-1]:
            return 0.0
        return _interp_linear(self.a, self.lmfp, atime)

    def during_helium_reionization(self, redshift):
        """:671-684"""
        if redshift > self.heIIIreion_start:
            return False
        if redshift < 1. / self.a[-1] - 1:
            return False
        return True

    def active_at(self, atime):
        """the guards of do_heiii_reionization, :646-651"""
        return not (atime < 1 / (1 + self.heIIIreion_start)) and not (atime > self.a[-1])


def non_overlapping_bubble_number(n_gas_tot, mean_bubble, atime, OmegaBaryon, HubbleParam):
    """:550-554: the ionisations expected from one bubble at mean density (int64 truncation of the product)"""
    a3inv = 1 / math.pow(atime, 3)
    rhobar = OmegaBaryon * (3 * HUBBLE * HubbleParam * HUBBLE * HubbleParam) / (8 * math.pi * GRAVITY) * a3inv
    totbubblegasmass = 4 * math.pi / 3. * math.pow(mean_bubble, 3) * rhobar
    return int(n_gas_tot * totbubblegasmass / OmegaBaryon)


def step(hist, atime, uu_in_cgs, n_gas_tot, TotNgroups, mean_bubble, OmegaBaryon, HubbleParam):
    """the members of mpg_heiii_step for one call, from a ReionHistory"""
    return dict(atime=atime, desired_ion_frac=hist.desired_fraction(atime), qso_inst_heating=hist.qso_inst_heating, uu_in_cgs=uu_in_cgs,
                n_gas_tot=int(n_gas_tot), non_overlapping_bubble_number=non_overlapping_bubble_number(n_gas_tot, mean_bubble, atime, OmegaBaryon, HubbleParam),
                TotNgroups=int(TotNgroups))
