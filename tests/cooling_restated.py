"""The radiative cooling of the reference restated in plain Python, line by line (file:line of the reference in every function):
cooling.c (DoCooling, GetCoolingTime, GetNeutralFraction, get_lambdanet), cooling_rates.c (the rate network, its 13 tables, the UV
background from a TREECOOL table, self-shielding, the helium reionisation factor, inverse Compton), cooling_uvfluc.c
(TableMetalCoolingRate) with utils/interp.c (interp_eval), and cooling_direct of sfr_eff.c.  Scalar code on purpose: the result of
DoCooling is a function of discrete decisions (sign tests, |ne1 - ne0| < 1e-6), and every one of them is taken here exactly where the
reference takes it.  Test infrastructure: the GPU tests compare csrc/cooling.hip with it, tests/test_cooling_restated.py pins it to the
reference's own known answers.

`perturb` multiplies every table lookup (and every direct evaluation that stands for one) by 1 + perturb: the stability condition of the
tests repeats a run with +-2e-15 and asks that no decision changes."""
import math

import numpy as np

# physconst.h
GRAVITY = 6.672e-8
BOLTZMANN = 1.38066e-16
BOLEVK = 8.61734e-5
eVinergs = 1.60218e-12
PROTONMASS = 1.6726e-24
ELECTRONMASS = 9.10953e-28
THOMPSON = 6.65245e-25
RAD_CONST = 7.565e-15
LIGHTCGS = 2.99792458e10
HUBBLE = 3.2407789e-18
GAMMA = 5.0 / 3.0
GAMMA_MINUS1 = GAMMA - 1
HYDROGEN_MASSFRAC = 0.76

Cen92, Verner96, Badnell06 = 0, 1, 2          # enum RecombType, cooling_rates.h:10-14
KWH92, Enzo2Nyx, Sherwood = 0, 1, 2           # enum CoolingType, cooling_rates.h:16-20

NRECOMBTAB = 1000                             # cooling_rates.c:108
RECOMBTMAX = math.log(1e9)                    # cooling_rates.c:109
RECOMBTMIN = 0                                # cooling_rates.c:110
MAXITER = 1000                                # cooling.c:32, cooling_rates.c:768
ITERCONV = 1e-6                               # cooling_rates.c:771
BRACKET_MAXITER = 8192                        # the engine's cap on the two bracketing loops the reference leaves unbounded

sqrt, exp, log, log10, fabs, floor = math.sqrt, math.exp, math.log, math.log10, math.fabs, math.floor


def pow_(x, y):
    """C's pow for the arguments met here (math.pow raises where C returns inf or nan)"""
    try:
        return math.pow(x, y)
    except (OverflowError, ValueError):
        return float(np.power(np.float64(x), np.float64(y)))


def exp_(x):
    try:
        return math.exp(x)
    except OverflowError:
        return math.inf


class NotConverged(Exception):
    """the reference's endrun in scipy_optimize_fixed_point / DoCooling; the engine's error counter"""


# ---- the UV background from a TREECOOL table ------------------------------------------------------------------------------------------------
class TreeCool:
    """load_treecool, cooling_rates.c:142-224: columns log10(1+z), Gamma_HI, Gamma_HeI, Gamma_HeII, Qdot_HI, Qdot_HeI, Qdot_HeII; the six
    rate columns are kept as log10, a rate that is not positive as -9000 (load_tree_value :127-134)"""

    def __init__(self, columns, HydrogenHeatAmp=0.0):
        c = np.asarray(columns, np.float64)
        assert c.ndim == 2 and c.shape[0] == 7 and c.shape[1] > 2        # :171
        self.log1z = [float(x) for x in c[0]]
        tab = [[(log10(float(x)) if x > 0 else -9000.0) for x in c[k]] for k in range(1, 7)]
        tab[3] = [x + HydrogenHeatAmp for x in tab[3]]                  # :204 (HydrogenHeatAmp is log10 of the parameter, :1091)
        self.Gamma_HI, self.Gamma_HeI, self.Gamma_HeII, self.Eps_HI, self.Eps_HeI, self.Eps_HeII = tab


def gsl_interp_linear(xa, ya, x):
    """gsl_interp_eval of gsl_interp_linear: the interval [xa[i], xa[i+1]) that holds x (the last one for x == xa[-1])"""
    lo, hi = 0, len(xa) - 1
    while hi > lo + 1:                         # gsl_interp_bsearch
        i = (hi + lo) // 2
        if xa[i] > x:
            hi = i
        else:
            lo = i
    x_lo, x_hi, y_lo, y_hi = xa[lo], xa[lo + 1], ya[lo], ya[lo + 1]
    dx = x_hi - x_lo
    return y_lo + (x - x_lo) / dx * (y_hi - y_lo)


GrayOpac_ydata = [2.59e-18, 2.37e-18, 2.27e-18, 2.15e-18, 2.02e-18, 1.94e-18]   # cooling_rates.c:75
GrayOpac_zz = [0.0, 1.0, 2.0, 3.0, 4.0, 5.0]                                    # cooling_rates.c:76


def default_params(**kw):
    """struct cooling_params (cooling_rates.h:23-58) as get_test_coolpar fills it (test_cooling_rates.c:34-49), struct cooling_units
    (cooling.h:32-44) in the unit system of test_cooling.c:179-197, and the three members of sfr_params that cooling_direct reads"""
    HubbleParam = 0.7
    UnitDensity_in_cgs, UnitTime_in_s, UnitMass_in_g, UnitLength_in_cm = 6.76991e-22, 3.08568e+16, 1.989e+43, 3.08568e+21
    UnitEnergy_in_cgs = UnitMass_in_g * pow_(UnitLength_in_cm, 2) / pow_(UnitTime_in_s, 2)
    fBar, OmegaCDM = 0.17, 0.3
    rcb = fBar * OmegaCDM * 3.0 * pow_(HubbleParam * HUBBLE, 2.0) / (8.0 * math.pi * GRAVITY)   # cooling_rates.c:1108
    uu = UnitEnergy_in_cgs / UnitMass_in_g
    p = dict(recomb=Verner96, cooling=Sherwood, SelfShieldingOn=1, PhotoIonizationOn=1, fBar=fBar, PhotoIonizeFactor=1.0,
             CMBTemperature=2.7255, MinGasTemp=100.0, UVRedshiftThreshold=-1.0, HydrogenHeatAmp=0.0, HeliumHeatOn=0, HeliumHeatThresh=10.0,
             HeliumHeatAmp=1.0, HeliumHeatExp=0.0, rho_crit_baryon=rcb,
             CoolingOn=1, density_in_phys_cgs=UnitDensity_in_cgs * HubbleParam * HubbleParam, uu_in_cgs=uu, tt_in_s=UnitTime_in_s / HubbleParam,
             units_rho_crit_baryon=3 * pow_(HubbleParam * HUBBLE, 2) * fBar * OmegaCDM / (8 * math.pi * GRAVITY),   # test_cooling.c:197
             sfr_MinGasTemp=5.0, temp_to_u=(1.0 / GAMMA_MINUS1) * (BOLTZMANN / PROTONMASS) / uu,   # sfr_eff.c:899
             HIReionTemp=0.0, test_network_maxiter=0)
    p.update(kw)
    return p


def zero_uvbg():
    return dict(J_UV=0.0, gJH0=0.0, gJHep=0.0, gJHe0=0.0, epsH0=0.0, epsHep=0.0, epsHe0=0.0, self_shield_dens=0.0, zreion=0.0)


class MetalTable:
    """InitMetalCooling, cooling_uvfluc.c:265-305, with interp_init / interp_init_dim (utils/interp.c:9-54): only the ends and the lengths of
    the three bin vectors count"""

    def __init__(self, zbins, nhbins, tbins, rate):
        rate = np.ascontiguousarray(rate, np.float64)
        self.dims = [len(zbins), len(nhbins), len(tbins)]
        assert list(rate.shape) == self.dims
        self.data = [float(x) for x in rate.ravel()]
        self.strides = [self.dims[1] * self.dims[2], self.dims[2], 1]         # :31-36
        self.Min = [float(zbins[0]), float(nhbins[0]), float(tbins[0])]
        self.Max = [float(zbins[-1]), float(nhbins[-1]), float(tbins[-1])]
        self.Step = [(self.Max[d] - self.Min[d]) / (self.dims[d] - 1) for d in range(3)]   # :53

    def interp_eval(self, x):
        """utils/interp.c:72-131.  One departure, shared with the engine: a coordinate inside [Min, Max] whose rounded position reaches the
        last point gets weight 0 there (the reference would read one element past the table with a weight of a few ulp)."""
        xi, f = [0, 0, 0], [0.0, 0.0, 0.0]
        for d in range(3):
            xd = (x[d] - self.Min[d]) / self.Step[d]
            if x[d] < self.Min[d]:
                xi[d], f[d] = 0, 0.0
            elif x[d] > self.Max[d]:
                xi[d], f[d] = self.dims[d] - 1, 0.0
            else:
                xi[d] = int(floor(xd))
                f[d] = xd - xi[d]
                if xi[d] >= self.dims[d] - 1:
                    xi[d], f[d] = self.dims[d] - 1, 0.0
        ret = 0.0
        l0 = sum(self.strides[d] * xi[d] for d in range(3))                   # linearindex, :57-64
        for i in range(8):
            filt, l, skip = 1.0, l0, False
            for d in range(3):
                foffset = 1 if (i & (1 << d)) else 0
                if f[d] == 0 and foffset == 1:
                    skip = True
                    break
                filt *= f[d] if foffset else (1 - f[d])
                l += foffset * self.strides[d]
            if not skip:
                ret += self.data[l] * filt
        return ret


class Cooling:
    """the module state of cooling.c / cooling_rates.c: CoolingParams, coolunits, the TREECOOL table, the 13 rate tables, the metal table"""

    def __init__(self, par, treecool=None, metal=None, perturb=0.0):
        self.p = dict(par)
        self.tc = treecool
        self.metal = metal
        self.perturb = perturb
        self.evals = 0            # ne_internal evaluations since the caller last reset it
        self.max_fp = 0           # most iterations one fixed-point solve took since the caller last reset it
        self.net_maxiter = par.get("test_network_maxiter", 0) or MAXITER
        self.recomb, self.cooling = par["recomb"], par["cooling"]
        self.init_tables()

    # ---- recombination and collisional ionisation rates, cooling_rates.c:452-641
    @staticmethod
    def _Verner96Fit(temp, aa, bb, temp0, temp1):                              # :472-478
        sqrttt0 = sqrt(temp / temp0)
        sqrttt1 = sqrt(temp / temp1)
        return aa / (sqrttt0 * pow_(1 + sqrttt0, 1 - bb) * pow_(1 + sqrttt1, 1 + bb))

    def recomb_alphaHp(self, temp):                                            # :481-498
        if self.recomb == Cen92:
            return 8.4e-11 / sqrt(temp) / pow_(temp / 1000, 0.2) / (1 + pow_(temp / 1e6, 0.7))
        if self.recomb == Verner96:
            return self._Verner96Fit(temp, 7.982e-11, 0.748, 3.148, 7.036e+05)
        return self._Verner96Fit(temp, 8.318e-11, 0.7472, 2.965, 7.001e5)

    def _Verner96alphaHep(self, temp):                                         # :501-518
        lowTfit = self._Verner96Fit(temp, 3.294e-11, 0.6910, 1.554e+01, 3.676e+07)
        highTfit = self._Verner96Fit(temp, 9.356e-10, 0.7892, 4.266e-02, 4.677e+06)
        swtmp, deltat = 7e5, 1e5
        upper, lower = swtmp + deltat, swtmp - deltat
        interpfit = (lowTfit * (upper - temp) + highTfit * (temp - lower)) / (2 * deltat)
        return (temp < lower) * lowTfit + (temp > upper) * highTfit + (upper > temp) * (temp > lower) * interpfit

    def recomb_alphaHep(self, temp):                                           # :521-535
        if self.recomb == Cen92:
            return 1.5e-10 / pow_(temp, 0.6353)
        if self.recomb == Verner96:
            return self._Verner96alphaHep(temp)
        return self._Verner96Fit(temp, 1.818E-10, 0.7492, 10.17, 2.786e6)

    def recomb_alphad(self, temp):                                             # :540-558
        if self.recomb == Cen92:
            return 1.9e-3 / pow_(temp, 1.5) * exp(-4.7e5 / temp) * (1 + 0.3 * exp(-9.4e4 / temp))
        return 1.23e-3 / pow_(temp, 1.5) * exp(-4.72e5 / temp) * (1 + 0.3 * exp(-9.4e4 / temp))

    def recomb_alphaHepd(self, temp):                                          # :561-565
        return self.recomb_alphad(temp) + self.recomb_alphaHep(temp)

    def recomb_alphaHepp(self, temp):                                          # :568-582
        if self.recomb == Cen92:
            return 4 * self.recomb_alphaHp(temp)
        if self.recomb == Verner96:
            return self._Verner96Fit(temp, 1.891e-10, 0.7524, 9.370, 2.774e6)
        return self._Verner96Fit(temp, 5.235E-11, 0.6988 + 0.0829 * exp(-1.682e5 / temp), 7.301, 4.475e6)

    @staticmethod
    def _Voronov96Fit(temp, dE, PP, AA, XX, KK):                               # :585-590
        UU = dE / (BOLEVK * temp)
        return AA * (1 + PP * sqrt(UU)) / (XX + UU) * pow_(UU, KK) * exp(-UU)

    def recomb_GammaeH0(self, temp):                                           # :593-607
        if self.recomb == Cen92:
            return 5.85e-11 * sqrt(temp) * exp(-157809.1 / temp) / (1 + sqrt(temp / 1e5))
        return self._Voronov96Fit(temp, 13.6, 0, 0.291e-07, 0.232, 0.39)

    def recomb_GammaeHe0(self, temp):                                          # :610-624
        if self.recomb == Cen92:
            return 2.38e-11 * sqrt(temp) * exp(-285335.4 / temp) / (1 + sqrt(temp / 1e5))
        return self._Voronov96Fit(temp, 24.6, 0, 0.175e-07, 0.180, 0.35)

    def recomb_GammaeHep(self, temp):                                          # :627-641
        if self.recomb == Cen92:
            return 5.68e-12 * sqrt(temp) * exp(-631515.0 / temp) / (1 + sqrt(temp / 1e5))
        return self._Voronov96Fit(temp, 54.4, 1, 0.205e-08, 0.265, 0.25)

    # ---- cooling rates, cooling_rates.c:879-1049
    def _t5(self, temp):                                                       # :880-892
        t0 = 1e5 if self.cooling == KWH92 else 5e7
        return 1 + sqrt(temp / t0)

    def cool_CollisionalExciteH0(self, temp):                                  # :895-899
        return 7.5e-19 * exp(-118348.0 / temp) / self._t5(temp)

    def cool_CollisionalExciteHeP(self, temp):                                 # :902-906
        return 5.54e-17 * pow_(temp, -0.397) * exp(-473638. / temp) / self._t5(temp)

    def cool_CollisionalExciteHe0(self, temp):                                 # :909-913
        return 9.1e-27 * pow_(temp, -0.1687) * exp(-473638 / temp) / self._t5(temp)

    def cool_CollisionalIonizeH0(self, temp):                                  # :916-921
        return 13.5984 * eVinergs * self.recomb_GammaeH0(temp)

    def cool_CollisionalIonizeHe0(self, temp):                                 # :924-928
        return 24.5874 * eVinergs * self.recomb_GammaeHe0(temp)

    def cool_CollisionalIonizeHeP(self, temp):                                 # :931-935
        return 54.417760 * eVinergs * self.recomb_GammaeHep(temp)

    def cool_CollisionalH0(self, temp):                                        # :938-959
        if self.cooling == Enzo2Nyx:
            y = log(temp)
            Ryd = 2.1798741e-11
            tot = -0.75 / BOLTZMANN * Ryd / temp
            coeffslowT = [213.7913, 113.9492, 25.06062, 2.762755, 0.1515352, 3.290382e-3]
            coeffshighT = [271.25446, 98.019455, 14.00728, 0.9780842, 3.356289e-2, 4.553323e-4]
            for j in range(6):
                tot += ((temp < 1e5) * coeffslowT[j] + (temp >= 1e5) * coeffshighT[j]) * pow_(-y, j)
            return 1e-20 * exp_(tot)
        return self.cool_CollisionalExciteH0(temp) + self.cool_CollisionalIonizeH0(temp)

    def cool_CollisionalHe0(self, temp):                                       # :962-966
        return self.cool_CollisionalExciteHe0(temp) + self.cool_CollisionalIonizeHe0(temp)

    def cool_CollisionalHeP(self, temp):                                       # :969-973
        return self.cool_CollisionalExciteHeP(temp) + self.cool_CollisionalIonizeHeP(temp)

    def cool_RecombHp(self, temp):                                             # :976-984
        if self.cooling == Enzo2Nyx:
            return 2.851e-27 * sqrt(temp) * (5.914 - 0.5 * log(temp) + 0.01184 * pow_(temp, 1. / 3))
        return 0.75 * BOLTZMANN * temp * self.recomb_alphaHp(temp)

    def cool_RecombDielect(self, temp):                                        # :987-992
        return 6.526e-11 * self.recomb_alphad(temp)

    def cool_RecombHeP(self, temp):                                            # :995-999
        return 0.75 * BOLTZMANN * temp * self.recomb_alphaHep(temp) + self.cool_RecombDielect(temp)

    def cool_RecombHePP(self, temp):                                           # :1002-1010
        if self.cooling == Enzo2Nyx:
            return 1.140e-26 * sqrt(temp) * (6.607 - 0.5 * log(temp) + 7.459e-3 * pow_(temp, 1. / 3))
        return 0.75 * BOLTZMANN * temp * self.recomb_alphaHepp(temp)

    def cool_FreeFree(self, temp, zz):                                         # :1015-1033
        if self.cooling == Enzo2Nyx:
            lt = 2 * log10(temp / zz)
            if lt <= log10(3.2e5):
                gff = (0.79464 + 0.1243 * lt)
            else:
                gff = (2.13164 - 0.1240 * lt)
        else:
            gff = 1.1 + 0.34 * exp(-pow_(5.5 - log10(temp), 2) / 3.)
        return 1.426e-27 * sqrt(temp) * pow_(zz, 2) * gff

    def cool_FreeFree1(self, temp):                                            # :1035-1039
        return self.cool_FreeFree(temp, 1)

    def cool_InverseCompton(self, temp, redshift):                             # :1044-1049
        tcmb_red = self.p["CMBTemperature"] * (1 + redshift)
        return 4 * THOMPSON * RAD_CONST / (ELECTRONMASS * LIGHTCGS) * pow_(tcmb_red, 4) * BOLTZMANN * (temp - tcmb_red)

    def cool_he_reion_factor(self, nHcgs, helium, redshift):                   # :1058-1068
        if not self.p["HeliumHeatOn"]:
            return 1.
        rho = PROTONMASS * nHcgs / (1 - helium)
        overden = rho / (self.p["rho_crit_baryon"] * pow_(1 + redshift, 3.0))
        if overden >= self.p["HeliumHeatThresh"]:
            overden = self.p["HeliumHeatThresh"]
        return self.p["HeliumHeatAmp"] * pow_(overden, self.p["HeliumHeatExp"])

    # ---- the 13 tables, init_cooling_rates cooling_rates.c:1135-1171
    TABLES = ("rec_GammaH0", "rec_GammaHe0", "rec_GammaHep", "rec_alphaHp", "rec_alphaHep", "rec_alphaHepp", "cool_collisH0", "cool_collisHe0",
              "cool_collisHeP", "cool_recombHp", "cool_recombHeP", "cool_recombHePP", "cool_freefree1")

    def init_tables(self):
        self.fn = dict(rec_GammaH0=self.recomb_GammaeH0, rec_GammaHe0=self.recomb_GammaeHe0, rec_GammaHep=self.recomb_GammaeHep,
                       rec_alphaHp=self.recomb_alphaHp, rec_alphaHep=self.recomb_alphaHepd, rec_alphaHepp=self.recomb_alphaHepp,
                       cool_collisH0=self.cool_CollisionalH0, cool_collisHe0=self.cool_CollisionalHe0, cool_collisHeP=self.cool_CollisionalHeP,
                       cool_recombHp=self.cool_RecombHp, cool_recombHeP=self.cool_RecombHeP, cool_recombHePP=self.cool_RecombHePP,
                       cool_freefree1=self.cool_FreeFree1)
        self.temp_tab = [RECOMBTMIN + (RECOMBTMAX - RECOMBTMIN) * i / NRECOMBTAB for i in range(NRECOMBTAB)]   # :1155
        tt = [exp(t) for t in self.temp_tab]                                                                   # :1156
        self.tab = {name: [self.fn[name](t) for t in tt] for name in self.TABLES}

    def get_interpolated_recomb(self, logt, name):                             # :644-656
        dind = (logt - RECOMBTMIN) / (RECOMBTMAX - RECOMBTMIN) * NRECOMBTAB
        # (int) truncates towards zero; a value no int holds (or NaN) is outside the table, as in the engine
        if not (dind > -1.0 and dind < NRECOMBTAB - 1):
            return self.fn[name](exp_(logt)) * (1 + self.perturb)
        index = int(dind)
        rec_tab = self.tab[name]
        return (rec_tab[index + 1] * (dind - index) + rec_tab[index] * (1 - (dind - index))) * (1 + self.perturb)

    # ---- the UV background, cooling_rates.c:315-397
    def get_photo_rate(self, redshift, ydata):                                 # :316-331
        if not self.p["PhotoIonizationOn"]:
            return 0
        log1z = log10(1 + redshift)
        tc = self.tc
        if tc is None or log1z >= tc.log1z[-1]:
            return 0
        elif log1z < tc.log1z[0]:
            photo_rate = ydata[0]
        else:
            photo_rate = gsl_interp_linear(tc.log1z, ydata, log1z)
        return pow_(10, photo_rate) * self.p["PhotoIonizeFactor"]

    def get_self_shield_dens(self, redshift, uvbg):                            # :345-361
        if uvbg["gJH0"] == 0:
            return 1e10
        G12 = uvbg["gJH0"] / 1e-12
        if redshift <= GrayOpac_zz[0]:
            greyopac = GrayOpac_ydata[0]
        elif redshift >= GrayOpac_zz[-1]:
            greyopac = GrayOpac_ydata[-1]
        else:
            greyopac = gsl_interp_linear(GrayOpac_zz, GrayOpac_ydata, redshift)
        return 6.73e-3 * pow_(greyopac / 2.49e-18, -2. / 3) * pow_(G12, 2. / 3) * pow_(self.p["fBar"] / 0.17, -1. / 3)

    def get_global_UVBG(self, redshift, during_helium_reionization=False):     # :365-397
        uvbg = zero_uvbg()
        if not self.p["PhotoIonizationOn"] or self.tc is None:
            return uvbg
        uvbg["zreion"] = pow_(10, self.tc.log1z[-1]) - 1
        thr = self.p["UVRedshiftThreshold"]
        if thr >= 0.:
            uvbg["zreion"] = thr
        if thr >= 0. and redshift > thr:
            return uvbg
        uvbg["gJH0"] = self.get_photo_rate(redshift, self.tc.Gamma_HI)
        uvbg["gJHe0"] = self.get_photo_rate(redshift, self.tc.Gamma_HeI)
        uvbg["gJHep"] = self.get_photo_rate(redshift, self.tc.Gamma_HeII)
        uvbg["epsH0"] = self.get_photo_rate(redshift, self.tc.Eps_HI)
        uvbg["epsHe0"] = self.get_photo_rate(redshift, self.tc.Eps_HeI)
        uvbg["epsHep"] = 0 if during_helium_reionization else self.get_photo_rate(redshift, self.tc.Eps_HeII)
        uvbg["self_shield_dens"] = self.get_self_shield_dens(redshift, uvbg)
        return uvbg

    # ---- the network, cooling_rates.c:432-835
    def self_shield_corr(self, nh, logt, ssdens):                              # :438-450
        if not self.p["SelfShieldingOn"] or nh < ssdens * 0.01:
            return 1
        T4 = exp_(0.17 * (logt - log(1e4)))
        nSSh = 1.003 * ssdens * T4
        return 0.98 * pow_(1 + pow_(nh / nSSh, 1.64), -2.28) + 0.02 * pow_(1 + nh / nSSh, -0.84)

    def nH0_internal(self, logt, ne, uvbg, photofac):                          # :660-670
        alphaHp = self.get_interpolated_recomb(logt, "rec_alphaHp")
        GammaeH0 = self.get_interpolated_recomb(logt, "rec_GammaH0")
        photorate = 0
        if uvbg["gJH0"] > 0. and ne > 1e-50:
            photorate = uvbg["gJH0"] / ne * photofac
        return alphaHp / (alphaHp + GammaeH0 + photorate)

    @staticmethod
    def nHp_internal(nH0):                                                     # :673-680
        nHp = 1. - nH0
        if nHp < 0:
            return 0
        return nHp

    def nHe_internal(self, nh, logt, ne, uvbg, photofac):                      # :690-715; returns (nHe0, nHep, nHepp)
        alphaHep = self.get_interpolated_recomb(logt, "rec_alphaHep")
        alphaHepp = self.get_interpolated_recomb(logt, "rec_alphaHepp")
        GammaHe0 = self.get_interpolated_recomb(logt, "rec_GammaHe0")
        GammaHep = self.get_interpolated_recomb(logt, "rec_GammaHep")
        if uvbg["gJHe0"] > 0. and ne > 1e-50:
            GammaHe0 += uvbg["gJHe0"] / ne * photofac
            GammaHep += uvbg["gJHep"] / ne * photofac
        if GammaHe0 > 1e-50:
            nHep = nh / (1 + alphaHep / GammaHe0 + GammaHep / alphaHepp)
            nHe0 = nHep * alphaHep / GammaHe0
            nHepp = nHep * GammaHep / alphaHepp
        else:
            nHep, nHe0, nHepp = 0, nh, 0
        return nHe0, nHep, nHepp

    def get_temp_internal(self, nebynh, ienergy, helium):                      # :735-752
        hy_mass = 1 - helium
        muienergy = 4 / (hy_mass * (3 + 4 * nebynh) + 1) * ienergy
        temp = GAMMA_MINUS1 * PROTONMASS / BOLTZMANN * muienergy
        if temp < self.p["MinGasTemp"]:
            return self.p["MinGasTemp"]
        return temp

    def ne_internal(self, nh, ienergy, ne, helium, uvbg):                      # :755-765; returns (ne, logt)
        self.evals += 1
        yy = helium / 4 / (1 - helium)
        temp = self.get_temp_internal(ne / nh, ienergy, helium)
        logt = log(temp) if temp > 0 else (-math.inf if temp == 0 else math.nan)
        photofac = self.self_shield_corr(nh, logt, uvbg["self_shield_dens"])
        nH0 = self.nH0_internal(logt, ne, uvbg, photofac)
        nHp = self.nHp_internal(nH0)
        nHe0, nHep, nHepp = self.nHe_internal(nh, logt, ne, uvbg, photofac)
        return nh * nHp + yy * nHep + 2 * yy * nHepp, logt

    def scipy_optimize_fixed_point(self, ne_init, nh, ienergy, helium, uvbg):  # :779-809; returns (ne, logt)
        ne0 = ne_init
        logt = math.nan
        done = False
        for i in range(self.net_maxiter):
            ne1, logt1 = self.ne_internal(nh, ienergy, ne0 * nh, helium, uvbg)
            ne1 /= nh
            if fabs(ne1 - ne0) < ITERCONV:
                logt = logt1
                ne0 = ne1
                done = True
                self.max_fp = max(self.max_fp, i + 1)
                break
            ne2, logt1 = self.ne_internal(nh, ienergy, ne1 * nh, helium, uvbg)
            ne2 /= nh
            d = ne0 + ne2 - 2.0 * ne1
            pp = ne2
            if d > 1e-15 or d < -1e-15:
                pp = ne0 - (ne1 - ne0) * (ne1 - ne0) / d
            ne0 = pp
            if ne0 < 0:
                ne0 = 0
        if not math.isfinite(ne0) or not done:
            self.max_fp = max(self.max_fp, self.net_maxiter + 1)
            raise NotConverged("Ionization rate network failed to converge")
        return ne0 * nh, logt

    def get_equilib_ne(self, density, ienergy, helium, uvbg, ne_init):         # :817-827; returns (ne, logt)
        nh = density * (1 - helium)
        if ne_init <= 0:
            ne_init = 1.0
        return self.scipy_optimize_fixed_point(ne_init, nh, ienergy, helium, uvbg)

    def TableMetalCoolingRate(self, redshift, temp, nHcgs):                    # cooling_uvfluc.c:307-322
        if self.metal is None:
            return 0
        return self.metal.interp_eval([redshift, log10(nHcgs), log10(temp)])

    def get_heatingcooling_rate(self, density, ienergy, helium, redshift, metallicity, uvbg, ne_equilib):
        """cooling_rates.c:1248-1310; returns (LambdaNet in erg/s/g, ne / nh)"""
        ne, logt = self.get_equilib_ne(density, ienergy, helium, uvbg, ne_equilib)
        nh = density * (1 - helium)
        nebynh = ne / nh
        temp = self.get_temp_internal(nebynh, ienergy, helium)
        photofac = self.self_shield_corr(nh, logt, uvbg["self_shield_dens"])
        yy = helium / 4 / (1 - helium)
        nH0 = self.nH0_internal(logt, ne, uvbg, photofac)
        nHp = self.nHp_internal(nH0)
        nHe0, nHep, nHepp = self.nHe_internal(nh, logt, ne, uvbg, photofac)
        nHep *= yy / nh
        nHe0 *= yy / nh
        nHepp *= yy / nh
        gi = self.get_interpolated_recomb
        LambdaCollis = nebynh * (gi(logt, "cool_collisH0") * nH0 + gi(logt, "cool_collisHe0") * nHe0 + gi(logt, "cool_collisHeP") * nHep)
        LambdaRecomb = nebynh * (gi(logt, "cool_recombHp") * nHp + gi(logt, "cool_recombHeP") * nHep + gi(logt, "cool_recombHePP") * nHepp)
        cff = gi(logt, "cool_freefree1")
        if self.cooling == Enzo2Nyx:
            LambdaFF = nebynh * (cff * (nHp + nHep) + self.cool_FreeFree(temp, 2) * nHepp)
        else:
            LambdaFF = nebynh * (cff * (nHp + nHep) + 4 * cff * nHepp)
        LambdaCmptn = nebynh * self.cool_InverseCompton(temp, redshift) / nh
        Lambda = LambdaCollis + LambdaRecomb + LambdaFF + LambdaCmptn
        Heat = (nH0 * uvbg["epsH0"] + nHe0 * uvbg["epsHe0"] + nHep * uvbg["epsHep"]) / nh
        Heat *= self.cool_he_reion_factor(density, helium, redshift)
        MetalCooling = metallicity * self.TableMetalCoolingRate(redshift, temp, nh) if metallicity != 0 else 0.0
        LambdaNet = Heat - Lambda - MetalCooling
        return LambdaNet * pow_(1 - helium, 2) * density / PROTONMASS, nebynh

    def get_temp(self, density, ienergy, helium, uvbg, ne_init):               # :1316-1324; returns (temp, ne / nh)
        ne, _ = self.get_equilib_ne(density, ienergy, helium, uvbg, ne_init)
        nh = density * (1 - helium)
        return self.get_temp_internal(ne / nh, ienergy, helium), ne / nh

    def get_neutral_fraction_phys_cgs(self, density, ienergy, helium, uvbg, ne_init):   # :1330-1339; returns (nH0, ne / nh)
        ne, logt = self.get_equilib_ne(density, ienergy, helium, uvbg, ne_init)
        nh = density * (1 - helium)
        photofac = self.self_shield_corr(nh, logt, uvbg["self_shield_dens"])
        return self.nH0_internal(logt, ne, uvbg, photofac), ne / nh

    # ---- cooling.c
    def get_lambdanet(self, rho, u, redshift, Z, uvbg, ne_guess, isHeIIIionized, lmfp_heating):   # cooling.c:42-52
        LambdaNet, ne_guess = self.get_heatingcooling_rate(rho, u, 1 - HYDROGEN_MASSFRAC, redshift, Z, uvbg, ne_guess)
        if not isHeIIIionized:
            LambdaNet += lmfp_heating / (self.p["units_rho_crit_baryon"] * pow_(1 + redshift, 3))
        return LambdaNet, ne_guess

    def DoCooling(self, redshift, u_old, rho, dt, uvbg, ne_guess, Z, MinEgySpec, isHeIIIionized, lmfp_heating=0.0):
        """cooling.c:57-138; returns (unew, ne_guess, info) with info = dict(bisections, floor)"""
        info = dict(bisections=0, floor=0)
        if not self.p["CoolingOn"]:
            return 0, ne_guess, info
        it = 0
        rho *= self.p["density_in_phys_cgs"] / PROTONMASS
        u_old *= self.p["uu_in_cgs"]
        MinEgySpec *= self.p["uu_in_cgs"]
        if u_old < MinEgySpec:
            u_old = MinEgySpec
        dt *= self.p["tt_in_s"]
        u = u_old
        u_lower = u
        u_upper = u
        lam = lambda uu, ng: self.get_lambdanet(rho, uu, redshift, Z, uvbg, ng, isHeIIIionized, lmfp_heating)
        LambdaNet, ne_guess = lam(u, ne_guess)
        guard = 0
        if u - u_old - LambdaNet * dt < 0:          # heating
            while True:
                u_lower = u_upper
                u_upper *= 1.1
                guard += 1
                if guard > BRACKET_MAXITER:
                    raise NotConverged("bracketing")
                LambdaNet, ne_guess = lam(u_upper, ne_guess)
                if not (u_upper - u_old - LambdaNet * dt < 0):
                    break
        else:
            while True:
                u_upper = u_lower
                u_lower /= 1.1
                if u_upper <= MinEgySpec:
                    break
                guard += 1
                if guard > BRACKET_MAXITER:
                    raise NotConverged("bracketing")
                LambdaNet, ne_guess = lam(u_lower, ne_guess)
                if not (u_lower - u_old - LambdaNet * dt > 0):
                    break
        while True:
            u = 0.5 * (u_lower + u_upper)
            if u_upper <= MinEgySpec:
                u = MinEgySpec
                info["floor"] = 1
                break
            LambdaNet, ne_guess = lam(u, ne_guess)
            if u - u_old - LambdaNet * dt > 0:
                u_upper = u
            else:
                u_lower = u
            du = u_upper - u_lower
            it += 1
            info["bisections"] += 1
            if not (fabs(du / u) > 1.0e-6 and it < MAXITER):
                break
        if it >= MAXITER:
            raise NotConverged("failed to converge in DoCooling()")
        u /= self.p["uu_in_cgs"]
        return u, ne_guess, info

    def GetCoolingTime(self, redshift, u_old, rho, uvbg, ne_guess, Z):         # cooling.c:143-163; returns (tcool, ne_guess)
        if not self.p["CoolingOn"]:
            return 0, ne_guess
        rho *= self.p["density_in_phys_cgs"] / PROTONMASS
        u_old *= self.p["uu_in_cgs"]
        LambdaNet, ne_guess = self.get_heatingcooling_rate(rho, u_old, 1 - HYDROGEN_MASSFRAC, redshift, Z, uvbg, ne_guess)
        if LambdaNet >= 0:
            return 0, ne_guess
        coolingtime = u_old / (-LambdaNet)
        coolingtime /= self.p["tt_in_s"]
        return coolingtime, ne_guess

    def GetNeutralFraction(self, u_old, rho, uvbg, ne_init):                   # cooling.c:166-176
        if not self.p["CoolingOn"]:
            return 1
        rho *= self.p["density_in_phys_cgs"] / PROTONMASS
        u_old *= self.p["uu_in_cgs"]
        return self.get_neutral_fraction_phys_cgs(rho, u_old, 1 - HYDROGEN_MASSFRAC, uvbg, ne_init)[0]

    # ---- sfr_eff.c
    @staticmethod
    def entropy_to_u(density, a3inv):                                          # sfr_eff.c:138-142
        return exp(GAMMA_MINUS1 * log(density * a3inv)) / GAMMA_MINUS1

    def cooling_direct(self, density, entropy, ne, Z, heiii, dtime, redshift, a3inv, uvbg, lastred, lmfp_heating=0.0):
        """sfr_eff.c:463-514 for one particle, with the step's UV background; returns (Entropy, Ne, info)"""
        enttou = self.entropy_to_u(density, a3inv)
        uold = entropy * enttou
        info = dict(bisections=0, floor=0, reion=0)
        if self.p["HIReionTemp"] > 0 and uvbg["zreion"] >= redshift and uvbg["zreion"] < lastred:
            meanweight = 4 / (8 - 6 * (1 - HYDROGEN_MASSFRAC))
            unew = self.p["temp_to_u"] / meanweight * self.p["HIReionTemp"]
            if uold > unew:
                unew = uold
            info["reion"] = 1
        else:
            meanweight = 4.0 / (1 + 3 * HYDROGEN_MASSFRAC)
            MinEgySpec = self.p["temp_to_u"] / meanweight * self.p["sfr_MinGasTemp"]
            unew, ne, di = self.DoCooling(redshift, uold, density * a3inv, dtime, uvbg, ne, Z, MinEgySpec, heiii, lmfp_heating)
            info.update(di)
        info["unew"] = unew
        return unew / enttou, ne, info


def cool_particles(C, d, times, step, active=None):
    """cooling_and_starformation's loop with StarformationOn == 0 (sfr_eff.c:224-272) over the table `d` (dict of arrays: type, mass,
    density, entropy, ne, sfr and optionally metallicity, heiii_ionized, tb_hydro; type 7 = garbage).  times: dict(atime, hubble,
    dloga_bin[47]); step: dict(uvbg, long_mean_free_path_heating, lastred[47]).  Returns new entropy / ne / sfr arrays, the evaluations
    per particle (-1: not treated), the per-particle info and the list of particles that did not converge (left untouched)."""
    n = len(d["type"])
    ent, ne, sfr = d["entropy"].copy(), d["ne"].copy(), d["sfr"].copy()
    evals = np.full(n, -1, np.int32)
    maxfp = np.zeros(n, np.int32)
    infos, failed = {}, []
    redshift = 1. / times["atime"] - 1
    a3inv = 1. / (times["atime"] * times["atime"] * times["atime"])
    lastred = np.broadcast_to(np.asarray(step.get("lastred", 0.0), np.float64), (47,))
    for p_i in (range(n) if active is None else [int(x) for x in active]):
        if d["type"][p_i] != 0 or not d["mass"][p_i] > 0:
            continue
        b = int(d["tb_hydro"][p_i]) if d.get("tb_hydro") is not None else 0
        dtime = times["dloga_bin"][b] / times["hubble"]
        Z = float(d["metallicity"][p_i]) if d.get("metallicity") is not None else 0.0
        he = int(d["heiii_ionized"][p_i]) if d.get("heiii_ionized") is not None else 0
        C.evals, C.max_fp = 0, 0
        try:
            e, x, info = C.cooling_direct(float(d["density"][p_i]), float(d["entropy"][p_i]), float(d["ne"][p_i]), Z, he, dtime, redshift, a3inv,
                                          step["uvbg"], float(lastred[b]), step.get("long_mean_free_path_heating", 0.0))
            ent[p_i], ne[p_i], sfr[p_i] = e, x, 0.0
            infos[p_i] = info
        except NotConverged:
            failed.append(p_i)
        evals[p_i] = C.evals
        maxfp[p_i] = C.max_fp
    return dict(entropy=ent, ne=ne, sfr=sfr, evals=evals, maxfp=maxfp, info=infos, failed=failed)


# ---- the input sets of the tests (tests/test_cooling_restated.py checks what they cover, tests/test_gpu_cooling.py runs them on the GPU) ----
def synthetic_metal_table():
    """a 3 x 5 x 7 stand-in for the 4 MB Cloudy table: redshift 0 .. 4, log10 nH -6 .. -1, log10 T 3 .. 8; rates of the table's magnitude"""
    z, nh, t = np.linspace(0.0, 4.0, 3), np.linspace(-6.0, -1.0, 5), np.linspace(3.0, 8.0, 7)
    rate = 1e-23 * (1.0 + 0.3 * z[:, None, None]) * (1.2 + np.sin(1.7 * nh[None, :, None])) * (0.2 + np.exp(-0.5 * (t[None, None, :] - 5.3) ** 2))
    return z, nh, t, np.ascontiguousarray(rate)


def sample_times(atime, seed):
    """mpg_sph_times as far as the cooling reads it: atime, hubble and dloga_bin (bin 0 has no step, as in the reference; the others give
    dtime = 1e-4 .. 0.5 in a shuffled order)"""
    rs = np.random.RandomState(seed)
    hubble = 0.1 * atime ** -1.5
    dt = np.concatenate([[0.0], rs.permutation(np.exp(np.linspace(np.log(1e-4), np.log(0.5), 46)))])
    return dict(atime=atime, hubble=hubble, dloga_bin=dt * hubble)


def sample_inputs(n, seed, atime, metals=False, cold_hot=False):
    """n rows: gas with proper density 1e-9 .. 1e-1, u = 1 .. 3e6, an Ne guess in 0 .. 1.2 (every eighth exactly 0), both values of
    HeIIIionized, every hydro bin; every 13th row is no gas, every 17th is garbage (type 7), every 19th has no mass.  cold_hot: one row in
    sixteen has u = 1e-4 .. 1e-2 (T < 1 K) or 3e7 .. 3e8 (T > 1e9 K)."""
    rs = np.random.RandomState(seed)
    a3inv = 1. / atime ** 3
    typ = np.zeros(n, np.uint8)
    idx = np.arange(n)
    typ[idx % 13 == 5] = rs.choice([1, 4, 5], size=int((idx % 13 == 5).sum()))
    typ[idx % 17 == 7] = 7
    mass = np.ones(n, np.float32)
    mass[idx % 19 == 11] = rs.choice([0.0, -1.0], size=int((idx % 19 == 11).sum()))
    rho = np.exp(rs.uniform(np.log(1e-9), np.log(1e-1), n))
    u = np.exp(rs.uniform(np.log(1.0), np.log(3e6), n))
    if cold_hot:
        k = idx % 16 == 3
        u[k] = np.where(rs.uniform(size=int(k.sum())) < 0.5, np.exp(rs.uniform(np.log(1e-4), np.log(1e-2), int(k.sum()))),
                        np.exp(rs.uniform(np.log(3e7), np.log(3e8), int(k.sum()))))
    density = rho / a3inv
    enttou = np.array([Cooling.entropy_to_u(float(x), a3inv) for x in density])
    ne = rs.uniform(0.0, 1.2, n)
    ne[idx % 8 == 1] = 0.0
    d = dict(type=typ, mass=mass, density=density, entropy=u / enttou, ne=ne, sfr=rs.uniform(0.5, 1.5, n),
             heiii_ionized=(rs.uniform(size=n) < 0.5).astype(np.uint8), tb_hydro=rs.randint(0, 47, n).astype(np.uint8))
    if metals:
        d["metallicity"] = np.where(rs.uniform(size=n) < 0.6, rs.uniform(0.0, 2.0, n), 0.0)
    return d


def config(name, treecool_columns, perturb=0.0):
    """the settings of the tests by name: returns (Cooling, times, step, inputs-maker)"""
    tc = TreeCool(treecool_columns)
    metal = None
    if name == "sherwood_z3":      # Verner96 / Sherwood at z = 3: self-shielding, HeliumHeatOn, long-mean-free-path heating, metals
        par = default_params(HeliumHeatOn=1, HeliumHeatThresh=10.0, HeliumHeatAmp=1.4, HeliumHeatExp=0.3, sfr_MinGasTemp=5.0)
        atime, lmfp, seed, kw = 0.25, 3e-30, 101, dict(metals=True)
        metal = MetalTable(*synthetic_metal_table())
    elif name == "sherwood_reion":  # ... at z = 15, just after the UV background switches on (zreion = 15.1): the HIReionTemp branch for the
        par = default_params(HIReionTemp=2e4, sfr_MinGasTemp=2000.0)   # bins whose step began before it; a high energy floor
        atime, lmfp, seed, kw = 1 / 16.0, 0.0, 102, {}
    elif name == "sherwood_z16":    # ... at z = 16, above the table: gJH0 = 0
        par = default_params(sfr_MinGasTemp=300.0)
        atime, lmfp, seed, kw = 1 / 17.0, 0.0, 103, {}
    elif name == "kwh_z0":          # Cen92 / KWH92 at z = 0 as test_cooling.c sets it, no temperature floors: T < 1 K and T > 1e9 K
        par = default_params(recomb=Cen92, cooling=KWH92, SelfShieldingOn=0, MinGasTemp=0.0, sfr_MinGasTemp=0.0)
        atime, lmfp, seed, kw = 1.0, 1e-31, 104, dict(cold_hot=True)
    elif name == "badnell_nyx":     # Badnell06 / Enzo2Nyx at z = 2
        par = default_params(recomb=Badnell06, cooling=Enzo2Nyx, MinGasTemp=0.0, sfr_MinGasTemp=1.0)
        atime, lmfp, seed, kw = 1 / 3.0, 0.0, 105, dict(cold_hot=True)
    else:
        raise KeyError(name)
    C = Cooling(par, tc, metal, perturb)
    redshift = 1. / atime - 1
    uvbg = C.get_global_UVBG(redshift)
    lastred = np.full(47, redshift + 0.05)
    if name == "sherwood_reion":
        lastred[::2] = 15.3           # even bins began their step before zreion = 15.1, odd bins after it
    step = dict(uvbg=uvbg, long_mean_free_path_heating=lmfp, lastred=lastred, redshift=redshift, helium=0.0)
    times = sample_times(atime, seed)
    return C, times, step, (lambda n, s=seed, a=atime, k=kw: sample_inputs(n, s, a, **k))


CONFIGS = ("sherwood_z3", "sherwood_reion", "sherwood_z16", "kwh_z0", "badnell_nyx")
