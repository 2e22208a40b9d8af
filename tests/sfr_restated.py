"""Plain-Python restatement of the star-formation loop of MP-Gadget (libgadget/sfr_eff.c:186-394 without the spawning of :288-393), statement
by statement, on top of cooling_restated.Cooling.  IEEE semantics where Python would raise: a cooling time of 0 (net heating) gives
y = inf, cloudfrac = 1 and trelax = 0, as in C.  Test infrastructure: the GPU tests compare csrc/sfr.hip with it, tests/test_sfr_restated.py
holds it to identities that need no second implementation and shows its decisions to be stable on the very inputs the GPU tests use."""
import math

import numpy as np

import cooling_restated as R

METAL_YIELD = 0.02                                                    # sfr_eff.h:11
CRIT_DENSITY, CRIT_MOLECULAR_H2, CRIT_SELFGRAVITY, CRIT_CONVERGENT_FLOW, CRIT_CONTINUOUS_CUTOFF = 1, 3, 5, 13, 21   # sfr_eff.h:16-23
WIND_SUBGRID, WIND_USE_HALO, WIND_FIXED_EFFICIENCY = 1, 4, 8          # winds.h:13-20
ROW_SKIPPED, ROW_COOLED, ROW_STARFORMING = 0, 1, 2
OUT_NOSTAR, OUT_CONVERT, OUT_SPAWN, OUT_ERROR = 0, 1, 2, 3

# The largest error (column_error below) of every output column of a star-forming row under (a) a +-2e-15 perturbation of every table
# lookup and (b) a +-1-ulp perturbation of every pow / exp / sqrt / log result of the model, as tests/test_sfr_restated.py measures them
# on the input sets of the GPU tests over all 18 cases (it asserts that what it measures stays below these).  Sfr carries the cancellation
# of 1 - exp(-p) at small p.  The GPU tests hold every column to 100 x these, with a floor of 1e-13 (TOLERANCE).
SENSITIVITY = dict(entropy=1.6e-14, ne=4.5e-16, sfr=8.5e-13, metallicity=4.3e-16, stellarmass=8.8e-16)
TOLERANCE = {k: max(100 * v, 1e-13) for k, v in SENSITIVITY.items()}


def column_error(k, got, ref):
    """the error of column k of star-forming rows, as the tests measure it: absolute for Ne (of order one); for the others relative to the
    reference value or, where that is smaller (a rate clipped to zero, a particle without metals), to the median of the column's non-zero
    reference values"""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    if k == "ne":
        return np.abs(got - ref)
    nz = np.abs(ref[ref != 0])
    floor = float(np.median(nz)) if len(nz) else 1.0
    return np.abs(got - ref) / np.maximum(np.abs(ref), floor)


def HAS(val, flag):                                                   # types.h:19
    return (flag & val) == flag


def div(a, b):
    """a / b as C gives it"""
    try:
        return a / b
    except ZeroDivisionError:
        if a != a or a == 0:
            return math.nan
        return math.copysign(math.inf, a) * math.copysign(1.0, b)


class Sfr:
    """sfr_params after init_cooling_and_star_formation, on a Cooling; `ulp` moves every pow / exp / sqrt / log result of the model by that
    many units in the last place (the stability test)"""

    def __init__(self, C, par, ulp=0):
        self.C, self.p, self.ulp = C, dict(par), ulp

    def _f(self, x):
        if self.ulp and math.isfinite(x) and x != 0:
            for _ in range(abs(self.ulp)):
                x = math.nextafter(x, math.inf if self.ulp > 0 else -math.inf)
        return x

    def pow(self, x, y):
        return self._f(R.pow_(x, y))

    def exp(self, x):
        return self._f(R.exp_(x)) if x != 0 else 1.0       # (exp(0) is exact in every libm)

    def sqrt(self, x):
        return self._f(math.sqrt(x)) if x >= 0 else math.nan

    def log(self, x):
        return self._f(math.log(x))

    def entropy_to_u(self, density, a3inv):                           # sfr_eff.c:138-142
        return self.exp(R.GAMMA_MINUS1 * self.log(density * a3inv)) / R.GAMMA_MINUS1

    def sfreff_on_eeqos(self, density, delaytime, a3inv):             # :534-566
        P = self.p
        flag = 0
        if density * a3inv >= P["PhysDensThresh"]:
            flag = 1
        if density < P["OverDensThresh"]:
            flag = 0
        if delaytime > 0:
            flag = 0
        assert P["BHFeedbackUseTcool"] != 2
        return flag

    def quicklyastarformation(self, density, entropy, a3inv, rnd1):   # :706-725
        P = self.p
        if density <= P["OverDensThresh"]:
            return 0
        enttou = R.Cooling.entropy_to_u(density, a3inv)
        unew = entropy * enttou
        meanweight = (4 / (8 - 5 * (1 - R.HYDROGEN_MASSFRAC)))
        temp = unew * meanweight / self.C.p["temp_to_u"]
        if temp >= P["QuickLymanAlphaTempThresh"]:
            return 0
        if rnd1 < P["QuickLymanAlphaProbability"]:
            return 1
        return 0

    def get_sfr_eeqos(self, r, dtime, uvbg, redshift, a3inv):        # :804-841
        P = self.p
        data = dict(trelax=P["MaxSfrTimescale"], tsfr=P["MaxSfrTimescale"], egyhot=P["EgySpecCold"], egycold=P["EgySpecCold"], cloudfrac=0.0, ne=0.0)
        if not self.sfreff_on_eeqos(r["density"], r["delaytime"], a3inv):
            return data
        data["ne"] = r["ne"]
        data["tsfr"] = self.sqrt(P["PhysDensThresh"] / (r["density"] * a3inv)) * P["MaxSfrTimescale"]
        if P["BoostSFDenseGas"] and ((r["density"] * a3inv) / P["PhysDensThresh"] > P["BoostSFOverDenseFactor"]):
            data["tsfr"] = P["PhysDensThresh"] / (r["density"] * a3inv) * P["MaxSfrTimescale"]
        if data["tsfr"] < dtime and dtime > 0:
            data["tsfr"] = dtime
        factorEVP = self.pow(r["density"] * a3inv / P["PhysDensThresh"], -0.8) * P["FactorEVP"]
        data["egyhot"] = P["EgySpecSN"] / (1 + factorEVP) + P["EgySpecCold"]
        data["egycold"] = P["EgySpecCold"]
        tcool, data["ne"] = self.C.GetCoolingTime(redshift, data["egyhot"], r["density"] * a3inv, uvbg, data["ne"], r["metallicity"])
        y = div(data["tsfr"], tcool) * data["egyhot"] / (P["FactorSN"] * P["EgySpecSN"] - (1 - P["FactorSN"]) * P["EgySpecCold"])
        data["cloudfrac"] = 1 + div(1, 2 * y) - self.sqrt(div(1, y) + div(1, 4 * y * y))
        data["trelax"] = data["tsfr"] * (1 - data["cloudfrac"]) / data["cloudfrac"] / (P["FactorSN"] * (1 + factorEVP))
        data["y"], data["tcool"] = y, tcool
        return data

    def get_sfr_factor_due_to_h2(self, r, atime):                     # :1041-1077
        a2 = atime * atime
        zoverzsun = r["metallicity"] / METAL_YIELD
        ev_NH = 0.0
        if r["density"] > 0:
            if r["gradrho_mag"] > 0:
                ev_NH = r["density"] * r["density"] / r["gradrho_mag"]
            ev_NH += r["density"] * r["hsml"]
        tau_fmol = ev_NH / a2
        tau_fmol *= (0.1 + zoverzsun)
        if tau_fmol > 0:
            tau_fmol *= 434.78 * self.p["tau_fmol_unit"]
            y = 0.756 * (1 + 3.1 * self.pow(zoverzsun, 0.365))
            y = self.log(1 + 0.6 * y + 0.01 * y * y) / (0.6 * tau_fmol)
            y = 1 - 0.75 * y / (1 + 0.25 * y)
            if y < 0:
                y = 0
            if y > 1:
                y = 1
            return y
        return 1.0

    def get_sfr_factor_due_to_selfgravity(self, r, atime, a3inv, hubble):   # :1079-1112
        P = self.p
        a2 = atime * atime
        divv = r["divvel"] / a2
        divv += 3.0 * hubble * a2
        if HAS(P["StarformationCriterion"], CRIT_CONVERGENT_FLOW):
            if divv >= 0:
                return 0
        dv2abs = (divv * divv + (r["curlvel"] / a2) * (r["curlvel"] / a2))
        alpha_vir = 0.2387 * dv2abs / (P["GravInternal"] * r["density"] * a3inv)
        if (alpha_vir < 1.0) or (r["density"] * a3inv > 100. * P["PhysDensThresh"]):
            y = 66.7
        else:
            y = 0.1
        if HAS(P["StarformationCriterion"], CRIT_CONTINUOUS_CUTOFF):
            y *= 1.0 / (1.0 + alpha_vir)
        return y

    def get_starformation_rate_full(self, r, d, atime, a3inv, hubble):      # :843-862
        P = self.p
        if not self.sfreff_on_eeqos(r["density"], r["delaytime"], a3inv):
            return 0
        cloudmass = d["cloudfrac"] * r["mass"]
        rateOfSF = (1 - P["FactorSN"]) * cloudmass / d["tsfr"]
        if HAS(P["StarformationCriterion"], CRIT_MOLECULAR_H2):
            rateOfSF *= self.get_sfr_factor_due_to_h2(r, atime)
        if HAS(P["StarformationCriterion"], CRIT_SELFGRAVITY):
            rateOfSF *= self.get_sfr_factor_due_to_selfgravity(r, atime, a3inv, hubble)
        return rateOfSF

    def cooling_relaxed(self, r, d, dtime, uvbg, redshift, a3inv, ne, Z, bhheated):   # :666-701; returns (Entropy, BHHeated)
        P = self.p
        egyeff = P["EgySpecCold"] * d["cloudfrac"] + (1 - d["cloudfrac"]) * d["egyhot"]
        densityfac = self.entropy_to_u(r["density"], a3inv)
        egycurrent = r["entropy"] * densityfac
        trelax = d["trelax"]
        if P["BHFeedbackUseTcool"] == 3 or (P["BHFeedbackUseTcool"] == 1 and (bhheated or egycurrent > 5e6)):
            if egycurrent > egyeff:
                tcool, _ = self.C.GetCoolingTime(redshift, egycurrent, r["density"] * a3inv, uvbg, ne, Z)
                if tcool < trelax and tcool > 0:
                    trelax = tcool
            bhheated = 0
        return (egyeff + (egycurrent - egyeff) * self.exp(div(-dtime, trelax))) / densityfac, bhheated

    def find_star_mass(self, mass, generation):                        # :1002-1023
        P = self.p
        if P["QuickLymanAlphaProbability"] > 0:
            return mass
        mass_of_star = P["avg_baryon_mass"] / P["Generations"]
        if mass_of_star > mass:
            mass_of_star = mass
        if mass < 2 * mass_of_star or generation > P["Generations"]:
            mass_of_star = mass
        return mass_of_star

    def starformation(self, r, dloga, hubble, redshift, a3inv, uvbg, w, rnd1):   # :731-800, without slots_split_particle
        P = self.p
        dtime = dloga / hubble
        d = self.get_sfr_eeqos(r, dtime, uvbg, redshift, a3inv)
        atime = 1 / (1 + redshift)
        smr = self.get_starformation_rate_full(r, d, atime, a3inv, hubble)
        sm = smr * dtime
        p = sm / r["mass"]
        dM = r["mass"] * (1 - self.exp(-p))
        if dtime > 0:
            sfr = dM / dtime * P["UnitSfr_in_solar_per_year"]
        else:
            sfr = smr * P["UnitSfr_in_solar_per_year"]
        ne = d["ne"]
        frac = (1 - self.exp(-p))
        Z = r["metallicity"] + w * METAL_YIELD * frac / P["Generations"]
        entropy, bhheated = r["entropy"], r["bhheated"]
        if dloga > 0 and r["tb_hydro"]:
            entropy, bhheated = self.cooling_relaxed(r, d, dtime, uvbg, redshift, a3inv, ne, Z, bhheated)
        mass_of_star = self.find_star_mass(r["mass"], r["generation"])
        prob = dM / mass_of_star
        form_star = rnd1 < prob
        outcome = OUT_NOSTAR
        if form_star:
            outcome = OUT_SPAWN if r["mass"] >= 1.1 * mass_of_star else OUT_CONVERT
        if not form_star or outcome == OUT_SPAWN:
            Z += (1 - w) * METAL_YIELD * frac / P["Generations"]
        return dict(entropy=entropy, ne=ne, sfr=sfr, metallicity=Z, bhheated=bhheated, sm=sm, dM=dM, dtime=dtime, mass_of_star=mass_of_star, prob=prob,
                    outcome=outcome, cloudfrac=d["cloudfrac"], trelax=d["trelax"], y=d.get("y", math.nan), tcool=d.get("tcool", math.nan), frac=frac, w=w)


def winds_evolve(W, delaytime, density, a3inv, dtime):                 # winds.c:374-391
    if delaytime > 0 and density * a3inv < W["WindFreeTravelDensThresh"]:
        delaytime = 0.0
    if delaytime > 0:
        if delaytime > W["MaxWindFreeTravelTime"]:
            delaytime = W["MaxWindFreeTravelTime"]
        delaytime = max(delaytime - dtime, 0.0)
    return delaytime


COLUMNS_IO = ("entropy", "ne", "sfr", "metallicity", "delaytime", "bhheated")


def cooling_and_starformation(S, d, times, step, rnd, active=None, wind=None, maybewind=True, cool=True, cool_cache=None):
    """the loop of sfr_eff.c:224-272 and the sums of :343-350 over the table `d` (dict of arrays by particle: type (7 = garbage), mass (float32),
    id, generation, density, entropy, ne, sfr, metallicity, delaytime, bhheated, tb_hydro, heiii_ionized, hsml, divvel, curlvel, gradrho_mag).
    `wind`: the wind parameters when there is a delaytime column to evolve.  Returns the new columns, the class and the evaluations per
    particle, the two lists in list order, the four sums and the per-row record of the star-forming rows.  The subgrid winds are not here:
    tests/winds_restated.py has them.  cool False: the rows that do not form stars are classified and left alone.  cool_cache: a dict that
    keeps cooling_direct's result by row across calls on the SAME table, times and step (a cooled row does not depend on the star-formation
    settings)."""
    C, P = S.C, S.p
    n = len(d["type"])
    out = {k: d[k].copy() for k in COLUMNS_IO if d.get(k) is not None}
    out["stellarmass"] = np.zeros(n)
    cls = np.zeros(n, np.uint8)
    evals = np.full(n, -1, np.int32)                # network evaluations of the cooled rows ...
    sfevals = np.full(n, -1, np.int32)              # ... and of the star-forming rows
    redshift = 1. / times["atime"] - 1
    a3inv = 1. / (times["atime"] * times["atime"] * times["atime"])
    hubble = times["hubble"]
    lastred = np.broadcast_to(np.asarray(step.get("lastred", 0.0), np.float64), (47,))
    size = len(rnd)
    get = lambda k, i, default=0: (d[k][i] if d.get(k) is not None else default)
    parents, star_mass, spawn, wind_list, failed, info = [], [], [], [], [], {}
    sum_sm = localsfr = sum_dtime = 0.0
    sum_sf_part = 0
    for p_i in (range(n) if active is None else [int(x) for x in active]):
        if p_i < 0 or p_i >= n:
            continue                                                   # (the engine ignores a list entry outside the table)
        if d["type"][p_i] != 0 or not d["mass"][p_i] > 0:
            continue
        b = min(int(get("tb_hydro", p_i)), 46)
        dloga = float(times["dloga_bin"][b])
        density = float(d["density"][p_i])
        delay = 0.0
        if d.get("delaytime") is not None:
            delay = winds_evolve(wind, float(out["delaytime"][p_i]), density, a3inv, dloga / hubble)
            out["delaytime"][p_i] = delay
        ID = int(d["id"][p_i])
        w, rnd1 = float(rnd[ID % size]), float(rnd[((ID + 1) % (1 << 64)) % size])
        if P["QuickLymanAlphaProbability"] > 0:
            sf = S.quicklyastarformation(density, float(out["entropy"][p_i]), a3inv, rnd1)
        else:
            sf = S.sfreff_on_eeqos(density, delay, a3inv)
        mass = float(d["mass"][p_i])
        if sf:
            cls[p_i] = ROW_STARFORMING
            sum_sf_part += 1
            if P["QuickLymanAlphaProbability"] > 0:
                sum_sm += mass
                parents.append(p_i), star_mass.append(mass), spawn.append(0)
                sfevals[p_i] = 0
                continue
            r = dict(density=density, entropy=float(out["entropy"][p_i]), ne=float(out["ne"][p_i]), metallicity=float(out["metallicity"][p_i]),
                     delaytime=delay, hsml=float(get("hsml", p_i)), divvel=float(get("divvel", p_i)), curlvel=float(get("curlvel", p_i)),
                     gradrho_mag=float(get("gradrho_mag", p_i)), mass=mass, generation=int(get("generation", p_i)), bhheated=int(get("bhheated", p_i)),
                     tb_hydro=b)
            C.evals, C.max_fp = 0, 0
            try:
                o = S.starformation(r, dloga, hubble, redshift, a3inv, step["uvbg"], w, rnd1)
            except R.NotConverged:
                failed.append(p_i)
                sfevals[p_i] = C.evals
                continue
            sfevals[p_i] = C.evals
            o["maxfp"] = C.max_fp
            info[p_i] = o
            out["entropy"][p_i], out["ne"][p_i], out["sfr"][p_i], out["metallicity"][p_i] = o["entropy"], o["ne"], o["sfr"], o["metallicity"]
            if d.get("bhheated") is not None:
                out["bhheated"][p_i] = o["bhheated"]
            sum_sm += o["dM"]
            localsfr += o["sfr"]
            sum_dtime += o["dtime"]
            if o["outcome"] == OUT_NOSTAR:
                if maybewind:
                    wind_list.append(p_i)
                    out["stellarmass"][p_i] = o["sm"]
            else:
                parents.append(p_i), star_mass.append(o["mass_of_star"]), spawn.append(int(o["outcome"] == OUT_SPAWN))
        else:
            cls[p_i] = ROW_COOLED
            if not cool:
                continue
            if cool_cache is not None and p_i in cool_cache:
                got = cool_cache[p_i]
            else:
                Z = float(out["metallicity"][p_i])
                he = int(get("heiii_ionized", p_i))
                C.evals, C.max_fp = 0, 0
                try:
                    e, x, ci = C.cooling_direct(density, float(out["entropy"][p_i]), float(out["ne"][p_i]), Z, he, dloga / hubble, redshift, a3inv,
                                                step["uvbg"], float(lastred[b]), step.get("long_mean_free_path_heating", 0.0))
                    got = (e, x, C.evals)
                except R.NotConverged:
                    got = (None, None, C.evals)
                if cool_cache is not None:
                    cool_cache[p_i] = got
            if got[0] is None:
                failed.append(p_i)
            else:
                out["entropy"][p_i], out["ne"][p_i], out["sfr"][p_i] = got[0], got[1], 0.0
            evals[p_i] = got[2]
    out.update(cls=cls, evals=evals, sfevals=sfevals, parent=np.array(parents, np.int32), mass_of_star=np.array(star_mass, np.float64),
               spawn=np.array(spawn, np.uint8), maybewind=np.array(wind_list, np.int32), sum_sm=sum_sm, localsfr=localsfr, sum_dtime=sum_dtime,
               sum_sf_part=sum_sf_part, failed=failed, info=info)
    return out


# ---- the parameters as init_cooling_and_star_formation derives them (sfr_eff.c:889-1000) ------------------------------------------------------
UNITS = dict(UnitDensity_in_cgs=6.76991e-22, UnitTime_in_s=3.08568e+16, UnitMass_in_g=1.989e+43, UnitLength_in_cm=3.08568e+21,
             HubbleParam=0.7, OmegaBaryon=0.045)          # the unit system of test_cooling.c:179-197
SOLAR_MASS, SEC_PER_YEAR = 1.989e33, 3.155e7              # physconst.h


def no_uvbg():
    """struct UVBG uvbg = {0} (sfr_eff.c:944).  With every photo rate zero the self-shielding factor multiplies nothing; the threshold density
    is set to infinity so that it is not evaluated, where C would divide by a zero density and go on."""
    return dict(R.zero_uvbg(), self_shield_dens=math.inf)


def init_star_formation(C, PhysDensThresh=None, **kw):
    """sfr_params as init_cooling_and_star_formation leaves them, with the defaults of params.c; PhysDensThresh None: computed as :932-958 does"""
    U = UNITS
    Hubble = R.HUBBLE * U["UnitTime_in_s"]
    G = R.GRAVITY / R.pow_(U["UnitLength_in_cm"], 3) * U["UnitMass_in_g"] * R.pow_(U["UnitTime_in_s"], 2)
    RhoCrit = 3 * Hubble * Hubble / (8 * math.pi * G)
    p = dict(StarformationCriterion=CRIT_DENSITY, BoostSFDenseGas=0, BoostSFOverDenseFactor=200.0, FactorSN=0.1, FactorEVP=1000.0, MaxSfrTimescale=1.5,
             Generations=2, BHFeedbackUseTcool=0, QuickLymanAlphaProbability=0.0, QuickLymanAlphaTempThresh=1e5, WindOn=0, UVFluctuationOn=0,
             ExcursionSetReion=0, NTask=1, TempSupernova=1e8, TempClouds=1000.0, CritOverDensity=57.7, avg_baryon_mass=1.0)
    p.update(kw)
    temp_to_u = C.p["temp_to_u"]
    p["UnitSfr_in_solar_per_year"] = (U["UnitMass_in_g"] / SOLAR_MASS) / (U["UnitTime_in_s"] / SEC_PER_YEAR)
    p["tau_fmol_unit"] = U["UnitDensity_in_cgs"] * U["HubbleParam"] * U["UnitLength_in_cm"]
    p["OverDensThresh"] = p["CritOverDensity"] * U["OmegaBaryon"] * RhoCrit
    p["GravInternal"] = G
    meanweight = 4.0 / (1 + 3 * R.HYDROGEN_MASSFRAC)
    p["EgySpecCold"] = (temp_to_u / meanweight) * p["TempClouds"]
    meanweight = 4 / (8 - 5 * (1 - R.HYDROGEN_MASSFRAC))
    p["EgySpecSN"] = temp_to_u / meanweight * p["TempSupernova"]
    p["RhoCrit"] = RhoCrit
    if PhysDensThresh is None:                                          # :932-958
        egyhot = p["EgySpecSN"] / p["FactorEVP"]
        u4 = temp_to_u / meanweight * 1.0e4
        dens = 1.0e6 * RhoCrit
        tcool, _ = C.GetCoolingTime(0, egyhot, dens, no_uvbg(), 1.0, 0.0)
        coolrate = egyhot / tcool / dens
        x = (egyhot - u4) / (egyhot - p["EgySpecCold"])
        PhysDensThresh = x / R.pow_(1 - x, 2) * (p["FactorSN"] * p["EgySpecSN"] - (1 - p["FactorSN"]) * p["EgySpecCold"]) / (p["MaxSfrTimescale"] * coolrate)
        p["u4"] = u4
    p["PhysDensThresh"] = PhysDensThresh
    return p


def get_egyeff(S, redshift, dens, uvbg):                                # :864-878
    P = S.p
    tsfr = math.sqrt(P["PhysDensThresh"] / dens) * P["MaxSfrTimescale"]
    factorEVP = R.pow_(dens / P["PhysDensThresh"], -0.8) * P["FactorEVP"]
    egyhot = P["EgySpecSN"] / (1 + factorEVP) + P["EgySpecCold"]
    tcool, _ = S.C.GetCoolingTime(redshift, egyhot, dens, uvbg, 0.5, 0.0)
    y = div(tsfr, tcool) * egyhot / (P["FactorSN"] * P["EgySpecSN"] - (1 - P["FactorSN"]) * P["EgySpecCold"])
    x = 1 + div(1, 2 * y) - math.sqrt(div(1, y) + div(1, 4 * y * y))
    return egyhot * (1 - x) + P["EgySpecCold"] * x


ENGINE_KEYS = ("StarformationCriterion", "BoostSFDenseGas", "BoostSFOverDenseFactor", "FactorSN", "FactorEVP", "MaxSfrTimescale", "Generations",
               "BHFeedbackUseTcool", "QuickLymanAlphaProbability", "QuickLymanAlphaTempThresh", "EgySpecSN", "EgySpecCold", "PhysDensThresh",
               "OverDensThresh", "UnitSfr_in_solar_per_year", "avg_baryon_mass", "tau_fmol_unit", "GravInternal", "WindOn", "UVFluctuationOn",
               "ExcursionSetReion", "NTask")


def engine_params(p):
    """the members of mpg_sfr_params"""
    return {k: p[k] for k in ENGINE_KEYS}


# ---- the input sets of the tests ---------------------------------------------------------------------------------------------------------------
RND_SIZE = 4093
WIND = dict(WindModel=WIND_SUBGRID | WIND_USE_HALO, WindEfficiency=2.0, WindSigma0=353.0, WindSpeedFactor=3.7, MinWindVelocity=0.0, WindThermalFactor=0.0,
            WindFreeTravelLength=20.0, WindSpeed=0.0, MaxWindFreeTravelTime=0.06, WindFreeTravelDensThresh=0.0)


def random_table(seed=7):
    return np.random.RandomState(seed).uniform(0.0, 1.0, RND_SIZE)


def sample_inputs(n, seed, P, atime):
    """n rows: every 13th no gas, every 17th garbage (type 7), every 19th without mass; of the gas a third below both thresholds, a sixth
    above the physical threshold only by comoving density, the rest 1 .. 1e4 x PhysDensThresh; DelayTime > 0 on every 7th row; BHHeated on every
    5th; hot rows (u > 5e6) on every 11th; every hydro bin including 0; Generation 0 .. 4; masses 0.3 .. 2.5 of the average baryon mass with
    exact 2 x and 1.1 x mass_of_star and their neighbours; metals, Ne guesses with exact zeros; IDs up to 2^64 - 1."""
    rs = np.random.RandomState(seed)
    a3inv = 1. / atime ** 3
    idx = np.arange(n)
    typ = np.zeros(n, np.uint8)
    typ[idx % 13 == 5] = rs.choice([1, 4, 5], size=int((idx % 13 == 5).sum()))
    typ[idx % 17 == 7] = 7
    mos = P["avg_baryon_mass"] / P["Generations"]
    mass = rs.uniform(0.3, 2.5, n).astype(np.float32) * np.float32(P["avg_baryon_mass"])
    special = np.array([2 * mos, np.nextafter(np.float32(2 * mos), np.float32(0)), np.nextafter(np.float32(2 * mos), np.float32(9)), 1.1 * mos, 0.9 * mos,
                        1.5 * mos, 3 * mos], np.float32)
    k = idx % 4 == 2
    mass[k] = special[rs.randint(0, len(special), int(k.sum()))]
    mass[idx % 19 == 11] = rs.choice([0.0, -1.0], size=int((idx % 19 == 11).sum()))
    thr = P["PhysDensThresh"]
    rho = np.exp(rs.uniform(np.log(1.0), np.log(1e4), n)) * thr                     # proper density
    low = idx % 3 == 0
    rho[low] = np.exp(rs.uniform(np.log(1e-6), np.log(0.999), int(low.sum()))) * thr
    density = rho / a3inv
    under = idx % 12 == 4                                                            # above PhysDensThresh, below OverDensThresh: only possible when
    density[under] = np.minimum(density[under], P["OverDensThresh"] * rs.uniform(0.2, 0.999, int(under.sum())))   # the comoving threshold is the higher
    u = np.exp(rs.uniform(np.log(10.0), np.log(3e5), n))
    hot = idx % 11 == 3
    u[hot] = np.exp(rs.uniform(np.log(6e6), np.log(5e7), int(hot.sum())))
    enttou = np.array([R.Cooling.entropy_to_u(float(x), a3inv) for x in density])
    ne = rs.uniform(0.0, 1.2, n)
    ne[idx % 8 == 1] = 0.0
    delay = np.zeros(n)
    wd = idx % 7 == 3
    delay[wd] = rs.uniform(0.0, 0.1, int(wd.sum()))
    ids = rs.randint(0, 2 ** 62, n).astype(np.uint64) * np.uint64(3)
    ids[idx % 29 == 1] = np.uint64(2 ** 64 - 1) - rs.randint(0, 5, int((idx % 29 == 1).sum())).astype(np.uint64)
    return dict(type=typ, mass=mass, id=ids, generation=rs.randint(0, 5, n).astype(np.uint8), density=density, entropy=u / enttou, ne=ne,
                sfr=rs.uniform(0.5, 1.5, n), metallicity=np.where(rs.uniform(size=n) < 0.7, rs.uniform(0.0, 0.04, n), 0.0), delaytime=delay,
                bhheated=(idx % 5 == 2).astype(np.uint8), tb_hydro=rs.randint(0, 47, n).astype(np.uint8),
                heiii_ionized=(rs.uniform(size=n) < 0.5).astype(np.uint8), hsml=np.exp(rs.uniform(np.log(0.5), np.log(50.0), n)),
                divvel=rs.normal(0.0, 30.0, n), curlvel=np.abs(rs.normal(0.0, 30.0, n)),
                gradrho_mag=np.where(rs.uniform(size=n) < 0.9, density / np.exp(rs.uniform(np.log(0.5), np.log(50.0), n)), 0.0),
                vdisp=rs.uniform(20.0, 400.0, n), vel=rs.normal(0.0, 100.0, (n, 3)))


SETTINGS = {
    # name: (members of sfr_params that differ from the defaults, synthetic heating)
    "density": (dict(), False),
    "h2": (dict(StarformationCriterion=CRIT_MOLECULAR_H2), False),
    "selfgravity": (dict(StarformationCriterion=CRIT_CONVERGENT_FLOW | CRIT_CONTINUOUS_CUTOFF), False),
    "selfgravity_plain": (dict(StarformationCriterion=CRIT_SELFGRAVITY | CRIT_MOLECULAR_H2), False),
    "boost": (dict(BoostSFDenseGas=1, BoostSFOverDenseFactor=200.0), False),
    "quicklya": (dict(QuickLymanAlphaProbability=0.7, QuickLymanAlphaTempThresh=1e5), False),
    "heating": (dict(), True),
}
SIZE = 4099


def config(name, treecool_columns, tcool_mode=0, perturb=0.0, ulp=0, **kw):
    """a setting of the tests by name at z = 3, Verner96 / Sherwood with metals: returns (Sfr, times, step, inputs-maker).  The threshold is
    computed once, without perturbation, as the caller of the engine would."""
    C0, times, step, _ = R.config("sherwood_z3", treecool_columns)
    C = R.Cooling(C0.p, C0.tc, C0.metal, perturb)
    over, heating = SETTINGS[name]
    P = init_star_formation(C0, BHFeedbackUseTcool=tcool_mode, **dict(over, **kw))
    if heating:                                                         # a UV background that heats whatever the temperature: tcool = 0
        step = dict(step, uvbg=dict(step["uvbg"], **{k: step["uvbg"][k] * 1e14 for k in ("epsH0", "epsHe0", "epsHep")}))
    S = Sfr(C, P, ulp)
    return S, times, step, (lambda n, P=P, a=times["atime"]: sample_inputs(n, 211, P, a))
