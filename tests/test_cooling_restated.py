"""tests/cooling_restated.py against the reference's own known answers (tests/golden/cooling_kat.npz: the numbers libgadget/tests/
test_cooling.c and test_cooling_rates.c assert, at their tolerances), interp_eval against a brute-force trilinear form, and the
conditions under which the GPU tests (tests/test_gpu_cooling.py) may ask for equal decisions: on the very inputs those tests use, a
relative perturbation of +-2e-15 of every table lookup changes a decision (unew beyond 1e-12 relative, or the number of network
evaluations) for at most 0.1 % of the particles, and the inputs cover the branches the kernel has."""
import math
import os

import numpy as np
import pytest

import cooling_restated as R

HERE = os.path.dirname(os.path.abspath(__file__))
G = np.load(os.path.join(HERE, "golden", "cooling_kat.npz"))

# the table sizes of the GPU tests (tests/test_gpu_cooling.py imports them): one large set, the others a few blocks
SIZES = dict(sherwood_z3=520, sherwood_reion=520, sherwood_z16=4099, kwh_z0=520, badnell_nyx=330)

UV_KEYS = ("epsH0", "epsHe0", "epsHep", "gJH0", "gJHe0", "gJHep", "self_shield_dens")


def units(HubbleParam):
    """the unit system of test_cooling.c:179-197 / test_cooling_rates.c:184-203"""
    UnitDensity_in_cgs, UnitTime_in_s, UnitMass_in_g, UnitLength_in_cm = 6.76991e-22, 3.08568e+16, 1.989e+43, 3.08568e+21
    UnitEnergy_in_cgs = UnitMass_in_g * math.pow(UnitLength_in_cm, 2) / math.pow(UnitTime_in_s, 2)
    return dict(density_in_phys_cgs=UnitDensity_in_cgs * HubbleParam * HubbleParam, uu_in_cgs=UnitEnergy_in_cgs / UnitMass_in_g,
                tt_in_s=UnitTime_in_s / HubbleParam)


def test_uvbg_loader():
    """test_uvbg_loader, test_cooling_rates.c:80-116"""
    C = R.Cooling(R.default_params(), R.TreeCool(G["treecool"]))
    uv = C.get_global_UVBG(16)
    assert uv["epsH0"] == 0 and uv["self_shield_dens"] > 1e8 and uv["gJH0"] == 0
    for z, want in ((0, G["uvbg_z0"]), (3., G["uvbg_z3"])):
        uv = C.get_global_UVBG(z)
        for k, w in zip(UV_KEYS, want):
            assert abs(uv[k] / w - 1) < 1e-5, (z, k)
    # the switch-on redshift is the table's last entry (cooling_rates.c:373), a threshold replaces it and zeroes the rates above it (:375-380)
    assert abs(uv["zreion"] - (10 ** G["treecool"][0][-1] - 1)) < 1e-12
    C2 = R.Cooling(R.default_params(UVRedshiftThreshold=2.5), R.TreeCool(G["treecool"]))
    assert C2.get_global_UVBG(3.)["gJH0"] == 0 and C2.get_global_UVBG(3.)["zreion"] == 2.5 and C2.get_global_UVBG(2.)["gJH0"] > 0
    # during helium reionisation the HeII photo-heating is left to the quasar model (:391-394)
    assert C.get_global_UVBG(3., during_helium_reionization=True)["epsHep"] == 0


def test_docooling_grid():
    """test_DoCooling, test_cooling.c:156-241: the 400-entry tables at 5e-3 and at the rule of line 233"""
    par = R.default_params(recomb=R.Cen92, cooling=R.KWH92, SelfShieldingOn=0, MinGasTemp=0.0,
                           rho_crit_baryon=0.045 * 3.0 * math.pow(0.7 * R.HUBBLE, 2.0) / (8.0 * math.pi * R.GRAVITY))
    C = R.Cooling(par, R.TreeCool(G["treecool"]))
    uvbg = C.get_global_UVBG(0)
    for k, w in zip(UV_KEYS[:3], G["uvbg_z0"][:3]):
        assert abs(uvbg[k] / w - 1) < 1e-5
    meanweight = 4.0 / (1 + 3 * R.HYDROGEN_MASSFRAC)
    MinEgySpec = 1 / meanweight * (1.0 / R.GAMMA_MINUS1) * (R.BOLTZMANN / R.PROTONMASS) * 1 / par["uu_in_cgs"]
    u, rho, want = G["coolingtime_single"]
    tcool, ne = C.GetCoolingTime(0, u, rho, uvbg, 1.0, 0)
    assert abs(tcool / want - 1) < 1e-3
    u, rho, dt, want = G["docooling_single"]
    unew, ne, _ = C.DoCooling(0, u, rho, dt, uvbg, ne, 0, MinEgySpec, 1)
    assert abs(unew / want - 1) < 1e-3
    NSTEP, worst = 20, 0.0
    for i in range(NSTEP):
        dens = math.exp(math.log(1e-9) + i * (math.log(1e-2) - math.log(1e-9)) / 1. / NSTEP)
        for j in range(NSTEP):
            uu = math.exp(math.log(200) + j * (math.log(36000) - math.log(200)) / 1. / NSTEP)
            tcool, _ = C.GetCoolingTime(0, uu, dens, uvbg, 1.0, 0)
            unew, _, _ = C.DoCooling(0, uu, dens, 0.2, uvbg, 1.0, 0, MinEgySpec, 1)
            assert not math.isnan(unew)
            worst = max(worst, abs(unew / G["unew_table"][i * NSTEP + j] - 1))
            tt = G["tcool_table"][i * NSTEP + j]
            assert abs(1 / (1e-20 + tcool) - 1. / (1e-20 + tt)) < 1 or abs((1e-20 + tcool) / (1e-20 + tt) - 1) < 2e-2, (i, j)
    print("DoCooling grid: max |unew / unew_table - 1| = %.2e" % worst)
    assert worst < 5e-3


def test_rate_network():
    """test_rate_network, test_cooling_rates.c:119-170"""
    tc = R.TreeCool(G["treecool"])
    C = R.Cooling(R.default_params(), tc)
    uvbg = C.get_global_UVBG(2)
    for dens, helium, tol in G["equilib_ne"]:
        ne, _ = C.get_equilib_ne(dens, 200. * 1e10, helium, uvbg, 1)
        assert abs(ne / (dens * (1 - helium)) - (1 + 2 * helium / (1 - helium) / 4)) < tol
    temp, ne = C.get_temp(1e-4, 200. * 1e10, 0.24, uvbg, 1.)
    assert G["temp_window"][0] < temp < G["temp_window"][1]
    t4, ne = C.get_temp(1e-4, 400. * 1e10, 0.24, uvbg, ne)
    t2, ne = C.get_temp(1e-4, 200. * 1e10, 0.24, uvbg, ne)
    assert abs(t4 / t2 - 2.) < 1e-3
    t1, ne = C.get_temp(1, 200. * 1e10, 0.24, uvbg, ne)
    assert abs(t1 - 14700) < 200
    for dens in (1e-4, 1e-5, 1e-6):
        nh0, ne = C.get_neutral_fraction_phys_cgs(dens, 200. * 1e10, 0.24, uvbg, ne)
        assert abs(nh0 / dens - float(G["nh0_slope"])) < 1e-3
    nh0, ne = C.get_neutral_fraction_phys_cgs(1, 100., 0.24, uvbg, ne)
    assert nh0 > 0.95
    nh0, ne = C.get_neutral_fraction_phys_cgs(0.1, 100. * 1e10, 0.24, uvbg, ne)
    assert 0.735 < nh0 < 0.75
    C = R.Cooling(R.default_params(SelfShieldingOn=0), tc)
    nh0, ne = C.get_neutral_fraction_phys_cgs(1, 100. * 1e10, 0.24, uvbg, ne)
    assert nh0 < 0.25
    nh0, ne = C.get_neutral_fraction_phys_cgs(0.1, 100. * 1e10, 0.24, uvbg, ne)
    assert nh0 < 0.05


def heatingcooling_cases():
    """the inputs and expected values of test_heatingcooling_rate (test_cooling_rates.c:174-253); shared with the GPU test.  Yields
    (SelfShieldingOn, with_uvbg, density, energy, expectation) in the order of the reference, ne carried from one to the next."""
    U = units(0.697)
    egyhot = 2104.92 * U["uu_in_cgs"]
    dens = 0.027755 * U["density_in_phys_cgs"] / R.PROTONMASS
    return U, egyhot, [(0, False, dens, egyhot, ("tcool", float(G["tcool_kwh"]))), (0, True, dens / 100, egyhot / 10., ("lambda", float(G["lambdanet"][0]))),
                       (0, True, dens / 100 / 2.5, egyhot / 10., ("positive", None)), (1, True, dens / 100 * 1.5, egyhot / 10., ("lambda", float(G["lambdanet"][1])))]


def test_heatingcooling_rate():
    """test_heatingcooling_rate, test_cooling_rates.c:174-253"""
    tc = R.TreeCool(G["treecool"])
    U, egyhot, cases = heatingcooling_cases()
    ne = 1.0
    for ss, with_uvbg, dens, u, (kind, want) in cases:
        C = R.Cooling(R.default_params(recomb=R.Cen92, cooling=R.KWH92, SelfShieldingOn=ss, **U), tc)
        uvbg = C.get_global_UVBG(0) if with_uvbg else R.zero_uvbg()
        assert not with_uvbg or (uvbg["epsHep"] > 0 and uvbg["gJHe0"] > 0)
        LambdaNet, ne = C.get_heatingcooling_rate(dens, u, 1 - R.HYDROGEN_MASSFRAC, 0, 0, uvbg, ne)
        if kind == "tcool":
            assert abs(egyhot / (-LambdaNet) / U["tt_in_s"] / want - 1) < 1e-3
        elif kind == "lambda":
            assert abs(LambdaNet / want - 1) < 1e-3
        else:
            assert LambdaNet > 0


def test_tables_as_init_cooling_rates_fills_them():
    """temp_tab[i] = i log(1e9) / 1000 (cooling_rates.c:1155); inside the table a lookup interpolates, outside it (index < 0 or >= 999) it is the
    function itself (:651-652); the truncation of (int) keeps -1 < dind < 0 inside"""
    for recomb, cooling in ((R.Cen92, R.KWH92), (R.Verner96, R.Sherwood), (R.Badnell06, R.Enzo2Nyx)):
        C = R.Cooling(R.default_params(recomb=recomb, cooling=cooling))
        assert C.temp_tab[0] == 0 and C.temp_tab[999] == 999 * math.log(1e9) / 1000
        for name in C.TABLES:
            assert len(C.tab[name]) == 1000 and all(math.isfinite(x) for x in C.tab[name])   # (the Nyx Gaunt factor turns negative above 1e8.6 K)
            logt = C.temp_tab[500]
            assert C.get_interpolated_recomb(logt, name) == pytest.approx(C.tab[name][500], rel=1e-12)
            mid = 0.5 * (C.temp_tab[500] + C.temp_tab[501])
            assert C.get_interpolated_recomb(mid, name) == pytest.approx(0.5 * (C.tab[name][500] + C.tab[name][501]), rel=1e-9)
            for out in (-0.5, math.log(0.3), C.temp_tab[999] + 1e-9, math.log(3e9)):
                assert C.get_interpolated_recomb(out, name) == C.fn[name](math.exp(out))
            inside = -0.5 * math.log(1e9) / 1000              # dind = -0.5: (int) gives 0, the reference extrapolates from entries 0 and 1
            assert C.get_interpolated_recomb(inside, name) == C.tab[name][1] * (-0.5) + C.tab[name][0] * 1.5


def test_interp_eval_against_brute_force():
    """TableMetalCoolingRate's interp_eval (utils/interp.c:72-131) on the synthetic 3 x 5 x 7 table: inside, on every face, beyond every face"""
    z, nh, t, rate = R.synthetic_metal_table()
    M = R.MetalTable(z, nh, t, rate)
    axes = (z, nh, t)

    def brute(x):
        # clamp to the table (beyond a face: the face's value), then the eight-corner trilinear sum
        idx, w = [], []
        for d in range(3):
            a = axes[d]
            xc = min(max(x[d], a[0]), a[-1])
            s = (xc - a[0]) / ((a[-1] - a[0]) / (len(a) - 1))
            i = min(int(math.floor(s)), len(a) - 2)
            idx.append(i)
            w.append(s - i)
        tot = 0.0
        for c in range(8):
            o = [(c >> d) & 1 for d in range(3)]
            tot += rate[idx[0] + o[0], idx[1] + o[1], idx[2] + o[2]] * np.prod([w[d] if o[d] else 1 - w[d] for d in range(3)])
        return tot

    rs = np.random.RandomState(4)
    pts = [[rs.uniform(a[0], a[-1]) for a in axes] for _ in range(200)]
    for d in range(3):                                       # on and beyond both faces of every axis, the other coordinates anywhere
        for v in (axes[d][0], axes[d][-1], axes[d][0] - 0.7, axes[d][-1] + 0.7, axes[d][1], axes[d][-2]):
            for _ in range(8):
                x = [rs.uniform(a[0] - 0.5, a[-1] + 0.5) for a in axes]
                x[d] = v
                pts.append(x)
    pts += [[a[0] - 1 for a in axes], [a[-1] + 1 for a in axes], [a[0] for a in axes], [a[-1] for a in axes]]
    for x in pts:
        assert M.interp_eval(x) == pytest.approx(brute(x), rel=1e-13), x
    # through TableMetalCoolingRate: log10 of density and temperature
    C = R.Cooling(R.default_params(), None, M)
    assert C.TableMetalCoolingRate(1.3, 10 ** 4.4, 10 ** -3.3) == pytest.approx(brute([1.3, -3.3, 4.4]), rel=1e-13)
    assert R.Cooling(R.default_params()).TableMetalCoolingRate(1.3, 1e4, 1e-3) == 0


_base = {}


def base_run(name):
    """the unperturbed restatement of a setting's input set (shared with nothing else: the GPU tests compute their own on the GPU box)"""
    if name not in _base:
        C, times, step, make = R.config(name, G["treecool"])
        d = make(SIZES[name])
        _base[name] = (C, times, step, d, R.cool_particles(C, d, times, step))
    return _base[name]


@pytest.mark.parametrize("name", R.CONFIGS)
def test_decisions_are_stable_on_the_gpu_tests_inputs(name):
    """every table lookup perturbed by +-2e-15 relative: at most 0.1 % of the particles change a decision; nothing fails to converge"""
    C, times, step, d, base = base_run(name)
    assert not base["failed"]
    treated = base["evals"] >= 0
    changed = np.zeros(len(treated), bool)
    dne = 0.0
    for eps in (2e-15, -2e-15):
        Cp = R.config(name, G["treecool"], perturb=eps)[0]
        r = R.cool_particles(Cp, d, times, step)
        assert not r["failed"]
        changed |= r["evals"] != base["evals"]
        changed[treated] |= np.abs(r["entropy"][treated] / base["entropy"][treated] - 1) > 1e-12
        same = treated & ~changed
        dne = max(dne, float(np.abs(r["ne"][same] - base["ne"][same]).max()))
    print("stability %s: %d of %d particles change a decision; max |dNe| of the others %.1e" % (name, changed.sum(), treated.sum(), dne))
    assert changed.sum() <= 1e-3 * treated.sum()
    assert dne < 1e-12


def test_input_sets_cover_the_branches():
    """what the issue asks the input sets to include, read off the restatement's own record of each particle"""
    def info(name):
        C, times, step, d, base = base_run(name)
        gas = np.array(sorted(base["info"]))
        return C, times, step, d, base, gas

    # skipped rows: non-gas, garbage, massless
    C, times, step, d, base, gas = info("sherwood_z3")
    skipped = base["evals"] < 0
    assert ((d["type"] != 0) | ~(d["mass"] > 0) == skipped).all() and (d["type"][skipped] == 7).any() and (d["mass"][skipped] <= 0).any()
    # heated and cooled particles, an Ne guess of 0, both HeIIIionized with long-mean-free-path heating, HeliumHeatOn, metals
    uold = d["entropy"][gas] * np.array([C.entropy_to_u(float(x), 1 / times["atime"] ** 3) for x in d["density"][gas]])
    unew = np.array([base["info"][i]["unew"] for i in gas])
    assert (unew > uold * 1.001).sum() > 20 and (unew < uold * 0.999).sum() > 20
    assert (d["ne"][gas] == 0).sum() > 20
    assert step["long_mean_free_path_heating"] > 0 and set(d["heiii_ionized"][gas]) == {0, 1} and C.p["HeliumHeatOn"] == 1
    assert C.metal is not None and (d["metallicity"][gas] > 0).sum() > 100 and (d["metallicity"][gas] == 0).sum() > 50
    # densities on both sides of 0.01 self_shield_dens
    nh = d["density"][gas] / times["atime"] ** 3 * C.p["density_in_phys_cgs"] / R.PROTONMASS * R.HYDROGEN_MASSFRAC
    ss = 0.01 * step["uvbg"]["self_shield_dens"]
    assert (nh < ss).sum() > 50 and (nh > ss).sum() > 50
    # the energy floor: reached from above, and an entry below it
    floor = sum(base["info"][i]["floor"] for i in gas)
    C16, times16, step16, d16, base16, gas16 = info("sherwood_z16")
    floor16 = sum(base16["info"][i]["floor"] for i in gas16)
    print("floor: %d (sherwood_z3), %d (sherwood_z16)" % (floor, floor16))
    assert floor + floor16 > 20
    mes = C16.p["temp_to_u"] / (4.0 / (1 + 3 * R.HYDROGEN_MASSFRAC)) * C16.p["sfr_MinGasTemp"]
    u16 = d16["entropy"][gas16] * np.array([C16.entropy_to_u(float(x), 1 / times16["atime"] ** 3) for x in d16["density"][gas16]])
    assert (u16 < mes).sum() > 5
    assert step16["uvbg"]["gJH0"] == 0                                   # z above the table
    # T outside the table on both sides (no temperature floors)
    Ck, timesk, stepk, dk, basek, gask = info("kwh_z0")
    assert Ck.p["MinGasTemp"] == 0 and Ck.p["sfr_MinGasTemp"] == 0
    uk = dk["entropy"][gask] * np.array([Ck.entropy_to_u(float(x), 1.0) for x in dk["density"][gask]]) * Ck.p["uu_in_cgs"]
    tk_lo = np.array([Ck.get_temp_internal(1.2, float(x), 0.24) for x in uk])      # the highest temperature an energy can mean ...
    tk_hi = np.array([Ck.get_temp_internal(0.0, float(x), 0.24) for x in uk])      # ... and the lowest
    assert (tk_hi < 1).sum() > 5 and (tk_lo > 1e9).sum() > 5
    # the HIReionTemp branch: taken by the bins whose step began before zreion, with particles hotter and colder than HIReionTemp
    Cr, timesr, stepr, dr, baser, gasr = info("sherwood_reion")
    reion = [i for i in gasr if baser["info"][i]["reion"]]
    assert len(reion) > 50 and len(reion) < len(gasr) - 50
    assert all(dr["tb_hydro"][i] % 2 == 0 for i in reion)
    ureion = Cr.p["temp_to_u"] / (4 / (8 - 6 * (1 - R.HYDROGEN_MASSFRAC))) * Cr.p["HIReionTemp"]
    kept = [i for i in reion if baser["info"][i]["unew"] > ureion]
    assert len(kept) > 10 and len(reion) - len(kept) > 10
    assert all(baser["evals"][i] == 0 and baser["ne"][i] == dr["ne"][i] for i in reion)
    # the spread of the cost
    ev = np.concatenate([base_run(nm)[4]["evals"] for nm in R.CONFIGS])
    ev = ev[ev > 0]
    print("evaluations per particle: min %d, median %d, max %d" % (ev.min(), np.median(ev), ev.max()))
    assert ev.min() >= 3 and ev.max() > 10 * np.median(ev)
