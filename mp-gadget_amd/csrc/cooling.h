// cooling.h -- radiative cooling of gas: the ionisation network (libgadget/cooling_rates.c), DoCooling (cooling.c:57-138) and
// cooling_direct (sfr_eff.c:463-514).  The solver is written once for host and device on top of cooling_rates.h; cooling.hip holds the
// kernels and the engine's state.
#pragma once
#include "../../include/mpgadget_hip.h"
#include "cooling_rates.h"
#include "mpg_common.h"
#include <vector>

namespace mpg {
namespace cool {

constexpr int NET_MAXITER = 1000;    // MAXITER, cooling_rates.c:768
constexpr int COOL_MAXITER = 1000;   // MAXITER, cooling.c:32
constexpr int BRACKET_MAXITER = 8192; // the two bracketing loops of DoCooling have no bound in the reference

// what the solver reads besides the particle: the parameters, the step and the tables (pointers valid where the solver runs)
struct Setup {
    int recomb, cooling, SelfShieldingOn, HeliumHeatOn, CoolingOn;
    int net_maxiter; // NET_MAXITER, or the test-only limit of mpg_cooling_params
    double CMBTemperature, MinGasTemp, HeliumHeatThresh, HeliumHeatAmp, HeliumHeatExp, rho_crit_baryon;
    double density_in_phys_cgs, uu_in_cgs, tt_in_s, units_rho_crit_baryon;
    double sfr_MinGasTemp, temp_to_u, HIReionTemp;
    double tmax; // RECOMBTMAX = log(1e9), as the host's log gives it
    mpg_uvbg uvbg;
    double redshift, lmfp_heating;
    const double *net;  // [NRECOMBTAB][NNET]
    const double *ctab; // [NRECOMBTAB][NCOOL_PAD]
    // metal cooling table (cooling_uvfluc.c:249-322), or metal == nullptr
    const double *metal;
    int mdim[3];
    double mmin[3], mmax[3], mstep[3];
};

// the UV-fluctuation table as a kernel reads it: Zreion_Table[Nside][Nside][Nside] in C order, interp_init_dim(d, 0, BoxSize) on every axis
// (cooling_uvfluc.c:158-162), PartManager->CurrentParticleOffset
struct UvfView {
    const double *table;
    long long nside;
    double step; // BoxSize / (Nside - 1), utils/interp.c:53
    double off[3];
};

// interp_eval_periodic (utils/interp.c:134-170) at pos - off: the cell and the fraction per axis, the eight corners wrapped into
// [0, Nside), the sum in the reference's corner order (bit d of the corner number selects axis d).  The table wraps after Nside cells of
// width BoxSize / (Nside - 1), as the reference's does.  The wrap is an integer modulo where the reference loops; the two agree for every
// finite cell below 2^31 in magnitude.  A coordinate that is not finite or lies beyond that range (the reference: undefined) gives NaN
// without reading the table.
MPG_HD double uvf_zreion(const UvfView &U, const double *pos)
{
    long long xi[3];
    double f[3];
    for(int d = 0; d < 3; d++) {
        const double xd = (pos[d] - U.off[d]) / U.step;
        if(!(fabs(xd) < 2147483648.0)) // (false for NaN too)
            return NAN;
        const double fl = floor(xd);
        xi[d] = (long long)fl;
        f[d] = xd - fl;
    }
    const long long stride[3] = {U.nside * U.nside, U.nside, 1};
    double ret = 0;
    for(int i = 0; i < 8; i++) {
        double filter = 1.0;
        long long l = 0;
        for(int d = 0; d < 3; d++) {
            const int foffset = (i & (1 << d)) ? 1 : 0;
            long long c = (xi[d] + foffset) % U.nside;
            if(c < 0)
                c += U.nside;
            filter *= foffset ? f[d] : (1 - f[d]);
            l += stride[d] * c;
        }
        ret += U.table[l] * filter;
    }
    return ret;
}

// get_local_UVBG_from_global (cooling_uvfluc.c:174-197) with the table's value at the particle: before its own reionisation every rate
// is zero and self_shield_dens the global one, afterwards the global background; uvbg.zreion is the local value either way.  Only the
// members of uvbg differ between the lanes of a wave; everything else of the copy stays what the kernel was given.
MPG_HD Setup dark_setup(const Setup &S, bool dark)
{
    Setup L = S;
    if(dark) {
        L.uvbg.J_UV = 0;
        L.uvbg.gJH0 = 0;
        L.uvbg.gJHep = 0;
        L.uvbg.gJHe0 = 0;
        L.uvbg.epsH0 = 0;
        L.uvbg.epsHep = 0;
        L.uvbg.epsHe0 = 0;
    }
    return L;
}
MPG_HD Setup local_setup(const Setup &S, double zreion)
{
    Setup L = dark_setup(S, zreion < S.redshift);
    L.uvbg.zreion = zreion;
    return L;
}

// the excursion set's model as a kernel reads it: get_J21_coeffs(AlphaUV) (the four members get_local_UVBG_from_J21 reads) and the two
// factors of get_self_shield_dens at the call's redshift
struct J21View {
    double gJH0, gJHe0, epsH0, epsHe0;
    SelfShieldFactors ss;
};
// a row of the two columns that has no background: J21 NaN or negative, zreion NaN
MPG_HD bool j21_row_bad(double J21, double zreion) { return !(J21 >= 0) || zreion != zreion; }
// get_local_UVBG_from_J21, cooling_uvfluc.c:199-231: the rates, each the reference's products in the reference's order ...
MPG_HD void j21_rates(mpg_uvbg &u, const J21View &X, double J21)
{
    u.J_UV = J21;
    u.gJH0 = X.gJH0 * J21;
    u.epsH0 = X.epsH0 * J21 * 1.60218e-12;
    u.gJHe0 = X.gJHe0 * J21;
    u.epsHe0 = X.epsHe0 * J21 * 1.60218e-12;
    u.gJHep = 0.;
    u.epsHep = 0.;
}
// ... and the whole background of a row.  As in dark_setup only the members of uvbg differ between the lanes of a wave.
MPG_HD Setup j21_setup(const Setup &S, const J21View &X, double J21, double zreion)
{
    Setup L = S;
    j21_rates(L.uvbg, X, J21);
    L.uvbg.zreion = zreion;
    L.uvbg.self_shield_dens = self_shield_dens(X.ss, L.uvbg.gJH0);
    return L;
}
// ... rebuilt from the two numbers a lane of the queue form keeps across its evaluations (zreion is read before the first of them only)
MPG_HD Setup j21_lane_setup(const Setup &S, const J21View &X, double J21, double ssdens)
{
    Setup L = S;
    j21_rates(L.uvbg, X, J21);
    L.uvbg.self_shield_dens = ssdens;
    return L;
}

struct Counters {
    int evals = 0;      // ne_internal evaluations
    int bisections = 0; // steps of DoCooling's bisection
    int floor = 0;      // ended on MinEgySpec
    int error = 0;      // an iteration limit was hit or ne is not finite
};

// where a table lookup falls: the index and weight of get_interpolated_recomb (cooling_rates.c:648-655), index -1 = call the function
struct TabPos {
    int index;
    double w;
};
MPG_HD TabPos tab_pos(double logt, double tmax)
{
    const double dind = (logt - 0) / (tmax - 0) * NRECOMBTAB;
    TabPos p;
    // (int) truncates towards zero, as in the reference; a dind outside int's range (or NaN) is outside the table
    if(!(dind > -1.0 && dind < (double)(NRECOMBTAB - 1))) {
        p.index = -1;
        p.w = 0;
        return p;
    }
    p.index = (int)dind;
    p.w = dind - p.index;
    return p;
}
MPG_HD double net_lookup(const Setup &S, const TabPos &p, double logt, int k)
{
    if(p.index < 0)
        return net_fit(k, exp(logt), S.recomb);
    return S.net[(p.index + 1) * NNET + k] * p.w + S.net[p.index * NNET + k] * (1 - p.w);
}
MPG_HD double cool_lookup(const Setup &S, const TabPos &p, double logt, int k)
{
    if(p.index < 0)
        return cool_fit(k, exp(logt), S.recomb, S.cooling);
    return S.ctab[(p.index + 1) * NCOOL_PAD + k] * p.w + S.ctab[p.index * NCOOL_PAD + k] * (1 - p.w);
}

// self_shield_corr, cooling_rates.c:438-450
MPG_HD double self_shield_corr(const Setup &S, double nh, double logt, double ssdens)
{
    if(!S.SelfShieldingOn || nh < ssdens * 0.01)
        return 1;
    const double T4 = exp(0.17 * (logt - log(1e4)));
    const double nSSh = 1.003 * ssdens * T4;
    return 0.98 * pow(1 + pow(nh / nSSh, 1.64), -2.28) + 0.02 * pow(1 + nh / nSSh, -0.84);
}

// nH0_internal, cooling_rates.c:660-670
MPG_HD double nH0_internal(const Setup &S, const TabPos &p, double logt, double ne, double photofac)
{
    const double alphaHp = net_lookup(S, p, logt, T_alphaHp);
    const double GammaeH0 = net_lookup(S, p, logt, T_GammaH0);
    double photorate = 0;
    if(S.uvbg.gJH0 > 0. && ne > 1e-50)
        photorate = S.uvbg.gJH0 / ne * photofac;
    return alphaHp / (alphaHp + GammaeH0 + photorate);
}

struct HeIons {
    double nHe0, nHep, nHepp;
};
// nHe_internal, cooling_rates.c:690-715
MPG_HD HeIons nHe_internal(const Setup &S, const TabPos &p, double nh, double logt, double ne, double photofac)
{
    const double alphaHep = net_lookup(S, p, logt, T_alphaHep);
    const double alphaHepp = net_lookup(S, p, logt, T_alphaHepp);
    double GammaHe0 = net_lookup(S, p, logt, T_GammaHe0);
    double GammaHep = net_lookup(S, p, logt, T_GammaHep);
    HeIons He;
    if(S.uvbg.gJHe0 > 0. && ne > 1e-50) {
        GammaHe0 += S.uvbg.gJHe0 / ne * photofac;
        GammaHep += S.uvbg.gJHep / ne * photofac;
    }
    if(GammaHe0 > 1e-50) {
        He.nHep = nh / (1 + alphaHep / GammaHe0 + GammaHep / alphaHepp);
        He.nHe0 = He.nHep * alphaHep / GammaHe0;
        He.nHepp = He.nHep * GammaHep / alphaHepp;
    }
    else {
        He.nHep = 0;
        He.nHe0 = nh;
        He.nHepp = 0;
    }
    return He;
}

// get_temp_internal, cooling_rates.c:735-752
MPG_HD double get_temp_internal(const Setup &S, double nebynh, double ienergy, double helium)
{
    const double hy_mass = 1 - helium;
    const double muienergy = 4 / (hy_mass * (3 + 4 * nebynh) + 1) * ienergy;
    const double temp = GAMMA_MINUS1 * PROTONMASS / BOLTZMANN * muienergy;
    if(temp < S.MinGasTemp)
        return S.MinGasTemp;
    return temp;
}

// ne_internal, cooling_rates.c:755-765
MPG_HD double ne_internal(const Setup &S, double nh, double ienergy, double ne, double helium, double *logt, Counters &C)
{
    C.evals++;
    const double yy = helium / 4 / (1 - helium);
    *logt = log(get_temp_internal(S, ne / nh, ienergy, helium));
    const TabPos p = tab_pos(*logt, S.tmax);
    const double photofac = self_shield_corr(S, nh, *logt, S.uvbg.self_shield_dens);
    const double nH0 = nH0_internal(S, p, *logt, ne, photofac);
    double nHp = 1. - nH0; // nHp_internal, :673-680
    if(nHp < 0)
        nHp = 0;
    const HeIons He = nHe_internal(S, p, nh, *logt, ne, photofac);
    return nh * nHp + yy * He.nHep + 2 * yy * He.nHepp;
}

// get_equilib_ne with scipy_optimize_fixed_point, cooling_rates.c:779-827
MPG_HD double get_equilib_ne(const Setup &S, double density, double ienergy, double helium, double *logt, double ne_init, Counters &C)
{
    const double nh = density * (1 - helium);
    if(ne_init <= 0)
        ne_init = 1.0;
    double ne0 = ne_init;
    int i;
    for(i = 0; i < S.net_maxiter; i++) {
        double logt1;
        const double ne1 = ne_internal(S, nh, ienergy, ne0 * nh, helium, &logt1, C) / nh;
        if(fabs(ne1 - ne0) < 1e-6) { // ITERCONV
            *logt = logt1;
            ne0 = ne1;
            break;
        }
        const double ne2 = ne_internal(S, nh, ienergy, ne1 * nh, helium, &logt1, C) / nh;
        const double d = ne0 + ne2 - 2.0 * ne1;
        double pp = ne2;
        if(d > 1e-15 || d < -1e-15)
            pp = ne0 - (ne1 - ne0) * (ne1 - ne0) / d;
        ne0 = pp;
        if(ne0 < 0)
            ne0 = 0;
    }
    // the reference's endrun(1, "Ionization rate network failed to converge"); ne0 - ne0 is 0 for a finite ne0 and NaN otherwise
    if(!(ne0 - ne0 == 0) || i == S.net_maxiter)
        C.error = 1;
    return ne0 * nh;
}

// cool_InverseCompton, cooling_rates.c:1044-1049
MPG_HD double cool_InverseCompton(const Setup &S, double temp, double redshift)
{
    const double tcmb_red = S.CMBTemperature * (1 + redshift);
    return 4 * THOMPSON * RAD_CONST / (ELECTRONMASS * LIGHTCGS) * pow(tcmb_red, 4.0) * BOLTZMANN * (temp - tcmb_red);
}

// cool_he_reion_factor, cooling_rates.c:1058-1068
MPG_HD double cool_he_reion_factor(const Setup &S, double nHcgs, double helium, double redshift)
{
    if(!S.HeliumHeatOn)
        return 1.;
    const double rho = PROTONMASS * nHcgs / (1 - helium);
    double overden = rho / (S.rho_crit_baryon * pow(1 + redshift, 3.0));
    if(overden >= S.HeliumHeatThresh)
        overden = S.HeliumHeatThresh;
    return S.HeliumHeatAmp * pow(overden, S.HeliumHeatExp);
}

// TableMetalCoolingRate (cooling_uvfluc.c:307-322) through interp_eval (utils/interp.c:72-131): outside a face the face's value, a
// second point only where its weight is not zero.  One departure: a coordinate inside [Min, Max] whose rounded position reaches the last
// point gets weight 0 there, where the reference would read one element past the table with a weight of a few ulp.
MPG_HD double metal_cooling_rate(const Setup &S, double redshift, double temp, double nHcgs)
{
    if(!S.metal)
        return 0;
    const double x[3] = {redshift, log10(nHcgs), log10(temp)};
    int xi[3];
    double f[3];
    for(int d = 0; d < 3; d++) {
        const double xd = (x[d] - S.mmin[d]) / S.mstep[d];
        if(x[d] < S.mmin[d]) {
            xi[d] = 0;
            f[d] = 0;
        }
        else if(x[d] > S.mmax[d]) {
            xi[d] = S.mdim[d] - 1;
            f[d] = 0;
        }
        else if(xd == xd) {
            xi[d] = (int)floor(xd);
            f[d] = xd - xi[d];
            if(xi[d] >= S.mdim[d] - 1) {
                xi[d] = S.mdim[d] - 1;
                f[d] = 0;
            }
        }
        else { // NaN: no table value
            return xd;
        }
    }
    const long long stride[3] = {(long long)S.mdim[1] * S.mdim[2], (long long)S.mdim[2], 1};
    const long long l0 = stride[0] * xi[0] + stride[1] * xi[1] + stride[2] * xi[2];
    double ret = 0;
    for(int i = 0; i < 8; i++) {
        double filter = 1.0;
        long long l = l0;
        bool skip = false;
        for(int d = 0; d < 3; d++) {
            const int foffset = (i & (1 << d)) ? 1 : 0;
            if(f[d] == 0 && foffset == 1) {
                skip = true;
                break;
            }
            filter *= foffset ? f[d] : (1 - f[d]);
            l += foffset * stride[d];
        }
        if(!skip)
            ret += S.metal[l] * filter;
    }
    return ret;
}

// the abundances and the temperature at the equilibrium of one (density, energy): what get_heatingcooling_rate and the accessors share
struct NetState {
    double nebynh, temp, logt, nH0;
};

// get_heatingcooling_rate, cooling_rates.c:1248-1310
// ... its part after get_equilib_ne (:1253-1309): the rates at the equilibrium ne (cgs) and logt
MPG_HD double heatingcooling_at_equilibrium(const Setup &S, double density, double ienergy, double helium, double redshift, double metallicity,
                                            double ne, double logt, double *ne_equilib, NetState *out = nullptr)
{
    const double nh = density * (1 - helium);
    const double nebynh = ne / nh;
    const double temp = get_temp_internal(S, nebynh, ienergy, helium);
    const double photofac = self_shield_corr(S, nh, logt, S.uvbg.self_shield_dens);
    const double yy = helium / 4 / (1 - helium);
    const TabPos p = tab_pos(logt, S.tmax);
    const double nH0 = nH0_internal(S, p, logt, ne, photofac);
    double nHp = 1. - nH0;
    if(nHp < 0)
        nHp = 0;
    HeIons He = nHe_internal(S, p, nh, logt, ne, photofac);
    He.nHep *= yy / nh;
    He.nHe0 *= yy / nh;
    He.nHepp *= yy / nh;
    const double LambdaCollis = nebynh * (cool_lookup(S, p, logt, T_collisH0) * nH0 + cool_lookup(S, p, logt, T_collisHe0) * He.nHe0 +
                                          cool_lookup(S, p, logt, T_collisHeP) * He.nHep);
    const double LambdaRecomb = nebynh * (cool_lookup(S, p, logt, T_recombHp) * nHp + cool_lookup(S, p, logt, T_recombHeP) * He.nHep +
                                          cool_lookup(S, p, logt, T_recombHePP) * He.nHepp);
    double LambdaFF = 0;
    const double cff = cool_lookup(S, p, logt, T_freefree1);
    if(S.cooling == Enzo2Nyx)
        LambdaFF = nebynh * (cff * (nHp + He.nHep) + cool_FreeFree(temp, 2, S.cooling) * He.nHepp);
    else
        LambdaFF = nebynh * (cff * (nHp + He.nHep) + 4 * cff * He.nHepp);
    const double LambdaCmptn = nebynh * cool_InverseCompton(S, temp, redshift) / nh;
    const double Lambda = LambdaCollis + LambdaRecomb + LambdaFF + LambdaCmptn;
    double Heat = (nH0 * S.uvbg.epsH0 + He.nHe0 * S.uvbg.epsHe0 + He.nHep * S.uvbg.epsHep) / nh;
    Heat *= cool_he_reion_factor(S, density, helium, redshift);
    *ne_equilib = nebynh;
    // (the reference multiplies a zero metallicity into the table value; the product is the same without the lookup unless that
    //  value is not finite, which a table of finite entries cannot give)
    const double MetalCooling = metallicity != 0 ? metallicity * metal_cooling_rate(S, redshift, temp, nh) : 0.0;
    const double LambdaNet = Heat - Lambda - MetalCooling;
    if(out) {
        out->nebynh = nebynh;
        out->temp = temp;
        out->logt = logt;
        out->nH0 = nH0;
    }
    return LambdaNet * pow(1 - helium, 2.0) * density / PROTONMASS;
}
MPG_HD double get_heatingcooling_rate(const Setup &S, double density, double ienergy, double helium, double redshift, double metallicity,
                                      double *ne_equilib, Counters &C, NetState *out = nullptr)
{
    double logt;
    const double ne = get_equilib_ne(S, density, ienergy, helium, &logt, *ne_equilib, C);
    return heatingcooling_at_equilibrium(S, density, ienergy, helium, redshift, metallicity, ne, logt, ne_equilib, out);
}

// get_lambdanet, cooling.c:42-52
MPG_HD double get_lambdanet(const Setup &S, double rho, double u, double redshift, double Z, double *ne_guess, int isHeIIIionized, Counters &C)
{
    double LambdaNet = get_heatingcooling_rate(S, rho, u, 1 - HYDROGEN_MASSFRAC, redshift, Z, ne_guess, C);
    if(!isHeIIIionized)
        LambdaNet += S.lmfp_heating / (S.units_rho_crit_baryon * pow(1 + redshift, 3.0));
    return LambdaNet;
}

// GetCoolingTime, cooling.c:143-163: code units in and out, rho the proper density; one get_heatingcooling_rate WITHOUT the
// long-mean-free-path term; 0 for net heating
MPG_HD double get_cooling_time(const Setup &S, double redshift, double u_old, double rho, double *ne_guess, double Z, Counters &C)
{
    if(!S.CoolingOn)
        return 0;
    rho *= S.density_in_phys_cgs / PROTONMASS;
    u_old *= S.uu_in_cgs;
    const double LambdaNet = get_heatingcooling_rate(S, rho, u_old, 1 - HYDROGEN_MASSFRAC, redshift, Z, ne_guess, C);
    if(LambdaNet >= 0)
        return 0;
    double coolingtime = u_old / (-LambdaNet);
    coolingtime /= S.tt_in_s;
    return coolingtime;
}

// DoCooling, cooling.c:57-138.  Code units in and out; rho is the proper density.
MPG_HD double do_cooling(const Setup &S, double redshift, double u_old, double rho, double dt, double *ne_guess, double Z, double MinEgySpec,
                         int isHeIIIionized, Counters &C)
{
    if(!S.CoolingOn)
        return 0;
    double u, du;
    double u_lower, u_upper;
    double LambdaNet;
    int iter = 0;

    rho *= S.density_in_phys_cgs / PROTONMASS;
    u_old *= S.uu_in_cgs;
    MinEgySpec *= S.uu_in_cgs;
    if(u_old < MinEgySpec)
        u_old = MinEgySpec;
    dt *= S.tt_in_s;

    u = u_old;
    u_lower = u;
    u_upper = u;

    LambdaNet = get_lambdanet(S, rho, u, redshift, Z, ne_guess, isHeIIIionized, C);

    int guard = 0;
    if(u - u_old - LambdaNet * dt < 0) { /* heating */
        do {
            u_lower = u_upper;
            u_upper *= 1.1;
            if(++guard > BRACKET_MAXITER || C.error) {
                C.error = 1;
                return 0;
            }
        } while(u_upper - u_old - get_lambdanet(S, rho, u_upper, redshift, Z, ne_guess, isHeIIIionized, C) * dt < 0);
    }
    else {
        do {
            u_upper = u_lower;
            u_lower /= 1.1;
            if(u_upper <= MinEgySpec)
                break;
            if(++guard > BRACKET_MAXITER || C.error) {
                C.error = 1;
                return 0;
            }
        } while(u_lower - u_old - get_lambdanet(S, rho, u_lower, redshift, Z, ne_guess, isHeIIIionized, C) * dt > 0);
    }

    do {
        u = 0.5 * (u_lower + u_upper);
        if(u_upper <= MinEgySpec) {
            u = MinEgySpec;
            C.floor = 1;
            break;
        }
        LambdaNet = get_lambdanet(S, rho, u, redshift, Z, ne_guess, isHeIIIionized, C);
        if(u - u_old - LambdaNet * dt > 0)
            u_upper = u;
        else
            u_lower = u;
        du = u_upper - u_lower;
        iter++;
        C.bisections++;
    } while(fabs(du / u) > 1.0e-6 && iter < COOL_MAXITER && !C.error);

    if(iter >= COOL_MAXITER) // the reference's endrun(10, "failed to converge in DoCooling()")
        C.error = 1;
    u /= S.uu_in_cgs;
    return u;
}

// entropy_to_u, sfr_eff.c:138-142
MPG_HD double entropy_to_u(double density, double a3inv) { return exp(GAMMA_MINUS1 * log(density * a3inv)) / GAMMA_MINUS1; }

// cooling_direct, sfr_eff.c:463-514, for one particle; the UV background is S's: the step's, or with a fluctuation table the particle's own
// (local_setup), or with the excursion set's columns the one of its J21 (j21_setup).
// Returns the new entropy; *ne holds SphP.Ne in and out; *reion tells whether the HIReionTemp branch was taken.
MPG_HD double cooling_direct(const Setup &S, double density, double entropy, double *ne, double Z, int heiii, double dtime, double a3inv,
                             double lastred, Counters &C, int *reion)
{
    const double enttou = entropy_to_u(density, a3inv);
    const double uold = entropy * enttou;
    double unew;
    *reion = 0;
    if(S.HIReionTemp > 0 && S.uvbg.zreion >= S.redshift && S.uvbg.zreion < lastred) {
        const double meanweight = 4 / (8 - 6 * (1 - HYDROGEN_MASSFRAC));
        unew = S.temp_to_u / meanweight * S.HIReionTemp;
        if(uold > unew)
            unew = uold;
        *reion = 1;
    }
    else {
        const double meanweight = 4.0 / (1 + 3 * HYDROGEN_MASSFRAC);
        const double MinEgySpec = S.temp_to_u / meanweight * S.sfr_MinGasTemp;
        unew = do_cooling(S, S.redshift, uold, density * a3inv, dtime, ne, Z, MinEgySpec, heiii, C);
    }
    return unew / enttou;
}

// the 13 tables as init_cooling_rates fills them (cooling_rates.c:1153-1171), interleaved per temperature bin
inline void fill_tables(int recomb, int cooling, std::vector<double> &net, std::vector<double> &ctab)
{
    net.assign((size_t)NRECOMBTAB * NNET, 0.0);
    ctab.assign((size_t)NRECOMBTAB * NCOOL_PAD, 0.0);
    const double tmax = log(1e9);
    for(int i = 0; i < NRECOMBTAB; i++) {
        const double tt = exp(0 + (tmax - 0) * i / NRECOMBTAB);
        for(int k = 0; k < NNET; k++)
            net[(size_t)i * NNET + k] = net_fit(k, tt, recomb);
        for(int k = 0; k < NCOOL; k++)
            ctab[(size_t)i * NCOOL_PAD + k] = cool_fit(k, tt, recomb, cooling);
    }
}

} // namespace cool

// the engine's cooling state: parameters, tables on the device, the counters and per-particle evaluation counts of the last call
struct CoolingEngine {
    bool have_params = false;
    mpg_cooling_params par{};
    DevBuf<double> net, ctab, metal;
    int mdim[3] = {0, 0, 0};
    double mmin[3] = {0, 0, 0}, mmax[3] = {0, 0, 0};
    bool have_metal = false;
    DevBuf<unsigned long long> d_stats;
    DevBuf<int> d_evals;
    int64_t n_evals = 0; // particles d_evals was last written for
    int64_t stats[6] = {0, 0, 0, 0, 0, 0};
    int lds_tables = 0; // 1: the six network tables in LDS (MPG_COOLING_LDS), 0: in global memory
    int num_cus = 0;
    int form = 0;       // 0: one particle per lane to completion, 1: per-lane state machine with a wave-aggregated queue (MPG_COOLING_FORM)
    // the UV-fluctuation table (init_uvf_table, cooling_uvfluc.c:115-167) and the zreion column of the last call (NaN: row not evaluated)
    bool have_uvf = false;
    DevBuf<double> uvf_table, uvf_z;
    DevBuf<unsigned> uvf_bad;
    int64_t uvf_nside = 0, n_uvf = 0;
    double uvf_box = 0, uvf_off[3] = {0, 0, 0};
    // the excursion set (set_uvf_params, cooling_uvfluc.c:33-45, with get_J21_coeffs(AlphaUV)) and SphP.local_J21 / SphP.zreion: the device
    // columns in effect (mpg_dev_set_excursion_columns, or s_j21 / s_zre after mpg_resident_sph_set_excursion_columns) and the table size
    // they were bound for; the host columns the host forms upload per call into s_j21_call / s_zre_call
    bool have_exc = false;
    mpg_excursion_set_params exc{};
    const double *d_j21 = nullptr, *d_zre = nullptr;
    int64_t n_exc = 0;
    const double *h_j21 = nullptr, *h_zre = nullptr;
    DevBuf<double> s_j21, s_zre, s_j21_call, s_zre_call;
    DevBuf<unsigned> exc_bad;

    void set_excursion_set(const mpg_excursion_set_params *p);
    // get_local_UVBG's switch (cooling_uvfluc.c:238)
    bool j21_mode(double redshift) const { return have_exc && exc.ExcursionSetReionOn && redshift > exc.ExcursionSetZStop; }
    cool::J21View j21_view(double redshift) const;
    // in the J21 mode: the columns are bound, and for a table of n particles; `who` names the call in the refusal
    void check_excursion_columns(const char *who, double redshift, int64_t n) const;
    // get_local_UVBG at n arbitrary points; returns the number of points without a background (J21 NaN or negative, zreion NaN)
    int64_t excursion_points(int64_t n, const double *d_J21, const double *d_zreion, double redshift, const mpg_uvbg &global, mpg_uvbg *d_out,
                             hipStream_t st);
    void set_params(const mpg_cooling_params &p, hipStream_t st);
    void set_metal_table(int nz, const double *zbins, int nnh, const double *nhbins, int nt, const double *tbins, const double *rate, hipStream_t st);
    void set_uvf_table(int64_t nside, const double *table, double BoxSize, hipStream_t st);
    cool::UvfView uvf_view() const;
    // zreion of n arbitrary points; returns the number of points whose coordinates are not finite or out of range (their zreion is NaN)
    int64_t uvf_points(int64_t n, const double *d_pos, double *d_zreion, hipStream_t st);
    // ... and of the listed gas rows of the bound table into uvf_z (every other row: NaN)
    void uvf_rows(const double *d_pos, const uint8_t *type, const float *mass, const int *d_active, int64_t nactive, int64_t n, hipStream_t st);
    cool::Setup setup(const mpg_cooling_step &step, double redshift) const;
    // cooling_direct on the listed particles; returns the number of particles that hit an iteration limit.  With a table loaded every row
    // takes its background from uvf_z, which the caller has filled (uvf_rows); a row whose zreion is NaN counts among the errors.
    int64_t run(const mpg_cooling_arrays &A, const uint8_t *type, const float *mass, const mpg_sph_times &T, const mpg_cooling_step &step,
                const int *d_active, int64_t nactive, int64_t n, hipStream_t st);
    int64_t state(int64_t n, const double *rho, const double *u, double *ne, double *lambdanet, double *temp, double *nh0,
                  const mpg_cooling_step &step, hipStream_t st);
};

} // namespace mpg
