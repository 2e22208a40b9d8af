// cooling_rates.h -- the rate fits of the ionisation network and of the cooling function (libgadget/cooling_rates.c:452-1049), once, for
// the host (which tabulates them, init_cooling_rates cooling_rates.c:1152-1171) and for the device (which calls them only outside the
// tables, get_interpolated_recomb cooling_rates.c:651-652).  Selected by the two enums of cooling_rates.h:10-20.  Temperatures in K, rates
// in cm^3/s, cooling rates in erg cm^3/s.
#pragma once
#include <cmath>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define MPG_HD __host__ __device__ inline
#else
#define MPG_HD inline
#endif

namespace mpg {
namespace cool {

// physconst.h
constexpr double BOLTZMANN = 1.38066e-16;
constexpr double BOLEVK = 8.61734e-5;
constexpr double eVinergs = 1.60218e-12;
constexpr double PROTONMASS = 1.6726e-24;
constexpr double ELECTRONMASS = 9.10953e-28;
constexpr double THOMPSON = 6.65245e-25;
constexpr double RAD_CONST = 7.565e-15;
constexpr double LIGHTCGS = 2.99792458e10;
constexpr double GAMMA_MINUS1 = (5.0 / 3.0) - 1;
constexpr double HYDROGEN_MASSFRAC = 0.76;

enum RecombType { Cen92 = 0, Verner96 = 1, Badnell06 = 2 };
enum CoolingType { KWH92 = 0, Enzo2Nyx = 1, Sherwood = 2 };

constexpr int NRECOMBTAB = 1000; // cooling_rates.c:108
// the 13 tabulated functions: six of the network (read together at one index by ne_internal) and seven of the cooling function
enum NetTab { T_alphaHp = 0, T_GammaH0, T_alphaHep, T_alphaHepp, T_GammaHe0, T_GammaHep, NNET };
enum CoolTab { T_collisH0 = 0, T_collisHe0, T_collisHeP, T_recombHp, T_recombHeP, T_recombHePP, T_freefree1, NCOOL };
constexpr int NCOOL_PAD = 8; // row length of the interleaved cooling table

// _Verner96Fit, cooling_rates.c:472-478
MPG_HD double verner96_fit(double temp, double aa, double bb, double temp0, double temp1)
{
    const double sqrttt0 = sqrt(temp / temp0);
    const double sqrttt1 = sqrt(temp / temp1);
    return aa / (sqrttt0 * pow(1 + sqrttt0, 1 - bb) * pow(1 + sqrttt1, 1 + bb));
}

// recomb_alphaHp, cooling_rates.c:481-498
MPG_HD double recomb_alphaHp(double temp, int recomb)
{
    switch(recomb) {
    case Cen92:
        return 8.4e-11 / sqrt(temp) / pow(temp / 1000, 0.2) / (1 + pow(temp / 1e6, 0.7));
    case Verner96:
        return verner96_fit(temp, 7.982e-11, 0.748, 3.148, 7.036e+05);
    default:
        return verner96_fit(temp, 8.318e-11, 0.7472, 2.965, 7.001e5);
    }
}

// _Verner96alphaHep, cooling_rates.c:501-518
MPG_HD double verner96_alphaHep(double temp)
{
    const double lowTfit = verner96_fit(temp, 3.294e-11, 0.6910, 1.554e+01, 3.676e+07);
    const double highTfit = verner96_fit(temp, 9.356e-10, 0.7892, 4.266e-02, 4.677e+06);
    const double swtmp = 7e5;
    const double deltat = 1e5;
    const double upper = swtmp + deltat;
    const double lower = swtmp - deltat;
    const double interpfit = (lowTfit * (upper - temp) + highTfit * (temp - lower)) / (2 * deltat);
    return (temp < lower) * lowTfit + (temp > upper) * highTfit + (upper > temp) * (temp > lower) * interpfit;
}

// recomb_alphaHep, cooling_rates.c:521-535
MPG_HD double recomb_alphaHep(double temp, int recomb)
{
    switch(recomb) {
    case Cen92:
        return 1.5e-10 / pow(temp, 0.6353);
    case Verner96:
        return verner96_alphaHep(temp);
    default:
        return verner96_fit(temp, 1.818E-10, 0.7492, 10.17, 2.786e6);
    }
}

// recomb_alphad, cooling_rates.c:540-558
MPG_HD double recomb_alphad(double temp, int recomb)
{
    if(recomb == Cen92)
        return 1.9e-3 / pow(temp, 1.5) * exp(-4.7e5 / temp) * (1 + 0.3 * exp(-9.4e4 / temp));
    return 1.23e-3 / pow(temp, 1.5) * exp(-4.72e5 / temp) * (1 + 0.3 * exp(-9.4e4 / temp));
}

// recomb_alphaHepd, cooling_rates.c:561-565
MPG_HD double recomb_alphaHepd(double temp, int recomb) { return recomb_alphad(temp, recomb) + recomb_alphaHep(temp, recomb); }

// recomb_alphaHepp, cooling_rates.c:568-582
MPG_HD double recomb_alphaHepp(double temp, int recomb)
{
    switch(recomb) {
    case Cen92:
        return 4 * recomb_alphaHp(temp, recomb);
    case Verner96:
        return verner96_fit(temp, 1.891e-10, 0.7524, 9.370, 2.774e6);
    default:
        return verner96_fit(temp, 5.235E-11, 0.6988 + 0.0829 * exp(-1.682e5 / temp), 7.301, 4.475e6);
    }
}

// _Voronov96Fit, cooling_rates.c:585-590
MPG_HD double voronov96_fit(double temp, double dE, double PP, double AA, double XX, double KK)
{
    const double UU = dE / (BOLEVK * temp);
    return AA * (1 + PP * sqrt(UU)) / (XX + UU) * pow(UU, KK) * exp(-UU);
}

// recomb_GammaeH0 / He0 / Hep, cooling_rates.c:593-641
MPG_HD double recomb_GammaeH0(double temp, int recomb)
{
    if(recomb == Cen92)
        return 5.85e-11 * sqrt(temp) * exp(-157809.1 / temp) / (1 + sqrt(temp / 1e5));
    return voronov96_fit(temp, 13.6, 0, 0.291e-07, 0.232, 0.39);
}
MPG_HD double recomb_GammaeHe0(double temp, int recomb)
{
    if(recomb == Cen92)
        return 2.38e-11 * sqrt(temp) * exp(-285335.4 / temp) / (1 + sqrt(temp / 1e5));
    return voronov96_fit(temp, 24.6, 0, 0.175e-07, 0.180, 0.35);
}
MPG_HD double recomb_GammaeHep(double temp, int recomb)
{
    if(recomb == Cen92)
        return 5.68e-12 * sqrt(temp) * exp(-631515.0 / temp) / (1 + sqrt(temp / 1e5));
    return voronov96_fit(temp, 54.4, 1, 0.205e-08, 0.265, 0.25);
}

// _t5, cooling_rates.c:880-892
MPG_HD double cen92_t5(double temp, int cooling)
{
    const double t0 = cooling == KWH92 ? 1e5 : 5e7;
    return 1 + sqrt(temp / t0);
}

// cooling_rates.c:895-913
MPG_HD double cool_CollisionalExciteH0(double temp, int cooling) { return 7.5e-19 * exp(-118348.0 / temp) / cen92_t5(temp, cooling); }
MPG_HD double cool_CollisionalExciteHeP(double temp, int cooling)
{
    return 5.54e-17 * pow(temp, -0.397) * exp(-473638. / temp) / cen92_t5(temp, cooling);
}
MPG_HD double cool_CollisionalExciteHe0(double temp, int cooling)
{
    return 9.1e-27 * pow(temp, -0.1687) * exp(-473638 / temp) / cen92_t5(temp, cooling);
}

// cool_CollisionalH0, cooling_rates.c:938-959 (with cool_CollisionalIonizeH0 :916-921)
MPG_HD double cool_CollisionalH0(double temp, int recomb, int cooling)
{
    if(cooling == Enzo2Nyx) {
        const double y = log(temp);
        const double Ryd = 2.1798741e-11;
        double tot = -0.75 / BOLTZMANN * Ryd / temp;
        const double coeffslowT[6] = {213.7913, 113.9492, 25.06062, 2.762755, 0.1515352, 3.290382e-3};
        const double coeffshighT[6] = {271.25446, 98.019455, 14.00728, 0.9780842, 3.356289e-2, 4.553323e-4};
        for(int j = 0; j < 6; j++)
            tot += ((temp < 1e5) * coeffslowT[j] + (temp >= 1e5) * coeffshighT[j]) * pow(-y, (double)j);
        return 1e-20 * exp(tot);
    }
    return cool_CollisionalExciteH0(temp, cooling) + 13.5984 * eVinergs * recomb_GammaeH0(temp, recomb);
}
// cool_CollisionalHe0, :962-966 (with :924-928)
MPG_HD double cool_CollisionalHe0(double temp, int recomb, int cooling)
{
    return cool_CollisionalExciteHe0(temp, cooling) + 24.5874 * eVinergs * recomb_GammaeHe0(temp, recomb);
}
// cool_CollisionalHeP, :969-973 (with :931-935)
MPG_HD double cool_CollisionalHeP(double temp, int recomb, int cooling)
{
    return cool_CollisionalExciteHeP(temp, cooling) + 54.417760 * eVinergs * recomb_GammaeHep(temp, recomb);
}

// cool_RecombHp, cooling_rates.c:976-984
MPG_HD double cool_RecombHp(double temp, int recomb, int cooling)
{
    if(cooling == Enzo2Nyx)
        return 2.851e-27 * sqrt(temp) * (5.914 - 0.5 * log(temp) + 0.01184 * pow(temp, 1. / 3));
    return 0.75 * BOLTZMANN * temp * recomb_alphaHp(temp, recomb);
}
// cool_RecombHeP with cool_RecombDielect, cooling_rates.c:987-999
MPG_HD double cool_RecombHeP(double temp, int recomb)
{
    return 0.75 * BOLTZMANN * temp * recomb_alphaHep(temp, recomb) + 6.526e-11 * recomb_alphad(temp, recomb);
}
// cool_RecombHePP, cooling_rates.c:1002-1010
MPG_HD double cool_RecombHePP(double temp, int recomb, int cooling)
{
    if(cooling == Enzo2Nyx)
        return 1.140e-26 * sqrt(temp) * (6.607 - 0.5 * log(temp) + 7.459e-3 * pow(temp, 1. / 3));
    return 0.75 * BOLTZMANN * temp * recomb_alphaHepp(temp, recomb);
}

// cool_FreeFree, cooling_rates.c:1015-1033
MPG_HD double cool_FreeFree(double temp, int zz, int cooling)
{
    double gff;
    if(cooling == Enzo2Nyx) {
        const double lt = 2 * log10(temp / zz);
        if(lt <= log10(3.2e5))
            gff = (0.79464 + 0.1243 * lt);
        else
            gff = (2.13164 - 0.1240 * lt);
    }
    else {
        gff = 1.1 + 0.34 * exp(-pow(5.5 - log10(temp), 2.0) / 3.);
    }
    return 1.426e-27 * sqrt(temp) * pow((double)zz, 2.0) * gff;
}

// the functions behind the tables, by table number
MPG_HD double net_fit(int k, double temp, int recomb)
{
    switch(k) {
    case T_alphaHp:
        return recomb_alphaHp(temp, recomb);
    case T_GammaH0:
        return recomb_GammaeH0(temp, recomb);
    case T_alphaHep:
        return recomb_alphaHepd(temp, recomb); // (includes dielectronic recombination, cooling_rates.c:1161-1162)
    case T_alphaHepp:
        return recomb_alphaHepp(temp, recomb);
    case T_GammaHe0:
        return recomb_GammaeHe0(temp, recomb);
    default:
        return recomb_GammaeHep(temp, recomb);
    }
}
MPG_HD double cool_fit(int k, double temp, int recomb, int cooling)
{
    switch(k) {
    case T_collisH0:
        return cool_CollisionalH0(temp, recomb, cooling);
    case T_collisHe0:
        return cool_CollisionalHe0(temp, recomb, cooling);
    case T_collisHeP:
        return cool_CollisionalHeP(temp, recomb, cooling);
    case T_recombHp:
        return cool_RecombHp(temp, recomb, cooling);
    case T_recombHeP:
        return cool_RecombHeP(temp, recomb);
    case T_recombHePP:
        return cool_RecombHePP(temp, recomb, cooling);
    default:
        return cool_FreeFree(temp, 1, cooling);
    }
}

// get_self_shield_dens, cooling_rates.c:345-361 (Rahmati 2012 eq. 13), in three pieces: the grey opacity of the Faucher-Giguere 2009
// background at a redshift (GrayOpac, cooling_rates.c:75-76; clamped outside the table, gsl's linear interpolation inside), the two
// factors that depend on the redshift and on fBar alone, and what is left per background
constexpr int NGRAY = 6;
MPG_HD double grey_opacity(double redshift)
{
    const double ydata[NGRAY] = {2.59e-18, 2.37e-18, 2.27e-18, 2.15e-18, 2.02e-18, 1.94e-18};
    const double zz[NGRAY] = {0, 1, 2, 3, 4, 5};
    if(redshift <= zz[0])
        return ydata[0];
    if(redshift >= zz[NGRAY - 1])
        return ydata[NGRAY - 1];
    int i = 0; // gsl_interp_bsearch: zz[i] <= redshift < zz[i + 1]
    while(i < NGRAY - 2 && redshift >= zz[i + 1])
        i++;
    const double dx = zz[i + 1] - zz[i], dy = ydata[i + 1] - ydata[i]; // linear_eval, gsl interpolation/linear.c
    return ydata[i] + (redshift - zz[i]) / dx * dy;
}
struct SelfShieldFactors {
    double opac; // pow(greyopac / 2.49e-18, -2./3)
    double fbar; // pow(fBar / 0.17, -1./3)
};
MPG_HD SelfShieldFactors self_shield_factors(double redshift, double fBar)
{
    SelfShieldFactors F;
    F.opac = pow(grey_opacity(redshift) / 2.49e-18, -2. / 3);
    F.fbar = pow(fBar / 0.17, -1. / 3);
    return F;
}
MPG_HD double self_shield_dens(const SelfShieldFactors &F, double gJH0)
{
    if(gJH0 == 0) // before the background switches on there is no self-shielding
        return 1e10;
    const double G12 = gJH0 / 1e-12;
    return 6.73e-3 * F.opac * pow(G12, 2. / 3) * F.fbar;
}

} // namespace cool
} // namespace mpg
