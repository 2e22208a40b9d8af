// sfr.h -- star formation on the effective equation of state: what cooling_and_starformation (libgadget/sfr_eff.c:186-394) does per gas
// particle besides cooling_direct.  The model is written once for host and device on top of cooling.h's network; sfr.hip holds the
// kernels and the engine's state.  DESIGN 3.15.
#pragma once
#include "../../include/mpgadget_hip.h"
#include "cooling.h"
#include "mpg_common.h"
#include "winds.h"

namespace mpg {
namespace sfr {

using namespace cool;

constexpr double METAL_YIELD = 0.02; // sfr_eff.h:11
// enum StarformationCriterion, sfr_eff.h:16-23, read with HAS (types.h:19)
constexpr int CRIT_MOLECULAR_H2 = 3, CRIT_SELFGRAVITY = 5, CRIT_CONVERGENT_FLOW = 13, CRIT_CONTINUOUS_CUTOFF = 21;
MPG_HD bool has(int val, int flag) { return (flag & val) == flag; }

// the class of a listed row, and the outcome of a star-forming one
enum RowClass { ROW_SKIPPED = 0, ROW_COOLED = 1, ROW_STARFORMING = 2 };
enum Outcome { OUT_NOSTAR = 0, OUT_CONVERT = 1, OUT_SPAWN = 2, OUT_ERROR = 3 };

// sfreff_on_eeqos, sfr_eff.c:534-566 (BHFeedbackUseTcool == 2 is refused by mpg_set_sfr_params)
MPG_HD int sfreff_on_eeqos(const mpg_sfr_params &P, double density, double delaytime, double a3inv)
{
    int flag = 0;
    if(density * a3inv >= P.PhysDensThresh)
        flag = 1;
    if(density < P.OverDensThresh)
        flag = 0;
    if(delaytime > 0)
        flag = 0;
    return flag;
}

// quicklyastarformation, sfr_eff.c:706-725; rnd1 = table[(ID + 1) % size]
MPG_HD int quicklyastarformation(const mpg_sfr_params &P, double temp_to_u, double density, double entropy, double a3inv, double rnd1)
{
    if(density <= P.OverDensThresh)
        return 0;
    const double enttou = entropy_to_u(density, a3inv);
    const double unew = entropy * enttou;
    const double meanweight = (4 / (8 - 5 * (1 - HYDROGEN_MASSFRAC)));
    const double temp = unew * meanweight / temp_to_u;
    if(temp >= P.QuickLymanAlphaTempThresh)
        return 0;
    if(rnd1 < P.QuickLymanAlphaProbability)
        return 1;
    return 0;
}

// struct sfr_eeqos_data, sfr_eff.c:98-112
struct Eeqos {
    double trelax, tsfr, egyhot, cloudfrac, ne;
};

// one gas particle as starformation reads it
struct Row {
    double density, entropy, ne, metallicity, delaytime;
    double hsml, divvel, curlvel, gradrho_mag; // of the criteria that read them, else 0
    float mass;                                // P.Mass is a float: promoted where the C promotes it
    int generation, bhheated, tb_hydro;
};
// ... and what it leaves
struct RowResult {
    double entropy, ne, sfr, metallicity;
    int bhheated;
    double sm, dM, dtime, mass_of_star, cloudfrac;
    int outcome;
};

// get_sfr_eeqos, sfr_eff.c:804-841
MPG_HD Eeqos get_sfr_eeqos(const Setup &S, const mpg_sfr_params &P, const Row &r, double dtime, double a3inv, Counters &C)
{
    Eeqos data;
    data.trelax = P.MaxSfrTimescale;
    data.tsfr = P.MaxSfrTimescale;
    data.egyhot = P.EgySpecCold;
    data.cloudfrac = 0;
    data.ne = 0;
    if(!sfreff_on_eeqos(P, r.density, r.delaytime, a3inv))
        return data;
    data.ne = r.ne;
    data.tsfr = sqrt(P.PhysDensThresh / (r.density * a3inv)) * P.MaxSfrTimescale;
    if(P.BoostSFDenseGas && ((r.density * a3inv) / P.PhysDensThresh > P.BoostSFOverDenseFactor))
        data.tsfr = P.PhysDensThresh / (r.density * a3inv) * P.MaxSfrTimescale;
    if(data.tsfr < dtime && dtime > 0)
        data.tsfr = dtime;
    const double factorEVP = pow(r.density * a3inv / P.PhysDensThresh, -0.8) * P.FactorEVP;
    data.egyhot = P.EgySpecSN / (1 + factorEVP) + P.EgySpecCold;
    const double tcool = get_cooling_time(S, S.redshift, data.egyhot, r.density * a3inv, &data.ne, r.metallicity, C);
    const double y = data.tsfr / tcool * data.egyhot / (P.FactorSN * P.EgySpecSN - (1 - P.FactorSN) * P.EgySpecCold);
    data.cloudfrac = 1 + 1 / (2 * y) - sqrt(1 / y + 1 / (4 * y * y));
    data.trelax = data.tsfr * (1 - data.cloudfrac) / data.cloudfrac / (P.FactorSN * (1 + factorEVP));
    return data;
}

// ev_NH_from_GradRho and get_sfr_factor_due_to_h2, sfr_eff.c:1041-1077
MPG_HD double sfr_factor_due_to_h2(const mpg_sfr_params &P, const Row &r, double atime)
{
    const double a2 = atime * atime;
    const double zoverzsun = r.metallicity / METAL_YIELD;
    double ev_NH = 0;
    if(r.density > 0) {
        if(r.gradrho_mag > 0)
            ev_NH = r.density * r.density / r.gradrho_mag;
        ev_NH += r.density * r.hsml; // include_h == 1
    }
    double tau_fmol = ev_NH / a2;
    tau_fmol *= (0.1 + zoverzsun);
    if(tau_fmol > 0) {
        tau_fmol *= 434.78 * P.tau_fmol_unit;
        double y = 0.756 * (1 + 3.1 * pow(zoverzsun, 0.365));
        y = log(1 + 0.6 * y + 0.01 * y * y) / (0.6 * tau_fmol);
        y = 1 - 0.75 * y / (1 + 0.25 * y);
        if(y < 0)
            y = 0;
        if(y > 1)
            y = 1;
        return y;
    }
    return 1.0;
}

// get_sfr_factor_due_to_selfgravity, sfr_eff.c:1079-1112
MPG_HD double sfr_factor_due_to_selfgravity(const mpg_sfr_params &P, const Row &r, double atime, double a3inv, double hubble)
{
    const double a2 = atime * atime;
    double divv = r.divvel / a2;
    divv += 3.0 * hubble * a2;
    if(has(P.StarformationCriterion, CRIT_CONVERGENT_FLOW)) {
        if(divv >= 0)
            return 0;
    }
    const double dv2abs = (divv * divv + (r.curlvel / a2) * (r.curlvel / a2));
    const double alpha_vir = 0.2387 * dv2abs / (P.GravInternal * r.density * a3inv);
    double y = 1.0;
    if((alpha_vir < 1.0) || (r.density * a3inv > 100. * P.PhysDensThresh))
        y = 66.7;
    else
        y = 0.1;
    if(has(P.StarformationCriterion, CRIT_CONTINUOUS_CUTOFF))
        y *= 1.0 / (1.0 + alpha_vir);
    return y;
}

// get_starformation_rate_full, sfr_eff.c:843-862
MPG_HD double starformation_rate_full(const mpg_sfr_params &P, const Row &r, const Eeqos &d, double atime, double a3inv, double hubble)
{
    if(!sfreff_on_eeqos(P, r.density, r.delaytime, a3inv))
        return 0;
    const double cloudmass = d.cloudfrac * r.mass;
    double rateOfSF = (1 - P.FactorSN) * cloudmass / d.tsfr;
    if(has(P.StarformationCriterion, CRIT_MOLECULAR_H2))
        rateOfSF *= sfr_factor_due_to_h2(P, r, atime);
    if(has(P.StarformationCriterion, CRIT_SELFGRAVITY))
        rateOfSF *= sfr_factor_due_to_selfgravity(P, r, atime, a3inv, hubble);
    return rateOfSF;
}

// cooling_relaxed, sfr_eff.c:666-701: the new entropy; ne and Z are the particle's AFTER starformation's updates (:769, :774)
MPG_HD double cooling_relaxed(const Setup &S, const mpg_sfr_params &P, const Row &r, const Eeqos &d, double dtime, double a3inv, double ne,
                              double Z, int *bhheated, Counters &C)
{
    const double egyeff = P.EgySpecCold * d.cloudfrac + (1 - d.cloudfrac) * d.egyhot;
    const double densityfac = entropy_to_u(r.density, a3inv);
    const double egycurrent = r.entropy * densityfac;
    double trelax = d.trelax;
    if(P.BHFeedbackUseTcool == 3 || (P.BHFeedbackUseTcool == 1 && (*bhheated || egycurrent > 5e6))) {
        if(egycurrent > egyeff) {
            const double tcool = get_cooling_time(S, S.redshift, egycurrent, r.density * a3inv, &ne, Z, C);
            if(tcool < trelax && tcool > 0)
                trelax = tcool;
        }
        *bhheated = 0;
    }
    return (egyeff + (egycurrent - egyeff) * exp(-dtime / trelax)) / densityfac;
}

// find_star_mass, sfr_eff.c:1002-1023 (QuickLymanAlphaProbability == 0)
MPG_HD double find_star_mass(const mpg_sfr_params &P, float mass, int generation)
{
    double mass_of_star = P.avg_baryon_mass / P.Generations;
    if(mass_of_star > mass)
        mass_of_star = mass;
    if(mass < 2 * mass_of_star || generation > P.Generations)
        mass_of_star = mass;
    return mass_of_star;
}

// starformation, sfr_eff.c:731-800, for one particle on the effective equation of state: everything but the spawning.
// w = table[ID % size], rnd1 = table[(ID + 1) % size].  With C.error set the result is not to be used.
MPG_HD RowResult starformation(const Setup &S, const mpg_sfr_params &P, const Row &r, double dloga, double hubble, double atime, double a3inv,
                               double w, double rnd1, Counters &C)
{
    RowResult o;
    const double dtime = dloga / hubble;
    o.dtime = dtime;
    const Eeqos d = get_sfr_eeqos(S, P, r, dtime, a3inv, C);
    o.cloudfrac = d.cloudfrac;
    const double smr = starformation_rate_full(P, r, d, atime, a3inv, hubble);
    const double sm = smr * dtime;
    o.sm = sm;
    const double p = sm / r.mass;
    const double dM = r.mass * (1 - exp(-p));
    o.dM = dM;
    if(dtime > 0)
        o.sfr = dM / dtime * P.UnitSfr_in_solar_per_year;
    else
        o.sfr = smr * P.UnitSfr_in_solar_per_year;
    o.ne = d.ne;
    const double frac = (1 - exp(-p));
    o.metallicity = r.metallicity + w * METAL_YIELD * frac / P.Generations;
    o.bhheated = r.bhheated;
    o.entropy = r.entropy;
    if(dloga > 0 && r.tb_hydro)
        o.entropy = cooling_relaxed(S, P, r, d, dtime, a3inv, o.ne, o.metallicity, &o.bhheated, C);
    const double mass_of_star = find_star_mass(P, r.mass, r.generation);
    o.mass_of_star = mass_of_star;
    const double prob = dM / mass_of_star;
    const int form_star = (rnd1 < prob);
    o.outcome = OUT_NOSTAR;
    if(form_star)
        o.outcome = r.mass >= 1.1 * mass_of_star ? OUT_SPAWN : OUT_CONVERT;
    if(!form_star || o.outcome == OUT_SPAWN)
        o.metallicity += (1 - w) * METAL_YIELD * frac / P.Generations;
    if(C.error)
        o.outcome = OUT_ERROR;
    return o;
}

} // namespace sfr

// device view of mpg_sfr_columns with the bound table's Type and Mass
struct SfrView {
    const uint8_t *type; // null: all type 1 (nothing is gas)
    const float *mass;
    int64_t n;
    mpg_sfr_columns a;
    const double *pos = nullptr; // the bound positions: read with a UV-fluctuation table only
};

constexpr int SFR_NSTATS = 8; // mpg_sfr_get_stats

// the engine's star-formation state: parameters, the lists and counters of the last call
struct SfrEngine {
    bool have_params = false;
    mpg_sfr_params par{};
    DevBuf<uint8_t> cls, outcome, rowclass, ns_spawn; // per list entry: RowClass; per star-forming entry: Outcome; per particle: RowClass; per new star
    DevBuf<int> coollist, sflist, ns_parent, maybewind;
    DevBuf<int> sfevals;                              // per particle: network evaluations of a star-forming row, -1 otherwise
    DevBuf<double> sfmass, ns_mass, partial, sums;    // mass_of_star per star-forming entry / per new star; per-block partial sums; the three sums
    DevBuf<unsigned> blockcnt, totals;
    DevBuf<unsigned long long> ctr;                   // evaluations, errors and spawned stars of k_sfr_eeqos
    int64_t n_rows = 0; // particles rowclass / sfevals were last written for
    mpg_sfr_result last{};
    int64_t last_stats[SFR_NSTATS] = {0, 0, 0, 0, 0, 0, 0, 0};
    // have_uvf_table: the engine holds a UV-fluctuation table, which UVFluctuationOn must agree with; have_excursion_set: it holds an
    // excursion-set model, without which ExcursionSetReion is refused
    void set_params(const mpg_sfr_params &p, bool have_uvf_table, bool have_excursion_set);
    // the loop of cooling_and_starformation up to the spawning; returns the rows that hit an iteration limit (cooled and star-forming)
    int64_t run(CoolingEngine &cooling, const SfrView &A, const mpg_wind_params *wind, const double *rnd, uint64_t rndsize, const mpg_sph_times &T,
                const mpg_cooling_step &step, const int *d_active, int64_t nactive, hipStream_t st);
};

} // namespace mpg
