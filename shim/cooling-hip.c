/* libgadget/cooling-hip.c -- the cooling of cooling_and_starformation() (sfr_eff.c:186-394, called at run.c:663-664 on every step of a run
 * with CoolingOn) forwarded to libmpgadget_hip.so.
 *
 * The reference's own definition stays in the link under another name (sfr_eff.o is compiled with
 * -Dcooling_and_starformation=cpu_cooling_and_starformation, tools/link_reference.sh).
 *   StarformationOn == 0 (Lyman-alpha forest runs): cooling_direct (sfr_eff.c:463-514) is the whole loop.  This file gathers the SphP
 *     columns it reads in particle order the way veldisp-hip.c does, takes the step's UV background, the long-mean-free-path heating and the
 *     bin tables from the reference's own functions (get_global_UVBG, get_long_mean_free_path_heating, get_dloga_for_bin, loga_from_ti)
 *     and forwards the active list.  Inside a resident stretch (timestep-hip.c) Density, Entropy and TimeBinHydro are the resident
 *     columns and only Ne, Metallicity and HeIIIionized travel.
 *   StarformationOn != 0: the reference's function runs, and a hook written by tools/link_reference.sh in front of its loop
 *     (sfr_eff.c:219-273) hands that loop to mpg_shim_sfr_loop() below: the columns of mpg_sfr_columns are gathered from P / SphP in particle
 *     order, mpg_cooling_and_starformation (inside a resident stretch mpg_resident_sph_cooling_and_starformation) does everything that
 *     changes neither the number of rows nor a row's type, the columns are scattered back, and the new-star list comes back IN THE ORDER OF
 *     THE ACTIVE LIST into the reference's own NewStars / NewParents arrays (slots_split_particle for a spawned star, the parent itself for
 *     a converted one) with the four sums.  The reference's own code from :275 on - winds_subgrid, sfr_reserve_slots, make_particle_star,
 *     add_new_particle_to_active, the FdSfr line, winds_and_feedback - then runs on them unchanged.  A resident stretch is ended only when
 *     that code has something to do: a new star, or - subgrid winds, whose kicks the resident form does not carry - a MaybeWind list that
 *     is not empty, which then goes to the reference's winds_subgrid.
 *     BHFeedbackUseTcool == 2, which the engine refuses: the reference's loop runs with the two older hook lines: the `else
 *     cooling_direct(...)` of sfr_eff.c:270-271 first offers the particle to mpg_shim_cooling_queue(), and mpg_shim_cooling_flush() runs the
 *     queued list on the device before walltime_measure("/Cooling/Cooling").  Deferring is equivalent: starformation(p_i) reads and writes
 *     particle p_i only.
 * A UV-fluctuation table (init_uvf_table) is loaded onto the device once, with PartManager->BoxSize, and every device call is preceded by
 * mpg_set_uvf_offset(PartManager->CurrentParticleOffset): the engine then gives every row the background of get_local_UVBG_from_global.
 * With the excursion set in use (ExcursionSetReionOn, a build with EXCUR_REION) the model goes to the engine once with the coefficients of the
 * reference's own get_J21_coeffs(AlphaUV), and every device call binds SphP.local_J21 / SphP.zreion gathered by particle.
 * With several ranks the reference's code runs unchanged: the queue refuses every particle.
 * The parameters are file-static in the reference; tools/link_reference.sh appends one accessor each to cooling_rates.c, cooling.c,
 * cooling_uvfluc.c and sfr_eff.c (listed in INTEGRATION.md).
 * Compiled inside the reference tree (see gravity-hip.c). */
#include <mpi.h>
#include <math.h>
#include <string.h>
#include <omp.h>
#include "cooling.h"
#include "cooling_rates.h"
#include "cooling_qso_lightup.h"
#include "sfr_eff.h"
#include "winds.h"
#include "utils/system.h"
#include "timebinmgr.h"
#include "partmanager.h"
#include "slotsmanager.h"
#include "walltime.h"
#include "utils/endrun.h"
#include "utils/mymalloc.h"
#include <mpgadget_hip.h>
#include "mpg_shim.h"

#define ck mpg_shim_ck

/* the reference's function under the name the build gives it (see above) */
void cpu_cooling_and_starformation(ActiveParticles *act, double Time, double dloga, ForceTree *tree, struct grav_accel_store GravAccel,
                                   DomainDecomp *ddecomp, Cosmology *CP, MyFloat *GradRho, RandTable *rnd, FILE *FdSfr);
/* the accessors appended to the reference files (tools/link_reference.sh, step 4) */
struct cooling_params mpg_shim_cooling_params(void);                       /* cooling_rates.c: CoolingParams */
struct cooling_units mpg_shim_cooling_units(void);                         /* cooling.c: coolunits */
int mpg_shim_uvf_table(int64_t *nside, double **table);                    /* cooling_uvfluc.c: UVF.Nside, UVF.Table; returns UVF.enabled */
int mpg_shim_excursion_set_on(void);                                       /* cooling_uvfluc.c: uvf_params.ExcursionSetReionOn */
void mpg_shim_uvf_params(int *ExcursionSetReionOn, double *ExcursionSetZStop, double *AlphaUV); /* cooling_uvfluc.c: uvf_params */
int mpg_shim_metal_table(int *n, double **bins, double **rate);            /* cooling_uvfluc.c: MetalCool; returns !CoolingNoMetal */
void mpg_shim_sfr_cooling(int *StarformationOn, double *MinGasTemp, double *temp_to_u, double *HIReionTemp); /* sfr_eff.c: sfr_params */
void mpg_shim_sfr_params(mpg_sfr_params *p);                               /* sfr_eff.c: sfr_params after init_cooling_and_star_formation */
void mpg_shim_wind_params(mpg_wind_params *p);                             /* winds.c: wind_params after init_winds */

static int params_set;
static int *queue;          /* particles deferred by the hook of a star-forming run */
static int64_t nqueue;
static int queue_open;
static int sfr_open;        /* the device runs the loop of the reference's function (mpg_shim_sfr_loop) */
static double sfr_grav;     /* CP->GravInternal of that call */

/* set_coolpar / init_cooling / InitMetalCooling as the reference holds them now (once per run: they do not change after begrun) */
static void set_params(void)
{
    if(params_set)
        return;
    const struct cooling_params cp = mpg_shim_cooling_params();
    const struct cooling_units cu = mpg_shim_cooling_units();
    int sfon;
    mpg_cooling_params p;
    memset(&p, 0, sizeof(p));
    p.recomb = cp.recomb;
    p.cooling = cp.cooling;
    p.SelfShieldingOn = cp.SelfShieldingOn;
    p.PhotoIonizationOn = cp.PhotoIonizationOn;
    p.fBar = cp.fBar;
    p.PhotoIonizeFactor = cp.PhotoIonizeFactor;
    p.CMBTemperature = cp.CMBTemperature;
    p.MinGasTemp = cp.MinGasTemp;
    p.UVRedshiftThreshold = cp.UVRedshiftThreshold;
    p.HydrogenHeatAmp = cp.HydrogenHeatAmp;
    p.HeliumHeatOn = cp.HeliumHeatOn;
    p.HeliumHeatThresh = cp.HeliumHeatThresh;
    p.HeliumHeatAmp = cp.HeliumHeatAmp;
    p.HeliumHeatExp = cp.HeliumHeatExp;
    p.rho_crit_baryon = cp.rho_crit_baryon;
    p.CoolingOn = cu.CoolingOn;
    p.density_in_phys_cgs = cu.density_in_phys_cgs;
    p.uu_in_cgs = cu.uu_in_cgs;
    p.tt_in_s = cu.tt_in_s;
    p.units_rho_crit_baryon = cu.rho_crit_baryon;
    mpg_shim_sfr_cooling(&sfon, &p.sfr_MinGasTemp, &p.temp_to_u, &p.HIReionTemp);
    ck(mpg_set_cooling_params(mpg_shim_engine(), &p));
    int n[3];
    double *bins[3], *rate;
    if(mpg_shim_metal_table(n, bins, &rate))
        ck(mpg_set_metal_cooling_table(mpg_shim_engine(), n[0], bins[0], n[1], bins[1], n[2], bins[2], rate));
    else
        ck(mpg_set_metal_cooling_table(mpg_shim_engine(), 0, NULL, 0, NULL, 0, NULL, NULL));
    /* init_uvf_table (cooling_uvfluc.c:158-162): the table spans the box */
    int64_t nside;
    double *table;
    if(mpg_shim_uvf_table(&nside, &table))
        ck(mpg_set_uvf_table(mpg_shim_engine(), nside, table, PartManager->BoxSize));
    else
        ck(mpg_set_uvf_table(mpg_shim_engine(), 0, NULL, 0));
    /* set_uvf_params (cooling_uvfluc.c:33-45) with get_J21_coeffs(AlphaUV), which get_local_UVBG_from_J21 evaluates per particle */
    if(mpg_shim_excursion_set_on()) {
        mpg_excursion_set_params ep;
        memset(&ep, 0, sizeof(ep));
        mpg_shim_uvf_params(&ep.ExcursionSetReionOn, &ep.ExcursionSetZStop, &ep.AlphaUV);
        const struct J21_coeffs c = get_J21_coeffs(ep.AlphaUV);
        ep.gJH0 = c.gJH0;
        ep.gJHe0 = c.gJHe0;
        ep.gJHep = c.gJHep;
        ep.epsH0 = c.epsH0;
        ep.epsHe0 = c.epsHe0;
        ep.epsHep = c.epsHep;
        ck(mpg_set_excursion_set(mpg_shim_engine(), &ep));
    }
    else
        ck(mpg_set_excursion_set(mpg_shim_engine(), NULL));
    params_set = 1;
}

/* SphP.local_J21 / SphP.zreion by particle for the device call that follows (sfr_eff.c:478-480, :741-743); the caller frees the block.
 * Without the excursion set nothing is gathered and nothing is bound. */
static double *bind_excursion_columns(int resident)
{
    double *cols = NULL;
#ifdef EXCUR_REION
    if(mpg_shim_excursion_set_on()) {
        const int64_t n = PartManager->NumPart;
        int64_t i;
        cols = (double *)mymalloc("mpg_excursion", ((size_t)n * 2 + 1) * sizeof(double));
        #pragma omp parallel for
        for(i = 0; i < n; i++) {
            const int gas = P[i].Type == 0 && !P[i].IsGarbage;
            cols[i] = gas ? SPHP(i).local_J21 : 0;
            cols[n + i] = gas ? SPHP(i).zreion : -1;
        }
        if(resident)
            ck(mpg_resident_sph_set_excursion_columns(mpg_shim_engine(), cols, cols + n));
        else
            ck(mpg_set_excursion_columns(mpg_shim_engine(), cols, cols + n));
    }
#else
    (void)resident;
#endif
    return cols;
}

static void unbind_excursion_columns(double *cols, int resident)
{
    if(!cols)
        return;
    if(resident)
        ck(mpg_resident_sph_set_excursion_columns(mpg_shim_engine(), NULL, NULL));
    else
        ck(mpg_set_excursion_columns(mpg_shim_engine(), NULL, NULL));
    myfree(cols);
}

/* the device form serves one rank, with the global UV background, that of a UV-fluctuation table or that of the excursion set's J21 */
static int device_cooling_usable(void)
{
    return mpg_shim_ntask() == 1;
}

/* PartManager->CurrentParticleOffset (cooling_uvfluc.c:185-188) for the device call that follows */
static void set_uvf_offset(void)
{
    ck(mpg_set_uvf_offset(mpg_shim_engine(), PartManager->CurrentParticleOffset));
}

/* the bin tables and the UV background of a step */
static void fill_step(inttime_t Ti, double Time, double hubble, const struct UVBG *GlobalUVBG, mpg_sph_times *t, mpg_cooling_step *step)
{
    const double redshift = 1. / Time - 1;
    int i;
    memset(t, 0, sizeof(*t));
    memset(step, 0, sizeof(*step));
    t->atime = Time;
    t->hubble = hubble;
    for(i = 0; i <= TIMEBINS; i++) {
        t->dloga_bin[i] = get_dloga_for_bin(i, Ti);                                        /* sfr_eff.c:467 */
        step->lastred[i] = 1 / exp(loga_from_ti(Ti - dti_from_timebin(i))) - 1;            /* sfr_eff.c:483-484 */
    }
    step->uvbg.J_UV = GlobalUVBG->J_UV;
    step->uvbg.gJH0 = GlobalUVBG->gJH0;
    step->uvbg.gJHep = GlobalUVBG->gJHep;
    step->uvbg.gJHe0 = GlobalUVBG->gJHe0;
    step->uvbg.epsH0 = GlobalUVBG->epsH0;
    step->uvbg.epsHep = GlobalUVBG->epsHep;
    step->uvbg.epsHe0 = GlobalUVBG->epsHe0;
    step->uvbg.self_shield_dens = GlobalUVBG->self_shield_dens;
    step->uvbg.zreion = GlobalUVBG->zreion;
    step->long_mean_free_path_heating = get_long_mean_free_path_heating(redshift);         /* cooling.c:49 */
    step->redshift = redshift;
}

/* cooling_direct for the listed particles (NULL: all) on the device */
static void cool_on_device(const int *list, int64_t nlist, double Time, double hubble, const struct UVBG *GlobalUVBG)
{
    const int64_t n = PartManager->NumPart;
    int64_t i;
    if((list && nlist == 0) || n == 0)
        return;
    set_params();
    /* every listed particle has been drifted to the current time (run.c:414): its Ti_drift is Ti_Current */
    const inttime_t Ti = P[list ? list[0] : 0].Ti_drift;
    mpg_sph_times t;
    mpg_cooling_step step;
    fill_step(Ti, Time, hubble, GlobalUVBG, &t, &step);
    const int resident = mpg_shim_resident();
    double *block = (double *)mymalloc("mpg_cooling", (size_t)n * 5 * sizeof(double));
    uint8_t *bytes = (uint8_t *)mymalloc("mpg_cooling_u8", (size_t)n * 2);
    double *density = block, *entropy = block + n, *ne = block + 2 * n, *sfr = block + 3 * n, *metallicity = block + 4 * n;
    uint8_t *heiii = bytes, *tb = bytes + n;
    #pragma omp parallel for
    for(i = 0; i < n; i++) {
        const int gas = P[i].Type == 0 && !P[i].IsGarbage;
        density[i] = gas ? SPHP(i).Density : 0;
        entropy[i] = gas ? SPHP(i).Entropy : 0;
        ne[i] = gas ? SPHP(i).Ne : 0;
        sfr[i] = gas ? SPHP(i).Sfr : 0;
        metallicity[i] = gas ? SPHP(i).Metallicity : 0;
        heiii[i] = P[i].HeIIIionized;
        tb[i] = P[i].TimeBinHydro;
    }
    mpg_particle_view v = mpg_shim_view();
    set_uvf_offset();
    double *excursion = bind_excursion_columns(resident);
    if(resident)
        ck(mpg_resident_sph_cooling(mpg_shim_engine(), &v, &t, &step, list, nlist, ne, metallicity, heiii));
    else {
        mpg_shim_sync(Ti, 0, PartManager->BoxSize, 0);
        v = mpg_shim_view();
        mpg_cooling_arrays A = {density, entropy, ne, sfr, metallicity, heiii, tb};
        ck(mpg_cooling(mpg_shim_engine(), &v, PartManager->BoxSize, &A, &t, &step, list, nlist));
    }
    unbind_excursion_columns(excursion, resident);
    /* sfr_eff.c:509-513 for the particles the loop treats (sfr_eff.c:229) */
    const int64_t count = list ? nlist : n;
    #pragma omp parallel for
    for(i = 0; i < count; i++) {
        const int p = list ? list[i] : (int)i;
        if(P[p].Type != 0 || P[p].IsGarbage || P[p].Mass <= 0)
            continue;
        SPHP(p).Ne = ne[p];
        if(!resident) /* (resident: the entropy is the device's column until mpg_shim_resident_end) */
            SPHP(p).Entropy = entropy[p];
        SPHP(p).Sfr = 0;
    }
    myfree(bytes);
    myfree(block);
}

/* ---- the hooks of a star-forming run (sfr_eff.c:270-271, :277) ---- */
/* 1: the particle is taken, its cooling_direct runs in mpg_shim_cooling_flush; 0: the caller runs cooling_direct itself */
int mpg_shim_cooling_queue(int p_i)
{
    if(!queue_open)
        return 0;
    int64_t k;
    #pragma omp atomic capture
    k = nqueue++;
    queue[k] = p_i;
    return 1;
}

void mpg_shim_cooling_flush(double Time, double hubble, const struct UVBG *GlobalUVBG)
{
    if(!queue_open)
        return;
    queue_open = 0;
    cool_on_device(queue, nqueue, Time, hubble, GlobalUVBG);
    nqueue = 0;
}

/* ---- the loop of a star-forming run on the device (the hook in front of sfr_eff.c:219) ----
 * 0: the reference runs its own loop (with the two hooks above).  1: the loop is done: the columns are in P / SphP, NewStar / NewParent
 * (and, see the head of this file, MaybeWind with StellarMass) hold the lists in the order of the active list in their first segment, the
 * four sums are set. */
int mpg_shim_sfr_loop(ActiveParticles *act, double Time, double hubble, const struct UVBG *GlobalUVBG, MyFloat *GradRho, RandTable *rnd,
                      gadget_thread_arrays *NewStar, gadget_thread_arrays *NewParent, gadget_thread_arrays *MaybeWind, MyFloat *StellarMass,
                      double *sum_sm, double *localsfr, double *sum_dtime, int64_t *sum_sf_part)
{
    if(!sfr_open)
        return 0;
    const int64_t n = PartManager->NumPart;
    const int *list = act->ActiveParticle;
    const int64_t nlist = act->NumActiveParticle;
    int64_t i;
    if(nlist == 0 || n == 0)
        return 1;
    set_params();
    mpg_sfr_params sp;
    memset(&sp, 0, sizeof(sp));
    mpg_shim_sfr_params(&sp); /* (UVFluctuationOn from UVF.enabled: set_params above has loaded that table) */
    sp.GravInternal = sfr_grav;
    sp.NTask = 1;
    sp.ExcursionSetReion = mpg_shim_excursion_set_on(); /* (set_params above has passed the model) */
    const int resident = mpg_shim_resident();
    const int subgrid = sp.WindOn && winds_are_subgrid() && MaybeWind->sizes && StellarMass;
    if(resident && subgrid)
        sp.WindOn = 0; /* the kicks are the reference's, after the stretch has ended */
    ck(mpg_set_sfr_params(mpg_shim_engine(), &sp));
    ck(mpg_set_random_table(mpg_shim_engine(), rnd->Table, (int64_t)rnd->tablesize));
    const int winds = sp.WindOn || subgrid; /* without winds nothing sets a DelayTime: no column, no winds_evolve */
    if(winds) {
        mpg_wind_params wp;
        mpg_shim_wind_params(&wp);
        ck(mpg_set_wind_params(mpg_shim_engine(), &wp));
    }
    const inttime_t Ti = P[list ? list[0] : 0].Ti_drift;
    mpg_sph_times t;
    mpg_cooling_step step;
    fill_step(Ti, Time, hubble, GlobalUVBG, &t, &step);
    /* only what the settings read travels; inside a resident stretch Density, Entropy, TimeBinHydro, Hsml, DivVel and CurlVel are the
     * stretch's own columns (the host copies are stale) and are neither gathered nor staged */
    const int model = !(sp.QuickLymanAlphaProbability > 0);
    const int h2 = model && (sp.StarformationCriterion & 3) == 3, selfgrav = model && (sp.StarformationCriterion & 5) == 5; /* HAS(), sfr_eff.h:16-23 */
    const int kicks = subgrid && !resident;                   /* the device makes the subgrid kicks: VDisp and Vel */
    const int heated = model && sp.BHFeedbackUseTcool != 0;   /* cooling_relaxed reads and clears BHHeated in modes 1 and 3 */
    const int use_density = !resident, use_hsml = h2 && !resident, use_div = selfgrav && !resident, use_grad = h2 && GradRho != NULL;
    const int ncol = use_density * 2 + use_hsml + use_div * 2 + use_grad + kicks * 4 + 3 + winds + subgrid + 1 /* id */;
    double *block = (double *)mymalloc("mpg_sfr", ((size_t)n * ncol + 1) * sizeof(double));
    uint8_t *bytes = (uint8_t *)mymalloc("mpg_sfr_u8", (size_t)n * 4 + 1);
    double *q = block;
#define COL(use, w) ((use) ? (q += (size_t)n * (w), q - (size_t)n * (w)) : NULL)
    double *density = COL(use_density, 1), *entropy = COL(use_density, 1), *hsml = COL(use_hsml, 1), *divvel = COL(use_div, 1), *curlvel = COL(use_div, 1);
    double *gradrho = COL(use_grad, 1), *vdisp = COL(kicks, 1), *vel = COL(kicks, 3), *ne = COL(1, 1), *sfr = COL(1, 1), *metallicity = COL(1, 1);
    double *delaytime = COL(winds, 1), *stellarmass = COL(subgrid, 1);
    uint64_t *id = (uint64_t *)COL(1, 1);
#undef COL
    uint8_t *generation = bytes, *heiii = bytes + n, *tb = resident ? NULL : bytes + 2 * n, *bhheated = heated ? bytes + 3 * n : NULL;
    #pragma omp parallel for
    for(i = 0; i < n; i++) {
        const int gas = P[i].Type == 0 && !P[i].IsGarbage;
        int k;
        id[i] = P[i].ID;
        generation[i] = P[i].Generation;
        heiii[i] = P[i].HeIIIionized;
        if(tb)
            tb[i] = P[i].TimeBinHydro;
        if(bhheated)
            bhheated[i] = P[i].BHHeated;
        if(hsml)
            hsml[i] = P[i].Hsml;
        if(use_density) {
            density[i] = gas ? SPHP(i).Density : 0;
            entropy[i] = gas ? SPHP(i).Entropy : 0;
        }
        if(use_div) {
            divvel[i] = gas ? SPHP(i).DivVel : 0;
            curlvel[i] = gas ? SPHP(i).CurlVel : 0;
        }
        if(gradrho)
            gradrho[i] = gas ? GradRho[P[i].PI] : 0;
        if(kicks) {
            vdisp[i] = gas ? SPHP(i).VDisp : 0;
            for(k = 0; k < 3; k++)
                vel[3 * i + k] = P[i].Vel[k];
        }
        ne[i] = gas ? SPHP(i).Ne : 0;
        sfr[i] = gas ? SPHP(i).Sfr : 0;
        metallicity[i] = gas ? SPHP(i).Metallicity : 0;
        if(delaytime)
            delaytime[i] = gas ? SPHP(i).DelayTime : 0;
        if(stellarmass)
            stellarmass[i] = 0;
    }
    mpg_sfr_columns A;
    memset(&A, 0, sizeof(A));
    A.id = id;
    A.generation = generation;
    A.density = density;
    A.hsml = hsml;
    A.divvel = divvel;
    A.curlvel = curlvel;
    A.gradrho_mag = gradrho;
    A.tb_hydro = tb;
    A.heiii_ionized = heiii;
    A.vdisp = vdisp;
    A.entropy = entropy;
    A.ne = ne;
    A.sfr = sfr;
    A.metallicity = metallicity;
    A.delaytime = delaytime;
    A.bhheated = bhheated;
    A.vel = vel;
    A.stellarmass = stellarmass;
    mpg_particle_view v = mpg_shim_view();
    set_uvf_offset();
    double *excursion = bind_excursion_columns(resident);
    if(resident)
        ck(mpg_resident_sph_cooling_and_starformation(mpg_shim_engine(), &v, &A, &t, &step, list, nlist));
    else {
        mpg_shim_sync(Ti, 0, PartManager->BoxSize, 0);
        v = mpg_shim_view();
        ck(mpg_cooling_and_starformation(mpg_shim_engine(), &v, PartManager->BoxSize, &A, &t, &step, list, nlist));
    }
    unbind_excursion_columns(excursion, resident);
    /* the columns of the rows the loop treats (sfr_eff.c:229) back into P / SphP */
    const int64_t count = list ? nlist : n;
    #pragma omp parallel for
    for(i = 0; i < count; i++) {
        const int p = list ? list[i] : (int)i;
        if(P[p].Type != 0 || P[p].IsGarbage || P[p].Mass <= 0)
            continue;
        SPHP(p).Ne = ne[p];
        SPHP(p).Sfr = sfr[p];
        SPHP(p).Metallicity = metallicity[p];
        if(bhheated)
            P[p].BHHeated = bhheated[p];
        if(winds)
            SPHP(p).DelayTime = delaytime[p];
        if(!resident) { /* (resident: the entropy is the device's column until mpg_shim_resident_end; no kick was applied) */
            SPHP(p).Entropy = entropy[p];
            if(kicks) {
                int k;
                for(k = 0; k < 3; k++)
                    P[p].Vel[k] = vel[3 * p + k];
            }
        }
    }
    mpg_sfr_result r;
    ck(mpg_sfr_get_result(mpg_shim_engine(), &r));
    const int wind_list = resident && subgrid; /* the reference's winds_subgrid gets the list */
    if(r.newstars > (int64_t)NewStar->total_size || (wind_list && r.maybewind > (int64_t)MaybeWind->total_size))
        endrun(5, "cooling_and_starformation(): %ld new stars and %ld wind candidates for lists of %ld\n", (long)r.newstars, (long)r.maybewind,
               (long)NewStar->total_size);
    int32_t *parent = (int32_t *)mymalloc("mpg_sfr_parent", ((size_t)r.newstars + 1) * sizeof(int32_t));
    double *starmass = (double *)mymalloc("mpg_sfr_mass", ((size_t)r.newstars + 1) * sizeof(double));
    uint8_t *spawn = (uint8_t *)mymalloc("mpg_sfr_spawn", (size_t)r.newstars + 1);
    int64_t nnew = 0, nwind = 0;
    ck(mpg_sfr_export(mpg_shim_engine(), r.newstars, parent, starmass, spawn, &nnew, wind_list ? r.maybewind : 0, wind_list ? MaybeWind->srcs[0] : NULL,
                      &nwind));
    if(resident && (nnew > 0 || (wind_list && nwind > 0)))
        mpg_shim_resident_end(); /* P / SphP are read and written by what follows.  In the middle of the step: its two host blocks are
                                  * malloc'ed, not on the stack allocator whose top the blocks above and the reference's occupy (timestep-hip.c) */
    /* sfr_eff.c:783-791 and :256-261, in the order of the active list (what gadget_compact_thread_arrays gives under the static schedule) */
    int64_t spawned = 0;
    for(i = 0; i < nnew; i++) {
        int child = parent[i];
        if(spawn[i]) {
            child = slots_split_particle(parent[i], starmass[i], PartManager);
            spawned++;
        }
        NewStar->srcs[0][i] = child;
        NewParent->srcs[0][i] = parent[i];
    }
    NewStar->sizes[0] = nnew;
    NewParent->sizes[0] = nnew;
    if(spawned)
        mpg_shim_particles_changed();
    if(wind_list) { /* sfr_eff.c:264-268 */
        for(i = 0; i < nwind; i++)
            StellarMass[P[MaybeWind->srcs[0][i]].PI] = stellarmass[MaybeWind->srcs[0][i]];
        MaybeWind->sizes[0] = nwind;
    }
    *sum_sm = r.sum_sm;
    *localsfr = r.localsfr;
    *sum_dtime = r.sum_dtime;
    *sum_sf_part = r.sum_sf_part;
    myfree(spawn);
    myfree(starmass);
    myfree(parent);
    myfree(bytes);
    myfree(block);
    return 1;
}

void cooling_and_starformation(ActiveParticles *act, double Time, double dloga, ForceTree *tree, struct grav_accel_store GravAccel,
                               DomainDecomp *ddecomp, Cosmology *CP, MyFloat *GradRho, RandTable *rnd, FILE *FdSfr)
{
    int sfon;
    double a, b, c;
    mpg_shim_sfr_cooling(&sfon, &a, &b, &c);
    if(!device_cooling_usable()) { /* several ranks: the reference's own code */
        if(mpg_shim_resident())
            endrun(5, "cooling_and_starformation(): the reference's loop inside a resident stretch (mpg_shim_resident_end first)\n");
        cpu_cooling_and_starformation(act, Time, dloga, tree, GravAccel, ddecomp, CP, GradRho, rnd, FdSfr);
        return;
    }
    if(sfon) {
        mpg_sfr_params sp;
        memset(&sp, 0, sizeof(sp));
        mpg_shim_sfr_params(&sp);
        if(sp.BHFeedbackUseTcool != 2) {
            /* the reference's function with its loop on the device (mpg_shim_sfr_loop); it spawns the stars of the list it gets back */
            sfr_open = 1;
            sfr_grav = CP->GravInternal;
            cpu_cooling_and_starformation(act, Time, dloga, tree, GravAccel, ddecomp, CP, GradRho, rnd, FdSfr);
            sfr_open = 0;
            return;
        }
        /* BHFeedbackUseTcool == 2: the reference's loop decides who forms stars; the others are queued by the hook and cooled on the
         * device by the flush */
        if(mpg_shim_resident())
            endrun(5, "cooling_and_starformation(): BHFeedbackUseTcool == 2 reads SphP on the host (mpg_shim_resident_end first)\n");
        /* from the upper end of the reference's stack allocator, released after everything the loop allocates */
        queue = (int *)mymalloc2("mpg_cooling_queue", ((size_t)act->NumActiveParticle + 1) * sizeof(int));
        nqueue = 0;
        queue_open = 1;
        cpu_cooling_and_starformation(act, Time, dloga, tree, GravAccel, ddecomp, CP, GradRho, rnd, FdSfr);
        myfree(queue);
        queue = NULL;
        queue_open = 0;
        return;
    }
    /* StarformationOn == 0: sfr_eff.c:210-277 with cooling_direct on the device; the function returns at :302-303 */
    walltime_measure("/Misc");
    const double hubble = hubble_function(CP, Time);
    const double redshift = 1. / Time - 1;
    struct UVBG GlobalUVBG = get_global_UVBG(redshift);
    cool_on_device(act->ActiveParticle, act->NumActiveParticle, Time, hubble, &GlobalUVBG);
    walltime_measure("/Cooling/Cooling");
}
