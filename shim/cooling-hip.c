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
 *   StarformationOn != 0: the reference's loop runs, with two hook lines written by tools/link_reference.sh: the `else cooling_direct(...)`
 *     of sfr_eff.c:270-271 first offers the particle to mpg_shim_cooling_queue(), and mpg_shim_cooling_flush() runs the queued list on the
 *     device before walltime_measure("/Cooling/Cooling").  Deferring is equivalent: starformation(p_i) reads and writes particle p_i only.
 * With several ranks, a UV-fluctuation table (init_uvf_table) or the excursion-set reionisation in use, the reference's code runs
 * unchanged: the queue refuses every particle.
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
int mpg_shim_uvf_in_use(void);                                             /* cooling_uvfluc.c: UVF.enabled || uvf_params.ExcursionSetReionOn */
int mpg_shim_metal_table(int *n, double **bins, double **rate);            /* cooling_uvfluc.c: MetalCool; returns !CoolingNoMetal */
void mpg_shim_sfr_cooling(int *StarformationOn, double *MinGasTemp, double *temp_to_u, double *HIReionTemp); /* sfr_eff.c: sfr_params */

static int params_set;
static int *queue;          /* particles deferred by the hook of a star-forming run */
static int64_t nqueue;
static int queue_open;

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
    params_set = 1;
}

/* the device form serves one rank with the global UV background */
static int device_cooling_usable(void)
{
    return mpg_shim_ntask() == 1 && !mpg_shim_uvf_in_use();
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
    const double redshift = 1. / Time - 1;
    mpg_sph_times t;
    mpg_cooling_step step;
    memset(&t, 0, sizeof(t));
    memset(&step, 0, sizeof(step));
    t.atime = Time;
    t.hubble = hubble;
    for(i = 0; i <= TIMEBINS; i++) {
        t.dloga_bin[i] = get_dloga_for_bin((int)i, Ti);                                   /* sfr_eff.c:467 */
        step.lastred[i] = 1 / exp(loga_from_ti(Ti - dti_from_timebin((int)i))) - 1;       /* sfr_eff.c:483-484 */
    }
    step.uvbg.J_UV = GlobalUVBG->J_UV;
    step.uvbg.gJH0 = GlobalUVBG->gJH0;
    step.uvbg.gJHep = GlobalUVBG->gJHep;
    step.uvbg.gJHe0 = GlobalUVBG->gJHe0;
    step.uvbg.epsH0 = GlobalUVBG->epsH0;
    step.uvbg.epsHep = GlobalUVBG->epsHep;
    step.uvbg.epsHe0 = GlobalUVBG->epsHe0;
    step.uvbg.self_shield_dens = GlobalUVBG->self_shield_dens;
    step.uvbg.zreion = GlobalUVBG->zreion;
    step.long_mean_free_path_heating = get_long_mean_free_path_heating(redshift);         /* cooling.c:49 */
    step.redshift = redshift;
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
    if(resident)
        ck(mpg_resident_sph_cooling(mpg_shim_engine(), &v, &t, &step, list, nlist, ne, metallicity, heiii));
    else {
        mpg_shim_sync(Ti, 0, PartManager->BoxSize, 0);
        v = mpg_shim_view();
        mpg_cooling_arrays A = {density, entropy, ne, sfr, metallicity, heiii, tb};
        ck(mpg_cooling(mpg_shim_engine(), &v, PartManager->BoxSize, &A, &t, &step, list, nlist));
    }
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

void cooling_and_starformation(ActiveParticles *act, double Time, double dloga, ForceTree *tree, struct grav_accel_store GravAccel,
                               DomainDecomp *ddecomp, Cosmology *CP, MyFloat *GradRho, RandTable *rnd, FILE *FdSfr)
{
    int sfon;
    double a, b, c;
    mpg_shim_sfr_cooling(&sfon, &a, &b, &c);
    if(!device_cooling_usable()) { /* several ranks, a UV-fluctuation table, the excursion set: the reference's own code */
        if(mpg_shim_resident())
            endrun(5, "cooling_and_starformation(): the reference's loop inside a resident stretch (mpg_shim_resident_end first)\n");
        cpu_cooling_and_starformation(act, Time, dloga, tree, GravAccel, ddecomp, CP, GradRho, rnd, FdSfr);
        return;
    }
    if(sfon) {
        /* the reference's loop decides who forms stars; the others are queued by the hook and cooled on the device by the flush */
        if(mpg_shim_resident())
            endrun(5, "cooling_and_starformation(): star formation reads SphP on the host (mpg_shim_resident_end first)\n");
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
