/* libgadget/veldisp-hip.c -- winds_find_vel_disp() of the reference (veldisp.c:375-466, called at run.c:646-647 on every PM step of a
 * run with CoolingOn) forwarded to libmpgadget_hip.so.
 *
 * The reference's own definition stays in the link under another name (veldisp.o is compiled with
 * -Dwinds_find_vel_disp=cpu_winds_find_vel_disp, tools/link_reference.sh): with several ranks this file calls it, because the library
 * has no several-rank form of this loop.  With one rank the loop runs on the device: the file gathers the fields
 * the loop reads in particle order the way sph-hip.c does - Vel, FullTreeGravAccel, GravPM, TimeBinGravity, Hsml, DtHsml of P[],
 * SphP.Density, and VDisp of the gas (SphP) and black-hole (BHP) slots, which is in/out - and scatters VDisp back.  The star-formation
 * threshold and the drift factor over the next PM step come from the reference's own functions (sfr_density_threshold,
 * get_exact_drift_factor), the kick factors of DM_VelPred from init_kick_factor_data.  Inside a resident stretch (timestep-hip.c) only
 * VDisp travels: everything else the loop reads is the resident table's.
 * After the call the engine's current tree is the tree of the DM particles; the next density() / force_tree_full() of the shim builds
 * its own tree, as it does on every call.
 * Compiled inside the reference tree (see gravity-hip.c). */
#include <mpi.h>
#include <string.h>
#include "veldisp.h"
#include "density.h"
#include "sfr_eff.h"
#include "timefac.h"
#include "partmanager.h"
#include "slotsmanager.h"
#include "walltime.h"
#include "utils/endrun.h"
#include "utils/mymalloc.h"
#include <mpgadget_hip.h>
#include "mpg_shim.h"

#define ck mpg_shim_ck

/* the reference's loop under the name the build gives it (see above) */
void cpu_winds_find_vel_disp(const ActiveParticles *act, const double Time, const double hubble, Cosmology *CP, DriftKickTimes *times,
                             DomainDecomp *ddecomp);

/* SphP.VDisp / BHP.VDisp in particle order (0 for the other types), and back */
static void gather_vdisp(double *vdisp)
{
    int64_t i;
    #pragma omp parallel for
    for(i = 0; i < PartManager->NumPart; i++)
        vdisp[i] = P[i].IsGarbage ? 0 : (P[i].Type == 0 ? SPHP(i).VDisp : (P[i].Type == 5 ? BHP(i).VDisp : 0));
}

static void scatter_vdisp(const double *vdisp)
{
    int64_t i;
    #pragma omp parallel for
    for(i = 0; i < PartManager->NumPart; i++) {
        if(P[i].IsGarbage)
            continue;
        if(P[i].Type == 0)
            SPHP(i).VDisp = vdisp[i];
        else if(P[i].Type == 5)
            BHP(i).VDisp = vdisp[i];
    }
}

/* The engine takes its targets from the active list and the type byte (7 for garbage and swallowed BLACK HOLES, as everywhere).  A gas
 * particle flagged Swallowed is no target of the reference either (winds_veldisp_haswork, veldisp.c:352): when the table holds one, the
 * list handed over leaves it out.  Returns NULL when the caller's list serves as it is. */
static int *active_without_swallowed_gas(const ActiveParticles *act, int64_t *nout)
{
    int64_t i, any = 0;
    #pragma omp parallel for reduction(+ : any)
    for(i = 0; i < PartManager->NumPart; i++)
        any += (P[i].Type == 0 && P[i].Swallowed && !P[i].IsGarbage);
    if(!any)
        return NULL;
    int *list = (int *)mymalloc("mpg_vdisp_active", (size_t)act->NumActiveParticle * sizeof(int));
    int64_t n = 0;
    for(i = 0; i < act->NumActiveParticle; i++) {
        const int p = act->ActiveParticle ? act->ActiveParticle[i] : (int)i;
        if(!(P[p].Type == 0 && P[p].Swallowed))
            list[n++] = p;
    }
    *nout = n;
    return list;
}

void winds_find_vel_disp(const ActiveParticles *act, const double Time, const double hubble, Cosmology *CP, DriftKickTimes *times,
                         DomainDecomp *ddecomp)
{
    if(mpg_shim_ntask() > 1) { /* several ranks: the reference's own loop (no mpg_dist_* form of it) */
        if(mpg_shim_resident())
            endrun(5, "winds_find_vel_disp(): several ranks inside a resident stretch (mpg_shim_resident_end first)\n");
        cpu_winds_find_vel_disp(act, Time, hubble, CP, times, ddecomp);
        return;
    }
    walltime_measure("/Misc");
    const int64_t n = PartManager->NumPart;
    int64_t i;
    struct kick_factor_data kf;
    mpg_sph_times t;
    mpg_veldisp_params par;
    init_kick_factor_data(&kf, times, CP);
    memset(&t, 0, sizeof(t));
    t.FgravkickB = kf.FgravkickB;
    for(i = 0; i <= TIMEBINS; i++)
        t.gravkicks[i] = kf.gravkicks[i];
    par.Time = Time;
    par.hubble = hubble;
    par.ddrift = get_exact_drift_factor(CP, times->Ti_Current, times->Ti_Current + times->PM_length); /* veldisp.c:399 */
    par.sfr_density_threshold = sfr_density_threshold(Time);                                          /* veldisp.c:362 */
    int64_t nact = act->NumActiveParticle;
    int *own_list = active_without_swallowed_gas(act, &nact);
    const int *list = own_list ? own_list : act->ActiveParticle;
    if(mpg_shim_resident()) {
        double *vdisp = (double *)mymalloc("mpg_vdisp", (size_t)n * sizeof(double));
        gather_vdisp(vdisp);
        mpg_particle_view rv = mpg_shim_view();
        ck(mpg_resident_sph_find_vel_disp(mpg_shim_engine(), &rv, &t, &par, list, nact, vdisp));
        scatter_vdisp(vdisp);
        myfree(vdisp);
    }
    else {
        mpg_shim_set_domain(ddecomp);
        mpg_shim_sync(times->Ti_Current, 0, PartManager->BoxSize, 0);
        mpg_particle_view v = mpg_shim_view();
        double *block = (double *)mymalloc("mpg_vdisp", (size_t)n * 13 * sizeof(double));
        uint8_t *tb = (uint8_t *)mymalloc("mpg_vdisp_tb", (size_t)n);
        double *vel = block, *gacc = block + 3 * n, *gpm = block + 6 * n, *hsml = block + 9 * n, *dthsml = block + 10 * n,
               *density = block + 11 * n, *vdisp = block + 12 * n;
        #pragma omp parallel for
        for(i = 0; i < n; i++) {
            int k;
            for(k = 0; k < 3; k++) {
                vel[3 * i + k] = P[i].Vel[k];
                gacc[3 * i + k] = P[i].FullTreeGravAccel[k];
                gpm[3 * i + k] = P[i].GravPM[k];
            }
            hsml[i] = P[i].Hsml;
            dthsml[i] = P[i].DtHsml;
            density[i] = (P[i].Type == 0 && !P[i].IsGarbage) ? SPHP(i).Density : 0;
            tb[i] = P[i].TimeBinGravity;
        }
        gather_vdisp(vdisp);
        mpg_veldisp_arrays A = {vel, gacc, gpm, tb, hsml, dthsml, density, vdisp};
        ck(mpg_find_vel_disp(mpg_shim_engine(), &v, PartManager->BoxSize, &A, &t, &par, list, nact));
        scatter_vdisp(vdisp);
        myfree(tb);
        myfree(block);
    }
    if(own_list)
        myfree(own_list);
    walltime_measure("/Cooling/VDisp");
}
