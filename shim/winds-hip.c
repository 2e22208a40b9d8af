/* libgadget/winds-hip.c -- winds_and_feedback() of the reference (winds.c:298-371; called from cooling_and_starformation,
 * sfr_eff.c:391-392) forwarded to libmpgadget_hip.so.
 *
 * The reference's own definition stays in the link under another name (winds.o is compiled with
 * -Dwinds_and_feedback=cpu_winds_and_feedback, tools/link_reference.sh): with several ranks this file calls it, because the library has
 * no several-rank form of these walks.  winds_subgrid (:275-295) and winds_evolve (:374-391) stay the
 * reference's: both are per particle and without a neighbour.  The second is called particle by particle from inside the loop of
 * cooling_and_starformation, so there is no place for a batched call.  The first could be forwarded, but the library has no host form of
 * it, and a host form would move seven columns to the device and three back for one exp and three table reads per listed particle; that
 * this costs more than the reference's loop is SUPPOSED, nobody has measured it.  The library's batched forms (mpg_dev_winds_subgrid,
 * mpg_dev_winds_evolve) are for callers whose columns are on the device already.
 * With one rank the two tree walks around the new stars - the weight walk and the feedback walk - the nearest-star rule and the kicks run
 * on the device.  cooling_and_starformation runs outside a resident stretch (cooling-hip.c ends it first), so the host form is the
 * only one: it stages the table and builds the gas tree - the `tree` argument is not read, and the CPU tree that the reference would
 * build here when it has none ("Building tree in wind", winds.c:235-240) is not built.  This file gathers ID, Hsml, VDisp, Density, Vel,
 * Entropy and DelayTime in particle order the way blackhole-hip.c does and scatters Vel, Entropy and DelayTime of the gas back.  The
 * step's random table goes over on every call (mpg_set_random_table), the parameters through the accessor that tools/link_reference.sh
 * appends to its working copy of winds.c (struct WindParams is file-static).
 * The message of :364 is written from mpg_winds_get_stats; clock /Cooling/Wind as the reference.
 * Compiled inside the reference tree (see gravity-hip.c). */
#include <mpi.h>
#include <math.h>
#include <string.h>
#include <omp.h>
#include "winds.h"
#include "partmanager.h"
#include "slotsmanager.h"
#include "walltime.h"
#include "utils/endrun.h"
#include "utils/mymalloc.h"
#include <mpgadget_hip.h>
#include "mpg_shim.h"

#define ck mpg_shim_ck

/* the reference's function under the name the build gives it (see above) */
void cpu_winds_and_feedback(int *NewStars, const int64_t NumNewStars, const double Time, RandTable *rnd, ForceTree *tree, DomainDecomp *ddecomp);
/* appended to the working copy of winds.c (tools/link_reference.sh, step 4) */
void mpg_shim_wind_params(mpg_wind_params *p);

/* the columns of mpg_wind_arrays in particle order: one block, freed by the caller */
static double *gather(mpg_wind_arrays *A, uint64_t **id)
{
    const int64_t n = PartManager->NumPart;
    int64_t i;
    double *block = (double *)mymalloc("mpg_winds", (size_t)n * 9 * sizeof(double));
    double *hsml = block, *vdisp = block + n, *density = block + 2 * n, *entropy = block + 3 * n, *delaytime = block + 4 * n, *vel = block + 5 * n;
    *id = (uint64_t *)(block + 8 * n);
    #pragma omp parallel for
    for(i = 0; i < n; i++) {
        int k;
        hsml[i] = P[i].Hsml;
        (*id)[i] = P[i].ID;
        vdisp[i] = density[i] = entropy[i] = delaytime[i] = 0;
        for(k = 0; k < 3; k++)
            vel[3 * i + k] = P[i].Vel[k];
        if(P[i].IsGarbage || P[i].Swallowed)
            continue;
        if(P[i].Type == 0) {
            vdisp[i] = SPHP(i).VDisp;
            density[i] = SPHP(i).Density;
            entropy[i] = SPHP(i).Entropy;
            delaytime[i] = SPHP(i).DelayTime;
        }
        else if(P[i].Type == 4)
            vdisp[i] = STARP(i).VDisp;
    }
    memset(A, 0, sizeof(*A));
    A->id = *id;
    A->hsml = hsml;
    A->vdisp = vdisp;
    A->density = density;
    A->vel = vel;
    A->entropy = entropy;
    A->delaytime = delaytime;
    return block;
}

/* Vel, Entropy and DelayTime of the gas back into P[] / SphP[] */
static void scatter(const mpg_wind_arrays *A)
{
    const int64_t n = PartManager->NumPart;
    int64_t i;
    #pragma omp parallel for
    for(i = 0; i < n; i++) {
        int k;
        if(P[i].Type != 0 || P[i].IsGarbage || P[i].Swallowed)
            continue;
        for(k = 0; k < 3; k++)
            P[i].Vel[k] = A->vel[3 * i + k];
        SPHP(i).Entropy = A->entropy[i];
        SPHP(i).DelayTime = A->delaytime[i];
    }
}

static void hand_over_parameters(const RandTable *rnd)
{
    mpg_wind_params par;
    mpg_shim_wind_params(&par);
    ck(mpg_set_wind_params(mpg_shim_engine(), &par));
    ck(mpg_set_random_table(mpg_shim_engine(), rnd->Table, (int64_t)rnd->tablesize));
}

void winds_and_feedback(int *NewStars, const int64_t NumNewStars, const double Time, RandTable *rnd, ForceTree *tree, DomainDecomp *ddecomp)
{
    if(mpg_shim_ntask() > 1) { /* several ranks: the reference's own walks (no mpg_dist_* form of them) */
        if(mpg_shim_resident())
            endrun(5, "winds_and_feedback(): several ranks inside a resident stretch (mpg_shim_resident_end first)\n");
        cpu_winds_and_feedback(NewStars, NumNewStars, Time, rnd, tree, ddecomp);
        return;
    }
    if(winds_are_subgrid() || NumNewStars <= 0) /* winds.c:302-306 */
        return;
    if(mpg_shim_resident())
        endrun(5, "winds_and_feedback(): inside a resident stretch (cooling-hip.c ends it in a step that has made a star)\n");
    hand_over_parameters(rnd);
    mpg_wind_arrays A;
    uint64_t *id;
    double *block = gather(&A, &id);
    /* the new stars were gas when the step began: P[] changed inside this Ti_Current */
    mpg_shim_particles_changed();
    mpg_shim_sync(-1, Time, PartManager->BoxSize, 0);
    mpg_particle_view v = mpg_shim_view();
    ck(mpg_winds_and_feedback(mpg_shim_engine(), &v, PartManager->BoxSize, &A, NewStars, NumNewStars, Time));
    scatter(&A);
    myfree(block);
    int64_t st[6];
    double maxvel = 0;
    ck(mpg_winds_get_stats(mpg_shim_engine(), st, &maxvel));
    message(0, "Made %ld gas wind, discarded %ld kicks from %ld stars. Vel %g\n", (long)st[4], (long)st[5], (long)st[0], maxvel);
    walltime_measure("/Cooling/Wind");
}
