/* libgadget/metals-hip.c -- metal_return() of the reference (metal_return.c:518-576, called at run.c:613 after hydro_force on every step
 * of a run with MetalReturnOn) forwarded to libmpgadget_hip.so.
 *
 * The reference's own definition stays in the link under another name (metal_return.o is compiled with
 * -Dmetal_return=cpu_metal_return, tools/link_reference.sh): with several ranks this file calls it, because the library has no
 * several-rank form of these walks.
 * With one rank the two tree walks - stellar_density and the return walk - run on the device.  What stays on the host, in the reference's
 * own code, is the yield of a stellar population over its step: metal_return_init() (ages, dying-mass limits, the mass returned) and, per
 * returning star, metal_yield() - GSL quadrature over the yield tables.  metal_yield is static: tools/link_reference.sh appends a
 * forwarding function (mpg_shim_metal_yield) and the accessor of the file-static MetalParams to its working copy of metal_return.c.  This
 * file does what metal_return_copy does with the yields (scaled by the initial mass, negatives clamped, metal_return.c:581-611), gathers
 * the columns the walks read in particle order the way veldisp-hip.c does, and scatters the results back.  P[].Mass is read from and
 * written into the records by the library.  Inside a resident stretch (timestep-hip.c) Pos, Mass, Hsml and Density are the resident
 * table's; the metal columns and the per-star inputs travel.  So does the stars' Hsml, which no other call of a stretch reads or writes:
 * the library takes the rows of type 4 from the array handed over and returns the column, and P[].Hsml of the stars is written here in
 * both forms - stellar_density assigns it and the next step starts from it (mpg_shim_resident_end brings back the gas rows only).
 * The reference's repair of a star with Hsml == 0 (effhsml, :786-791) reads the father node of a particle that is not in the gas tree; the
 * repair here is its second branch, BoxSize / NumPart^(1/3) / 4, before the call (it reaches the device through the same array).
 * Clocks: /SPH/Metals/Init as the reference; the device time of the radius loop (mpg_metals_get_times) goes to
 * /SPH/Metals/Density/Compute - there is no Wait / Reduce / Misc on one rank - and the rest of the call to /SPH/Metals/Yield.
 * The gasTree argument is not read on one rank: the library walks the gas tree it built for density() / hydro_force() (resident stretch)
 * or builds it (host form), as sph-hip.c's loops do.
 * Compiled inside the reference tree (see gravity-hip.c). */
#include <mpi.h>
#include <math.h>
#include <string.h>
#include <omp.h>
#include "metal_return.h"
#include "partmanager.h"
#include "slotsmanager.h"
#include "walltime.h"
#include "utils/endrun.h"
#include "utils/mymalloc.h"
#include <mpgadget_hip.h>
#include "mpg_shim.h"

#define ck mpg_shim_ck

/* the reference's function under the name the build gives it (see above) */
void cpu_metal_return(const ActiveParticles *act, ForceTree *gasTree, Cosmology *CP, const double atime, const double AvgGasMass);
/* appended to the working copy of metal_return.c (tools/link_reference.sh, step 4) */
double mpg_shim_metal_yield(double dtmyrstart, double dtmyrend, double stellarmetal, struct MetalReturnPriv *priv, MyFloat *MetalYields, int tid,
                            double masslow, double masshigh);
void mpg_shim_metal_params(int *SPHWeighting, double *MaxNgbDeviation);

void metal_return(const ActiveParticles *act, ForceTree *gasTree, Cosmology *CP, const double atime, const double AvgGasMass)
{
    if(mpg_shim_ntask() > 1) { /* several ranks: the reference's own walks (no mpg_dist_* form of them) */
        if(mpg_shim_resident())
            endrun(5, "metal_return(): several ranks inside a resident stretch (mpg_shim_resident_end first)\n");
        cpu_metal_return(act, gasTree, CP, atime, AvgGasMass);
        return;
    }
    if(SlotsManager->info[4].size == 0) /* no stars yet, metal_return.c:522-525 */
        return;
    struct MetalReturnPriv priv[1];
    const int64_t nwork = metal_return_init(act, CP, priv, atime);
    walltime_measure("/SPH/Metals/Init");
    if(nwork == 0) {
        metal_return_priv_free(priv);
        return;
    }
    const int64_t n = PartManager->NumPart;
    int64_t i;
    /* per particle: massgenerated, metalgenerated, stellarage, hsml, totalmassreturned, lastenrichment, density, metallicity, and the two
     * blocks of NMETALS */
    double *block = (double *)mymalloc("mpg_metals", (size_t)n * (8 + 2 * NMETALS) * sizeof(double));
    double *massgen = block, *metalgen = block + n, *age = block + 2 * n, *hsml = block + 3 * n, *tmr = block + 4 * n, *last = block + 5 * n,
           *density = block + 6 * n, *metallicity = block + 7 * n, *species = block + 8 * n, *metals = block + (8 + NMETALS) * n;
    #pragma omp parallel for
    for(i = 0; i < n; i++) {
        int k;
        massgen[i] = metalgen[i] = age[i] = tmr[i] = last[i] = density[i] = metallicity[i] = 0;
        for(k = 0; k < NMETALS; k++)
            species[NMETALS * i + k] = metals[NMETALS * i + k] = 0;
        hsml[i] = P[i].Hsml;
        if(P[i].IsGarbage)
            continue;
        if(P[i].Type == 0) {
            density[i] = SPHP(i).Density;
            metallicity[i] = SPHP(i).Metallicity;
            for(k = 0; k < NMETALS; k++)
                metals[NMETALS * i + k] = SPHP(i).Metals[k];
        }
        else if(P[i].Type == 4) {
            tmr[i] = STARP(i).TotalMassReturned;
            last[i] = STARP(i).LastEnrichmentMyr;
        }
    }
    /* the returning stars of the active list: what metal_return_copy computes (metal_return.c:581-611).  priv->MassReturn is defined for
     * the active stars only: every other row keeps massgenerated = 0 and is no target */
    #pragma omp parallel for
    for(i = 0; i < act->NumActiveParticle; i++) {
        const int p = act->ActiveParticle ? act->ActiveParticle[i] : (int)i;
        if(P[p].IsGarbage || !metals_haswork(p, priv->MassReturn))
            continue;
        const int pi = P[p].PI;
        const int tid = omp_get_thread_num();
        const double InitialMass = P[p].Mass + STARP(p).TotalMassReturned;
        MyFloat yields[NMETALS];
        int k;
        double z = mpg_shim_metal_yield(STARP(p).LastEnrichmentMyr, priv->StellarAges[pi], STARP(p).Metallicity, priv, yields, tid,
                                        priv->LowDyingMass[pi], priv->HighDyingMass[pi]);
        massgen[p] = priv->MassReturn[pi];
        age[p] = priv->StellarAges[pi];
        metalgen[p] = InitialMass * z;
        if(metalgen[p] < 0)
            metalgen[p] = 0;
        for(k = 0; k < NMETALS; k++) {
            const double y = yields[k] * InitialMass;
            species[NMETALS * p + k] = y < 0 ? 0 : y;
        }
        if(hsml[p] == 0) /* see the head of the file */
            hsml[p] = PartManager->BoxSize / pow(PartManager->NumPart, 1. / 3) / 4.;
    }
    mpg_metal_params par;
    mpg_shim_metal_params(&par.SPHWeighting, &par.MaxNgbDeviation);
    par.MaxGasMass = 4 * AvgGasMass; /* metal_return.c:535 */
    ck(mpg_set_metal_params(mpg_shim_engine(), &par));
    mpg_metal_arrays A;
    memset(&A, 0, sizeof(A));
    A.massgenerated = massgen;
    A.metalgenerated = metalgen;
    A.speciesgenerated = species;
    A.stellarage = age;
    A.hsml = hsml;
    A.totalmassreturned = tmr;
    A.lastenrichment = last;
    A.density = density;
    A.metallicity = metallicity;
    A.metals = metals;
    if(mpg_shim_resident()) {
        mpg_particle_view rv = mpg_shim_view();
        ck(mpg_resident_sph_metal_return(mpg_shim_engine(), &rv, &A, act->ActiveParticle, act->NumActiveParticle));
    }
    else {
        mpg_shim_sync(-1, atime, PartManager->BoxSize, 0);
        mpg_particle_view v = mpg_shim_view();
        ck(mpg_metal_return(mpg_shim_engine(), &v, PartManager->BoxSize, &A, act->ActiveParticle, act->NumActiveParticle));
    }
    const int resident = mpg_shim_resident();
    #pragma omp parallel for
    for(i = 0; i < n; i++) {
        int k;
        if(P[i].IsGarbage)
            continue;
        if(P[i].Type == 0) {
            if(!resident) /* (a resident stretch holds Density on the device) */
                SPHP(i).Density = density[i];
            SPHP(i).Metallicity = metallicity[i];
            for(k = 0; k < NMETALS; k++)
                SPHP(i).Metals[k] = metals[NMETALS * i + k];
        }
        else if(P[i].Type == 4) {
            P[i].Hsml = hsml[i];
            STARP(i).TotalMassReturned = tmr[i];
            STARP(i).LastEnrichmentMyr = last[i];
        }
    }
    myfree(block);
    metal_return_priv_free(priv);
    double ms[3] = {0, 0, 0};
    ck(mpg_metals_get_times(mpg_shim_engine(), ms));
    walltime_add("/SPH/Metals/Density/Compute", ms[0] * 1e-3);
    walltime_measure("/SPH/Metals/Yield");
}
