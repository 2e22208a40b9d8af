/* libgadget/heiii-hip.c -- do_heiii_reionization() of the reference (cooling_qso_lightup.c:641-659; called from run.c:632-635 inside the
 * FOF block of a PM step) forwarded to libmpgadget_hip.so.
 *
 * The reference's own definition stays in the link under another name (cooling_qso_lightup.o is compiled with
 * -Ddo_heiii_reionization=cpu_do_heiii_reionization, tools/link_reference.sh): with several ranks this file calls it, because the library
 * has no several-rank form (count_QSO_halos).
 * With one rank turn_on_quasars (:523-638) runs on the device: the flash, the fraction, and the bubbles as batched scans of the gas.  No
 * tree is used: the `gasTree` argument is not read, and a tree that exists only on the device (forcetree-hip.c) is left as it is.  The call
 * sits behind fof_fof, which exchanges particles, so it runs outside a resident stretch and the host form is the only one.  This file
 * gathers Density, Entropy and HeIIIionized in particle order and Mass, CM and MinID of fof->Group, makes the call, scatters Entropy and
 * the flag of the gas back, and writes the reference's messages and the lines of FdHelium from mpg_heiii_export.  The guards (:644-651),
 * the interpolation of the history table (:530) and the rhobar arithmetic (:550-554) stay here, behind two accessors that
 * tools/link_reference.sh appends to its working copy of cooling_qso_lightup.c (the parameters, qso_inst_heating and the table are
 * file-static there).  The step's random table goes over on every call.  Clocks /HeIII/Find, /HeIII/Build and /HeIII/Ionize as the reference.
 * Compiled inside the reference tree (see gravity-hip.c). */
#include <mpi.h>
#include <math.h>
#include <stdio.h>
#include <string.h>
#include <omp.h>
#include "cooling_qso_lightup.h"
#include "physconst.h"
#include "partmanager.h"
#include "slotsmanager.h"
#include "walltime.h"
#include "utils/endrun.h"
#include "utils/mymalloc.h"
#include <mpgadget_hip.h>
#include "mpg_shim.h"

#define ck mpg_shim_ck

/* the reference's function under the name the build gives it (see above) */
void cpu_do_heiii_reionization(double atime, FOFGroups *fof, ForceTree *gasTree, Cosmology *CP, RandTable *rnd, double uu_in_cgs, FILE *FdHelium);
/* appended to the working copy of cooling_qso_lightup.c (tools/link_reference.sh, step 4) */
void mpg_shim_heiii_params(mpg_heiii_params *p, double *inst_heating, double *heIIIreion_start, double *table_end);
double mpg_shim_heiii_desired(double atime);

void do_heiii_reionization(double atime, FOFGroups *fof, ForceTree *gasTree, Cosmology *CP, RandTable *rnd, double uu_in_cgs, FILE *FdHelium)
{
    if(mpg_shim_ntask() > 1) { /* several ranks: the reference's own loop (no mpg_dist_* form of it) */
        if(mpg_shim_resident())
            endrun(5, "do_heiii_reionization(): several ranks inside a resident stretch (mpg_shim_resident_end first)\n");
        cpu_do_heiii_reionization(atime, fof, gasTree, CP, rnd, uu_in_cgs, FdHelium);
        return;
    }
    (void)gasTree;
    if(!qso_lightup_on()) /* :644-651 */
        return;
    mpg_heiii_params par;
    mpg_heiii_step st;
    double start, table_end;
    mpg_shim_heiii_params(&par, &st.qso_inst_heating, &start, &table_end);
    if(atime < 1 / (1 + start))
        return;
    if(atime > table_end)
        return;
    if(mpg_shim_resident())
        endrun(5, "do_heiii_reionization(): inside a resident stretch (fof_fof exchanges particles: mpg_shim_resident_end first)\n");
    walltime_measure("/Misc");
    const int64_t n = PartManager->NumPart, ng = fof->Ngroups;
    const double a3inv = 1 / pow(atime, 3);
    st.atime = atime;
    st.desired_ion_frac = mpg_shim_heiii_desired(atime);
    st.uu_in_cgs = uu_in_cgs;
    st.n_gas_tot = SlotsManager->info[0].size;
    /* :550-554 */
    const double rhobar = CP->OmegaBaryon * (3 * HUBBLE * CP->HubbleParam * HUBBLE * CP->HubbleParam) / (8 * M_PI * GRAVITY) * a3inv;
    const double totbubblegasmass = 4 * M_PI / 3. * pow(par.mean_bubble, 3) * rhobar;
    st.non_overlapping_bubble_number = st.n_gas_tot * totbubblegasmass / CP->OmegaBaryon;
    st.TotNgroups = fof->TotNgroups;
    ck(mpg_set_heiii_params(mpg_shim_engine(), &par));
    ck(mpg_set_random_table(mpg_shim_engine(), rnd->Table, (int64_t)rnd->tablesize));

    /* the columns in particle order and the group table: one block */
    double *block = (double *)mymalloc("mpg_heiii", ((size_t)n * 2 + (size_t)ng * 5 + 2) * sizeof(double) + (size_t)n);
    double *density = block, *entropy = block + n, *gmass = block + 2 * n, *gcm = gmass + ng;
    uint64_t *gminid = (uint64_t *)(gcm + 3 * ng);
    uint8_t *flag = (uint8_t *)(gminid + ng + 1);
    int64_t i, ncand = 0;
    #pragma omp parallel for
    for(i = 0; i < n; i++) {
        density[i] = entropy[i] = 0;
        flag[i] = P[i].HeIIIionized;
        if(P[i].Type == 0 && !P[i].IsGarbage && !P[i].Swallowed) {
            density[i] = SPHP(i).Density;
            entropy[i] = SPHP(i).Entropy;
        }
    }
    for(i = 0; i < ng; i++) {
        int k;
        gmass[i] = fof->Group[i].Mass;
        for(k = 0; k < 3; k++)
            gcm[3 * i + k] = fof->Group[i].CM[k];
        gminid[i] = fof->Group[i].base.MinID;
        if(!(gmass[i] < par.qso_candidate_min_mass) && !(gmass[i] > par.qso_candidate_max_mass))
            ncand++;
    }
    /* fof_fof has exchanged particles inside this Ti_Current */
    mpg_shim_particles_changed();
    mpg_shim_sync(-1, atime, PartManager->BoxSize, 0);
    mpg_particle_view v = mpg_shim_view();
    mpg_heiii_result res;
    ck(mpg_heiii_reionization(mpg_shim_engine(), &v, PartManager->BoxSize, &st, density, entropy, flag, gmass, gcm, gminid, ng, &res));
    #pragma omp parallel for
    for(i = 0; i < n; i++) {
        if(P[i].Type != 0 || P[i].IsGarbage || P[i].Swallowed)
            continue;
        P[i].HeIIIionized = flag[i];
        SPHP(i).Entropy = entropy[i];
    }

    /* the reference's messages and the lines of FdHelium (:547, :558, :573, :583, :603-621, :633-636) */
    if(st.desired_ion_frac > par.heIIIreion_finish_frac)
        message(0, "HeII: Helium ionization finished, flash-ionizing %ld particles (%g of total)\n", (long)res.flash_ionized,
                (double)res.flash_ionized / (double)st.n_gas_tot);
    message(0, "HeII: Started helium reionization model with ionization fraction %g\n", res.initionfrac);
    if(res.stop_reason != MPG_HEIII_NOTHING_TO_DO)
        walltime_measure("/HeIII/Find");
    if(res.stop_reason == MPG_HEIII_NOTHING_TO_DO || res.stop_reason == MPG_HEIII_NO_CANDIDATES) { /* :568-572 */
        myfree(block);
        return;
    }
    message(0, "HeII: Built quasar candidate list from %ld quasars\n", (long)ncand);
    walltime_measure("/HeIII/Build");
    const int64_t nit = res.iterations;
    int64_t *position = (int64_t *)mymalloc("mpg_heiii_it", (size_t)(nit + 1) * 5 * sizeof(int64_t));
    int64_t *group = position + nit + 1, *count = group + nit + 1, got = 0;
    double *curionfrac = (double *)(count + nit + 1);
    ck(mpg_heiii_export(mpg_shim_engine(), nit, position, group, NULL, count, curionfrac, &got));
    for(i = 0; i < got && i < nit; i++) {
        double qso_pos[3] = {0};
        if(position[i] > 0) {
            int k;
            for(k = 0; k < 3; k++) { /* :598-602 */
                qso_pos[k] = fof->Group[group[i]].CM[k] - PartManager->CurrentParticleOffset[k];
                while(qso_pos[k] > PartManager->BoxSize)
                    qso_pos[k] -= PartManager->BoxSize;
                while(qso_pos[k] <= 0)
                    qso_pos[k] += PartManager->BoxSize;
            }
            message(1, "HeII: Quasar %d changed the HeIII ionization fraction to %g, ionizing %ld\n", (int)group[i], curionfrac[i], (long)count[i]);
        }
        if(FdHelium) {
            fprintf(FdHelium, "%g %g %g %g %g %ld\n", atime, qso_pos[0], qso_pos[1], qso_pos[2], curionfrac[i], (long)count[i]);
            fflush(FdHelium);
        }
    }
    myfree(position);
    if(res.stop_reason == MPG_HEIII_EXHAUSTED && st.desired_ion_frac - res.curionfrac > 0.1)
        message(0, "HeII: Ionization fraction %g less than desired ionization fraction of %g because not enough quasars\n", res.curionfrac,
                st.desired_ion_frac);
    if(res.stop_reason == MPG_HEIII_INSUFFICIENT)
        message(0, "HeII: Stopping ionization at iteration %d because insufficient ionization happened.\n", (int)(nit - 1));
    myfree(block);
    if(res.tot_n_ionized > 0)
        message(0, "HeII: HeIII fraction from %g -> %g, ionizing %ld. Wanted %g.\n", res.initionfrac, res.curionfrac, (long)res.tot_n_ionized,
                st.desired_ion_frac);
    else
        message(0, "HeII: HeIII fraction unchanged at %g. Wanted %g\n", res.curionfrac, st.desired_ion_frac);
    walltime_measure("/HeIII/Ionize");
}
