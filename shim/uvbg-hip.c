/* libgadget/uvbg-hip.c -- calculate_uvbg() of the reference (uvbg.c:506-593; called from run.c:636-642 inside the FOF block of a PM step,
 * in a build with EXCUR_REION) forwarded to libmpgadget_hip.so.
 *
 * The reference's own definition stays in the link under another name (uvbg.o is compiled with -Dcalculate_uvbg=cpu_calculate_uvbg,
 * tools/link_reference.sh): with several ranks this file calls it, because the library has no several-rank form.
 * With one rank the three deposits, the transforms, the loop over the filter radii and the read-out run on the device
 * (mpg_calculate_uvbg); the three PetaPM objects are not used.  The call sits behind fof_fof, which exchanges particles, so it runs outside
 * a resident stretch and the host form is the only one.  This file gathers Sfr, EscapeFraction (the halo mass fof_set_escapefraction left
 * there), local_J21 and zreion of SphP / StarP in particle order, makes the call, scatters EscapeFraction, local_J21 and zreion back and
 * writes the reference's two messages.  The consumer is not carried: the reference's own cooling loop reads local_J21 / zreion
 * (cooling-hip.c keeps refusing to take that loop over in such a build).  The parameters are file-static in uvbg.c: one accessor that
 * tools/link_reference.sh appends to its working copy.  Not carried: save_uvbg_grids (a DEBUG build's snapshot of the grids;
 * mpg_dev_uvbg_grids has them).  Clocks /UVBG/find_HII_bubbles and /UVBG as the reference.
 * Without EXCUR_REION this file is empty, as the reference's definition is.
 * Compiled inside the reference tree (see gravity-hip.c). */
#include <mpi.h>
#include <math.h>
#include <stdio.h>
#include <string.h>
#include <omp.h>
#include "uvbg.h"
#include "physconst.h"
#include "partmanager.h"
#include "slotsmanager.h"
#include "walltime.h"
#include "utils/endrun.h"
#include "utils/mymalloc.h"
#include <mpgadget_hip.h>
#include "mpg_shim.h"

#ifdef EXCUR_REION
#define ck mpg_shim_ck

/* the reference's function under the name the build gives it (see above) */
void cpu_calculate_uvbg(PetaPM *pm_mass, PetaPM *pm_star, PetaPM *pm_sfr, int WriteSnapshot, int SnapshotFileCount, char *OutputDir, double Time,
                        Cosmology *CP, const struct UnitSystem units);
/* appended to the working copy of uvbg.c (tools/link_reference.sh, step 4) */
void mpg_shim_uvbg_params(mpg_uvbg_params *p);

void calculate_uvbg(PetaPM *pm_mass, PetaPM *pm_star, PetaPM *pm_sfr, int WriteSnapshot, int SnapshotFileCount, char *OutputDir, double Time,
                    Cosmology *CP, const struct UnitSystem units)
{
    if(mpg_shim_ntask() > 1) { /* several ranks: the reference's own loop (no mpg_dist_* form of it) */
        if(mpg_shim_resident())
            endrun(5, "calculate_uvbg(): several ranks inside a resident stretch (mpg_shim_resident_end first)\n");
        cpu_calculate_uvbg(pm_mass, pm_star, pm_sfr, WriteSnapshot, SnapshotFileCount, OutputDir, Time, CP, units);
        return;
    }
    (void)pm_mass; (void)pm_star; (void)pm_sfr; (void)WriteSnapshot; (void)SnapshotFileCount; (void)OutputDir;
    if(mpg_shim_resident())
        endrun(5, "calculate_uvbg(): inside a resident stretch (fof_fof exchanges particles: mpg_shim_resident_end first)\n");
    walltime_measure("/Misc");
    mpg_uvbg_params par;
    memset(&par, 0, sizeof(par));
    mpg_shim_uvbg_params(&par);
    par.Time = Time;
    par.Omega0 = CP->Omega0;
    par.OmegaBaryon = CP->OmegaBaryon;
    par.RhoCrit = CP->RhoCrit;
    par.HubbleParam = CP->HubbleParam;
    par.hubble = hubble_function(CP, Time);
    par.UnitLength_in_cm = units.UnitLength_in_cm;
    par.UnitMass_in_g = units.UnitMass_in_g;
    par.UnitTime_in_s = units.UnitTime_in_s;
    par.NTask = 1;

    /* the columns in particle order: one block */
    const int64_t n = PartManager->NumPart;
    double *block = (double *)mymalloc("mpg_uvbg", ((size_t)n * 4 + 1) * sizeof(double));
    mpg_uvbg_columns c;
    c.sfr = block;
    c.escfrac = block + n;
    c.local_J21 = block + 2 * n;
    c.zreion = block + 3 * n;
    int64_t i;
    #pragma omp parallel for
    for(i = 0; i < n; i++) {
        c.sfr[i] = c.escfrac[i] = c.local_J21[i] = 0;
        c.zreion[i] = -1;
        if(P[i].IsGarbage || P[i].Swallowed)
            continue;
        if(P[i].Type == 0) {
            c.sfr[i] = SPHP(i).Sfr;
            c.escfrac[i] = SPHP(i).EscapeFraction;
            c.local_J21[i] = SPHP(i).local_J21;
            c.zreion[i] = SPHP(i).zreion;
        }
        else if(P[i].Type == 4)
            c.escfrac[i] = STARP(i).EscapeFraction;
    }
    /* fof_fof has exchanged particles inside this Ti_Current */
    mpg_shim_particles_changed();
    mpg_shim_sync(-1, Time, PartManager->BoxSize, 0);
    mpg_particle_view v = mpg_shim_view();
    mpg_uvbg_result res;
    memset(&res, 0, sizeof(res));
    message(0, "Away to call find_HII_bubbles...\n");
    ck(mpg_calculate_uvbg(mpg_shim_engine(), &v, PartManager->BoxSize, &par, &c, &res));
    #pragma omp parallel for
    for(i = 0; i < n; i++) {
        if(P[i].IsGarbage || P[i].Swallowed)
            continue;
        if(P[i].Type == 0) {
            SPHP(i).EscapeFraction = c.escfrac[i];
            SPHP(i).local_J21 = c.local_J21[i];
            SPHP(i).zreion = c.zreion[i];
        }
        else if(P[i].Type == 4)
            STARP(i).EscapeFraction = c.escfrac[i];
    }
    myfree(block);
    message(0, "vol weighted xhi : %f\n", res.volume_weighted_global_xHI);
    message(0, "mass weighted xhi : %f\n", res.mass_weighted_global_xHI);
    walltime_measure("/UVBG/find_HII_bubbles");
    walltime_measure("/UVBG");
}
#endif /* EXCUR_REION */
