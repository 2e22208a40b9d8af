/* libgadget/blackhole-hip.c -- blackhole() of the reference (blackhole.c:215-370, called at run.c:660 on every step of a run with
 * BlackHoleOn) forwarded to libmpgadget_hip.so.
 *
 * The reference's own definition stays in the link under another name (blackhole.o is compiled with -Dblackhole=cpu_blackhole,
 * tools/link_reference.sh).  This file calls it with several ranks (the library has no several-rank form of these walks, DESIGN.md section
 * 3.11) and with the two settings the engine does not carry: BH_FEEDBACK_OPTTHIN and BHFeedbackUseTcool == 2.
 * With one rank everything between the queue and the file writers runs on the device: dynamical friction and the potential minimum
 * (mpg_blackhole_dynfric / mpg_resident_sph_blackhole_dynfric in place of the reference's blackhole_dynfric and blackhole_dfaccel, which are
 * not called), then the two tree walks - accretion and feedback - and their post-processes.  What stays on the host, in the reference's
 * own code: the queue (blackholes_active) and the two file writers (collect_BH_info, write_blackhole_txt), which are fed from the optional
 * outputs of mpg_blackhole_arrays through a struct BHPriv filled by slot.  The step's random table goes over on every call
 * (mpg_set_random_table).
 * The file-static parameters are read through accessors that tools/link_reference.sh appends to its working copies of blackhole.c,
 * bhdynfric.c, winds.c and sfr_eff.c.  Gas that the call swallowed comes back with IsGarbage in the flags array; slots_mark_garbage is
 * then called here for its counter side effects.  P[].Mass and the flags byte are read from and written into the records by the library.
 * Inside a resident stretch (timestep-hip.c) the table's and the gas arrays' columns are the resident ones - Potential among them, so the
 * dynamical-friction walk needs nothing of P[] there; ID, DelayTime and the per-black-hole members travel.
 * The tree argument is not read on one rank: the dynamical-friction call builds the tree of its own type mask, and the black-hole call then
 * builds its tree of gas and black holes because the current one is another (as after winds_find_vel_disp: the DM tree).
 * Clocks: /BH/DynFric, /BH/Accretion and /BH/Feedback from the device times (mpg_blackhole_get_times), /BH/Info as the reference.
 * Compiled inside the reference tree (see gravity-hip.c). */
#include <mpi.h>
#include <math.h>
#include <string.h>
#include <omp.h>
#include "blackhole.h"
#include "bhdynfric.h"
#include "density.h"
#include "bhinfo.h"
#include "partmanager.h"
#include "slotsmanager.h"
#include "timestep.h"
#include "gravity.h"
#include "walltime.h"
#include "utils/endrun.h"
#include "utils/mymalloc.h"
#include <mpgadget_hip.h>
#include "mpg_shim.h"

#define ck mpg_shim_ck

/* the reference's function under the name the build gives it (see above) */
void cpu_blackhole(const ActiveParticles *act, double atime, Cosmology *CP, ForceTree *tree, DomainDecomp *ddecomp, DriftKickTimes *times,
                   RandTable *rnd, const struct UnitSystem units, FILE *FdBlackHoles, FILE *FdBlackholeDetails, size_t *bhdetailswritten);
int blackholes_active(const ActiveParticles *act, int **ActiveBlackHoles, int64_t *NumActiveBlackHoles); /* blackhole.c:191 */
/* appended to the working copies of blackhole.c, bhdynfric.c, winds.c and sfr_eff.c (tools/link_reference.sh, step 4) */
void mpg_shim_blackhole_params(mpg_blackhole_params *p);
void mpg_shim_bh_dynfric_params(int *BH_DynFrictionMethod, int *BH_DFBoostFactor, double *BH_DFbmax);
int mpg_shim_wind_decouple(void);
void mpg_shim_sfr_blackhole(int *StarformationOn, int *BHFeedbackUseTcool, double *PhysDensThresh, double *OverDensThresh);

void blackhole(const ActiveParticles *act, double atime, Cosmology *CP, ForceTree *tree, DomainDecomp *ddecomp, DriftKickTimes *times,
               RandTable *rnd, const struct UnitSystem units, FILE *FdBlackHoles, FILE *FdBlackholeDetails, size_t *bhdetailswritten)
{
    mpg_blackhole_params par;
    memset(&par, 0, sizeof(par));
    mpg_shim_blackhole_params(&par);
    mpg_shim_sfr_blackhole(&par.StarformationOn, &par.BHFeedbackUseTcool, &par.PhysDensThresh, &par.OverDensThresh);
    if(mpg_shim_ntask() > 1 || (par.BlackHoleFeedbackMethod & BH_FEEDBACK_OPTTHIN) || par.BHFeedbackUseTcool == 2) {
        if(mpg_shim_resident())
            endrun(5, "blackhole(): several ranks or a setting the device walks do not carry inside a resident stretch (mpg_shim_resident_end first)\n");
        cpu_blackhole(act, atime, CP, tree, ddecomp, times, rnd, units, FdBlackHoles, FdBlackholeDetails, bhdetailswritten);
        return;
    }
    if(SlotsManager->info[5].size == 0) /* no black holes, blackhole.c:219-222 */
        return;
    walltime_measure("/Misc");
    int *ActiveBlackHoles = NULL;
    int64_t NumActiveBlackHoles = 0;
    if(blackholes_active(act, &ActiveBlackHoles, &NumActiveBlackHoles) == 0)
        return;
    const int resident = mpg_shim_resident();
    par.BlackHoleRepositionEnabled = BHGetRepositionEnabled();
    par.WindDecouple = mpg_shim_wind_decouple();
    par.ForceSoftening = FORCE_SOFTENING();
    par.GravInternal = CP->GravInternal;
    par.HubbleParam = CP->HubbleParam;
    par.OmegaBaryon = CP->OmegaBaryon;
    par.Hubble = CP->Hubble;
    par.UnitTime_in_s = units.UnitTime_in_s;
    par.UnitVelocity_in_cm_per_s = units.UnitVelocity_in_cm_per_s;
    par.uu_in_cgs = units.UnitEnergy_in_cgs / units.UnitMass_in_g;
    struct kick_factor_data kf;
    init_kick_factor_data(&kf, times, CP);
    mpg_bh_dynfric_params dfpar;
    memset(&dfpar, 0, sizeof(dfpar));
    mpg_shim_bh_dynfric_params(&dfpar.BH_DynFrictionMethod, &dfpar.BH_DFBoostFactor, &dfpar.BH_DFbmax);
    dfpar.BlackHoleRepositionEnabled = par.BlackHoleRepositionEnabled;
    dfpar.GravInternal = CP->GravInternal;
    dfpar.DensityKernelType = (int)GetDensityKernelType();

    const int64_t n = PartManager->NumPart;
    int64_t i;
    mpg_sph_times t;
    int b;
    memset(&t, 0, sizeof(t));
    t.FgravkickB = kf.FgravkickB;
    for(b = 0; b <= TIMEBINS; b++) {
        t.gravkicks[b] = kf.gravkicks[b];
        t.hydrokicks[b] = kf.hydrokicks[b];
        t.dloga_bin[b] = get_dloga_for_bin(b, times->Ti_Current);
    }
    t.atime = atime;
    t.hubble = hubble_function(CP, atime);
    /* columns in particle order, from the arena (freed in reverse order) */
    double *block = (double *)mymalloc("mpg_bh", (size_t)n * 52 * sizeof(double));
    uint64_t *ids = (uint64_t *)mymalloc("mpg_bh_id", (size_t)n * 4 * sizeof(uint64_t));
    int32_t *ints = (int32_t *)mymalloc("mpg_bh_int", (size_t)n * 5 * sizeof(int32_t));
    uint8_t *bytes = (uint8_t *)mymalloc("mpg_bh_u8", (size_t)n * 6);
    double *q = block;
#define COL(w) (q += (size_t)n * (w), q - (size_t)n * (w))
    double *gacc = COL(3), *gpm = COL(3), *hydroacc = COL(3), *hsml = COL(1), *density = COL(1), *delaytime = COL(1), *dfaccel = COL(3),
           *vdisp = COL(1), *vel = COL(3), *entropy = COL(1), *bhmass = COL(1), *mtrack = COL(1), *ke = COL(1), *mdot = COL(1), *drag = COL(3),
           *swallowtime = COL(1), *fws = COL(1), *bhent = COL(1), *gasvel = COL(3), *mgas = COL(1), *accm = COL(1), *accbh = COL(1),
           *accmom = COL(3), *potential = COL(1), *dfdens = COL(1), *dfvel = COL(3), *dfrms = COL(1), *minpot = COL(1), *minpotpos = COL(3),
           *minpotvel = COL(3);
#undef COL
    uint64_t *id = ids, *swallowid = ids + n, *sphswal = ids + 2 * n, *bhswal = ids + 3 * n;
    int32_t *countprogs = ints, *encounter = ints + n, *mintimebin = ints + 2 * n, *keflag = ints + 3 * n, *jump = ints + 4 * n;
    uint8_t *tbh = bytes, *tbg = bytes + n, *active_hydro = bytes + 2 * n, *flags = bytes + 3 * n, *heated = bytes + 4 * n,
            *active_dynfric = bytes + 5 * n;
    memset(block, 0, (size_t)n * 52 * sizeof(double));
    memset(ids, 0, (size_t)n * 4 * sizeof(uint64_t));
    memset(ints, 0, (size_t)n * 5 * sizeof(int32_t));
    #pragma omp parallel for
    for(i = 0; i < n; i++) {
        int k;
        id[i] = P[i].ID;
        tbh[i] = P[i].TimeBinHydro;
        tbg[i] = P[i].TimeBinGravity;
        active_hydro[i] = is_timebin_active(P[i].TimeBinHydro, P[i].Ti_drift) ? 1 : 0;
        flags[i] = (P[i].IsGarbage ? 1 : 0) | (P[i].Swallowed ? 2 : 0);
        heated[i] = P[i].BHHeated;
        hsml[i] = P[i].Hsml;
        potential[i] = P[i].Potential;
        active_dynfric[i] = 0;
        for(k = 0; k < 3; k++) {
            vel[3 * i + k] = P[i].Vel[k];
            gacc[3 * i + k] = P[i].FullTreeGravAccel[k];
            gpm[3 * i + k] = P[i].GravPM[k];
        }
        if(P[i].IsGarbage)
            continue;
        if(P[i].Type == 0) {
            density[i] = SPHP(i).Density;
            entropy[i] = SPHP(i).Entropy;
            delaytime[i] = SPHP(i).DelayTime;
            for(k = 0; k < 3; k++)
                hydroacc[3 * i + k] = SPHP(i).HydroAccel[k];
        }
        else if(P[i].Type == 5) {
            density[i] = BHP(i).Density;
            vdisp[i] = BHP(i).VDisp;
            bhmass[i] = BHP(i).Mass;
            mtrack[i] = BHP(i).Mtrack;
            ke[i] = BHP(i).KineticFdbkEnergy;
            countprogs[i] = BHP(i).CountProgs;
            mdot[i] = BHP(i).Mdot;
            swallowid[i] = BHP(i).SwallowID;
            swallowtime[i] = BHP(i).SwallowTime;
            encounter[i] = BHP(i).encounter;
            mintimebin[i] = BHP(i).minTimeBin;
            active_dynfric[i] = is_timebin_active(BHP(i).TimeBinDynFric, times->Ti_Current) ? 1 : 0;
            dfdens[i] = BHP(i).DF_SurroundingDensity;
            dfrms[i] = BHP(i).DF_SurroundingRmsVel;
            jump[i] = BHP(i).JumpToMinPot;
            minpot[i] = BHP(i).MinPot;
            for(k = 0; k < 3; k++) {
                dfaccel[3 * i + k] = BHP(i).DFAccel[k];
                drag[3 * i + k] = BHP(i).DragAccel[k];
                dfvel[3 * i + k] = BHP(i).DF_SurroundingVel[k];
                minpotpos[3 * i + k] = BHP(i).MinPotPos[k];
                minpotvel[3 * i + k] = BHP(i).MinPotVel[k];
            }
        }
    }
    /* dynamical friction and the potential minimum (blackhole.c:246-256) on the device; the rows of black holes that were no targets come
     * back as they went */
    mpg_bh_dynfric_arrays D;
    memset(&D, 0, sizeof(D));
    D.vel = vel;
    D.gacc = gacc;
    D.gpm = gpm;
    D.hydroacc = hydroacc;
    D.tb_grav = tbg;
    D.tb_hydro = tbh;
    D.hsml = hsml;
    D.potential = potential;
    D.bh_mass = bhmass;
    D.active_dynfric = active_dynfric;
    D.df_density = dfdens;
    D.df_vel = dfvel;
    D.df_rmsvel = dfrms;
    D.jumptominpot = jump;
    D.minpot = minpot;
    D.minpotpos = minpotpos;
    D.minpotvel = minpotvel;
    D.dfaccel = dfaccel;
    ck(mpg_set_bh_dynfric_params(mpg_shim_engine(), &dfpar));
    if(resident) {
        mpg_particle_view rv = mpg_shim_view();
        ck(mpg_resident_sph_blackhole_dynfric(mpg_shim_engine(), &rv, &D, &t, act->ActiveParticle, act->NumActiveParticle));
    }
    else {
        mpg_shim_set_domain(ddecomp);
        mpg_shim_sync(times->Ti_Current, atime, PartManager->BoxSize, 0);
        mpg_particle_view v = mpg_shim_view();
        ck(mpg_blackhole_dynfric(mpg_shim_engine(), &v, PartManager->BoxSize, &D, &t, act->ActiveParticle, act->NumActiveParticle));
    }
    if(dfpar.BH_DynFrictionMethod > 0 || dfpar.BlackHoleRepositionEnabled) {
        #pragma omp parallel for
        for(i = 0; i < n; i++) {
            int k;
            if(P[i].IsGarbage || P[i].Type != 5)
                continue;
            BHP(i).DF_SurroundingDensity = dfdens[i];
            BHP(i).DF_SurroundingRmsVel = dfrms[i];
            BHP(i).JumpToMinPot = (char)jump[i];
            BHP(i).MinPot = minpot[i];
            for(k = 0; k < 3; k++) {
                BHP(i).DFAccel[k] = dfaccel[3 * i + k];
                BHP(i).DF_SurroundingVel[k] = dfvel[3 * i + k];
                BHP(i).MinPotPos[k] = minpotpos[3 * i + k];
                BHP(i).MinPotVel[k] = minpotvel[3 * i + k];
            }
        }
        int64_t dstats[5];
        double zeromass = 0;
        ck(mpg_bh_dynfric_get_stats(mpg_shim_engine(), dstats, &zeromass));
        if(dstats[3] > 0)
            message(0, "Dynamic Friction density is zero for %ld BHs avg mass %g.\n", (long)dstats[3], zeromass / dstats[3]);
    }
    walltime_measure("/BH/DynFric");

    mpg_blackhole_arrays A;
    memset(&A, 0, sizeof(A));
    A.id = id;
    A.gacc = gacc;
    A.gpm = gpm;
    A.hydroacc = hydroacc;
    A.tb_hydro = tbh;
    A.tb_grav = tbg;
    A.hsml = hsml;
    A.density = density;
    A.delaytime = delaytime;
    A.dfaccel = dfaccel;
    A.vdisp = vdisp;
    A.active_hydro = active_hydro;
    A.vel = vel;
    A.entropy = entropy;
    A.flags = flags;
    A.bh_mass = bhmass;
    A.mtrack = mtrack;
    A.kineticfdbkenergy = ke;
    A.countprogs = countprogs;
    A.mdot = mdot;
    A.dragaccel = drag;
    A.encounter = encounter;
    A.mintimebin = mintimebin;
    A.swallowid = swallowid;
    A.swallowtime = swallowtime;
    A.bhheated = heated;
    A.feedbackweightsum = fws;
    A.bh_entropy = bhent;
    A.gasvel = gasvel;
    A.mgasenc = mgas;
    A.keflag = keflag;
    A.accreted_mass = accm;
    A.accreted_bhmass = accbh;
    A.accreted_momentum = accmom;
    A.sph_swallowid = sphswal;
    A.bh_swallowid = bhswal;
    ck(mpg_set_blackhole_params(mpg_shim_engine(), &par));
    ck(mpg_set_random_table(mpg_shim_engine(), rnd->Table, (int64_t)rnd->tablesize));
    if(resident) {
        mpg_particle_view rv = mpg_shim_view();
        ck(mpg_resident_sph_blackhole(mpg_shim_engine(), &rv, &A, &t, act->ActiveParticle, act->NumActiveParticle));
    }
    else {
        mpg_shim_set_domain(ddecomp);
        mpg_shim_sync(times->Ti_Current, atime, PartManager->BoxSize, 0);
        mpg_particle_view v = mpg_shim_view();
        ck(mpg_blackhole(mpg_shim_engine(), &v, PartManager->BoxSize, &A, &t, act->ActiveParticle, act->NumActiveParticle));
    }
    /* the outputs into P / BhP / SphP (P[].Mass and the flags byte were written by the library).  Only the rows of the call's targets and
     * of what they touched differ from what went over. */
    #pragma omp parallel for
    for(i = 0; i < n; i++) {
        int k;
        if(P[i].Type == 0) {
            if(heated[i])
                P[i].BHHeated = 1;
            if(!resident && !(flags[i] & 1)) { /* (a resident stretch holds Vel and Entropy on the device) */
                SPHP(i).Entropy = entropy[i];
                for(k = 0; k < 3; k++)
                    P[i].Vel[k] = vel[3 * i + k];
            }
        }
        else if(P[i].Type == 5) {
            if(!resident)
                for(k = 0; k < 3; k++)
                    P[i].Vel[k] = vel[3 * i + k];
            BHP(i).Mass = bhmass[i];
            BHP(i).Mtrack = mtrack[i];
            BHP(i).KineticFdbkEnergy = ke[i];
            BHP(i).CountProgs = countprogs[i];
            BHP(i).Mdot = mdot[i];
            BHP(i).SwallowID = swallowid[i];
            BHP(i).SwallowTime = swallowtime[i];
            BHP(i).encounter = (char)encounter[i];
            BHP(i).minTimeBin = (unsigned char)mintimebin[i];
            for(k = 0; k < 3; k++)
                BHP(i).DragAccel[k] = drag[3 * i + k];
        }
    }
    /* the gas swallowed: the library set IsGarbage in the records; slots_mark_garbage also marks the slot and counts (serial: it
     * updates the managers' counters) */
    for(i = 0; i < n; i++)
        if(P[i].Type == 0 && (flags[i] & 1) && sphswal[i] != 0) /* (a mark exists only on gas that was live at entry) */
            slots_mark_garbage((int)i, PartManager, SlotsManager);
    int64_t stats[8];
    double ms[3] = {0, 0, 0};
    ck(mpg_blackhole_get_stats(mpg_shim_engine(), stats));
    ck(mpg_blackhole_get_times(mpg_shim_engine(), ms));
    if(stats[0] + stats[1] > 0)
        message(0, "Accretion done: %ld gas particles swallowed, %ld BH particles swallowed\n", (long)stats[0], (long)stats[1]);
    walltime_add("/BH/Accretion", ms[0] * 1e-3);
    walltime_add("/BH/Feedback", (ms[1] + ms[2]) * 1e-3);
    /* the file writers, from the optional outputs: struct BHPriv's arrays are indexed by slot */
    if(FdBlackholeDetails) {
        const size_t nbh = (size_t)SlotsManager->info[5].size, ngas = (size_t)SlotsManager->info[0].size;
        /* (collect_BH_info reads SPH_SwallowID at the BLACK HOLE's slot index, bhinfo.c:129: sized for both) */
        const size_t nsph = ngas > nbh ? ngas : nbh;
        struct BHPriv priv[1];
        memset(priv, 0, sizeof(priv));
        priv->atime = atime;
        priv->SPH_SwallowID = (MyIDType *)mymalloc("SPH_SwallowID", (nsph + 1) * sizeof(MyIDType));
        MyFloat *pb = (MyFloat *)mymalloc("mpg_bh_priv", (nbh + 1) * 12 * sizeof(MyFloat));
        priv->KEflag = (int *)mymalloc("KEflag", (nbh + 1) * sizeof(int));
        memset(priv->SPH_SwallowID, 0, (nsph + 1) * sizeof(MyIDType));
        memset(pb, 0, (nbh + 1) * 12 * sizeof(MyFloat));
        memset(priv->KEflag, 0, (nbh + 1) * sizeof(int));
        priv->BH_Entropy = pb;
        priv->BH_accreted_Mass = pb + nbh;
        priv->BH_accreted_BHMass = pb + 2 * nbh;
        priv->BH_FeedbackWeightSum = pb + 3 * nbh;
        priv->NumDM = pb + 4 * nbh;
        priv->MgasEnc = pb + 5 * nbh;
        priv->BH_SurroundingGasVel = (MyFloat(*)[3])(pb + 6 * nbh);
        priv->BH_accreted_momentum = (MyFloat(*)[3])(pb + 9 * nbh);
        for(i = 0; i < n; i++) {
            int k;
            if(P[i].Type == 0 && P[i].PI >= 0 && (size_t)P[i].PI < nsph)
                priv->SPH_SwallowID[P[i].PI] = sphswal[i];
            if(P[i].Type != 5 || P[i].IsGarbage)
                continue;
            const int PI = P[i].PI;
            priv->BH_Entropy[PI] = bhent[i];
            priv->BH_accreted_Mass[PI] = accm[i];
            priv->BH_accreted_BHMass[PI] = accbh[i];
            priv->BH_FeedbackWeightSum[PI] = fws[i];
            priv->MgasEnc[PI] = mgas[i];
            priv->KEflag[PI] = keflag[i];
            for(k = 0; k < 3; k++) {
                priv->BH_SurroundingGasVel[PI][k] = gasvel[3 * i + k];
                priv->BH_accreted_momentum[PI][k] = accmom[3 * i + k];
            }
        }
        *bhdetailswritten += collect_BH_info(ActiveBlackHoles, NumActiveBlackHoles, priv, PartManager, (struct bh_particle_data *)SlotsManager->info[5].ptr,
                                             FdBlackholeDetails);
        myfree(priv->KEflag);
        myfree(pb);
        myfree(priv->SPH_SwallowID);
    }
    myfree(bytes);
    myfree(ints);
    myfree(ids);
    myfree(block);
    myfree(ActiveBlackHoles);
    write_blackhole_txt(FdBlackHoles, units, atime);
    walltime_measure("/BH/Info");
}
