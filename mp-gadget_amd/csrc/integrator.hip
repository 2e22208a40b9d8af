// integrator.hip -- the time integration on device-resident arrays: drift, the kicks, the step assignment (find_timesteps,
// find_hydro_timesteps, the dynamic-friction bins) and the hierarchical gravity level loop (timestep.c:239-599).  Host side only: the
// kernels are timestep.hip's, the tree and the walk of a level are engine.hip's, called through the C ABI.
#include "engine_internal.h"

static inline int64_t dti_from_timebin(int bin) { return bin > 0 ? ((int64_t)1 << bin) : 0; } // timebinmgr.h:47-50
static inline bool is_timebin_active(int i, int64_t current) // timestep.c:143-150
{
    if(i <= 0 || current <= 0)
        return true;
    return current % dti_from_timebin(i) == 0;
}

// build_active_sublist on the device; returns the count (one small D2H copy: the reference needs the count on the host as well)
static int64_t hier_sublist(mpg_engine *eng, const int *list, int64_t nlist, const uint8_t *tb, const uint8_t *flags, int maxtimebin,
                            int64_t Ti_Current, int *out)
{
    eng->hier_val.reserve((size_t)nlist + 1);
    eng->hier_keep.reserve((size_t)nlist + 1);
    eng->hier_cnt.reserve(64);
    launch_sublist_flags(list, nlist, tb, flags, maxtimebin, Ti_Current, eng->hier_val.p, eng->hier_keep.p, eng->stream);
    compact_flagged(eng->hier_val.p, eng->hier_keep.p, nlist, out, eng->hier_cnt.p + 60, eng->hier_tmp, eng->stream);
    unsigned long long c = 0;
    MPG_HIP(hipMemcpyAsync(&c, eng->hier_cnt.p + 60, sizeof(c), hipMemcpyDeviceToHost, eng->stream));
    MPG_HIP(hipStreamSynchronize(eng->stream));
    return (int64_t)c;
}

// grav_short_tree_build_tree (timestep.c:281-291): tree of the listed particles, walk for them into `accel`
static void hier_tree_and_walk(mpg_engine *eng, const mpg_hiergrav_arrays *A, const int *list, int64_t nlist, double *accel, double rho0,
                               int HybridNuGrav)
{
    if(list && nlist == 0)
        return; // nothing active on this rank: an empty tree and an empty walk
    MPG_CALL(mpg_dev_force_tree_active_moments(eng, list, list ? nlist : 0, HybridNuGrav));
    MPG_CALL(mpg_dev_grav_short_tree(eng, nullptr, A->d_fulltree_accel, A->d_gravpm, list, nlist, accel, A->d_potential, rho0));
    // a tree of all particles: grav_short_postprocess also stores the result in P[].FullTreeGravAccel (gravshort.h:47-67)
    if(eng->full_particle_tree && accel != A->d_fulltree_accel)
        MPG_HIP(hipMemcpyAsync(A->d_fulltree_accel, accel, 3 * (size_t)eng->n * sizeof(double), hipMemcpyDeviceToDevice, eng->stream));
}

// apply_hierarchical_grav_kick, timestep.c:238-278
static void hier_kick(mpg_engine *eng, const mpg_hiergrav_arrays *A, const int *list, int64_t nlist, const double *accel,
                      const mpg_drift_kick_times *times, int ti, int largest_active, mpg_gravkick_fn fn, void *ctx)
{
    const int64_t dti = dti_from_timebin(ti);
    double gravkick = fn(ctx, times->Ti_kick[ti], times->Ti_kick[ti] + dti / 2);
    if(ti < largest_active) {
        const int64_t lowerdti = dti_from_timebin(ti + 1);
        gravkick -= fn(ctx, times->Ti_kick[ti + 1], times->Ti_kick[ti + 1] + lowerdti / 2);
    }
    launch_kick_list(list, nlist, A->d_vel, accel ? accel : A->d_fulltree_accel, A->d_flags, gravkick, eng->stream);
}

static int hier_largest_active(const mpg_drift_kick_times *times, int *ti_out)
{
    int ti, largest_active = MPG_TIMEBINS;
    for(ti = MPG_TIMEBINS; ti >= 0; ti--)
        if(is_timebin_active(ti, times->Ti_Current) && dti_from_timebin(ti) <= times->PM_length) {
            largest_active = ti;
            break;
        }
    if(ti_out)
        *ti_out = ti;
    return largest_active;
}

// timebinmgr.c:372-417 on the host
static double host_dloga_interval(const mpg_timeline *tl, int64_t ti)
{
    const int64_t lastsnap = ti >> MPG_TIMEBINS;
    if(lastsnap >= tl->nsync - 1)
        return 0;
    return (tl->loga[lastsnap + 1] - tl->loga[lastsnap]) / (double)(1ull << MPG_TIMEBINS);
}
static double host_loga_from_ti(const mpg_timeline *tl, int64_t ti)
{
    const int64_t lastsnap = ti >> MPG_TIMEBINS;
    MPG_CHECK(lastsnap >= 0 && lastsnap < tl->nsync, "loga_from_ti: Ti_Current beyond the last sync point");
    const int64_t dti = ti & (((int64_t)1 << MPG_TIMEBINS) - 1);
    return tl->loga[lastsnap] + dti * host_dloga_interval(tl, ti);
}
static int64_t host_ti_from_loga(const mpg_timeline *tl, double loga)
{
    int64_t i;
    for(i = 1; i < tl->nsync - 1; i++)
        if(tl->loga[i] > loga)
            break;
    const double logDTime = (tl->loga[i] - tl->loga[i - 1]) / (double)(1ull << MPG_TIMEBINS);
    int64_t ti = (i - 1) << MPG_TIMEBINS;
    ti = (int64_t)((double)ti + (loga - tl->loga[i - 1]) / logDTime);
    return ti;
}

// What a step-assignment call hands its kernels: the scalars of the step and, behind the timeline in hier_sp, get_dloga_for_bin of every
// bin (timebinmgr.c:443-447; null when not asked for).  The uploads are queued on the engine's stream.
struct StepContext {
    StepScalars S;
    const double *d_bins;
};
static StepContext step_context(mpg_engine *eng, const mpg_drift_kick_times *times, const mpg_timeline *timeline, const mpg_timestep_params *par,
                                double atime, double hubble, double CourantFac, int64_t dti_max, bool want_bins)
{
    StepContext C{};
    eng->hier_sp.reserve((size_t)timeline->nsync + MPG_TIMEBINS + 2);
    MPG_HIP(hipMemcpyAsync(eng->hier_sp.p, timeline->loga, (size_t)timeline->nsync * sizeof(double), hipMemcpyHostToDevice, eng->stream));
    if(want_bins) {
        double bins[MPG_TIMEBINS + 1];
        const double logDTime = host_dloga_interval(timeline, times->Ti_Current);
        for(int b = 0; b <= MPG_TIMEBINS; b++)
            bins[b] = (double)dti_from_timebin(b) * logDTime;
        double *d_bins = eng->hier_sp.p + timeline->nsync;
        MPG_HIP(hipMemcpyAsync(d_bins, bins, sizeof(bins), hipMemcpyHostToDevice, eng->stream));
        C.d_bins = d_bins;
    }
    HierTimeline &T = C.S.T;
    T.sp = eng->hier_sp.p;
    T.nsync = (int)timeline->nsync;
    T.loga_cur = host_loga_from_ti(timeline, times->Ti_Current);
    T.ti0 = host_ti_from_loga(timeline, T.loga_cur);
    T.MinSizeTimestep = par->MinSizeTimestep;
    C.S.atime = atime;
    C.S.hubble = hubble;
    C.S.errtol = par->ErrTolIntAccuracy;
    C.S.soft = 2.8 * eng->GravitySoftening; // FORCE_SOFTENING
    C.S.courant = CourantFac;
    C.S.fac3 = pow(atime, 3 * (1 - 5.0 / 3.0) / 2.0); // timestep.c:1083, GAMMA = 5/3 (physconst.h:35)
    C.S.dti_max = dti_max;
    C.S.Ti_Current = times->Ti_Current;
    return C;
}

// is_PM_timestep (timestep.c:153-159) and, on a PM step, the new PM step of the caller's get_PM_timestep_ti (timestep.c:303-309, 748-755)
// entered in `times`; dti_max is the longest step a particle may take
struct PMStep {
    bool isPM;
    int64_t dti_max;
};
static PMStep pm_step_rule(mpg_drift_kick_times *times, int64_t dti_max_pm)
{
    MPG_CHECK(times->Ti_Current <= times->PM_start + times->PM_length, "Passed end of PM step!");
    PMStep pm{times->Ti_Current == times->PM_start + times->PM_length, times->PM_length};
    if(pm.isPM) {
        pm.dti_max = dti_max_pm;
        times->PM_length = pm.dti_max;
        times->PM_start = times->PM_kick;
    }
    return pm;
}

// the counter round trip of a step-assignment kernel: the k initial words of h up into hier_cnt, launch(hier_cnt), the k words back into h
// with the stream synchronised
template <class Launch> static void counted_launch(mpg_engine *eng, unsigned long long *h, int k, Launch &&launch)
{
    eng->hier_cnt.reserve(64);
    MPG_HIP(hipMemcpyAsync(eng->hier_cnt.p, h, k * sizeof(*h), hipMemcpyHostToDevice, eng->stream));
    launch(eng->hier_cnt.p);
    MPG_HIP(hipMemcpyAsync(h, eng->hier_cnt.p, k * sizeof(*h), hipMemcpyDeviceToHost, eng->stream));
    MPG_HIP(hipStreamSynchronize(eng->stream));
}

__global__ void __launch_bounds__(256) k_set_bh_bins(int64_t n, const uint8_t *__restrict__ type, uint8_t *__restrict__ tb, int bin)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if(i < n && (type[i] & 7) == 5)
        tb[i] = (uint8_t)bin;
}

extern "C" {

int mpg_dev_drift_all_particles(mpg_engine *eng, int64_t n, double *d_pos, const double *d_vel, const unsigned char *d_type,
                                const unsigned char *d_flags, double *d_hsml, const double *d_dthsml, double ddrift, double BoxSize,
                                const double random_shift[3])
{
    API_BEGIN
    MPG_CHECK(eng && d_pos && d_vel && random_shift && n >= 0, "null argument");
    MPG_CHECK(!d_hsml || (d_dthsml && d_type), "drift: Hsml needs DtHsml and Type");
    MPG_HIP(hipSetDevice(eng->device));
    eng->pm_queued = false; // positions move: a tree build that follows must stay behind this on the main stream
    flagged_launch(eng, "drift: a particle has Hsml <= 0 or a non-finite position (drift.c:62-75)", [&](unsigned *err) {
        launch_drift(n, d_pos, d_vel, d_type, d_flags, d_hsml, d_dthsml, ddrift, BoxSize, random_shift, err, eng->stream);
    });
    API_END
}

int mpg_dev_apply_pm_half_kick(mpg_engine *eng, int64_t n, double *d_vel, const double *d_gravpm, const unsigned char *d_flags, double Fgravkick)
{
    API_BEGIN
    MPG_CHECK(eng && d_vel && d_gravpm && n >= 0, "null argument");
    MPG_HIP(hipSetDevice(eng->device));
    launch_pm_half_kick(n, d_vel, d_gravpm, d_flags, Fgravkick, eng->stream);
    API_END
}

int mpg_dev_apply_half_kick(mpg_engine *eng, int64_t n, const int *d_active, int64_t nactive, double *d_vel, const double *d_gravaccel,
                            const unsigned char *d_type, const unsigned char *d_flags, const unsigned char *d_tb_grav,
                            const unsigned char *d_tb_hydro, const double *d_hydroaccel, double *d_entropy, const double *d_dtentropy,
                            const mpg_kick_factors *K)
{
    API_BEGIN
    MPG_CHECK(eng && d_vel && d_gravaccel && K && n >= 0, "null argument");
    MPG_CHECK(!d_type || (d_hydroaccel && d_entropy && d_dtentropy), "half kick: gas needs HydroAccel, Entropy and DtEntropy");
    MPG_HIP(hipSetDevice(eng->device));
    flagged_launch(eng, "half kick: a particle has an unexpected time bin (timestep.c:900-901)", [&](unsigned *err) {
        launch_half_kick(n, d_active, nactive, d_vel, d_gravaccel, d_type, d_flags, d_tb_grav, d_tb_hydro, d_hydroaccel, d_entropy, d_dtentropy, *K, err,
                         eng->stream);
    });
    API_END
}

int mpg_dev_apply_hydro_half_kick(mpg_engine *eng, int64_t n, const int *d_active, int64_t nactive, double *d_vel, const unsigned char *d_type,
                                  const unsigned char *d_flags, const unsigned char *d_tb_hydro, const double *d_hydroaccel, double *d_entropy,
                                  const double *d_dtentropy, const mpg_kick_factors *K)
{
    API_BEGIN
    MPG_CHECK(eng && d_vel && d_type && d_hydroaccel && d_entropy && d_dtentropy && K && n >= 0 && nactive >= 0, "null argument");
    MPG_HIP(hipSetDevice(eng->device));
    flagged_launch(eng, "hydro half kick: a particle has an unexpected hydro time bin (> TIMEBINS)", [&](unsigned *err) {
        launch_hydro_half_kick(n, d_active, nactive, d_vel, d_type, d_flags, d_tb_hydro, d_hydroaccel, d_entropy, d_dtentropy, *K, err, eng->stream);
    });
    API_END
}

int mpg_dev_apply_bh_subgrid_kick(mpg_engine *eng, int64_t n, const int *d_active, int64_t nactive, double *d_vel, const unsigned char *d_type,
                                  const unsigned char *d_flags, const unsigned char *d_tb_hydro, const double *d_dfaccel, const double *d_dragaccel,
                                  const mpg_kick_factors *K)
{
    API_BEGIN
    MPG_CHECK(eng && d_vel && d_type && d_dfaccel && d_dragaccel && K && n >= 0 && nactive >= 0, "null argument");
    MPG_HIP(hipSetDevice(eng->device));
    flagged_launch(eng, "black-hole sub-grid kick: a black hole has an unexpected hydro time bin (> TIMEBINS)", [&](unsigned *err) {
        launch_bh_subgrid_kick(n, d_active, nactive, d_vel, d_type, d_flags, d_tb_hydro, d_dfaccel, d_dragaccel, *K, err, eng->stream);
    });
    API_END
}

int mpg_dev_reposition_blackholes(mpg_engine *eng, int64_t n, double *d_pos, double *d_vel, const unsigned char *d_type, const unsigned char *d_flags,
                                  int32_t *d_jumptominpot, const double *d_minpotpos, const double *d_minpotvel, double BoxSize)
{
    API_BEGIN
    MPG_CHECK(eng && d_pos && d_vel && d_type && d_jumptominpot && d_minpotpos && d_minpotvel && n >= 0 && BoxSize > 0, "null argument");
    MPG_HIP(hipSetDevice(eng->device));
    flagged_launch(eng, "reposition: drifting a black hole very far (more than 0.1 BoxSize to its potential minimum): the time step is too sparse",
                   [&](unsigned *err) {
                       launch_reposition_blackholes(n, d_pos, d_vel, d_type, d_flags, d_jumptominpot, d_minpotpos, d_minpotvel, BoxSize, err, eng->stream);
                   });
    API_END
}

int mpg_dev_timestep_gravity_dloga(mpg_engine *eng, int64_t n, const double *d_gravaccel, const double *d_gravpm, double atime, double hubble,
                                   double ErrTolIntAccuracy, double *d_dloga)
{
    API_BEGIN
    MPG_CHECK(eng && d_gravaccel && d_gravpm && d_dloga && n >= 0, "null argument");
    MPG_CHECK(eng->GravitySoftening > 0, "timestep: gravshort_set_softenings has not been called");
    MPG_HIP(hipSetDevice(eng->device));
    launch_timestep_gravity(n, d_gravaccel, d_gravpm, atime, hubble, ErrTolIntAccuracy, 2.8 * eng->GravitySoftening, d_dloga, eng->stream);
    API_END
}

int mpg_dev_timestep_hydro_dloga(mpg_engine *eng, int64_t n, const unsigned char *d_type, const double *d_hsml, const double *d_dthsml,
                                 const double *d_maxsignalvel, const unsigned char *d_bh_mintimebin, const double *dloga_for_bin, double atime,
                                 double hubble, double CourantFac, double *d_dloga, unsigned char *d_titype)
{
    API_BEGIN
    MPG_CHECK(eng && d_dloga && n >= 0, "null argument");
    MPG_CHECK(!d_type || (d_hsml && d_maxsignalvel), "timestep_hydro_dloga: gas needs Hsml and MaxSignalVel");
    MPG_HIP(hipSetDevice(eng->device));
    const double *d_bins = nullptr;
    if(d_bh_mintimebin && dloga_for_bin) {
        eng->hier_sp.reserve((size_t)MPG_TIMEBINS + 2);
        MPG_HIP(hipMemcpyAsync(eng->hier_sp.p, dloga_for_bin, (MPG_TIMEBINS + 1) * sizeof(double), hipMemcpyHostToDevice, eng->stream));
        d_bins = eng->hier_sp.p;
    }
    const double fac3 = pow(atime, 3 * (1 - 5.0 / 3.0) / 2.0); // timestep.c:1083, GAMMA = 5/3 (physconst.h:35)
    launch_timestep_hydro(n, d_type, d_hsml, d_dthsml, d_maxsignalvel, d_bins ? d_bh_mintimebin : nullptr, d_bins, atime, hubble, CourantFac, fac3,
                          d_dloga, d_titype, eng->stream);
    if(d_bins)
        MPG_HIP(hipStreamSynchronize(eng->stream)); // (the table sits in a scratch buffer the hierarchical loop shares)
    API_END
}

int mpg_dev_build_active_sublist(mpg_engine *eng, const int *d_active, int64_t NumActiveParticle, const unsigned char *d_tb_grav,
                                 const unsigned char *d_flags, int maxtimebin, int64_t Ti_Current, int *d_out, int64_t *n_out)
{
    API_BEGIN
    MPG_CHECK(eng && d_tb_grav && d_out && n_out && NumActiveParticle >= 0, "null argument");
    MPG_HIP(hipSetDevice(eng->device));
    *n_out = hier_sublist(eng, d_active, NumActiveParticle, d_tb_grav, d_flags, maxtimebin, Ti_Current, d_out);
    API_END
}

int mpg_dev_find_hydro_timesteps(mpg_engine *eng, const mpg_hydrostep_arrays *A, const int *d_active, int64_t NumActiveParticle,
                                 const mpg_drift_kick_times *times, const mpg_timeline *timeline, const mpg_timestep_params *par, double CourantFac,
                                 double atime, double hubble, mpg_hydrostep_result *out)
{
    API_BEGIN
    MPG_CHECK(eng && A && times && timeline && par && out, "null argument");
    MPG_CHECK(A->d_tb_hydro, "find_hydro_timesteps: TimeBinHydro is needed");
    MPG_CHECK(!A->d_type || (A->d_hsml && A->d_maxsignalvel), "find_hydro_timesteps: gas needs Hsml and MaxSignalVel");
    MPG_CHECK(timeline->nsync >= 2 && timeline->loga, "find_hydro_timesteps: the timeline needs at least two sync points");
    MPG_HIP(hipSetDevice(eng->device));
    const int64_t nact = d_active ? NumActiveParticle : eng->n;
    const StepContext C = step_context(eng, times, timeline, par, atime, hubble, CourantFac, times->PM_length, true);
    unsigned long long h[8] = {0, 0, 0, 0, 0, 0, 0, (unsigned long long)MPG_TIMEBINS};
    counted_launch(eng, h, 8, [&](unsigned long long *d_cnt) {
        launch_find_hydro_timesteps(d_active, nact, A->d_type, A->d_flags, A->d_hsml, A->d_dthsml, A->d_maxsignalvel, A->d_bh_mintimebin, C.d_bins,
                                    A->d_tb_grav, A->d_tb_hydro, C.S, d_cnt, eng->stream);
    });
    for(int k = 0; k < 5; k++)
        out->ntitype[k] = (int64_t)h[k];
    out->badstepsizecount = (int64_t)h[5];
    out->badtimebins = (int64_t)h[6];
    out->mTimeBin = (int)h[7];
    API_END
}

// the dynamic-friction bins of the black holes (timestep.c:676-691), after mpg_dev_find_hydro_timesteps: it reads the new hydro bin
int mpg_dev_find_dynfric_timesteps(mpg_engine *eng, const mpg_dynfricstep_arrays *A, const int *d_active, int64_t NumActiveParticle,
                                   const mpg_drift_kick_times *times, const mpg_timeline *timeline, const mpg_timestep_params *par, double CourantFac,
                                   double atime, double hubble, mpg_dynfricstep_result *out)
{
    API_BEGIN
    MPG_CHECK(eng && A && times && timeline && par && out, "null argument");
    MPG_CHECK(A->d_type && A->d_vel && A->d_df_vel && A->d_hsml && A->d_tb_hydro && A->d_tb_dynfric,
              "find_dynfric_timesteps: the arrays type, vel, df_vel, hsml, tb_hydro and tb_dynfric are needed");
    MPG_CHECK(timeline->nsync >= 2 && timeline->loga, "find_dynfric_timesteps: the timeline needs at least two sync points");
    MPG_HIP(hipSetDevice(eng->device));
    const int64_t nact = d_active ? NumActiveParticle : eng->n;
    const StepContext C = step_context(eng, times, timeline, par, atime, hubble, CourantFac, times->PM_length, false);
    unsigned long long h[3] = {0, 0, 0};
    counted_launch(eng, h, 3, [&](unsigned long long *d_cnt) {
        launch_find_dynfric_timesteps(d_active, nact, A->d_type, A->d_flags, A->d_vel, A->d_df_vel, A->d_hsml, A->d_dthsml, A->d_tb_grav, A->d_tb_hydro,
                                      A->d_tb_dynfric, C.S, d_cnt, eng->stream);
    });
    out->dynratio = (int64_t)h[0];
    out->maxdyndiff = (int)h[1];
    out->nbh = (int64_t)h[2];
    API_END
}

// find_timesteps (timestep.c:739-849), the step assignment of a run without SplitGravityTimestepsOn (run.c:756): the particle loop on the
// device; the PM step (get_PM_timestep_ti) comes from the caller, the shrink of the PM step onto the longest tree step and
// times->mintimebin / maxtimebin are done here as the reference does (one rank; several ranks reduce `out` first and call
// mpg_find_timesteps_finish)
int mpg_dev_find_timesteps(mpg_engine *eng, const mpg_hydrostep_arrays *A, const double *d_fulltree_accel, const double *d_gravpm,
                           unsigned char *d_tb_grav, const int *d_active, int64_t NumActiveParticle, mpg_drift_kick_times *times,
                           const mpg_timeline *timeline, const mpg_timestep_params *par, double CourantFac, double atime, double hubble,
                           int64_t dti_max_pm, mpg_timestep_result *out)
{
    API_BEGIN
    MPG_CHECK(eng && A && times && timeline && par && out && d_fulltree_accel && d_gravpm && d_tb_grav, "null argument");
    MPG_CHECK(A->d_tb_hydro, "find_timesteps: TimeBinHydro is needed");
    MPG_CHECK(!A->d_type || (A->d_hsml && A->d_maxsignalvel), "find_timesteps: gas needs Hsml and MaxSignalVel");
    MPG_CHECK(timeline->nsync >= 2 && timeline->loga, "find_timesteps: the timeline needs at least two sync points");
    MPG_CHECK(eng->GravitySoftening > 0, "timestep: gravshort_set_softenings has not been called");
    MPG_HIP(hipSetDevice(eng->device));
    const int64_t nact = d_active ? NumActiveParticle : eng->n;
    const PMStep pm = pm_step_rule(times, dti_max_pm);
    const StepContext C = step_context(eng, times, timeline, par, atime, hubble, CourantFac, pm.dti_max, true);
    unsigned long long h[9] = {0, 0, 0, 0, 0, 0, 0, (unsigned long long)MPG_TIMEBINS, 0};
    counted_launch(eng, h, 9, [&](unsigned long long *d_cnt) {
        launch_find_timesteps(d_active, nact, A->d_type, A->d_flags, d_fulltree_accel, d_gravpm, A->d_hsml, A->d_dthsml, A->d_maxsignalvel,
                              A->d_bh_mintimebin, C.d_bins, d_tb_grav, A->d_tb_hydro, C.S, d_cnt, eng->stream);
    });
    for(int k = 0; k < 5; k++)
        out->ntitype[k] = (int64_t)h[k];
    out->badstepsizecount = (int64_t)h[5];
    out->badtimebins = (int64_t)h[6];
    out->mTimeBin = (int)h[7];
    out->maxTimeBin = (int)h[8];
    out->isPM = pm.isPM ? 1 : 0;
    API_END
}

// the tail of find_timesteps (timestep.c:825-848) with the all-reduced smallest / largest bin
int mpg_find_timesteps_finish(int mTimeBin, int maxTimeBin, int isPM, mpg_drift_kick_times *times)
{
    API_BEGIN
    MPG_CHECK(times, "null argument");
    if(isPM && times->PM_length > dti_from_timebin(maxTimeBin))
        times->PM_length = dti_from_timebin(maxTimeBin);
    times->mintimebin = mTimeBin;
    times->maxtimebin = maxTimeBin;
    API_END
}

int mpg_dev_hydro_timesteps_finish(mpg_engine *eng, int mTimeBin, int isFirstTimeStep, int64_t n, const unsigned char *d_type,
                                   unsigned char *d_tb_hydro, mpg_drift_kick_times *times)
{
    API_BEGIN
    MPG_CHECK(eng && times, "null argument");
    // all gas of the shortest bin turned into stars: keep the step, or lengthen it if the next bin is active (timestep.c:709-715)
    if(!is_timebin_active(mTimeBin, times->Ti_Current)) {
        mTimeBin = times->mintimebin;
        if(is_timebin_active(mTimeBin + 1, times->Ti_Current))
            mTimeBin++;
    }
    if(isFirstTimeStep && d_type && d_tb_hydro && n > 0) { // set_bh_first_timestep, timestep.c:600-612
        MPG_HIP(hipSetDevice(eng->device));
        hipLaunchKernelGGL(k_set_bh_bins, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, eng->stream, n, d_type, d_tb_hydro, mTimeBin);
        MPG_HIP(hipGetLastError());
    }
    times->mintimebin = mTimeBin;
    if(times->mintimebin > times->mingravtimebin && times->mingravtimebin > 0) // (a dark-matter particle in the shortest bin)
        times->mintimebin = times->mingravtimebin;
    API_END
}

int mpg_dev_hierarchical_gravity_and_timesteps(mpg_engine *eng, const mpg_hiergrav_arrays *A, const int *d_active, int64_t NumActiveParticle,
                                               int64_t NumActiveGravity, mpg_drift_kick_times *times, const mpg_timeline *timeline,
                                               const mpg_timestep_params *par, double atime, double hubble, int64_t dti_max_pm, double rho0,
                                               int HybridNuGrav, mpg_gravkick_fn gravkick, void *gravkick_ctx, int64_t *badstepsizecount)
{
    API_BEGIN
    MPG_CHECK(eng && A && times && timeline && par && gravkick && badstepsizecount, "null argument");
    MPG_CHECK(A->d_vel && A->d_gravpm && A->d_fulltree_accel && A->d_tb_grav, "hierarchical gravity: Vel, GravPM, FullTreeGravAccel and TimeBinGravity are needed");
    MPG_CHECK(timeline->nsync >= 2 && timeline->loga, "hierarchical gravity: the timeline needs at least two sync points");
    MPG_CHECK(eng->GravitySoftening > 0, "timestep: gravshort_set_softenings has not been called");
    MPG_HIP(hipSetDevice(eng->device));
    const int64_t n = eng->n;
    const int64_t nact = d_active ? NumActiveParticle : n;
    const PMStep pm = pm_step_rule(times, dti_max_pm);
    int largest_active = hier_largest_active(times, nullptr);
    // the gravitationally active particles (timestep.c:323-328)
    eng->hier_list[0].reserve((size_t)nact + 1);
    eng->hier_list[1].reserve((size_t)nact + 1);
    const int *sub = d_active;
    int64_t nsub = nact;
    int cur = 0; // hier_list[cur] is free
    if(!(NumActiveGravity == NumActiveParticle || pm.isPM)) {
        nsub = hier_sublist(eng, d_active, nact, A->d_tb_grav, A->d_flags, largest_active, times->Ti_Current, eng->hier_list[0].p);
        sub = eng->hier_list[0].p;
        cur = 1;
    }
    const StepScalars S = step_context(eng, times, timeline, par, atime, hubble, 0, pm.dti_max, false).S; // (no hydro criterion: no CourantFac)
    // new gravity bins from the acceleration of the longest step (timestep.c:345-370)
    eng->hier_cnt.reserve(64);
    MPG_HIP(hipMemsetAsync(eng->hier_cnt.p, 0, 64 * sizeof(unsigned long long), eng->stream));
    const double *topacc = A->d_stored_accel ? A->d_stored_accel : A->d_fulltree_accel;
    launch_assign_gravity_bins(sub, nsub, topacc, A->d_gravpm, A->d_flags, S, largest_active, A->d_tb_grav, eng->hier_cnt.p, eng->hier_cnt.p + 48,
                               eng->stream);
    unsigned long long hc[49];
    MPG_HIP(hipMemcpyAsync(hc, eng->hier_cnt.p, sizeof(hc), hipMemcpyDeviceToHost, eng->stream));
    MPG_HIP(hipStreamSynchronize(eng->stream));
    int64_t counts[MPG_TIMEBINS + 1];
    for(int b = 0; b <= MPG_TIMEBINS; b++)
        counts[b] = (int64_t)hc[b];
    int64_t bad = (int64_t)hc[48];
    // largest bin with particles (timestep.c:379-385)
    for(int ti = largest_active; ti >= 1; ti--)
        if(counts[ti] > 0) {
            largest_active = ti;
            break;
        }
    // push the top bin down where it holds too few particles (PM steps only, timestep.c:392-413)
    int push_down_bin = largest_active;
    if(pm.isPM) {
        for(int ti = largest_active; ti >= 1; ti--) {
            if(counts[ti] / 3 > counts[ti - 1])
                break;
            push_down_bin = ti - 1;
            counts[ti - 1] += counts[ti];
        }
    }
    MPG_CHECK(push_down_bin != 0, "Bad timestep: every particle wants the shortest bin");
    if(push_down_bin != largest_active) {
        launch_push_down_bins(sub, nsub, push_down_bin, A->d_tb_grav, eng->stream);
        largest_active = push_down_bin;
    }
    times->maxtimebin = largest_active;
    // the kick of the topmost bin (timestep.c:417)
    hier_kick(eng, A, sub, nsub, A->d_stored_accel, times, largest_active, largest_active, gravkick, gravkick_ctx);
    // all lower bins (timestep.c:433-490)
    eng->hier_accel.reserve(3 * (size_t)n + 3);
    MPG_HIP(hipMemsetAsync(eng->hier_cnt.p + 48, 0, sizeof(unsigned long long), eng->stream));
    const int *last = sub;
    int64_t nlast = nsub;
    for(int ti = largest_active - 1; ti > 0; ti--) {
        int *subl = eng->hier_list[cur].p;
        const int64_t ns = hier_sublist(eng, last, nlast, A->d_tb_grav, A->d_flags, ti, times->Ti_Current, subl);
        if(ns == 0) {
            times->mingravtimebin = ti + 1;
            break;
        }
        hier_tree_and_walk(eng, A, subl, ns, eng->hier_accel.p, rho0, HybridNuGrav);
        launch_level_gravity_bins(subl, ns, eng->hier_accel.p, A->d_gravpm, A->d_flags, S, ti, A->d_tb_grav, eng->hier_cnt.p + 48, eng->stream);
        hier_kick(eng, A, subl, ns, eng->hier_accel.p, times, ti, largest_active, gravkick, gravkick_ctx);
        last = subl;
        nlast = ns;
        cur ^= 1;
    }
    times->mintimebin = times->mingravtimebin;
    unsigned long long b2 = 0;
    MPG_HIP(hipMemcpyAsync(&b2, eng->hier_cnt.p + 48, sizeof(b2), hipMemcpyDeviceToHost, eng->stream));
    MPG_HIP(hipStreamSynchronize(eng->stream));
    *badstepsizecount = bad + (int64_t)b2;
    API_END
}

int mpg_dev_hierarchical_gravity_accelerations(mpg_engine *eng, const mpg_hiergrav_arrays *A, const int *d_active, int64_t NumActiveParticle,
                                               int64_t NumActiveGravity, mpg_drift_kick_times *times, double rho0, int HybridNuGrav,
                                               mpg_gravkick_fn gravkick, void *gravkick_ctx)
{
    API_BEGIN
    MPG_CHECK(eng && A && times && gravkick, "null argument");
    MPG_CHECK(A->d_vel && A->d_gravpm && A->d_fulltree_accel && A->d_tb_grav, "hierarchical gravity: Vel, GravPM, FullTreeGravAccel and TimeBinGravity are needed");
    MPG_HIP(hipSetDevice(eng->device));
    const int64_t n = eng->n;
    const int64_t nact = d_active ? NumActiveParticle : n;
    int ti = 0;
    const int largest_active = hier_largest_active(times, &ti);
    eng->hier_list[0].reserve((size_t)nact + 1);
    eng->hier_list[1].reserve((size_t)nact + 1);
    eng->hier_accel.reserve(3 * (size_t)n + 3);
    const int *last = d_active;
    int64_t nlast = nact, last_grav = NumActiveGravity;
    int cur = 0;
    if(NumActiveGravity != NumActiveParticle) { // some particles are only hydro active (timestep.c:520-524)
        nlast = hier_sublist(eng, d_active, nact, A->d_tb_grav, A->d_flags, ti, times->Ti_Current, eng->hier_list[0].p);
        last = eng->hier_list[0].p;
        last_grav = nlast;
        cur = 1;
    }
    // all currently active particles: into StoredGravAccel (or, without it, a scratch array: only a full tree then leaves a
    // result, in FullTreeGravAccel, as in the reference where grav_short_tree allocates the array itself)
    hier_tree_and_walk(eng, A, last, nlast, A->d_stored_accel ? A->d_stored_accel : eng->hier_accel.p, rho0, HybridNuGrav);
    hier_kick(eng, A, last, nlast, A->d_stored_accel, times, ti, largest_active, gravkick, gravkick_ctx);
    const double *gravaccel = nullptr;
    for(ti = largest_active - 1; ti >= times->mingravtimebin; ti--) {
        int *subl = eng->hier_list[cur].p;
        const int64_t ns = hier_sublist(eng, last, nlast, A->d_tb_grav, A->d_flags, ti, times->Ti_Current, subl);
        if(ns != last_grav) { // (the same particles as one level up: the accelerations are the same, timestep.c:556-564)
            gravaccel = eng->hier_accel.p;
            hier_tree_and_walk(eng, A, subl, ns, eng->hier_accel.p, rho0, HybridNuGrav);
        }
        hier_kick(eng, A, subl, ns, gravaccel ? gravaccel : A->d_stored_accel, times, ti, largest_active, gravkick, gravkick_ctx);
        last = subl;
        nlast = ns;
        last_grav = ns;
        cur ^= 1;
    }
    API_END
}

} // extern "C"
