// blackhole.h -- black-hole accretion, mergers and feedback on the device tree (see blackhole.hip)
#pragma once
#include "../../include/mpgadget_hip.h"
#include "mpg_common.h"
#include "tree_build.h"

namespace mpg {

constexpr int BH_TIMEBINS = 46;  // TIMEBINS, timebinmgr.h:13: BH_minTimeBin of a target without unmarked gas inside Hsml
constexpr int BH_NACC = 4;       // accumulators per particle of the tree: injected energy, velocity kick[3]
constexpr int BH_NSTATS = 8;     // mpg_blackhole_get_stats

// device view of the caller's particle table and of mpg_blackhole_arrays (caller order, n entries each)
struct BhView {
    const double *pos;
    const uint8_t *type; // null: all type 1 (then there are no targets)
    mpg_blackhole_arrays a;
};

// what the walks read beside the arrays: mpg_blackhole_params with the derived constants, the random table, the call's own state
struct BhScalars {
    mpg_blackhole_params p;
    double merge_dist;   // 2 FORCE_SOFTENING / 2.8
    double a3inv;
    double meddington_fac; // M_Eddington = meddington_fac * BHP.Mass
    double c2;           // (LIGHTCGS / UnitVelocity_in_cm_per_s)^2
    double rho_sfr;      // BHKE_SfrCritOverDensity * rho_crit_baryon
    double ucap;         // 5e8 K as internal energy per mass
    int ktype;           // KERNELS[] index of the density kernel
    const double *rnd;   // RandTable.Table
    uint64_t rndsize;
};

// per-particle state of one call (n entries; zeroed or written per call for the targets)
struct BhState {
    unsigned long long *swal; // SPH_SwallowID / BH_SwallowID: ID + 1 of the swallower, 0 unmarked
    double *fws;              // BH_FeedbackWeightSum
    int *keflag;
};

struct BlackholeEngine {
    DevBuf<unsigned long long> swal;
    DevBuf<double> fws, hsml_t, acc;
    DevBuf<int> keflag, queue_0, queue_1;
    DevBuf<unsigned> ctr;
    DevBuf<unsigned long long> stats;
    DevBuf<double> rnd; // the random table (mpg_set_random_table)
    int64_t rndsize = 0;
    int64_t ntargets = 0, nfeedback = 0;
    int64_t last_stats[BH_NSTATS] = {0, 0, 0, 0, 0, 0, 0, 0};
    hipEvent_t ev[5] = {}; // around the accretion walk; before the feedback walk, between it and the apply pass, behind that pass ...
    float last_ms[3] = {0, 0, 0}; // ... and what they took (tools/blackhole_time.py)
    ~BlackholeEngine()
    {
        for(hipEvent_t e : ev)
            if(e)
                (void)hipEventDestroy(e);
    }
    void set_random_table(const double *table, int64_t size, hipStream_t st);
    // blackhole_haswork (blackhole.c:185-188) on the active particles, in particle order; returns the number of targets
    int64_t make_queue(const uint8_t *type, const uint8_t *active_flags, int64_t n, hipStream_t st);
    // both walks, their post-processes and the apply pass on the current tree (gas + black holes, with hmax)
    void run(TreeBuilder &tree, const BhView &A, const mpg_sph_times &T, const BhScalars &S, int64_t n, hipStream_t st);
    // type[i] = 7 for the rows whose flags carry IsGarbage or Swallowed: the type column of a staged or resident table after a call
    static void retype(uint8_t *type, const uint8_t *flags, int64_t n, hipStream_t st);
};

} // namespace mpg
