// dynfric.h -- black-hole dynamical friction and the potential minimum of repositioning on the device tree (see dynfric.hip)
#pragma once
#include "../../include/mpgadget_hip.h"
#include "mpg_common.h"
#include "tree_build.h"

namespace mpg {

constexpr int DF_NSTATS = 5; // mpg_bh_dynfric_get_stats
constexpr int DF_NRAW = 5;   // raw sums per particle: sum m wk, sum m wk v[3], sum m wk v^2

// device view of the caller's particle table and of mpg_bh_dynfric_arrays (caller order, n entries each)
struct DfView {
    const double *pos;
    const float *mass;   // P.Mass of the bound table
    const uint8_t *type; // null: all type 1 (then there are no targets)
    mpg_bh_dynfric_arrays a;
};

struct DfScalars {
    mpg_bh_dynfric_params p;
    int ktype; // KERNELS[] index of the density kernel
};

// per-particle state of one call (n entries, written for the targets): what the tests read back through mpg_bh_dynfric_export
struct DfState {
    double *raw; // [n][DF_NRAW] the sums before the post-process
    int *minidx; // particle of the smallest potential, -1: no neighbour lower than the target
    int *numngb; // tree particles inside Hsml
};

struct DynfricEngine {
    DevBuf<double> raw, zeromass;
    DevBuf<int> minidx, numngb, queue_t, queue_bh;
    DevBuf<unsigned> ctr;
    DevBuf<unsigned long long> stats;
    int64_t n_state = -1; // particles the per-target arrays were last written for
    int64_t ntargets = 0, nlisted = 0;
    int64_t last_stats[DF_NSTATS] = {0, 0, 0, 0, 0};
    double last_zeromass = 0;
    hipEvent_t ev[3] = {}; // around the walk, behind the DFAccel pass ...
    float last_ms[2] = {0, 0}; // ... and what they took (tools/dynfric_time.py)
    ~DynfricEngine()
    {
        for(hipEvent_t e : ev)
            if(e)
                (void)hipEventDestroy(e);
    }
    void reset() // the statistics of a call that does nothing
    {
        for(int64_t &s : last_stats)
            s = 0;
        last_zeromass = 0;
        last_ms[0] = last_ms[1] = 0;
        ntargets = nlisted = 0;
        n_state = -1;
    }
    DfState state() { return DfState{raw.p, minidx.p, numngb.p}; }
    // the listed black holes (queue_bh: blackhole_dfaccel's loop) and, among them, the targets of the walk (queue_t:
    // blackhole_dynfric_haswork, or every listed black hole when only the potential minimum is searched); returns the number of targets
    int64_t make_queues(const uint8_t *type, const uint8_t *active_flags, const uint8_t *active_dynfric, int method, int64_t n, hipStream_t st);
    // the walk with its post-process over queue_t on the current tree
    void walk(TreeBuilder &tree, const DfView &A, const mpg_sph_times &T, const DfScalars &S, int64_t n, hipStream_t st);
    // blackhole_compute_dfaccel over queue_bh
    void dfaccel(const DfView &A, const mpg_sph_times &T, const DfScalars &S, hipStream_t st);
};

} // namespace mpg
