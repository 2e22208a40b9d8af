// winds.h -- the wind model: kicks from new stars, subgrid winds, the evolution of the delay time (see winds.hip)
#pragma once
#include "../../include/mpgadget_hip.h"
#include "mpg_common.h"
#include "tree_build.h"

namespace mpg {

constexpr int WIND_SUBGRID = 1, WIND_DECOUPLE_SPH = 2, WIND_USE_HALO = 4, WIND_FIXED_EFFICIENCY = 8, WIND_ISOTROPIC = 512; // enum WindModel, winds.h:13-20
constexpr int WD_NSTATS = 6; // mpg_winds_get_stats

#ifndef MPG_HD
#if defined(__HIPCC__) || defined(__CUDACC__)
#define MPG_HD __host__ __device__ inline
#else
#define MPG_HD inline
#endif
#endif
// winds_evolve, winds.c:374-391, in two parts, for k_wind_evolve and for the star-formation loop (sfr.hip).  Is the particle still in the
// wind once the density rule of :378-380 has been applied: only then is its time step read ...
MPG_HD bool wind_still_delayed(const mpg_wind_params &P, double delaytime, double density, double a3inv)
{
    return delaytime > 0 && !(density * a3inv < P.WindFreeTravelDensThresh);
}
// ... and its new DelayTime (dtime = dloga / hubble of its hydro bin, read by a particle that is still delayed only)
MPG_HD double wind_evolve_delay(const mpg_wind_params &P, double delaytime, double density, double a3inv, double dtime)
{
    if(delaytime > 0 && !wind_still_delayed(P, delaytime, density, a3inv))
        return 0;
    if(delaytime > 0) {
        if(delaytime > P.MaxWindFreeTravelTime)
            delaytime = P.MaxWindFreeTravelTime;
        delaytime = delaytime - dtime > 0 ? delaytime - dtime : 0; // DMAX
    }
    return delaytime;
}

// device view of the caller's particle table and of mpg_wind_arrays (caller order, n entries each)
struct WindView {
    const double *pos;
    const float *mass;   // the caller's CURRENT column, not the tree-order copy of the last build
    const uint8_t *type; // null: all type 1 (then every listed row is an error)
    int64_t n;
    mpg_wind_arrays a;
};

// what the kernels read beside the arrays: struct WindParams, the time, the random table
struct WindScalars {
    mpg_wind_params p;
    double atime;
    const double *rnd; // RandTable.Table
    uint64_t rndsize;
};

// a potential kick (struct StarKick, winds.c:178-190): the kick velocity and the thermal energy follow from the star
struct alignas(16) WindKick {
    int star; // particle index of the star
    int slot; // tree slot of the gas particle
    double r; // StarDistance; after the apply pass of the entry that was applied: its kick velocity
};

struct WindsEngine {
    DevBuf<double> weight;             // TotalWeight per row of the star list
    DevBuf<unsigned> count, offset;    // per row of the star list: its eligible neighbours, the start of its segment of the kick list
    DevBuf<WindKick> kicks;            // the potential kicks of the last call, a segment per star; star = -1: unused entry
    int64_t last_capacity = 0;         // entries of the list of the last call
    DevBuf<unsigned long long> rmin;   // per gas particle of the tree: the bits of the smallest StarDistance among its potential kicks ...
    DevBuf<unsigned long long> win;    // ... and the smallest StarID among those at that distance
    DevBuf<unsigned> ctr;
    DevBuf<unsigned long long> stats;
    int64_t last_stats[WD_NSTATS] = {0, 0, 0, 0, 0, 0};
    double last_maxvel = 0;
    hipEvent_t ev[4] = {}; // around the weight walk; before the feedback walk, between it and the resolve pass, behind the apply pass ...
    float last_ms[3] = {0, 0, 0}; // ... and what they took (tools/winds_time.py)
    ~WindsEngine()
    {
        for(hipEvent_t e : ev)
            if(e)
                (void)hipEventDestroy(e);
    }
    void reset();
    // the listed rows are stars inside the table (winds.c:406-407), checked before anything is written
    void check_stars(const WindView &A, const int *d_newstars, int64_t nnew, hipStream_t st);
    // both walks, the nearest-star rule and the kicks on the current tree (which holds the gas)
    void run(TreeBuilder &tree, const WindView &A, const WindScalars &S, const int *d_newstars, int64_t nnew, hipStream_t st);
    // winds_subgrid / winds_make_after_sf for the listed gas (d_list NULL: rows 0 .. n - 1)
    void subgrid(const WindView &A, const WindScalars &S, const int *d_list, int64_t nlist, const double *d_stellarmass, hipStream_t st);
    // winds_evolve for the listed gas (d_list NULL: every row)
    void evolve(const WindView &A, const WindScalars &S, const mpg_sph_times &T, const int *d_list, int64_t nlist, hipStream_t st);
};

} // namespace mpg
