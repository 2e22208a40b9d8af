// metals.h -- stellar mass and metal return to the gas on the device tree (see metals.hip)
#pragma once
#include "mpg_common.h"
#include "tree_build.h"
#include <vector>

namespace mpg {

constexpr int NHSML = 10;       // trial radii per iteration of stellar_density, metal_return.c:733
constexpr int NMETALS = 9;      // metal species per particle, slotsmanager.h
constexpr int MT_MAXITER = 400; // MAXITER, treewalk.h:214

// device view of the caller's particle table and of mpg_metal_arrays (caller order, n entries each)
struct MetalView {
    const double *pos;
    const uint8_t *type; // null: all type 1 (then there are no targets)
    const double *massgenerated, *metalgenerated, *speciesgenerated, *stellarage;
    float *mass;
    double *hsml, *totalmassreturned, *lastenrichment;
    double *density, *metallicity, *metals;
    double *massreturned, *starvolume; // optional outputs
};

// per-target state of the radius loop (struct StellarDensityPriv, metal_return.c:755-767) and what the tests read back, by particle
struct MetalState {
    double *Left, *Right;
    double *Volume;     // VolumeSPH[0] after the last pass: the volume at trial radius `close`
    double *evalradius; // the trial radius the last pass took its sums at (evalhsml[close])
    int *niter, *maxcmpte, *close;
};

struct MetalScalars {
    double box;
    double desnumngb;  // GetNumNgb(GetDensityKernelType())
    double maxdev;     // MetalParams.MaxNgbDeviation
    double maxgasmass; // 4 AvgGasMass
    int sphweight;     // MetalParams.SPHWeighting
    int ktype;         // KERNELS[] index of the density kernel
};

// tree-ordered record of a candidate, taken at call entry: its volume Mass / Density (negative: no gas particle) and its mass
struct alignas(16) MetalSrc {
    double vol, mass;
};

struct MetalsEngine {
    DevBuf<double> left, right, volume, evalradius;
    DevBuf<int> niter, maxcmpte, close;
    DevBuf<int> queue_0, queue_a, queue_b;
    DevBuf<MetalSrc> msrc;
    DevBuf<double> acc; // per particle: dM, dZ, dMetals[9]
    DevBuf<unsigned> ctr;
    DevBuf<unsigned long long> stats;
    int64_t n_state = 0; // particles the per-target arrays were last written for
    int64_t ntargets = 0;
    int64_t last_iterations = 0, last_targets = 0, last_neighbours = 0, last_candidates = 0, last_refused = 0, last_tight = 0;
    std::vector<int64_t> queue_lengths; // targets of every iteration of the last call
    hipEvent_t ev[4] = {};                // around the radius loop, the return walk and the apply pass of the last call ...
    float last_ms[3] = {0, 0, 0};         // ... and what they took (tools/metals_time.py)
    ~MetalsEngine()
    {
        for(hipEvent_t e : ev)
            if(e)
                (void)hipEventDestroy(e);
    }

    MetalState state() { return MetalState{left.p, right.p, volume.p, evalradius.p, niter.p, maxcmpte.p, close.p}; }
    // the targets of metals_haswork (metal_return.c:714-724) in particle order; returns their number
    int64_t make_queue(const MetalView &A, const MetalScalars &S, const uint8_t *active_flags, int64_t n, hipStream_t st);
    // dst[i] = src[i] for the rows of type 4: the stars' Hsml of a resident gas run, whose other rows belong to the SPH loops
    static void take_star_hsml(double *dst, const double *src, const uint8_t *type, int64_t n, hipStream_t st);
    // stellar_density + the return walk + metal_return_postprocess on the current (gas) tree
    void run(TreeBuilder &tree, const MetalView &A, const MetalScalars &S, int64_t n, hipStream_t st);
};

} // namespace mpg
