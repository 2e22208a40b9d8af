// veldisp.h -- DM velocity dispersion around gas particles and black holes on the device tree (see veldisp.hip)
#pragma once
#include "mpg_common.h"
#include "sph.h"
#include "tree_build.h"
#include <vector>

namespace mpg {

constexpr int NWINDHSML = 5;  // trial radii per iteration, veldisp.c:16
constexpr int NUMDMNGB = 40;  // DM neighbours of the dispersion, veldisp.c:17
constexpr int VD_MAXITER = 400; // MAXITER, treewalk.h:214

// device view of the caller's particle table (caller order, n entries each)
struct VdispView {
    const double *pos;
    const uint8_t *type; // null: all type 1 (then there are no targets)
    const double *vel, *gacc, *gpm;
    const uint8_t *tb_grav;
    const double *hsml, *dthsml, *density;
    double *vdisp; // in/out: SphP.VDisp of gas, BHP.VDisp of black holes
};

// per-target state of the radius loop (struct WindVDispPriv, veldisp.c:189-201) and what the tests read back, by particle
struct VdispState {
    double *Left, *Right, *DMRadius;
    double *evalradius; // the trial radius the last pass took its sums at (evaldmradius[close])
    int *niter, *ngb, *maxcmpte;
};

struct VdispScalars {
    double box, hubble_a2, ddrift, dens_threshold; // dens_threshold = 0.1 * sfr_density_threshold(Time)
};

struct VdispEngine {
    DevBuf<double> left, right, dmradius, evalradius;
    DevBuf<int> niter, ngb, maxcmpte;
    DevBuf<int> queue_a, queue_b, queue_bh;
    DevBuf<Aux4> velpred; // the DM sources' predicted velocities in tree order
    DevBuf<unsigned> ctr;
    DevBuf<unsigned long long> stats;
    int64_t n_state = 0; // particles the per-target arrays were last written for
    int64_t ngas = 0, nbh = 0, nbh_exist = 0;
    int64_t last_iterations = 0, last_targets = 0, last_neighbours = 0, last_candidates = 0, last_tight = 0;
    std::vector<int64_t> queue_lengths; // targets of every iteration of the last call

    VdispState state() { return VdispState{left.p, right.p, dmradius.p, evalradius.p, niter.p, ngb.p, maxcmpte.p}; }
    // the queues of winds_find_vel_disp (veldisp.c:402-411): qualifying gas, active black holes; returns whether the DM tree is needed
    bool make_queues(const VdispView &A, const VdispScalars &S, const uint8_t *active_flags, int64_t n, hipStream_t st);
    // blackhole_veldisp + treewalk_do_hsml_loop over the queues, on a tree of the DM particles
    void search(TreeBuilder &tree, const VdispView &A, const mpg_sph_times &T, const VdispScalars &S, hipStream_t st);
};

} // namespace mpg
