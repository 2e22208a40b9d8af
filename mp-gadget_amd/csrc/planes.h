// planes.h -- lensing potential planes on the device (see planes.hip): write_plane (libgadget/plane.c:572-683) without its file output
#pragma once
#include "../../include/mpgadget_hip.h"
#include "mpg_common.h"
#include "pm.h"
#include <vector>

namespace mpg {

constexpr int PLANE_MAXCUTS = 1024; // PlaneParams.CutPoints[1024], plane.c:567

// What one call needs besides the particles, with the reference's defaults resolved (plane.c:579-597) and the bin edges made on the
// host in linspace's order of operations (lenstools.c:39-44, 252-261), so that the device only subtracts, divides and multiplies.
struct PlaneSetup {
    int R = 0, ncuts = 0, nnormals = 0;
    int normals[3] = {0, 0, 0};
    double box = 0, thickness = 0;
    double offset[3] = {0, 0, 0};                   // PartManager->CurrentParticleOffset
    double img_b0[3] = {0, 0, 0}, img_w[3] = {0, 0, 0}; // per axis: bins[0] and bins[R] - bins[0] of the image direction
    std::vector<double> cuts;                       // the cut points
    std::vector<double> slab;                       // per cut: bins[0], bins[1] - bins[0] along the normal
    int tracer = 0;                                 // hybrid_nu_tracer: type 2 is not active
    int64_t nplanes() const { return (int64_t)ncuts * nnormals; }
};

struct PlaneEngine {
    DevBuf<unsigned> counts;         // [planes of a batch][R][R]
    DevBuf<double> slabs;            // the cut table of the call
    DevBuf<unsigned long long> sums; // [0] active particles, [1] rows with a position the wrap cannot take, [2 + p] particles of plane p
    DevBuf<unsigned long long> wide; // the counters as 64-bit integers, for the sum over the ranks
    size_t budget = 0;               // bytes a call may hold in counters (mpg_set_plane_counter_budget); 0: a quarter of the free memory
    struct Solver {                  // the 2-D Poisson solve of one image size: R x R rocFFT plans and the Hermitian half of one plane
        FftPlan r2c, c2r;
        DevBuf<double> cplx;
        int R = 0;
        void ensure(int R);
        void run(int R, double b, double chi, double post, double *d_plane, hipStream_t st);
        ~Solver()
        {
            r2c.destroy();
            c2r.destroy();
        }
    } image, mesh;                   // Resolution^2 (the particle plane), Nmesh^2 (the neutrino correction)
    // the neutrino correction of a call (plane.c:313-478)
    DevBuf<uint8_t> active;
    DevBuf<double> shifted, overlap, corr;
    double mean_mass_cell = 0, inv_fft_norm = 0;
    void correction_init(PMesh &pm, const PlaneSetup &S, int64_t n, const double *d_pos, const float *d_mass, const uint8_t *d_type,
                         const uint8_t *d_flags, mpg_nu_response_fn fn, void *ctx, double box_mpc, hipStream_t st);
    void correction_add(PMesh &pm, const PlaneSetup &S, int cut, int normal, double chi, double post, double *d_plane, hipStream_t st);
    // ONE pass over the particles for the planes [p0, p1) of the call (plane = cut * nnormals + normal slot), counters zeroed first;
    // sums[0..1] and sums[2 + p] are (re)made for those planes
    void count(const PlaneSetup &S, int64_t n, const double *d_pos, const uint8_t *d_type, const uint8_t *d_flags, int64_t p0, int64_t p1,
               unsigned *d_counts, hipStream_t st);
    // counts (32- or 64-bit) -> the potential of one plane in d_plane[R][R] (lenstools.c:292-311, 168-231)
    void solve(const PlaneSetup &S, const void *d_counts, bool wide64, double density_norm_factor, double b, double chi, double post, double *d_plane,
               hipStream_t st);
};

} // namespace mpg
