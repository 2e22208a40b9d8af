// pm.h -- single-GPU particle-mesh solver (see pm.hip)
#pragma once
#include "../../include/mpgadget_hip.h"
#include "mpg_common.h"
#include "tree_build.h"
#include <rocfft/rocfft.h>
#include <cmath>
#include <vector>

namespace mpg {

// One rocFFT plan with its execution info and work buffer (the plans of the PM solver: rocFFT's own API - rocfft_plan_create,
// rocfft_execute on the engine's stream - not the hipFFT front end of rounds 1-4).
struct FftPlan {
    rocfft_plan plan = nullptr;
    rocfft_execution_info info = nullptr;
    DevBuf<char> work;
    // lengths: fastest dimension first (rocFFT's order); contiguous layouts
    void create(rocfft_result_placement placement, rocfft_transform_type type, int dims, const size_t *lengths, size_t batch);
    void exec(void *in, void *out, hipStream_t st);
    void destroy();
    bool ready() const { return plan != nullptr; }
};

struct PMesh {
    double box = 0, Asmth = 0, G = 0, cellsize = 0;
    int nmesh = 0;
    bool have_plans = false;
    bool kspace_force = false; // true: forces by four inverse transforms as the reference does; false: by differencing the potential (pm.hip)
    FftPlan plan_r2c, plan_c2r;   // 3-D, made on first use (ensure_3d)
    // the fused x-pass form of the default step (pm.hip, k_xpass_solve): batched 2-D transforms over (y, z), one batch per x-plane, around
    // one hand-written pass along x; made on first use (ensure_xpass).  xp_tw: exp(-2 pi i m / Nmesh), m < Nmesh
    FftPlan plan2_r2c, plan2_c2r;
    DevBuf<double> xp_tw;
    int xp_blocks = 0;
    bool xpass_usable() const; // this mesh and these settings take the fused x-pass unless MPG_PM_XPASS=0
    void ensure_3d();
    void ensure_xpass(hipStream_t st);
    void xpass_solve(hipStream_t st);
    DevBuf<double> real;    // Nmesh^3
    DevBuf<double> rho_k;   // 2 * Nmesh^2 (Nmesh/2+1): potential in Fourier space after the transfer
    DevBuf<double> work_k;  // same size: per-component work array (Z2D overwrites its input)
    DevBuf<double> invsinc2, difffac;
    // deposit: 0 not tuned yet, 1 plain atomics, 2 cell-sorted with wave-aggregated atomics (pm.hip)
    struct DepositState {
        int mode = 0, since_tune = 0;
    } dep_single, dep_slab;
    void deposit(int64_t n, const double *d_pos, const float *d_mass, const uint8_t *d_active, double *mesh, int x0, int P, DepositState &ds,
                 hipStream_t st, EventTimer *tm);
    DevBuf<unsigned long long> dep_keys_a, dep_keys_b;
    DevBuf<int> dep_idx_a, dep_idx_b;
    DevBuf<char> dep_tmp;
    // matter power spectrum of the PM density field (gravpm.c:331-382): raw sums of the last PM step
    bool measure_power = true, ps_valid = false;
    int ps_nmesh = 0;                    // the Nmesh the accumulators were last zeroed for (ps_valid survives gravpm_init_periodic)
    DevBuf<double> ps_acc;               // Power[Nmesh], kk[Nmesh], Norm
    DevBuf<unsigned long long> ps_modes; // Nmodes[Nmesh]
    void ps_zero(hipStream_t st);
    // constants of the potential transfer (gravpm.c:388-389)
    double asmth2() const { return pow((2 * M_PI) * Asmth / nmesh, 2); }
    double pot_factor() const { return -G / (M_PI * box); }
    // the transfer stage on a Fourier mesh in either layout, whole or in its two parts (pm.hip)
    enum { TR_MEASURE = 1, TR_APPLY = 2, TR_BOTH = 3 };
    template <bool XLAST, bool FUSE, bool NU> void measure_spectrum(double *rho, int ny, int y0, unsigned grid, hipStream_t st);
    template <bool XLAST, bool FUSE> void transfer_stage(int parts, double *rho, int ny, int y0, unsigned grid, hipStream_t st);
    size_t ps_lds_bytes() const { return (size_t)nmesh * 3 * sizeof(double); }

    // massive-neutrino linear response (MassiveNuLinRespOn, gravpm.c:72-79, 303-326, 418-446).  With nu_fn set the transfer becomes
    // two passes over rho_k: the measurement of the CDM field, a host step (nu_fetch + nu_table: powerspectrum_sum, delta_cdm =
    // sqrt(Power), the callback, the table uploaded), then k_power_spectrum<..., NU>: every k2 > 0 mode times nufac(k), measured again
    // (the total-matter spectrum, Norm times MtotbyMcdm^2), then the potential transfer.  nu_fn == null: the one-pass path, unchanged.
    mpg_nu_response_fn nu_fn = nullptr;
    void *nu_ctx = nullptr;
    double nu_box_mpc = 0;
    int nu_nonzero = 0;
    const char *nu_who = "gravpm_force"; // the call nu_table names in its refusals (the potential planes borrow the host step)
    double nu_prefac = 0, nu_normfac = 1;
    DevBuf<double> nu_tab;              // logknu[nmesh], delta_nu_ratio[nmesh]
    DevBuf<int> nu_guess;               // per log-k bin: the table interval its modes start the search from
    double *nu_host = nullptr;          // pinned: the raw sums of pass 1 (2 nmesh + 1 doubles, nmesh u64), then the table going up
    size_t nu_host_cap = 0;
    size_t ps_lds_bytes_nu() const { return ps_lds_bytes() + (size_t)nmesh * (2 * sizeof(double) + sizeof(int)); }
    // pass 1's raw sums -> the pinned buffer, then wait for the stream (the one host wait of the response); returns {acc, modes}
    void nu_fetch(hipStream_t st, double **acc, unsigned long long **modes);
    // acc / modes: the raw sums over the whole mesh (all-reduced over the ranks in the slab form).  Runs the callback, checks its
    // table, uploads it and zeroes the accumulators for the second measurement
    void nu_table(const double *acc, const unsigned long long *modes, hipStream_t st);
    // the neutrino correction of the lensing planes (plane_pm_grid_init_neutrino_correction, plane.c:313-351; used by planes.hip): the active
    // particles' mass on the mesh, r2c, the CDM spectrum measured as in pass 1 above, the host step with the CALLER's callback of this call
    // (not the registered nu_fn), then every mode times nufac - 1 = nu_prefac * interp(delta_nu_ratio, log k), the k = 0 mode zeroed - no
    // potential transfer, no second measurement - and c2r.  Leaves the unnormalised result in `real` and returns the deposited mass (the
    // k = 0 mode of the transform).  The meshes are scratch here: the raw spectrum of the last PM step, ps_valid, the registered callback
    // and the deposit tuner of gravpm_force (a tuner of its own is used) come out as they went in.
    DepositState dep_plane;
    DevBuf<double> ps_keep;
    double plane_nu_correction(int64_t n, const double *d_pos, const float *d_mass, const uint8_t *d_active, mpg_nu_response_fn fn, void *ctx,
                               double box_mpc, hipStream_t st);
    // hybrid neutrinos as passive tracers (HybridNeutrinosOn, gravpm.c:84-85, 469-474): type-2 particles are not deposited but are read
    // out.  tracer_mass() gives the mass array with those masses zeroed (a zero adds nothing to a cell), or d_mass when off
    bool hybrid_tracer = false;
    DevBuf<float> tracer_mass_buf;
    const float *tracer_mass(int64_t n, const float *d_mass, const uint8_t *d_type, hipStream_t st);

    // gravpm_init_periodic -> petapm_init (gravpm.c:51-54, petapm.c:105-223)
    void init(double BoxSize, double Asmth, int Nmesh, double G, hipStream_t st);
    void ensure_single(); // meshes of the single-GPU form, made on first use (the plans when a step first needs them)
    // petapm_destroy (petapm.c:225-232)
    void destroy();
    // gravpm_force (gravpm.c:61-119): d_gravpm[n][3] is assigned, d_potential[n] (may be null) is incremented
    void force(int64_t n, const double *d_pos, const float *d_mass, const uint8_t *d_active, double *d_gravpm, double *d_potential,
               hipStream_t st, EventTimer *tm);
    ~PMesh() { destroy(); }

    // ---- slab-decomposed form for several GPUs (one process per GPU): rank r owns the x-planes [r P, (r+1) P), P = Nmesh / world,
    // of the real mesh and, between the two transposes, the ky-rows [r Py, (r+1) Py) of the Fourier mesh.  The transposes are
    // all-to-alls done by the caller (RCCL); see pm.hip.
    struct Slab {
        int rank = 0, world = 1, P = 0, Py = 0;
        bool ready = false;
        FftPlan p2d_r2c, p2d_c2r, p1d_fwd, p1d_inv;
        DevBuf<double> phi;      // the potential: planes -2 .. P+2 of Nmesh^2 each (2 + 3 ghost planes around the slab)
        DevBuf<double> force;    // the density slab before the forward transform (planes 0 .. P)
        DevBuf<double> C;        // 2 * P * Nmesh * (Nmesh/2+1): the slab after / before the 2-D transforms
        DevBuf<double> rho_k;    // 2 * Nmesh * Py * (Nmesh/2+1): potential in Fourier space, layout [ky local][kz][kx]
        DevBuf<double> work;     // same size: per-function work array
    } slab;
    DevBuf<unsigned> slab_err;
    size_t slab_cplx_per_peer() const { return (size_t)slab.P * slab.Py * (nmesh / 2 + 1); }
    void slab_init(int rank, int world);
    void slab_destroy();
    // deposit the particles whose CIC cloud touches this rank's planes, 2-D r2c, pack for the transpose: sendA[world][P][Py][Nz]
    void slab_forward_a(int64_t n, const double *d_pos, const float *d_mass, double *sendA, hipStream_t st);
    // recvA[Nmesh][Py][Nz] (x slowest): 1-D transform along x, potential transfer, inverse 1-D transform -> sendB[Nmesh][Py][Nz]
    void slab_forward_b(double *recvA, double *sendB, hipStream_t st);
    // the same in two halves around the measurement, for the neutrino response: b1 = transform along x + this rank's bins of
    // P(k); the caller sums the bins over the ranks and runs nu_table; b2 = nufac, measurement, potential transfer, inverse transform
    void slab_forward_b1(double *recvA, hipStream_t st);
    void slab_forward_b2(double *sendB, hipStream_t st);
    // recvB[world][P][Py][Nz] -> the potential slab (2-D c2r); ghost_send[5][Nmesh^2] = its first 3 and last 2 planes
    void slab_inverse_c(const double *recvB, double *ghost_send, hipStream_t st);
    // ghost_recv[5][Nmesh^2] = the next rank's first 3 planes, then the previous rank's last 2; forces by differencing the
    // potential, CIC readout for `nt` targets (caller indices) that lie in the slab
    void slab_take_ghosts(const double *ghost_recv, hipStream_t st);
    void slab_readout_rows(const double *ghost_recv, int64_t nrows, const double *d_pos, double *d_gravpm, double *d_potential, hipStream_t st);
    void slab_readout(const double *ghost_recv, const int *targets, int64_t nt, const double *d_pos, double *d_gravpm, double *d_potential,
                      hipStream_t st);
};

} // namespace mpg
