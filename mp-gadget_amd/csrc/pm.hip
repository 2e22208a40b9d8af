// pm.hip -- long-range particle-mesh gravity (libgadget/petapm.c + gravpm.c) on one gfx950 GPU.
//
// Reference pipeline (gravpm_force, gravpm.c:61-119 -> petapm_force, petapm.c:359-379):
//   CIC deposit into per-region buffers (petapm.c:955-1020,1138-1144) -> pencil exchange into the FFT layout
//   (:786-840) -> r2c (:305) -> potential_transfer (gravpm.c:383-454) -> for Potential, ForceX, ForceY, ForceZ:
//   force_transfer (gravpm.c:458-489) -> c2r (petapm.c:344) -> exchange back (:842-885) -> CIC readout (gravpm.c:499-510).
// On one rank the regions / pencils only relocate cells: here particles deposit straight into
// the global Nmesh^3 mesh with hardware fp64 atomics (global_atomic_add_f64) and read straight back from it.
// PFFT (third-party, not vendored) is an unnormalised DFT; the real-to-complex / complex-to-real transforms of rocFFT are the same transform.
// All kernels are HBM-streaming: per PM step ~ N*(28+128) + 5*3*2*R + 5*2*R + N*(24+256+32) bytes, R = 8*Nmesh^3.
#include "pm.h"
#include "pm_cic.h"
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <rocprim/rocprim.hpp>

namespace mpg {

#define MPG_FFT(expr)                                                                                          \
    do {                                                                                                       \
        rocfft_status _r = (expr);                                                                             \
        if(_r != rocfft_status_success)                                                                        \
            ::mpg::fail(__FILE__, __LINE__, std::string("rocFFT error ") + std::to_string((int)_r) + " in " #expr); \
    } while(0)

// put_particle_to_mesh through pm_iterate_one (petapm.c:955-1020, :1138-1144).  Two lanes per particle: lane 2j + h adds the four corners
// of particle j with z-bit h (c = 4h + 0 .. 3 in the corner order of pm_cic.h), so the lanes of a pair write z and z + 1, neighbours in
// memory, in the SAME instruction.  The atomics run at the memory side as 64-byte requests and their number is what costs: in lattice
// order at Nmesh = 2 N^(1/3) a wave of one particle per lane wrote every second double of 1 KiB per corner (16 half-used requests), a wave
// of pairs writes 512 contiguous bytes (8 full ones).  Every addend is the expression of before, cic_weight(c, res, 1.0) * m; at
// iz = Nmesh - 1 the pair's cells are a row apart and each lane's atomic goes its own way.
__global__ void __launch_bounds__(256) k_cic_deposit(int64_t n, const double *__restrict__ pos, const float *__restrict__ mass,
                                                     const uint8_t *__restrict__ active, double cellsize, int nmesh,
                                                     double *__restrict__ mesh)
{
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t i = t >> 1;
    const int h = (int)(t & 1);
    if(i >= n)
        return;
    if(active && !active[i])
        return;
    int ic[3];
    double res[3];
    cic_cell3(pos + 3 * i, cellsize, nmesh, ic, res);
    const double m = (double)mass[i];
#pragma unroll
    for(int q = 0; q < 4; q++) {
        const int c = 4 * h + q;
        unsafeAtomicAdd(&mesh[cic_index(c, ic, nmesh)], cic_weight(c, res, 1.0) * m);
    }
}

// the same onto the x-planes [x0, x0 + P) of a slab: the part of the particle's cloud that falls on them.  x is looked at first:
// every rank sees particles of which most touch none of its planes
__global__ void __launch_bounds__(256) k_cic_deposit_slab(int64_t n, const double *__restrict__ pos, const float *__restrict__ mass,
                                                          const uint8_t *__restrict__ active, double cellsize, int nmesh, int x0, int P,
                                                          double *__restrict__ slab)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if(i >= n)
        return;
    if(active && !active[i])
        return;
    int ic[3];
    double res[3];
    ic[0] = cic_cell(pos[3 * i], cellsize, nmesh, res[0]);
    if(!in_slab(ic[0], x0, P) && !in_slab(wrap(ic[0] + 1, nmesh), x0, P))
        return;
#pragma unroll
    for(int k = 1; k < 3; k++)
        ic[k] = cic_cell(pos[3 * i + k], cellsize, nmesh, res[k]);
    const double m = (double)mass[i];
#pragma unroll
    for(int c = 0; c < 8; c++) {
        size_t lin;
        if(cic_index_slab(c, ic, nmesh, x0, P, lin))
            unsafeAtomicAdd(&slab[lin], cic_weight(c, res, 1.0) * m);
    }
}

// ---- deposit for clustered sets.  In a dense clump thousands of particles share a handful of mesh cells and the plain kernel's
// atomics serialise on those addresses (256^3 clustered set: 29.8 ms instead of 4.0).  Here the particles are first sorted by
// their base cell (one radix sort of cell index -> particle); a wave then holds RUNS of particles with the same 8 target cells,
// their corner weights are summed over each run with a segmented wave scan, and only the last lane of a run issues the 8
// atomics ("wavefront atomics": one per cell and wave instead of one per particle).  Slower than the plain kernel when cells hold
// less than one particle (the sort costs what the atomics do), so PMesh::force times both and keeps the faster one.
__global__ void __launch_bounds__(256) k_cell_keys(int64_t n, const double *__restrict__ pos, const uint8_t *__restrict__ active, double cellsize,
                                                   int nmesh, unsigned long long *__restrict__ keys, int *__restrict__ idx)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if(i >= n)
        return;
    int ic[3];
    double res[3];
    cic_cell3(pos + 3 * i, cellsize, nmesh, ic, res);
    keys[i] = (active && !active[i]) ? ~0ull : (unsigned long long)cic_index(0, ic, nmesh); // inactive particles sort to the end and are skipped
    idx[i] = (int)i;
}

__global__ void __launch_bounds__(256) k_cic_deposit_sorted(int64_t n, const unsigned long long *__restrict__ skeys, const int *__restrict__ sidx,
                                                            const double *__restrict__ pos, const float *__restrict__ mass, double cellsize,
                                                            int nmesh, int x0, int P, double *__restrict__ mesh)
{
    // mesh holds the x-planes [x0, x0 + P) (all of them on one GPU: x0 = 0, P = nmesh); corners on other planes are skipped
    const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int lane = threadIdx.x & 63;
    unsigned long long key = ~0ull;
    double w[8];
    int ic[3] = {0, 0, 0};
#pragma unroll
    for(int c = 0; c < 8; c++)
        w[c] = 0;
    if(k < n) {
        key = skeys[k];
        if(key != ~0ull) {
            const int i = sidx[k];
            double res[3];
            cic_cell3(pos + 3 * (int64_t)i, cellsize, nmesh, ic, res);
            const double m = (double)mass[i];
#pragma unroll
            for(int c = 0; c < 8; c++)
                w[c] = cic_weight(c, res, m); // the mass first: the run sums below add weights that carry it
        }
    }
    // segmented inclusive scan over the lanes of the wave (segments = runs of equal keys)
    const unsigned long long prev = __shfl_up(key, 1);
    bool f = lane == 0 || prev != key; // head of a run (within this wave)
    const bool head_next = __shfl_down(f ? 1 : 0, 1) != 0;
    const bool tail = lane == 63 || head_next;
    for(int d = 1; d < 64; d <<= 1) {
        const bool f2 = __shfl_up(f ? 1 : 0, d) != 0;
        double v2[8];
#pragma unroll
        for(int c = 0; c < 8; c++)
            v2[c] = __shfl_up(w[c], d);
        if(lane >= d && !f) {
#pragma unroll
            for(int c = 0; c < 8; c++)
                w[c] += v2[c];
            f = f2;
        }
    }
    if(tail && key != ~0ull) {
#pragma unroll
        for(int c = 0; c < 8; c++) {
            size_t lin;
            if(cic_index_slab(c, ic, nmesh, x0, P, lin))
                unsafeAtomicAdd(&mesh[lin], w[c]);
        }
    }
}

__device__ __forceinline__ double sinc_unnormed(double x)
{
    // gravpm.c:295-302
    if(x < 1e-5 && x > -1e-5) {
        const double x2 = x * x;
        return 1.0 - x2 / 6. + x2 * x2 / 120.;
    }
    return sin(x) / x;
}

// ---- the Fourier-space rules, once.  Cell ip of a Fourier mesh that holds ny rows of ky starting at y0 (ny = nmesh, y0 = 0 on one
// GPU; a ky-slab in the slab-decomposed form): its indices and k^2 of the signed mode (petapm_mesh_to_k, petapm.c:81-84; kz in
// [0, N/2]).  Layout [kx][ky local][kz]; XLAST: [ky local][kz][kx] (kx fastest: the slab form after its transpose).
struct FourierCell {
    int ix, iy, iz;
    long long k2;
};
__device__ __forceinline__ long long fourier_k2(int ix, int iy, int iz, int nmesh)
{
    const int kx = ix <= nmesh / 2 ? ix : ix - nmesh;
    const int ky = iy <= nmesh / 2 ? iy : iy - nmesh;
    const int kz = iz;
    return (long long)kx * kx + (long long)ky * ky + (long long)kz * kz;
}
template <bool XLAST>
__device__ __forceinline__ FourierCell fourier_cell(size_t ip, int nmesh, int ny, int y0)
{
    const int nz = nmesh / 2 + 1;
    FourierCell c;
    if(XLAST) {
        c.ix = (int)(ip % nmesh);
        const size_t j = ip / nmesh;
        c.iz = (int)(j % nz);
        c.iy = y0 + (int)(j / nz);
    }
    else {
        c.iz = (int)(ip % nz);
        const size_t t = ip / nz;
        c.iy = y0 + (int)(t % ny);
        c.ix = (int)(t / ny);
    }
    c.k2 = fourier_k2(c.ix, c.iy, c.iz, nmesh);
    return c;
}

// what a k2 > 0 mode of the density is multiplied by to become the potential (gravpm.c:403-421): pot_factor * smth * f * f,
// smth = exp(-k2 asmth2) / k2, f = prod 1/sinc^2.  (exp(-k2 asmth2) / k2 and the bin below from tables indexed by k2 - 2.4 MB of them
// at Nmesh 512 - measured SLOWER than the exp and the log: 1.06 against 0.64 ms, the gathers miss)
__device__ __forceinline__ double potential_fac(long long k2, double asmth2, double pot_factor, double f)
{
    const double smth = exp(-(double)k2 * asmth2) / (double)k2;
    return pot_factor * smth * f * f;
}

// logarithmic bin of |k| (powerspectrum_add_mode, gravpm.c:331-347); a bin >= Nmesh is not counted
__device__ __forceinline__ int logk_bin(long long k2, double binsperunit) { return (int)floor(binsperunit * log((double)k2) / 2.); }

// potential_transfer, gravpm.c:383-454, swept as pm_apply_transfer_function does (petapm.c:1092-1132).
template <bool XLAST>
__global__ void __launch_bounds__(256) k_potential_transfer(int nmesh, int ny, int y0, double asmth2, double pot_factor,
                                                            const double *__restrict__ invsinc2, double2 *__restrict__ cplx)
{
    const int nz = nmesh / 2 + 1;
    const size_t total = (size_t)nmesh * ny * nz;
    const size_t ip = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if(ip >= total)
        return;
    const FourierCell c = fourier_cell<XLAST>(ip, nmesh, ny, y0);
    double2 v = cplx[ip];
    if(c.k2 == 0) {
        v.x = 0.0;
        v.y = 0.0;
    }
    else {
        const double fac = potential_fac(c.k2, asmth2, pot_factor, invsinc2[c.ix] * invsinc2[c.iy] * invsinc2[c.iz]);
        v.x *= fac;
        v.y *= fac;
    }
    cplx[ip] = v;
}

// measure_power_spectrum + powerspectrum_add_mode, gravpm.c:331-382: per Fourier cell (before the potential transfer touches
// it) m = |delta_k|^2 de-convolved with the CIC window once (invwindow^2), weight 2 except on the kz = 0 and Nyquist planes,
// logarithmic bins in |k| (Nmesh bins up to sqrt(3) Nmesh / 2); the k = 0 mode is the normalisation.  acc = [Power[nbins],
// kk[nbins], Norm], modes[nbins]; the reference's per-thread copies are per-block LDS histograms here.
// FUSE (round 6): the potential transfer of the same cell in the same pass (k_potential_transfer's arithmetic, after the mode has been
// measured: gravpm.c measures before it multiplies) - one read of the 1.07 GB of rho_k instead of two
// NU (the massive-neutrino linear response, gravpm.c:418-446): first each k2 > 0 mode is multiplied by
// nufac = 1 + prefac * delta_nu_ratio(log k) and written back, then measured (the total-matter spectrum), then - FUSE - transferred;
// Norm is |rho_0|^2 * normfac (MtotbyMcdm^2).  The table (logknu, delta_nu_ratio: nonzero entries; guess: per log-k bin the interval
// to start from) is copied to LDS: 2.5 Nmesh more words beside the 3 Nmesh of the histograms (44 KB at Nmesh 1024).
struct NuArgs {
    const double *tab;   // logknu[nbins], delta_nu_ratio[nbins]
    const int *guess;    // [nbins]
    int nonzero;
    double prefac, normfac;
    double kscale;       // 2 pi / BoxSize_in_MPC: log k in the table's units = log(sqrt(k2) kscale)
};

// gsl_interp_linear on the LDS table after the two clamps of gravpm.c:423-428.  The interval j with logknu[j] <= x < logknu[j+1]
// (j = nonzero - 2 for x = logknu[nonzero-1], as gsl_interp_bsearch) is found by stepping from the guess of the mode's log-k bin: the
// table is the bins' own log kk, so a mode lies in the interval of its bin or the one before (one or two steps, no binary search).
__device__ __forceinline__ double nu_factor(double x, int kint, const double *s_lk, const double *s_rt, const int *s_gs, int nonzero,
                                            double prefac)
{
    const double x0 = s_lk[0], x1 = s_lk[nonzero - 1];
    if(x < x0 && x > x0 - log(2.0))
        x = x0;
    else if(x > x1)
        x = x1;
    // (further below, where gsl_interp_eval fails with a domain error, the first value is used as well)
    x = x < x0 ? x0 : x;
    int j = s_gs[kint];
    while(j > 0 && x < s_lk[j])
        j--;
    while(j < nonzero - 2 && x >= s_lk[j + 1])
        j++;
    const double x_lo = s_lk[j], x_hi = s_lk[j + 1], y_lo = s_rt[j], y_hi = s_rt[j + 1];
    return 1 + prefac * (y_lo + (x - x_lo) / (x_hi - x_lo) * (y_hi - y_lo));
}

// the LDS of a measuring block: the histograms Power[nbins], kk[nbins], Nmodes[nbins] and, NU, the response table
struct PsLds {
    double *pow, *kk;
    unsigned long long *n;
    const double *lk, *rt;
    const int *gs;
};

__device__ __forceinline__ double ps_binsperunit(int nmesh) { return (nmesh - 1) / log(sqrt(3.0) * nmesh / 2.0); }

// One mode of that pass, written once for the kernels that sweep rho_k (k_power_spectrum, k_xpass_solve): v is the mode fc as
// transformed; it is measured into the block's histograms (the k = 0 mode into Norm) and comes back as what the mesh holds afterwards.
// Returns whether that differs from what came in, i.e. has to be stored.
template <bool FUSE, bool NU>
__device__ __forceinline__ bool spectrum_mode(const FourierCell &fc, int nmesh, double binsperunit, const double *__restrict__ invsinc2, double2 &v,
                                              const PsLds &s, double *__restrict__ acc, double asmth2, double pot_factor, const NuArgs &nu)
{
    const int nbins = nmesh;
    const long long k2 = fc.k2;
    if(k2 == 0) {
        const double m0 = v.x * v.x + v.y * v.y;
        acc[2 * nbins] = NU ? m0 * nu.normfac : m0; // Norm (gravpm.c:437-441: Norm *= MtotbyMcdm^2 with the response)
        if(FUSE)
            v = make_double2(0.0, 0.0);
        return FUSE;
    }
    int kint = 0;
    if(NU) { // the mode times nufac before it is measured (gravpm.c:418-436)
        kint = logk_bin(k2, binsperunit);
        const double nufac = nu_factor(log(sqrt((double)k2) * nu.kscale), kint < nbins ? kint : nbins - 1, s.lk, s.rt, s.gs, nu.nonzero, nu.prefac);
        v.x *= nufac;
        v.y *= nufac;
    }
    const double m = v.x * v.x + v.y * v.y;
    const double f = invsinc2[fc.ix] * invsinc2[fc.iy] * invsinc2[fc.iz];
    if(FUSE) { // (k_potential_transfer's factor)
        const double fac = potential_fac(k2, asmth2, pot_factor, f);
        v = make_double2(v.x * fac, v.y * fac);
    }
    if(!NU)
        kint = logk_bin(k2, binsperunit);
    if(kint < nbins) {
        const int w = (fc.iz == 0 || fc.iz == nmesh / 2) ? 1 : 2;
        __hip_atomic_fetch_add(&s.pow[kint], w * m * f * f, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        __hip_atomic_fetch_add(&s.kk[kint], w * sqrt((double)k2), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        __hip_atomic_fetch_add(&s.n[kint], (unsigned long long)w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    }
    return FUSE || NU;
}

// a block's histograms added to the mesh's accumulators
__device__ __forceinline__ void spectrum_flush(int nbins, const PsLds &s, double *__restrict__ acc, unsigned long long *__restrict__ modes)
{
    for(int b = threadIdx.x; b < nbins; b += blockDim.x)
        if(s.n[b]) {
            unsafeAtomicAdd(&acc[b], s.pow[b]);
            unsafeAtomicAdd(&acc[nbins + b], s.kk[b]);
            atomicAdd(&modes[b], s.n[b]);
        }
}

template <bool XLAST, bool FUSE = false, bool NU = false>
__global__ void __launch_bounds__(256) k_power_spectrum(int nmesh, int ny, int y0, const double *__restrict__ invsinc2,
                                                        double2 *__restrict__ cplx, double *__restrict__ acc,
                                                        unsigned long long *__restrict__ modes, double asmth2 = 0, double pot_factor = 0,
                                                        NuArgs nu = NuArgs{})
{
    extern __shared__ double s_ps[]; // Power[nbins], kk[nbins], then modes[nbins] (u64); NU: logknu[nbins], ratio[nbins], guess[nbins] (int)
    const int nbins = nmesh;
    double *s_pow = s_ps, *s_kk = s_ps + nbins;
    unsigned long long *s_n = (unsigned long long *)(s_ps + 2 * nbins);
    double *s_lk = s_ps + 3 * nbins, *s_rt = s_ps + 4 * nbins;
    int *s_gs = (int *)(s_ps + 5 * nbins);
    for(int b = threadIdx.x; b < nbins; b += blockDim.x) {
        s_pow[b] = 0;
        s_kk[b] = 0;
        s_n[b] = 0;
        if(NU) {
            s_lk[b] = nu.tab[b];
            s_rt[b] = nu.tab[nbins + b];
            s_gs[b] = nu.guess[b];
        }
    }
    __syncthreads();
    const PsLds s{s_pow, s_kk, s_n, s_lk, s_rt, s_gs};
    const int nz = nmesh / 2 + 1;
    const size_t total = (size_t)nmesh * ny * nz;
    const double binsperunit = ps_binsperunit(nbins);
    for(size_t ip = (size_t)blockIdx.x * blockDim.x + threadIdx.x; ip < total; ip += (size_t)gridDim.x * blockDim.x) {
        double2 v = cplx[ip];
        if(spectrum_mode<FUSE, NU>(fourier_cell<XLAST>(ip, nmesh, ny, y0), nmesh, binsperunit, invsinc2, v, s, acc, asmth2, pot_factor, nu))
            cplx[ip] = v;
    }
    __syncthreads();
    spectrum_flush(nbins, s, acc, modes);
}

// The x-transform of the fused solve (k_xpass_solve): a Stockham transform of length N = 2^n in passes of radix 8 (and one of 4 or 2
// first when n is no multiple of 3), written for N / 8 "threads" per column that hold 8 points each.  Thread j holds, before every pass
// and after the last, the points j + q N / 8, q = 0 .. 7: in a pass of radix r it computes the 8 / r butterflies jb = j + u N / 8, whose
// inputs jb + t N / r are its points q = u + t 8 / r, and whose outputs go to (jb - k) r + k + t Ns, k = jb mod Ns (Ns = the product of
// the radices before) - after the last pass, Ns = N / r, those are the points it read.  So a column comes from memory into registers, is
// exchanged through LDS between passes only, and leaves from registers.  DIR = -1: forward (exp(-2 pi i jk / N)), +1: backward; both
// unnormalised as rocFFT's and PFFT's.  tw[m] = exp(-2 pi i m / N), m < N (fp64, rounded from extended precision on the host).
__device__ __forceinline__ double2 xp_mul(double2 a, double2 b) { return make_double2(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x); }
template <int DIR> __device__ __forceinline__ double2 xp_mul_i(double2 a) // a times DIR i
{
    return DIR < 0 ? make_double2(a.y, -a.x) : make_double2(-a.y, a.x);
}
__device__ __forceinline__ void xp_dft2(double2 &a, double2 &b)
{
    const double2 t = a;
    a = make_double2(t.x + b.x, t.y + b.y);
    b = make_double2(t.x - b.x, t.y - b.y);
}
template <int DIR> __device__ __forceinline__ void xp_dft4(double2 &v0, double2 &v1, double2 &v2, double2 &v3)
{
    xp_dft2(v0, v2);
    xp_dft2(v1, v3);
    v3 = xp_mul_i<DIR>(v3);
    xp_dft2(v0, v1); // y0, y2
    xp_dft2(v2, v3); // y1, y3
    const double2 t = v1;
    v1 = v2;
    v2 = t;
}
template <int DIR> __device__ __forceinline__ void xp_dft8(double2 v[8], int s /* stride between the 8 points in v */)
{
    const double h = 0.70710678118654752440; // sqrt(1/2)
#pragma unroll
    for(int n = 0; n < 4; n++)
        xp_dft2(v[n * s], v[(n + 4) * s]);
    // times w8^n, w8 = exp(DIR 2 pi i / 8)
    {
        const double2 a = v[5 * s], b = v[7 * s];
        v[5 * s] = DIR < 0 ? make_double2((a.x + a.y) * h, (a.y - a.x) * h) : make_double2((a.x - a.y) * h, (a.y + a.x) * h);
        v[6 * s] = xp_mul_i<DIR>(v[6 * s]);
        v[7 * s] = DIR < 0 ? make_double2((b.y - b.x) * h, -(b.x + b.y) * h) : make_double2(-(b.x + b.y) * h, (b.x - b.y) * h);
    }
    xp_dft4<DIR>(v[0], v[1 * s], v[2 * s], v[3 * s]); // y0, y2, y4, y6
    xp_dft4<DIR>(v[4 * s], v[5 * s], v[6 * s], v[7 * s]); // y1, y3, y5, y7
    const double2 e1 = v[1 * s], e2 = v[2 * s], e3 = v[3 * s], o0 = v[4 * s], o1 = v[5 * s], o2 = v[6 * s];
    v[1 * s] = o0;
    v[2 * s] = e1;
    v[3 * s] = o1;
    v[4 * s] = e2;
    v[5 * s] = o2;
    v[6 * s] = e3;
}

// radix of the pass that starts at Ns: the odd factor (2 or 4) first, then 8s
template <int N> __device__ constexpr int xp_radix(int Ns)
{
    int n = 0;
    for(int m = N; m > 1; m >>= 1)
        n++;
    return Ns == 1 && n % 3 ? 1 << (n % 3) : 8;
}

// one pass on the 8 points of thread j: twiddles, butterflies.  Leaves output t of butterfly u in v[u + t 8 / r].
template <int N, int DIR, int Ns> __device__ __forceinline__ void xp_pass(double2 v[8], int j, const double2 *__restrict__ tw)
{
    constexpr int r = xp_radix<N>(Ns), nb = 8 / r;
#pragma unroll
    for(int u = 0; u < nb; u++) {
        if(Ns > 1) {
            const int k = (j + u * (N / 8)) % Ns;
#pragma unroll
            for(int t = 1; t < r; t++) {
                double2 w = tw[t * k * (N / (Ns * r))];
                if(DIR > 0)
                    w.y = -w.y;
                v[u + t * nb] = xp_mul(v[u + t * nb], w);
            }
        }
        if(r == 8)
            xp_dft8<DIR>(v + u, nb);
        else if(r == 4)
            xp_dft4<DIR>(v[u], v[u + nb], v[u + 2 * nb], v[u + 3 * nb]);
        else
            xp_dft2(v[u], v[u + nb]);
    }
}

// where output t of butterfly u of thread j goes in the pass that starts at Ns
template <int N, int Ns> __device__ __forceinline__ int xp_out(int j, int u, int t)
{
    constexpr int r = xp_radix<N>(Ns);
    const int jb = j + u * (N / 8), k = jb % Ns;
    return (jb - k) * r + k + t * Ns;
}

// the exchange between two passes: buf[x * ld + c] is column c of the tile
template <int N, int Ns> __device__ __forceinline__ void xp_scatter(const double2 v[8], int j, double2 *buf, int ld, int c)
{
    constexpr int r = xp_radix<N>(Ns), nb = 8 / r;
#pragma unroll
    for(int u = 0; u < nb; u++)
#pragma unroll
        for(int t = 0; t < r; t++)
            buf[xp_out<N, Ns>(j, u, t) * ld + c] = v[u + t * nb];
}
template <int N> __device__ __forceinline__ void xp_gather(double2 v[8], int j, const double2 *buf, int ld, int c)
{
#pragma unroll
    for(int q = 0; q < 8; q++)
        v[q] = buf[(j + q * (N / 8)) * ld + c];
}

// the passes of one transform from Ns on, with the exchanges between them through `tile`
template <int N, int DIR, int Ns> __device__ __forceinline__ void xp_transform(double2 v[8], int j, int c, int ld, double2 *tile, const double2 *__restrict__ tw)
{
    constexpr int r = xp_radix<N>(Ns);
    xp_pass<N, DIR, Ns>(v, j, tw);
    if constexpr(Ns * r < N) {
        __syncthreads(); // (the tile may still be read: the exchange before this one)
        xp_scatter<N, Ns>(v, j, tile, ld, c);
        __syncthreads();
        xp_gather<N>(v, j, tile, ld, c);
        xp_transform<N, DIR, Ns * r>(v, j, c, ld, tile, tw);
    }
}

// columns of kz per tile: 8 modes of 16 bytes are one 128-byte line per x; the tile N x columns stays within 64 KiB
constexpr int xp_cols(int N) { return N <= 512 ? 8 : 4; }
// waves per SIMD of the blocks a CU holds - two (one computes while the other waits for memory), or the one that its 160 KiB of LDS have
// room for at N = 1024: the register budget of the kernel
constexpr int xp_waves(int N)
{
    const int lds = N * xp_cols(N) * 16 + 3 * N * 8, blocks = 2 * lds <= 160 * 1024 ? 2 : 1, w = blocks * (N / 8 * xp_cols(N)) / 256;
    return w > 1 ? w : 1;
}
constexpr bool xp_supported(int N) { return N == 64 || N == 128 || N == 256 || N == 512 || N == 1024; }

// The x-part of the transfer stage in ONE pass over rho_k (layout [x][ky][kz], as the batched 2-D transforms over (y, z) leave and take
// it): forward transform along x, the mode measured and multiplied by the potential factor (spectrum_mode<FUSE>: the arithmetic of
// k_power_spectrum<false, true, false>), backward transform along x.  The 3-D plans sweep the same columns three times (forward x-pass,
// k_power_spectrum, backward x-pass: 6 x 1.07 GB at Nmesh 512); this is one read and one write.  A work item is a tile of xp_cols(N)
// consecutive kz at one ky (the first and the last tile of a row are ragged: their dead columns transform zeros and store nothing);
// a block takes a contiguous share of them, ky-major, so that it walks along rows that are contiguous in memory, and keeps its P(k)
// histograms in LDS across all of them.  N / 8 threads per column (xp_pass): a column comes from memory into registers, passes through
// the LDS tile between the passes and for the mode arithmetic, and leaves from registers.
template <int N>
__global__ void __launch_bounds__(N / 8 * xp_cols(N), xp_waves(N)) k_xpass_solve(const double2 *__restrict__ tw, const double *__restrict__ invsinc2,
                                                                    double2 *__restrict__ cplx, double *__restrict__ acc,
                                                                    unsigned long long *__restrict__ modes, double asmth2, double pot_factor)
{
    constexpr int TC = xp_cols(N), nz = N / 2 + 1, ntile = N / 2 / TC + 1, nbins = N;
    extern __shared__ __attribute__((aligned(16))) double2 s_xp[]; // the tile [N][TC], then Power[nbins], kk[nbins], modes[nbins] (u64)
    double2 *tile = s_xp;
    double *s_pow = (double *)(tile + N * TC);
    const PsLds s{s_pow, s_pow + nbins, (unsigned long long *)(s_pow + 2 * nbins), nullptr, nullptr, nullptr};
    for(int b = threadIdx.x; b < nbins; b += blockDim.x) {
        s.pow[b] = 0;
        s.kk[b] = 0;
        s.n[b] = 0;
    }
    __syncthreads();
    const int c = threadIdx.x % TC, j = threadIdx.x / TC;
    // (the same for every thread: in scalar registers)
    const double bpu = ps_binsperunit(nbins);
    const double binsperunit = __hiloint2double(__builtin_amdgcn_readfirstlane(__double2hiint(bpu)), __builtin_amdgcn_readfirstlane(__double2loint(bpu)));
    const int items = N * ntile, per = (items + (int)gridDim.x - 1) / (int)gridDim.x;
    const int it0 = (int)blockIdx.x * per, it1 = it0 + per < items ? it0 + per : items;
    for(int it = it0; it < it1; it++) {
        FourierCell fc;
        // tile t of row iy holds kz = t TC - s .. + TC - 1, s = iy mod TC: a row of nz = N / 2 + 1 modes starts s modes behind a
        // boundary of TC modes in memory, the same s for every x, so each tile is ONE aligned line (128 bytes at TC = 8) per x - with
        // tiles counted from kz = 0 every line was fetched and written by two tiles
        fc.iy = it / ntile;
        const int kz0 = (it % ntile) * TC - fc.iy % TC;
        fc.iz = kz0 + c;
        const bool live = fc.iz >= 0 && fc.iz < nz;
        // mode (x, iy, iz) is cplx[(x N + iy) nz + iz].  Of x = j + q N / 8 the part q goes into a base that is the same for the whole
        // block and the rest into ONE 32-bit byte offset per thread (j N nz 16 < 2^31 up to N = 1024): eight 64-bit addresses per thread
        // would cost the registers that the second block per CU needs
        char *base = (char *)(cplx + ((ptrdiff_t)fc.iy * nz + kz0)); // (never in front of the mesh: kz0 < 0 only for iy > 0)
        const unsigned off = ((unsigned)j * (N * nz) + c) * (unsigned)sizeof(double2);
        double2 v[8];
#pragma unroll
        for(int q = 0; q < 8; q++)
            v[q] = live ? *(const double2 *)(base + (size_t)q * (N / 8) * (N * nz) * sizeof(double2) + off) : make_double2(0.0, 0.0);
        // (jt is j, but not to the compiler: the twiddles and window factors of a thread are the same for every item, and kept in
        // registers across the loop - 70 of them - they leave no room for two blocks per CU)
        int jt = j;
        asm volatile("" : "+v"(jt));
        xp_transform<N, -1, 1>(v, jt, c, TC, tile, tw);
        // the modes, one at a time from the thread's own slots of the tile: with the 8 points in registers beside the polynomials of exp
        // and log there is no room for two blocks per CU
        __syncthreads(); // (the tile may still be read: the last exchange)
#pragma unroll
        for(int q = 0; q < 8; q++)
            tile[(jt + q * (N / 8)) * TC + c] = v[q];
        if(live) {
#pragma unroll 1
            for(int q = 0; q < 8; q++) {
                fc.ix = jt + q * (N / 8);
                fc.k2 = fourier_k2(fc.ix, fc.iy, fc.iz, N);
                double2 m = tile[fc.ix * TC + c];
                spectrum_mode<true, false>(fc, N, binsperunit, invsinc2, m, s, acc, asmth2, pot_factor, NuArgs{});
                tile[fc.ix * TC + c] = m;
            }
        }
        xp_gather<N>(v, jt, tile, TC, c);
        xp_transform<N, 1, 1>(v, jt, c, TC, tile, tw);
        if(live) {
#pragma unroll
            for(int q = 0; q < 8; q++)
                *(double2 *)(base + (size_t)q * (N / 8) * (N * nz) * sizeof(double2) + off) = v[q];
        }
    }
    __syncthreads();
    spectrum_flush(nbins, s, acc, modes);
}

// plane_neutrino_correction_transfer, plane.c:291-311: every mode times nufac - 1 (the same table, clamps and interpolation as NU above,
// without the 1), the k = 0 mode zeroed.  Single-GPU layout only.
__global__ void __launch_bounds__(256) k_nu_correction(int nmesh, double2 *__restrict__ cplx, NuArgs nu)
{
    extern __shared__ double s_ps[]; // logknu[nbins], ratio[nbins], guess[nbins] (int)
    const int nbins = nmesh;
    double *s_lk = s_ps, *s_rt = s_ps + nbins;
    int *s_gs = (int *)(s_ps + 2 * nbins);
    for(int b = threadIdx.x; b < nbins; b += blockDim.x) {
        s_lk[b] = nu.tab[b];
        s_rt[b] = nu.tab[nbins + b];
        s_gs[b] = nu.guess[b];
    }
    __syncthreads();
    const int nz = nmesh / 2 + 1;
    const size_t total = (size_t)nmesh * nmesh * nz;
    const double binsperunit = (nbins - 1) / log(sqrt(3.0) * nmesh / 2.0);
    for(size_t ip = (size_t)blockIdx.x * blockDim.x + threadIdx.x; ip < total; ip += (size_t)gridDim.x * blockDim.x) {
        const long long k2 = fourier_cell<false>(ip, nmesh, nmesh, 0).k2;
        if(k2 == 0) {
            cplx[ip] = make_double2(0.0, 0.0);
            continue;
        }
        const int kint = logk_bin(k2, binsperunit);
        const double f = nu_factor(log(sqrt((double)k2) * nu.kscale), kint < nbins ? kint : nbins - 1, s_lk, s_rt, s_gs, nu.nonzero, nu.prefac) - 1;
        double2 v = cplx[ip];
        v.x *= f;
        v.y *= f;
        cplx[ip] = v;
    }
}

// force_transfer for one axis, gravpm.c:476-498: (re, im) <- (-im*fac, re*fac), fac = -diff_kernel(k 2pi/N) N/Box.
// axis < 0: plain copy (the Potential pass has no transfer function, gravpm.c:32-39).
// The destination element of source (ix, row, iz) is dst[(ix * xmul + xoff) * ny * nz + row * nz + iz]: xmul = 1, xoff = 0 on one
// GPU; (4, function) in the slab form, which interleaves the four functions so that each all-to-all block stays contiguous.
template <bool XLAST>
__global__ void __launch_bounds__(256) k_force_transfer(int nmesh, int ny, int y0, int axis, const double *__restrict__ difffac,
                                                        const double2 *__restrict__ src, double2 *__restrict__ dst, int xmul, int xoff)
{
    const int nz = nmesh / 2 + 1;
    const size_t total = (size_t)nmesh * ny * nz;
    const size_t ip = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if(ip >= total)
        return;
    double2 v = src[ip];
    const FourierCell fc = fourier_cell<XLAST>(ip, nmesh, ny, y0);
    if(axis >= 0) {
        const double fac = difffac[axis == 0 ? fc.ix : (axis == 1 ? fc.iy : fc.iz)];
        const double t0 = -v.y * fac, t1 = v.x * fac;
        v.x = t0;
        v.y = t1;
    }
    const size_t rowsz = (size_t)ny * nz;
    if(XLAST) // same layout in and out
        dst[ip] = v;
    else
        dst[((size_t)fc.ix * xmul + xoff) * rowsz + (ip - (size_t)fc.ix * rowsz)] = v;
}

// readout_potential / readout_force_{x,y,z} through pm_iterate_one (gravpm.c:499-510).
// comp < 3: out[3*i+comp] = sum (GravPM is zeroed before, gravpm.c:88-92); comp == 3: out[i] += sum (Potential).
__global__ void __launch_bounds__(256) k_cic_readout(int64_t n, const double *__restrict__ pos, const uint8_t *__restrict__ active,
                                                     double cellsize, int nmesh, const double *__restrict__ mesh, int comp,
                                                     double *__restrict__ out)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if(i >= n)
        return;
    if(active && !active[i]) // garbage / swallowed: outside every region (gravpm.c:176-179), GravPM stays at the zero of gravpm.c:88-92
        return;
    int ic[3];
    double res[3];
    cic_cell3(pos + 3 * i, cellsize, nmesh, ic, res);
    double acc = 0;
#pragma unroll
    for(int c = 0; c < 8; c++)
        acc += cic_weight(c, res, 1.0) * mesh[cic_index(c, ic, nmesh)];
    if(comp < 3)
        out[3 * i + comp] = acc;
    else
        out[i] += acc;
}

// Forces from the potential mesh by the 4-point central difference
//     F = -[ 2/3 (phi[+1] - phi[-1]) - 1/12 (phi[+2] - phi[-2]) ] N / Box          (periodic)
// This IS the reference's force_transfer (gravpm.c:456-489): its Fourier-space factor i * (-diff_kernel(w)) N/Box,
// diff_kernel(w) = (8 sin w - sin 2w) / 6 ("the same as GADGET-2 but in fourier space: c1 = 2/3, c2 = 1/12"), is the symbol of
// exactly this stencil, so differencing the potential in real space replaces three of the four inverse transforms (and their
// transfer sweeps); the results differ from the Fourier-space form by rounding only.
//
// readout_potential + readout_force_x/y/z (gravpm.c:491-510, petapm.c:1106-1144) in ONE pass without force meshes (round 4): the force at
// a CIC corner is the 4-point difference of the potential there (above: the reference's force_transfer in real space), so
// a particle gathers, per corner, the potential and its 12 stencil neighbours straight from the potential mesh and differences on the
// fly.  104 gathers per particle instead of 32 - but from ONE mesh, with the z neighbours in the same cache line and the lanes of a wave
// (particles come in some spatial order: Peano-Hilbert after a domain decomposition, lattice order in initial conditions) sharing lines -
// and the gradient pass with its 3 x Nmesh^3 stores (4.3 GB moved at Nmesh = 512) is gone: gradient 1.5 ms + four read-outs 1.6 ms ->
// 1.2 ms at 256^3 / 512^3, PM 9.9 -> 7.9 ms.  Same weights and corner order as k_cic_readout.  (The force meshes and four read-out passes
// of rounds 2-3 are removed: DESIGN.md 3.3.)
// (Measured against it and not kept, profiles/r04a_experiments: the potential staged in LDS tiles of 16^3 cells + halo, 74 KB per block,
// with the particles grouped by tile first - 2.0 ms + 0.5 ms for the grouping; the same gathers in tile order - 1.6 + 0.5 ms.)
__global__ void __launch_bounds__(256) k_cic_readout_stencil(int64_t n, const double *__restrict__ pos, const uint8_t *__restrict__ active,
                                                             double cellsize, int nmesh, double scale, const double *__restrict__ phi,
                                                             double *__restrict__ gravpm, double *__restrict__ potential)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if(i >= n)
        return;
    if(active && !active[i]) // garbage / swallowed: outside every region (gravpm.c:176-179)
        return;
    size_t wi[3][6]; // the six rows per axis, times the axis stride
    double res[3], a[4];
    const size_t stride[3] = {(size_t)nmesh * nmesh, (size_t)nmesh, 1};
    int ic[3];
    cic_cell3(pos + 3 * i, cellsize, nmesh, ic, res);
#pragma unroll
    for(int k = 0; k < 3; k++)
        stencil_rows(ic[k], nmesh, stride[k], wi[k]);
    cic_stencil_gather(wi, res, scale, phi, a);
    if(potential)
        potential[i] += a[0];
#pragma unroll
    for(int k = 0; k < 3; k++)
        gravpm[3 * i + k] = a[1 + k];
}

// the same for a slab: potential and forces of the listed targets in one pass from the slab's potential, which is stored with two ghost
// planes below plane 0 and planes P .. P+2 above (x is not wrapped: the neighbours' planes are there; y and z wrap)
__global__ void __launch_bounds__(256) k_cic_readout_slab_stencil(int64_t nt, const int *__restrict__ targets, const double *__restrict__ pos,
                                                                  double cellsize, int nmesh, int x0, int P, double scale,
                                                                  const double *__restrict__ phi /* plane -2 first */, double *__restrict__ gravpm,
                                                                  double *__restrict__ potential, unsigned *__restrict__ err)
{
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if(t >= nt)
        return;
    const int64_t i = targets ? targets[t] : t; // (no list: every row whose base cell lies in the slab is a target, the others are skipped)
    size_t wi[3][6];
    double res[3], a[4];
    const size_t stride[3] = {(size_t)nmesh * nmesh, (size_t)nmesh, 1};
    const int ix = cic_cell(pos[3 * i], cellsize, nmesh, res[0]);
    if(!in_slab(ix, x0, P)) { // not this rank's slab: an error in a caller's target list
        if(targets)
            atomicExch(err, 1u);
        return;
    }
    stencil_rows_ghost(ix - x0, stride[0], wi[0]);
#pragma unroll
    for(int k = 1; k < 3; k++)
        stencil_rows(cic_cell(pos[3 * i + k], cellsize, nmesh, res[k]), nmesh, stride[k], wi[k]);
    cic_stencil_gather(wi, res, scale, phi, a);
    if(potential)
        potential[i] += a[0];
#pragma unroll
    for(int k = 0; k < 3; k++)
        gravpm[3 * i + k] = a[1 + k];
}

void PMesh::init(double BoxSize, double Asmth_, int Nmesh_, double G_, hipStream_t st)
{
    destroy();
    MPG_CHECK(Nmesh_ >= 2 && (Nmesh_ % 2) == 0, "gravpm_init_periodic: Nmesh must be even and >= 2");
    box = BoxSize;
    Asmth = Asmth_;
    nmesh = Nmesh_;
    G = G_;
    cellsize = box / nmesh; // petapm.c:112
    dep_single = DepositState(); // (the faster deposit form is chosen again on the next particle set)
    dep_slab = DepositState();
    // the meshes and the 3-D plans are made by the first gravpm_force (ensure_single): the slab-decomposed form never needs them
    // per-index tables: 1/sinc^2(pi k / N) (gravpm.c:412-418) and the differencing factor (gravpm.c:482)
    std::vector<double> is2(nmesh), dff(nmesh);
    for(int i = 0; i < nmesh; i++) {
        const int k = i <= nmesh / 2 ? i : i - nmesh;
        double tmp = (k * M_PI) / nmesh;
        double s = (tmp < 1e-5 && tmp > -1e-5) ? 1.0 - tmp * tmp / 6. + tmp * tmp * tmp * tmp / 120. : sin(tmp) / tmp;
        is2[i] = 1. / (s * s);
        const double w = k * (2 * M_PI / nmesh);
        dff[i] = -1 * (1 / 6.0 * (8 * sin(w) - sin(2 * w))) * (nmesh / box);
    }
    invsinc2.reserve(nmesh);
    difffac.reserve(nmesh);
    MPG_HIP(hipMemcpyAsync(invsinc2.p, is2.data(), nmesh * sizeof(double), hipMemcpyHostToDevice, st));
    MPG_HIP(hipMemcpyAsync(difffac.p, dff.data(), nmesh * sizeof(double), hipMemcpyHostToDevice, st));
    MPG_HIP(hipStreamSynchronize(st));
}

// ---- rocFFT plans (petapm.c:284-357 builds its PFFT plans here) ------------------------------------------------------------------
void FftPlan::create(rocfft_result_placement placement, rocfft_transform_type type, int dims, const size_t *lengths, size_t batch)
{
    static const bool once = (rocfft_setup(), true);
    (void)once;
    destroy();
    MPG_FFT(rocfft_plan_create(&plan, placement, type, rocfft_precision_double, (size_t)dims, lengths, batch, nullptr));
    MPG_FFT(rocfft_execution_info_create(&info));
    size_t wb = 0;
    MPG_FFT(rocfft_plan_get_work_buffer_size(plan, &wb));
    if(wb > 0) {
        work.reserve(wb + 64);
        MPG_FFT(rocfft_execution_info_set_work_buffer(info, work.p, wb));
    }
}

void FftPlan::exec(void *in, void *out, hipStream_t st)
{
    MPG_FFT(rocfft_execution_info_set_stream(info, st));
    void *ib[1] = {in}, *ob[1] = {out};
    MPG_FFT(rocfft_execute(plan, ib, out == in ? nullptr : ob, info));
}

void FftPlan::destroy()
{
    if(info)
        (void)rocfft_execution_info_destroy(info);
    if(plan)
        (void)rocfft_plan_destroy(plan);
    info = nullptr;
    plan = nullptr;
    work.release();
}

void PMesh::ensure_single()
{
    if(have_plans)
        return;
    const size_t nreal = (size_t)nmesh * nmesh * nmesh;
    const size_t ncplx = (size_t)nmesh * nmesh * (nmesh / 2 + 1);
    real.reserve(nreal);
    rho_k.reserve(2 * ncplx);
    work_k.reserve(2 * ncplx);
    have_plans = true;
}

void PMesh::ensure_3d()
{
    if(plan_r2c.ready())
        return;
    // x slowest, z fastest: rocFFT takes the lengths fastest first; contiguous real mesh <-> Nmesh^2 (Nmesh/2 + 1) Hermitian half
    const size_t len3[3] = {(size_t)nmesh, (size_t)nmesh, (size_t)nmesh};
    plan_r2c.create(rocfft_placement_notinplace, rocfft_transform_type_real_forward, 3, len3, 1);
    plan_c2r.create(rocfft_placement_notinplace, rocfft_transform_type_real_inverse, 3, len3, 1);
}

bool PMesh::xpass_usable() const { return xp_supported(nmesh) && !kspace_force && !nu_fn && measure_power; }

using XpKernel = void (*)(const double2 *, const double *, double2 *, double *, unsigned long long *, double, double);
static XpKernel xp_kernel(int nmesh)
{
    switch(nmesh) {
    case 64: return k_xpass_solve<64>;
    case 128: return k_xpass_solve<128>;
    case 256: return k_xpass_solve<256>;
    case 512: return k_xpass_solve<512>;
    case 1024: return k_xpass_solve<1024>;
    }
    return nullptr;
}
static size_t xp_lds_bytes(int nmesh) { return (size_t)nmesh * xp_cols(nmesh) * sizeof(double2) + (size_t)nmesh * 3 * sizeof(double); }

void PMesh::ensure_xpass(hipStream_t st)
{
    if(plan2_r2c.ready())
        return;
    const size_t len2[2] = {(size_t)nmesh, (size_t)nmesh};
    plan2_r2c.create(rocfft_placement_notinplace, rocfft_transform_type_real_forward, 2, len2, (size_t)nmesh);
    plan2_c2r.create(rocfft_placement_notinplace, rocfft_transform_type_real_inverse, 2, len2, (size_t)nmesh);
    std::vector<double> tw(2 * (size_t)nmesh);
    for(int m = 0; m < nmesh; m++) { // in extended precision, rounded once
        const long double a = -2 * M_PIl * m / nmesh;
        tw[2 * m] = (double)cosl(a);
        tw[2 * m + 1] = (double)sinl(a);
    }
    xp_tw.reserve(tw.size());
    MPG_HIP(hipMemcpyAsync(xp_tw.p, tw.data(), tw.size() * sizeof(double), hipMemcpyHostToDevice, st));
    MPG_HIP(hipStreamSynchronize(st));
    // (the tile and the histograms are more than the 64 KiB a launch may ask for unannounced)
    MPG_HIP(hipFuncSetAttribute((const void *)xp_kernel(nmesh), hipFuncAttributeMaxDynamicSharedMemorySize, (int)xp_lds_bytes(nmesh)));
    // two blocks per CU hold a tile each, and a block's share is whole work items
    int dev = 0, cus = 0;
    MPG_HIP(hipGetDevice(&dev));
    MPG_HIP(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev));
    const int items = nmesh * (nmesh / 2 / xp_cols(nmesh) + 1);
    xp_blocks = std::max(1, std::min(items, 2 * cus));
}

void PMesh::xpass_solve(hipStream_t st)
{
    ps_zero(st);
    hipLaunchKernelGGL(xp_kernel(nmesh), dim3(xp_blocks), dim3(nmesh / 8 * xp_cols(nmesh)), xp_lds_bytes(nmesh), st, (const double2 *)xp_tw.p,
                       (const double *)invsinc2.p, (double2 *)rho_k.p, ps_acc.p, ps_modes.p, asmth2(), pot_factor());
}

void PMesh::ps_zero(hipStream_t st)
{
    ps_acc.reserve(2 * (size_t)nmesh + 8);
    ps_modes.reserve((size_t)nmesh + 8);
    MPG_HIP(hipMemsetAsync(ps_acc.p, 0, (2 * (size_t)nmesh + 1) * sizeof(double), st));
    MPG_HIP(hipMemsetAsync(ps_modes.p, 0, (size_t)nmesh * sizeof(unsigned long long), st));
    ps_valid = true;
    ps_nmesh = nmesh;
}

void PMesh::nu_fetch(hipStream_t st, double **acc, unsigned long long **modes)
{
    const size_t nb = (size_t)nmesh, want = 3 * nb + 1;
    if(nu_host_cap < want) {
        if(nu_host)
            (void)hipHostFree(nu_host);
        nu_host = nullptr;
        nu_host_cap = 0;
        MPG_HIP(hipHostMalloc((void **)&nu_host, want * sizeof(double), hipHostMallocDefault));
        nu_host_cap = want;
    }
    MPG_HIP(hipMemcpyAsync(nu_host, ps_acc.p, (2 * nb + 1) * sizeof(double), hipMemcpyDeviceToHost, st));
    MPG_HIP(hipMemcpyAsync(nu_host + 2 * nb + 1, ps_modes.p, nb * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
    MPG_HIP(hipStreamSynchronize(st));
    *acc = nu_host;
    *modes = (unsigned long long *)(nu_host + 2 * nb + 1);
}

void PMesh::nu_table(const double *acc, const unsigned long long *modes, hipStream_t st)
{
    // compute_neutrino_power, gravpm.c:308-326: powerspectrum_sum, Power -> sqrt(Power) = delta_cdm, delta_nu_from_power, zero
    const int nb = nmesh;
    MPG_CHECK(ps_lds_bytes_nu() <= 65536, std::string(nu_who) + ": the neutrino response keeps its table in LDS: Nmesh " + std::to_string(nmesh) + " is too large");
    std::vector<double> kk(nb), dcdm(nb), tab(2 * (size_t)nb, 0.0);
    std::vector<int64_t> nm(nb);
    int nonzero = 0;
    if(mpg_powerspectrum_sum(nb, acc, (const int64_t *)modes, nu_box_mpc, kk.data(), dcdm.data(), nm.data(), &nonzero) != 0)
        throw Error(mpg_last_error());
    for(int i = 0; i < nonzero; i++)
        dcdm[i] = sqrt(dcdm[i]);
    double prefac = NAN, mtot = NAN;
    double *lk = tab.data(), *rt = tab.data() + nb;
    for(int i = 0; i < nonzero; i++)
        lk[i] = rt[i] = NAN;
    const int rc = nu_fn(nu_ctx, nonzero, kk.data(), dcdm.data(), nm.data(), lk, rt, &prefac, &mtot);
    MPG_CHECK(rc == 0, std::string(nu_who) + ": the neutrino response callback failed (returned " + std::to_string(rc) + ")");
    MPG_CHECK(nonzero >= 2, std::string(nu_who) + ": neutrino response table: " + std::to_string(nonzero) + " power spectrum bins, at least 2 needed");
    MPG_CHECK(std::isfinite(prefac) && std::isfinite(mtot), std::string(nu_who) + ": neutrino response callback: nu_prefac / MtotbyMcdm not finite");
    for(int i = 0; i < nonzero; i++) {
        MPG_CHECK(std::isfinite(lk[i]) && std::isfinite(rt[i]),
                  std::string(nu_who) + ": neutrino response table: entry " + std::to_string(i) + " is not finite");
        MPG_CHECK(i == 0 || lk[i] > lk[i - 1], std::string(nu_who) + ": neutrino response table: logknu is not strictly increasing at entry " + std::to_string(i));
    }
    // per log-k bin the table interval to start from: the bin's position among the non-empty bins (the table is their log kk)
    std::vector<int> guess(nb);
    int c = 0;
    for(int b = 0; b < nb; b++) {
        guess[b] = std::min(std::max(c - 1, 0), nonzero - 2);
        if(modes[b])
            c++;
    }
    nu_tab.reserve(2 * (size_t)nb);
    nu_guess.reserve((size_t)nb);
    // (through the pinned buffer: the raw sums in it have been read)
    memcpy(nu_host, tab.data(), 2 * (size_t)nb * sizeof(double));
    memcpy(nu_host + 2 * (size_t)nb, guess.data(), (size_t)nb * sizeof(int));
    MPG_HIP(hipMemcpyAsync(nu_tab.p, nu_host, 2 * (size_t)nb * sizeof(double), hipMemcpyHostToDevice, st));
    MPG_HIP(hipMemcpyAsync(nu_guess.p, nu_host + 2 * (size_t)nb, (size_t)nb * sizeof(int), hipMemcpyHostToDevice, st));
    nu_nonzero = nonzero;
    nu_prefac = prefac;
    nu_normfac = mtot * mtot;
    ps_zero(st); // the second measurement: total matter (powerspectrum_zero, gravpm.c:325)
}

__global__ void __launch_bounds__(256) k_tracer_mass(int64_t n, const float *__restrict__ mass, const uint8_t *__restrict__ type,
                                                     float *__restrict__ out)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if(i < n)
        out[i] = type[i] == 2 ? 0.0f : mass[i]; // hybrid_nu_gravpm_is_active, gravpm.c:469-474
}

const float *PMesh::tracer_mass(int64_t n, const float *d_mass, const uint8_t *d_type, hipStream_t st)
{
    if(!hybrid_tracer || n <= 0)
        return d_mass;
    MPG_CHECK(d_type != nullptr, "gravpm_force: the hybrid-neutrino deposit mask needs the particle types");
    tracer_mass_buf.reserve((size_t)n);
    hipLaunchKernelGGL(k_tracer_mass, dim3(nblk(n)), dim3(256), 0, st, n, d_mass, d_type, tracer_mass_buf.p);
    return tracer_mass_buf.p;
}

void PMesh::destroy()
{
    plan_r2c.destroy();
    plan_c2r.destroy();
    plan2_r2c.destroy();
    plan2_c2r.destroy();
    have_plans = false;
    slab_destroy();
    real.release();
    rho_k.release();
    work_k.release();
    if(nu_host)
        (void)hipHostFree(nu_host);
    nu_host = nullptr;
    nu_host_cap = 0;
    nmesh = 0;
}

// CIC deposit onto the x-planes [x0, x0 + P) of `mesh` (zeroed by the caller): plain atomics, or cell-sorted with wave-aggregated
// atomics; the first call and every 64th time both forms on the set at hand and keep the faster one.
void PMesh::deposit(int64_t n, const double *d_pos, const float *d_mass, const uint8_t *d_active, double *mesh, int x0, int P, DepositState &ds,
                    hipStream_t st, EventTimer *tm)
{
    const size_t ncell = (size_t)P * nmesh * nmesh, nreal = (size_t)nmesh * nmesh * nmesh;
    const bool whole = x0 == 0 && P == nmesh;
    auto plain = [&]() {
        if(whole)
            hipLaunchKernelGGL(k_cic_deposit, dim3(nblk(2 * n)), dim3(256), 0, st, n, d_pos, d_mass, d_active, cellsize, nmesh, mesh);
        else
            hipLaunchKernelGGL(k_cic_deposit_slab, dim3(nblk(n)), dim3(256), 0, st, n, d_pos, d_mass, d_active, cellsize, nmesh, x0, P, mesh);
    };
    auto sorted = [&]() {
        dep_keys_a.reserve((size_t)n + 1);
        dep_keys_b.reserve((size_t)n + 1);
        dep_idx_a.reserve((size_t)n + 1);
        dep_idx_b.reserve((size_t)n + 1);
        hipLaunchKernelGGL(k_cell_keys, dim3(nblk(n)), dim3(256), 0, st, n, d_pos, d_active, cellsize, nmesh, dep_keys_a.p, dep_idx_a.p);
        int bits = 1;
        while(bits < 64 && ((unsigned long long)1 << bits) < (unsigned long long)nreal)
            bits++;
        size_t tb = 0;
        MPG_HIP(rocprim::radix_sort_pairs(nullptr, tb, dep_keys_a.p, dep_keys_b.p, dep_idx_a.p, dep_idx_b.p, (size_t)n, 0, 64, st));
        dep_tmp.reserve(tb + 16);
        // (all 64 bits when there are inactive particles: they carry the all-ones key)
        MPG_HIP(rocprim::radix_sort_pairs((void *)dep_tmp.p, tb, dep_keys_a.p, dep_keys_b.p, dep_idx_a.p, dep_idx_b.p, (size_t)n, 0,
                                          d_active ? 64 : bits, st));
        hipLaunchKernelGGL(k_cic_deposit_sorted, dim3(nblk(n)), dim3(256), 0, st, n, dep_keys_b.p, dep_idx_b.p, d_pos, d_mass, cellsize, nmesh, x0, P,
                           mesh);
    };
    if(const char *e = getenv("MPG_PM_DEPOSIT")) // experiment knob: "plain" / "sorted"
        ds.mode = !strcmp(e, "sorted") ? 2 : 1;
    if(ds.mode == 0 || ++ds.since_tune >= 64) {
        hipEvent_t e0, e1, e2;
        MPG_HIP(hipEventCreate(&e0));
        MPG_HIP(hipEventCreate(&e1));
        MPG_HIP(hipEventCreate(&e2));
        MPG_HIP(hipEventRecord(e0, st));
        sorted();
        MPG_HIP(hipEventRecord(e1, st));
        MPG_HIP(hipMemsetAsync(mesh, 0, ncell * sizeof(double), st));
        plain();
        MPG_HIP(hipEventRecord(e2, st));
        MPG_HIP(hipEventSynchronize(e2));
        float ts = 0, tp = 0;
        MPG_HIP(hipEventElapsedTime(&ts, e0, e1));
        MPG_HIP(hipEventElapsedTime(&tp, e1, e2));
        (void)hipEventDestroy(e0);
        (void)hipEventDestroy(e1);
        (void)hipEventDestroy(e2);
        ds.mode = ts < tp ? 2 : 1;
        ds.since_tune = 0;
        if(tm)
            tm->start(st); // the trial is not the deposit's time
        MPG_HIP(hipMemsetAsync(mesh, 0, ncell * sizeof(double), st));
    }
    if(ds.mode == 2)
        sorted();
    else
        plain();
}

// One k_power_spectrum pass over rho (ny rows of ky from y0 in the layout XLAST) with `grid` blocks.  Without NU it starts a
// measurement and zeroes the accumulators; with NU it is the second one, whose accumulators and table nu_table has just made.
template <bool XLAST, bool FUSE, bool NU>
void PMesh::measure_spectrum(double *rho, int ny, int y0, unsigned grid, hipStream_t st)
{
    if(!NU)
        ps_zero(st);
    const NuArgs na = NU ? NuArgs{nu_tab.p, nu_guess.p, nu_nonzero, nu_prefac, nu_normfac, 2 * M_PI / nu_box_mpc} : NuArgs{};
    hipLaunchKernelGGL((k_power_spectrum<XLAST, FUSE, NU>), dim3(grid), dim3(256), NU ? ps_lds_bytes_nu() : ps_lds_bytes(), st, nmesh, ny, y0,
                       invsinc2.p, (double2 *)rho, ps_acc.p, ps_modes.p, FUSE ? asmth2() : 0.0, FUSE ? pot_factor() : 0.0, na);
}

// The transfer stage: rho, the density in Fourier space, becomes the potential.  Three cases -
//   measure            P(k) of the field as deposited (measure_power), then the potential transfer;
//   neutrino response  (nu_fn) that measurement, the host step (the raw sums fetched, nu_table), then every mode times nufac, measured
//                      again, and the transfer (see pm.h);
//   fused              (FUSE: MPG_PM_FUSE_PS unset or not 0, single mesh only) the last measurement and the transfer in one pass over rho
// - in two parts around the host step: the slab form runs them apart (forward_b1, forward_b2), the caller sums the bins over the
// ranks and runs nu_table between them.
template <bool XLAST, bool FUSE>
void PMesh::transfer_stage(int parts, double *rho, int ny, int y0, unsigned grid, hipStream_t st)
{
    if((parts & TR_MEASURE) && (nu_fn || (measure_power && !FUSE)))
        measure_spectrum<XLAST, false, false>(rho, ny, y0, grid, st);
    if(parts == TR_BOTH && nu_fn) {
        double *acc;
        unsigned long long *modes;
        nu_fetch(st, &acc, &modes);
        nu_table(acc, modes, st);
    }
    if(!(parts & TR_APPLY))
        return;
    if(nu_fn)
        measure_spectrum<XLAST, FUSE, true>(rho, ny, y0, grid, st);
    else if(FUSE && measure_power)
        measure_spectrum<XLAST, FUSE, false>(rho, ny, y0, grid, st);
    if(!FUSE || !(nu_fn || measure_power))
        hipLaunchKernelGGL(k_potential_transfer<XLAST>, dim3(nblk((size_t)nmesh * ny * (nmesh / 2 + 1))), dim3(256), 0, st, nmesh, ny, y0, asmth2(),
                           pot_factor(), invsinc2.p, (double2 *)rho);
}

double PMesh::plane_nu_correction(int64_t n, const double *d_pos, const float *d_mass, const uint8_t *d_active, mpg_nu_response_fn fn, void *ctx,
                                  double box_mpc, hipStream_t st)
{
    MPG_CHECK(nmesh > 0, "potential planes: the massive-neutrino correction needs the PM mesh (gravpm_init_periodic first)"); // plane.c:620
    MPG_CHECK(!slab.ready, "potential planes: the massive-neutrino correction is not available while the mesh is in its slab-decomposed form");
    MPG_CHECK(fn && box_mpc > 0, "potential planes: the massive-neutrino correction needs a callback and BoxSize_in_MPC > 0");
    ensure_single();
    ensure_3d();
    const size_t nreal = (size_t)nmesh * nmesh * nmesh, nb = (size_t)nmesh;
    // what the last PM step left for mpg_gravpm_get_powerspectrum is set aside
    // (ps_valid survives gravpm_init_periodic: after a change of Nmesh without a PM step the accumulators are still the old mesh's and
    // hold nothing a caller could ask for; ps_valid then comes out false, whatever capacity the buffers happen to have)
    const bool had_ps = ps_valid && ps_nmesh == nmesh;
    if(had_ps) {
        ps_keep.reserve(3 * nb + 1);
        MPG_HIP(hipMemcpyAsync(ps_keep.p, ps_acc.p, (2 * nb + 1) * sizeof(double), hipMemcpyDeviceToDevice, st));
        MPG_HIP(hipMemcpyAsync(ps_keep.p + 2 * nb + 1, ps_modes.p, nb * sizeof(unsigned long long), hipMemcpyDeviceToDevice, st));
    }
    struct Restore { // (also when the callback's table is refused)
        PMesh *pm;
        mpg_nu_response_fn fn;
        void *ctx;
        double box_mpc, prefac, normfac;
        int nonzero;
        bool had_ps;
        hipStream_t st;
        ~Restore()
        {
            pm->nu_who = "gravpm_force";
            pm->nu_fn = fn;
            pm->nu_ctx = ctx;
            pm->nu_box_mpc = box_mpc;
            pm->nu_prefac = prefac;
            pm->nu_normfac = normfac;
            pm->nu_nonzero = nonzero;
            pm->ps_valid = had_ps;
            if(had_ps) {
                const size_t nb = (size_t)pm->nmesh;
                (void)hipMemcpyAsync(pm->ps_acc.p, pm->ps_keep.p, (2 * nb + 1) * sizeof(double), hipMemcpyDeviceToDevice, st);
                (void)hipMemcpyAsync(pm->ps_modes.p, pm->ps_keep.p + 2 * nb + 1, nb * sizeof(unsigned long long), hipMemcpyDeviceToDevice, st);
            }
        }
    } restore{this, nu_fn, nu_ctx, nu_box_mpc, nu_prefac, nu_normfac, nu_nonzero, had_ps, st};
    MPG_HIP(hipMemsetAsync(real.p, 0, nreal * sizeof(double), st));
    if(n > 0)
        deposit(n, d_pos, d_mass, d_active, real.p, 0, nmesh, dep_plane, st, nullptr);
    plan_r2c.exec(real.p, rho_k.p, st);
    measure_spectrum<false, false, false>(rho_k.p, nmesh, 0, 2048, st);
    double total_mass = 0;
    MPG_HIP(hipMemcpyAsync(&total_mass, rho_k.p, sizeof(double), hipMemcpyDeviceToHost, st));
    double *acc;
    unsigned long long *modes;
    nu_fetch(st, &acc, &modes); // (waits for the stream)
    MPG_CHECK(total_mass > 0, "potential planes: cannot build a potential plane from zero active particle mass"); // plane.c:161
    nu_who = "potential planes";
    nu_fn = fn;
    nu_ctx = ctx;
    nu_box_mpc = box_mpc;
    nu_table(acc, modes, st);
    const NuArgs na{nu_tab.p, nu_guess.p, nu_nonzero, nu_prefac, nu_normfac, 2 * M_PI / nu_box_mpc};
    hipLaunchKernelGGL(k_nu_correction, dim3(2048), dim3(256), (size_t)nmesh * (2 * sizeof(double) + sizeof(int)), st, nmesh, (double2 *)rho_k.p, na);
    MPG_HIP(hipGetLastError());
    plan_c2r.exec(rho_k.p, real.p, st);
    return total_mass;
}

void PMesh::force(int64_t n, const double *d_pos, const float *d_mass, const uint8_t *d_active, double *d_gravpm, double *d_potential,
                  hipStream_t st, EventTimer *tm)
{
    MPG_CHECK(nmesh > 0, "gravpm_force called before gravpm_init_periodic");
    MPG_CHECK(!slab.ready, "gravpm_force: the mesh is in its slab-decomposed form (use the pm_slab calls)");
    ensure_single();
    const size_t nreal = (size_t)nmesh * nmesh * nmesh;
    const size_t ncplx = (size_t)nmesh * nmesh * (nmesh / 2 + 1);
    float t_fft = 0, t_tr = 0, t_ro = 0;
    auto lap = [&](float &sum) { // the time since the last lap is added to `sum`
        float t;
        if(tm) {
            tm->lap(st, &t);
            sum += t;
        }
    };
    if(tm)
        tm->start(st);
    // pm_init_regions zeroes the mesh (petapm.c:932-952); deposit
    MPG_HIP(hipMemsetAsync(real.p, 0, nreal * sizeof(double), st));
    if(n > 0)
        deposit(n, d_pos, d_mass, d_active, real.p, 0, nmesh, dep_single, st, tm);
    if(tm)
        tm->lap(st, &tm->t.pm_deposit);
    static const bool fuse_ps = !(getenv("MPG_PM_FUSE_PS") && getenv("MPG_PM_FUSE_PS")[0] == '0');
    // the default step on a mesh the kernel is built for: 2-D transforms over (y, z) and the x-transforms fused with the transfer stage
    // (k_xpass_solve); MPG_PM_XPASS=0 (read on every call) keeps the 3-D plans
    const char *xe = getenv("MPG_PM_XPASS");
    const bool xpass = fuse_ps && xpass_usable() && !(xe && xe[0] == '0');
    if(xpass) {
        ensure_xpass(st);
        plan2_r2c.exec(real.p, rho_k.p, st);
        lap(t_fft);
        xpass_solve(st);
        lap(t_tr);
        plan2_c2r.exec(rho_k.p, real.p, st);
    }
    else {
        ensure_3d();
        plan_r2c.exec(real.p, rho_k.p, st);
        lap(t_fft);
        if(fuse_ps) // P(k) and the potential transfer in one pass over rho_k (round 6)
            transfer_stage<false, true>(TR_BOTH, rho_k.p, nmesh, 0, 2048, st);
        else
            transfer_stage<false, false>(TR_BOTH, rho_k.p, nmesh, 0, 2048, st);
        lap(t_tr);
    }
    // functions[] = Potential, ForceX, ForceY, ForceZ (gravpm.c:32-39).  Default: one inverse transform (the potential), the
    // forces by differencing it in real space (k_cic_readout_stencil: the same operator as force_transfer); kspace_force restores
    // the reference's four inverse transforms.
    if(!kspace_force) {
        if(!xpass)
            plan_c2r.exec(rho_k.p, real.p, st); // rho_k is consumed: it is not needed again
        lap(t_fft);
        // potential and forces in one read-out pass straight from the potential mesh (k_cic_readout_stencil)
        if(n > 0)
            hipLaunchKernelGGL(k_cic_readout_stencil, dim3(nblk(n)), dim3(256), 0, st, n, d_pos, d_active, cellsize, nmesh, (double)nmesh / box,
                               (const double *)real.p, d_gravpm, d_potential);
        lap(t_ro);
    }
    else
        for(int f = 0; f < 4; f++) {
        const int axis = f - 1;
        if(f == 0 && !d_potential)
            continue;
        hipLaunchKernelGGL(k_force_transfer<false>, dim3(nblk(ncplx)), dim3(256), 0, st, nmesh, nmesh, 0, axis, difffac.p,
                           (const double2 *)rho_k.p, (double2 *)work_k.p, 1, 0);
        lap(t_tr);
        plan_c2r.exec(work_k.p, real.p, st);
        lap(t_fft);
        if(n > 0) {
            if(f == 0)
                hipLaunchKernelGGL(k_cic_readout, dim3(nblk(n)), dim3(256), 0, st, n, d_pos, d_active, cellsize, nmesh, real.p, 3, d_potential);
            else
                hipLaunchKernelGGL(k_cic_readout, dim3(nblk(n)), dim3(256), 0, st, n, d_pos, d_active, cellsize, nmesh, real.p, axis, d_gravpm);
        }
        lap(t_ro);
    }
    MPG_HIP(hipGetLastError());
    if(tm && tm->enabled) {
        tm->t.pm_fft = t_fft;
        tm->t.pm_transfer = t_tr;
        tm->t.pm_readout = t_ro;
        tm->t.pm_total = tm->t.pm_deposit + t_fft + t_tr + t_ro;
    }
}

// ================================================================================================ slab-decomposed form
// Reference: petapm.c lays the mesh out in 2-D pencils over all ranks and moves particles' "region" meshes to them and back
// (petapm.c:584-885); PFFT transposes between the three 1-D transform stages.  With <= 8 GPUs on one node a 1-D (slab)
// decomposition needs one transpose per 3-D transform and keeps every message large (xGMI is point-to-point: 7 peers x one
// contiguous block each).  Every rank holds all particle positions, so instead of exchanging region
// meshes each rank deposits, straight into its own planes, the part of every particle's CIC cloud that falls on them, and
// reads forces back for the particles whose base cell lies in its slab (one ghost plane from the next rank).
//
//   forward_a : deposit -> 2-D r2c over (y,z) of the P own planes -> pack by destination ky-slab     [sendA]
//   all-to-all (caller)                                                                               [recvA = [x][ky local][kz]]
//   forward_b : tiled transpose to [ky local][kz][kx] -> 1-D c2c along x (contiguous rows) -> potential transfer -> inverse 1-D
//               c2c -> tiled transpose back to [x][ky local][kz] (the block for rank d, its x-planes, is contiguous)  [sendB]
//   all-to-all (caller)                                                                               [recvB]
//   inverse_c : unpack to [x local][ky][kz] -> 2-D c2r -> the potential slab; its first 3 / last 2 planes out as ghosts [ghost_send]
//   neighbour exchange (caller) -> readout: forces by differencing the potential during the CIC readout (k_cic_readout_slab_stencil).
// rocFFT transforms are unnormalised like PFFT's; the three 1-D stages compose to the same 3-D DFT.

// C[xl][y][z] -> sendA[d][xl][yl][z], d = y / Py
__global__ void __launch_bounds__(256) k_slab_pack_a(int nmesh, int P, int Py, const double2 *__restrict__ C, double2 *__restrict__ sendA)
{
    const int nz = nmesh / 2 + 1;
    const size_t total = (size_t)P * nmesh * nz;
    const size_t ip = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if(ip >= total)
        return;
    const int iz = (int)(ip % nz);
    const size_t t = ip / nz;
    const int y = (int)(t % nmesh);
    const int xl = (int)(t / nmesh);
    const int d = y / Py, yl = y - d * Py;
    sendA[(((size_t)d * P + xl) * Py + yl) * nz + iz] = C[ip];
}

// recvB[s][xl][yl][z] -> C[xl][y = s Py + yl][z]
__global__ void __launch_bounds__(256) k_slab_unpack_b(int nmesh, int P, int Py, const double2 *__restrict__ recvB, double2 *__restrict__ C)
{
    const int nz = nmesh / 2 + 1;
    const size_t total = (size_t)P * nmesh * nz;
    const size_t ip = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if(ip >= total)
        return;
    const int iz = (int)(ip % nz);
    const size_t t = ip / nz;
    const int y = (int)(t % nmesh);
    const int xl = (int)(t / nmesh);
    const int s = y / Py, yl = y - s * Py;
    C[ip] = recvB[(((size_t)s * P + xl) * Py + yl) * nz + iz];
}

// out[c * out_ld + r] = in[r * in_ld + c] for r < rows, c < cols (complex doubles), through a 32 x 32 LDS tile so that both the
// reads and the writes are coalesced.  The 1-D transforms along x then run on contiguous rows: rocFFT's strided plan for the
// same transform (stride Py*Nz, batch Py*Nz) measured 2.06 ms against 0.4 ms + 0.5 ms for transpose + contiguous transform.
__global__ void __launch_bounds__(256) k_transpose(int rows, int cols, const double2 *__restrict__ in, size_t in_ld, double2 *__restrict__ out,
                                                   size_t out_ld)
{
    __shared__ double2 tile[32][33];
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5; // 32 x 8
    const int c0 = blockIdx.x * 32, r0 = blockIdx.y * 32;
#pragma unroll
    for(int k = 0; k < 32; k += 8) {
        const int r = r0 + ty + k, c = c0 + tx;
        if(r < rows && c < cols)
            tile[ty + k][tx] = in[(size_t)r * in_ld + c];
    }
    __syncthreads();
#pragma unroll
    for(int k = 0; k < 32; k += 8) {
        const int c = c0 + ty + k, r = r0 + tx;
        if(r < rows && c < cols)
            out[(size_t)c * out_ld + r] = tile[tx][ty + k];
    }
}

void PMesh::slab_destroy()
{
    if(slab.ready) {
        slab.p2d_r2c.destroy();
        slab.p2d_c2r.destroy();
        slab.p1d_fwd.destroy();
        slab.p1d_inv.destroy();
        slab.ready = false;
    }
    slab.phi.release();
    slab.force.release();
    slab.C.release();
    slab.rho_k.release();
    slab.work.release();
}

void PMesh::slab_init(int rank, int world)
{
    MPG_CHECK(nmesh > 0, "pm_slab_init called before gravpm_init_periodic");
    MPG_CHECK(world >= 1 && rank >= 0 && rank < world, "pm_slab_init: bad rank / world");
    MPG_CHECK(nmesh % world == 0, "pm_slab_init: Nmesh must be a multiple of the number of GPUs");
    slab_destroy();
    slab.rank = rank;
    slab.world = world;
    slab.P = slab.Py = nmesh / world;
    const int nz = nmesh / 2 + 1;
    const size_t S = (size_t)slab.Py * nz;
    MPG_CHECK(slab.P >= 3, "pm_slab_init: at least 3 mesh planes per GPU are needed");
    slab.phi.reserve((size_t)(slab.P + 5) * nmesh * nmesh);
    slab.force.reserve((size_t)(slab.P + 1) * nmesh * nmesh);
    slab.C.reserve(2 * (size_t)slab.P * nmesh * nz);
    slab.rho_k.reserve(2 * (size_t)nmesh * S);
    // the single-GPU meshes and plans are not needed in this form
    plan_r2c.destroy();
    plan_c2r.destroy();
    plan2_r2c.destroy();
    plan2_c2r.destroy();
    have_plans = false;
    real.release();
    rho_k.release();
    work_k.release();
    const size_t len2[2] = {(size_t)nmesh, (size_t)nmesh}, len1[1] = {(size_t)nmesh};
    slab.p2d_r2c.create(rocfft_placement_notinplace, rocfft_transform_type_real_forward, 2, len2, (size_t)slab.P); // the slab's planes
    slab.p2d_c2r.create(rocfft_placement_notinplace, rocfft_transform_type_real_inverse, 2, len2, (size_t)slab.P);
    slab.p1d_fwd.create(rocfft_placement_inplace, rocfft_transform_type_complex_forward, 1, len1, S); // contiguous rows of kx
    slab.p1d_inv.create(rocfft_placement_inplace, rocfft_transform_type_complex_inverse, 1, len1, S);
    slab.work.reserve(2 * (size_t)nmesh * S);
    slab.ready = true;
}

void PMesh::slab_forward_a(int64_t n, const double *d_pos, const float *d_mass, double *sendA, hipStream_t st)
{
    MPG_CHECK(slab.ready, "pm_slab: not initialised");
    const int nz = nmesh / 2 + 1;
    const size_t nreal = (size_t)slab.P * nmesh * nmesh;
    MPG_HIP(hipMemsetAsync(slab.force.p, 0, nreal * sizeof(double), st)); // (the force buffer doubles as the density slab)
    if(n > 0)
        deposit(n, d_pos, d_mass, nullptr, slab.force.p, slab.rank * slab.P, slab.P, dep_slab, st, nullptr);
    slab.p2d_r2c.exec(slab.force.p, slab.C.p, st);
    hipLaunchKernelGGL(k_slab_pack_a, dim3(nblk((size_t)slab.P * nmesh * nz)), dim3(256), 0, st, nmesh, slab.P, slab.Py, (const double2 *)slab.C.p,
                       (double2 *)sendA);
    MPG_HIP(hipGetLastError());
}

void PMesh::slab_forward_b(double *recvA, double *sendB, hipStream_t st)
{
    slab_forward_b1(recvA, st);
    slab_forward_b2(sendB, st);
}

void PMesh::slab_forward_b1(double *recvA, hipStream_t st)
{
    MPG_CHECK(slab.ready, "pm_slab: not initialised");
    const int nz = nmesh / 2 + 1;
    const int y0 = slab.rank * slab.Py;
    const size_t S = (size_t)slab.Py * nz;
    // [x][j] -> [j][x], j = (ky local, kz): the transforms along x run on contiguous rows
    const dim3 tgrid_f((unsigned)((S + 31) / 32), (unsigned)((nmesh + 31) / 32));
    hipLaunchKernelGGL(k_transpose, tgrid_f, dim3(256), 0, st, nmesh, (int)S, (const double2 *)recvA, S, (double2 *)slab.rho_k.p, (size_t)nmesh);
    slab.p1d_fwd.exec(slab.rho_k.p, slab.rho_k.p, st);
    // this rank's ky rows: the caller sums the raw accumulators over the ranks (powerspectrum_sum's Allreduce)
    transfer_stage<true, false>(TR_MEASURE, slab.rho_k.p, slab.Py, y0, 1024, st);
}

void PMesh::slab_forward_b2(double *sendB, hipStream_t st)
{
    MPG_CHECK(slab.ready, "pm_slab: not initialised");
    const int nz = nmesh / 2 + 1;
    const int y0 = slab.rank * slab.Py;
    const size_t S = (size_t)slab.Py * nz;
    const dim3 tgrid_b((unsigned)((nmesh + 31) / 32), (unsigned)((S + 31) / 32));
    // with the response the table is up (nu_table, after the bins were summed over the ranks): nufac + this rank's bins of the total matter
    transfer_stage<true, false>(TR_APPLY, slab.rho_k.p, slab.Py, y0, 1024, st);
    // only the potential is transformed back: the forces are its real-space differences (k_cic_readout_slab_stencil), which also cuts
    // the inverse all-to-all to a quarter
    slab.p1d_inv.exec(slab.rho_k.p, slab.rho_k.p, st);
    // [j][x] -> sendB[x][j]: the block for rank d (its x-planes) is contiguous
    hipLaunchKernelGGL(k_transpose, tgrid_b, dim3(256), 0, st, (int)S, nmesh, (const double2 *)slab.rho_k.p, (size_t)nmesh, (double2 *)sendB, S);
    MPG_HIP(hipGetLastError());
}

void PMesh::slab_inverse_c(const double *recvB, double *ghost_send, hipStream_t st)
{
    MPG_CHECK(slab.ready, "pm_slab: not initialised");
    const int nz = nmesh / 2 + 1;
    const size_t plane = (size_t)nmesh * nmesh;
    hipLaunchKernelGGL(k_slab_unpack_b, dim3(nblk((size_t)slab.P * nmesh * nz)), dim3(256), 0, st, nmesh, slab.P, slab.Py, (const double2 *)recvB,
                       (double2 *)slab.C.p);
    double *phi0 = slab.phi.p + 2 * plane; // plane 0 of the slab; planes -2, -1 and P .. P+2 are ghosts
    slab.p2d_c2r.exec(slab.C.p, phi0, st);
    // ghosts the neighbours need: the first 3 planes go to the previous rank, the last 2 to the next
    MPG_HIP(hipMemcpyAsync(ghost_send, phi0, 3 * plane * sizeof(double), hipMemcpyDeviceToDevice, st));
    MPG_HIP(hipMemcpyAsync(ghost_send + 3 * plane, phi0 + (size_t)(slab.P - 2) * plane, 2 * plane * sizeof(double), hipMemcpyDeviceToDevice, st));
    MPG_HIP(hipGetLastError());
}

// ghost_recv: planes P, P+1, P+2 (the next rank's first three), then planes -2, -1 (the previous rank's last two)
void PMesh::slab_take_ghosts(const double *ghost_recv, hipStream_t st)
{
    const size_t plane = (size_t)nmesh * nmesh;
    MPG_HIP(hipMemcpyAsync(slab.phi.p + (size_t)(2 + slab.P) * plane, ghost_recv, 3 * plane * sizeof(double), hipMemcpyDeviceToDevice, st));
    MPG_HIP(hipMemcpyAsync(slab.phi.p, ghost_recv + 3 * plane, 2 * plane * sizeof(double), hipMemcpyDeviceToDevice, st));
}

// slab_readout for ALL rows of d_pos whose base cell lies in the slab (the rows a rank received for its slab: a particle whose CIC cloud
// straddles two slabs was shipped to both, its base cell's owner reads it out); nothing is read back: no target list, no count
void PMesh::slab_readout_rows(const double *ghost_recv, int64_t nrows, const double *d_pos, double *d_gravpm, double *d_potential, hipStream_t st)
{
    MPG_CHECK(slab.ready, "pm_slab: not initialised");
    slab_take_ghosts(ghost_recv, st);
    if(nrows > 0)
        hipLaunchKernelGGL(k_cic_readout_slab_stencil, dim3(nblk(nrows)), dim3(256), 0, st, nrows, (const int *)nullptr, d_pos, cellsize, nmesh,
                           slab.rank * slab.P, slab.P, (double)nmesh / box, (const double *)slab.phi.p, d_gravpm, d_potential, (unsigned *)nullptr);
    MPG_HIP(hipGetLastError());
}

void PMesh::slab_readout(const double *ghost_recv, const int *targets, int64_t nt, const double *d_pos, double *d_gravpm, double *d_potential,
                         hipStream_t st)
{
    MPG_CHECK(slab.ready, "pm_slab: not initialised");
    DevBuf<unsigned> &flag = slab_err;
    flag.reserve(1);
    MPG_HIP(hipMemsetAsync(flag.p, 0, sizeof(unsigned), st));
    slab_take_ghosts(ghost_recv, st);
    if(nt > 0)
        hipLaunchKernelGGL(k_cic_readout_slab_stencil, dim3(nblk(nt)), dim3(256), 0, st, nt, targets, d_pos, cellsize, nmesh, slab.rank * slab.P,
                           slab.P, (double)nmesh / box, (const double *)slab.phi.p, d_gravpm, d_potential, flag.p);
    MPG_HIP(hipGetLastError());
    unsigned e = 0;
    MPG_HIP(hipMemcpyAsync(&e, flag.p, sizeof(unsigned), hipMemcpyDeviceToHost, st));
    MPG_HIP(hipStreamSynchronize(st));
    MPG_CHECK(e == 0, "pm_slab_readout: a target's base cell is outside this rank's slab");
}

} // namespace mpg
