// uvbg.hip -- excursion-set reionisation (EXCUR_REION): calculate_uvbg (libgadget/uvbg.c:471-594) through petapm_reion
// (petapm.c:381-577) on one gfx950 GPU, for the bound particles of one rank.
//
// Reference pipeline: init_particle_uvbg -> three CIC deposits (put_particle_to_mesh, put_star_to_mesh, put_sfr_to_mesh,
// petapm.c:1138-1162) -> three r2c with divide_by_ncell -> for every radius: filter_pm on the three spectra, three c2r, reion_loop_pm
// over the cells -> readout_J21.  On one rank the regions and pencils only relocate cells: the particles deposit straight into
// UVBGdim^3 meshes (pm_cic.h: the PM's cell, fold and corner order) and read straight back.
//
// Per radius the device streams: one pass over the modes (k_uvbg_filter: reads the 2 or 3 unfiltered spectra, W(kR) once per mode, writes
// as many filtered ones), ONE batched inverse transform, one pass over the cells (k_uvbg_cells: reads the 2 or 3 filtered grids and the two
// float grids J21 / xHI, writes those two).  With B grids and N = UVBGdim^3 that is 16 B N bytes for the filter and (8 B + 16) N for the
// cells, beside the transform's own passes.  The list of radii depends on nothing the device computes, so the whole loop is queued without
// a host wait; the one wait of a call is at its end, for the two neutral fractions and the error word.
#include "engine_internal.h"
#include "pm_cic.h"
#include "uvbg.h"
#include <algorithm>
#include <rocprim/rocprim.hpp>

namespace mpg {

using namespace uvbg;

// init_particle_uvbg (uvbg.c:471-504).  err: a converted escape fraction came out negative (endrun there)
__global__ void __launch_bounds__(256) k_uvbg_init(int64_t n, const uint8_t *__restrict__ type, double *__restrict__ escfrac,
                                                   double *__restrict__ local_J21, int use_sfr, double norm, double unit_conv, double scaling,
                                                   unsigned *__restrict__ err)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if(i >= n)
        return;
    const int t = type ? type[i] : 1;
    if(t == 0) {
        local_J21[i] = 0.;
        if(!use_sfr || escfrac[i] == 0)
            return;
    }
    else if(t == 4) {
        if(escfrac[i] == 0)
            return;
    }
    else
        return;
    double fesc = norm * pow(escfrac[i] * unit_conv, scaling);
    if(fesc > 1)
        fesc = 1;
    if(fesc < 0)
        atomicOr(err, 1u);
    escfrac[i] = fesc;
}

// The three deposits of petapm_reion (petapm.c:531-536) WITHOUT atomics, so that equal input gives equal grids - and with them equal neutral
// fractions - on every run: the rows are sorted by their base cell (a stable radix sort: rows of one cell stay in particle order), and every
// mesh cell then GATHERS, in a fixed order, what the rows of its eight neighbouring base cells put on it.  Cell, fold, corner order and weight
// are those of the PM deposit (pm_cic.h); the addends are (w Mass), (w Mass) fesc and (w Sfr) fesc in the reference's order of
// multiplication.  Rows of type 7 get the key behind every cell and deposit nothing.
__global__ void __launch_bounds__(256) k_uvbg_keys(int64_t n, const double *__restrict__ pos, const uint8_t *__restrict__ type, double cellsize, int dim,
                                                   unsigned *__restrict__ keys, unsigned *__restrict__ idx)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if(i >= n)
        return;
    unsigned key = 0xffffffffu;
    if(!type || type[i] != 7) {
        int ic[3];
        double res[3];
        cic_cell3(pos + 3 * i, cellsize, dim, ic, res);
        key = (unsigned)cic_index(0, ic, dim);
    }
    keys[i] = key;
    idx[i] = (unsigned)i;
}

// start[c] = the first sorted row whose key is >= c, for c = 0 .. ncell (start[ncell]: the rows that deposit)
__global__ void __launch_bounds__(256) k_uvbg_cell_start(int64_t ncell, int64_t n, const unsigned *__restrict__ keys, unsigned *__restrict__ start)
{
    const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if(c > ncell)
        return;
    int64_t lo = 0, hi = n;
    while(lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if((int64_t)keys[mid] < c)
            lo = mid + 1;
        else
            hi = mid;
    }
    start[c] = (unsigned)lo;
}

__global__ void __launch_bounds__(256) k_uvbg_deposit(int dim, const unsigned *__restrict__ start, const unsigned *__restrict__ idx,
                                                      const double *__restrict__ pos, const float *__restrict__ mass, const uint8_t *__restrict__ type,
                                                      const double *__restrict__ sfr, const double *__restrict__ escfrac, double cellsize,
                                                      int use_sfr, double *__restrict__ g_mass, double *__restrict__ g_star, double *__restrict__ g_sfr)
{
    const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if(c >= (int64_t)dim * dim * dim)
        return;
    const int z = (int)(c % dim), y = (int)((c / dim) % dim), x = (int)(c / ((int64_t)dim * dim));
    double a_mass = 0, a_star = 0, a_sfr = 0;
    for(int cc = 0; cc < 8; cc++) {
        // the base cell whose corner cc this cell is (bit 0 -> x, bit 1 -> y, bit 2 -> z)
        const int base[3] = {wrap(x - (cc & 1), dim), wrap(y - ((cc >> 1) & 1), dim), wrap(z - ((cc >> 2) & 1), dim)};
        const size_t b = cic_index(0, base, dim);
        for(unsigned j = start[b]; j < start[b + 1]; j++) {
            const int64_t i = idx[j];
            double res[3];
#pragma unroll
            for(int k = 0; k < 3; k++)
                (void)cic_axis(pos[3 * i + k], cellsize, res[k]);
            const double w = cic_weight(cc, res, 1.0);
            const double m = (double)mass[i];
            const int ty = type ? type[i] : 1;
            a_mass += w * m;
            if(ty == 4)
                a_star += w * m * escfrac[i];
            else if(ty == 0 && use_sfr)
                a_sfr += w * sfr[i] * escfrac[i];
        }
    }
    g_mass[c] = a_mass;
    g_star[c] = a_star;
    g_sfr[c] = a_sfr;
}

// divide_by_ncell (uvbg.c:208-212) on all spectra at once: a division, as there
__global__ void __launch_bounds__(256) k_uvbg_divide(int64_t count, double2 *__restrict__ v, double ncell)
{
    for(int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < count; i += (int64_t)gridDim.x * blockDim.x) {
        double2 x = v[i];
        x.x /= ncell;
        x.y /= ncell;
        v[i] = x;
    }
}

// filter_pm (uvbg.c:215-248) through pm_apply_transfer_function (petapm.c:1092-1132) on the B spectra of one radius: W(kR) once per mode.
// kfac1 = 2 pi / Nmesh and kfac2 = Nmesh / BoxSize stay two factors (k_mag = sqrt(k2) kfac1 kfac2, uvbg.c:218).  The real-space top hat is
// evaluated in fp64 (the reference: sinf / cosf / powf of the double kR); the k-space top hat's cut is the reference's fp64 comparison.
template <int FT>
__global__ void __launch_bounds__(256) k_uvbg_filter(int dim, int nz, int B, size_t ncplx, double kfac1, double kfac2, double R,
                                                     const double2 *__restrict__ unf, double2 *__restrict__ filt)
{
    const int64_t total = (int64_t)ncplx;
    for(int64_t ip = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; ip < total; ip += (int64_t)gridDim.x * blockDim.x) {
        const int iz = (int)(ip % nz);
        const int64_t r = ip / nz;
        const int iy = (int)(r % dim), ix = (int)(r / dim);
        const int64_t kx = ix <= dim / 2 ? ix : ix - dim, ky = iy <= dim / 2 ? iy : iy - dim, kz = iz; // petapm_mesh_to_k (iz <= dim / 2)
        const int64_t k2 = kx * kx + ky * ky + kz * kz;
        const double k_mag = sqrt((double)k2) * kfac1 * kfac2;
        double kR = k_mag * R;
        double W = 1.0;
        if(FT == 0) {
            if(kR > 1e-4) {
                double s, c;
                sincos(kR, &s, &c);
                W = 3.0 * (s / (kR * kR * kR) - c / (kR * kR));
            }
        }
        else if(FT == 1) {
            kR *= 0.413566994;
            if(kR > 1)
                W = 0.0;
        }
        else {
            kR *= 0.643;
            W = exp(-kR * kR / 2.0);
        }
        for(int b = 0; b < B; b++) {
            double2 v = unf[(size_t)b * ncplx + ip];
            if(FT == 1) { // value = 0.0, not value *= 0: a NaN or an infinity does not survive the cut
                if(W == 0.0)
                    v.x = v.y = 0.0;
            }
            else {
                v.x *= W;
                v.y *= W;
            }
            filt[(size_t)b * ncplx + ip] = v;
        }
    }
}

// reion_loop_pm (uvbg.c:319-455) for the cells of one radius.  LAST: the partial ionisation of the cells that never crossed the barrier and
// the three sums of uvbg.c:428-441 - xHI, xHI delta, delta - as block partials in a fixed order (every thread its cells in increasing
// order, the lanes of a wave by a shuffle tree, the four waves in order), so that equal input gives equal sums.
template <bool LAST>
__global__ void __launch_bounds__(256) k_uvbg_cells(int64_t ncell, UvbgCellPar P, const double *__restrict__ g_mass, const double *__restrict__ g_star,
                                                    const double *__restrict__ g_sfr, float *__restrict__ J21, float *__restrict__ xHI,
                                                    double *__restrict__ partial)
{
    double a0 = 0, a1 = 0, a2 = 0;
    for(int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < ncell; i += (int64_t)gridDim.x * blockDim.x) {
        const double m = fmax(g_mass[i], 0.0), s = fmax(g_star[i], 0.0); // the sanity checks for aliasing, uvbg.c:355-364
        const double density_over_mean = m * P.deltax_conv;
        const double f_coll_stars = s / (P.rtom * density_over_mean) * (4.0 / 3.0) * M_PI * P.R * P.R * P.R / P.pixel_volume;
        double sfr_density;
        if(P.use_sfr)
            sfr_density = fmax(g_sfr[i], 0.0) / P.pixel_volume / P.sfr_unit_m * P.sfr_unit_t;
        else
            sfr_density = s / P.sfr_time / P.pixel_volume;
        const float J21_aux = (float)(sfr_density * P.J21c);
        float x = xHI[i];
        if(f_coll_stars > P.inv_eff) { // (an infinity ionises, a NaN does not)
            if(x > FLOAT_REL_TOL)
                J21[i] = J21_aux; // the first crossing: the largest radius
            x = 0.0f;
            xHI[i] = x;
        }
        else if(LAST && x > FLOAT_REL_TOL) {
            x = (float)(1.0 - f_coll_stars * P.eff);
            xHI[i] = x;
        }
        if(LAST) {
            a0 += (double)x;
            a1 += (double)x * density_over_mean;
            a2 += density_over_mean;
        }
    }
    if(LAST) {
        __shared__ double sh[4][3];
#pragma unroll
        for(int o = 32; o > 0; o >>= 1) {
            a0 += __shfl_down(a0, o);
            a1 += __shfl_down(a1, o);
            a2 += __shfl_down(a2, o);
        }
        if((threadIdx.x & 63) == 0) {
            sh[threadIdx.x >> 6][0] = a0;
            sh[threadIdx.x >> 6][1] = a1;
            sh[threadIdx.x >> 6][2] = a2;
        }
        __syncthreads();
        if(threadIdx.x < 3)
            partial[3 * (size_t)blockIdx.x + threadIdx.x] = ((sh[0][threadIdx.x] + sh[1][threadIdx.x]) + sh[2][threadIdx.x]) + sh[3][threadIdx.x];
    }
}

// ... and the block partials by ONE block: thread t takes the blocks t, t + 256, ... in order, then the same tree
__global__ void __launch_bounds__(256) k_uvbg_sum(int nblocks, const double *__restrict__ partial, double *__restrict__ total)
{
    double a[3] = {0, 0, 0};
    for(int b = threadIdx.x; b < nblocks; b += 256)
        for(int q = 0; q < 3; q++)
            a[q] += partial[3 * (size_t)b + q];
    __shared__ double sh[4][3];
    for(int q = 0; q < 3; q++) {
#pragma unroll
        for(int o = 32; o > 0; o >>= 1)
            a[q] += __shfl_down(a[q], o);
        if((threadIdx.x & 63) == 0)
            sh[threadIdx.x >> 6][q] = a[q];
    }
    __syncthreads();
    if(threadIdx.x < 3)
        total[threadIdx.x] = ((sh[0][threadIdx.x] + sh[1][threadIdx.x]) + sh[2][threadIdx.x]) + sh[3][threadIdx.x];
}

// readout_J21 (uvbg.c:458-469) through pm_iterate_one: the eight corners in the corner order, whatever their weights
__global__ void __launch_bounds__(256) k_uvbg_readout(int64_t n, const double *__restrict__ pos, const uint8_t *__restrict__ type, double cellsize,
                                                      int dim, const float *__restrict__ J21, double *__restrict__ local_J21,
                                                      double *__restrict__ zreion, double znow)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if(i >= n || !type || type[i] != 0)
        return;
    int ic[3];
    double res[3];
    cic_cell3(pos + 3 * i, cellsize, dim, ic, res);
    double lj = local_J21[i], z = zreion[i];
#pragma unroll
    for(int c = 0; c < 8; c++) {
        const double v = (double)J21[cic_index(c, ic, dim)];
        if(v > lj) {
            lj = v;
            if(z == -1)
                z = znow;
        }
    }
    local_J21[i] = lj;
    zreion[i] = z;
}

void UvbgEngine::ensure(int d, int b)
{
    const size_t nreal = (size_t)d * d * d, ncplx = (size_t)d * d * (d / 2 + 1);
    if(d != dim || b != batch) {
        // x slowest, z fastest: rocFFT takes the lengths fastest first; `b` contiguous meshes per execution
        const size_t len3[3] = {(size_t)d, (size_t)d, (size_t)d};
        plan_r2c.create(rocfft_placement_notinplace, rocfft_transform_type_real_forward, 3, len3, (size_t)b);
        plan_c2r.create(rocfft_placement_notinplace, rocfft_transform_type_real_inverse, 3, len3, (size_t)b);
        dim = d;
        batch = b;
    }
    dep.reserve(3 * nreal);
    real.reserve((size_t)b * nreal);
    unf.reserve((size_t)b * 2 * ncplx);
    filt.reserve((size_t)b * 2 * ncplx);
    J21.reserve(nreal);
    xHI.reserve(nreal);
    partial.reserve(3 * (size_t)SUM_BLOCKS + 3);
    err.reserve(4);
}

std::vector<double> UvbgEngine::radii(double R_max, double R_min, double R_delta, double box, int d)
{
    // petapm_reion_c2r, petapm.c:426-499, in its own operations; the last entry is the unfiltered step at the cell size
    const double CellSize = box / d; // petapm.c:112
    std::vector<double> out;
    double R = fmin(R_max, box);
    int last_step = 0, f_count = 0;
    while(!last_step) {
        f_count++;
        if(R / R_delta < R_min || R / R_delta < CellSize || f_count > MAX_R_ITERATIONS) {
            last_step = 1;
            R = CellSize;
        }
        out.push_back(R);
        R = R / R_delta;
    }
    return out;
}

static double rtom(int filter, double R, double OmegaM, double RhoCrit)
{
    // RtoM, uvbg.c:155-173
    if(filter == 0)
        return (4.0 / 3.0) * M_PI * pow(R, 3) * (OmegaM * RhoCrit);
    return pow(2 * M_PI, 1.5) * OmegaM * RhoCrit * pow(R, 3);
}

bool UvbgEngine::run(int64_t n, const double *pos, const float *mass, const uint8_t *type, double box, const mpg_uvbg_params &par,
                     const mpg_uvbg_columns &cols, const std::vector<double> &R, double xhi[2], hipStream_t st)
{
    const int d = par.UVBGdim, use_sfr = par.ReionUseParticleSFR ? 1 : 0, B = use_sfr ? 3 : 2;
    ensure(d, B);
    const size_t nreal = (size_t)d * d * d, ncplx = (size_t)d * d * (d / 2 + 1);
    const double cellsize = box / d;
    const unsigned sgrid = (unsigned)std::min<int64_t>(SUM_BLOCKS, nblk((int64_t)nreal));
    MPG_HIP(hipMemsetAsync(err.p, 0, sizeof(unsigned), st));
    MPG_HIP(hipMemsetAsync(dep.p, 0, 3 * nreal * sizeof(double), st));
    // J21 = 0, xHI = 1 (uvbg.c:566-569)
    MPG_HIP(hipMemsetAsync(J21.p, 0, nreal * sizeof(float), st));
    MPG_HIP(hipMemsetD32Async((hipDeviceptr_t)xHI.p, 0x3f800000, nreal, st));
    if(n > 0) {
        const double fesc_unit_conv = par.UnitMass_in_g / SOLAR_MASS / 1e10 / par.HubbleParam; // uvbg.c:473
        hipLaunchKernelGGL(k_uvbg_init, dim3(nblk(n)), dim3(256), 0, st, n, type, cols.escfrac, cols.local_J21, use_sfr, par.EscapeFractionNorm,
                           fesc_unit_conv, par.EscapeFractionScaling, err.p);
        key_a.reserve((size_t)n);
        key_b.reserve((size_t)n);
        idx_a.reserve((size_t)n);
        idx_b.reserve((size_t)n);
        cell_start.reserve(nreal + 1);
        hipLaunchKernelGGL(k_uvbg_keys, dim3(nblk(n)), dim3(256), 0, st, n, pos, type, cellsize, d, key_a.p, idx_a.p);
        size_t bytes = 0;
        MPG_HIP(rocprim::radix_sort_pairs(nullptr, bytes, key_a.p, key_b.p, idx_a.p, idx_b.p, (size_t)n, 0, 32, st));
        sort_tmp.reserve(bytes + 16);
        MPG_HIP(rocprim::radix_sort_pairs((void *)sort_tmp.p, bytes, key_a.p, key_b.p, idx_a.p, idx_b.p, (size_t)n, 0, 32, st));
        hipLaunchKernelGGL(k_uvbg_cell_start, dim3(nblk((int64_t)nreal + 1)), dim3(256), 0, st, (int64_t)nreal, n, (const unsigned *)key_b.p, cell_start.p);
        hipLaunchKernelGGL(k_uvbg_deposit, dim3(nblk((int64_t)nreal)), dim3(256), 0, st, d, (const unsigned *)cell_start.p, (const unsigned *)idx_b.p, pos,
                           mass, type, (const double *)cols.sfr, (const double *)cols.escfrac, cellsize, use_sfr, dep.p, dep.p + nreal,
                           dep.p + 2 * nreal);
    }
    // (the deposited grids are kept for mpg_dev_uvbg_grids: the transform reads a copy)
    MPG_HIP(hipMemcpyAsync(real.p, dep.p, (size_t)B * nreal * sizeof(double), hipMemcpyDeviceToDevice, st));
    plan_r2c.exec(real.p, unf.p, st);
    const int64_t nmodes = (int64_t)B * (int64_t)ncplx;
    hipLaunchKernelGGL(k_uvbg_divide, dim3((unsigned)std::min<int64_t>(2048, nblk(nmodes))), dim3(256), 0, st, nmodes, (double2 *)unf.p,
                       (double)d * (double)d * (double)d);

    // the constants of reion_loop_pm that do not depend on the radius (uvbg.c:330-371)
    const double redshift = 1.0 / par.Time - 1.;
    const double Y_He = 1.0 - HYDROGEN_MASSFRAC;
    const double BaryonFrac = par.OmegaBaryon / par.Omega0;
    const double ReionEfficiency = 1.0 / BaryonFrac * par.ReionNionPhotPerBary / (1.0 - 0.75 * Y_He);
    const double tot_n_cells = (double)d * (double)d * (double)d;
    UvbgCellPar C{};
    C.pixel_volume = cellsize * cellsize * cellsize;
    C.deltax_conv = tot_n_cells / (par.RhoCrit * par.Omega0 * box * box * box);
    C.eff = ReionEfficiency;
    C.inv_eff = 1.0 / ReionEfficiency;
    C.sfr_unit_m = par.UnitMass_in_g / SOLAR_MASS;
    C.sfr_unit_t = par.UnitTime_in_s / SEC_PER_YEAR;
    const double hubble_time = 1 / (par.hubble * par.HubbleParam);
    C.sfr_time = par.ReionSFRTimescale * hubble_time;
    C.use_sfr = use_sfr;
    const double kfac1 = 2 * M_PI / d, kfac2 = d / box;
    const unsigned fgrid = (unsigned)std::min<int64_t>(2048, nblk((int64_t)ncplx));
    for(size_t r = 0; r < R.size(); r++) {
        const bool last = r + 1 == R.size();
        C.R = R[r];
        C.rtom = rtom(par.RtoMFilterType, C.R, par.Omega0, par.RhoCrit);
        C.J21c = (1.0 + redshift) * (1.0 + redshift) / (4.0 * M_PI) * par.AlphaUV * PLANCK * 1e21 * C.R * par.UnitLength_in_cm *
                 par.ReionNionPhotPerBary / PROTONMASS * par.UnitMass_in_g / pow(par.UnitLength_in_cm, 3) / par.UnitTime_in_s;
        if(last) // the last step is unfiltered: the transfer is a copy (petapm.c:462)
            MPG_HIP(hipMemcpyAsync(filt.p, unf.p, (size_t)B * 2 * ncplx * sizeof(double), hipMemcpyDeviceToDevice, st));
        else {
            auto k = par.ReionFilterType == 0 ? k_uvbg_filter<0> : par.ReionFilterType == 1 ? k_uvbg_filter<1> : k_uvbg_filter<2>;
            hipLaunchKernelGGL(k, dim3(fgrid), dim3(256), 0, st, d, d / 2 + 1, B, ncplx, kfac1, kfac2, C.R, (const double2 *)unf.p, (double2 *)filt.p);
        }
        plan_c2r.exec(filt.p, real.p, st);
        const double *gm = real.p, *gs = real.p + nreal, *gf = use_sfr ? real.p + 2 * nreal : nullptr;
        if(last)
            hipLaunchKernelGGL(k_uvbg_cells<true>, dim3(sgrid), dim3(256), 0, st, (int64_t)nreal, C, gm, gs, gf, J21.p, xHI.p, partial.p);
        else
            hipLaunchKernelGGL(k_uvbg_cells<false>, dim3(sgrid), dim3(256), 0, st, (int64_t)nreal, C, gm, gs, gf, J21.p, xHI.p, partial.p);
    }
    hipLaunchKernelGGL(k_uvbg_sum, dim3(1), dim3(256), 0, st, (int)sgrid, (const double *)partial.p, partial.p + 3 * (size_t)SUM_BLOCKS);
    if(n > 0)
        hipLaunchKernelGGL(k_uvbg_readout, dim3(nblk(n)), dim3(256), 0, st, n, pos, type, cellsize, d, (const float *)J21.p, cols.local_J21, cols.zreion,
                           1 / par.Time - 1);
    MPG_HIP(hipGetLastError());
    double tot[3];
    unsigned e = 0;
    MPG_HIP(hipMemcpyAsync(tot, partial.p + 3 * (size_t)SUM_BLOCKS, sizeof(tot), hipMemcpyDeviceToHost, st));
    MPG_HIP(hipMemcpyAsync(&e, err.p, sizeof(e), hipMemcpyDeviceToHost, st));
    MPG_HIP(hipStreamSynchronize(st));
    const int grid_n_real = d * d * d; // uvbg.c:427, :447-448
    xhi[0] = tot[0] / grid_n_real;
    xhi[1] = tot[1] / tot[2];
    return e == 0;
}

} // namespace mpg

// ---- C-ABI (include/mpgadget_hip.h) ----
static std::vector<double> uvbg_check(const mpg_engine *eng, const mpg_uvbg_params *par, const mpg_uvbg_columns *cols)
{
    MPG_CHECK(par->NTask <= 1, "calculate_uvbg: NTask > 1 is not carried; several ranks keep the CPU function");
    MPG_CHECK(par->ReionFilterType >= 0 && par->ReionFilterType <= 2, "calculate_uvbg: ReionFilterType " + std::to_string(par->ReionFilterType) + " is undefined");
    MPG_CHECK(par->RtoMFilterType == 0 || par->RtoMFilterType == 1, "calculate_uvbg: unrecognised RtoMFilterType " + std::to_string(par->RtoMFilterType));
    MPG_CHECK(par->ReionDeltaRFactor > 1, "calculate_uvbg: ReionDeltaRFactor must be larger than 1 (the radii would never shrink)");
    MPG_CHECK(par->ReionRBubbleMax > 0, "calculate_uvbg: ReionRBubbleMax must be positive");
    MPG_CHECK(par->ReionRBubbleMin > 0, "calculate_uvbg: ReionRBubbleMin must be positive");
    MPG_CHECK(par->UVBGdim >= 4, "calculate_uvbg: UVBGdim must be at least 4");
    MPG_CHECK(par->UVBGdim <= mpg::uvbg::MAX_DIM, "calculate_uvbg: UVBGdim above 1290 is refused (the reference's int cell count overflows)");
    MPG_CHECK(!par->ReionUseParticleSFR || eng->n == 0 || cols->sfr, "calculate_uvbg: ReionUseParticleSFR needs the sfr column");
    MPG_CHECK(eng->n == 0 || (cols->escfrac && cols->local_J21 && cols->zreion), "calculate_uvbg: the columns escfrac, local_J21 and zreion are required");
    MPG_CHECK(eng->n < ((int64_t)1 << 31), "calculate_uvbg: more than 2^31 - 1 rows");
    MPG_CHECK(par->Time > 0 && eng->box > 0, "calculate_uvbg: Time and the box of the bound particles must be positive");
    return UvbgEngine::radii(par->ReionRBubbleMax, par->ReionRBubbleMin, par->ReionDeltaRFactor, eng->box, par->UVBGdim);
}

int mpg_dev_calculate_uvbg(mpg_engine *eng, const mpg_uvbg_params *par, const mpg_uvbg_columns *cols, mpg_uvbg_result *result)
{
    API_BEGIN
    MPG_CHECK(eng && par && cols && result, "calculate_uvbg: null argument");
    MPG_CHECK(eng->d_pos || eng->n == 0, "calculate_uvbg: no particles bound (mpg_dev_bind_particles)");
    const std::vector<double> R = uvbg_check(eng, par, cols);
    MPG_HIP(hipSetDevice(eng->device));
    double xhi[2];
    const bool ok = eng->uvbg.run(eng->n, eng->d_pos, eng->d_mass, eng->d_type, eng->box, *par, *cols, R, xhi, eng->stream);
    result->volume_weighted_global_xHI = xhi[0];
    result->mass_weighted_global_xHI = xhi[1];
    result->nradii = (int64_t)R.size();
    for(int64_t k = 0; result->radii && k < result->radii_cap && k < (int64_t)R.size(); k++)
        result->radii[k] = R[(size_t)k];
    MPG_CHECK(ok, "calculate_uvbg: negative escape fraction (EscapeFractionNorm)");
    API_END
}

int mpg_dev_uvbg_grids(mpg_engine *eng, int dim, float *d_J21, float *d_xHI, double *d_deposit)
{
    API_BEGIN
    MPG_CHECK(eng, "uvbg_grids: null argument");
    MPG_CHECK(eng->uvbg.dim > 0 && eng->uvbg.J21.p, "uvbg_grids: no mpg_dev_calculate_uvbg on this engine yet");
    MPG_CHECK(dim == eng->uvbg.dim, "uvbg_grids: dim differs from the UVBGdim of the last mpg_dev_calculate_uvbg");
    MPG_HIP(hipSetDevice(eng->device));
    const size_t nreal = (size_t)dim * dim * dim;
    if(d_J21)
        MPG_HIP(hipMemcpyAsync(d_J21, eng->uvbg.J21.p, nreal * sizeof(float), hipMemcpyDeviceToDevice, eng->stream));
    if(d_xHI)
        MPG_HIP(hipMemcpyAsync(d_xHI, eng->uvbg.xHI.p, nreal * sizeof(float), hipMemcpyDeviceToDevice, eng->stream));
    if(d_deposit)
        MPG_HIP(hipMemcpyAsync(d_deposit, eng->uvbg.dep.p, 3 * nreal * sizeof(double), hipMemcpyDeviceToDevice, eng->stream));
    API_END
}
