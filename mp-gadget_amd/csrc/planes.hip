// planes.hip -- lensing potential planes (write_plane, libgadget/plane.c:572-683) on the bound device particles.
//
// The particle plane is cutPlaneGaussianGrid (lenstools.c:233-319): nearest-grid-point COUNTS of the active particles of a slab on an
// R x R image (grid3d_ngb / find_bin, lenstools.c:68-124; the image axes are projectDensity's, lenstools.c:126-166), normalised to the
// density contrast and turned into the lensing potential by a 2-D Poisson solve (calculate_lensing_potential, lenstools.c:168-231).
//
//   k_plane_count   ONE pass over the particles for every plane of a call (each cut point x each normal): Pos, Type and the flags are read
//                   once, the pixel index along each axis is made once, and the particle is counted into every slab that holds it (slabs may
//                   overlap) with no-return 32-bit integer atomics.  The reference counts particles, not mass, so the counters are exact and do
//                   not depend on the order of the adds.  The active particles (lenstools_particle_is_active, lenstools.c:18-26;
//                   plane_count_active_particles, plane.c:76-87) are counted in the same pass.
//   k_plane_sums    num_particles_plane (lenstools.c:296) of every plane
//   k_plane_density counters -> double times density_norm_factor (lenstools.c:292-298)
//   k_plane_transfer  zero the DC mode, -2 (b0 b1 / chi^2) / (4 pi^2 l^2) exp(-(2 pi smooth)^2 l^2 / 2) (lenstools.c:184-211)
//   k_plane_scale   / R^2, times cosmo_normalization density_normalization (lenstools.c:217-221, 306-310)
//
// The bin index repeats the reference's arithmetic operation for operation: the wrap of lenstools.c:106-110 (note its asymmetry: a
// coordinate of exactly 0 becomes Box, one of exactly Box stays), find_bin's own wrap into [0, L), the rejection rel >= width and
// floor(rel / width * resolution).  bins[0] and bins[resolution] - bins[0] come from the host (linspace in its order of operations); what
// is left for the device is a subtraction, a division and a multiplication, none of which the compiler can contract into a fused
// multiply-add.  That is what makes the counters comparable for equality with a CPU restatement.
//
// Rows with IsGarbage are skipped here as in every other loop of the engine.  The reference does not test the bit in these loops because
// write_plane runs at a sync point, after the table has been collected (run.c:727).
#include "engine_internal.h"
#include "planes.h"

namespace mpg {

namespace {

struct PlaneKArgs {
    int R, ncuts, nnormals, tracer;
    int normals[3];
    double box;
    double offset[3], img_b0[3], img_w[3];
    long long p0, p1;
};

// lenstools.c:106-110; false for a coordinate the two loops could not bring home in a bounded number of turns (the reference would spin)
__device__ inline bool plane_wrap(double &p, const double box)
{
    if(!(fabs(p) <= 1024. * box))
        return false;
    while(p > box)
        p -= box;
    while(p <= 0)
        p += box;
    return true;
}

// find_bin, lenstools.c:68-95, with bins[0] and width = bins[resolution] - bins[0] handed in (|b0| <= 1024 L is checked on the host)
__device__ inline int plane_find_bin(const double value, const double b0, const double width, const int resolution, const double L)
{
    double rel = value - b0;
    while(rel < 0)
        rel += L;
    while(rel >= L)
        rel -= L;
    if(rel >= width)
        return -1;
    const double iflt = rel / width * resolution;
    const int index = (int)floor(iflt);
    return (index >= 0 && index < resolution) ? index : -1;
}

__global__ __launch_bounds__(256) void k_plane_count(const long long n, const double *__restrict__ pos, const uint8_t *__restrict__ type,
                                                     const uint8_t *__restrict__ flags, const PlaneKArgs A, const double *__restrict__ slabs,
                                                     unsigned *__restrict__ counts, unsigned long long *__restrict__ sums)
{
    extern __shared__ double s_slab[]; // per cut: bins[0], width along the normal
    for(int i = threadIdx.x; i < 2 * A.ncuts; i += blockDim.x)
        s_slab[i] = slabs[i];
    __syncthreads();
    const size_t R2 = (size_t)A.R * A.R;
    unsigned long long nact = 0, nbad = 0;
    for(long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        const unsigned fl = flags ? flags[i] : 0u;
        const unsigned ty = type ? type[i] : 1u;
        // IsGarbage, Swallowed (partmanager.h:17-21), the engine's own "no longer a particle" type, the hybrid-neutrino tracers
        if((fl & 3u) || ty == 7u || (A.tracer && ty == 2u))
            continue;
        nact++;
        int bin[3];
        double p[3];
        bool ok = true;
        for(int d = 0; d < 3; d++) {
            p[d] = pos[3 * i + d] - A.offset[d];
            ok = plane_wrap(p[d], A.box) && ok;
        }
        if(!ok) {
            nbad++;
            continue;
        }
        for(int d = 0; d < 3; d++)
            bin[d] = plane_find_bin(p[d], A.img_b0[d], A.img_w[d], A.R, A.box);
        for(int s = 0; s < A.nnormals; s++) {
            const int nrm = A.normals[s];
            // projectDensity, lenstools.c:126-166: normal 0 -> (y, z), 1 -> (x, z), 2 -> (x, y), the first one is the row
            const int r = nrm == 0 ? bin[1] : bin[0], c = nrm == 2 ? bin[1] : bin[2];
            if(r < 0 || c < 0)
                continue;
            const size_t pix = (size_t)r * A.R + c;
            for(int k = 0; k < A.ncuts; k++) {
                const long long plane = (long long)k * A.nnormals + s;
                if(plane < A.p0 || plane >= A.p1)
                    continue;
                if(plane_find_bin(p[nrm], s_slab[2 * k], s_slab[2 * k + 1], 1, A.box) < 0)
                    continue;
                atomicAdd(&counts[(size_t)(plane - A.p0) * R2 + pix], 1u);
            }
        }
    }
    // one 64-bit add per wave
    for(int o = warpSize / 2; o > 0; o >>= 1) {
        nact += __shfl_down(nact, o);
        nbad += __shfl_down(nbad, o);
    }
    if((threadIdx.x & (warpSize - 1)) == 0) {
        if(nact)
            atomicAdd(&sums[0], nact);
        if(nbad)
            atomicAdd(&sums[1], nbad);
    }
}

__global__ __launch_bounds__(256) void k_plane_sums(const size_t R2, const unsigned *__restrict__ counts, unsigned long long *__restrict__ sums)
{
    const unsigned *c = counts + (size_t)blockIdx.y * R2;
    unsigned long long s = 0;
    for(size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < R2; i += (size_t)gridDim.x * blockDim.x)
        s += c[i];
    for(int o = warpSize / 2; o > 0; o >>= 1)
        s += __shfl_down(s, o);
    if((threadIdx.x & (warpSize - 1)) == 0 && s)
        atomicAdd(&sums[blockIdx.y], s);
}

__global__ __launch_bounds__(256) void k_plane_widen(const size_t m, const unsigned *__restrict__ in, unsigned long long *__restrict__ out)
{
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if(i < m)
        out[i] = in[i];
}

template <typename T> __global__ __launch_bounds__(256) void k_plane_density(const size_t R2, const T *__restrict__ counts, const double f, double *__restrict__ out)
{
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if(i < R2)
        out[i] = (double)counts[i] * f;
}

// rows i = 0 .. R-1 (lx), columns j = 0 .. R/2 (ly) of the Hermitian half, lenstools.c:184-211 with smooth = 1
__global__ __launch_bounds__(256) void k_plane_transfer(const int R, const double pref, double *__restrict__ cplx)
{
    const int nc = R / 2 + 1;
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if(idx >= (size_t)R * nc)
        return;
    const int i = (int)(idx / nc), j = (int)(idx % nc);
    if(idx == 0) {
        cplx[0] = 0;
        cplx[1] = 0;
        return;
    }
    double lx = i < R / 2 ? i : -(R - i);
    lx /= R;
    double ly = j;
    ly /= R;
    const double l2 = lx * lx + ly * ly;
    const double smooth = 1.0;
    const double factor = pref / (l2 * 4 * M_PI * M_PI);
    const double f = factor * exp(-0.5 * ((2.0 * M_PI * smooth) * (2.0 * M_PI * smooth)) * l2);
    cplx[2 * idx] *= f;
    cplx[2 * idx + 1] *= f;
}

__global__ __launch_bounds__(256) void k_plane_scale(const size_t R2, const double r2, const double post, double *__restrict__ plane)
{
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if(i < R2)
        plane[i] = plane[i] / r2 * post;
}

// ---- the massive-neutrino correction (plane.c:313-478) ---------------------------------------------------------------------------------
// the activity mask of the mass deposit and, when the table carries an offset, the positions plane_pm_particle_cic deposits
// (plane.c:98-110: Pos - CurrentParticleOffset wrapped into [0, L))
__global__ __launch_bounds__(256) void k_plane_active(const long long n, const uint8_t *__restrict__ type, const uint8_t *__restrict__ flags,
                                                      const int tracer, const double *__restrict__ pos, const double3 off, const double box,
                                                      uint8_t *__restrict__ active, double *__restrict__ shifted)
{
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if(i >= n)
        return;
    const unsigned fl = flags ? flags[i] : 0u;
    const unsigned ty = type ? type[i] : 1u;
    bool on = !((fl & 3u) || ty == 7u || (tracer && ty == 2u));
    if(shifted) {
        const double o[3] = {off.x, off.y, off.z};
        for(int d = 0; d < 3; d++) {
            double x = pos[3 * i + d] - o[d];
            if(!(fabs(x) <= 1024. * box)) { // (the counting pass has refused such a row already)
                on = false;
                x = 0;
            }
            while(x < 0)
                x += box;
            while(x >= box)
                x -= box;
            shifted[3 * i + d] = x;
        }
    }
    active[i] = on;
}

// cutPlanePMNeutrinoCorrection's projection, plane.c:402-428: the image axes are plane_directions[] = (normal + 1) % 3, (normal + 2) % 3 -
// for normal 1 that is (z, x), the TRANSPOSE of the particle plane's (x, z); restated as the reference has it.  One thread per pixel,
// the cells along the normal in index order; overlap[k] is plane_periodic_slab_overlap of cell k.
__global__ __launch_bounds__(256) void k_plane_project(const int N, const int normal, const double *__restrict__ real,
                                                       const double *__restrict__ overlap, const double inv_fft_norm, const double mean_mass_cell,
                                                       const double thickness, double *__restrict__ out)
{
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if(idx >= (size_t)N * N)
        return;
    const int pix0 = (int)(idx / N), pix1 = (int)(idx % N);
    const size_t st[3] = {(size_t)N * N, (size_t)N, 1}; // x slowest, z fastest
    const int d0 = (normal + 1) % 3, d1 = (normal + 2) % 3;
    const size_t base = pix0 * st[d0] + pix1 * st[d1];
    double sum = 0;
    for(int k = 0; k < N; k++) {
        const double ov = overlap[k];
        if(ov <= 0)
            continue;
        const double delta_nu_scaled = real[base + k * st[normal]] * inv_fft_norm / mean_mass_cell;
        sum += delta_nu_scaled * ov / thickness;
    }
    out[idx] = sum;
}

// plane_add_periodic_bilinear, plane.c:447-478
__global__ __launch_bounds__(256) void k_plane_bilinear_add(const int dst_n, const int src_n, const double *__restrict__ src, double *__restrict__ dst)
{
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if(idx >= (size_t)dst_n * dst_n)
        return;
    const int i = (int)(idx / dst_n), j = (int)(idx % dst_n);
    const double x = ((i + 0.5) * src_n / dst_n) - 0.5;
    int i0 = (int)floor(x);
    const double tx = x - i0;
    while(i0 < 0)
        i0 += src_n;
    while(i0 >= src_n)
        i0 -= src_n;
    const int i1 = (i0 + 1) % src_n;
    const double y = ((j + 0.5) * src_n / dst_n) - 0.5;
    int j0 = (int)floor(y);
    const double ty = y - j0;
    while(j0 < 0)
        j0 += src_n;
    while(j0 >= src_n)
        j0 -= src_n;
    const int j1 = (j0 + 1) % src_n;
    const double v00 = src[(size_t)i0 * src_n + j0], v10 = src[(size_t)i1 * src_n + j0];
    const double v01 = src[(size_t)i0 * src_n + j1], v11 = src[(size_t)i1 * src_n + j1];
    dst[idx] += (1 - tx) * (1 - ty) * v00 + tx * (1 - ty) * v10 + (1 - tx) * ty * v01 + tx * ty * v11;
}

inline unsigned blocks_for(size_t m) { return (unsigned)((m + 255) / 256); }

} // namespace

void PlaneEngine::Solver::ensure(int R_)
{
    if(R == R_ && r2c.ready())
        return;
    const size_t len2[2] = {(size_t)R_, (size_t)R_};
    r2c.create(rocfft_placement_notinplace, rocfft_transform_type_real_forward, 2, len2, 1);
    c2r.create(rocfft_placement_notinplace, rocfft_transform_type_real_inverse, 2, len2, 1);
    cplx.reserve(2 * (size_t)R_ * (R_ / 2 + 1));
    R = R_;
}

// calculate_lensing_potential (lenstools.c:168-231) on the density in d_plane[R][R], then times `post`
void PlaneEngine::Solver::run(int R_, double b, double chi, double post, double *d_plane, hipStream_t st)
{
    const size_t R2 = (size_t)R_ * R_;
    ensure(R_);
    r2c.exec(d_plane, cplx.p, st);
    const double pref = -2.0 * (b * b / (chi * chi));
    hipLaunchKernelGGL(k_plane_transfer, dim3(blocks_for((size_t)R_ * (R_ / 2 + 1))), dim3(256), 0, st, R_, pref, cplx.p);
    c2r.exec(cplx.p, d_plane, st);
    hipLaunchKernelGGL(k_plane_scale, dim3(blocks_for(R2)), dim3(256), 0, st, R2, (double)R_ * (double)R_, post, d_plane);
    MPG_HIP(hipGetLastError());
}

void PlaneEngine::count(const PlaneSetup &S, int64_t n, const double *d_pos, const uint8_t *d_type, const uint8_t *d_flags, int64_t p0, int64_t p1,
                        unsigned *d_counts, hipStream_t st)
{
    const size_t R2 = (size_t)S.R * S.R;
    const int64_t nb = p1 - p0;
    MPG_CHECK(nb > 0 && p0 >= 0 && p1 <= S.nplanes(), "potential planes: bad plane range");
    sums.reserve(2 + (size_t)S.nplanes());
    slabs.reserve(2 * (size_t)S.ncuts);
    MPG_HIP(hipMemcpyAsync(slabs.p, S.slab.data(), 2 * (size_t)S.ncuts * sizeof(double), hipMemcpyHostToDevice, st));
    MPG_HIP(hipMemsetAsync(d_counts, 0, (size_t)nb * R2 * sizeof(unsigned), st));
    MPG_HIP(hipMemsetAsync(sums.p, 0, 2 * sizeof(unsigned long long), st));
    MPG_HIP(hipMemsetAsync(sums.p + 2 + p0, 0, (size_t)nb * sizeof(unsigned long long), st));
    PlaneKArgs A;
    A.R = S.R;
    A.ncuts = S.ncuts;
    A.nnormals = S.nnormals;
    A.tracer = S.tracer;
    A.box = S.box;
    for(int d = 0; d < 3; d++) {
        A.normals[d] = S.normals[d];
        A.offset[d] = S.offset[d];
        A.img_b0[d] = S.img_b0[d];
        A.img_w[d] = S.img_w[d];
    }
    A.p0 = p0;
    A.p1 = p1;
    if(n > 0) {
        // a grid-stride loop: enough blocks to fill the device, few enough that the per-wave sums are a few thousand adds on one address
        const unsigned blocks = (unsigned)std::min<int64_t>((n + 255) / 256, 4096);
        hipLaunchKernelGGL(k_plane_count, dim3(blocks), dim3(256), 2 * (size_t)S.ncuts * sizeof(double), st, (long long)n, d_pos, d_type, d_flags, A,
                           slabs.p, d_counts, sums.p);
        MPG_HIP(hipGetLastError());
    }
    const unsigned bx = (unsigned)std::min<size_t>((R2 + 255) / 256, 1024);
    hipLaunchKernelGGL(k_plane_sums, dim3(bx, (unsigned)nb), dim3(256), 0, st, R2, d_counts, sums.p + 2 + p0);
    MPG_HIP(hipGetLastError());
}

void PlaneEngine::solve(const PlaneSetup &S, const void *d_counts, bool wide64, double f, double b, double chi, double post, double *d_plane,
                        hipStream_t st)
{
    const int R = S.R;
    const size_t R2 = (size_t)R * R;
    if(R == 1) { // the only mode is the uniform one, which is dropped (lenstools.c:200-201)
        MPG_HIP(hipMemsetAsync(d_plane, 0, sizeof(double), st));
        return;
    }
    if(wide64)
        hipLaunchKernelGGL(k_plane_density<unsigned long long>, dim3(blocks_for(R2)), dim3(256), 0, st, R2, (const unsigned long long *)d_counts, f, d_plane);
    else
        hipLaunchKernelGGL(k_plane_density<unsigned>, dim3(blocks_for(R2)), dim3(256), 0, st, R2, (const unsigned *)d_counts, f, d_plane);
    image.run(R, b, chi, post, d_plane, st);
}

// plane_pm_grid_init_neutrino_correction (plane.c:313-351): once per call
void PlaneEngine::correction_init(PMesh &pm, const PlaneSetup &S, int64_t n, const double *d_pos, const float *d_mass, const uint8_t *d_type,
                                  const uint8_t *d_flags, mpg_nu_response_fn fn, void *ctx, double box_mpc, hipStream_t st)
{
    MPG_CHECK(pm.nmesh > 0, "potential planes: the massive-neutrino correction needs the PM mesh (gravpm_init_periodic first)"); // plane.c:620
    MPG_CHECK(pm.box == S.box, "potential planes: BoxSize of the PM mesh differs from the particles'");
    const bool shift = S.offset[0] != 0 || S.offset[1] != 0 || S.offset[2] != 0;
    active.reserve((size_t)n + 1);
    if(shift)
        shifted.reserve(3 * (size_t)n + 1);
    if(n > 0)
        hipLaunchKernelGGL(k_plane_active, dim3(blocks_for((size_t)n)), dim3(256), 0, st, (long long)n, d_type, d_flags, S.tracer, d_pos,
                           make_double3(S.offset[0], S.offset[1], S.offset[2]), S.box, active.p, shift ? shifted.p : nullptr);
    const double total_mass = pm.plane_nu_correction(n, shift ? shifted.p : d_pos, d_mass, active.p, fn, ctx, box_mpc, st);
    const int N = pm.nmesh;
    mean_mass_cell = total_mass / ((double)N * N * N);
    inv_fft_norm = 1.0 / ((double)N * N * N);
    // plane_periodic_slab_overlap (plane.c:369-387) of every cell index, per cut
    const double L = S.box, cellsize = L / N, thickness = S.thickness;
    std::vector<double> ov((size_t)S.ncuts * N);
    for(int c = 0; c < S.ncuts; c++)
        for(int k = 0; k < N; k++) {
            const double cell_start = k * cellsize;
            double o = 0;
            if(thickness >= L)
                o = cellsize;
            else {
                double cc = S.cuts[c];
                while(cc < 0)
                    cc += L;
                while(cc >= L)
                    cc -= L;
                const double slab_start = cc - 0.5 * thickness, slab_end = slab_start + thickness, cell_end = cell_start + cellsize;
                for(int sh = -1; sh <= 1; sh++) {
                    const double off = sh * L;
                    const double a = slab_start + off, b = slab_end + off;
                    const double lo = cell_start > a ? cell_start : a, hi = cell_end < b ? cell_end : b;
                    o += hi > lo ? hi - lo : 0.0;
                }
            }
            ov[(size_t)c * N + k] = o;
        }
    overlap.reserve(ov.size() + 1);
    MPG_HIP(hipMemcpyAsync(overlap.p, ov.data(), ov.size() * sizeof(double), hipMemcpyHostToDevice, st));
    MPG_HIP(hipStreamSynchronize(st));
    corr.reserve((size_t)N * N);
}

// cutPlanePMNeutrinoCorrection + plane_add_periodic_bilinear (plane.c:389-478) for one plane, added to d_plane[R][R]
void PlaneEngine::correction_add(PMesh &pm, const PlaneSetup &S, int cut, int normal, double chi, double post, double *d_plane, hipStream_t st)
{
    const int N = pm.nmesh;
    hipLaunchKernelGGL(k_plane_project, dim3(blocks_for((size_t)N * N)), dim3(256), 0, st, N, normal, (const double *)pm.real.p,
                       (const double *)(overlap.p + (size_t)cut * N), inv_fft_norm, mean_mass_cell, S.thickness, corr.p);
    mesh.run(N, S.box / N, chi, post, corr.p, st);
    hipLaunchKernelGGL(k_plane_bilinear_add, dim3(blocks_for((size_t)S.R * S.R)), dim3(256), 0, st, S.R, N, (const double *)corr.p, d_plane);
    MPG_HIP(hipGetLastError());
}

} // namespace mpg

// ---- the call: parameters resolved as write_plane does (plane.c:579-597), the loop of plane.c:633-634 ---------------------------------------

static void linspace_ends(double start, double stop, int num, double *b0, double *width)
{
    // linspace, lenstools.c:39-44: step = (stop - start) / (num - 1), result[i] = start + i * step; find_bin reads bins[0], bins[num - 1]
    const volatile double step = (stop - start) / (num - 1);
    const volatile double first = start + 0 * step;
    const volatile double last = start + (num - 1) * step;
    *b0 = first;
    *width = last - first;
}

void planes_setup(mpg_engine *eng, const mpg_plane_params *par, PlaneSetup &S)
{
    MPG_CHECK(par, "potential planes: null parameters");
    MPG_CHECK(eng->box > 0, "potential planes: no particles bound");
    S.box = eng->box;
    MPG_CHECK(par->Resolution >= 1, "potential planes: Resolution must be at least 1");
    MPG_CHECK(par->Resolution <= 32768, "potential planes: Resolution above 32768");
    S.R = par->Resolution;
    S.thickness = par->Thickness > 0 ? par->Thickness : S.box; // plane.c:581-584
    MPG_CHECK(par->ncuts >= 0 && par->ncuts <= PLANE_MAXCUTS, "potential planes: more than 1024 cut points (ncuts > 1024)");
    MPG_CHECK(par->ncuts == 0 || par->CutPoints, "potential planes: ncuts > 0 without CutPoints");
    if(par->ncuts == 0) { // plane.c:587-591
        const int64_t nc = (int64_t)(S.box / S.thickness);
        MPG_CHECK(nc <= PLANE_MAXCUTS, "potential planes: more than 1024 cut points (ncuts > 1024) from Box / Thickness");
        for(int64_t i = 0; i < nc; i++)
            S.cuts.push_back((.5 + i) * S.thickness);
    }
    else
        S.cuts.assign(par->CutPoints, par->CutPoints + par->ncuts);
    S.ncuts = (int)S.cuts.size();
    MPG_CHECK(par->nnormals >= 0 && par->nnormals <= 3 && (par->nnormals == 0 || par->Normals), "potential planes: nnormals must be 0 .. 3");
    S.nnormals = par->nnormals;
    for(int j = 0; j < S.nnormals; j++) {
        MPG_CHECK(par->Normals[j] >= 0 && par->Normals[j] <= 2, "potential planes: requesting a normal direction beyond 0, 1 and 2"); // plane.c:527
        S.normals[j] = par->Normals[j];
    }
    MPG_CHECK(par->omega_source > 0, "potential planes: non-positive particle matter density (omega_source <= 0)"); // plane.c:71
    MPG_CHECK(par->atime > 0 && par->comoving_distance > 0 && par->HubbleParam > 0,
              "potential planes: atime, comoving_distance and HubbleParam must be positive");
    const double far = 1024. * S.box;
    for(int d = 0; d < 3; d++) {
        S.offset[d] = par->CurrentParticleOffset[d];
        MPG_CHECK(std::isfinite(S.offset[d]) && std::isfinite(par->left_corner[d]) && fabs(par->left_corner[d]) <= far,
                  "potential planes: CurrentParticleOffset / left_corner not finite or far outside the box");
        linspace_ends(par->left_corner[d], par->left_corner[d] + S.box, S.R + 1, &S.img_b0[d], &S.img_w[d]); // lenstools.c:258-260
    }
    S.slab.resize(2 * (size_t)S.ncuts);
    for(int k = 0; k < S.ncuts; k++) {
        MPG_CHECK(std::isfinite(S.cuts[k]) && fabs(S.cuts[k]) + S.thickness <= far, "potential planes: a cut point is not finite or far outside the box");
        linspace_ends(S.cuts[k] - S.thickness / 2, S.cuts[k] + S.thickness / 2, 2, &S.slab[2 * k], &S.slab[2 * k + 1]);
    }
    S.tracer = eng->pm.hybrid_tracer ? 1 : 0;
}

// The counters of [p0, p1) and the sums of the call so far, read back: sums[0] active rows of this rank, sums[2 + p] particles per plane.
// Returns 0, or the rank-local refusal of the pass: 1 a position the wrap cannot take, 2 too many active rows for 32-bit counters
static int planes_count_batch(mpg_engine *eng, const PlaneSetup &S, const uint8_t *d_flags, int64_t p0, int64_t p1, unsigned *d_counts,
                              std::vector<unsigned long long> &hs)
{
    PlaneEngine &pe = eng->planes;
    pe.count(S, eng->n, eng->d_pos, eng->d_type, d_flags, p0, p1, d_counts, eng->stream);
    hs.resize(2 + (size_t)S.nplanes());
    MPG_HIP(hipMemcpyAsync(hs.data(), pe.sums.p, hs.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost, eng->stream));
    MPG_HIP(hipStreamSynchronize(eng->stream));
    return hs[1] != 0 ? 1 : (hs[0] >= (1ull << 32) ? 2 : 0);
}

static void planes_count_refuse(int err)
{
    MPG_CHECK(err != 1, "potential planes: a particle position is not finite or far outside the box");
    MPG_CHECK(err != 2, "potential planes: 2^32 or more active particles on one rank (32-bit counters)");
    MPG_CHECK(err == 0, "potential planes: the counting pass failed on another rank");
}

void planes_run(mpg_engine *eng, const mpg_plane_params *par, const uint8_t *d_flags, double *d_planes, int64_t *npart, const PlaneReduce *red)
{
    PlaneSetup S;
    planes_setup(eng, par, S);
    const bool many = red && red->nt > 1;
    // the refusal comes before anything collective, so that every rank returns
    MPG_CHECK(!(par->fn && many), "potential planes: the massive-neutrino correction on several ranks is not implemented");
    MPG_CHECK(!par->fn || S.R >= 2, "potential planes: Resolution must be at least 2 for the massive-neutrino correction"); // plane.c:618
    MPG_CHECK(!par->fn || eng->pm.nmesh > 0,
              "potential planes: the massive-neutrino correction needs the PM mesh (gravpm_init_periodic first)"); // plane.c:620
    MPG_CHECK(!S.tracer || eng->d_type || eng->n == 0, "potential planes: the hybrid-neutrino tracer switch needs the particle types");
    const int64_t np = S.nplanes();
    if(np == 0)
        return;
    MPG_CHECK(d_planes && npart, "potential planes: null output");
    PlaneEngine &pe = eng->planes;
    const size_t R2 = (size_t)S.R * S.R;
    // counters: what mpg_set_plane_counter_budget allows, else a quarter of what is free on the device now (the PM meshes, the tree and the
    // particles are allocated already); one plane at least.  Over several ranks the batch sets the number and the lengths of the
    // collectives below, so it is the smallest any rank can hold (a MIN made of a MAX all-reduce)
    const size_t per_plane = R2 * (sizeof(unsigned) + (many ? sizeof(unsigned long long) : 0));
    size_t room = pe.budget;
    if(room == 0) {
        size_t free_b = 0, total_b = 0;
        MPG_HIP(hipMemGetInfo(&free_b, &total_b));
        room = std::max(pe.counts.cap * sizeof(unsigned), free_b / 4);
    }
    int64_t batch = (int64_t)std::max<size_t>(1, room / per_plane);
    if(batch > np)
        batch = np;
    if(many) {
        int64_t neg = -batch;
        red->max_host(red->ctx, &neg, 1);
        batch = -neg;
    }
    pe.counts.reserve((size_t)batch * R2);
    if(many)
        pe.wide.reserve((size_t)batch * R2);
    // lenstools.c:248-249, 264-271, 292
    const double H0 = 100 * par->HubbleParam * 3.2407793e-20;
    const double LIGHTCGS = 2.99792458e10, CM_PER_KPC = 3.085678e21;
    const double cosmo_normalization = 1.5 * pow(H0, 2) * par->omega_source / pow(LIGHTCGS, 2);
    const double b = S.box / S.R;
    const double density_normalization = S.thickness * par->comoving_distance * pow(CM_PER_KPC / par->HubbleParam, 2) / par->atime;
    const double post = cosmo_normalization * density_normalization;
    std::vector<unsigned long long> hs;
    bool corr_ready = false;
    for(int64_t p0 = 0; p0 < np; p0 += batch) {
        const int64_t p1 = std::min(np, p0 + batch);
        int64_t err = planes_count_batch(eng, S, d_flags, p0, p1, pe.counts.p, hs);
        if(many) // (a rank that refused alone would leave the others waiting in the sums below)
            red->max_host(red->ctx, &err, 1);
        planes_count_refuse((int)err);
        int64_t nact = (int64_t)hs[0];
        std::vector<int64_t> tot(hs.begin() + 2 + p0, hs.begin() + 2 + p1);
        if(many) { // every rank's counters, widened, are summed: one solve instead of one per rank (the solve is linear; plane.c:654)
            const size_t m = (size_t)(p1 - p0) * R2;
            hipLaunchKernelGGL(k_plane_widen, dim3(blocks_for(m)), dim3(256), 0, eng->stream, m, pe.counts.p, pe.wide.p);
            MPG_HIP(hipGetLastError());
            red->sum_device(red->ctx, (int64_t *)pe.wide.p, (int64_t)m);
            tot.push_back(nact);
            red->sum_host(red->ctx, tot.data(), (int64_t)tot.size());
            nact = tot.back();
            tot.pop_back();
        }
        MPG_CHECK(nact > 0, "potential planes: cannot build a potential plane from zero active particle count"); // lenstools.c:290
        const double f = 1. / nact * (pow(S.box, 3) / (b * b * S.thickness));
        if(par->fn && !corr_ready) { // (after the counting pass has vouched for the positions)
            pe.correction_init(eng->pm, S, eng->n, eng->d_pos, eng->d_mass, eng->d_type, d_flags, par->fn, par->ctx, par->BoxSize_in_MPC, eng->stream);
            corr_ready = true;
        }
        for(int64_t p = p0; p < p1; p++) {
            npart[p] = tot[p - p0];
            double *out = d_planes + (size_t)p * R2;
            if(npart[p] <= 0) // lenstools.c:301: the plane stays zero
                MPG_HIP(hipMemsetAsync(out, 0, R2 * sizeof(double), eng->stream));
            else if(many)
                pe.solve(S, pe.wide.p + (size_t)(p - p0) * R2, true, f, b, par->comoving_distance, post, out, eng->stream);
            else
                pe.solve(S, pe.counts.p + (size_t)(p - p0) * R2, false, f, b, par->comoving_distance, post, out, eng->stream);
            if(par->fn)
                pe.correction_add(eng->pm, S, (int)(p / S.nnormals), S.normals[p % S.nnormals], par->comoving_distance, post, out, eng->stream);
        }
    }
}

extern "C" {

int mpg_plane_count(mpg_engine *eng, const mpg_plane_params *par, double BoxSize, int64_t *ncuts)
{
    API_BEGIN
    MPG_CHECK(par && ncuts, "mpg_plane_count: null argument");
    if(!(BoxSize > 0)) { // the box of the particles a device or resident call would run on
        MPG_CHECK(eng && eng->box > 0, "mpg_plane_count: no BoxSize given and no particles bound");
        BoxSize = eng->box;
    }
    const double th = par->Thickness > 0 ? par->Thickness : BoxSize;
    *ncuts = par->ncuts > 0 ? par->ncuts : (int64_t)(BoxSize / th);
    API_END
}

int mpg_set_plane_counter_budget(mpg_engine *eng, int64_t bytes)
{
    API_BEGIN
    MPG_CHECK(eng && bytes >= 0, "mpg_set_plane_counter_budget: bad argument");
    eng->planes.budget = (size_t)bytes;
    API_END
}

int mpg_dev_potential_planes(mpg_engine *eng, const mpg_plane_params *params, const unsigned char *d_flags, double *d_planes, int64_t *npart)
{
    API_BEGIN
    MPG_CHECK(eng && params, "null argument");
    MPG_HIP(hipSetDevice(eng->device));
    eng->host_join();
    planes_run(eng, params, d_flags, d_planes, npart, nullptr);
    API_END
}

int mpg_dev_plane_counts(mpg_engine *eng, const mpg_plane_params *params, const unsigned char *d_flags, uint32_t *d_counts, int64_t *n_active)
{
    API_BEGIN
    MPG_CHECK(eng && params && d_counts, "null argument");
    MPG_HIP(hipSetDevice(eng->device));
    eng->host_join();
    PlaneSetup S;
    planes_setup(eng, params, S);
    if(S.nplanes() > 0) {
        std::vector<unsigned long long> hs;
        MPG_CHECK(!S.tracer || eng->d_type || eng->n == 0, "potential planes: the hybrid-neutrino tracer switch needs the particle types");
        planes_count_refuse(planes_count_batch(eng, S, d_flags, 0, S.nplanes(), d_counts, hs));
        if(n_active)
            *n_active = (int64_t)hs[0];
    }
    API_END
}
}
