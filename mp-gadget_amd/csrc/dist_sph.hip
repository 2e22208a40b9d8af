// dist_sph.hip -- density() and hydro_force() of the multi-rank layer (dist.hip has the overview): the SPH loops over the rank's own gas
// with the ghosts of the last mpg_dist_dev_force_tree_build as neighbours.
#include "dist_internal.h"
#include <rocprim/rocprim.hpp>

namespace {

// ---- SPH columns of the ghosts: 16 words per row before the density loop, 6 after it
struct SphIn { // own arrays (device, may be null)
    const uint8_t *type, *tbh, *tbg;
    const double *hsml, *vel, *entropy, *gacc, *gpm, *hin, *dte;
};

__global__ void __launch_bounds__(256) k_pack_sph_in(int64_t ns, const int *__restrict__ idx, SphIn a, double *__restrict__ rows)
{
    const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if(k >= ns)
        return;
    const int64_t i = idx[k];
    double *r = rows + 16 * k;
    r[0] = a.hsml[i];
    for(int j = 0; j < 3; j++) {
        r[1 + j] = a.vel ? a.vel[3 * i + j] : 0.0;
        r[5 + j] = a.gacc ? a.gacc[3 * i + j] : 0.0;
        r[8 + j] = a.gpm ? a.gpm[3 * i + j] : 0.0;
        r[11 + j] = a.hin ? a.hin[3 * i + j] : 0.0;
    }
    r[4] = a.entropy ? a.entropy[i] : 0.0;
    r[14] = a.dte ? a.dte[i] : 0.0;
    const unsigned long long w = (unsigned long long)(a.type ? a.type[i] : 0) | ((unsigned long long)(a.tbh ? a.tbh[i] : 0) << 8) |
                                 ((unsigned long long)(a.tbg ? a.tbg[i] : 0) << 16);
    r[15] = __longlong_as_double((long long)w);
}

struct SphLocal { // arrays over [own | ghosts]
    uint8_t *type, *tbh, *tbg;
    double *hsml, *vel, *entropy, *gacc, *gpm, *hin, *dte;
};

__global__ void __launch_bounds__(256) k_unpack_sph_in(int64_t nr, const double *__restrict__ rows, SphLocal a, int64_t off)
{
    const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if(k >= nr)
        return;
    const double *r = rows + 16 * k;
    const int64_t i = off + k;
    a.hsml[i] = r[0];
    for(int j = 0; j < 3; j++) {
        a.vel[3 * i + j] = r[1 + j];
        a.gacc[3 * i + j] = r[5 + j];
        a.gpm[3 * i + j] = r[8 + j];
        a.hin[3 * i + j] = r[11 + j];
    }
    a.entropy[i] = r[4];
    a.dte[i] = r[14];
    const unsigned long long w = (unsigned long long)__double_as_longlong(r[15]);
    a.type[i] = (uint8_t)(w & 255);
    a.tbh[i] = (uint8_t)((w >> 8) & 255);
    a.tbg[i] = (uint8_t)((w >> 16) & 255);
}

// own rows of the local inputs (absent optional inputs read as zero)
__global__ void __launch_bounds__(256) k_fill_sph_own(int64_t n, SphIn a, SphLocal l)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if(i >= n)
        return;
    l.hsml[i] = a.hsml[i];
    for(int j = 0; j < 3; j++) {
        l.vel[3 * i + j] = a.vel ? a.vel[3 * i + j] : 0.0;
        l.gacc[3 * i + j] = a.gacc ? a.gacc[3 * i + j] : 0.0;
        l.gpm[3 * i + j] = a.gpm ? a.gpm[3 * i + j] : 0.0;
        l.hin[3 * i + j] = a.hin ? a.hin[3 * i + j] : 0.0;
    }
    l.entropy[i] = a.entropy ? a.entropy[i] : 0.0;
    l.dte[i] = a.dte ? a.dte[i] : 0.0;
    l.type[i] = a.type ? a.type[i] : (uint8_t)0;
    l.tbh[i] = a.tbh ? a.tbh[i] : (uint8_t)0;
    l.tbg[i] = a.tbg ? a.tbg[i] : (uint8_t)0;
}

// the six fields the hydro loop reads of its neighbours, of the own particles that are somebody's ghosts
__global__ void __launch_bounds__(256) k_pack_sph_mid(int64_t ns, const int *__restrict__ idx, const double *hsml, const double *density,
                                                      const double *egy, const double *dhsml, const double *divvel, const double *curlvel,
                                                      double *__restrict__ rows)
{
    const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if(k >= ns)
        return;
    const int64_t i = idx[k];
    double *r = rows + 6 * k;
    r[0] = hsml[i];
    r[1] = density[i];
    r[2] = egy ? egy[i] : 0.0;
    r[3] = dhsml[i];
    r[4] = divvel[i];
    r[5] = curlvel[i];
}

__global__ void __launch_bounds__(256) k_unpack_sph_mid(int64_t nr, const double *__restrict__ rows, int64_t off, double *hsml, double *density,
                                                        double *egy, double *dhsml, double *divvel, double *curlvel)
{
    const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if(k >= nr)
        return;
    const double *r = rows + 6 * k;
    const int64_t i = off + k;
    hsml[i] = r[0];
    density[i] = r[1];
    if(egy)
        egy[i] = r[2];
    dhsml[i] = r[3];
    divvel[i] = r[4];
    curlvel[i] = r[5];
}

// density_haswork (density.c:521-530): gas and black holes (bh = 1; swallowed ones carry type 7 here, like garbage); hydro_haswork: gas
struct IsOwnGas {
    const uint8_t *type;
    int bh;
    __host__ __device__ bool operator()(const int &i) const { return type[i] == 0 || (bh && type[i] == 5); }
};
struct IsActiveGas {
    const uint8_t *type, *flag;
    int bh;
    __host__ __device__ bool operator()(const int &i) const { return (type[i] == 0 || (bh && type[i] == 5)) && flag[i] != 0; }
};

__global__ void __launch_bounds__(256) k_max_gas_hsml(int64_t n, const uint8_t *__restrict__ type, const double *__restrict__ hsml, const int bh,
                                                      unsigned long long *__restrict__ out)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    double h = (i < n && (type[i] == 0 || (bh && type[i] == 5))) ? hsml[i] : 0.0;
    for(int off = 32; off > 0; off >>= 1)
        h = fmax(h, __shfl_down(h, off));
    if((threadIdx.x & 63) == 0 && h > 0)
        atomicMax(out, (unsigned long long)__double_as_longlong(h)); // (positive doubles order like their bit patterns)
}

// the arrays over [own | ghosts] as the loops of sph.hip take them (d->s_in, d->s_out, d->s_tbh, d->s_tbg)
mpg_sph_arrays sph_local_arrays(mpg_dist *d, bool gradrho)
{
    mpg_sph_arrays L;
    memset(&L, 0, sizeof(L));
    L.hsml = d->s_in[0].p;
    L.vel = d->s_in[1].p;
    L.entropy = d->s_in[2].p;
    L.gacc = d->s_in[3].p;
    L.gpm = d->s_in[4].p;
    L.hydroacc_in = d->s_in[5].p;
    L.dtentropy_in = d->s_in[6].p;
    L.tb_hydro = d->s_tbh.p;
    L.tb_grav = d->s_tbg.p;
    L.dthsml = d->s_out[0].p;
    L.density = d->s_out[1].p;
    L.egywtdensity = d->s_out[2].p;
    L.dhsmlegyfac = d->s_out[3].p;
    L.divvel = d->s_out[4].p;
    L.curlvel = d->s_out[5].p;
    L.gradrho = gradrho ? d->s_out[6].p : nullptr;
    L.hydroacc_out = d->s_out[7].p;
    L.dtentropy_out = d->s_out[8].p;
    L.maxsignalvel = d->s_out[9].p;
    return L;
}

// the own rows of some columns between the caller's arrays and the local ones; a column either side lacks is left out
struct OwnRows {
    double *dst;
    const double *src;
    int w;
};
void copy_own_rows(mpg_dist *d, int64_t n_own, std::initializer_list<OwnRows> cols)
{
    for(const OwnRows &c : cols)
        if(c.dst && c.src && n_own > 0)
            MPG_HIP(hipMemcpyAsync(c.dst, c.src, (size_t)c.w * n_own * sizeof(double), hipMemcpyDeviceToDevice, d->eng->stream));
}

} // namespace

extern "C" {

/* ---- density() and hydro_force() for the rank's own gas (density.h:42, hydra.h) on the particle set of the last
 * mpg_dist_dev_force_tree_build: own particles + the ghosts of every tree cell within the domain margin, which must cover the largest
 * smoothing length (checked).  The ghosts' inputs arrive along the ghost plan before the density loop; their Hsml, Density,
 * EgyWtDensity, DhsmlEgyDensityFactor, DivVel, CurlVel are refreshed from their owners before the hydro loop (the search of
 * hydro_force is symmetric in the two smoothing lengths, treewalk.c:1015-1042). */
int mpg_dist_dev_density(mpg_dist *d, int64_t n_own, const uint8_t *d_type, const mpg_sph_arrays *A, const mpg_sph_times *T, int update_hsml,
                         int DoEgyDensity)
{
    return mpg_dist_dev_density_active(d, n_own, d_type, A, T, nullptr, 0, update_hsml, DoEgyDensity);
}

// the loop's targets: the own gas (d_active == null) or the own gas among the listed particles, ascending
static void sph_targets(mpg_dist *d, int64_t n_own, const int *d_active, int64_t nactive, const int bh)
{
    hipStream_t st = d->eng->stream;
    d->gas.reserve((size_t)n_own + 1);
    d->scount.reserve(4);
    d->ngas = 0;
    if(n_own == 0 || (d_active && nactive == 0))
        return;
    rocprim::counting_iterator<int> iota(0);
    unsigned bad = 0;
    if(d_active) {
        MPG_CHECK(nactive > 0 && nactive <= n_own, "mpg_dist SPH loop: bad number of active particles");
        flag_active_list(d, d_active, nactive, n_own);
        const IsActiveGas pred{d->s_type.p, d->actflag.p, bh};
        with_tmp(d, [&](void *tmp, size_t &tb) { return rocprim::select(tmp, tb, iota, d->gas.p, d->scount.p, (size_t)n_own, pred, st); });
        MPG_HIP(hipMemcpyAsync(&bad, d->err.p, sizeof(bad), hipMemcpyDeviceToHost, st));
    }
    else
        with_tmp(d, [&](void *tmp, size_t &tb) {
            return rocprim::select(tmp, tb, iota, d->gas.p, d->scount.p, (size_t)n_own, IsOwnGas{d->s_type.p, bh}, st);
        });
    unsigned long long c = 0;
    MPG_HIP(hipMemcpyAsync(&c, d->scount.p, sizeof(c), hipMemcpyDeviceToHost, st));
    sync(d);
    MPG_CHECK(bad == 0, "mpg_dist SPH loop: an active index is not an own particle");
    d->ngas = (int64_t)c;
}

int mpg_dist_dev_density_active(mpg_dist *d, int64_t n_own, const uint8_t *d_type, const mpg_sph_arrays *A, const mpg_sph_times *T,
                                const int *d_active, int64_t nactive, int update_hsml, int DoEgyDensity)
{
    API_BEGIN
    MPG_CHECK(d && A && T && A->hsml && A->density && A->dhsmlegyfac && A->divvel && A->curlvel, "null argument");
    MPG_CHECK(d->n_own_tree == n_own, "mpg_dist_dev_density: mpg_dist_dev_force_tree_build of this particle set first");
    mpg_engine *e = d->eng;
    MPG_HIP(hipSetDevice(e->device));
    hipStream_t st = e->stream;
    const Plan &pl = d->ghost;
    const int64_t nl = n_own + pl.nrecv;
    d->s_type.reserve((size_t)nl + 1);
    d->s_tbh.reserve((size_t)nl + 1);
    d->s_tbg.reserve((size_t)nl + 1);
    const int w_in[7] = {1, 3, 1, 3, 3, 3, 1}, w_out[11] = {1, 1, 1, 1, 1, 1, 3, 3, 1, 1, 0};
    for(int k = 0; k < 7; k++)
        d->s_in[k].reserve((size_t)w_in[k] * nl + 3);
    for(int k = 0; k < 10; k++) {
        d->s_out[k].reserve((size_t)w_out[k] * nl + 3);
        MPG_HIP(hipMemsetAsync(d->s_out[k].p, 0, (size_t)w_out[k] * nl * sizeof(double), st));
    }
    const SphIn in{d_type, A->tb_hydro, A->tb_grav, A->hsml, A->vel, A->entropy, A->gacc, A->gpm, A->hydroacc_in, A->dtentropy_in};
    const SphLocal loc{d->s_type.p, d->s_tbh.p, d->s_tbg.p, d->s_in[0].p, d->s_in[1].p, d->s_in[2].p, d->s_in[3].p, d->s_in[4].p, d->s_in[5].p,
                       d->s_in[6].p};
    if(n_own > 0)
        hipLaunchKernelGGL(k_fill_sph_own, dim3(nblk(n_own)), dim3(256), 0, st, n_own, in, loc);
    ship_rows(
        d, pl, 128, false,
        [&](char *rows) { hipLaunchKernelGGL(k_pack_sph_in, dim3(nblk(pl.nsend)), dim3(256), 0, st, pl.nsend, pl.idx.p, in, (double *)rows); },
        [&](const char *rows) { hipLaunchKernelGGL(k_unpack_sph_in, dim3(nblk(pl.nrecv)), dim3(256), 0, st, pl.nrecv, (const double *)rows, loc, n_own); });
    // the gas tree of the local set (force_tree_rebuild_mask(GASMASK), run.c:466); it REPLACES the gravity tree in the engine
    d->grav_tree_valid = false;
    MPG_CALL(mpg_dev_bind_particles(e, nl, d->lpos.p, d->lmass.p, d->s_type.p, d->box));
    MPG_CALL(mpg_dev_force_tree_rebuild_mask(e, 1, 0));
    sph_targets(d, n_own, d_active, nactive, 1); // (black holes are density targets whatever BlackHoleOn says: density_haswork)
    mpg_sph_arrays L = sph_local_arrays(d, A->gradrho != nullptr);
    if(d_active) {
        // a sub-step: the inactive own particles keep the results of their last density loop, which the hydro loop of this sub-step
        // reads and their owners hand to the ghosts (the reference leaves SphP of inactive particles alone)
        copy_own_rows(d, n_own, {{L.dthsml, A->dthsml, 1}, {L.density, A->density, 1}, {L.egywtdensity, A->egywtdensity, 1},
                                 {L.dhsmlegyfac, A->dhsmlegyfac, 1}, {L.divvel, A->divvel, 1}, {L.curlvel, A->curlvel, 1}, {L.gradrho, A->gradrho, 3}});
    }
    MPG_CALL(mpg_dev_density(e, &L, T, d->gas.p, d->ngas, update_hsml, DoEgyDensity, d->blackholes));
    // every neighbour within a smoothing length must be local: the largest one against the domain margin
    d->scount.reserve(4);
    MPG_HIP(hipMemsetAsync(d->scount.p, 0, sizeof(unsigned long long), st));
    if(n_own > 0)
        hipLaunchKernelGGL(k_max_gas_hsml, dim3(nblk(n_own)), dim3(256), 0, st, n_own, d->s_type.p, d->s_in[0].p, 1, d->scount.p);
    unsigned long long hb = 0;
    MPG_HIP(hipMemcpyAsync(&hb, d->scount.p, sizeof(hb), hipMemcpyDeviceToHost, st));
    sync(d);
    double hmax;
    memcpy(&hmax, &hb, sizeof(double));
    allreduce_host_f64(d, &hmax, 1, 1);
    d->last_hmax = hmax;
    MPG_CHECK(hmax <= d->margin, "mpg_dist_dev_density: the largest smoothing length exceeds the domain margin (mpg_dist_set_domain with a larger one)");
    // own rows out
    copy_own_rows(d, n_own, {{A->hsml, L.hsml, 1}, {A->dthsml, L.dthsml, 1}, {A->density, L.density, 1}, {A->egywtdensity, L.egywtdensity, 1},
                             {A->dhsmlegyfac, L.dhsmlegyfac, 1}, {A->divvel, L.divvel, 1}, {A->curlvel, L.curlvel, 1}, {A->gradrho, L.gradrho, 3}});
    d->sph_nl = nl;
    d->sph_n_own = n_own;
    API_END
}

int mpg_dist_dev_hydro_force(mpg_dist *d, int64_t n_own, const mpg_sph_arrays *A, const mpg_sph_times *T)
{
    return mpg_dist_dev_hydro_force_active(d, n_own, A, T, nullptr, 0);
}

int mpg_dist_dev_hydro_force_active(mpg_dist *d, int64_t n_own, const mpg_sph_arrays *A, const mpg_sph_times *T, const int *d_active,
                                    int64_t nactive)
{
    API_BEGIN
    MPG_CHECK(d && A && T && A->hydroacc_out && A->dtentropy_out && A->maxsignalvel, "null argument");
    MPG_CHECK(d->sph_n_own == n_own && d->sph_nl >= n_own, "mpg_dist_dev_hydro_force: mpg_dist_dev_density of this particle set first");
    mpg_engine *e = d->eng;
    MPG_HIP(hipSetDevice(e->device));
    hipStream_t st = e->stream;
    const Plan &pl = d->ghost;
    // the ghosts' density-loop results from their owners
    mpg_sph_arrays L = sph_local_arrays(d, false);
    ship_rows(
        d, pl, 48, false,
        [&](char *rows) {
            hipLaunchKernelGGL(k_pack_sph_mid, dim3(nblk(pl.nsend)), dim3(256), 0, st, pl.nsend, pl.idx.p, L.hsml, L.density, L.egywtdensity, L.dhsmlegyfac,
                               L.divvel, L.curlvel, (double *)rows);
        },
        [&](const char *rows) {
            hipLaunchKernelGGL(k_unpack_sph_mid, dim3(nblk(pl.nrecv)), dim3(256), 0, st, pl.nrecv, (const double *)rows, n_own, L.hsml, L.density, L.egywtdensity,
                               L.dhsmlegyfac, L.divvel, L.curlvel);
        });
    MPG_CALL(mpg_dev_force_tree_calc_hmax(e)); // force_tree_calc_moments of the gas tree, run.c:477
    sph_targets(d, n_own, d_active, nactive, 0); // (hydro_force: gas only, hydra.c:193)
    if(d_active) // (inactive particles keep their HydroAccel / DtEntropy / MaxSignalVel)
        copy_own_rows(d, n_own, {{L.hydroacc_out, A->hydroacc_out, 3}, {L.dtentropy_out, A->dtentropy_out, 1}, {L.maxsignalvel, A->maxsignalvel, 1}});
    MPG_CALL(mpg_dev_hydro_force(e, &L, T, d->gas.p, d->ngas));
    copy_own_rows(d, n_own, {{A->hydroacc_out, L.hydroacc_out, 3}, {A->dtentropy_out, L.dtentropy_out, 1}, {A->maxsignalvel, L.maxsignalvel, 1}});
    sync(d);
    API_END
}

double mpg_dist_last_max_hsml(mpg_dist *d) { return d ? d->last_hmax : 0; }

} // extern "C"
