// dist_gravity.hip -- gravity of the multi-rank layer (dist.hip has the overview): the slab PM by particle shipping, the ghost import, the
// local tree under the all-reduced top, the short-range walks on it, the tree of the active particles alone, the power spectrum and the
// potential planes over the ranks.
#include "dist_internal.h"
#include "pm_cic.h"
#include <algorithm>
#include <thread>
#include <rocprim/rocprim.hpp>

namespace {

struct alignas(16) PRow { // a particle on the wire
    double x, y, z;
    float m;
    unsigned pad;
};
struct alignas(16) RRow { // a PM result on the wire
    double gx, gy, gz, pot;
};
static_assert(sizeof(PRow) == 32 && sizeof(RRow) == 32, "wire rows are 32 bytes");

// skip (may be null): garbage and swallowed particles take no part in the force (gravpm.c:176-179, forcetree.c:806): they go nowhere
__global__ void __launch_bounds__(256) k_pm_mask(int64_t n, const double *__restrict__ pos, double cellsize, int nmesh, int P,
                                                 const unsigned char *__restrict__ skip, unsigned long long *__restrict__ mask)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if(i >= n)
        return;
    int o0, o1;
    mpg::pm_owners(pos[3 * i], cellsize, nmesh, P, o0, o1);
    mask[i] = (skip && skip[i]) ? 0ull : ((1ull << o0) | (1ull << o1));
}

// level-La tree cell of a position by the reference's own floating-point descent (forcetree.c get_subnode, as k_keys of
// tree_build.hip replays it), so that "cell" here is bit for bit the cell of the tree; cells numbered (ix * nc + iy) * nc + iz
__device__ __forceinline__ unsigned tree_cell(double x, double y, double z, double box, int La)
{
    double cx = box / 2., cy = box / 2., cz = box / 2.;
    double len = box * 1.001;
    unsigned ix = 0, iy = 0, iz = 0;
    for(int l = 0; l < La; l++) {
        const double q = 0.25 * len;
        const int bx = x > cx, by = y > cy, bz = z > cz;
        ix = 2 * ix + bx;
        iy = 2 * iy + by;
        iz = 2 * iz + bz;
        cx += bx ? q : -q;
        cy += by ? q : -q;
        cz += bz ? q : -q;
        len *= 0.5;
    }
    return ((ix << La) | iy) << La | iz;
}

__global__ void __launch_bounds__(256) k_need_mask(int64_t n, const double *__restrict__ pos, double box, int La,
                                                   const unsigned long long *__restrict__ need, int me, const unsigned char *__restrict__ skip,
                                                   unsigned long long *__restrict__ mask)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if(i >= n)
        return;
    mask[i] = (skip && skip[i]) ? 0ull : (need[tree_cell(pos[3 * i], pos[3 * i + 1], pos[3 * i + 2], box, La)] & ~(1ull << me));
}

// types of the local set [own | ghosts] when the own rows hold garbage: 7 (no bit of any tree mask) for those, 1 otherwise
__global__ void __launch_bounds__(256) k_local_types(int64_t nl, int64_t n_own, const unsigned char *__restrict__ skip, uint8_t *__restrict__ type)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if(i < nl)
        type[i] = (i < n_own && skip[i]) ? 7 : 1;
}

__global__ void __launch_bounds__(256) k_count_listed(int64_t n, const int *__restrict__ list, const unsigned char *__restrict__ flags,
                                                       unsigned long long *__restrict__ count)
{
    const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const bool hit = k < n && flags[list[k]] != 0;
    const unsigned long long m = __builtin_amdgcn_ballot_w64(hit);
    if(m != 0ull && (threadIdx.x & 63) == 0)
        atomicAdd(count, (unsigned long long)__builtin_popcountll(m));
}

__global__ void __launch_bounds__(256) k_pack_particles(int64_t ns, const int *__restrict__ idx, const double *__restrict__ pos,
                                                        const float *__restrict__ mass, PRow *__restrict__ rows)
{
    const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if(k >= ns)
        return;
    const int64_t i = idx[k];
    PRow r;
    r.x = pos[3 * i];
    r.y = pos[3 * i + 1];
    r.z = pos[3 * i + 2];
    r.m = mass[i];
    r.pad = 0u;
    rows[k] = r;
}

__global__ void __launch_bounds__(256) k_unpack_particles(int64_t nr, const PRow *__restrict__ rows, double *__restrict__ pos,
                                                          float *__restrict__ mass)
{
    const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if(k >= nr)
        return;
    const PRow r = rows[k];
    pos[3 * k] = r.x;
    pos[3 * k + 1] = r.y;
    pos[3 * k + 2] = r.z;
    mass[k] = r.m;
}

__global__ void __launch_bounds__(256) k_pack_results(int64_t n, const double *__restrict__ gravpm, const double *__restrict__ pot,
                                                      RRow *__restrict__ rows)
{
    const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if(k >= n)
        return;
    RRow r;
    r.gx = gravpm[3 * k];
    r.gy = gravpm[3 * k + 1];
    r.gz = gravpm[3 * k + 2];
    r.pot = pot[k];
    rows[k] = r;
}

// rows come back in the order of the send list; the row from the owner of the particle's BASE cell carries the result
__global__ void __launch_bounds__(256) k_scatter_results(int64_t ns, const int *__restrict__ idx, const RRow *__restrict__ rows,
                                                         const long long *__restrict__ sdsp, int nt, const double *__restrict__ pos,
                                                         double cellsize, int nmesh, int P, double *__restrict__ gravpm,
                                                         double *__restrict__ pot)
{
    const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if(k >= ns)
        return;
    int d = 0;
    while(d + 1 < nt && k >= sdsp[d + 1])
        d++;
    const int64_t i = idx[k];
    int o0, o1;
    mpg::pm_owners(pos[3 * i], cellsize, nmesh, P, o0, o1);
    if(o0 != d)
        return;
    const RRow r = rows[k];
    gravpm[3 * i] = r.gx;
    gravpm[3 * i + 1] = r.gy;
    gravpm[3 * i + 2] = r.gz;
    if(pot)
        pot[i] += r.pot; // readout_potential accumulates (gravpm.c:499-501)
}

struct IsFlagged {
    const uint8_t *flag;
    __host__ __device__ bool operator()(const int &i) const { return flag[i] != 0; }
};

// own particles of the local tree, in tree order (caller index < n_own)
struct IsOwn {
    int n_own;
    __host__ __device__ bool operator()(const unsigned &ci) const { return (int)ci < n_own; }
};

// number of OWN particles per level-(La-1) cell (sorted keys: mostly one cell per wave)
__global__ void __launch_bounds__(256) k_top_counts(int64_t npart, const uint64_t *__restrict__ keys, const uint32_t *__restrict__ order,
                                                    int64_t n_own, int shift, double *__restrict__ out)
{
    const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const bool own = k < npart && (int64_t)order[k] < n_own;
    const unsigned long long cell = own ? (unsigned long long)(keys[k] >> shift) : ~0ull;
    const unsigned long long c0 = __shfl(cell, 0);
    const unsigned long long nown = __popcll(__ballot(own)); // (taken by all lanes: inside the branch below only lane 0 would vote)
    if(__ballot(cell != c0) == 0) {
        if(c0 != ~0ull && (threadIdx.x & 63) == 0)
            unsafeAtomicAdd(&out[c0], (double)nown);
    }
    else if(own)
        unsafeAtomicAdd(&out[cell], 1.0);
}

struct InRange {
    int lo, hi;
    __host__ __device__ bool operator()(const unsigned &ci) const { return (int)ci >= lo && (int)ci < hi; }
};

void pm_slab_setup(mpg_dist *d)
{
    mpg_engine *e = d->eng;
    MPG_CHECK(e->pm.nmesh > 0, "mpg_dist: gravpm_init_periodic first");
    MPG_CHECK(e->pm.nmesh % d->nt == 0, "mpg_dist: Nmesh must be a multiple of the number of ranks");
    e->pm.slab_init(d->me, d->nt);
    d->per_peer = (int64_t)e->pm.slab_cplx_per_peer();
    d->plane = (int64_t)e->pm.nmesh * e->pm.nmesh;
    const size_t tr = (size_t)2 * d->per_peer * d->nt;
    d->sendA.reserve(tr);
    d->recvA.reserve(tr);
    d->sendB.reserve(tr);
    d->recvB.reserve(tr);
    d->gsend.reserve((size_t)5 * d->plane);
    d->grecv.reserve((size_t)5 * d->plane);
    d->slab_ready = true;
}

// gravpm_force over the ranks: ship particles to their slabs, solve, return the results
void pm_step(mpg_dist *d, int64_t n, const double *pos, const float *mass, double *gravpm, double *pot)
{
    mpg_engine *e = d->eng;
    hipStream_t st = e->stream;
    PMesh &pm = e->pm;
    if(!d->slab_ready || pm.slab.rank != d->me || pm.slab.world != d->nt || !pm.slab.ready)
        pm_slab_setup(d);
    const int nmesh = pm.nmesh, P = nmesh / d->nt;
    // hybrid neutrinos as tracers: type-2 rows travel with mass 0 (they are still read out)
    MPG_CHECK(!pm.hybrid_tracer || n == 0 || d->types_for(n),
              "mpg_dist: the hybrid-neutrino deposit mask needs the types of the own rows (mpg_dist_dev_set_types with this n_own)");
    mass = pm.tracer_mass(n, mass, d->types_for(n), st);
    d->mask.reserve((size_t)n + 1);
    if(n > 0)
        hipLaunchKernelGGL(k_pm_mask, dim3(nblk(n)), dim3(256), 0, st, n, pos, pm.cellsize, nmesh, P, d->skip_for(n), d->mask.p);
    build_plan(d, d->pm, n, d->mask.p);
    Plan &pl = d->pm;
    const int64_t nr = pl.nrecv;
    d->spos.reserve((size_t)3 * nr + 3);
    d->smass.reserve((size_t)nr + 1);
    d->sgrav.reserve((size_t)3 * nr + 3);
    d->spot.reserve((size_t)nr + 1);
    ship_rows(
        d, pl, sizeof(PRow), false,
        [&](char *out) { hipLaunchKernelGGL(k_pack_particles, dim3(nblk(pl.nsend)), dim3(256), 0, st, pl.nsend, pl.idx.p, pos, mass, (PRow *)out); },
        [&](const char *in) { hipLaunchKernelGGL(k_unpack_particles, dim3(nblk(nr)), dim3(256), 0, st, nr, (const PRow *)in, d->spos.p, d->smass.p); });
    // local stages of the slab solver with the two transposes and the neighbour planes in between (pm.hip, "slab-decomposed form")
    pm.slab_forward_a(nr, d->spos.p, d->smass.p, d->sendA.p, st);
    a2a_uniform(d, d->sendA.p, d->recvA.p, 16 * d->per_peer);
    if(pm.nu_fn) { // neutrino response: the bins of every rank summed (powerspectrum_sum's MPI_Allreduce), then the same callback everywhere
        pm.slab_forward_b1(d->recvA.p, st);
        const size_t nb = (size_t)nmesh;
        double *acc;
        unsigned long long *modes;
        pm.nu_fetch(st, &acc, &modes);
        std::vector<double> a(acc, acc + 2 * nb + 1);
        std::vector<int64_t> m((const int64_t *)modes, (const int64_t *)modes + nb);
        allreduce_host_f64(d, a.data(), (int64_t)a.size(), 0);
        allreduce_i64(d, m.data(), (int64_t)nb, 0);
        pm.nu_table(a.data(), (const unsigned long long *)m.data(), st);
        pm.slab_forward_b2(d->sendB.p, st);
    }
    else
        pm.slab_forward_b(d->recvA.p, d->sendB.p, st);
    a2a_uniform(d, d->sendB.p, d->recvB.p, 16 * d->per_peer);
    pm.slab_inverse_c(d->recvB.p, d->gsend.p, st);
    {
        // the first 3 planes go to the previous rank (its upper ghosts), the last 2 to the next rank (its lower ghosts);
        // received: from the next rank its first 3, from the previous rank its last 2.  One alltoallv; with 1 or 2 ranks both
        // neighbours are the same rank, which then gets [first 3 | last 2] in one block and sends the same
        const int nt = d->nt, prev = (d->me + nt - 1) % nt, next = (d->me + 1) % nt;
        const int64_t pb = d->plane * 8;
        std::vector<int64_t> sb(nt, 0), sd(nt, 0), rb(nt, 0), rd(nt, 0);
        if(prev == next) { // (nt <= 2)
            sb[prev] = 5 * pb;
            rb[prev] = 5 * pb;
        }
        else {
            sb[prev] = 3 * pb;
            sd[prev] = 0;
            sb[next] = 2 * pb;
            sd[next] = 3 * pb;
            rb[next] = 3 * pb;
            rd[next] = 0;
            rb[prev] = 2 * pb;
            rd[prev] = 3 * pb;
        }
        a2av(d, d->gsend.p, sb, sd, d->grecv.p, rb, rd, 5 * pb, 5 * pb);
    }
    // the received particles whose base cell is mine are read out (the kernel tells: no target list, no count read back - round 4)
    if(nr > 0) {
        MPG_HIP(hipMemsetAsync(d->sgrav.p, 0, (size_t)3 * nr * sizeof(double), st));
        MPG_HIP(hipMemsetAsync(d->spot.p, 0, (size_t)nr * sizeof(double), st));
    }
    pm.slab_readout_rows(d->grecv.p, nr, d->spos.p, d->sgrav.p, d->spot.p, st);
    // results back along the same lists
    ship_rows(
        d, pl, sizeof(RRow), true, [&](char *out) { hipLaunchKernelGGL(k_pack_results, dim3(nblk(nr)), dim3(256), 0, st, nr, d->sgrav.p, d->spot.p, (RRow *)out); },
        [&](const char *in) {
            hipLaunchKernelGGL(k_scatter_results, dim3(nblk(pl.nsend)), dim3(256), 0, st, pl.nsend, pl.idx.p, (const RRow *)in, pl.d_sdsp.p, d->nt, pos,
                               pm.cellsize, nmesh, P, gravpm, pot);
        });
    MPG_HIP(hipGetLastError());
    d->stats[1] = pl.nsend;
}

} // namespace

// own particles followed by the ghosts of every needed cell: d->lpos / d->lmass; returns the local count
int64_t import_ghosts(mpg_dist *d, int64_t n, const double *pos, const float *mass)
{
    hipStream_t st = d->eng->stream;
    d->mask.reserve((size_t)n + 1);
    if(n > 0)
        hipLaunchKernelGGL(k_need_mask, dim3(nblk(n)), dim3(256), 0, st, n, pos, d->box, d->La, d->need.p, d->me, d->skip_for(n), d->mask.p);
    build_plan(d, d->ghost, n, d->mask.p);
    Plan &pl = d->ghost;
    // (the own rows are copied between the exchange and the unpack launch, which therefore stands below)
    const char *rows = ship_rows(d, pl, sizeof(PRow), false, [&](char *out) {
        hipLaunchKernelGGL(k_pack_particles, dim3(nblk(pl.nsend)), dim3(256), 0, st, pl.nsend, pl.idx.p, pos, mass, (PRow *)out);
    });
    const int64_t nl = n + pl.nrecv;
    d->lpos.reserve((size_t)3 * nl + 3);
    d->lmass.reserve((size_t)nl + 1);
    if(n > 0) {
        MPG_HIP(hipMemcpyAsync(d->lpos.p, pos, (size_t)3 * n * sizeof(double), hipMemcpyDeviceToDevice, st));
        MPG_HIP(hipMemcpyAsync(d->lmass.p, mass, (size_t)n * sizeof(float), hipMemcpyDeviceToDevice, st));
    }
    if(pl.nrecv > 0)
        hipLaunchKernelGGL(k_unpack_particles, dim3(nblk(pl.nrecv)), dim3(256), 0, st, pl.nrecv, (const PRow *)rows, d->lpos.p + 3 * n, d->lmass.p + n);
    MPG_HIP(hipGetLastError());
    d->stats[0] = pl.nrecv;
    d->stats[2] = nl;
    return nl;
}

namespace {

// moments of the nodes above level La from the sums over all ranks (tree_build.hip, "the top of the tree from global sums")
// levels La-2 .. 0 of the global top from the all-reduced sums of level La-1 (4 doubles per cell, children consecutive in octant-path
// numbering), laid out level 0 first as k_top_set reads them; the all-reduced particle counts are checked on the way: a cell above
// the decomposition level is internal on every rank whatever it holds locally, and the global tree agrees only if it holds more than
// NMAXCHILD particles in all.  One block: the levels depend on each other and the whole top is a few thousand cells.
__global__ void __launch_bounds__(1024) k_top_levels(int La, const double *__restrict__ fine, const double *__restrict__ cnt, double *__restrict__ all,
                                                     unsigned *__restrict__ err)
{
    const size_t nfine = (size_t)1 << (3 * (La - 1));
    size_t off = 0;
    for(int l = 0; l < La - 1; l++)
        off += (size_t)1 << (3 * l);
    for(size_t c = threadIdx.x; c < nfine; c += blockDim.x) {
        const double k = cnt[c];
        if(!(k == 0 || k > NMAXCHILD))
            atomicOr(err, 1u);
        for(int j = 0; j < 4; j++)
            all[(off + c) * 4 + j] = fine[c * 4 + j];
    }
    for(int l = La - 2; l >= 0; l--) {
        __syncthreads();
        const size_t nc = (size_t)1 << (3 * l), coff = off;
        off -= nc;
        for(size_t c = threadIdx.x; c < nc; c += blockDim.x)
            for(int j = 0; j < 4; j++) {
                double sum = 0.0; // (children added in octant order, as the host loop of rounds 2-3 did: same bits)
                for(int k = 0; k < 8; k++)
                    sum += all[(coff + 8 * c + k) * 4 + j];
                all[(off + c) * 4 + j] = sum;
            }
    }
}

void global_top(mpg_dist *d, int64_t n_own)
{
    mpg_engine *e = d->eng;
    hipStream_t st = e->stream;
    const int La = d->La;
    const size_t nfine = (size_t)1 << (3 * (La - 1));
    size_t ntot = 0;
    for(int l = 0; l < La; l++)
        ntot += (size_t)1 << (3 * l);
    // [nfine * 4 sums | nfine counts | ntot * 4 levels]
    d->top.reserve(nfine * 5 + ntot * 4 + 8);
    e->tree.top_partial(La, n_own, d->top.p, st);
    double *cnt = d->top.p + nfine * 4, *all = d->top.p + nfine * 5;
    MPG_HIP(hipMemsetAsync(cnt, 0, nfine * sizeof(double), st));
    if(e->tree.npart > 0)
        hipLaunchKernelGGL(k_top_counts, dim3(nblk(e->tree.npart)), dim3(256), 0, st, e->tree.npart, e->tree.keys_b.p, e->tree.idx_b.p, n_own,
                           3 * (MAXLEVEL - (La - 1)), cnt);
    if(d->stream_ordered) { // (RCCL: the all-reduce is the next piece of work on the stream)
        comm_ready(d);
        cb(d->comm.allreduce(d->comm.ctx, d->top.p, (int64_t)(nfine * 5), 0, 0, 1), "allreduce");
    }
    else if(!(d->nt == 1 && !d->comm.allreduce)) {
        d->htop.reserve(nfine * 5 + 8);
        MPG_HIP(hipMemcpyAsync(d->htop.p, d->top.p, nfine * 5 * sizeof(double), hipMemcpyDeviceToHost, st));
        sync(d);
        allreduce_host_f64(d, d->htop.p, (int64_t)(nfine * 5), 0);
        MPG_HIP(hipMemcpyAsync(d->top.p, d->htop.p, nfine * 5 * sizeof(double), hipMemcpyHostToDevice, st));
    }
    // the checks of this phase raise bits of d->err[1..2]; tree_finish reads them with the target count (no wait here)
    d->err.reserve(8);
    MPG_HIP(hipMemsetAsync(d->err.p + 1, 0, 2 * sizeof(unsigned), st));
    hipLaunchKernelGGL(k_top_levels, dim3(1), dim3(1024), 0, st, La, (const double *)d->top.p, (const double *)cnt, all, d->err.p + 1);
    e->tree.top_set(La, all, st, (int *)(d->err.p + 2));
}

// What opens the calls that take the rank's particles, behind their own null checks and before their first side effect: the domain,
// the device, the particle number ...
mpg_engine *particles_begin(mpg_dist *d, int64_t n_own)
{
    MPG_CHECK(d->have_domain, "mpg_dist: mpg_dist_set_domain first");
    MPG_HIP(hipSetDevice(d->eng->device));
    MPG_CHECK(n_own < (1ll << 31), "mpg_dist: too many particles on one rank");
    return d->eng;
}

// ... and of those with a PM step the mesh, the byte counts of the step and the GravPM of the rows that take no part
mpg_engine *pm_begin(mpg_dist *d, int64_t n_own, double *d_gravpm)
{
    mpg_engine *e = particles_begin(d, n_own);
    MPG_CHECK(e->pm.box == d->box, "mpg_dist: BoxSize of the mesh differs from the domain's");
    d->stats[4] = d->stats[5] = 0;
    if(d->skip_for(n_own)) // (gravpm.c:88-92 zeroes GravPM of every particle; the readout then reaches the live ones only)
        MPG_HIP(hipMemsetAsync(d_gravpm, 0, (size_t)3 * n_own * sizeof(double), e->stream));
    return e;
}

} // namespace

// The three phases of the local tree: ghosts (collective), build (no collective: may run on another stream beside the PM), global top
// + targets (collective).
void tree_build_local(mpg_dist *d, int64_t n_own, int64_t nl, hipStream_t st)
{
    mpg_engine *e = d->eng;
    const uint8_t *ltype = nullptr;
    if(d->skip_for(n_own)) { // garbage among the own rows: type 7 keeps them out of the tree (forcetree.c:806)
        d->ltype.reserve((size_t)nl + 1);
        hipLaunchKernelGGL(k_local_types, dim3(nblk(nl)), dim3(256), 0, st, nl, n_own, d->d_skip, d->ltype.p);
        ltype = d->ltype.p;
    }
    MPG_CALL(mpg_dev_bind_particles(e, nl, d->lpos.p, d->lmass.p, ltype, d->box));
    e->tree.force_internal_above = d->La;
    try {
        engine_tree_build_on(e, 63, st);
    }
    catch(...) {
        e->tree.force_internal_above = 0;
        throw;
    }
    e->tree.force_internal_above = 0;
}

// the deferred checks of tree_finish; call after a synchronisation of the engine's stream
void tree_checks(mpg_dist *d)
{
    if(!d->chk_pending)
        return;
    d->chk_pending = false;
    const unsigned *ef = (const unsigned *)&d->chk.p[1];
    MPG_CHECK(ef[0] == 0, "mpg_dist: a cell above the decomposition level holds <= 8 particles in all (use a coarser level La)");
    MPG_CHECK(ef[1] == 0, "domain decomposition: a cell above the decomposition level holds <= 8 local particles (use a coarser level)");
    MPG_CHECK((int64_t)d->chk.p[0] == d->ntarg, "mpg_dist: own particles missing from the local tree");
}

void tree_finish(mpg_dist *d, int64_t n_own, int64_t nl)
{
    mpg_engine *e = d->eng;
    hipStream_t st = e->stream;
    global_top(d, n_own);
    // own particles in tree order: the walk's targets
    d->targets.reserve((size_t)nl + 1);
    d->scount.reserve(4);
    d->ntarg = 0;
    d->n_own_tree = n_own;
    if(nl > 0) {
        with_tmp(d, [&](void *tmp, size_t &tb) {
            return rocprim::select(tmp, tb, e->tree.idx_b.p, (int *)d->targets.p, d->scount.p, (size_t)e->tree.npart, IsOwn{(int)n_own}, st);
        });
        // every own live particle is in the local tree, so the number of targets is known; the count the selection found and the flags of
        // the global top travel to pinned memory behind it and are checked at the next point the host waits anyway (tree_checks)
        d->ntarg = n_own - (d->skip_for(n_own) ? d->n_skip : 0);
        d->chk.reserve(4);
        d->chk.p[0] = ~0ull;
        MPG_HIP(hipMemcpyAsync(&d->chk.p[0], d->scount.p, sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
    }
    else {
        d->chk.reserve(4);
        d->chk.p[0] = 0;
    }
    d->chk.p[1] = 0;
    MPG_HIP(hipMemcpyAsync(&d->chk.p[1], d->err.p + 1, 2 * sizeof(unsigned), hipMemcpyDeviceToHost, st));
    d->chk_pending = true;
    d->grav_tree_valid = true;
}

extern "C" {

int mpg_dist_dev_gravpm_force(mpg_dist *d, int64_t n_own, const double *d_pos, const float *d_mass, double *d_gravpm, double *d_potential)
{
    API_BEGIN
    MPG_CHECK(d && d_gravpm && (n_own == 0 || (d_pos && d_mass)), "null argument");
    pm_begin(d, n_own, d_gravpm);
    sync(d);
    const double t0 = now_ms();
    pm_step(d, n_own, d_pos, d_mass, d_gravpm, d_potential);
    sync(d);
    d->times[0] = now_ms() - t0;
    API_END
}

int mpg_dist_dev_force_tree_build(mpg_dist *d, int64_t n_own, const double *d_pos, const float *d_mass)
{
    API_BEGIN
    MPG_CHECK(d && (n_own == 0 || (d_pos && d_mass)), "null argument");
    mpg_engine *e = particles_begin(d, n_own);
    sync(d);
    const double t1 = now_ms();
    // ---- ghosts, local tree, global top
    const int64_t nl = import_ghosts(d, n_own, d_pos, d_mass);
    sync(d);
    const double t2 = now_ms();
    d->times[1] = t2 - t1;
    tree_build_local(d, n_own, nl, e->stream);
    tree_finish(d, n_own, nl);
    sync(d); // (this entry point stands alone - the SPH loops and FOF follow it as well as the walk: its checks are made here)
    tree_checks(d);
    d->times[2] = now_ms() - t2;
    d->times[4] = 0;
    API_END
}

int mpg_dist_dev_grav_short_tree(mpg_dist *d, const double *d_oldacc, const double *d_prev_accel, const double *d_gravpm, double *d_accel,
                                 double *d_potential, double rho0)
{
    return mpg_dist_dev_grav_short_tree_active(d, nullptr, 0, d_oldacc, d_prev_accel, d_gravpm, d_accel, d_potential, rho0);
}

int mpg_dist_dev_grav_short_tree_active(mpg_dist *d, const int *d_active, int64_t nactive, const double *d_oldacc, const double *d_prev_accel,
                                        const double *d_gravpm, double *d_accel, double *d_potential, double rho0)
{
    API_BEGIN
    MPG_CHECK(d && d_accel, "null argument");
    MPG_CHECK(d->n_own_tree >= 0, "mpg_dist_dev_grav_short_tree: mpg_dist_dev_force_tree_build first");
    MPG_CHECK(d->grav_tree_valid, "mpg_dist_dev_grav_short_tree: the local tree was replaced since mpg_dist_dev_force_tree_build (the density loop "
                                  "builds a gas tree, FOF a tree of the primary types): build the gravity tree again");
    MPG_CHECK(nactive >= 0 && nactive <= d->n_own_tree, "mpg_dist_dev_grav_short_tree_active: bad number of active particles");
    mpg_engine *e = d->eng;
    MPG_HIP(hipSetDevice(e->device));
    sync(d);
    tree_checks(d);
    const double t3 = now_ms();
    // the walk's targets: the own particles in tree order, or those of them the caller lists as active (ActiveParticle of the
    // sub-steps, run.c:392-470: the tree holds every particle, a subset is walked)
    const int *targets = d->targets.p;
    int64_t ntarg = d->ntarg;
    if(d_active) {
        hipStream_t st = e->stream;
        ntarg = 0;
        if(nactive > 0 && d->ntarg > 0) {
            d->act_targets.reserve((size_t)d->n_own_tree + 1);
            flag_active_list(d, d_active, nactive, d->n_own_tree);
            with_tmp(d, [&](void *tmp, size_t &tb) {
                return rocprim::select(tmp, tb, d->targets.p, d->act_targets.p, d->scount.p, (size_t)d->ntarg, IsFlagged{d->actflag.p}, st);
            });
            unsigned long long c = 0;
            unsigned bad = 0;
            MPG_HIP(hipMemcpyAsync(&c, d->scount.p, sizeof(c), hipMemcpyDeviceToHost, st));
            MPG_HIP(hipMemcpyAsync(&bad, d->err.p, sizeof(bad), hipMemcpyDeviceToHost, st));
            sync(d);
            MPG_CHECK(bad == 0, "mpg_dist_dev_grav_short_tree_active: an active index is not an own particle");
            // (garbage on the active list is skipped in place, treewalk.c:234: it is not in the tree, hence not among the targets.  The
            // garbage entries ON the list are counted, so that a duplicate cannot hide behind them: ADVICE round 4)
            int64_t ngarb = 0;
            if(d->skip_for(d->n_own_tree)) {
                MPG_HIP(hipMemsetAsync(d->scount.p, 0, sizeof(unsigned long long), st));
                hipLaunchKernelGGL(k_count_listed, dim3(nblk(nactive)), dim3(256), 0, st, nactive, d_active, d->d_skip, d->scount.p);
                unsigned long long g = 0;
                MPG_HIP(hipMemcpyAsync(&g, d->scount.p, sizeof(g), hipMemcpyDeviceToHost, st));
                sync(d);
                ngarb = (int64_t)g;
            }
            MPG_CHECK((int64_t)c + ngarb == nactive, "mpg_dist_dev_grav_short_tree_active: the active list holds duplicates");
            ntarg = (int64_t)c;
        }
        targets = d->act_targets.p;
    }
    if(ntarg > 0) {
        d->cost.reserve((size_t)d->n_own_tree + 1);
        MPG_HIP(hipMemsetAsync(d->cost.p, 0, (size_t)d->n_own_tree * sizeof(float), e->stream));
        float *keep = e->d_walk_cost;
        const int keep_variant = e->walk_variant;
        e->d_walk_cost = d->cost.p;
        if(e->walk_variant == 0) // the two-kernel walk whatever the target count: it is the one that records the work per target
            e->walk_variant = 6;
        const int rc = mpg_dev_grav_short_tree(e, d_oldacc, d_prev_accel, d_gravpm, targets, ntarg, d_accel, d_potential, rho0);
        e->d_walk_cost = keep;
        e->walk_variant = keep_variant;
        MPG_CHECK(rc == 0, mpg_last_error());
    }
    sync(d);
    d->times[3] = now_ms() - t3;
    API_END
}

int mpg_dist_gravity_step(mpg_dist *d, int64_t n_own, const double *d_pos, const float *d_mass, const double *d_oldacc,
                          const double *d_prev_accel, double *d_accel, double *d_gravpm, double *d_potential, double rho0)
{
    if(d && d_potential && n_own > 0) // (readout_potential accumulates; the walk then assigns the tree's, gravshort.h:94-95)
        if(hipMemsetAsync(d_potential, 0, (size_t)n_own * sizeof(double), d->eng->stream) != hipSuccess)
            return 1;
    static const bool no_overlap = getenv("MPG_DIST_NO_OVERLAP") != nullptr;
    if(no_overlap) {
        if(int rc = mpg_dist_dev_gravpm_force(d, n_own, d_pos, d_mass, d_gravpm, d_potential))
            return rc;
        if(int rc = mpg_dist_dev_force_tree_build(d, n_own, d_pos, d_mass))
            return rc;
        return mpg_dist_dev_grav_short_tree(d, d_oldacc, d_prev_accel, d_gravpm, d_accel, d_potential, rho0);
    }
    // The local tree does not depend on the PM force (run.c:522-546 runs them one after the other; both only read the positions): the
    // ghosts are imported first, then the tree of own + ghost particles is built by a second host thread on a second stream WHILE this
    // thread runs the PM step - whose phases end in collectives the host waits for, so the tree's kernels fill the gaps (one rank of a
    // 256^3-per-GPU run: 5 ms of tree build beside 18 ms of PM).  Every collective stays on this thread, in the same order on every rank.
    {
        API_BEGIN
        MPG_CHECK(d && d_gravpm && d_accel && (n_own == 0 || (d_pos && d_mass)), "null argument");
        mpg_engine *e = pm_begin(d, n_own, d_gravpm);
        sync(d);
        const double t0 = now_ms();
        const int64_t nl = import_ghosts(d, n_own, d_pos, d_mass);
        sync(d); // (d->lpos / d->lmass are complete: the other stream may read them)
        const double t1 = now_ms();
        d->times[1] = t1 - t0;
        if(!d->tree_stream)
            MPG_HIP(hipStreamCreateWithFlags(&d->tree_stream, hipStreamNonBlocking));
        std::string werr;
        double t_tree = 0;
        std::thread worker([&]() {
            try {
                MPG_HIP(hipSetDevice(e->device));
                const double ta = now_ms();
                tree_build_local(d, n_own, nl, d->tree_stream);
                MPG_HIP(hipStreamSynchronize(d->tree_stream));
                t_tree = now_ms() - ta;
            }
            catch(const std::exception &ex) {
                werr = ex.what();
                if(werr.empty())
                    werr = "tree build failed";
            }
        });
        std::string perr;
        try {
            pm_step(d, n_own, d_pos, d_mass, d_gravpm, d_potential);
            sync(d);
        }
        catch(const std::exception &ex) {
            perr = ex.what();
        }
        worker.join();
        // (both failures are reported; ADVICE round 3.  The invariant the two threads rely on: tree_build_local touches the engine's tree,
        // its particle binding (eng->n, d_pos, tree_mask) and d->tree_stream only, pm_step touches the mesh, the slab buffers, the
        // communicator and eng->stream only, and neither reads what the other writes before the join above.)
        MPG_CHECK(perr.empty() && werr.empty(), perr.empty() ? werr : (werr.empty() ? perr : perr + " | and the tree build beside it: " + werr));
        const double t2 = now_ms();
        d->times[0] = t2 - t1; // PM with the tree build beside it
        d->times[4] = t_tree;  // ... of which the tree build took this long on its stream
        tree_finish(d, n_own, nl);
        d->times[2] = now_ms() - t2;
        API_END_NORETURN
    }
    return mpg_dist_dev_grav_short_tree(d, d_oldacc, d_prev_accel, d_gravpm, d_accel, d_potential, rho0);
}

const float *mpg_dist_walk_cost(mpg_dist *d) { return d ? d->cost.p : nullptr; }

/* measure_power_spectrum + powerspectrum_sum over the ranks (gravpm.c:110-118, powerspectrum.c:55-91): every rank binned the k_y rows of
 * its slab during mpg_dist_(dev_)gravpm_force; the raw sums (Power, k, Norm, mode counts) are all-reduced as the reference's
 * MPI_Allreduce does, then normalised.  Collective; every rank gets the spectrum. */
int mpg_dist_gravpm_get_powerspectrum(mpg_dist *d, double BoxSize_in_MPC, double *kk, double *Power, int64_t *Nmodes, int *nonzero)
{
    API_BEGIN
    MPG_CHECK(d && kk && Power && Nmodes && nonzero, "null argument");
    mpg_engine *e = d->eng;
    MPG_CHECK(e->pm.nmesh > 0 && e->pm.ps_valid, "power spectrum: no PM step has been run with the measurement on");
    MPG_HIP(hipSetDevice(e->device));
    const size_t nb = (size_t)e->pm.nmesh;
    std::vector<double> acc(2 * nb + 1);
    std::vector<int64_t> modes(nb);
    MPG_HIP(hipMemcpyAsync(acc.data(), e->pm.ps_acc.p, (2 * nb + 1) * sizeof(double), hipMemcpyDeviceToHost, e->stream));
    MPG_HIP(hipMemcpyAsync(modes.data(), e->pm.ps_modes.p, nb * sizeof(int64_t), hipMemcpyDeviceToHost, e->stream));
    sync(d);
    allreduce_host_f64(d, acc.data(), (int64_t)(2 * nb + 1), 0);
    allreduce_i64(d, modes.data(), (int64_t)nb, 0);
    MPG_CALL(mpg_powerspectrum_sum((int)nb, acc.data(), modes.data(), BoxSize_in_MPC, kk, Power, Nmodes, nonzero));
    API_END
}

} // extern "C"

/* ---- hierarchical gravity on several ranks: the tree of the ACTIVE particles only (force_tree_active_moments, forcetree.c:129-148;
 * hierarchical_gravity_accelerations of timestep.c) -------------------------------------------------------------------------------
 * The active sets of the short time bins are sparse: the tree of such a set has cells with <= 8 particles far above any domain level,
 * which the all-reduced top of mpg_dist_dev_force_tree_build excludes.  They are also small.  So every rank receives the whole active
 * set (28 bytes per particle, one all-gather), builds ITS tree itself - the tree one GPU would build - and walks its own members. */
extern "C" int mpg_dist_dev_grav_short_tree_active_tree(mpg_dist *d, int64_t n_act, const double *d_pos, const float *d_mass, const double *d_oldacc,
                                                        double *d_accel, double *d_potential, double rho0)
{
    API_BEGIN
    MPG_CHECK(d && (n_act == 0 || (d_pos && d_mass && d_accel)), "null argument");
    MPG_CHECK(d->box > 0, "mpg_dist: mpg_dist_set_domain first (the box size)");
    mpg_engine *e = d->eng;
    MPG_HIP(hipSetDevice(e->device));
    hipStream_t st = e->stream;
    // this rank's active particles as one host block: [n][3] positions, then [n] masses
    std::vector<char> blk(sizeof(int64_t) + (size_t)n_act * 28);
    memcpy(blk.data(), &n_act, sizeof(int64_t));
    if(n_act > 0) {
        MPG_HIP(hipMemcpyAsync(blk.data() + 8, d_pos, (size_t)n_act * 24, hipMemcpyDeviceToHost, st));
        MPG_HIP(hipMemcpyAsync(blk.data() + 8 + (size_t)n_act * 24, d_mass, (size_t)n_act * 4, hipMemcpyDeviceToHost, st));
    }
    sync(d);
    std::vector<std::vector<char>> all;
    allgather_host(d, blk.data(), (int64_t)blk.size(), all);
    int64_t ntot = 0, off = 0;
    std::vector<int64_t> cnt(d->nt);
    for(int r = 0; r < d->nt; r++) {
        memcpy(&cnt[r], all[r].data(), sizeof(int64_t));
        if(r < d->me)
            off += cnt[r];
        ntot += cnt[r];
    }
    MPG_CHECK(ntot < (1ll << 27), "mpg_dist_dev_grav_short_tree_active_tree: the active set is not small (use the tree of all particles)");
    d->n_own_tree = -1; // the local tree of mpg_dist_dev_force_tree_build is gone after this call
    d->sph_n_own = -1;
    if(ntot == 0)
        return 0;
    d->lpos.reserve(3 * (size_t)ntot + 3);
    d->lmass.reserve((size_t)ntot + 1);
    int64_t at = 0;
    for(int r = 0; r < d->nt; r++) {
        if(cnt[r] > 0) {
            MPG_HIP(hipMemcpyAsync(d->lpos.p + 3 * at, all[r].data() + 8, (size_t)cnt[r] * 24, hipMemcpyHostToDevice, st));
            MPG_HIP(hipMemcpyAsync(d->lmass.p + at, all[r].data() + 8 + (size_t)cnt[r] * 24, (size_t)cnt[r] * 4, hipMemcpyHostToDevice, st));
        }
        at += cnt[r];
    }
    sync(d); // (`all` is read by the copies)
    d->grav_tree_valid = false;
    MPG_CALL(mpg_dev_bind_particles(e, ntot, d->lpos.p, d->lmass.p, nullptr, d->box));
    MPG_CALL(mpg_dev_force_tree_build(e, 63));
    e->full_particle_tree = false; // (force_tree_active_moments, forcetree.c:129-148: P[].Potential and FullTreeGravAccel are not this walk's)
    if(n_act == 0)
        return 0;
    // own members in tree order; inputs / outputs over the whole set, the own range copied in and out
    d->targets.reserve((size_t)ntot + 1);
    d->scount.reserve(4);
    const InRange mine{(int)off, (int)(off + n_act)};
    with_tmp(d, [&](void *tmp, size_t &tb) {
        return rocprim::select(tmp, tb, e->tree.idx_b.p, (int *)d->targets.p, d->scount.p, (size_t)e->tree.npart, mine, st);
    });
    d->o_prev.reserve((size_t)ntot + 1);
    d->o_acc.reserve(3 * (size_t)ntot + 3);
    d->o_pot.reserve((size_t)ntot + 1);
    MPG_HIP(hipMemsetAsync(d->o_prev.p, 0, (size_t)ntot * sizeof(double), st));
    if(d_oldacc)
        MPG_HIP(hipMemcpyAsync(d->o_prev.p + off, d_oldacc, (size_t)n_act * sizeof(double), hipMemcpyDeviceToDevice, st));
    (void)d_potential; // (left alone: the tree does not hold every particle, gravshort.h:57-67)
    MPG_CALL(mpg_dev_grav_short_tree(e, d->o_prev.p, nullptr, nullptr, d->targets.p, n_act, d->o_acc.p, nullptr, rho0));
    MPG_HIP(hipMemcpyAsync(d_accel, d->o_acc.p + 3 * off, (size_t)n_act * 24, hipMemcpyDeviceToDevice, st));
    sync(d);
    d->o_n = -1; // (the staging columns of the host drop-in calls were reused)
    API_END
}

/* ---- potential planes over the ranks (write_plane, plane.c:572-683; the kernels are planes.hip's).  Every rank counts its own rows; the
 * counters are widened to 64-bit integers and summed with the communicator's allreduce, as are the active-particle number and the
 * particles per plane.  The reference reduces the finished potentials (plane.c:654); the solve is linear, so summing the integer counts
 * first gives the same plane with one solve instead of one per rank, and every rank holds the result.  The neutrino correction would need
 * the slab form of the mesh pass and is refused - before any collective, so that every rank returns.  The planes of a batch (what the
 * counter budget holds) are agreed on as the smallest number any rank can hold, and a rank-local refusal of the counting pass (a
 * position that cannot be wrapped, 2^32 active rows) travels with a MAX all-reduce, so every rank makes the same collectives and
 * returns the same error. */
namespace {
void planes_sum_device(void *ctx, int64_t *d_v, int64_t count)
{
    mpg_dist *d = (mpg_dist *)ctx;
    MPG_CHECK(d->comm.allreduce, "mpg_comm: allreduce callback missing");
    hipStream_t st = d->eng->stream;
    if(d->comm.device_buffers) {
        comm_ready(d);
        cb(d->comm.allreduce(d->comm.ctx, d_v, count, 1, 0, 1), "allreduce");
        return;
    }
    std::vector<int64_t> h((size_t)count);
    MPG_HIP(hipMemcpyAsync(h.data(), d_v, (size_t)count * sizeof(int64_t), hipMemcpyDeviceToHost, st));
    sync(d);
    cb(d->comm.allreduce(d->comm.ctx, h.data(), count, 1, 0, 0), "allreduce");
    MPG_HIP(hipMemcpyAsync(d_v, h.data(), (size_t)count * sizeof(int64_t), hipMemcpyHostToDevice, st));
    sync(d);
}
void planes_sum_host(void *ctx, int64_t *v, int64_t count) { allreduce_i64((mpg_dist *)ctx, v, count, 0); }
void planes_max_host(void *ctx, int64_t *v, int64_t count) { allreduce_i64((mpg_dist *)ctx, v, count, 1); }
} // namespace

extern "C" int mpg_dist_potential_planes(mpg_dist *d, int64_t n_own, const double *d_pos, const float *d_mass, const uint8_t *d_type,
                                         const unsigned char *d_flags, double BoxSize, const mpg_plane_params *params, double *d_planes,
                                         int64_t *npart)
{
    API_BEGIN
    MPG_CHECK(d && params, "null argument");
    MPG_CHECK(n_own >= 0 && (n_own == 0 || d_pos), "mpg_dist_potential_planes: null positions");
    MPG_CHECK(BoxSize > 0, "mpg_dist_potential_planes: BoxSize must be positive");
    MPG_CHECK(!(params->fn && d->nt > 1), "potential planes: the massive-neutrino correction on several ranks is not implemented");
    mpg_engine *e = d->eng;
    MPG_HIP(hipSetDevice(e->device));
    e->host_join();
    e->n = n_own;
    e->d_pos = d_pos;
    e->d_mass = d_mass;
    e->d_type = d_type;
    e->box = BoxSize;
    e->pm_queued = false;
    const PlaneReduce red{d, d->nt, planes_sum_device, planes_sum_host, planes_max_host};
    planes_run(e, params, d_flags, d_planes, npart, d->nt > 1 ? &red : nullptr);
    API_END
}
