// dist.hip -- the force step on several ranks (one process per GPU) behind the caller's communicator: mpg_dist_* of
// include/mpgadget_hip.h.
//
// The reference's gravpm_force / force_tree_full / grav_short_tree are collective over MPI_COMM_WORLD: particles live on the
// rank that owns their Peano-Hilbert TopLeaf (domain.c:153-258), petapm ships region meshes to 2-D pencils and back
// (petapm.c:584-885), the force tree hangs local sub-trees under a replicated top-tree whose remote leaves are pseudo nodes
// (forcetree.c:654-723, 1145-1284) and the walk exports targets to the owners of the pseudo nodes they open
// (treewalk.c:325-793).  Here, MI355X-first (288 GB per GPU, xGMI point-to-point links):
//
//   PM    {Pos, Mass} of every particle (32 B) goes to the rank(s) owning the x-planes its CIC cloud touches - at Nmesh = 2 N^(1/3)
//         a particle is an eighth of the mesh cells it deposits on, so shipping particles beats shipping region meshes -, the
//         slab solver of pm.hip runs on what arrived (two all-to-all transposes, five neighbour planes), and {GravPM, Potential}
//         (32 B) returns along the same lists.
//   tree  a rank imports the particles of every level-La tree cell within `margin` (>= Rcut) of its TopLeaves: WHOLE cells, so
//         that every node at level >= La a target can reach is complete and identical to the global tree's; cells that are not
//         imported lie more than Rcut from every own target, where the walk discards on geometry alone.  Nodes above level La
//         hold remote particles: they are kept internal (TreeBuilder::force_internal_above) and their moments are the
//         all-reduced sums of the ranks' own particles - the counterpart of the replicated top-tree.  Ghost import replaces the
//         target export: same interaction sets, no return trip, and the walk kernels are the single-GPU ones.
//
// The library links neither MPI nor RCCL; the collectives are the caller's (mpg_comm).  All ordering is on the engine's stream;
// a callback is entered with the stream idle.
//
// This file is the core of the layer: the object behind the handle, the communicator wrappers, the plans (who gets which of my rows) and
// the row exchange along them.  The subjects built on it: dist_gravity.hip, dist_sph.hip, dist_domain.hip, dist_fof.hip, dist_host.hip;
// what they share is declared in dist_internal.h.
#include "dist_internal.h"
#include "peano_tables.h"
#include <algorithm>
#include <chrono>
#include <rocprim/rocprim.hpp>

namespace {

constexpr int PH_BITS = 21;
const unsigned char H_SUBPIX[MPG_PEANO_NSTATES][8] = MPG_PEANO_SUBPIX;
const unsigned char H_NEXT[MPG_PEANO_NSTATES][8] = MPG_PEANO_NEXT;

__global__ void __launch_bounds__(256) k_count_nonzero(int64_t n, const unsigned char *__restrict__ b, unsigned long long *__restrict__ out)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const unsigned long long m = __ballot(i < n && b[i] != 0);
    if((threadIdx.x & 63) == 0 && m)
        atomicAdd(out, (unsigned long long)__popcll(m));
}

// ---- send lists for all destinations in two passes (a stable multi-way split).  A row may go to several destinations (one bit per
// rank in its mask); within a destination the rows keep their order, so the lists - and with them the order of the ghosts in the
// receivers' arrays - do not depend on scheduling.  Tiles of 1024 consecutive rows: pass 1 counts the rows of every tile per
// destination (tilecnt[d][tile]: an exclusive scan over that array, destinations back to back, IS the start of (d, tile) in the
// concatenated lists) and adds the totals up (one global atomic per tile and destination: per WAVE and destination on the same 8
// words it took 1.76 ms for 16.8 M rows); pass 2 ranks the rows of a tile by ballots and wave totals in LDS and writes the indices.
// (Round 2: one rocprim::select pass over all rows PER DESTINATION.)
constexpr int SPLIT_TILE = 1024;
__global__ void __launch_bounds__(256) k_split_count(int64_t n, const unsigned long long *__restrict__ mask, int nt, int64_t ntiles,
                                                     unsigned *__restrict__ tilecnt, unsigned long long *__restrict__ counts)
{
    __shared__ unsigned s_cnt[64];
    if(threadIdx.x < 64)
        s_cnt[threadIdx.x] = 0u;
    __syncthreads();
    const int64_t base = (int64_t)blockIdx.x * SPLIT_TILE;
    for(int j = 0; j < SPLIT_TILE / 256; j++) {
        const int64_t i = base + j * 256 + threadIdx.x;
        const unsigned long long m = i < n ? mask[i] : 0ull;
        for(int d = 0; d < nt; d++) {
            const unsigned long long b = __builtin_amdgcn_ballot_w64((m >> d) & 1ull);
            if(b && (threadIdx.x & 63) == 0)
                atomicAdd(&s_cnt[d], (unsigned)__popcll(b));
        }
    }
    __syncthreads();
    if(threadIdx.x < nt) {
        const unsigned c = s_cnt[threadIdx.x];
        tilecnt[(int64_t)threadIdx.x * ntiles + blockIdx.x] = c;
        if(c)
            atomicAdd(&counts[threadIdx.x], (unsigned long long)c);
    }
}

__global__ void __launch_bounds__(256) k_split_scatter(int64_t n, const unsigned long long *__restrict__ mask, int nt, int64_t ntiles,
                                                       const unsigned *__restrict__ tilepos, int *__restrict__ idx)
{
    __shared__ unsigned s_base[64], s_w[4][64];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    if(threadIdx.x < nt)
        s_base[threadIdx.x] = tilepos[(int64_t)threadIdx.x * ntiles + blockIdx.x];
    const int64_t base = (int64_t)blockIdx.x * SPLIT_TILE;
    for(int j = 0; j < SPLIT_TILE / 256; j++) {
        const int64_t i = base + j * 256 + threadIdx.x;
        const unsigned long long m = i < n ? mask[i] : 0ull;
        for(int d = 0; d < nt; d++) {
            const unsigned long long b = __builtin_amdgcn_ballot_w64((m >> d) & 1ull);
            if(lane == 0)
                s_w[wave][d] = (unsigned)__popcll(b);
        }
        __syncthreads();
        for(int d = 0; d < nt; d++) {
            const unsigned long long b = __builtin_amdgcn_ballot_w64((m >> d) & 1ull);
            if((m >> d) & 1ull) {
                unsigned pos = s_base[d] + (unsigned)__popcll(b & ((1ull << lane) - 1ull));
                for(int w = 0; w < wave; w++)
                    pos += s_w[w][d];
                idx[pos] = (int)i;
            }
        }
        __syncthreads();
        if(threadIdx.x < nt)
            s_base[threadIdx.x] += s_w[0][threadIdx.x] + s_w[1][threadIdx.x] + s_w[2][threadIdx.x] + s_w[3][threadIdx.x];
        __syncthreads();
    }
}

// flag[list[i]] = 1; an index outside [0, n) raises *err
__global__ void __launch_bounds__(256) k_flag_list(int64_t m, const int *__restrict__ list, int n, uint8_t *__restrict__ flag,
                                                   unsigned *__restrict__ err)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if(i >= m)
        return;
    const int j = list[i];
    if(j < 0 || j >= n)
        atomicOr(err, 1u);
    else
        flag[j] = 1;
}

} // namespace

double now_ms()
{
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

void sync(mpg_dist *d) { MPG_HIP(hipStreamSynchronize(d->eng->stream)); }

void cb(int rc, const char *what) { MPG_CHECK(rc == 0, std::string("mpg_comm callback failed: ") + what); }

// a stream-ordered communicator follows the engine's stream (mpg_use_stream may have replaced it since mpg_dist_create); a blocking one
// works outside the stream: what it sends must be complete
void comm_ready(mpg_dist *d)
{
    if(!d->stream_ordered)
        sync(d);
    else if(d->bound_stream != d->eng->stream) {
        cb(d->comm.bind_stream(d->comm.ctx, (void *)d->eng->stream), "bind_stream");
        d->bound_stream = d->eng->stream;
    }
}

// alltoallv of bytes between device buffers (staged through pinned host memory unless the communicator takes device pointers)
void a2av(mpg_dist *d, const void *dsend, const std::vector<int64_t> &sb, const std::vector<int64_t> &sd, void *drecv,
          const std::vector<int64_t> &rb, const std::vector<int64_t> &rd, int64_t stot, int64_t rtot)
{
    hipStream_t st = d->eng->stream;
    d->stats[4] += stot;
    if(d->nt == 1 && !d->comm.alltoallv) {
        if(stot > 0)
            MPG_HIP(hipMemcpyAsync(drecv, dsend, (size_t)stot, hipMemcpyDeviceToDevice, st));
        return;
    }
    MPG_CHECK(d->comm.alltoallv, "mpg_comm: alltoallv callback missing");
    if(d->comm.device_buffers) {
        comm_ready(d);
        cb(d->comm.alltoallv(d->comm.ctx, dsend, sb.data(), sd.data(), drecv, rb.data(), rd.data(), 1), "alltoallv");
        return;
    }
    d->hsend.reserve((size_t)stot + 16);
    d->hrecv.reserve((size_t)rtot + 16);
    if(stot > 0)
        MPG_HIP(hipMemcpyAsync(d->hsend.p, dsend, (size_t)stot, hipMemcpyDeviceToHost, st));
    sync(d);
    cb(d->comm.alltoallv(d->comm.ctx, d->hsend.p, sb.data(), sd.data(), d->hrecv.p, rb.data(), rd.data(), 0), "alltoallv");
    if(rtot > 0)
        MPG_HIP(hipMemcpyAsync(drecv, d->hrecv.p, (size_t)rtot, hipMemcpyHostToDevice, st));
    sync(d); // (hrecv is reused by the next exchange)
}

// uniform all-to-all of `bytes_per_peer` per rank pair (the transposes of the slab PM)
void a2a_uniform(mpg_dist *d, const void *dsend, void *drecv, int64_t bytes_per_peer)
{
    std::vector<int64_t> b((size_t)d->nt, bytes_per_peer), dsp((size_t)d->nt);
    for(int r = 0; r < d->nt; r++)
        dsp[r] = (int64_t)r * bytes_per_peer;
    a2av(d, dsend, b, dsp, drecv, b, dsp, bytes_per_peer * d->nt, bytes_per_peer * d->nt);
    d->stats[4] -= bytes_per_peer * d->nt;
    d->stats[5] += bytes_per_peer * d->nt;
}

void allreduce_i64(mpg_dist *d, int64_t *v, int64_t n, int op)
{
    if(d->nt == 1 && !d->comm.allreduce)
        return;
    MPG_CHECK(d->comm.allreduce, "mpg_comm: allreduce callback missing");
    cb(d->comm.allreduce(d->comm.ctx, v, n, 1, op, 0), "allreduce");
}

void allreduce_host_f64(mpg_dist *d, double *h, int64_t n, int op)
{
    if(d->nt == 1 && !d->comm.allreduce)
        return;
    MPG_CHECK(d->comm.allreduce, "mpg_comm: allreduce callback missing");
    cb(d->comm.allreduce(d->comm.ctx, h, n, 0, op, 0), "allreduce");
}

bool any_rank(mpg_dist *d, bool f)
{
    int64_t v = f ? 1 : 0;
    allreduce_i64(d, &v, 1, 0);
    return v > 0;
}

// every rank's block of host bytes (padded to 8): out[r] = the block of rank r
void allgather_host(mpg_dist *d, const void *buf, int64_t nbytes, std::vector<std::vector<char>> &out)
{
    const int nt = d->nt;
    out.assign(nt, {});
    if(nt == 1) {
        out[0].assign((const char *)buf, (const char *)buf + nbytes);
        return;
    }
    const int64_t pad = (nbytes + 7) / 8 * 8;
    std::vector<int64_t> sc(nt, pad), rc(nt, 0), sd(nt, 0), rd(nt + 1, 0);
    cb(d->comm.alltoall_i64(d->comm.ctx, sc.data(), rc.data()), "alltoall_i64");
    for(int r = 0; r < nt; r++)
        rd[r + 1] = rd[r] + rc[r];
    std::vector<char> sb((size_t)pad + 8, 0), rb((size_t)rd[nt] + 8);
    memcpy(sb.data(), buf, (size_t)nbytes);
    std::vector<int64_t> rdv(rd.begin(), rd.begin() + nt);
    cb(d->comm.alltoallv(d->comm.ctx, sb.data(), sc.data(), sd.data(), rb.data(), rc.data(), rdv.data(), 0), "alltoallv");
    for(int r = 0; r < nt; r++)
        out[r].assign(rb.begin() + rd[r], rb.begin() + rd[r] + rc[r]); // (padded: the receiver knows the true sizes from the data)
}

// send lists from per-particle destination masks; the counts travel through alltoall_i64
void build_plan(mpg_dist *d, Plan &pl, int64_t n, const unsigned long long *mask)
{
    hipStream_t st = d->eng->stream;
    const int nt = d->nt;
    d->cnt.reserve(64);
    MPG_HIP(hipMemsetAsync(d->cnt.p, 0, 64 * sizeof(unsigned long long), st));
    const int64_t ntiles = (n + SPLIT_TILE - 1) / SPLIT_TILE;
    d->tilecnt.reserve((size_t)nt * ntiles + 1);
    d->tilepos.reserve((size_t)nt * ntiles + 1);
    if(n > 0)
        hipLaunchKernelGGL(k_split_count, dim3((unsigned)ntiles), dim3(256), 0, st, n, mask, nt, ntiles, d->tilecnt.p, d->cnt.p);
    unsigned long long hc[64];
    MPG_HIP(hipMemcpyAsync(hc, d->cnt.p, 64 * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
    if(n > 0) // (queued behind the count pass, before the host looks at the totals)
        with_tmp(d, [&](void *tmp, size_t &tb) {
            return rocprim::exclusive_scan(tmp, tb, d->tilecnt.p, d->tilepos.p, 0u, (size_t)nt * ntiles, rocprim::plus<unsigned>(), st);
        });
    sync(d);
    pl.scnt.assign(nt, 0);
    pl.sdsp.assign(nt + 1, 0);
    for(int r = 0; r < nt; r++) {
        pl.scnt[r] = (int64_t)hc[r];
        pl.sdsp[r + 1] = pl.sdsp[r] + pl.scnt[r];
    }
    pl.nsend = pl.sdsp[nt];
    MPG_CHECK(pl.nsend < (1ll << 31), "mpg_dist: more than 2^31 rows in one exchange");
    pl.idx.reserve((size_t)pl.nsend + 1);
    pl.d_sdsp.reserve((size_t)nt + 1);
    pl.h_sdsp.reserve((size_t)nt + 1); // (pinned, owned by the plan: the copy needs no wait; the next build_plan of this plan starts with one)
    for(int r = 0; r <= nt; r++)
        pl.h_sdsp.p[r] = (long long)pl.sdsp[r];
    MPG_HIP(hipMemcpyAsync(pl.d_sdsp.p, pl.h_sdsp.p, (nt + 1) * sizeof(long long), hipMemcpyHostToDevice, st));
    if(n > 0 && pl.nsend > 0)
        hipLaunchKernelGGL(k_split_scatter, dim3((unsigned)ntiles), dim3(256), 0, st, n, mask, nt, ntiles, d->tilepos.p, pl.idx.p);
    pl.rcnt.assign(nt, 0);
    if(nt == 1 && !d->comm.alltoall_i64)
        pl.rcnt[0] = pl.scnt[0];
    else {
        MPG_CHECK(d->comm.alltoall_i64, "mpg_comm: alltoall_i64 callback missing");
        cb(d->comm.alltoall_i64(d->comm.ctx, pl.scnt.data(), pl.rcnt.data()), "alltoall_i64");
    }
    pl.rdsp.assign(nt + 1, 0);
    for(int r = 0; r < nt; r++)
        pl.rdsp[r + 1] = pl.rdsp[r] + pl.rcnt[r];
    pl.nrecv = pl.rdsp[nt];
}

// rows of `rb_` bytes each along a plan; reverse: the answers travel back (what I received, I return; what I sent, I get back)
void exchange_rows(mpg_dist *d, const Plan &pl, const void *dsend, void *drecv, bool reverse, int64_t rb_)
{
    const int nt = d->nt;
    std::vector<int64_t> sb(nt), sd(nt), rb(nt), rd(nt);
    for(int r = 0; r < nt; r++) {
        sb[r] = rb_ * (reverse ? pl.rcnt[r] : pl.scnt[r]);
        sd[r] = rb_ * (reverse ? pl.rdsp[r] : pl.sdsp[r]);
        rb[r] = rb_ * (reverse ? pl.scnt[r] : pl.rcnt[r]);
        rd[r] = rb_ * (reverse ? pl.sdsp[r] : pl.rdsp[r]);
    }
    a2av(d, dsend, sb, sd, drecv, rb, rd, rb_ * (reverse ? pl.nrecv : pl.nsend), rb_ * (reverse ? pl.nsend : pl.nrecv));
}

void flag_active_list(mpg_dist *d, const int *d_list, int64_t m, int64_t n)
{
    hipStream_t st = d->eng->stream;
    d->actflag.reserve((size_t)n + 1);
    d->err.reserve(4);
    MPG_HIP(hipMemsetAsync(d->err.p, 0, sizeof(unsigned), st));
    MPG_HIP(hipMemsetAsync(d->actflag.p, 0, (size_t)n, st));
    hipLaunchKernelGGL(k_flag_list, dim3(nblk(m)), dim3(256), 0, st, m, d_list, (int)n, d->actflag.p, d->err.p);
}

namespace {

// cube (integer coordinates at its level) of a TopNode: the prefix of its Peano-Hilbert key walked through the curve's state
// machine backwards (digit -> octant)
void topnode_cube(const mpg_topnode &tn, int &level, unsigned &x, unsigned &y, unsigned &z)
{
    level = (3 * PH_BITS - tn.Shift) / 3;
    x = y = z = 0;
    unsigned state = 0;
    for(int l = 0; l < level; l++) {
        const unsigned digit = (unsigned)((tn.StartKey >> (3 * (PH_BITS - 1 - l))) & 7ull);
        unsigned pix = 0;
        while(pix < 8 && H_SUBPIX[state][pix] != digit)
            pix++;
        MPG_CHECK(pix < 8, "mpg_dist_set_domain: corrupt Peano-Hilbert key");
        x = 2 * x + ((pix >> 2) & 1u);
        y = 2 * y + ((pix >> 1) & 1u);
        z = 2 * z + (pix & 1u);
        state = H_NEXT[state][pix];
    }
}

// cells (of nc across the 1.001-Box root cell starting at lo0) that the interval [a, b] touches, periodic with period Box
void cells_of_interval(double a, double b, double box, double lo0, double w, int nc, std::vector<char> &sel)
{
    sel.assign((size_t)nc, 0);
    if(b - a >= box) {
        std::fill(sel.begin(), sel.end(), 1);
        return;
    }
    for(int k = -1; k <= 1; k++) {
        const double aa = a + k * box, bb = b + k * box;
        int k0 = (int)floor((aa - lo0) / w), k1 = (int)floor((bb - lo0) / w);
        if(k1 < 0 || k0 >= nc)
            continue;
        k0 = std::max(k0, 0);
        k1 = std::min(k1, nc - 1);
        for(int c = k0; c <= k1; c++)
            sel[(size_t)c] = 1;
    }
}

} // namespace

extern "C" {

int mpg_dist_create(mpg_dist **out, mpg_engine *eng, const mpg_comm *comm)
{
    API_BEGIN
    MPG_CHECK(out && eng && comm, "null argument");
    MPG_CHECK(comm->NTask >= 1 && comm->NTask <= 64 && comm->ThisTask >= 0 && comm->ThisTask < comm->NTask, "mpg_dist_create: bad ThisTask / NTask");
    mpg_dist *d = new mpg_dist();
    d->eng = eng;
    d->comm = *comm;
    d->me = comm->ThisTask;
    d->nt = comm->NTask;
    if(comm->bind_stream && comm->device_buffers) {
        if(comm->bind_stream(comm->ctx, (void *)eng->stream) != 0) {
            delete d;
            throw Error("mpg_comm: bind_stream failed");
        }
        d->stream_ordered = true;
        d->bound_stream = eng->stream;
    }
    *out = d;
    API_END
}

void mpg_dist_destroy(mpg_dist *d)
{
    if(!d)
        return;
    if(d->eng) {
        (void)hipSetDevice(d->eng->device);
        (void)hipStreamSynchronize(d->eng->stream);
        d->eng->tree.force_internal_above = 0;
        if(d->tree_stream)
            (void)hipStreamDestroy(d->tree_stream);
    }
    delete d;
}

int mpg_dist_set_domain(mpg_dist *d, double BoxSize, const mpg_topnode *TopNodes, int NTopNodes, const int *leaf_task, int NTopLeaves,
                        double margin, int La)
{
    API_BEGIN
    MPG_CHECK(d && TopNodes && leaf_task && NTopNodes > 0 && NTopLeaves > 0, "null argument");
    MPG_CHECK(BoxSize > 0 && margin > 0, "mpg_dist_set_domain: BoxSize and margin must be positive");
    MPG_HIP(hipSetDevice(d->eng->device));
    if(La <= 0) // cells [margin, 2 margin) wide: little over-import, few levels above the decomposition level
        La = (int)floor(log2(1.001 * BoxSize / margin));
    La = std::max(1, std::min(7, La));
    const int nc = 1 << La;
    const double w = 1.001 * BoxSize / nc, lo0 = BoxSize / 2. - 0.5 * 1.001 * BoxSize;
    // A node above level La that holds no particle of a needed cell is absent from the local tree.  That is harmless only if the
    // global walk could not have drawn a force from it: a node used unopened has len^2 / r^2 <= MaxBHOpeningAngle^2 <= 1, i.e. lies
    // at r >= len >= 2 w >= 2 margin from the target, beyond the short-range window's table (15 mesh cells, gravity.c:57-61)
    // whenever margin >= Rcut = 9 cells - so cells must not be narrower than the margin
    MPG_CHECK(w >= margin || La == 1, "mpg_dist_set_domain: cells of level La are narrower than the margin");
    const double grow = margin + 1e-9 * BoxSize; // (ownership is by integer key, cells by floating-point descent)
    std::vector<unsigned long long> need((size_t)nc * nc * nc, 0ull);
    std::vector<char> sx, sy, sz;
    int seen = 0;
    for(int i = 0; i < NTopNodes; i++) {
        const mpg_topnode &tn = TopNodes[i];
        if(tn.Daughter >= 0)
            continue;
        MPG_CHECK(tn.Leaf >= 0 && tn.Leaf < NTopLeaves, "mpg_dist_set_domain: TopNode without a valid Leaf");
        const int task = leaf_task[tn.Leaf];
        MPG_CHECK(task >= 0 && task < d->nt, "mpg_dist_set_domain: Task of a TopLeaf out of range");
        seen++;
        int level;
        unsigned x, y, z;
        topnode_cube(tn, level, x, y, z);
        const double s = 1.001 * BoxSize / (double)(1u << level);
        cells_of_interval(lo0 + x * s - grow, lo0 + (x + 1) * s + grow, BoxSize, lo0, w, nc, sx);
        cells_of_interval(lo0 + y * s - grow, lo0 + (y + 1) * s + grow, BoxSize, lo0, w, nc, sy);
        cells_of_interval(lo0 + z * s - grow, lo0 + (z + 1) * s + grow, BoxSize, lo0, w, nc, sz);
        const unsigned long long bit = 1ull << task;
        for(int a = 0; a < nc; a++) {
            if(!sx[a])
                continue;
            for(int b = 0; b < nc; b++) {
                if(!sy[b])
                    continue;
                unsigned long long *row = need.data() + ((size_t)a * nc + b) * nc;
                for(int c = 0; c < nc; c++)
                    if(sz[c])
                        row[c] |= bit;
            }
        }
    }
    MPG_CHECK(seen == NTopLeaves, "mpg_dist_set_domain: the TopNodes do not hold NTopLeaves leaves");
    d->need.reserve(need.size());
    MPG_HIP(hipMemcpy(d->need.p, need.data(), need.size() * sizeof(unsigned long long), hipMemcpyHostToDevice));
    d->box = BoxSize;
    d->margin = margin;
    d->La = La;
    d->have_domain = true;
    d->stats[3] = La;
    API_END
}

int mpg_dist_dev_set_garbage(mpg_dist *d, int64_t n_own, const unsigned char *d_garbage)
{
    API_BEGIN
    MPG_CHECK(d && n_own >= 0, "null argument");
    MPG_HIP(hipSetDevice(d->eng->device));
    d->d_skip = nullptr;
    d->n_skip = 0;
    d->n_skip_rows = -1;
    if(d_garbage && n_own > 0) {
        hipStream_t st = d->eng->stream;
        d->scount.reserve(4);
        MPG_HIP(hipMemsetAsync(d->scount.p, 0, sizeof(unsigned long long), st));
        hipLaunchKernelGGL(k_count_nonzero, dim3(nblk(n_own)), dim3(256), 0, st, n_own, d_garbage, d->scount.p);
        unsigned long long c = 0;
        MPG_HIP(hipMemcpyAsync(&c, d->scount.p, sizeof(c), hipMemcpyDeviceToHost, st));
        sync(d);
        if(c > 0) {
            // a COPY of the flags (the caller's pointer was kept "until the next call" and matched to a table by its row
            // count alone - a caller moving to another table of the same size without calling this again would have had freed or stale
            // flags applied to it); they stay in force until the next call of this function, as documented
            d->skip_own.reserve((size_t)n_own + 1);
            MPG_HIP(hipMemcpyAsync(d->skip_own.p, d_garbage, (size_t)n_own, hipMemcpyDeviceToDevice, st));
            d->d_skip = d->skip_own.p;
            d->n_skip = (int64_t)c;
            d->n_skip_rows = n_own;
        }
    }
    API_END
}

int mpg_dist_dev_set_types(mpg_dist *d, int64_t n_own, const uint8_t *d_type)
{
    API_BEGIN
    MPG_CHECK(d && n_own >= 0, "null argument");
    MPG_HIP(hipSetDevice(d->eng->device));
    d->n_type_rows = -1;
    if(d_type) {
        d->type_own.reserve((size_t)n_own + 1);
        if(n_own > 0)
            MPG_HIP(hipMemcpyAsync(d->type_own.p, d_type, (size_t)n_own, hipMemcpyDeviceToDevice, d->eng->stream));
        d->n_type_rows = n_own;
    }
    API_END
}

int mpg_dist_set_sph_options(mpg_dist *d, int BlackHoleOn)
{
    API_BEGIN
    MPG_CHECK(d, "null argument");
    d->blackholes = BlackHoleOn != 0;
    API_END
}

int mpg_dist_get_stats(mpg_dist *d, int64_t stats[8])
{
    API_BEGIN
    MPG_CHECK(d && stats, "null argument");
    for(int i = 0; i < 8; i++)
        stats[i] = d->stats[i];
    API_END
}

int mpg_dist_get_times(mpg_dist *d, double ms[8])
{
    API_BEGIN
    MPG_CHECK(d && ms, "null argument");
    for(int i = 0; i < 8; i++)
        ms[i] = d->times[i];
    API_END
}

} // extern "C"
