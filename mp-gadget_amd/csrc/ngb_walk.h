// ngb_walk.h -- group-cooperative neighbour search over the level-ordered tree (treewalk_visit_ngbiter / _nolist_ngbiter,
// treewalk.c:930-1265) and the host's radius iteration around it (treewalk_do_hsml_loop, treewalk.c:1269-1367).  One search behind
// five callers: k_density and k_hydro (sph.hip), k_vdisp<BH> (veldisp.hip), k_fof_walk<MODE> (fof.hip) and k_grav_short_pair<POT>
// (grav_pair_walk.hip).  A kernel declares the LDS, loads its target and says what a candidate is (fetch) and what is done with it
// (visit); the control flow - set-up, walk, list, pause and resume, overflow - is ngb_group / ngb_search / ngb_overflowed below.
#pragma once
#include "mpg_common.h"
#include <vector>

namespace mpg {

#define FACT1 0.366025403785      // treewalk.c:19

// wave-wide ballot of a predicate.  (HIP's ballot64(int) compares an integer with zero: a boolean that exists only as a lane mask is
// first materialised as 0 / 1 in a VGPR and compared again - two vector instructions per ballot that this form does not need.)
__device__ __forceinline__ unsigned long long ballot64(const bool b) { return __builtin_amdgcn_ballot_w64(b); }

__device__ __forceinline__ double nearest_img(double x, double box, double invbox) { return x - box * rint(x * invbox); }
// WRAP = false: plain differences, for the targets of a wave that all lie farther from every face of the box than their search radius
// (interior_wave below).  Exact, not approximate: a node / particle that the nearest-image form keeps has |d| <= radius + len < Box / 2 per
// axis on the unwrapped image for such a target (rint(d / Box) = 0: NEAREST() returns d itself), and one whose unwrapped |d| exceeds Box / 2
// on an axis lies, on its nearest image, beyond the face the target is `radius` away from, plus its own half length: culled by both forms.
template <bool WRAP> __device__ __forceinline__ double near_img(double x, double box, double invbox) { return WRAP ? x - box * rint(x * invbox) : x; }

// Do all targets of this wave (lanes with `valid`) lie farther than their search radius from every face of the box?  (Box / 500 of margin
// as in the gravity walk's MODE 2, and radius < Box / 4 so that "beyond Box / 2" implies "culled" for every node below the root.)
__device__ __forceinline__ bool interior_wave(const bool valid, const double px, const double py, const double pz, const double radius, const double box)
{
    const double face = radius + 0.002 * box;
    const bool out = valid && (!(radius < 0.25 * box) || fmin(fmin(px, py), pz) < face || fmax(fmax(px, py), pz) > box - face);
    return ballot64(out) == 0ull;
}

// cull_node, treewalk.c:1015-1042 (hm = 0: asymmetric search radius Hsml; symmetric: max(node hmax, Hsml)), without the reference's early
// returns (|d| > dist on any axis is max |d| > dist, and the wave's lanes never agree on an exit) and with its two comparisons taken as lane
// masks (walk_stepk): the ballot of a bare comparison is the comparison's own result register, and the boolean algebra of the step runs once
// per wave on the scalar unit (as in k_walk_lists8).  Written with per-lane booleans, hipcc materialised every `a && b` that went into a ballot
// as v_cndmask 0/1 + v_cmp again.
template <bool WRAP>
__device__ __forceinline__ unsigned long long cull_mask(const NodeGeo &g, double hm, double hsml, double px, double py, double pz, double box, double invbox)
{
    const double dist = fmax(hm, hsml) + 0.5 * g.len;
    const double dx = near_img<WRAP>(g.cx - px, box, invbox);
    const double dy = near_img<WRAP>(g.cy - py, box, invbox);
    const double dz = near_img<WRAP>(g.cz - pz, box, invbox);
    const double cmax = fmax(fmax(fabs(dx), fabs(dy)), fabs(dz));
    const double r2 = dx * dx + dy * dy + dz * dz;
    const double d2 = dist + FACT1 * g.len;
    return __builtin_amdgcn_ballot_w64(cmax > dist) | __builtin_amdgcn_ballot_w64(r2 > d2 * d2);
}

// ---------------------------------------------------------------------------------------------------------------------
// Group-cooperative neighbour search.  A wave is 8 groups of 8 lanes; a group owns ONE target and walks
// the level-ordered copy of the tree (children of a node contiguous): one step pops a child range from the group's LIFO in
// LDS, the 8 lanes cull the <= 8 children (treewalk.c:1015-1042) with one coalesced read each, internal survivors push their
// own child range, and the surviving leaves are evaluated at once, lane s <-> particle s of the leaf (one coalesced read
// per group).  The visited set is the reference's; only the order of the sums differs.  (The first form, one lane per
// target walking the depth-first arrays, spent its time in dependent, uncoalesced 48-byte node reads: 27 ms per density
// pass over 2.1 M targets against the figures in DESIGN.md section 3.4.)
constexpr int SPH_STK = 160; // pending child ranges per group: <= 7 per level + 8, 21 levels

// The walk and the leaf work are separated in time so that the 8 groups of a wave stay in step: phase A walks (walk_stepk) and
// only records the opened leaves in a per-group list in LDS; phase B lets every group take its next leaf per iteration.
// (Interleaving them made every group wait while one group tested the leaves it had just opened.)
constexpr int SPH_LCAP = 120; // leaf entries per group; phase A pauses when a group may not fit 8 more per child range of a step

__device__ __forceinline__ double group_sum(double v)
{
    for(int off = 1; off < 8; off <<= 1)
        v += __shfl_xor(v, off);
    return v;
}
__device__ __forceinline__ int group_sum_int(int v)
{
    for(int off = 1; off < 8; off <<= 1)
        v += __shfl_xor(v, off);
    return v;
}

// One cooperative search step: pops child ranges, culls, pushes; SYM: symmetric search radius max(node hmax, Hsml) (hydro);
// otherwise Hsml (density, FOF, the pair-wise gravity check).  K child ranges per step (round 3; rounds 1-2 took one): the search is a
// chain of dependent steps - LDS pop -> node loads -> cull ->
// ballots -> LDS push, ~57 per wave of 8 targets in the hydro loop and 45 % of that kernel's time (cycle counters) - whose
// latency 4 waves per SIMD do not hide; taking the K topmost ranges of the LIFO at once divides the number of sequential steps
// for the same node tests.  Lane s tests child s of every range.  The leaves opened go to the group's list, first those of the upper ranges.
// Returns the new number of list entries.
// MERGE (round 4): opened leaves of one child range whose particles are contiguous in tree order (siblings: the children of a split cell
// hold one or two particles each, gas leaves 2.7 on average) are joined into one list entry of <= 8 particles, so that the candidate tests
// of phase B run on fuller lanes (k_density 8.4 -> 7.5 ms, k_hydro 9.5 -> 8.8 at 2 x 128^3).  Which sets of siblings fit one entry is a
// property of the tree (a leaf's NodeLinkB::firstchild, written with the level-ordered copy): all children, a quad or a pair; a set is joined when every
// existing child of it was opened by this target, its first lane emitting the run.  The candidates are those of the opened leaves and no
// others, so the reference's counters are unchanged.  (First form: the lanes compared start / count / contiguity with their neighbours
// s ^ 1, s ^ 2, s ^ 4 at run time - 65 vector instructions per child range against ~20.)
// sgeo / shm: the geometry the cull tests and, for SYM, the radius per node - the nodes' cells and `hmax` as in the reference (tv.geoB,
// tv.hmaxB: FOF, the pair-wise gravity check), or the cubes around the nodes' particles and their largest Hsml (tv.geoS, tv.hsmaxS: the
// SPH loops; TreeBuilder::calc_search_boxes).
template <bool SYM, int K, bool MERGE = false, bool WRAP = true>
__device__ __forceinline__ int walk_stepk(const TreeView &tv, const NodeGeo *__restrict__ sgeo, const double *__restrict__ shm, unsigned *stack, int &sp,
                                          const bool valid_more, const int s, const int gshift, const double hsml, const double px, const double py,
                                          const double pz, unsigned *llist, int nl, bool &overflow)
{
    const bool can = valid_more;
    const double invbox = 1.0 / tv.box;
    const unsigned below = (1u << s) - 1u;
    unsigned r[K];
    int my[K];
    bool tst[K];
    // (more than one range only while the LIFO has room for all their children: a depth-first search with one range per step needs at
    // most 7 entries per tree level + 8, which is what SPH_STK is sized for; K ranges at once could need up to K times that)
    const int take = (SPH_STK - sp >= 7 * K) ? K : 1;
#pragma unroll
    for(int k = 0; k < K; k++) { // range k: the k-th entry from the top of the LIFO
        r[k] = (can && sp > k && k < take) ? stack[sp - 1 - k] : 0u;
        tst[k] = s < (int)(r[k] & 15u);
        my[k] = tst[k] ? (int)(r[k] >> 4) + s : 0; // (lanes without a child read node 0: no exec-mask regions, all loads issued together)
    }
    NodeGeo g[K];
    NodeLinkB lk[K];
    double hm[K];
#pragma unroll
    for(int k = 0; k < K; k++) {
        g[k] = sgeo[my[k]];
        lk[k] = tv.linkB[my[k]];
        hm[k] = SYM ? shm[my[k]] : 0.0;
    }
    unsigned gl[K], gp[K], ent[K];
    unsigned long long m_leaf[K], m_push[K]; // lane masks: the children opened as leaves / whose own children are pushed
#pragma unroll
    for(int k = 0; k < K; k++) {
        const unsigned long long m_in = __builtin_amdgcn_ballot_w64(tst[k]) & ~cull_mask<WRAP>(g[k], hm[k], hsml, px, py, pz, tv.box, invbox);
        const unsigned long long m_pc = __builtin_amdgcn_ballot_w64(lk[k].pcount > 0);
        m_leaf[k] = m_in & m_pc;
        m_push[k] = m_in & ~m_pc & __builtin_amdgcn_ballot_w64(lk[k].nchild > 0);
        ent[k] = ((unsigned)lk[k].pstart << 4) | (unsigned)lk[k].pcount;
        if(MERGE) {
            const bool lf = __builtin_amdgcn_inverse_ballot_w64(m_leaf[k]);
            unsigned pcm = lf ? (unsigned)lk[k].pcount : 0u;
            const unsigned h = lf ? (unsigned)lk[k].firstchild : 0u;                  // (a leaf's merge hints: NodeLinkB)
            const unsigned m = (unsigned)((m_leaf[k] >> gshift) & 0xffull);           // the children this target opened as leaves
            const unsigned x = m ^ ((1u << (r[k] & 15u)) - 1u);                       // existing children that are not among them
            const unsigned sq = (h >> 4) & 15u, sp = h & 15u;
            pcm = (sp != 0u && (x & (3u << (s & 6))) == 0u) ? ((s & 1) == 0 ? sp : 0u) : pcm;
            pcm = (sq != 0u && (x & (15u << (s & 4))) == 0u) ? ((s & 3) == 0 ? sq : 0u) : pcm;
            ent[k] = ((unsigned)lk[k].pstart << 4) | pcm;
            m_leaf[k] = __builtin_amdgcn_ballot_w64(pcm != 0u);
        }
        gl[k] = (unsigned)((m_leaf[k] >> gshift) & 0xffull);
        gp[k] = (unsigned)((m_push[k] >> gshift) & 0xffull);
    }
    const int taken = can ? (sp < take ? sp : take) : 0;
    const int base = sp - taken;
    int npush = 0;
#pragma unroll
    for(int k = 0; k < K; k++)
        npush += __popc(gp[k]);
    if(can && base + npush > SPH_STK)
        overflow = true;
    else {
        // the children of the lower ranges below those of the upper ones: the search stays depth-first in the topmost range
        int at = base;
#pragma unroll
        for(int k = K - 1; k >= 0; k--) {
            if(__builtin_amdgcn_inverse_ballot_w64(m_push[k]))
                stack[at + __popc(gp[k] & below)] = ((unsigned)lk[k].firstchild << 4) | (unsigned)lk[k].nchild;
            at += __popc(gp[k]);
        }
    }
    if(can)
        sp = base + npush;
#pragma unroll
    for(int k = 0; k < K; k++) {
        if(__builtin_amdgcn_inverse_ballot_w64(m_leaf[k]))
            llist[nl + __popc(gl[k] & below)] = ent[k];
        nl += can ? __popc(gl[k]) : 0;
    }
    return nl;
}

// The state of one group's search: who the lane is, the group's LIFO and leaf list in LDS, the queue slot of its target.
struct NgbGroup {
    int lane, s, gshift; // lane of the wave, lane of the group, the group's first bit in a wave mask
    unsigned *stack, *llist;
    int64_t q;           // queue slot of the group's target
    bool valid;          // q < ntargets
    int sp;              // entries on the LIFO
    bool overflow;       // the LIFO would not hold a step's children (walk_stepk)
};

// Group set-up for blocks of 256 threads (32 targets): s_stack / s_llist are the kernel's __shared__ unsigned[4 * 8 * SPH_STK] and
// [4 * 8 * SPH_LCAP].  A group with a target starts with the root on its LIFO.
__device__ __forceinline__ NgbGroup ngb_group(unsigned *s_stack, unsigned *s_llist, const int64_t ntargets)
{
    NgbGroup g;
    g.lane = threadIdx.x & 63;
    const int grp = g.lane >> 3, slot = (threadIdx.x >> 6) * 8 + grp;
    g.s = g.lane & 7;
    g.gshift = grp * 8;
    g.stack = s_stack + slot * SPH_STK;
    g.llist = s_llist + slot * SPH_LCAP;
    g.q = (int64_t)blockIdx.x * 32 + slot;
    g.valid = g.q < ntargets;
    g.sp = 0;
    g.overflow = false;
    if(g.valid) {
        if(g.s == 0)
            g.stack[0] = (0u << 4) | 1u; // the root
        g.sp = 1;
    }
    return g;
}

// The whole search of a group, in batches until the LIFO is empty.  The walk and the leaf work are separated in time (SPH_LCAP above):
//   phase A  walk_stepk until the LIFO is empty or the list may not fit one more step (nl + 8 K <= SPH_LCAP before every step: a step
//            lists at most 8 entries per child range).  A paused walk loses nothing: its pending ranges stay on the LIFO.
//   phase B  one list entry per iteration, lane s <-> particle s of the entry: visit(record, tree slot, live), live = s < count.  The
//            record of the NEXT entry is requested (fetch(tree slot)) before this one is visited: an iteration is a dependent LDS read ->
//            gather -> test chain, and 4 waves per SIMD do not hide the gather's latency.  Lanes beyond an entry's count fetch its first
//            particle (no exec-mask region around the load) and visit with live = false.
//   between() runs after a batch when some group of the wave has ranges left; `radius` is read again by every step, so a caller may
//            shrink it there (k_vdisp<false>).
// Ends at once when a group's LIFO overflowed: the caller ends with ngb_overflowed().  (Both ends leave through the one exit below the outer
// loop: with a `return` at each of them hipcc allocated k_density 58 and k_vdisp<false> 283 spilled registers instead of 0 and 40.)
template <bool SYM, int K, bool MERGE, bool WRAP, class Fetch, class Visit, class Between>
__device__ __forceinline__ void ngb_search(const TreeView &tv, const NodeGeo *__restrict__ sgeo, const double *__restrict__ shm, NgbGroup &g,
                                           const double &radius, const double px, const double py, const double pz, Fetch &&fetch, Visit &&visit,
                                           Between &&between)
{
    const int s = g.s;
    for(;;) {
        int nl = 0;
        for(;;) {
            const bool go = g.sp > 0 && nl + 8 * K <= SPH_LCAP;
            if(ballot64(go) == 0)
                break;
            nl = walk_stepk<SYM, K, MERGE, WRAP>(tv, sgeo, shm, g.stack, g.sp, go, s, g.gshift, radius, px, py, pz, g.llist, nl, g.overflow);
            if(ballot64(g.overflow) != 0)
                break;
        }
        if(ballot64(g.overflow) != 0)
            break;
        unsigned e = (0 < nl) ? g.llist[0] : 0u;
        int ps = (int)(e >> 4), pc = (int)(e & 15u);
        auto rec = fetch(ps + (s < pc ? s : 0));
        for(int it = 0;; it++) {
            const bool has = it < nl;
            if(ballot64(has) == 0)
                break;
            const unsigned e_n = (it + 1 < nl) ? g.llist[it + 1] : 0u;
            const int ps_n = (int)(e_n >> 4), pc_n = (int)(e_n & 15u);
            const auto rec_n = fetch(ps_n + (s < pc_n ? s : 0));
            visit(rec, ps + s, s < pc);
            rec = rec_n;
            ps = ps_n;
            pc = pc_n;
        }
        if(ballot64(g.sp > 0) == 0)
            break;
        between();
    }
}

// The end of a search whose LIFO overflowed in some group of the wave: the wave flags `err` and the kernel returns without results.
__device__ __forceinline__ bool ngb_overflowed(const NgbGroup &g, unsigned *__restrict__ err)
{
    if(ballot64(g.overflow) == 0)
        return false;
    if(g.lane == 0)
        atomicExch(err, 1u);
    return true;
}

// wave-aggregated append of `value` for the lanes with `flag`: one atomic per wave (same-address atomics serialise)
__device__ __forceinline__ void wave_append(const bool flag, const int value, int *__restrict__ queue, unsigned *__restrict__ counter)
{
    const unsigned long long m = ballot64(flag);
    if(m == 0)
        return;
    const int lane = threadIdx.x & 63;
    const int leader = __ffsll((long long)m) - 1;
    unsigned basepos = 0;
    if(lane == leader)
        basepos = atomicAdd(counter, (unsigned)__popcll(m));
    basepos = __shfl(basepos, leader);
    if(flag)
        queue[basepos + __popcll(m & ((1ull << lane) - 1ull))] = value;
}

// pass statistics: the wave's sums of two per-lane counters to stats[0], stats[1], its number of lanes with `third` to stats[2]
__device__ __forceinline__ void wave_stats(unsigned long long *__restrict__ stats, const unsigned n0, const unsigned n1, const bool third = false)
{
    unsigned long long c0 = n0, c1 = n1;
    for(int off = 32; off > 0; off >>= 1) {
        c0 += __shfl_down(c0, off);
        c1 += __shfl_down(c1, off);
    }
    const unsigned long long m = ballot64(third);
    if((threadIdx.x & 63) == 0 && stats) {
        atomicAdd(&stats[0], c0);
        atomicAdd(&stats[1], c1);
        if(m != 0)
            atomicAdd(&stats[2], (unsigned long long)__popcll(m));
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// The host side.  treewalk_do_hsml_loop, treewalk.c:1292-1364: passes over a shrinking queue until no target asks for another.  launch(queue,
// n, redo) starts one pass of n targets that appends its unfinished targets to `redo` and counts them in *d_nredo; d_err (at most 7 words
// behind d_nredo, read back with it) is the search's overflow flag.  Adds the passes and the targets they took to `iterations` and `targets`;
// `lengths`, when given, gets the queue length of every pass.
template <class Launch>
inline void ngb_hsml_loop(int *qa, int *qb, unsigned nq, unsigned *d_nredo, const unsigned *d_err, const int maxiter, const char *who, hipStream_t st,
                          int64_t &iterations, int64_t &targets, std::vector<int64_t> *lengths, Launch &&launch)
{
    const size_t nw = (size_t)(d_err - d_nredo) + 1;
    MPG_CHECK(nw >= 2 && nw <= 8, "ngb_hsml_loop: the overflow flag does not follow the redo counter");
    while(nq > 0) {
        iterations++;
        targets += nq;
        if(lengths)
            lengths->push_back(nq);
        MPG_HIP(hipMemsetAsync(d_nredo, 0, sizeof(unsigned), st));
        launch(qa, nq, qb);
        MPG_HIP(hipGetLastError());
        unsigned w[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        MPG_HIP(hipMemcpyAsync(w, d_nredo, nw * sizeof(unsigned), hipMemcpyDeviceToHost, st));
        MPG_HIP(hipStreamSynchronize(st));
        MPG_CHECK(w[nw - 1] == 0, std::string(who) + ": neighbour-search stack overflow (tree deeper than the walk supports)");
        nq = w[0];
        int *t = qa;
        qa = qb;
        qb = t;
        if(nq > 0 && iterations > maxiter) // MAXITER, endrun(1155), treewalk.c:1361-1364
            fail(__FILE__, __LINE__, std::string(who) + ": failed to converge for " + std::to_string(nq) + " particles");
    }
}

// the end of a loop: its first `n` statistics words, after the check of the overflow flag
inline void ngb_read_stats(const unsigned long long *d_stats, const int n, unsigned long long *out, const unsigned *d_err, const char *who,
                           hipStream_t st)
{
    unsigned e = 0;
    MPG_HIP(hipMemcpyAsync(out, d_stats, n * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
    MPG_HIP(hipMemcpyAsync(&e, d_err, sizeof(e), hipMemcpyDeviceToHost, st));
    MPG_HIP(hipStreamSynchronize(st));
    MPG_CHECK(e == 0, std::string(who) + ": neighbour-search stack overflow (tree deeper than the walk supports)");
}

} // namespace mpg
