// winds.hip -- the wind model (winds_and_feedback, sfr_eff.c:391-392; winds_subgrid, :283; winds_evolve, :235) for gfx950, fp64.
//
// Reference: libgadget/winds.c (winds_and_feedback :298-371, sfr_wind_copy :400-412, sfr_wind_weight_ngbiter :414-450,
// sfr_wind_feedback_ngbiter :513-569, cmp_by_part_id :207-224, wind_do_kick :453-475, get_wind_dir :477-490, get_wind_params :493-511,
// winds_subgrid :275-295, winds_make_after_sf :571-589, winds_evolve :374-391).
//
// Mapping: the group-cooperative search of ngb_walk.h with the asymmetric radius (as metals.hip), 8 lanes per new star, over the tree the
// caller has: the stars are not in it, the queue is the caller's list of rows.  Candidates are the rows of the tree whose CURRENT type is
// 0 and whose DelayTime is not positive; their mass is the caller's column, read by particle index for the candidates inside the radius
// (the tree-order copy of the masses is the one of the last build; metal_return and blackhole have changed masses since).
//
// The nearest-star rule.  The reference appends every potential kick (star, gas, r) to one list, sorts it by (gas, r, StarID) and applies
// the first entry of every gas particle: the kick of the star of smallest r, ties to the smaller ID.  Here:
//   k_wind_feedback  writes the entry into the star's own segment of the list - the weight walk has counted every star's eligible
//                    neighbours, k_wind_offsets turns the counts into segment starts, and a group numbers its entries with ballots: no
//                    shared counter (the first form took one position per entry from one global counter, one atomic per wave and leaf
//                    entry: 9.2 ms of the 10.9 ms of a call with 100 000 stars at 2 x 128^3, against 0.7 ms for the weight walk) - and
//                    takes atomicMin(rmin[gas], bits(r)): r = sqrt(r2) is not negative, and the bit patterns of non-negative doubles
//                    order as the numbers do.  Unused entries of a segment keep star = -1.
//   k_wind_resolve   over the list: an entry with bits(r) == rmin[gas] takes atomicMin(win[gas], StarID).
//   k_wind_apply     over the list: the entry with bits(r) == rmin[gas] and StarID == win[gas] is applied.
// rmin[gas] is complete when the walk's kernel has ended and win[gas] when k_wind_resolve has: each is the minimum of a fixed SET, so
// neither depends on the order of arrival, and no lane waits for another.  Exactly one entry per kicked gas particle matches both unless
// the list names one star twice (or two stars share an ID): the matching entries then carry the same star, and the one whose compare-and-
// swap of rmin[gas] against a sentinel succeeds applies the kick - once, with the same numbers whichever it is.
// Only the winning entry touches the gas particle's rows, so no accumulator and no separate per-particle pass are needed.
#include "winds.h"
#include "ngb_walk.h"
#include <cmath>
#include <type_traits>

namespace mpg {

#ifndef WD_OCC
// waves per SIMD the launch bound of both walks asks for (the compiler's resource report: DESIGN 3.13)
#define WD_OCC 4
#endif
constexpr int WD_WALK_K = 2;    // child ranges per search step (walk_stepk, ngb_walk.h), as the SPH loops
constexpr bool WD_MERGE = true; // sibling leaves joined into one list entry
constexpr double WD_GAMMA_MINUS1 = 5.0 / 3.0 - 1; // physconst.h:35-36

// words of WindsEngine::ctr: listed rows that are no stars (or no gas: subgrid, evolve), potential kicks, "Odd v" kicks, kicks applied,
// potential kicks beyond the list's capacity, the search's overflow flag
constexpr int CTR_BAD = 0, CTR_NKICK = 1, CTR_ODD = 2, CTR_APPLIED = 3, CTR_LISTFULL = 4, CTR_ERR = 7;
// words of stats beyond wave_stats' three: (particle index << 32 | list entry) of the applied kick of lowest particle index
constexpr int STAT_LOWEST = 4;
constexpr unsigned long long WD_NONE = ~0ull;

__device__ __forceinline__ double wd_random(const WindScalars &S, const unsigned long long id) { return S.rnd[id % S.rndsize]; }

// get_wind_params, winds.c:493-511
struct WindKickPar {
    double v, windeff, utherm;
};
__device__ __forceinline__ WindKickPar wd_params(const WindScalars &S, const double vdisp)
{
    const mpg_wind_params &P = S.p;
    const double vphys = vdisp / S.atime;
    WindKickPar k;
    k.utherm = P.WindThermalFactor * 1.5 * vphys * vphys;
    if(P.WindModel & WIND_FIXED_EFFICIENCY) {
        k.windeff = P.WindEfficiency;
        k.v = P.WindSpeed * S.atime;
    }
    else { // WIND_USE_HALO (mpg_set_wind_params refuses a model with neither)
        k.windeff = (P.WindSigma0 * P.WindSigma0) / (vphys * vphys + 2 * k.utherm);
        k.v = P.WindSpeedFactor * vdisp;
    }
    if(k.v < P.MinWindVelocity * S.atime)
        k.v = P.MinWindVelocity * S.atime;
    return k;
}

// wind_do_kick + get_wind_dir, winds.c:453-490, on row ci
__device__ __forceinline__ void wd_kick(const WindView &A, const WindScalars &S, const int64_t ci, const double v, const double therm)
{
    const mpg_wind_arrays &a = A.a;
    const unsigned long long id = a.id[ci];
    const double theta = acos(2 * wd_random(S, id + 3ull) - 1);
    const double phi = 2 * M_PI * wd_random(S, id + 4ull);
    if(v > 0 && S.atime > 0) {
        a.vel[3 * ci] += v * (sin(theta) * cos(phi));
        a.vel[3 * ci + 1] += v * (sin(theta) * sin(phi));
        a.vel[3 * ci + 2] += v * cos(theta);
        const double enttou = pow(a.density[ci] / pow(S.atime, 3), WD_GAMMA_MINUS1) / WD_GAMMA_MINUS1;
        a.entropy[ci] += therm / enttou;
        if(S.p.MaxWindFreeTravelTime > 0) { // winds_ever_decouple
            double delay = S.p.WindFreeTravelLength / (v / S.atime);
            if(delay > S.p.MaxWindFreeTravelTime)
                delay = S.p.MaxWindFreeTravelTime;
            a.delaytime[ci] = delay;
        }
    }
}

// is the row of the tree an eligible neighbour: gas NOW, not in the wind (sfr_wind_weight_ngbiter :436, sfr_wind_feedback_ngbiter :536-543)
__device__ __forceinline__ bool wd_eligible(const WindView &A, const int64_t ci) { return (A.type[ci] & 7) == 0 && !(A.a.delaytime[ci] > 0); }

// sfr_wind_copy's check, winds.c:406-407: every listed row is a star of the table
__global__ void __launch_bounds__(256) k_wind_check(const WindView A, const int *__restrict__ list, int64_t nlist, const int want, unsigned *__restrict__ ctr)
{
    const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    bool bad = false;
    if(q < nlist) {
        const int64_t i = list ? list[q] : q;
        bad = i < 0 || i >= A.n || !A.type || (A.type[i] & 7) != want;
    }
    const unsigned long long m = ballot64(bad);
    if(m != 0 && (threadIdx.x & 63) == 0)
        atomicAdd(ctr + CTR_BAD, (unsigned)__popcll(m));
}

// The weight walk: sfr_wind_weight_ngbiter.  TotalWeight per row of the list, the eligible neighbours to stats[0] (nvisited).
__global__ void __launch_bounds__(256, WD_OCC) k_wind_weight(const TreeView tv, const WindView A, const int *__restrict__ newstars, int64_t nnew,
                                                             double *__restrict__ weight, unsigned *__restrict__ count, unsigned *__restrict__ ctr,
                                                             unsigned long long *__restrict__ stats)
{
    __shared__ unsigned s_stack[4 * 8 * SPH_STK];
    __shared__ unsigned s_llist[4 * 8 * SPH_LCAP];
    NgbGroup g = ngb_group(s_stack, s_llist, nnew);
    const bool valid = g.valid;
    unsigned n_int = 0, n_cand = 0;
    int64_t i = 0;
    double px = 0, py = 0, pz = 0, hsml = 0;
    if(valid) {
        i = newstars[g.q];
        px = A.pos[3 * i];
        py = A.pos[3 * i + 1];
        pz = A.pos[3 * i + 2];
        hsml = A.a.hsml[i];
    }
    const double h2 = hsml * hsml;
    double w = 0;
    auto loops = [&](auto wrap_tag) {
        constexpr bool WRAP = decltype(wrap_tag)::value;
        ngb_search<false, WD_WALK_K, WD_MERGE, WRAP>(
            tv, tv.geoB, nullptr, g, hsml, px, py, pz, [&](const int slot) { return tv.src[slot]; },
            [&](const Src4 &cand, const int slot, const bool live) {
                if(live) {
                    n_cand++;
                    const double d0 = near_img<WRAP>(px - cand.x, tv.box, 1.0 / tv.box);
                    const double d1 = near_img<WRAP>(py - cand.y, tv.box, 1.0 / tv.box);
                    const double d2 = near_img<WRAP>(pz - cand.z, tv.box, 1.0 / tv.box);
                    const double r2 = d0 * d0 + d1 * d1 + d2 * d2;
                    if(!(r2 > h2) && !(sqrt(r2) > hsml)) { // treewalk.c:991, winds.c:433
                        const int64_t ci = tv.order[slot];
                        if(wd_eligible(A, ci)) {
                            n_int++;
                            w += (double)A.mass[ci];
                        }
                    }
                }
            },
            [] {});
    };
    if(interior_wave(valid, px, py, pz, hsml, tv.box))
        loops(std::false_type{});
    else
        loops(std::true_type{});
    if(ngb_overflowed(g, ctr + CTR_ERR))
        return;
    w = group_sum(w);
    const int elig = group_sum_int((int)n_int);
    if(valid && g.s == 0) {
        weight[g.q] = w;
        count[g.q] = (unsigned)elig;
        if(A.a.totalweight)
            A.a.totalweight[i] = w;
    }
    wave_stats(stats, n_int, n_cand);
}

// the stars' segments of the kick list: offset[q] = sum of count[0 .. q - 1], offset[nnew] the total (one block)
__global__ void __launch_bounds__(256) k_wind_offsets(const int64_t nnew, const unsigned *__restrict__ count, unsigned *__restrict__ offset)
{
    __shared__ unsigned s_sum[256];
    const int t = threadIdx.x;
    const int64_t chunk = (nnew + 255) / 256, lo = t * chunk, hi = lo + chunk < nnew ? lo + chunk : nnew;
    unsigned mine = 0;
    for(int64_t q = lo; q < hi; q++)
        mine += count[q];
    s_sum[t] = mine;
    __syncthreads();
    unsigned before = 0;
    for(int k = 0; k < t; k++)
        before += s_sum[k];
    for(int64_t q = lo; q < hi; q++) {
        offset[q] = before;
        before += count[q];
    }
    if(t == 255)
        offset[nnew] = before;
}

// The feedback walk: sfr_wind_feedback_ngbiter.  Potential kicks to the list, the smallest StarDistance per gas particle to rmin.
__global__ void __launch_bounds__(256, WD_OCC) k_wind_feedback(const TreeView tv, const WindView A, const WindScalars S, const int *__restrict__ newstars,
                                                               int64_t nnew, const double *__restrict__ weight, const unsigned *__restrict__ offset,
                                                               WindKick *__restrict__ kicks, const unsigned capacity,
                                                               unsigned long long *__restrict__ rmin, unsigned *__restrict__ ctr)
{
    __shared__ unsigned s_stack[4 * 8 * SPH_STK];
    __shared__ unsigned s_llist[4 * 8 * SPH_LCAP];
    NgbGroup g = ngb_group(s_stack, s_llist, nnew);
    int64_t i = 0;
    double px = 0, py = 0, pz = 0, hsml = 0, p = 0;
    unsigned long long id = 0;
    bool act = false;
    unsigned at0 = 0, at1 = 0, nk = 0; // the star's segment of the list [at0, at1), its entries so far (uniform in the group)
    if(g.valid) {
        i = newstars[g.q];
        at0 = offset[g.q];
        at1 = offset[g.q + 1];
        px = A.pos[3 * i];
        py = A.pos[3 * i + 1];
        pz = A.pos[3 * i + 2];
        hsml = A.a.hsml[i];
        id = A.a.id[i];
        const double tw = weight[g.q], vdisp = A.a.vdisp[i];
        if(!(tw == 0 || vdisp <= 0)) { // :539
            const WindKickPar k = wd_params(S, vdisp);
            p = k.windeff * (double)A.mass[i] / tw;
            act = k.v > 0; // :552
        }
    }
    if(!act)
        g.sp = 0; // no candidates: the group does not search
    const double h2 = hsml * hsml;
    const int s = g.s, gshift = g.gshift;
    auto loops = [&](auto wrap_tag) {
        constexpr bool WRAP = decltype(wrap_tag)::value;
        ngb_search<false, WD_WALK_K, WD_MERGE, WRAP>(
            tv, tv.geoB, nullptr, g, hsml, px, py, pz, [&](const int slot) { return tv.src[slot]; },
            [&](const Src4 &cand, const int slot, const bool live) {
                bool kick = false;
                double r = 0;
                if(live && act) {
                    const double d0 = near_img<WRAP>(px - cand.x, tv.box, 1.0 / tv.box);
                    const double d1 = near_img<WRAP>(py - cand.y, tv.box, 1.0 / tv.box);
                    const double d2 = near_img<WRAP>(pz - cand.z, tv.box, 1.0 / tv.box);
                    const double r2 = d0 * d0 + d1 * d1 + d2 * d2;
                    r = sqrt(r2);
                    if(!(r2 > h2) && !(r > hsml)) {
                        const int64_t ci = tv.order[slot];
                        if(wd_eligible(A, ci))
                            kick = wd_random(S, id + A.a.id[ci]) < p;
                    }
                }
                // the next entries of the star's segment, numbered inside the group
                const unsigned gm = (unsigned)((ballot64(kick) >> gshift) & 0xffull);
                if(kick) {
                    const unsigned at = at0 + nk + (unsigned)__popc(gm & ((1u << s) - 1u));
                    // (inside the star's own segment: the weight walk counted these pairs with the same tests; should the two walks ever
                    // disagree about a pair, that is the reference's "not enough room in kick queue", not an entry in a neighbour's segment)
                    if(at < at1 && at < capacity) {
                        kicks[at] = WindKick{(int)i, slot, r};
                        atomicMin(rmin + slot, (unsigned long long)__double_as_longlong(r));
                    }
                    else
                        atomicExch(ctr + CTR_LISTFULL, 1u);
                }
                nk += (unsigned)__popc(gm);
            },
            [] {});
    };
    if(interior_wave(g.valid, px, py, pz, hsml, tv.box))
        loops(std::false_type{});
    else
        loops(std::true_type{});
    (void)ngb_overflowed(g, ctr + CTR_ERR);
    unsigned tot = s == 0 ? nk : 0u; // the potential kicks of the wave's stars
    for(int off = 32; off > 0; off >>= 1)
        tot += __shfl_down(tot, off);
    if(g.lane == 0 && tot != 0)
        atomicAdd(ctr + CTR_NKICK, tot);
}

// of the entries at a gas particle's smallest distance, the smallest StarID
__global__ void __launch_bounds__(256) k_wind_resolve(const WindView A, const WindKick *__restrict__ kicks, const unsigned capacity,
                                                      const unsigned long long *__restrict__ rmin, unsigned long long *__restrict__ win)
{
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if(e >= capacity)
        return;
    const WindKick K = kicks[e];
    if(K.star < 0) // an unused entry of a segment
        return;
    if((unsigned long long)__double_as_longlong(K.r) == rmin[K.slot])
        atomicMin(win + K.slot, (unsigned long long)A.a.id[K.star]);
}

// the winning entry of every gas particle: wind_do_kick, and the reference's "Odd v" check (:350-355)
__global__ void __launch_bounds__(256) k_wind_apply(const TreeView tv, const WindView A, const WindScalars S, WindKick *__restrict__ kicks,
                                                    const unsigned capacity, unsigned long long *__restrict__ rmin,
                                                    const unsigned long long *__restrict__ win, unsigned *__restrict__ ctr,
                                                    unsigned long long *__restrict__ stats)
{
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if(e >= capacity || ctr[CTR_ERR] != 0 || ctr[CTR_LISTFULL] != 0) // an error of the walk: the call fails before anything is written
        return;
    const WindKick K = kicks[e];
    if(K.star < 0)
        return;
    const unsigned long long rb = (unsigned long long)__double_as_longlong(K.r), sid = A.a.id[K.star];
    if(sid != win[K.slot] || rb != rmin[K.slot])
        return;
    if(atomicCAS(rmin + K.slot, rb, WD_NONE) != rb) // (the same star listed twice: one of its entries)
        return;
    const int64_t ci = tv.order[K.slot];
    const WindKickPar k = wd_params(S, A.a.vdisp[K.star]);
    wd_kick(A, S, ci, k.v, k.utherm);
    if(A.a.kick_star)
        A.a.kick_star[ci] = sid + 1ull;
    if(k.v <= 0 || !isfinite(k.v) || !isfinite(A.a.delaytime[ci]))
        atomicAdd(ctr + CTR_ODD, 1u);
    atomicAdd(ctr + CTR_APPLIED, 1u);
    atomicMin(stats + STAT_LOWEST, ((unsigned long long)ci << 32) | (unsigned long long)e);
    kicks[e].r = k.v; // (the entry is read by this lane alone; mpg_winds_get_stats' maxvel)
}

// winds_subgrid: winds_make_after_sf for every listed gas particle
__global__ void __launch_bounds__(256) k_wind_subgrid(const WindView A, const WindScalars S, const int *__restrict__ list, int64_t nlist,
                                                      const double *__restrict__ stellarmass, unsigned *__restrict__ ctr)
{
    const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if(q >= nlist)
        return;
    const int64_t i = list ? list[q] : q;
    const WindKickPar k = wd_params(S, A.a.vdisp[i]);
    const double pw = k.windeff * stellarmass[i] / (double)A.mass[i];
    const double prob = 1 - exp(-pw);
    if(wd_random(S, A.a.id[i] + 2ull) < prob) {
        wd_kick(A, S, i, k.v, k.utherm);
        if(k.v > 0 && S.atime > 0)
            atomicAdd(ctr + CTR_APPLIED, 1u);
    }
}

// winds_evolve for every listed row of type 0
__global__ void __launch_bounds__(256) k_wind_evolve(const WindView A, const mpg_wind_params P, const mpg_sph_times T, const int *__restrict__ list,
                                                     int64_t nlist, unsigned *__restrict__ ctr)
{
    const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if(q >= nlist)
        return;
    const int64_t i = list ? list[q] : q;
    if(i < 0 || i >= A.n) {
        atomicAdd(ctr + CTR_BAD, 1u);
        return;
    }
    if(!A.type || (A.type[i] & 7) != 0) // (no type column: all type 1, as everywhere)
        return;
    const double a3inv = 1 / (T.atime * T.atime * T.atime); // sfr_eff.c:211
    const double before = A.a.delaytime[i], density = A.a.density[i];
    double dtime = 0;
    if(wind_still_delayed(P, before, density, a3inv)) {
        const int bin = A.a.tb_hydro[i];
        if(bin > 46) { // beyond TIMEBINS
            atomicAdd(ctr + CTR_BAD, 1u);
            return;
        }
        dtime = T.dloga_bin[bin] / T.hubble;
    }
    const double dt = wind_evolve_delay(P, before, density, a3inv, dtime);
    if(before > 0)
        A.a.delaytime[i] = dt;
}

void WindsEngine::reset()
{
    last_capacity = 0;
    for(int64_t &s : last_stats)
        s = 0;
    last_maxvel = 0;
    last_ms[0] = last_ms[1] = last_ms[2] = 0;
}

void WindsEngine::check_stars(const WindView &A, const int *d_newstars, int64_t nnew, hipStream_t st)
{
    ctr.reserve(8);
    stats.reserve(8);
    MPG_HIP(hipMemsetAsync(ctr.p, 0, 8 * sizeof(unsigned), st));
    MPG_HIP(hipMemsetAsync(stats.p, 0, 8 * sizeof(unsigned long long), st));
    MPG_HIP(hipMemsetAsync(stats.p + STAT_LOWEST, 0xff, sizeof(unsigned long long), st));
    hipLaunchKernelGGL(k_wind_check, dim3(nblk(nnew)), dim3(256), 0, st, A, d_newstars, nnew, 4, ctr.p);
    MPG_HIP(hipGetLastError());
    unsigned bad = 0;
    MPG_HIP(hipMemcpyAsync(&bad, ctr.p + CTR_BAD, sizeof(bad), hipMemcpyDeviceToHost, st));
    MPG_HIP(hipStreamSynchronize(st));
    MPG_CHECK(bad == 0, "winds_and_feedback: " + std::to_string(bad) + " listed row(s) outside the table or not of type 4 (not a star)");
}

void WindsEngine::run(TreeBuilder &tree, const WindView &A, const WindScalars &S, const int *d_newstars, int64_t nnew, hipStream_t st)
{
    tree.ensure_level_order(st); // the cooperative walk uses the level-ordered copy of the tree
    TreeView tv = tree.view();
    tv.geoS = nullptr; // the asymmetric search keeps the reference's cell test (cull_node), as the density loop does
    MPG_CHECK(tv.npart > 0, "winds_and_feedback: the tree holds no gas particles");
    last_stats[0] = nnew;
    weight.reserve(nnew + 1);
    count.reserve(nnew + 1);
    offset.reserve(nnew + 2);
    for(hipEvent_t &e : ev)
        if(!e)
            MPG_HIP(hipEventCreate(&e));
    unsigned *const err = ctr.p + CTR_ERR;
    MPG_HIP(hipEventRecord(ev[0], st));
    hipLaunchKernelGGL(k_wind_weight, dim3(nblk(nnew, 32)), dim3(256), 0, st, tv, A, d_newstars, nnew, weight.p, count.p, ctr.p, stats.p);
    hipLaunchKernelGGL(k_wind_offsets, dim3(1), dim3(256), 0, st, nnew, count.p, offset.p);
    MPG_HIP(hipEventRecord(ev[1], st));
    MPG_HIP(hipGetLastError());
    unsigned long long hs[2] = {0, 0};
    ngb_read_stats(stats.p, 2, hs, err, "winds_and_feedback", st);
    last_stats[1] = (int64_t)hs[1];
    last_stats[2] = (int64_t)hs[0];
    MPG_HIP(hipEventElapsedTime(&last_ms[0], ev[0], ev[1]));
    if(A.a.kick_star && A.n > 0)
        MPG_HIP(hipMemsetAsync(A.a.kick_star, 0, (size_t)A.n * sizeof(uint64_t), st));
    if(hs[0] == 0) // no eligible neighbour of any star: no candidate of the feedback walk
        return;
    // priv->maxkicks = nvisited + 2, winds.c:316; here a segment of nvisited entries per star
    MPG_CHECK(hs[0] < 0x7fffffffull, "winds_and_feedback: more eligible neighbours than the kick list can index");
    const unsigned capacity = (unsigned)hs[0];
    kicks.reserve(capacity);
    last_capacity = capacity;
    rmin.reserve(tv.npart + 1);
    win.reserve(tv.npart + 1);
    MPG_HIP(hipEventRecord(ev[1], st));
    MPG_HIP(hipMemsetAsync(rmin.p, 0xff, (size_t)tv.npart * sizeof(unsigned long long), st));
    MPG_HIP(hipMemsetAsync(win.p, 0xff, (size_t)tv.npart * sizeof(unsigned long long), st));
    MPG_HIP(hipMemsetAsync(kicks.p, 0xff, (size_t)capacity * sizeof(WindKick), st)); // star = -1: unused
    hipLaunchKernelGGL(k_wind_feedback, dim3(nblk(nnew, 32)), dim3(256), 0, st, tv, A, S, d_newstars, nnew, weight.p, offset.p, kicks.p, capacity, rmin.p, ctr.p);
    MPG_HIP(hipEventRecord(ev[2], st));
    hipLaunchKernelGGL(k_wind_resolve, dim3(nblk(capacity)), dim3(256), 0, st, A, kicks.p, capacity, rmin.p, win.p);
    hipLaunchKernelGGL(k_wind_apply, dim3(nblk(capacity)), dim3(256), 0, st, tv, A, S, kicks.p, capacity, rmin.p, win.p, ctr.p, stats.p);
    MPG_HIP(hipEventRecord(ev[3], st));
    MPG_HIP(hipGetLastError());
    unsigned c[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    unsigned long long lowest = WD_NONE;
    MPG_HIP(hipMemcpyAsync(c, ctr.p, sizeof(c), hipMemcpyDeviceToHost, st));
    MPG_HIP(hipMemcpyAsync(&lowest, stats.p + STAT_LOWEST, sizeof(lowest), hipMemcpyDeviceToHost, st));
    MPG_HIP(hipStreamSynchronize(st));
    MPG_CHECK(c[CTR_ERR] == 0, "winds_and_feedback: neighbour-search stack overflow (tree deeper than the walk supports)");
    // (the feedback walk finds the eligible pairs of the weight walk, or fewer: the reference's endrun(5), :559-561)
    MPG_CHECK(c[CTR_LISTFULL] == 0 && c[CTR_NKICK] <= capacity, "winds_and_feedback: not enough room in the kick queue");
    last_stats[3] = c[CTR_NKICK];
    last_stats[4] = c[CTR_APPLIED];
    last_stats[5] = (int64_t)c[CTR_NKICK] - (int64_t)c[CTR_APPLIED];
    if(lowest != WD_NONE) {
        WindKick k{};
        MPG_HIP(hipMemcpy(&k, kicks.p + (lowest & 0xffffffffull), sizeof(k), hipMemcpyDeviceToHost));
        last_maxvel = k.r;
    }
    MPG_HIP(hipEventElapsedTime(&last_ms[1], ev[1], ev[2]));
    MPG_HIP(hipEventElapsedTime(&last_ms[2], ev[2], ev[3]));
    MPG_CHECK(c[CTR_ODD] == 0, "winds_and_feedback: " + std::to_string(c[CTR_ODD]) + " kick(s) with a non-finite velocity or DelayTime (Odd v)");
}

void WindsEngine::subgrid(const WindView &A, const WindScalars &S, const int *d_list, int64_t nlist, const double *d_stellarmass, hipStream_t st)
{
    ctr.reserve(8);
    MPG_HIP(hipMemsetAsync(ctr.p, 0, 8 * sizeof(unsigned), st));
    // every listed row is a gas particle of the table, checked before anything is written
    hipLaunchKernelGGL(k_wind_check, dim3(nblk(nlist)), dim3(256), 0, st, A, d_list, nlist, 0, ctr.p);
    MPG_HIP(hipGetLastError());
    unsigned c[4] = {0, 0, 0, 0};
    MPG_HIP(hipMemcpyAsync(c, ctr.p, sizeof(unsigned), hipMemcpyDeviceToHost, st));
    MPG_HIP(hipStreamSynchronize(st));
    MPG_CHECK(c[CTR_BAD] == 0, "winds_subgrid: " + std::to_string(c[CTR_BAD]) + " listed row(s) outside the table or not of type 0 (not gas)");
    hipLaunchKernelGGL(k_wind_subgrid, dim3(nblk(nlist)), dim3(256), 0, st, A, S, d_list, nlist, d_stellarmass, ctr.p);
    MPG_HIP(hipGetLastError());
    MPG_HIP(hipMemcpyAsync(c, ctr.p, sizeof(c), hipMemcpyDeviceToHost, st));
    MPG_HIP(hipStreamSynchronize(st));
    last_stats[0] = nlist;
    last_stats[4] = c[CTR_APPLIED];
}

void WindsEngine::evolve(const WindView &A, const WindScalars &S, const mpg_sph_times &T, const int *d_list, int64_t nlist, hipStream_t st)
{
    ctr.reserve(8);
    MPG_HIP(hipMemsetAsync(ctr.p, 0, 8 * sizeof(unsigned), st));
    hipLaunchKernelGGL(k_wind_evolve, dim3(nblk(nlist)), dim3(256), 0, st, A, S.p, T, d_list, nlist, ctr.p);
    MPG_HIP(hipGetLastError());
    unsigned bad = 0;
    MPG_HIP(hipMemcpyAsync(&bad, ctr.p + CTR_BAD, sizeof(bad), hipMemcpyDeviceToHost, st));
    MPG_HIP(hipStreamSynchronize(st));
    MPG_CHECK(bad == 0, "winds_evolve: " + std::to_string(bad) + " listed row(s) outside the table or with a time bin beyond TIMEBINS");
}

} // namespace mpg
