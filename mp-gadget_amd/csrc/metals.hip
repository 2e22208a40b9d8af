// metals.hip -- the return of stellar mass and metals to the gas (metal_return, run.c:613) for gfx950, fp64.
//
// Reference: libgadget/metal_return.c (metals_haswork :714-724, effhsml :778-804, stellar_density_ngbiter :879-928,
// stellar_density_check_neighbours :827-877, stellar_density :930-1006, metal_return_ngbiter :637-709, metal_return_postprocess :623-631)
// and the radius loop of libgadget/treewalk.c (treewalk_do_hsml_loop :1269-1367, ngb_narrow_down :1371-1434: ngb_narrow.h).  The yields of
// a stellar population over the step (metal_return_init, metal_yield) are the caller's: MassGenerated, MetalGenerated and
// MetalSpeciesGenerated arrive as data, as the UV background arrives at the cooling call.
//
// Mapping: the group-cooperative search of ngb_walk.h, 8 lanes per target, over the gas tree the density and hydro loops have just used.
// The targets - stars - are not in that tree: the queue is filled from the particle table, in particle order.  Candidates are gas only; a
// black hole in the tree is skipped.  What a candidate contributes is fixed at call entry and precomputed in tree order (MetalSrc): its
// volume Mass / Density, which the reference's own update leaves unchanged (both are scaled by massfrac, :695-700), and its mass.
//
// k_stellar_density.  A target carries ten trial radii per pass and, per lane, 10 x (sum of kernel values, sum of volumes): 20 fp64 sums.
// Wknorm and kernel_volume depend on the radius alone and multiply the sums after the reduction, so a lane keeps the radius and
// support / radius per trial radius and nothing else.  The reference's shrinking search radius is an optimisation, not part of the result:
// stellar_density_ngbiter sets maxcmpte = i + 1 and the search radius to Hsml[i] as soon as the running Ngb[i] exceeds desnumngb.  The
// weights wk * kernel_volume are non-negative, so a running Ngb[i] never exceeds the complete one, and every particle inside Hsml[i] is
// inside every later search radius: it is still visited after a shrink.  Hence, in any visiting order,
//     maxcmpte = 1 + min{ i : Ngb_i > desnumngb }  (10 if there is none),  Ngb_i the COMPLETE sum at Hsml[i],
//     Ngb[j], VolumeSPH[j] complete for every j < maxcmpte;  entries at and beyond maxcmpte are never read.
// The kernel searches at the largest live trial radius, shrinks only between two batches of opened leaves (as k_vdisp does), and takes
// maxcmpte from the complete sums at the end.  tests/test_gpu_metals.py holds it against a restatement with the literal shrink.
//
// k_metal_scatter / k_metal_apply.  The reference serialises the writers of one gas particle with a spinlock: its result depends on the
// order in which threads arrive, and P.Mass is rounded to float after every contribution.  Here nothing waits: a contribution is accepted
// iff (double)Mass_j(entry) + thismass <= MaxGasMass, accepted contributions are added with fp64 hardware atomics to per-gas accumulators
// (dM, dZ, dMetals[9]; zeroed per call), and one thread per gas particle applies them:
//     Mnew = M + dM,  Metals_k = (Metals_k M + dMetals_k) / Mnew,  Metallicity likewise,  Density *= Mnew / M,  Mass = (float)Mnew.
// In exact arithmetic that is the reference's sequential update (metal mass is additive).  It differs in ONE case: a gas particle that
// several contributions of one call would push over MaxGasMass although each fits alone - there the reference accepts those that arrive
// first, i.e. its own answer depends on thread order; this form accepts all of them.
#include "metals.h"
#include "ngb_walk.h"
#include "ngb_narrow.h"
#include "density_kernel.h"
#include <cmath>
#include <type_traits>

namespace mpg {

#ifndef MT_OCC
// waves per SIMD the launch bound of k_stellar_density asks for.  The compiler's resource report: 2 -> 224 VGPRs, nothing
// spilled; 3 -> 168 VGPRs, 43 spilled; 4 -> 128 VGPRs, 115 spilled (560 bytes of scratch per lane, inside the candidate loop).  Measured
// per pass over 21 k / 210 k targets at 2 x 128^3: 0.42 / 1.98 ms, 0.35 / 1.60 ms, 0.66 / 3.39 ms - the middle form is the default
#define MT_OCC 3
#endif
constexpr int MT_WALK_K = 2;     // child ranges per search step (walk_stepk, ngb_walk.h), as the SPH loops
constexpr bool MT_MERGE = true;  // sibling leaves joined into one list entry
constexpr int MT_ACC = 2 + NMETALS; // accumulators per gas particle: dM, dZ, dMetals[9]

// words of MetalsEngine::ctr: targets, the redo queue's length, targets with Hsml <= 0, targets that end with VolumeSPH == 0, the search's
// overflow flag; words of stats beyond wave_stats' three: contributions refused by the cap
constexpr int CTR_Q = 0, CTR_REDO = 1, CTR_BADH = 2, CTR_ZEROVOL = 3, CTR_ERR = 7;
constexpr int STAT_REFUSED = 3;

// effhsml, metal_return.c:778-804: trial radius i of 10, evenly split in volume between left and right.  (The zero-Hsml repair of
// :786-791 reads the father node of a particle that is not in the tree; a target with Hsml <= 0 is an error of the call instead.)
__device__ __forceinline__ double mt_trial_radius(double left, double right, const double hsml, const double box, const int i)
{
    if(right > 0.99 * box)
        right = hsml * ((1. + NHSML) / NHSML);
    if(left == 0)
        left = 0.1 * hsml;
    const double rvol = pow(right, 3);
    const double lvol = pow(left, 3);
    return pow((1. * i + 1) / (1. * NHSML + 1) * (rvol - lvol) + lvol, 1. / 3);
}

// the kernel polynomial without Wknorm (densitykernel.c:24-90): an exact zero at and beyond the support
__device__ __forceinline__ double mt_wk_poly(const int type, const double q) { return type == 0 ? wk_q<0>(q) : (type == 1 ? wk_q<1>(q) : wk_q<2>(q)); }
// Wknorm * kernel_volume of a trial radius (density_kernel_init, density_kernel_volume): what turns the sum of polynomials into Ngb
__device__ __forceinline__ double mt_ngb_norm(const double H, const int type)
{
    const DKernel k = kernel_init(H, type);
    return k.Wknorm * (NORM_COEFF * p3(H));
}

// what every candidate contributes, once per call, in tree order beside the positions
__global__ void __launch_bounds__(256) k_mt_sources(int64_t npart, const int *__restrict__ order, const MetalView A, MetalSrc *__restrict__ msrc)
{
    const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if(k >= npart)
        return;
    const int64_t ci = order[k];
    const bool gas = (A.type[ci] & 7) == 0;
    const double m = (double)A.mass[ci];
    msrc[k] = MetalSrc{gas ? m / A.density[ci] : -1.0, m};
}

// The queue of both passes: metals_haswork (metal_return.c:714-724) on the active particles; garbage and swallowed rows carry type 7.
// With the initial state of stellar_density (:971-972).
__global__ void __launch_bounds__(256) k_mt_queue(int64_t n, const uint8_t *__restrict__ flags, const MetalView A, const double box, const MetalState W,
                                                  int *__restrict__ queue, unsigned *__restrict__ ctr)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const bool inb = i < n;
    const int ty = (inb && A.type) ? (A.type[i] & 7) : 1;
    bool star = inb && (!flags || flags[i]) && ty == 4;
    if(star && A.massgenerated[i] < 1e-3 * ((double)A.mass[i] + A.totalmassreturned[i]))
        star = false;
    bool badh = false;
    if(star) {
        W.Left[i] = 0;
        W.Right[i] = box;
        W.niter[i] = 0;
        badh = !(A.hsml[i] > 0);
    }
    wave_append(star, (int)i, queue, ctr + CTR_Q);
    const unsigned long long mb = ballot64(badh);
    if(mb != 0 && (threadIdx.x & 63) == 0)
        atomicAdd(ctr + CTR_BADH, (unsigned)__popcll(mb));
}

// One pass of stellar_density over the current queue: treewalk_visit_nolist_ngbiter + stellar_density_ngbiter +
// stellar_density_check_neighbours; unfinished targets are appended to `redo`.
__global__ void __launch_bounds__(256, MT_OCC) k_stellar_density(const TreeView tv, const MetalView A, const MetalScalars S, const MetalState W,
                                                                 const MetalSrc *__restrict__ msrc, const int *__restrict__ queue, int64_t nqueue,
                                                                 int *__restrict__ redo, unsigned *__restrict__ ctr, unsigned long long *__restrict__ stats)
{
    __shared__ unsigned s_stack[4 * 8 * SPH_STK];
    __shared__ unsigned s_llist[4 * 8 * SPH_LCAP];
    NgbGroup g = ngb_group(s_stack, s_llist, nqueue);
    const int s = g.s;
    const bool valid = g.valid;
    unsigned n_int = 0, n_cand = 0;
    int i = 0;
    double px = 0, py = 0, pz = 0;
    double rad[NHSML], hinvs[NHSML]; // per trial radius: H and support / H
    const double support = ksupport(S.ktype);
#pragma unroll
    for(int j = 0; j < NHSML; j++)
        rad[j] = 1.0;
    if(valid) {
        i = queue[g.q];
        px = A.pos[3 * (int64_t)i];
        py = A.pos[3 * (int64_t)i + 1];
        pz = A.pos[3 * (int64_t)i + 2];
        const double hsml = A.hsml[i], L = W.Left[i], R = W.Right[i];
#pragma unroll
        for(int j = 0; j < NHSML; j++)
            rad[j] = mt_trial_radius(L, R, hsml, tv.box, j);
    }
#pragma unroll
    for(int j = 0; j < NHSML; j++)
        hinvs[j] = (1. / rad[j]) * support;
    double hs = valid ? rad[NHSML - 1] : 0.0; // the search radius: the largest live trial radius
    double h2 = hs * hs;
    double N[NHSML], V[NHSML]; // sums of the kernel polynomial and of the (weighted) volumes
#pragma unroll
    for(int j = 0; j < NHSML; j++)
        N[j] = V[j] = 0;
    // the search and the candidate loop, with (WRAP) or without NEAREST(): see interior_wave, ngb_walk.h
    auto loops = [&](auto wrap_tag) {
        constexpr bool WRAP = decltype(wrap_tag)::value;
        ngb_search<false, MT_WALK_K, MT_MERGE, WRAP>(
            tv, tv.geoB, nullptr, g, hs, px, py, pz, [&](const int slot) { return tv.src[slot]; },
            [&](const Src4 &cand, const int slot, const bool live) {
                if(live) {
                    n_cand++;
                    const double d0 = near_img<WRAP>(px - cand.x, tv.box, 1.0 / tv.box);
                    const double d1 = near_img<WRAP>(py - cand.y, tv.box, 1.0 / tv.box);
                    const double d2 = near_img<WRAP>(pz - cand.z, tv.box, 1.0 / tv.box);
                    const double r2 = d0 * d0 + d1 * d1 + d2 * d2;
                    if(!(r2 > h2)) {
                        const double vol = msrc[slot].vol;
                        if(vol >= 0) { // gas only (GASMASK, metal_return.c:893)
                            n_int++;
                            const double r = sqrt(r2);
#pragma unroll
                            for(int j = 0; j < NHSML; j++) {
                                const bool in = r2 < rad[j] * rad[j]; // :904
                                const double p = mt_wk_poly(S.ktype, r * hinvs[j]);
                                N[j] += in ? p : 0.0;
                                V[j] += in ? (S.sphweight ? vol * p : vol) : 0.0;
                            }
                        }
                    }
                }
            },
            [&] {
                // between two batches: a partial Ngb above desnumngb at rad[j] means the complete one is too (non-negative weights), so nothing
                // beyond rad[j] can reach an entry that is read (the header's argument)
#pragma unroll
                for(int j = NHSML - 1; j >= 0; j--)
                    if(mt_ngb_norm(rad[j], S.ktype) * group_sum(N[j]) > S.desnumngb && rad[j] < hs)
                        hs = rad[j];
                h2 = hs * hs;
            });
    };
    if(interior_wave(valid, px, py, pz, hs, tv.box))
        loops(std::false_type{});
    else
        loops(std::true_type{});
    if(ngb_overflowed(g, ctr + CTR_ERR))
        return;
    double num[NHSML];
#pragma unroll
    for(int j = 0; j < NHSML; j++) {
        num[j] = group_sum(N[j]);
        V[j] = group_sum(V[j]);
    }
    bool notdone = false, tight = false;
    if(valid && s == 0) { // stellar_density_check_neighbours, metal_return.c:827-877
#pragma unroll
        for(int j = 0; j < NHSML; j++)
            num[j] *= mt_ngb_norm(rad[j], S.ktype);
        int maxcmpt = NHSML; // from the COMPLETE sums (the header's argument)
#pragma unroll
        for(int j = NHSML - 1; j >= 0; j--)
            if(num[j] > S.desnumngb)
                maxcmpt = j + 1;
        int close = 0;
        double L = W.Left[i], R = W.Right[i];
        // (the reference's parameter is `int desnumngb`: the neighbour number is truncated inside ngb_narrow_down and only there)
        const double newhsml = ngb_narrow_down<NHSML>(R, L, rad, num, maxcmpt, (int)S.desnumngb, tv.box, close);
        const double numngb = ngb_pick(num, close);
        const double hclose = ngb_pick(rad, close);
        // VolumeSPH[0] = VolumeSPH[close] (:848): the saved volume belongs to trial radius `close`, not to the new Hsml
        const double volume = ngb_pick(V, close) * (S.sphweight ? kernel_init(hclose, S.ktype).Wknorm : 1.0);
        A.hsml[i] = newhsml; // assigned on every pass, the converged one too (:844)
        W.Left[i] = L;
        W.Right[i] = R;
        W.Volume[i] = volume;
        W.evalradius[i] = hclose;
        W.niter[i] = W.niter[i] + 1;
        W.maxcmpte[i] = maxcmpt;
        W.close[i] = close;
        const bool off = numngb < (S.desnumngb - S.maxdev) || numngb > (S.desnumngb + S.maxdev);
        if(off && !((R - L) < 1.0e-4 * L))
            notdone = true;
        else {
            tight = off; // ended through the narrow bracket, not through the neighbour number
            if(volume == 0) // the reference's endrun(3), :988-989
                atomicAdd(ctr + CTR_ZEROVOL, 1u);
        }
    }
    wave_append(notdone, i, redo, ctr + CTR_REDO);
    wave_stats(stats, n_int, n_cand, tight);
}

// The return walk: one pass at the final Hsml over the gas around every target, metal_return_ngbiter (:637-709) with the cap taken at the
// entry mass, and metal_return_postprocess (:623-631) for the target itself.
__global__ void __launch_bounds__(256, 4) k_metal_scatter(const TreeView tv, const MetalView A, const MetalScalars S, const MetalState W,
                                                          const MetalSrc *__restrict__ msrc, const int *__restrict__ queue, int64_t nqueue,
                                                          double *__restrict__ acc, unsigned *__restrict__ ctr, unsigned long long *__restrict__ stats)
{
    __shared__ unsigned s_stack[4 * 8 * SPH_STK];
    __shared__ unsigned s_llist[4 * 8 * SPH_LCAP];
    NgbGroup g = ngb_group(s_stack, s_llist, nqueue);
    const bool valid = g.valid;
    unsigned n_int = 0, n_cand = 0, n_refused = 0;
    int i = 0;
    double px = 0, py = 0, pz = 0, hsml = 0, massgen = 0, metalgen = 0, starvol = 0;
    if(valid) {
        i = queue[g.q];
        px = A.pos[3 * (int64_t)i];
        py = A.pos[3 * (int64_t)i + 1];
        pz = A.pos[3 * (int64_t)i + 2];
        hsml = A.hsml[i];
        massgen = A.massgenerated[i];
        metalgen = A.metalgenerated[i];
        starvol = W.Volume[i];
    }
    const double *__restrict__ species = A.speciesgenerated + (int64_t)NMETALS * i;
    const DKernel kern = kernel_init(valid ? hsml : 1.0, S.ktype);
    double massreturn = 0;
    auto loops = [&](auto wrap_tag) {
        constexpr bool WRAP = decltype(wrap_tag)::value;
        ngb_search<false, MT_WALK_K, MT_MERGE, WRAP>(
            tv, tv.geoB, nullptr, g, hsml, px, py, pz, [&](const int slot) { return tv.src[slot]; },
            [&](const Src4 &cand, const int slot, const bool live) {
                if(live) {
                    n_cand++;
                    const double d0 = near_img<WRAP>(px - cand.x, tv.box, 1.0 / tv.box);
                    const double d1 = near_img<WRAP>(py - cand.y, tv.box, 1.0 / tv.box);
                    const double d2 = near_img<WRAP>(pz - cand.z, tv.box, 1.0 / tv.box);
                    const double r2 = d0 * d0 + d1 * d1 + d2 * d2;
                    if(r2 > 0 && r2 < kern.HH) { // :660
                        const MetalSrc o = msrc[slot];
                        if(o.vol >= 0) { // gas only
                            n_int++;
                            const double wk = S.sphweight ? kernel_wk(kern, S.ktype, sqrt(r2) * kern.Hinv) : 1.0;
                            const double returnfraction = wk * o.vol / starvol;
                            const double thismass = returnfraction * massgen;
                            if(o.mass + thismass > S.maxgasmass) // :680, on the mass of call entry
                                n_refused++;
                            else {
                                double *__restrict__ a = acc + (int64_t)MT_ACC * slot;
                                unsafeAtomicAdd(a, thismass);
                                unsafeAtomicAdd(a + 1, returnfraction * metalgen);
#pragma unroll
                                for(int k = 0; k < NMETALS; k++)
                                    unsafeAtomicAdd(a + 2 + k, returnfraction * species[k]);
                                massreturn += thismass;
                            }
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
    massreturn = group_sum(massreturn);
    if(valid && g.s == 0) { // metal_return_postprocess
        A.mass[i] = (float)((double)A.mass[i] - massreturn);
        A.totalmassreturned[i] += massreturn;
        A.lastenrichment[i] = A.stellarage[i];
        if(A.massreturned)
            A.massreturned[i] = massreturn;
        if(A.starvolume)
            A.starvolume[i] = starvol;
    }
    unsigned long long nr = n_refused;
    for(int off = 32; off > 0; off >>= 1)
        nr += __shfl_down(nr, off);
    if(g.lane == 0 && nr != 0)
        atomicAdd(&stats[STAT_REFUSED], nr);
    wave_stats(stats, n_int, n_cand);
}

// the accumulated contributions into the gas, one thread per particle of the tree
__global__ void __launch_bounds__(256) k_metal_apply(int64_t npart, const int *__restrict__ order, const MetalView A, const double *__restrict__ acc)
{
    const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if(k >= npart)
        return;
    const double *__restrict__ a = acc + (int64_t)MT_ACC * k;
    const double dM = a[0];
    if(!(dM > 0))
        return;
    const int64_t ci = order[k];
    const double M = (double)A.mass[ci], Mnew = M + dM;
    for(int j = 0; j < NMETALS; j++)
        A.metals[NMETALS * ci + j] = (A.metals[NMETALS * ci + j] * M + a[2 + j]) / Mnew;
    A.metallicity[ci] = (A.metallicity[ci] * M + a[1]) / Mnew;
    A.density[ci] *= Mnew / M;
    A.mass[ci] = (float)Mnew;
}

__global__ void __launch_bounds__(256) k_mt_star_hsml(int64_t n, const uint8_t *__restrict__ type, const double *__restrict__ src, double *__restrict__ dst)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if(i < n && (type[i] & 7) == 4)
        dst[i] = src[i];
}

void MetalsEngine::take_star_hsml(double *dst, const double *src, const uint8_t *type, int64_t n, hipStream_t st)
{
    if(n > 0 && type)
        hipLaunchKernelGGL(k_mt_star_hsml, dim3(nblk(n)), dim3(256), 0, st, n, type, src, dst);
    MPG_HIP(hipGetLastError());
}

int64_t MetalsEngine::make_queue(const MetalView &A, const MetalScalars &S, const uint8_t *active_flags, int64_t n, hipStream_t st)
{
    left.reserve(n + 1);
    right.reserve(n + 1);
    volume.reserve(n + 1);
    evalradius.reserve(n + 1);
    niter.reserve(n + 1);
    maxcmpte.reserve(n + 1);
    close.reserve(n + 1);
    queue_0.reserve(n + 1);
    ctr.reserve(8);
    stats.reserve(8);
    n_state = n;
    MPG_HIP(hipMemsetAsync(ctr.p, 0, 8 * sizeof(unsigned), st));
    MPG_HIP(hipMemsetAsync(stats.p, 0, 8 * sizeof(unsigned long long), st));
    MPG_HIP(hipMemsetAsync(niter.p, 0xff, (size_t)(n + 1) * sizeof(int), st)); // -1: not a target of this call
    if(n > 0)
        hipLaunchKernelGGL(k_mt_queue, dim3(nblk(n)), dim3(256), 0, st, n, active_flags, A, S.box, state(), queue_0.p, ctr.p);
    MPG_HIP(hipGetLastError());
    unsigned c[3] = {0, 0, 0};
    MPG_HIP(hipMemcpyAsync(c, ctr.p, sizeof(c), hipMemcpyDeviceToHost, st));
    MPG_HIP(hipStreamSynchronize(st));
    ntargets = c[CTR_Q];
    last_iterations = last_targets = last_neighbours = last_candidates = last_refused = last_tight = 0;
    last_ms[0] = last_ms[1] = last_ms[2] = 0;
    queue_lengths.clear();
    MPG_CHECK(c[CTR_BADH] == 0, "metal_return: " + std::to_string(c[CTR_BADH]) + " returning star(s) with Hsml <= 0 (the caller repairs Hsml before the call)");
    return ntargets;
}

void MetalsEngine::run(TreeBuilder &tree, const MetalView &A, const MetalScalars &S, int64_t n, hipStream_t st)
{
    tree.ensure_level_order(st); // the cooperative walk uses the level-ordered copy of the tree
    TreeView tv = tree.view();
    tv.geoS = nullptr; // the asymmetric search keeps the reference's cell test (cull_node), as the density loop does
    MPG_CHECK(tv.npart > 0, "metal_return: the tree holds no gas particles");
    msrc.reserve(tv.npart + 1);
    acc.reserve((size_t)MT_ACC * tv.npart + 1);
    queue_a.reserve(n + 1);
    queue_b.reserve(n + 1);
    hipLaunchKernelGGL(k_mt_sources, dim3(nblk(tv.npart)), dim3(256), 0, st, tv.npart, tv.order, A, msrc.p);
    // the radius loop consumes its queues; the return walk takes the targets again
    MPG_HIP(hipMemcpyAsync(queue_a.p, queue_0.p, (size_t)ntargets * sizeof(int), hipMemcpyDeviceToDevice, st));
    const MetalState W = state();
    unsigned *const nredo = ctr.p + CTR_REDO, *const err = ctr.p + CTR_ERR;
    for(hipEvent_t &e : ev)
        if(!e)
            MPG_HIP(hipEventCreate(&e));
    MPG_HIP(hipEventRecord(ev[0], st));
    ngb_hsml_loop(queue_a.p, queue_b.p, (unsigned)ntargets, nredo, err, MT_MAXITER, "metal_return", st, last_iterations, last_targets, &queue_lengths,
                  [&](const int *queue, const unsigned nqueue, int *redo) {
                      hipLaunchKernelGGL(k_stellar_density, dim3(nblk(nqueue, 32)), dim3(256), 0, st, tv, A, S, W, msrc.p, queue, (int64_t)nqueue, redo,
                                         ctr.p, stats.p);
                  });
    unsigned zerovol = 0;
    MPG_HIP(hipMemcpyAsync(&zerovol, ctr.p + CTR_ZEROVOL, sizeof(unsigned), hipMemcpyDeviceToHost, st));
    MPG_HIP(hipStreamSynchronize(st));
    MPG_CHECK(zerovol == 0, "metal_return: " + std::to_string(zerovol) + " returning star(s) with StarVolumeSPH == 0 (no gas inside the final radius)");
    MPG_HIP(hipEventRecord(ev[1], st));
    MPG_HIP(hipMemsetAsync(acc.p, 0, (size_t)MT_ACC * tv.npart * sizeof(double), st));
    hipLaunchKernelGGL(k_metal_scatter, dim3(nblk(ntargets, 32)), dim3(256), 0, st, tv, A, S, W, msrc.p, queue_0.p, ntargets, acc.p, ctr.p, stats.p);
    MPG_HIP(hipEventRecord(ev[2], st));
    hipLaunchKernelGGL(k_metal_apply, dim3(nblk(tv.npart)), dim3(256), 0, st, tv.npart, tv.order, A, acc.p);
    MPG_HIP(hipEventRecord(ev[3], st));
    MPG_HIP(hipGetLastError());
    unsigned long long hs[4] = {0, 0, 0, 0};
    ngb_read_stats(stats.p, 4, hs, err, "metal_return", st);
    last_neighbours = (int64_t)hs[0];
    last_candidates = (int64_t)hs[1];
    last_tight = (int64_t)hs[2];
    last_refused = (int64_t)hs[STAT_REFUSED];
    for(int k = 0; k < 3; k++)
        MPG_HIP(hipEventElapsedTime(&last_ms[k], ev[k], ev[k + 1]));
}

} // namespace mpg
