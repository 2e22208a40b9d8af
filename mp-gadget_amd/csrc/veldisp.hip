// veldisp.hip -- the one-dimensional DM velocity dispersion around star-forming gas (SphP.VDisp) and black holes (BHP.VDisp)
// for gfx950, fp64.
//
// Reference: libgadget/veldisp.c (winds_find_vel_disp :375-466, wind_vdisp_ngbiter :233-284, wind_vdisp_postprocess :305-346,
// vdispeffdmradius :204-219, winds_veldisp_haswork :348-371, blackhole_veldisp :59-168), the neighbour visitor and the radius loop of
// libgadget/treewalk.c (treewalk_visit_nolist_ngbiter :1152-1265, treewalk_do_hsml_loop :1269-1367, ngb_narrow_down :1371-1434) and
// DM_VelPred (density.c:106-112).
//
// Mapping: the group-cooperative search of ngb_walk.h, 8 lanes per target as in the SPH loops, over a tree of the DM particles
// alone.  The targets - gas and black holes - are not in that tree: the queues are filled from the particle table, in particle
// order (the reference keeps its table in (type, Peano-Hilbert key) order, so neighbours in the queue are neighbours in space).
// A gas target carries five trial radii per pass and 5 x (count, V2, V1[3]) per lane: 20 fp64 sums and 5 integer counts.
//
// The reference's shrinking search radius is an optimisation, not part of the result.  wind_vdisp_ngbiter sets maxcmpte = i + 1 and
// the search radius to DMRadius[i] as soon as the running Ngb[i] exceeds 40, scanning i from 0 at every neighbour.  A running count
// never exceeds the complete one, and every particle inside DMRadius[i] is inside every later search radius, so it is still visited
// after a shrink.  The final state therefore does not depend on the visiting order:
//     maxcmpte = 1 + min{ i : N_i > 40 }  (5 if there is none),  N_i the COMPLETE count inside DMRadius[i],
//     Ngb[j], V1sum[j], V2sum[j] complete for every j < maxcmpte;  entries at and beyond maxcmpte are never read.
// k_vdisp searches at the largest live trial radius, tests the candidates in the order the cooperative walk delivers them, shrinks the
// radius only between two batches of opened leaves (when a partial count already exceeds 40: the complete one does too), and takes
// maxcmpte from the complete counts at the end.  tests/test_gpu_veldisp.py holds it against a restatement that walks in a fixed
// order with the reference's literal shrink; tests/test_veldisp_restated.py shows the restatement itself independent of the order.
#include "veldisp.h"
#include "ngb_walk.h"
#include "ngb_narrow.h"
#include <cmath>
#include <type_traits>

namespace mpg {

#ifndef VD_K
#define VD_K 2
#endif
#ifndef VD_OCC
#define VD_OCC 4
#endif
constexpr int VD_WALK_K = VD_K;     // child ranges per search step (walk_stepk, ngb_walk.h), as the SPH loops
constexpr bool VD_MERGE = true;  // sibling leaves joined into one list entry

// vdispeffdmradius, veldisp.c:204-219: trial radius i of 5, evenly split in volume between left and right
__device__ __forceinline__ double vd_trial_radius(double left, double right, const double dmradius, const double box, const int i)
{
    if(right > 0.99 * box)
        right = dmradius;
    if(left == 0)
        left = 0.1 * dmradius;
    const double rvol = pow(right, 3);
    const double lvol = pow(left, 3);
    return pow((1.0 * i + 1) / (1.0 * NWINDHSML + 1) * (rvol - lvol) + lvol, 1. / 3);
}

// ngb_narrow_down for the 5 radii and desnumngb = 40 of this loop: ngb_narrow.h
__device__ __forceinline__ double vd_pick(const double (&a)[NWINDHSML], const int k) { return ngb_pick<NWINDHSML>(a, k); }
__device__ __forceinline__ double vd_narrow_down(double &right, double &left, const double (&radius)[NWINDHSML], const double (&num)[NWINDHSML],
                                                 const int maxcmpt, const double box, int &closeidx)
{
    return ngb_narrow_down<NWINDHSML>(right, left, radius, num, maxcmpt, NUMDMNGB, box, closeidx);
}

// DM_VelPred (density.c:106-112) of every particle of the DM tree, once per call, in tree order beside the positions
__global__ void __launch_bounds__(256) k_vd_predict(int64_t npart, const int *__restrict__ order, const VdispView A, const mpg_sph_times T,
                                                    Aux4 *__restrict__ velpred)
{
    const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if(k >= npart)
        return;
    const int64_t ci = order[k];
    const int bg = A.tb_grav ? A.tb_grav[ci] : 0;
    double v[3];
    for(int j = 0; j < 3; j++)
        v[j] = A.vel[3 * ci + j] + T.gravkicks[bg] * (A.gacc ? A.gacc[3 * ci + j] : 0.0) + (A.gpm ? A.gpm[3 * ci + j] : 0.0) * T.FgravkickB;
    velpred[k] = Aux4{v[0], v[1], v[2], 0.0};
}

// The two queues of winds_find_vel_disp: the gas of winds_veldisp_haswork (veldisp.c:348-371; garbage and swallowed particles carry
// type 7) with the initial state of :441-450, and the active black holes (blackhole_dynfric_haswork :53-57).
// Words of VdispEngine::ctr: gas targets, black-hole targets, black holes in the table, active or not (totbh, :409), the redo queue's
// length, the search's overflow flag.
constexpr int CTR_GAS = 0, CTR_BH = 1, CTR_TOTBH = 2, CTR_REDO = 3, CTR_ERR = 7;
__global__ void __launch_bounds__(256) k_vd_queues(int64_t n, const uint8_t *__restrict__ flags, const VdispView A, const VdispScalars S,
                                                   const VdispState W, int *__restrict__ queue_gas, int *__restrict__ queue_bh,
                                                   unsigned *__restrict__ ctr)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const bool inb = i < n;
    const int ty = (inb && A.type) ? (A.type[i] & 7) : 1;
    const bool act = inb && (!flags || flags[i]);
    bool gas = act && ty == 0;
    if(gas) {
        const double hsml = A.hsml[i];
        double densfac = (hsml + (A.dthsml ? A.dthsml[i] : 0.0) * S.ddrift) / hsml;
        if(densfac > 1)
            densfac = 1;
        if(A.density[i] / (densfac * densfac * densfac) < S.dens_threshold)
            gas = false;
        else {
            W.DMRadius[i] = hsml;
            W.Left[i] = 0;
            W.Right[i] = S.box;
            W.niter[i] = 0;
        }
    }
    const bool bh = act && ty == 5;
    if(bh)
        W.niter[i] = 0;
    wave_append(gas, (int)i, queue_gas, ctr + CTR_GAS);
    wave_append(bh, (int)i, queue_bh, ctr + CTR_BH);
    const unsigned long long mb = ballot64(inb && ty == 5);
    if(mb != 0 && (threadIdx.x & 63) == 0)
        atomicAdd(ctr + CTR_TOTBH, (unsigned)__popcll(mb));
}

// One pass over the current queue.  BH = false: treewalk_visit_nolist_ngbiter + wind_vdisp_ngbiter + wind_vdisp_postprocess for the
// gas targets, unfinished targets appended to `redo`.  BH = true: the single pass of blackhole_veldisp (one radius, Hsml; no Hubble
// term; nothing to redo).
template <bool BH>
__global__ void __launch_bounds__(256, VD_OCC) k_vdisp(const TreeView tv, const VdispView A, const VdispScalars S, const VdispState W,
                                                  const Aux4 *__restrict__ velpred, const int *__restrict__ queue, int64_t nqueue,
                                                  int *__restrict__ redo, unsigned *__restrict__ nredo, unsigned long long *__restrict__ stats,
                                                  unsigned *__restrict__ err)
{
    constexpr int NR = BH ? 1 : NWINDHSML;
    __shared__ unsigned s_stack[4 * 8 * SPH_STK];
    __shared__ unsigned s_llist[4 * 8 * SPH_LCAP];
    NgbGroup g = ngb_group(s_stack, s_llist, nqueue);
    const int s = g.s;
    const int64_t q = g.q;
    const bool valid = g.valid;
    unsigned n_int = 0, n_cand = 0;
    int i = 0;
    double px = 0, py = 0, pz = 0;
    double ivel[3] = {0, 0, 0};
    double rad[NR];
    double L = 0, R = 0;
#pragma unroll
    for(int j = 0; j < NR; j++)
        rad[j] = 0;
    if(valid) {
        i = queue[q];
        px = A.pos[3 * (int64_t)i];
        py = A.pos[3 * (int64_t)i + 1];
        pz = A.pos[3 * (int64_t)i + 2];
        ivel[0] = A.vel[3 * (int64_t)i]; // the target's own velocity is the raw Vel (wind_vdisp_copy, blackhole_veldisp_copy)
        ivel[1] = A.vel[3 * (int64_t)i + 1];
        ivel[2] = A.vel[3 * (int64_t)i + 2];
        if(BH)
            rad[0] = A.hsml[i];
        else {
            const double D = W.DMRadius[i];
            L = W.Left[i];
            R = W.Right[i];
#pragma unroll
            for(int j = 0; j < NR; j++)
                rad[j] = vd_trial_radius(L, R, D, tv.box, j);
        }
    }
    double hs = rad[NR - 1]; // the search radius: the largest live trial radius
    double h2 = hs * hs;
    const double HH = rad[0] * rad[0]; // (BH: feedback_kernel.HH)
    int cnt[NR];
    double V2[NR], V1x[NR], V1y[NR], V1z[NR];
#pragma unroll
    for(int j = 0; j < NR; j++) {
        cnt[j] = 0;
        V2[j] = V1x[j] = V1y[j] = V1z[j] = 0;
    }
    // the search and the candidate loop, with (WRAP) or without NEAREST(): see interior_wave, ngb_walk.h
    auto loops = [&](auto wrap_tag) {
        constexpr bool WRAP = decltype(wrap_tag)::value;
        ngb_search<false, VD_WALK_K, VD_MERGE, WRAP>(
            tv, tv.geoB, nullptr, g, hs, px, py, pz, [&](const int slot) { return tv.src[slot]; },
            [&](const Src4 &cand, const int slot, const bool live) {
                if(live) {
                    n_cand++;
                    // the distance vector points to 'other': I.Pos - P[other].Pos (treewalk.c:1223-1233)
                    const double d0 = near_img<WRAP>(px - cand.x, tv.box, 1.0 / tv.box);
                    const double d1 = near_img<WRAP>(py - cand.y, tv.box, 1.0 / tv.box);
                    const double d2 = near_img<WRAP>(pz - cand.z, tv.box, 1.0 / tv.box);
                    const double r2 = d0 * d0 + d1 * d1 + d2 * d2;
                    if(!(r2 > h2)) {
                        n_int++;
                        const Aux4 o = velpred[slot];
                        double v0 = o.x - ivel[0], v1 = o.y - ivel[1], v2 = o.z - ivel[2];
                        if(!BH) { // the Hubble flow of the separation (veldisp.c:265)
                            v0 += S.hubble_a2 * d0;
                            v1 += S.hubble_a2 * d1;
                            v2 += S.hubble_a2 * d2;
                        }
                        const double vv = v0 * v0 + v1 * v1 + v2 * v2;
                        const double r = sqrt(r2);
#pragma unroll
                        for(int j = 0; j < NR; j++) {
                            const bool in = BH ? (r2 < HH) : (r < rad[j]); // veldisp.c:96, :257
                            cnt[j] += in ? 1 : 0;
                            V2[j] += in ? vv : 0.0;
                            V1x[j] += in ? v0 : 0.0;
                            V1y[j] += in ? v1 : 0.0;
                            V1z[j] += in ? v2 : 0.0;
                        }
                    }
                }
            },
            [&] {
                if(!BH) {
                    // between two batches: a partial count above 40 inside rad[j] means the complete one is too, so nothing beyond rad[j] can
                    // reach an entry that is read (the header's argument); the nodes already on the LIFO were kept by a larger radius
#pragma unroll
                    for(int j = NR - 1; j >= 0; j--)
                        if(group_sum_int(cnt[j]) > NUMDMNGB && rad[j] < hs)
                            hs = rad[j];
                    h2 = hs * hs;
                }
            });
    };
    if(interior_wave(valid, px, py, pz, hs, tv.box))
        loops(std::false_type{});
    else
        loops(std::true_type{});
    if(ngb_overflowed(g, err))
        return;
    // sum over the 8 lanes of the group
    double num[NWINDHSML] = {0, 0, 0, 0, 0};
#pragma unroll
    for(int j = 0; j < NR; j++) {
        num[j] = (double)group_sum_int(cnt[j]);
        V2[j] = group_sum(V2[j]);
        V1x[j] = group_sum(V1x[j]);
        V1y[j] = group_sum(V1y[j]);
        V1z[j] = group_sum(V1z[j]);
    }
    bool notdone = false, tight = false;
    if(valid && s == 0) {
        if constexpr(BH) { // blackhole_veldisp_postprocess, veldisp.c:59-76
            const double numdm = num[0];
            if(numdm > 0) {
                double vdisp = V2[0] / numdm;
                vdisp -= pow(V1x[0] / numdm, 2);
                vdisp -= pow(V1y[0] / numdm, 2);
                vdisp -= pow(V1z[0] / numdm, 2);
                if(vdisp > 0)
                    A.vdisp[i] = sqrt(vdisp / 3);
            }
            W.niter[i] = 1;
            W.ngb[i] = (int)numdm;
            W.maxcmpte[i] = 1;
            W.evalradius[i] = rad[0];
        }
        else { // wind_vdisp_postprocess, veldisp.c:305-346
            int maxcmpt = NWINDHSML; // from the COMPLETE counts (the header's argument)
#pragma unroll
            for(int j = NWINDHSML - 1; j >= 0; j--)
                if(num[j] > NUMDMNGB)
                    maxcmpt = j + 1;
            int close = 0;
            L = W.Left[i]; // (read again rather than kept in registers through the search)
            R = W.Right[i];
            const double newradius = vd_narrow_down(R, L, rad, num, maxcmpt, tv.box, close);
            const double numngb = vd_pick(num, close);
            W.DMRadius[i] = newradius;
            W.Left[i] = L;
            W.Right[i] = R;
            W.niter[i] = W.niter[i] + 1;
            W.ngb[i] = (int)numngb;
            W.maxcmpte[i] = maxcmpt;
            W.evalradius[i] = vd_pick(rad, close);
            const bool off = numngb < (NUMDMNGB - 1) || numngb > (NUMDMNGB + 1); // MAXDMDEVIATION = 1
            if(off && (R - L > 5e-6 * L))
                notdone = true;
            else {
                tight = off; // ended through the narrow bracket, not through the count
                double vdisp = vd_pick(V2, close) / numngb;
                vdisp -= pow(vd_pick(V1x, close) / numngb, 2);
                vdisp -= pow(vd_pick(V1y, close) / numngb, 2);
                vdisp -= pow(vd_pick(V1z, close) / numngb, 2);
                if(vdisp > 0)
                    A.vdisp[i] = sqrt(vdisp / 3);
            }
        }
    }
    if(!BH)
        wave_append(notdone, i, redo, nredo); // the unfinished targets
    // statistics: candidates inside the search radius, candidates tested, targets that ended through the tight bracket
    wave_stats(stats, n_int, n_cand, tight);
}

bool VdispEngine::make_queues(const VdispView &A, const VdispScalars &S, const uint8_t *active_flags, int64_t n, hipStream_t st)
{
    left.reserve(n + 1);
    right.reserve(n + 1);
    dmradius.reserve(n + 1);
    evalradius.reserve(n + 1);
    niter.reserve(n + 1);
    ngb.reserve(n + 1);
    maxcmpte.reserve(n + 1);
    queue_a.reserve(n + 1);
    queue_b.reserve(n + 1);
    queue_bh.reserve(n + 1);
    ctr.reserve(8);
    stats.reserve(8);
    n_state = n;
    MPG_HIP(hipMemsetAsync(ctr.p, 0, 8 * sizeof(unsigned), st));
    MPG_HIP(hipMemsetAsync(stats.p, 0, 8 * sizeof(unsigned long long), st));
    MPG_HIP(hipMemsetAsync(niter.p, 0xff, (size_t)(n + 1) * sizeof(int), st)); // -1: not a target of this call
    if(n > 0)
        hipLaunchKernelGGL(k_vd_queues, dim3(nblk(n)), dim3(256), 0, st, n, active_flags, A, S, state(), queue_a.p, queue_bh.p, ctr.p);
    MPG_HIP(hipGetLastError());
    unsigned c[3] = {0, 0, 0};
    MPG_HIP(hipMemcpyAsync(c, ctr.p, sizeof(c), hipMemcpyDeviceToHost, st));
    MPG_HIP(hipStreamSynchronize(st));
    ngas = c[CTR_GAS];
    nbh = c[CTR_BH];
    nbh_exist = c[CTR_TOTBH];
    last_iterations = last_targets = last_neighbours = last_candidates = last_tight = 0;
    queue_lengths.clear();
    return ngas > 0 || nbh_exist > 0; // veldisp.c:413
}

void VdispEngine::search(TreeBuilder &tree, const VdispView &A, const mpg_sph_times &T, const VdispScalars &S, hipStream_t st)
{
    tree.ensure_level_order(st); // the cooperative walk uses the level-ordered copy of the tree
    TreeView tv = tree.view();
    tv.geoS = nullptr; // the asymmetric search keeps the reference's cell test (cull_node), as the density loop does
    MPG_CHECK(tv.npart > 0, "find_vel_disp: the tree holds no dark matter particles");
    velpred.reserve(tv.npart + 1);
    hipLaunchKernelGGL(k_vd_predict, dim3(nblk(tv.npart)), dim3(256), 0, st, tv.npart, tv.order, A, T, velpred.p);
    const VdispState W = state();
    // the black holes first (veldisp.c:419-421): one pass
    if(nbh > 0)
        hipLaunchKernelGGL(k_vdisp<true>, dim3(nblk(nbh, 32)), dim3(256), 0, st, tv, A, S, W, velpred.p, queue_bh.p, nbh, (int *)nullptr,
                           (unsigned *)nullptr, stats.p, ctr.p + CTR_ERR);
    MPG_HIP(hipGetLastError());
    unsigned *const nredo = ctr.p + CTR_REDO, *const err = ctr.p + CTR_ERR;
    ngb_hsml_loop(queue_a.p, queue_b.p, (unsigned)ngas, nredo, err, VD_MAXITER, "find_vel_disp", st, last_iterations, last_targets, &queue_lengths,
                  [&](const int *queue, const unsigned nqueue, int *redo) {
                      hipLaunchKernelGGL(k_vdisp<false>, dim3(nblk(nqueue, 32)), dim3(256), 0, st, tv, A, S, W, velpred.p, queue, (int64_t)nqueue, redo,
                                         nredo, stats.p, err);
                  });
    unsigned long long hs[3] = {0, 0, 0};
    ngb_read_stats(stats.p, 3, hs, err, "find_vel_disp", st);
    last_neighbours = (int64_t)hs[0];
    last_candidates = (int64_t)hs[1];
    last_tight = (int64_t)hs[2];
}

} // namespace mpg
