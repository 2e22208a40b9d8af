// dynfric.hip -- black-hole dynamical friction and the potential minimum of repositioning (blackhole_dynfric + blackhole_dfaccel, the
// first two calls of blackhole(), blackhole.c:254-256) for gfx950, fp64.
//
// Reference: libgadget/bhdynfric.c (blackhole_dynfric_treemask :66-81, blackhole_compute_dfaccel :86-145, blackhole_dynfric_postprocess
// :147-164, blackhole_repos_reduce :166-180, blackhole_minpot_ngbiter :199-231, blackhole_dynfric_ngbiter :233-270,
// blackhole_minpot_preprocess :273-286, blackhole_dynfric_haswork :323-328), SPH_VelPred / DM_VelPred (density.c:89-112).
//
// Mapping: the group-cooperative search of ngb_walk.h with the ASYMMETRIC radius Hsml, 8 lanes per target, over the cells of the tree
// (tv.geoB) as k_vdisp<true> does - the eighth caller of ngb_search.  The targets are hundreds to thousands, the tree holds millions: what a
// candidate needs beyond its position and mass - type, Potential, velocity, accelerations, bins - is gathered from the caller's arrays in
// particle order, and only for the candidates that pass the distance test (as blackhole.hip does); a velocity prediction of every particle
// of the tree, as k_vd_predict makes for the many gas targets of find_vel_disp, would cost more than the walk.
//
// The potential minimum.  A lane keeps the lowest (Potential, particle index) among the candidates it visits that lie strictly below the
// target's own Potential; the 8 lanes are reduced with the same order.  The reference keeps, of several neighbours with the SAME lowest
// potential, the one it visits first; here the one of smaller particle index wins.  That is the one defined difference.
//
// Every loop is bounded: the only loop is ngb_search's, bounded by the tree; ngb_overflowed is the error exit.
//
// Races.  k_dynfric writes rows of its own target only (and the statistics); what it reads of other rows (Potential, Vel, accelerations)
// it does not write.  k_dfaccel reads and writes the rows of its own black hole.
#include "dynfric.h"
#include "ngb_walk.h"
#include "density_kernel.h"
#include <cmath>
#include <type_traits>

namespace mpg {

constexpr int DF_WALK_K = 2;    // child ranges per search step (walk_stepk, ngb_walk.h), as the SPH loops
constexpr bool DF_MERGE = true; // sibling leaves joined into one list entry

// words of DynfricEngine::ctr: targets, listed black holes, ZeroDF, a non-finite bhvel, the search's overflow flag
constexpr int CTR_T = 0, CTR_BH = 1, CTR_ZERO = 2, CTR_BAD = 3, CTR_ERR = 7;

// SPH_VelPred (density.c:89-99; HYDRO) / DM_VelPred (:106-112), component k
template <bool HYDRO> __device__ __forceinline__ double df_velpred(const mpg_bh_dynfric_arrays &a, const mpg_sph_times &T, const int64_t i, const int k)
{
    double v = a.vel[3 * i + k] + T.gravkicks[a.tb_grav[i]] * a.gacc[3 * i + k] + a.gpm[3 * i + k] * T.FgravkickB;
    if(HYDRO)
        v += T.hydrokicks[a.tb_hydro[i]] * a.hydroacc[3 * i + k];
    return v;
}

// is (pot, idx) lower than the lane's best?  idx < 0: no candidate yet
__device__ __forceinline__ bool df_lower(const double pot, const int idx, const double bpot, const int bidx)
{
    return idx >= 0 && (bidx < 0 || pot < bpot || (pot == bpot && idx < bidx));
}

// the two queues: the listed black holes, and the targets of the walk among them; garbage and swallowed rows carry type 7
__global__ void __launch_bounds__(256) k_df_queues(int64_t n, const uint8_t *__restrict__ flags, const uint8_t *__restrict__ type,
                                                   const uint8_t *__restrict__ active_dynfric, int method, int *__restrict__ queue_bh,
                                                   int *__restrict__ queue_t, unsigned *__restrict__ ctr)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const bool bh = i < n && type && (!flags || flags[i]) && (type[i] & 7) == 5;
    const bool target = bh && (method == 0 || !active_dynfric || active_dynfric[i]);
    wave_append(bh, (int)i, queue_bh, ctr + CTR_BH);
    wave_append(target, (int)i, queue_t, ctr + CTR_T);
}

// blackhole_minpot_preprocess + blackhole_dynfric_ngbiter (method 0: blackhole_minpot_ngbiter) + the reduce + blackhole_dynfric_postprocess
__global__ void __launch_bounds__(256, 2) k_dynfric(const TreeView tv, const DfView A, const mpg_sph_times T, const DfScalars S, const DfState W,
                                                   const int *__restrict__ queue, int64_t nqueue, unsigned *__restrict__ ctr,
                                                   unsigned long long *__restrict__ stats, double *__restrict__ zeromass)
{
    __shared__ unsigned s_stack[4 * 8 * SPH_STK];
    __shared__ unsigned s_llist[4 * 8 * SPH_LCAP];
    NgbGroup g = ngb_group(s_stack, s_llist, nqueue);
    const bool valid = g.valid;
    const mpg_bh_dynfric_arrays &a = A.a;
    const int method = S.p.BH_DynFrictionMethod;
    unsigned n_int = 0, n_cand = 0;
    int64_t i = 0;
    double px = 0, py = 0, pz = 0, hsml = 0, ipot = 0;
    if(valid) {
        i = queue[g.q];
        px = A.pos[3 * i];
        py = A.pos[3 * i + 1];
        pz = A.pos[3 * i + 2];
        hsml = a.hsml[i];
        ipot = a.potential[i];
    }
    const DKernel kern = kernel_init(valid ? hsml : 1.0, S.ktype);
    double bpot = 0;
    int bidx = -1;
    double dens = 0, sv0 = 0, sv1 = 0, sv2 = 0, rms = 0;
    auto loops = [&](auto wrap_tag) {
        constexpr bool WRAP = decltype(wrap_tag)::value;
        ngb_search<false, DF_WALK_K, DF_MERGE, WRAP>(
            tv, tv.geoB, nullptr, g, hsml, px, py, pz, [&](const int slot) { return tv.src[slot]; },
            [&](const Src4 &cand, const int slot, const bool live) {
                if(!live)
                    return;
                n_cand++;
                const double d0 = near_img<WRAP>(px - cand.x, tv.box, 1.0 / tv.box);
                const double d1 = near_img<WRAP>(py - cand.y, tv.box, 1.0 / tv.box);
                const double d2 = near_img<WRAP>(pz - cand.z, tv.box, 1.0 / tv.box);
                const double r2 = d0 * d0 + d1 * d1 + d2 * d2;
                if(!(r2 < kern.HH))
                    return;
                n_int++;
                const int ci = tv.order[slot];
                const double pot = a.potential[ci];
                if(pot < ipot && df_lower(pot, ci, bpot, bidx)) {
                    bpot = pot;
                    bidx = ci;
                }
                if(method > 0) {
                    const int ty = A.type[ci] & 7;
                    if(ty == 4 || (ty == 1 && method > 1) || (ty == 0 && method == 3)) {
                        const double wk = kernel_wk(kern, S.ktype, sqrt(r2) * kern.Hinv);
                        const double mw = cand.m * wk; // (P.Mass is a float; the tree keeps it widened)
                        double v[3];
                        for(int k = 0; k < 3; k++)
                            v[k] = ty == 0 ? df_velpred<true>(a, T, ci, k) : df_velpred<false>(a, T, ci, k);
                        dens += mw;
                        sv0 += mw * v[0];
                        sv1 += mw * v[1];
                        sv2 += mw * v[2];
                        rms += mw * (v[0] * v[0]);
                        rms += mw * (v[1] * v[1]);
                        rms += mw * (v[2] * v[2]);
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
    dens = group_sum(dens);
    sv0 = group_sum(sv0);
    sv1 = group_sum(sv1);
    sv2 = group_sum(sv2);
    rms = group_sum(rms);
    const int numngb = group_sum_int((int)n_int);
    for(int off = 1; off < 8; off <<= 1) {
        const double op = __shfl_xor(bpot, off);
        const int oi = __shfl_xor(bidx, off);
        if(df_lower(op, oi, bpot, bidx)) {
            bpot = op;
            bidx = oi;
        }
    }
    bool zero = false;
    if(valid && g.s == 0) {
        W.minidx[i] = bidx;
        W.numngb[i] = numngb;
        if(bidx >= 0) { // blackhole_repos_reduce
            a.minpot[i] = bpot;
            a.jumptominpot[i] = S.p.BlackHoleRepositionEnabled;
            for(int k = 0; k < 3; k++) {
                a.minpotpos[3 * i + k] = A.pos[3 * (int64_t)bidx + k];
                a.minpotvel[3 * i + k] = a.vel[3 * (int64_t)bidx + k];
            }
        }
        else { // blackhole_minpot_preprocess
            a.minpot[i] = ipot;
            a.minpotpos[3 * i] = px;
            a.minpotpos[3 * i + 1] = py;
            a.minpotpos[3 * i + 2] = pz;
        }
        if(method > 0) { // blackhole_dynfric_reduce + blackhole_dynfric_postprocess
            double *raw = W.raw + DF_NRAW * i;
            raw[0] = dens;
            raw[1] = sv0;
            raw[2] = sv1;
            raw[3] = sv2;
            raw[4] = rms;
            if(dens > 0) {
                rms = sqrt(rms / dens);
                sv0 /= dens;
                sv1 /= dens;
                sv2 /= dens;
            }
            else {
                zero = true;
                unsafeAtomicAdd(zeromass, a.bh_mass[i]);
            }
            a.df_density[i] = dens;
            a.df_vel[3 * i] = sv0;
            a.df_vel[3 * i + 1] = sv1;
            a.df_vel[3 * i + 2] = sv2;
            a.df_rmsvel[i] = rms;
        }
    }
    const unsigned long long mz = ballot64(zero);
    if(mz != 0 && g.lane == 0)
        atomicAdd(ctr + CTR_ZERO, (unsigned)__popcll(mz));
    wave_stats(stats, n_cand, n_int);
}

// blackhole_compute_dfaccel, bhdynfric.c:86-145, one thread per listed black hole, in the reference's expression order (no contraction)
__global__ void __launch_bounds__(256) k_dfaccel(int64_t nq, const int *__restrict__ queue, const DfView A, const DfScalars S, double atime,
                                                 unsigned *__restrict__ ctr)
{
#pragma clang fp contract(off)
    const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if(q >= nq)
        return;
    const mpg_bh_dynfric_arrays &a = A.a;
    const int64_t n = queue[q];
    double acc[3] = {0, 0, 0};
    const double density = a.df_density[n];
    if(density > 0) {
        const double Grav = S.p.GravInternal, mass = (double)A.mass[n];
        double dv[3], bhvel = 0;
        for(int j = 0; j < 3; j++) {
            dv[j] = a.vel[3 * n + j] - a.df_vel[3 * n + j];
            bhvel += dv[j] * dv[j];
        }
        bhvel = sqrt(bhvel);
        if(!isfinite(bhvel)) {
            atomicExch(ctr + CTR_BAD, 1u);
            return;
        }
        const double x = bhvel / sqrt(2.0) / (a.df_rmsvel[n] / 3);
        // first term: the approximation of the error function
        const double a_erf = 8 * (M_PI - 3) / (3 * M_PI * (4. - M_PI));
        double f_of_x = x / fabs(x) * sqrt(1 - exp(-x * x * (4 / M_PI + a_erf * x * x) / (1 + a_erf * x * x))) - 2 * x / sqrt(M_PI) * exp(-x * x);
        if(f_of_x < 0)
            f_of_x = 0;
        const double va = bhvel / atime;
        const double lambda = 1. + S.p.BH_DFbmax * (va * va) / Grav / mass;
        if(bhvel > 0) // "prevent DFAccel from exploding": bhvel == 0 leaves exactly 0
            for(int j = 0; j < 3; j++) {
                double d = -4. * M_PI * Grav * Grav * mass * density * log(lambda) * f_of_x * dv[j] / (bhvel * bhvel * bhvel);
                d *= atime;
                d *= S.p.BH_DFBoostFactor;
                acc[j] = d;
            }
    }
    for(int j = 0; j < 3; j++)
        a.dfaccel[3 * n + j] = acc[j];
}

int64_t DynfricEngine::make_queues(const uint8_t *type, const uint8_t *active_flags, const uint8_t *active_dynfric, int method, int64_t n, hipStream_t st)
{
    queue_t.reserve(n + 1);
    queue_bh.reserve(n + 1);
    ctr.reserve(8);
    stats.reserve(8);
    zeromass.reserve(2);
    MPG_HIP(hipMemsetAsync(ctr.p, 0, 8 * sizeof(unsigned), st));
    MPG_HIP(hipMemsetAsync(stats.p, 0, 8 * sizeof(unsigned long long), st));
    MPG_HIP(hipMemsetAsync(zeromass.p, 0, sizeof(double), st));
    if(n > 0)
        hipLaunchKernelGGL(k_df_queues, dim3(nblk(n)), dim3(256), 0, st, n, active_flags, type, active_dynfric, method, queue_bh.p, queue_t.p, ctr.p);
    MPG_HIP(hipGetLastError());
    unsigned c[2] = {0, 0};
    MPG_HIP(hipMemcpyAsync(c, ctr.p, sizeof(c), hipMemcpyDeviceToHost, st));
    MPG_HIP(hipStreamSynchronize(st));
    reset();
    ntargets = c[CTR_T];
    nlisted = c[CTR_BH];
    last_stats[4] = nlisted;
    return ntargets;
}

void DynfricEngine::walk(TreeBuilder &tree, const DfView &A, const mpg_sph_times &T, const DfScalars &S, int64_t n, hipStream_t st)
{
    tree.ensure_level_order(st); // the cooperative walk uses the level-ordered copy of the tree
    TreeView tv = tree.view();
    tv.geoS = nullptr; // the asymmetric search keeps the reference's cell test (cull_node), as the density loop does
    MPG_CHECK(tv.npart > 0, "blackhole_dynfric: the tree holds no particles");
    raw.reserve((size_t)DF_NRAW * n + 1);
    minidx.reserve(n + 1);
    numngb.reserve(n + 1);
    for(hipEvent_t &e : ev)
        if(!e)
            MPG_HIP(hipEventCreate(&e));
    MPG_HIP(hipMemsetAsync(raw.p, 0, (size_t)DF_NRAW * n * sizeof(double), st));
    MPG_HIP(hipMemsetAsync(minidx.p, 0xff, (size_t)n * sizeof(int), st)); // -1: not a target of this call
    MPG_HIP(hipMemsetAsync(numngb.p, 0xff, (size_t)n * sizeof(int), st));
    n_state = n;
    MPG_HIP(hipEventRecord(ev[0], st));
    hipLaunchKernelGGL(k_dynfric, dim3(nblk(ntargets, 32)), dim3(256), 0, st, tv, A, T, S, state(), queue_t.p, ntargets, ctr.p, stats.p, zeromass.p);
    MPG_HIP(hipEventRecord(ev[1], st));
    MPG_HIP(hipGetLastError());
    unsigned long long hs[2] = {0, 0};
    ngb_read_stats(stats.p, 2, hs, ctr.p + CTR_ERR, "blackhole_dynfric", st);
    unsigned c[4] = {0, 0, 0, 0};
    MPG_HIP(hipMemcpyAsync(c, ctr.p, sizeof(c), hipMemcpyDeviceToHost, st));
    MPG_HIP(hipMemcpyAsync(&last_zeromass, zeromass.p, sizeof(double), hipMemcpyDeviceToHost, st));
    MPG_HIP(hipStreamSynchronize(st));
    last_stats[0] = ntargets;
    last_stats[1] = (int64_t)hs[0];
    last_stats[2] = (int64_t)hs[1];
    last_stats[3] = c[CTR_ZERO];
    MPG_HIP(hipEventElapsedTime(&last_ms[0], ev[0], ev[1]));
}

void DynfricEngine::dfaccel(const DfView &A, const mpg_sph_times &T, const DfScalars &S, hipStream_t st)
{
    if(nlisted == 0)
        return;
    for(hipEvent_t &e : ev)
        if(!e)
            MPG_HIP(hipEventCreate(&e));
    MPG_HIP(hipEventRecord(ev[1], st));
    hipLaunchKernelGGL(k_dfaccel, dim3(nblk(nlisted)), dim3(256), 0, st, nlisted, queue_bh.p, A, S, T.atime, ctr.p);
    MPG_HIP(hipEventRecord(ev[2], st));
    MPG_HIP(hipGetLastError());
    unsigned bad = 0;
    MPG_HIP(hipMemcpyAsync(&bad, ctr.p + CTR_BAD, sizeof(bad), hipMemcpyDeviceToHost, st));
    MPG_HIP(hipStreamSynchronize(st));
    MPG_HIP(hipEventElapsedTime(&last_ms[1], ev[1], ev[2]));
    MPG_CHECK(bad == 0, "blackhole_dfaccel: a black hole's velocity relative to its surroundings is not finite");
}

} // namespace mpg
