// blackhole.hip -- black-hole accretion, mergers and feedback (blackhole(), run.c:660) for gfx950, fp64.
//
// Reference: libgadget/blackhole.c (blackhole_haswork :185-188, blackhole_accretion_ngbiter :471-649, blackhole_accretion_postprocess
// :373-468, blackhole_feedback_ngbiter :746-902, blackhole_feedback_haswork :904-909, blackhole_feedback_copy :912-935,
// blackhole_feedback_postprocess :955-990, check_grav_bound :163-181, get_random_dir :731-740), SPH_VelPred / DM_VelPred (density.c:89-112),
// sfreff_on_eeqos (sfr_eff.c:535-551).  Dynamical friction and repositioning (bhdynfric.c) are the caller's: DFAccel arrives as data.
//
// Mapping: the group-cooperative search of ngb_walk.h with the SYMMETRIC radius (as k_hydro), 8 lanes per target, on the tree of gas and
// black holes with the reference's cells and hmax (tv.geoB / tv.hmaxB).  The targets are few - the active black holes - and each has
// BlackHoleNgbFactor times the neighbours of a gas particle, so a target is mostly phase B of the search (lane s <-> particle s of an
// opened leaf); what a candidate needs beyond its position and Hsml (kept in tree order) is gathered from the caller's arrays only for
// the candidates that pass the distance test.
//
// Marks.  A swallow mark is one 64-bit word per particle holding ID + 1 of the swallower, written with atomicMax.  For gas that is the
// reference's compare-and-swap loop (:604-613: it keeps the largest ID + 1) in every order of arrival.  For black holes the reference
// keeps the largest eligible swallower as well, except that it compares the STORED ID + 1 with the newcomer's ID (:548): of two
// candidates with consecutive IDs K and K + 1 it keeps whichever arrives first when K comes first.  Here: the largest.
//
// Feedback.  The reference adds every black hole's energy to a gas particle's entropy in a compare-and-swap loop, capping the internal
// energy at 5e8 K after every addition; the additions are positive, so with u_k = min(u_(k-1) + e_k, cap): u_n = min(u_0 + sum e_k, cap)
// in exact arithmetic for every order (induction: if no intermediate cap binds, both are u_0 + sum; once u_(k-1) + e_k >= cap, every later
// value is cap and u_0 + sum >= cap).  k_bh_feedback adds e_k with fp64 atomics to one accumulator per gas particle of the tree and
// k_bh_apply takes the minimum once; the kinetic kicks dvel * dir are three more accumulators, added to Vel by the same pass.  The
// swallower's own sums (mass, momentum, BHP.Mass, CountProgs, minTimeBin) are reduced inside its lane group.
//
// Races.  k_bh_accrete writes rows of its targets only, and marks.  k_bh_feedback's targets are unmarked; it reads and writes marked
// black holes (never targets) from the one group whose ID the mark names, marks gas garbage from that one group, and writes its own
// target's rows in the post-process - rows no other group reads (they read marked black holes and gas).
#include "blackhole.h"
#include "ngb_walk.h"
#include "density_kernel.h"
#include <cmath>
#include <type_traits>

namespace mpg {

constexpr int BH_WALK_K = 2;     // child ranges per search step (walk_stepk, ngb_walk.h), as the SPH loops
constexpr bool BH_MERGE = true;  // sibling leaves joined into one list entry
constexpr double BH_GAMMA = 5.0 / 3.0, BH_GAMMA_MINUS1 = BH_GAMMA - 1; // physconst.h:35-36
constexpr int FB_SPLINE = 0x4, FB_MASS = 0x8; // enum BlackHoleFeedbackMethod, blackhole.h:47-53

// words of BlackholeEngine::ctr: targets of the accretion walk, of the feedback walk, the search's overflow flag
constexpr int CTR_Q = 0, CTR_Q1 = 1, CTR_ERR = 7;
// words of stats: mpg_blackhole_get_stats [0] - [5]
constexpr int STAT_SWALLOWED = 0, STAT_ACCRETE = 2, STAT_FEEDBACK = 4;

struct BhCand { // what the distance test reads of a candidate
    Src4 p;
    double hsml; // negative: neither gas nor black hole
};

__device__ __forceinline__ double bh_random(const BhScalars &S, const unsigned long long id) { return S.rnd[id % S.rndsize]; }

// SPH_VelPred (density.c:89-99; HYDRO) / DM_VelPred (:106-112), component k
template <bool HYDRO> __device__ __forceinline__ double bh_velpred(const mpg_blackhole_arrays &a, const mpg_sph_times &T, const int64_t i, const int k)
{
    double v = a.vel[3 * i + k] + T.gravkicks[a.tb_grav[i]] * a.gacc[3 * i + k] + a.gpm[3 * i + k] * T.FgravkickB;
    if(HYDRO)
        v += T.hydrokicks[a.tb_hydro[i]] * a.hydroacc[3 * i + k];
    return v;
}

// the feedback weight of a gas particle: mass or Hsml^3 (blackhole.c:626-630, 834-838)
__device__ __forceinline__ double bh_weight(const BhScalars &S, const mpg_blackhole_arrays &a, const int64_t ci, const double mass)
{
    return (S.p.BlackHoleFeedbackMethod & FB_MASS) ? mass : p3(a.hsml[ci]);
}

// tree-ordered Hsml of the candidates, once per call beside the positions
__global__ void __launch_bounds__(256) k_bh_sources(int64_t npart, const int *__restrict__ order, const BhView A, double *__restrict__ hsml_t)
{
    const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if(k >= npart)
        return;
    const int64_t ci = order[k];
    const int ty = A.type[ci] & 7;
    hsml_t[k] = (ty == 0 || ty == 5) ? A.a.hsml[ci] : -1.0;
}

// the queue of the accretion walk: blackhole_haswork on the active particles; garbage and swallowed rows carry type 7
__global__ void __launch_bounds__(256) k_bh_queue(int64_t n, const uint8_t *__restrict__ flags, const uint8_t *__restrict__ type, int *__restrict__ queue,
                                                  unsigned *__restrict__ ctr)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const bool bh = i < n && type && (!flags || flags[i]) && (type[i] & 7) == 5;
    wave_append(bh, (int)i, queue, ctr + CTR_Q);
}

// ... and of the feedback walk: the targets that are not themselves marked (blackhole_feedback_haswork)
__global__ void __launch_bounds__(256) k_bh_queue_feedback(int64_t nq, const int *__restrict__ queue, const unsigned long long *__restrict__ swal,
                                                           int *__restrict__ queue1, unsigned *__restrict__ ctr)
{
    const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int i = q < nq ? queue[q] : 0;
    wave_append(q < nq && swal[i] == 0ull, i, queue1, ctr + CTR_Q1);
}

// blackhole_accretion_ngbiter + blackhole_accretion_postprocess
__global__ void __launch_bounds__(256, 2) k_bh_accrete(const TreeView tv, const BhView A, const mpg_sph_times T, const BhScalars S, const BhState W,
                                                      const double *__restrict__ hsml_t, const int *__restrict__ queue, int64_t nqueue,
                                                      unsigned *__restrict__ ctr, unsigned long long *__restrict__ stats)
{
    __shared__ unsigned s_stack[4 * 8 * SPH_STK];
    __shared__ unsigned s_llist[4 * 8 * SPH_LCAP];
    NgbGroup g = ngb_group(s_stack, s_llist, nqueue);
    const bool valid = g.valid;
    const mpg_blackhole_arrays &a = A.a;
    unsigned n_int = 0, n_cand = 0;
    int64_t i = 0;
    double px = 0, py = 0, pz = 0, hsml = 0, density = 0, bhmass = 0, partmass = 0;
    double ivel[3] = {0, 0, 0}, iacc[3] = {0, 0, 0};
    unsigned long long id = 0;
    if(valid) {
        i = queue[g.q];
        px = A.pos[3 * i];
        py = A.pos[3 * i + 1];
        pz = A.pos[3 * i + 2];
        hsml = a.hsml[i];
        density = a.density[i];
        bhmass = a.bh_mass[i];
        id = a.id[i];
        // BHPartMass: the dynamic mass, or Mtrack below the seed's dynamic mass (:582-588)
        partmass = (double)a.mass[i];
        if(S.p.SeedBHDynMass > 0 && a.mtrack[i] < S.p.SeedBHDynMass)
            partmass = a.mtrack[i];
        for(int k = 0; k < 3; k++) { // blackhole_accretion_copy, :673-687
            ivel[k] = a.vel[3 * i + k];
            iacc[k] = a.gacc[3 * i + k] + a.gpm[3 * i + k] + a.dfaccel[3 * i + k];
        }
    }
    const DKernel kern = kernel_init(valid ? hsml : 1.0, S.ktype);
    const bool spline = (S.p.BlackHoleFeedbackMethod & FB_SPLINE) != 0;
    double ent = 0, gv0 = 0, gv1 = 0, gv2 = 0, fws = 0, mgas = 0;
    int encounter = 0;
    auto loops = [&](auto wrap_tag) {
        constexpr bool WRAP = decltype(wrap_tag)::value;
        ngb_search<true, BH_WALK_K, BH_MERGE, WRAP>(
            tv, tv.geoB, tv.hmaxB, g, hsml, px, py, pz, [&](const int slot) { return BhCand{tv.src[slot], hsml_t[slot]}; },
            [&](const BhCand &cand, const int slot, const bool live) {
                if(!live || cand.hsml < 0)
                    return;
                n_cand++;
                const double d0 = near_img<WRAP>(px - cand.p.x, tv.box, 1.0 / tv.box);
                const double d1 = near_img<WRAP>(py - cand.p.y, tv.box, 1.0 / tv.box);
                const double d2 = near_img<WRAP>(pz - cand.p.z, tv.box, 1.0 / tv.box);
                const double r2 = d0 * d0 + d1 * d1 + d2 * d2;
                const double dist = fmax(cand.hsml, hsml); // treewalk.c:976-991
                if(r2 > dist * dist)
                    return;
                const int64_t ci = tv.order[slot];
                const int ty = A.type[ci] & 7;
                const double mass_j = (double)a.mass[ci];
                if(mass_j < 0)
                    return;
                if(S.p.WindDecouple && ty == 0 && a.delaytime[ci] > 0) // winds_is_particle_decoupled
                    return;
                const unsigned long long id_j = a.id[ci];
                if(id_j == id)
                    return;
                n_int++;
                const double r = sqrt(r2);
                if(ty == 5 && r < S.merge_dist) {
                    encounter = 1;
                    bool flag = S.p.BlackHoleRepositionEnabled == 1 || S.p.MergeGravBound == 0;
                    if(S.p.MergeGravBound == 1 && S.p.BlackHoleRepositionEnabled == 0) { // check_grav_bound, :163-181
                        const double dx[3] = {d0, d1, d2};
                        double KE = 0, PE = 0;
                        for(int k = 0; k < 3; k++) {
                            const double dv = ivel[k] - bh_velpred<false>(a, T, ci, k);
                            const double da = iacc[k] - a.gacc[3 * ci + k] - a.gpm[3 * ci + k] - a.dfaccel[3 * ci + k];
                            KE += 0.5 * dv * dv;
                            PE += da * dx[k];
                        }
                        KE /= T.atime * T.atime;
                        PE /= T.atime;
                        flag = PE + KE <= 0;
                    }
                    // eligible: the larger ID swallows; an inactive black hole is swallowed by any active one (:548-557)
                    const bool other_active = !a.active_hydro || a.active_hydro[ci];
                    if(flag && (id_j < id || !other_active))
                        atomicMax(W.swal + ci, id + 1ull);
                }
                if(ty == 0 && r2 < kern.HH) {
                    const double wk = kernel_wk(kern, S.ktype, r * kern.Hinv);
                    const double mw = mass_j * wk;
                    ent += mw * a.entropy[ci];
                    gv0 += mw * bh_velpred<true>(a, T, ci, 0);
                    gv1 += mw * bh_velpred<true>(a, T, ci, 1);
                    gv2 += mw * bh_velpred<true>(a, T, ci, 2);
                    double p = 0;
                    if((bhmass - partmass) > 0 && density > 0)
                        p = (bhmass - partmass) * wk / density;
                    if(bh_random(S, id_j) < p)
                        atomicMax(W.swal + ci, id + 1ull);
                    const double wj = bh_weight(S, a, ci, mass_j);
                    fws += spline ? wj * wk : wj;
                    if(S.p.BlackHoleKineticOn == 1)
                        mgas += mass_j;
                }
            },
            [] {});
    };
    // symmetric search: the radius of a cull is max(node hmax, Hsml) <= max(root hmax, Hsml)
    if(interior_wave(valid, px, py, pz, fmax(hsml, tv.hmaxB[0]), tv.box))
        loops(std::false_type{});
    else
        loops(std::true_type{});
    if(ngb_overflowed(g, ctr + CTR_ERR))
        return;
    ent = group_sum(ent);
    gv0 = group_sum(gv0);
    gv1 = group_sum(gv1);
    gv2 = group_sum(gv2);
    fws = group_sum(fws);
    mgas = group_sum(mgas);
    encounter = group_sum_int(encounter) > 0;
    if(valid && g.s == 0) { // blackhole_accretion_reduce + blackhole_accretion_postprocess
        double gv[3] = {gv0, gv1, gv2};
        double mdot = 0;
        const double meddington = S.meddington_fac * bhmass;
        if(density > 0) {
            ent /= density;
            double bhvel = 0;
            for(int k = 0; k < 3; k++) {
                gv[k] /= density;
                bhvel += (ivel[k] - gv[k]) * (ivel[k] - gv[k]);
            }
            bhvel = sqrt(bhvel) / T.atime;
            const double rho_proper = density * S.a3inv;
            // blackhole_soundspeed, :149-158
            const double soundspeed = sqrt(BH_GAMMA * ent * pow(density, BH_GAMMA_MINUS1)) * pow(T.atime, -1.5 * BH_GAMMA_MINUS1);
            const double norm = pow(soundspeed * soundspeed + bhvel * bhvel, 1.5);
            if(norm > 0)
                mdot = 4. * M_PI * S.p.BlackHoleAccretionFactor * S.p.GravInternal * S.p.GravInternal * bhmass * bhmass * rho_proper / norm;
        }
        if(S.p.BlackHoleEddingtonFactor > 0.0 && mdot > S.p.BlackHoleEddingtonFactor * meddington)
            mdot = S.p.BlackHoleEddingtonFactor * meddington;
        const double dtime = T.dloga_bin[a.tb_hydro[i]] / T.hubble;
        const double newmass = bhmass + mdot * dtime;
        a.mdot[i] = mdot;
        a.bh_mass[i] = newmass;
        double fac = 0;
        if(S.p.BH_DRAG == 1)
            fac = mdot / (double)a.mass[i];
        if(S.p.BH_DRAG == 2)
            fac = S.p.BlackHoleEddingtonFactor * meddington / newmass;
        fac *= T.atime;
        for(int k = 0; k < 3; k++)
            a.dragaccel[3 * i + k] = S.p.BH_DRAG > 0 ? -(ivel[k] - gv[k]) * fac : 0.0;
        int keflag = 0;
        if(S.p.BlackHoleKineticOn == 1) {
            const double edd_ratio = mdot / meddington;
            double lam_thresh = S.p.BHKE_EddingtonThrFactor;
            const double x = S.p.BHKE_EddingtonMFactor * pow(newmass / S.p.BHKE_EddingtonMPivot, S.p.BHKE_EddingtonMIndex);
            if(lam_thresh > x)
                lam_thresh = x;
            double ke = a.kineticfdbkenergy[i];
            if(edd_ratio < lam_thresh) {
                keflag = 1;
                double epsilon = (density / S.rho_sfr) / S.p.BHKE_EffRhoFactor;
                if(epsilon > S.p.BHKE_EffCap)
                    epsilon = S.p.BHKE_EffCap;
                ke += epsilon * (mdot * dtime * S.c2);
                a.kineticfdbkenergy[i] = ke;
            }
            const double vd = a.vdisp[i];
            const double ke_thresh = 0.5 * vd * vd * mgas * S.p.BHKE_InjEnergyThr;
            if(vd > 0 && ke > ke_thresh)
                keflag = 2;
        }
        a.encounter[i] = encounter;
        W.fws[i] = fws;
        W.keflag[i] = keflag;
        if(a.feedbackweightsum)
            a.feedbackweightsum[i] = fws;
        if(a.bh_entropy)
            a.bh_entropy[i] = ent;
        if(a.mgasenc)
            a.mgasenc[i] = mgas;
        if(a.keflag)
            a.keflag[i] = keflag;
        if(a.gasvel)
            for(int k = 0; k < 3; k++)
                a.gasvel[3 * i + k] = gv[k];
    }
    wave_stats(stats + STAT_ACCRETE, n_cand, n_int);
}

// blackhole_feedback_ngbiter + blackhole_feedback_postprocess for the unmarked targets
__global__ void __launch_bounds__(256, 2) k_bh_feedback(const TreeView tv, const BhView A, const mpg_sph_times T, const BhScalars S, const BhState W,
                                                       const double *__restrict__ hsml_t, const int *__restrict__ queue, int64_t nqueue,
                                                       double *__restrict__ acc, unsigned *__restrict__ ctr, unsigned long long *__restrict__ stats)
{
    __shared__ unsigned s_stack[4 * 8 * SPH_STK];
    __shared__ unsigned s_llist[4 * 8 * SPH_LCAP];
    NgbGroup g = ngb_group(s_stack, s_llist, nqueue);
    const bool valid = g.valid;
    const mpg_blackhole_arrays &a = A.a;
    unsigned n_int = 0, n_cand = 0, n_gas = 0, n_bh = 0;
    int64_t i = 0;
    double px = 0, py = 0, pz = 0, hsml = 0, density = 0, mtrack = 0, fws = 0, fenergy = 0, kenergy = 0;
    unsigned long long id = 0;
    int channel = 0, keflag = 0;
    if(valid) { // blackhole_feedback_copy, :912-935
        i = queue[g.q];
        px = A.pos[3 * i];
        py = A.pos[3 * i + 1];
        pz = A.pos[3 * i + 2];
        hsml = a.hsml[i];
        density = a.density[i];
        mtrack = a.mtrack[i];
        id = a.id[i];
        fws = W.fws[i];
        keflag = W.keflag[i];
        const double dtime = T.dloga_bin[a.tb_hydro[i]] / T.hubble;
        fenergy = S.p.BlackHoleFeedbackFactor * 0.1 * a.mdot[i] * dtime * S.c2;
        if(S.p.BlackHoleKineticOn == 1 && keflag > 0) {
            channel = 1;
            if(keflag == 2)
                kenergy = a.kineticfdbkenergy[i];
        }
    }
    const DKernel kern = kernel_init(valid ? hsml : 1.0, S.ktype);
    const bool spline = (S.p.BlackHoleFeedbackMethod & FB_SPLINE) != 0;
    double accmass = 0, accbh = 0, mom0 = 0, mom1 = 0, mom2 = 0;
    int progs = 0, mintb = BH_TIMEBINS;
    auto loops = [&](auto wrap_tag) {
        constexpr bool WRAP = decltype(wrap_tag)::value;
        ngb_search<true, BH_WALK_K, BH_MERGE, WRAP>(
            tv, tv.geoB, tv.hmaxB, g, hsml, px, py, pz, [&](const int slot) { return BhCand{tv.src[slot], hsml_t[slot]}; },
            [&](const BhCand &cand, const int slot, const bool live) {
                if(!live || cand.hsml < 0)
                    return;
                n_cand++;
                const double d0 = near_img<WRAP>(px - cand.p.x, tv.box, 1.0 / tv.box);
                const double d1 = near_img<WRAP>(py - cand.p.y, tv.box, 1.0 / tv.box);
                const double d2 = near_img<WRAP>(pz - cand.p.z, tv.box, 1.0 / tv.box);
                const double r2 = d0 * d0 + d1 * d1 + d2 * d2;
                const double dist = fmax(cand.hsml, hsml);
                if(r2 > dist * dist)
                    return;
                const int64_t ci = tv.order[slot];
                const int ty = A.type[ci] & 7;
                if(a.id[ci] == id)
                    return;
                if(S.p.WindDecouple && ty == 0 && a.delaytime[ci] > 0)
                    return;
                n_int++;
                const unsigned long long mark = W.swal[ci];
                if(ty == 5 && mark != 0ull) {
                    if(mark != id + 1ull)
                        return;
                    // swallow the black hole, :780-816
                    a.swallowid[ci] = id;
                    a.swallowtime[ci] = T.atime;
                    a.flags[ci] = a.flags[ci] | 2;
                    a.encounter[ci] = 0;
                    progs += a.countprogs[ci];
                    accbh += a.bh_mass[ci];
                    double othermass = (double)a.mass[ci];
                    if(S.p.SeedBHDynMass > 0 && mtrack > 0 && a.mtrack[ci] < S.p.SeedBHDynMass)
                        othermass = a.mtrack[ci];
                    accmass += othermass;
                    mom0 += othermass * bh_velpred<false>(a, T, ci, 0);
                    mom1 += othermass * bh_velpred<false>(a, T, ci, 1);
                    mom2 += othermass * bh_velpred<false>(a, T, ci, 2);
                    n_bh++;
                    return;
                }
                if(ty != 0)
                    return;
                const double mass_j = (double)a.mass[ci];
                if(mark == 0ull && r2 < kern.HH) { // thermal or kinetic feedback into gas that is not swallowed, :822-881
                    mintb = min(mintb, (int)a.tb_hydro[ci]);
                    const double wk = spline ? kernel_wk(kern, S.ktype, sqrt(r2) * kern.Hinv) : 1.0;
                    if(fws > 0 && fenergy > 0 && channel == 0 && mass_j > 0) {
                        unsafeAtomicAdd(acc + (int64_t)BH_NACC * slot, fenergy * bh_weight(S, a, ci, mass_j) * wk / fws);
                        // sfreff_on_eeqos, sfr_eff.c:535-551 (BHFeedbackUseTcool == 2 is not carried)
                        const double rho = a.density[ci];
                        if(S.p.StarformationOn && rho * S.a3inv >= S.p.PhysDensThresh && !(rho < S.p.OverDensThresh) && !(a.delaytime[ci] > 0))
                            a.bhheated[ci] = 1;
                    }
                    if(kenergy > 0 && channel == 1 && density > 0) {
                        const double dvel = sqrt(2 * kenergy * wk / density);
                        const unsigned long long id_j = a.id[ci];
                        const double theta = acos(2 * bh_random(S, id_j + 3ull) - 1); // get_random_dir, :731-740
                        const double phi = 2 * M_PI * bh_random(S, id_j + 4ull);
                        double *__restrict__ v = acc + (int64_t)BH_NACC * slot + 1;
                        unsafeAtomicAdd(v, dvel * (sin(theta) * cos(phi)));
                        unsafeAtomicAdd(v + 1, dvel * (sin(theta) * sin(phi)));
                        unsafeAtomicAdd(v + 2, dvel * cos(theta));
                    }
                }
                if(mark == id + 1ull) { // swallow the gas, :887-901
                    accmass += mass_j;
                    mom0 += mass_j * bh_velpred<true>(a, T, ci, 0);
                    mom1 += mass_j * bh_velpred<true>(a, T, ci, 1);
                    mom2 += mass_j * bh_velpred<true>(a, T, ci, 2);
                    a.flags[ci] = a.flags[ci] | 1; // slots_mark_garbage
                    n_gas++;
                }
            },
            [] {});
    };
    if(interior_wave(valid, px, py, pz, fmax(hsml, tv.hmaxB[0]), tv.box))
        loops(std::false_type{});
    else
        loops(std::true_type{});
    if(ngb_overflowed(g, ctr + CTR_ERR))
        return;
    accmass = group_sum(accmass);
    accbh = group_sum(accbh);
    mom0 = group_sum(mom0);
    mom1 = group_sum(mom1);
    mom2 = group_sum(mom2);
    progs = group_sum_int(progs);
    for(int off = 1; off < 8; off <<= 1)
        mintb = min(mintb, __shfl_xor(mintb, off));
    if(valid && g.s == 0) { // blackhole_feedback_reduce + blackhole_feedback_postprocess
        const double mom[3] = {mom0, mom1, mom2};
        a.mintimebin[i] = mintb;
        a.countprogs[i] += progs;
        if(accbh > 0)
            a.bh_mass[i] += accbh;
        if(accmass > 0) {
            const double M = (double)a.mass[i];
            for(int k = 0; k < 3; k++)
                a.vel[3 * i + k] = (a.vel[3 * i + k] * M + mom[k]) / (M + accmass);
            const double seed = S.p.SeedBHDynMass;
            if(seed > 0 && mtrack + accmass < seed)
                a.mtrack[i] = mtrack + accmass; // still in the seed mass regime
            else if(mtrack < seed) {            // the transition to a regular black hole
                a.mass[i] = (float)(mtrack + accmass);
                a.mtrack[i] = seed;
            }
            else
                a.mass[i] = (float)(M + accmass);
        }
        if(keflag == 2)
            a.kineticfdbkenergy[i] = 0;
        if(a.accreted_mass)
            a.accreted_mass[i] = accmass;
        if(a.accreted_bhmass)
            a.accreted_bhmass[i] = accbh;
        if(a.accreted_momentum)
            for(int k = 0; k < 3; k++)
                a.accreted_momentum[3 * i + k] = mom[k];
    }
    wave_stats(stats + STAT_SWALLOWED, n_gas, n_bh);
    wave_stats(stats + STAT_FEEDBACK, n_cand, n_int);
}

// the accumulated energy and kicks into the gas, one thread per particle of the tree; the optional copies of the marks
__global__ void __launch_bounds__(256) k_bh_apply(int64_t npart, const int *__restrict__ order, const BhView A, const BhScalars S, const BhState W,
                                                  const double *__restrict__ acc)
{
    const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if(k >= npart)
        return;
    const mpg_blackhole_arrays &a = A.a;
    const int64_t ci = order[k];
    const int ty = A.type[ci] & 7;
    if(a.sph_swallowid && ty == 0)
        a.sph_swallowid[ci] = W.swal[ci];
    if(a.bh_swallowid && ty == 5)
        a.bh_swallowid[ci] = W.swal[ci];
    const double e = acc[BH_NACC * k];
    if(e > 0) { // add_injected_BH_energy, :718-728, with the cap taken once
        const double enttou = pow(a.density[ci] * S.a3inv, BH_GAMMA_MINUS1) / BH_GAMMA_MINUS1;
        double unew = a.entropy[ci] * enttou + e / (double)a.mass[ci];
        if(unew > S.ucap)
            unew = S.ucap;
        a.entropy[ci] = unew / enttou;
    }
    for(int j = 0; j < 3; j++) {
        const double dv = acc[BH_NACC * k + 1 + j];
        if(dv != 0)
            a.vel[3 * ci + j] += dv;
    }
}

__global__ void __launch_bounds__(256) k_bh_retype(int64_t n, const uint8_t *__restrict__ flags, uint8_t *__restrict__ type)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if(i < n && (flags[i] & 3) != 0)
        type[i] = 7;
}

void BlackholeEngine::retype(uint8_t *type, const uint8_t *flags, int64_t n, hipStream_t st)
{
    if(n > 0)
        hipLaunchKernelGGL(k_bh_retype, dim3(nblk(n)), dim3(256), 0, st, n, flags, type);
    MPG_HIP(hipGetLastError());
}

void BlackholeEngine::set_random_table(const double *table, int64_t size, hipStream_t st)
{
    MPG_HIP(hipStreamSynchronize(st)); // (a kernel in flight may still read the table this call replaces)
    rnd.reserve((size_t)size + 1);
    MPG_HIP(hipMemcpyAsync(rnd.p, table, (size_t)size * sizeof(double), hipMemcpyHostToDevice, st));
    MPG_HIP(hipStreamSynchronize(st));
    rndsize = size;
}

int64_t BlackholeEngine::make_queue(const uint8_t *type, const uint8_t *active_flags, int64_t n, hipStream_t st)
{
    queue_0.reserve(n + 1);
    ctr.reserve(8);
    stats.reserve(8);
    MPG_HIP(hipMemsetAsync(ctr.p, 0, 8 * sizeof(unsigned), st));
    MPG_HIP(hipMemsetAsync(stats.p, 0, 8 * sizeof(unsigned long long), st));
    if(n > 0)
        hipLaunchKernelGGL(k_bh_queue, dim3(nblk(n)), dim3(256), 0, st, n, active_flags, type, queue_0.p, ctr.p);
    MPG_HIP(hipGetLastError());
    unsigned c = 0;
    MPG_HIP(hipMemcpyAsync(&c, ctr.p + CTR_Q, sizeof(c), hipMemcpyDeviceToHost, st));
    MPG_HIP(hipStreamSynchronize(st));
    ntargets = c;
    nfeedback = 0;
    for(int64_t &s : last_stats)
        s = 0;
    last_ms[0] = last_ms[1] = last_ms[2] = 0;
    return ntargets;
}

void BlackholeEngine::run(TreeBuilder &tree, const BhView &A, const mpg_sph_times &T, const BhScalars &S, int64_t n, hipStream_t st)
{
    tree.ensure_level_order(st); // the cooperative walk uses the level-ordered copy of the tree
    const TreeView tv = tree.view();
    MPG_CHECK(tv.npart > 0 && tv.hmaxB, "blackhole: the tree holds no particles or no hmax");
    swal.reserve(n + 1);
    fws.reserve(n + 1);
    keflag.reserve(n + 1);
    queue_1.reserve(ntargets + 1);
    hsml_t.reserve(tv.npart + 1);
    acc.reserve((size_t)BH_NACC * tv.npart + 1);
    const BhState W{swal.p, fws.p, keflag.p};
    for(hipEvent_t &e : ev)
        if(!e)
            MPG_HIP(hipEventCreate(&e));
    MPG_HIP(hipMemsetAsync(swal.p, 0, (size_t)n * sizeof(unsigned long long), st));
    hipLaunchKernelGGL(k_bh_sources, dim3(nblk(tv.npart)), dim3(256), 0, st, tv.npart, tv.order, A, hsml_t.p);
    MPG_HIP(hipEventRecord(ev[0], st));
    hipLaunchKernelGGL(k_bh_accrete, dim3(nblk(ntargets, 32)), dim3(256), 0, st, tv, A, T, S, W, hsml_t.p, queue_0.p, ntargets, ctr.p, stats.p);
    MPG_HIP(hipEventRecord(ev[1], st));
    // the queue of the feedback walk and its length: a host round trip, outside both timed spans
    hipLaunchKernelGGL(k_bh_queue_feedback, dim3(nblk(ntargets)), dim3(256), 0, st, ntargets, queue_0.p, swal.p, queue_1.p, ctr.p);
    MPG_HIP(hipGetLastError());
    unsigned c[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    MPG_HIP(hipMemcpyAsync(c, ctr.p, sizeof(c), hipMemcpyDeviceToHost, st));
    MPG_HIP(hipStreamSynchronize(st));
    MPG_CHECK(c[CTR_ERR] == 0, "blackhole: neighbour-search stack overflow (tree deeper than the walk supports)");
    nfeedback = c[CTR_Q1];
    MPG_HIP(hipEventRecord(ev[2], st));
    MPG_HIP(hipMemsetAsync(acc.p, 0, (size_t)BH_NACC * tv.npart * sizeof(double), st));
    if(nfeedback > 0)
        hipLaunchKernelGGL(k_bh_feedback, dim3(nblk(nfeedback, 32)), dim3(256), 0, st, tv, A, T, S, W, hsml_t.p, queue_1.p, nfeedback, acc.p, ctr.p,
                           stats.p);
    MPG_HIP(hipEventRecord(ev[3], st));
    hipLaunchKernelGGL(k_bh_apply, dim3(nblk(tv.npart)), dim3(256), 0, st, tv.npart, tv.order, A, S, W, acc.p);
    MPG_HIP(hipEventRecord(ev[4], st));
    MPG_HIP(hipGetLastError());
    unsigned long long hs[6] = {0, 0, 0, 0, 0, 0};
    ngb_read_stats(stats.p, 6, hs, ctr.p + CTR_ERR, "blackhole", st);
    for(int k = 0; k < 6; k++)
        last_stats[k] = (int64_t)hs[k];
    last_stats[6] = ntargets;
    last_stats[7] = nfeedback;
    MPG_HIP(hipEventElapsedTime(&last_ms[0], ev[0], ev[1]));
    MPG_HIP(hipEventElapsedTime(&last_ms[1], ev[2], ev[3]));
    MPG_HIP(hipEventElapsedTime(&last_ms[2], ev[3], ev[4]));
}

} // namespace mpg
