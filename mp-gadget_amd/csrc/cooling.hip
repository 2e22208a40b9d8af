// cooling.hip -- cooling_direct (sfr_eff.c:463-514) for the listed gas particles, one lane per particle, fp64 throughout; the solver is
// cooling.h's, the fits cooling_rates.h's.  DESIGN 3.9.
#include "cooling.h"
#include <cmath>
#include <cstring>

namespace mpg {

using namespace cool;

namespace {

constexpr int COOL_BLOCK = 128;
enum { ST_TREATED = 0, ST_EVALS, ST_BISECT, ST_FLOOR, ST_REION, ST_ERRORS, ST_N };

// the six tables ne_internal reads at one index, copied into LDS (48 000 bytes) when the kernel is launched with them
__device__ const double *stage_net_tables(const double *net, bool use_lds)
{
    extern __shared__ double lds_net[];
    if(!use_lds)
        return net;
    for(int i = threadIdx.x; i < NRECOMBTAB * NNET; i += blockDim.x)
        lds_net[i] = net[i];
    __syncthreads();
    return lds_net;
}

__device__ void add_block_stats(unsigned long long *stats, const unsigned long long *mine)
{
    __shared__ unsigned long long s[ST_N];
    if(threadIdx.x < ST_N)
        s[threadIdx.x] = 0;
    __syncthreads();
    for(int k = 0; k < ST_N; k++)
        if(mine[k])
            atomicAdd(&s[k], mine[k]);
    __syncthreads();
    if(threadIdx.x < ST_N && s[threadIdx.x])
        atomicAdd(&stats[threadIdx.x], s[threadIdx.x]);
}

struct CoolTimes {
    double dtime[47]; // dloga_bin / hubble, sfr_eff.c:467-468
    double lastred[47];
    double a3inv;
};

// where a row's background comes from (get_local_UVBG, cooling_uvfluc.c:236-246).
// BG_UVF: from its own zreion (zr, by particle; get_local_UVBG_from_global).  A row whose zreion is NaN has none: it is an error row.
// BG_J21: from its own J21 and zreion (j21 and zr, by particle; get_local_UVBG_from_J21, X the model).  A row whose J21 is NaN or negative
// or whose zreion is NaN is an error row.  Without either the kernels (k_cooling, k_cooling_queue) are what they were.
enum Background { BG_GLOBAL = 0, BG_UVF = 1, BG_J21 = 2 };
template <int BG>
__device__ __forceinline__ void cooling_rows(Setup S, const CoolTimes &T, const mpg_cooling_arrays &A, const uint8_t *type, const float *mass,
                                             const int *active, int64_t nlist, int64_t n, int *evals, unsigned long long *stats, const double *zr,
                                             int use_lds, const double *j21 = nullptr, const J21View *X = nullptr)
{
    constexpr bool UVF = BG == BG_UVF;
    S.net = stage_net_tables(S.net, use_lds != 0);
    unsigned long long mine[ST_N] = {0, 0, 0, 0, 0, 0};
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    int64_t p = -1;
    if(t < nlist) {
        p = active ? (int64_t)active[t] : t;
        // a list entry outside the table is ignored; non-gas, garbage (type 7) and massless rows are skipped (sfr_eff.c:229)
        if(p < 0 || p >= n || (type ? type[p] : (uint8_t)1) != 0 || !(mass[p] > 0))
            p = -1;
    }
    double zreion = 0, J21 = 0;
    if constexpr(BG != BG_GLOBAL)
        if(p >= 0)
            zreion = zr[p];
    if constexpr(BG == BG_J21)
        if(p >= 0)
            J21 = j21[p];
    if((UVF && p >= 0 && zreion != zreion) || (BG == BG_J21 && p >= 0 && j21_row_bad(J21, zreion))) {
        evals[p] = 0;
        mine[ST_TREATED] = 1;
        mine[ST_ERRORS] = 1;
    }
    else if(p >= 0) {
        const int bin = A.tb_hydro ? (A.tb_hydro[p] < 47 ? A.tb_hydro[p] : 46) : 0;
        double ne = A.ne[p];
        Counters C;
        int reion = 0;
        double ent;
        if constexpr(UVF)
            ent = cooling_direct(local_setup(S, zreion), A.density[p], A.entropy[p], &ne, A.metallicity ? A.metallicity[p] : 0.0,
                                 A.heiii_ionized ? (int)A.heiii_ionized[p] : 0, T.dtime[bin], T.a3inv, T.lastred[bin], C, &reion);
        else if constexpr(BG == BG_J21)
            ent = cooling_direct(j21_setup(S, *X, J21, zreion), A.density[p], A.entropy[p], &ne, A.metallicity ? A.metallicity[p] : 0.0,
                                 A.heiii_ionized ? (int)A.heiii_ionized[p] : 0, T.dtime[bin], T.a3inv, T.lastred[bin], C, &reion);
        else
            ent = cooling_direct(S, A.density[p], A.entropy[p], &ne, A.metallicity ? A.metallicity[p] : 0.0,
                                 A.heiii_ionized ? (int)A.heiii_ionized[p] : 0, T.dtime[bin], T.a3inv, T.lastred[bin], C, &reion);
        if(!C.error) {
            A.ne[p] = ne;
            A.entropy[p] = ent;
            A.sfr[p] = 0;
        }
        evals[p] = C.evals;
        mine[ST_TREATED] = 1;
        mine[ST_EVALS] = C.evals;
        mine[ST_BISECT] = C.bisections;
        mine[ST_FLOOR] = C.error ? 0 : C.floor; // (a particle that hit a limit ended nowhere)
        mine[ST_REION] = reion;
        mine[ST_ERRORS] = C.error;
    }
    add_block_stats(stats, mine);
}

__global__ __launch_bounds__(COOL_BLOCK) void k_cooling(Setup S, CoolTimes T, mpg_cooling_arrays A, const uint8_t *type, const float *mass,
                                                        const int *active, int64_t nlist, int64_t n, int *evals, unsigned long long *stats,
                                                        int use_lds)
{
    cooling_rows<BG_GLOBAL>(S, T, A, type, mass, active, nlist, n, evals, stats, nullptr, use_lds);
}
__global__ __launch_bounds__(COOL_BLOCK) void k_cooling_uvf(Setup S, CoolTimes T, mpg_cooling_arrays A, const uint8_t *type, const float *mass,
                                                            const int *active, int64_t nlist, int64_t n, int *evals, unsigned long long *stats,
                                                            const double *zr, int use_lds)
{
    cooling_rows<BG_UVF>(S, T, A, type, mass, active, nlist, n, evals, stats, zr, use_lds);
}
__global__ __launch_bounds__(COOL_BLOCK) void k_cooling_j21(Setup S, CoolTimes T, mpg_cooling_arrays A, const uint8_t *type, const float *mass,
                                                            const int *active, int64_t nlist, int64_t n, int *evals, unsigned long long *stats,
                                                            const double *j21, const double *zr, J21View X, int use_lds)
{
    cooling_rows<BG_J21>(S, T, A, type, mass, active, nlist, n, evals, stats, zr, use_lds, j21, &X);
}

// ---- the second form: a per-lane state machine whose unit step is ONE evaluation of the network -----------------------------------------
// The evaluations per particle differ by a factor of 17 and more (21 .. several hundred), so in k_cooling a wave runs as long as its
// slowest particle.  Here a lane that has finished its particle takes the next entry of the list from a counter the wave advances once for
// all its idle lanes, and every trip of the loop is the same code for every lane: one ne_internal.  The arithmetic is that of do_cooling /
// get_equilib_ne statement by statement (cooling.h), only the control flow is unrolled into the fields of Lane.
enum Phase { PH_INIT = 0, PH_UP, PH_DOWN, PH_BISECT };
struct Lane {
    int64_t p = -1; // the particle in work, -1: none
    int phase, heiii, fp_i, sub, guard, iter;
    int dark = 0; // with a UV-fluctuation table: the particle is not yet reionised (its zreion < redshift)
    double rho, u_old, MinEgySpec, dt, Z, enttou; // DoCooling's arguments in cgs
    double u_lower, u_upper, u;                   // the bracket, and the energy the network is being solved at
    double ne_guess, ne0, ne1;
    Counters C;
};

__device__ inline void lane_start_lambda(Lane &L, double u)
{
    L.u = u;
    L.ne0 = L.ne_guess <= 0 ? 1.0 : L.ne_guess; // get_equilib_ne, cooling_rates.c:824-825
    L.fp_i = 0;
    L.sub = 0;
}

// the bisection's next trial, or its end on the floor (cooling.c:102-108): returns true when the particle is finished
__device__ inline bool lane_bisect_begin(Lane &L)
{
    L.u = 0.5 * (L.u_lower + L.u_upper);
    if(L.u_upper <= L.MinEgySpec) {
        L.u = L.MinEgySpec;
        L.C.floor = 1;
        return true;
    }
    L.phase = PH_BISECT;
    lane_start_lambda(L, L.u);
    return false;
}

// DoCooling's step after one LambdaNet (cooling.c:77-128): returns true when the particle is finished (L.u is the result, or L.C.error)
__device__ inline bool lane_advance(Lane &L, double LambdaNet)
{
    switch(L.phase) {
    case PH_INIT:
        if(L.u - L.u_old - LambdaNet * L.dt < 0) {
            L.phase = PH_UP;
            L.u_lower = L.u_upper;
            L.u_upper *= 1.1;
            L.guard++;
            lane_start_lambda(L, L.u_upper);
            return false;
        }
        L.phase = PH_DOWN;
        L.u_upper = L.u_lower;
        L.u_lower /= 1.1;
        if(L.u_upper <= L.MinEgySpec)
            return lane_bisect_begin(L);
        L.guard++;
        lane_start_lambda(L, L.u_lower);
        return false;
    case PH_UP:
        if(L.u_upper - L.u_old - LambdaNet * L.dt < 0) {
            L.u_lower = L.u_upper;
            L.u_upper *= 1.1;
            if(++L.guard > BRACKET_MAXITER) {
                L.C.error = 1;
                return true;
            }
            lane_start_lambda(L, L.u_upper);
            return false;
        }
        return lane_bisect_begin(L);
    case PH_DOWN:
        if(L.u_lower - L.u_old - LambdaNet * L.dt > 0) {
            L.u_upper = L.u_lower;
            L.u_lower /= 1.1;
            if(L.u_upper <= L.MinEgySpec)
                return lane_bisect_begin(L);
            if(++L.guard > BRACKET_MAXITER) {
                L.C.error = 1;
                return true;
            }
            lane_start_lambda(L, L.u_lower);
            return false;
        }
        return lane_bisect_begin(L);
    default: {
        if(L.u - L.u_old - LambdaNet * L.dt > 0)
            L.u_upper = L.u;
        else
            L.u_lower = L.u;
        const double du = L.u_upper - L.u_lower;
        L.iter++;
        L.C.bisections++;
        if(fabs(du / L.u) > 1.0e-6 && L.iter < COOL_MAXITER)
            return lane_bisect_begin(L);
        if(L.iter >= COOL_MAXITER)
            L.C.error = 1;
        return true;
    }
    }
}

// one trip of k_cooling_queue's loop for a lane that holds a particle: one evaluation of the network (scipy_optimize_fixed_point,
// cooling_rates.c:784-805) under the background of S, and what follows from it
__device__ __forceinline__ void one_evaluation(const Setup &S, Lane &L, unsigned long long *mine, const mpg_cooling_arrays &A, int *evals)
{
    const double helium = 1 - HYDROGEN_MASSFRAC;
    const double nh = L.rho * (1 - helium);
    double logt1;
    bool converged = false;
    if(L.sub == 0) {
        L.ne1 = ne_internal(S, nh, L.u, L.ne0 * nh, helium, &logt1, L.C) / nh;
        if(fabs(L.ne1 - L.ne0) < 1e-6) {
            L.ne0 = L.ne1;
            converged = true;
        }
        else
            L.sub = 1;
    }
    else {
        const double ne2 = ne_internal(S, nh, L.u, L.ne1 * nh, helium, &logt1, L.C) / nh;
        const double d = L.ne0 + ne2 - 2.0 * L.ne1;
        double pp = ne2;
        if(d > 1e-15 || d < -1e-15)
            pp = L.ne0 - (L.ne1 - L.ne0) * (L.ne1 - L.ne0) / d;
        L.ne0 = pp;
        if(L.ne0 < 0)
            L.ne0 = 0;
        L.sub = 0;
        if(++L.fp_i == S.net_maxiter)
            L.C.error = 1;
    }
    bool done = L.C.error != 0;
    if(converged) {
        double LambdaNet = heatingcooling_at_equilibrium(S, L.rho, L.u, helium, S.redshift, L.Z, L.ne0 * nh, logt1, &L.ne_guess);
        if(!L.heiii)
            LambdaNet += S.lmfp_heating / (S.units_rho_crit_baryon * pow(1 + S.redshift, 3.0));
        done = lane_advance(L, LambdaNet);
    }
    if(done) {
        if(!L.C.error) {
            A.ne[L.p] = L.ne_guess;
            A.entropy[L.p] = (L.u / S.uu_in_cgs) / L.enttou;
            A.sfr[L.p] = 0;
        }
        evals[L.p] = L.C.evals;
        mine[ST_EVALS] += L.C.evals;
        mine[ST_BISECT] += L.C.bisections;
        mine[ST_FLOOR] += L.C.error ? 0 : L.C.floor;
        mine[ST_ERRORS] += L.C.error;
        L.p = -1;
    }
}

template <int BG>
__device__ __forceinline__ void cooling_queue(Setup S, const CoolTimes &T, const mpg_cooling_arrays &A, const uint8_t *type, const float *mass,
                                              const int *active, int64_t nlist, int64_t n, int *evals, unsigned long long *stats,
                                              unsigned long long *queue, const double *zr, int use_lds, const double *j21 = nullptr,
                                              const J21View *X = nullptr)
{
    constexpr bool UVF = BG == BG_UVF;
    // BG_J21: what a lane keeps of its particle's background across the evaluations: J21 and the self-shield density of its gJH0; the four
    // rates are two or three products each and are made again in every evaluation
    [[maybe_unused]] double lane_j21 = 0, lane_ssd = 0;
    S.net = stage_net_tables(S.net, use_lds != 0);
    unsigned long long mine[ST_N] = {0, 0, 0, 0, 0, 0};
    const int lane = __lane_id();
    Lane L;
    bool more = true; // the list may still hold entries
    for(;;) {
        // ---- idle lanes take the next entries of the list: one atomic per wave
        const bool need = L.p < 0 && more;
        const unsigned long long m = __ballot(need);
        if(m) {
            const int leader = __ffsll((long long)m) - 1;
            unsigned long long base = 0;
            if(lane == leader)
                base = atomicAdd(queue, (unsigned long long)__popcll(m));
            const unsigned lo = __shfl((unsigned)(base & 0xffffffffu), leader), hi = __shfl((unsigned)(base >> 32), leader);
            if(need) {
                const int64_t t = (int64_t)(((unsigned long long)hi << 32) | lo) + __popcll(m & ((1ull << lane) - 1));
                if(t >= nlist)
                    more = false;
                else {
                    int64_t p = active ? (int64_t)active[t] : t;
                    if(p < 0 || p >= n || (type ? type[p] : (uint8_t)1) != 0 || !(mass[p] > 0))
                        p = -1;
                    double zreion = S.uvbg.zreion;
                    if constexpr(UVF)
                        if(p >= 0) {
                            zreion = zr[p];
                            if(zreion != zreion) {
                                evals[p] = 0;
                                mine[ST_TREATED]++;
                                mine[ST_ERRORS]++;
                                p = -1;
                            }
                        }
                    if constexpr(BG == BG_J21)
                        if(p >= 0) {
                            zreion = zr[p];
                            lane_j21 = j21[p];
                            if(j21_row_bad(lane_j21, zreion)) {
                                evals[p] = 0;
                                mine[ST_TREATED]++;
                                mine[ST_ERRORS]++;
                                p = -1;
                            }
                        }
                    if(p >= 0) {
                        // cooling_direct up to the call of DoCooling (sfr_eff.c:463-506) and DoCooling's head (cooling.c:59-75)
                        const int bin = A.tb_hydro ? (A.tb_hydro[p] < 47 ? A.tb_hydro[p] : 46) : 0;
                        const double density = A.density[p];
                        L.C = Counters();
                        L.enttou = entropy_to_u(density, T.a3inv);
                        const double uold = A.entropy[p] * L.enttou;
                        mine[ST_TREATED]++;
                        if(S.HIReionTemp > 0 && zreion >= S.redshift && zreion < T.lastred[bin]) {
                            const double meanweight = 4 / (8 - 6 * (1 - HYDROGEN_MASSFRAC));
                            double unew = S.temp_to_u / meanweight * S.HIReionTemp;
                            if(uold > unew)
                                unew = uold;
                            A.entropy[p] = unew / L.enttou;
                            A.sfr[p] = 0;
                            evals[p] = 0;
                            mine[ST_REION]++;
                        }
                        else if(!S.CoolingOn) {
                            A.entropy[p] = 0 / L.enttou;
                            A.sfr[p] = 0;
                            evals[p] = 0;
                        }
                        else {
                            const double meanweight = 4.0 / (1 + 3 * HYDROGEN_MASSFRAC);
                            L.p = p;
                            L.dark = UVF && zreion < S.redshift;
                            if constexpr(BG == BG_J21)
                                lane_ssd = self_shield_dens(X->ss, X->gJH0 * lane_j21);
                            L.ne_guess = A.ne[p];
                            L.Z = A.metallicity ? A.metallicity[p] : 0.0;
                            L.heiii = A.heiii_ionized ? (int)A.heiii_ionized[p] : 0;
                            L.rho = density * T.a3inv * (S.density_in_phys_cgs / PROTONMASS);
                            L.u_old = uold * S.uu_in_cgs;
                            L.MinEgySpec = S.temp_to_u / meanweight * S.sfr_MinGasTemp * S.uu_in_cgs;
                            if(L.u_old < L.MinEgySpec)
                                L.u_old = L.MinEgySpec;
                            L.dt = T.dtime[bin] * S.tt_in_s;
                            L.u_lower = L.u_upper = L.u_old;
                            L.phase = PH_INIT;
                            L.guard = 0;
                            L.iter = 0;
                            lane_start_lambda(L, L.u_old);
                        }
                    }
                }
            }
        }
        if(!__any(L.p >= 0 || more))
            break;
        if(L.p >= 0) { // (an if, not a continue: all lanes of the wave meet again at the ballot above)
            // ---- one evaluation of the network (scipy_optimize_fixed_point, cooling_rates.c:784-805)
            if constexpr(UVF)
                one_evaluation(dark_setup(S, L.dark != 0), L, mine, A, evals);
            else if constexpr(BG == BG_J21)
                one_evaluation(j21_lane_setup(S, *X, lane_j21, lane_ssd), L, mine, A, evals);
            else
                one_evaluation(S, L, mine, A, evals);
        }
    }
    add_block_stats(stats, mine);
}

__global__ __launch_bounds__(COOL_BLOCK) void k_cooling_queue(Setup S, CoolTimes T, mpg_cooling_arrays A, const uint8_t *type, const float *mass,
                                                              const int *active, int64_t nlist, int64_t n, int *evals, unsigned long long *stats,
                                                              unsigned long long *queue, int use_lds)
{
    cooling_queue<BG_GLOBAL>(S, T, A, type, mass, active, nlist, n, evals, stats, queue, nullptr, use_lds);
}
// ... with a UV-fluctuation table.  The six rates of the lane's background are vector registers during an evaluation; left to itself the
// compiler ends two registers above what lets two waves share a SIMD as they do without a table, so it is told to stay within that.
__global__ __launch_bounds__(COOL_BLOCK) __attribute__((amdgpu_waves_per_eu(2))) void k_cooling_queue_uvf(
    Setup S, CoolTimes T, mpg_cooling_arrays A, const uint8_t *type, const float *mass, const int *active, int64_t nlist, int64_t n, int *evals,
    unsigned long long *stats, unsigned long long *queue, const double *zr, int use_lds)
{
    cooling_queue<BG_UVF>(S, T, A, type, mass, active, nlist, n, evals, stats, queue, zr, use_lds);
}
// ... with the excursion set's columns: two doubles per lane across the evaluations, the same limit
__global__ __launch_bounds__(COOL_BLOCK) __attribute__((amdgpu_waves_per_eu(2))) void k_cooling_queue_j21(
    Setup S, CoolTimes T, mpg_cooling_arrays A, const uint8_t *type, const float *mass, const int *active, int64_t nlist, int64_t n, int *evals,
    unsigned long long *stats, unsigned long long *queue, const double *j21, const double *zr, J21View X, int use_lds)
{
    cooling_queue<BG_J21>(S, T, A, type, mass, active, nlist, n, evals, stats, queue, zr, use_lds, j21, &X);
}

__global__ __launch_bounds__(COOL_BLOCK) void k_cooling_state(Setup S, double helium, int64_t n, const double *rho, const double *u, double *ne,
                                                              double *lambdanet, double *temp, double *nh0, unsigned long long *stats, int use_lds)
{
    S.net = stage_net_tables(S.net, use_lds != 0);
    unsigned long long mine[ST_N] = {0, 0, 0, 0, 0, 0};
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if(i < n) {
        Counters C;
        NetState N;
        double nebynh = ne[i];
        const double L = get_heatingcooling_rate(S, rho[i], u[i], helium, S.redshift, 0.0, &nebynh, C, &N);
        if(!C.error) {
            ne[i] = nebynh;
            if(lambdanet)
                lambdanet[i] = L;
            if(temp)
                temp[i] = N.temp;
            if(nh0)
                nh0[i] = N.nH0;
        }
        mine[ST_TREATED] = 1;
        mine[ST_EVALS] = C.evals;
        mine[ST_ERRORS] = C.error;
    }
    add_block_stats(stats, mine);
}

// the reionisation redshift of the UV-fluctuation table (cool::uvf_zreion), one lane per entry.  rows == 0: at the points pos[t], into
// out[t]; a point that gives NaN counts in *bad.  rows != 0: at the listed gas rows of the table of n particles (the filter of k_cooling),
// into out[p]; the cooling kernels count the NaN rows.
constexpr int UVF_BLOCK = 256;
__global__ __launch_bounds__(UVF_BLOCK) void k_uvf_zreion(const UvfView U, const double *__restrict__ pos, const uint8_t *__restrict__ type,
                                                          const float *__restrict__ mass, const int *__restrict__ active, const int64_t nlist,
                                                          const int64_t n, double *__restrict__ out, unsigned *__restrict__ bad, const int rows)
{
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if(t >= nlist)
        return;
    int64_t p = t;
    if(rows) {
        p = active ? (int64_t)active[t] : t;
        if(p < 0 || p >= n || (type ? type[p] : (uint8_t)1) != 0 || !(mass[p] > 0))
            return;
    }
    const double x[3] = {pos[3 * p], pos[3 * p + 1], pos[3 * p + 2]};
    const double z = uvf_zreion(U, x);
    out[p] = z;
    if(!rows && z != z)
        atomicAdd(bad, 1u);
}

// get_local_UVBG (cooling_uvfluc.c:236-246) at n arbitrary points, one lane per point.  j21mode == 0: the global background G for every
// point.  Otherwise get_local_UVBG_from_J21; a point without a background (j21_row_bad) gets NaN in every member and counts in *bad.
__global__ __launch_bounds__(UVF_BLOCK) void k_excursion_uvbg(const J21View X, const mpg_uvbg G, const int j21mode, const int64_t n,
                                                              const double *__restrict__ j21, const double *__restrict__ zr,
                                                              mpg_uvbg *__restrict__ out, unsigned *__restrict__ bad)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if(i >= n)
        return;
    mpg_uvbg u = G;
    if(j21mode) {
        const double J21 = j21[i], zreion = zr[i];
        if(j21_row_bad(J21, zreion)) {
            u.J_UV = u.gJH0 = u.gJHep = u.gJHe0 = u.epsH0 = u.epsHep = u.epsHe0 = u.self_shield_dens = u.zreion = NAN;
            atomicAdd(bad, 1u);
        }
        else {
            j21_rates(u, X, J21);
            u.zreion = zreion;
            u.self_shield_dens = self_shield_dens(X.ss, u.gJH0);
        }
    }
    out[i] = u;
}

void upload(DevBuf<double> &buf, const double *h, size_t count, hipStream_t st)
{
    buf.reserve(count + 1);
    MPG_HIP(hipMemcpyAsync(buf.p, h, count * sizeof(double), hipMemcpyHostToDevice, st));
    MPG_HIP(hipStreamSynchronize(st)); // (the host vector does not outlive the call)
}

} // namespace

void CoolingEngine::set_params(const mpg_cooling_params &p, hipStream_t st)
{
    MPG_CHECK(p.recomb >= Cen92 && p.recomb <= Badnell06, "mpg_set_cooling_params: recomb is none of Cen92 / Verner96 / Badnell06");
    MPG_CHECK(p.cooling >= KWH92 && p.cooling <= Sherwood, "mpg_set_cooling_params: cooling is none of KWH92 / Enzo2Nyx / Sherwood");
    MPG_CHECK(p.test_network_maxiter >= 0 && p.test_network_maxiter <= NET_MAXITER, "mpg_set_cooling_params: test_network_maxiter outside 0 .. 1000");
    std::vector<double> hnet, hcool;
    fill_tables(p.recomb, p.cooling, hnet, hcool);
    upload(net, hnet.data(), hnet.size(), st);
    upload(ctab, hcool.data(), hcool.size(), st);
    par = p;
    have_params = true;
    // the two measured design points; the environment overrides the defaults for the timing tool
    if(const char *e = getenv("MPG_COOLING_LDS"))
        lds_tables = atoi(e) != 0;
    if(const char *e = getenv("MPG_COOLING_FORM"))
        form = atoi(e) == 1;
    if(num_cus == 0) {
        int dev = 0;
        hipDeviceProp_t prop;
        MPG_HIP(hipGetDevice(&dev));
        MPG_HIP(hipGetDeviceProperties(&prop, dev));
        num_cus = prop.multiProcessorCount;
    }
}

void CoolingEngine::set_metal_table(int nz, const double *zbins, int nnh, const double *nhbins, int nt, const double *tbins, const double *rate,
                                    hipStream_t st)
{
    if(!zbins) {
        have_metal = false;
        return;
    }
    MPG_CHECK(nhbins && tbins && rate, "mpg_set_metal_cooling_table: null array");
    MPG_CHECK(nz >= 2 && nnh >= 2 && nt >= 2, "mpg_set_metal_cooling_table: every axis needs at least two bins");
    upload(metal, rate, (size_t)nz * nnh * nt, st);
    mdim[0] = nz, mdim[1] = nnh, mdim[2] = nt;
    mmin[0] = zbins[0], mmin[1] = nhbins[0], mmin[2] = tbins[0];
    mmax[0] = zbins[nz - 1], mmax[1] = nhbins[nnh - 1], mmax[2] = tbins[nt - 1];
    have_metal = true;
}

void CoolingEngine::set_uvf_table(int64_t nside, const double *table, double BoxSize, hipStream_t st)
{
    if(!table) {
        have_uvf = false;
        uvf_table.release();
        return;
    }
    // (a cube of 2^20 cells a side is far beyond any memory; the bound keeps Nside^3 inside 64 bits)
    MPG_CHECK(nside >= 2 && nside <= (1 << 20), "mpg_set_uvf_table: Nside outside 2 .. 2^20 (an axis needs two points)");
    MPG_CHECK(BoxSize > 0 && BoxSize - BoxSize == 0, "mpg_set_uvf_table: BoxSize must be positive and finite");
    const size_t count = (size_t)nside * nside * nside;
    for(size_t i = 0; i < count; i++)
        MPG_CHECK(table[i] - table[i] == 0, "mpg_set_uvf_table: table holds an entry that is not finite (entry " + std::to_string(i) + ")");
    // cooling_uvfluc.c:164
    MPG_CHECK(table[0] >= 0.01 && table[0] <= 100.0, "mpg_set_uvf_table: table[0] outside [0.01, 100] (UV Fluctuation out of range)");
    have_uvf = false;
    upload(uvf_table, table, count, st);
    uvf_nside = nside;
    uvf_box = BoxSize;
    have_uvf = true;
}

UvfView CoolingEngine::uvf_view() const
{
    UvfView U;
    U.table = uvf_table.p;
    U.nside = uvf_nside;
    U.step = (uvf_box - 0) / (uvf_nside - 1); // interp_init_dim(d, 0, BoxSize), utils/interp.c:53
    for(int d = 0; d < 3; d++)
        U.off[d] = uvf_off[d];
    return U;
}

int64_t CoolingEngine::uvf_points(int64_t n, const double *d_pos, double *d_zreion, hipStream_t st)
{
    MPG_CHECK(have_uvf, "mpg_dev_uvf_zreion: no table (mpg_set_uvf_table first)");
    if(n <= 0)
        return 0;
    uvf_bad.reserve(4);
    MPG_HIP(hipMemsetAsync(uvf_bad.p, 0, sizeof(unsigned), st));
    hipLaunchKernelGGL(k_uvf_zreion, dim3(nblk(n, UVF_BLOCK)), dim3(UVF_BLOCK), 0, st, uvf_view(), d_pos, (const uint8_t *)nullptr, (const float *)nullptr,
                       (const int *)nullptr, n, n, d_zreion, uvf_bad.p, 0);
    MPG_HIP(hipGetLastError());
    unsigned bad = 0;
    MPG_HIP(hipMemcpyAsync(&bad, uvf_bad.p, sizeof(bad), hipMemcpyDeviceToHost, st));
    MPG_HIP(hipStreamSynchronize(st));
    return bad;
}

void CoolingEngine::uvf_rows(const double *d_pos, const uint8_t *type, const float *mass, const int *d_active, int64_t nactive, int64_t n, hipStream_t st)
{
    MPG_CHECK(have_uvf, "cooling: no UV-fluctuation table");
    const int64_t nlist = d_active ? nactive : n;
    uvf_z.reserve((size_t)n + 1);
    n_uvf = n;
    if(n > 0)
        MPG_HIP(hipMemsetAsync(uvf_z.p, 0xff, (size_t)n * sizeof(double), st)); // (all bits set: a NaN)
    if(nlist > 0 && n > 0) {
        hipLaunchKernelGGL(k_uvf_zreion, dim3(nblk(nlist, UVF_BLOCK)), dim3(UVF_BLOCK), 0, st, uvf_view(), d_pos, type, mass, d_active, nlist, n, uvf_z.p,
                           (unsigned *)nullptr, 1);
        MPG_HIP(hipGetLastError());
    }
}

void CoolingEngine::set_excursion_set(const mpg_excursion_set_params *p)
{
    if(!p) {
        have_exc = false;
        exc = mpg_excursion_set_params{};
        return;
    }
    const double c[6] = {p->gJH0, p->gJHe0, p->gJHep, p->epsH0, p->epsHe0, p->epsHep};
    const char *const name[6] = {"gJH0", "gJHe0", "gJHep", "epsH0", "epsHe0", "epsHep"};
    for(int k = 0; k < 6; k++)
        MPG_CHECK(c[k] - c[k] == 0 && c[k] >= 0, std::string("mpg_set_excursion_set: the coefficient ") + name[k] + " is not finite or is negative");
    MPG_CHECK(p->ExcursionSetZStop - p->ExcursionSetZStop == 0, "mpg_set_excursion_set: ExcursionSetZStop is not finite");
    exc = *p;
    have_exc = true;
}

J21View CoolingEngine::j21_view(double redshift) const
{
    J21View X;
    X.gJH0 = exc.gJH0;
    X.gJHe0 = exc.gJHe0;
    X.epsH0 = exc.epsH0;
    X.epsHe0 = exc.epsHe0;
    X.ss = self_shield_factors(redshift, par.fBar);
    return X;
}

void CoolingEngine::check_excursion_columns(const char *who, double redshift, int64_t n) const
{
    if(!j21_mode(redshift))
        return;
    MPG_CHECK(d_j21 && d_zre, std::string(who) + ": the excursion set is on and redshift > ExcursionSetZStop, but no local_J21 / zreion columns are bound "
                                                 "(mpg_dev_set_excursion_columns, mpg_set_excursion_columns or mpg_resident_sph_set_excursion_columns first)");
    MPG_CHECK(n_exc == n, std::string(who) + ": the local_J21 / zreion columns were bound for a table of " + std::to_string(n_exc) +
                              " particles, this call is on " + std::to_string(n));
}

int64_t CoolingEngine::excursion_points(int64_t n, const double *d_J21, const double *d_zreion, double redshift, const mpg_uvbg &global,
                                        mpg_uvbg *d_out, hipStream_t st)
{
    if(n <= 0)
        return 0;
    const int jm = j21_mode(redshift);
    MPG_CHECK(!jm || have_params, "mpg_dev_excursion_uvbg: mpg_set_cooling_params has not been called (fBar)");
    exc_bad.reserve(4);
    MPG_HIP(hipMemsetAsync(exc_bad.p, 0, sizeof(unsigned), st));
    hipLaunchKernelGGL(k_excursion_uvbg, dim3(nblk(n, UVF_BLOCK)), dim3(UVF_BLOCK), 0, st, jm ? j21_view(redshift) : J21View{}, global, jm, n, d_J21,
                       d_zreion, d_out, exc_bad.p);
    MPG_HIP(hipGetLastError());
    unsigned bad = 0;
    MPG_HIP(hipMemcpyAsync(&bad, exc_bad.p, sizeof(bad), hipMemcpyDeviceToHost, st));
    MPG_HIP(hipStreamSynchronize(st));
    return bad;
}

Setup CoolingEngine::setup(const mpg_cooling_step &step, double redshift) const
{
    Setup S{};
    S.recomb = par.recomb;
    S.cooling = par.cooling;
    S.SelfShieldingOn = par.SelfShieldingOn;
    S.HeliumHeatOn = par.HeliumHeatOn;
    S.CoolingOn = par.CoolingOn;
    S.net_maxiter = par.test_network_maxiter > 0 ? par.test_network_maxiter : NET_MAXITER;
    S.CMBTemperature = par.CMBTemperature;
    S.MinGasTemp = par.MinGasTemp;
    S.HeliumHeatThresh = par.HeliumHeatThresh;
    S.HeliumHeatAmp = par.HeliumHeatAmp;
    S.HeliumHeatExp = par.HeliumHeatExp;
    S.rho_crit_baryon = par.rho_crit_baryon;
    S.density_in_phys_cgs = par.density_in_phys_cgs;
    S.uu_in_cgs = par.uu_in_cgs;
    S.tt_in_s = par.tt_in_s;
    S.units_rho_crit_baryon = par.units_rho_crit_baryon;
    S.sfr_MinGasTemp = par.sfr_MinGasTemp;
    S.temp_to_u = par.temp_to_u;
    S.HIReionTemp = par.HIReionTemp;
    S.tmax = log(1e9);
    S.uvbg = step.uvbg;
    S.redshift = redshift;
    S.lmfp_heating = step.long_mean_free_path_heating;
    S.net = net.p;
    S.ctab = ctab.p;
    S.metal = have_metal ? metal.p : nullptr;
    for(int d = 0; d < 3; d++) {
        S.mdim[d] = mdim[d];
        S.mmin[d] = mmin[d];
        S.mmax[d] = mmax[d];
        S.mstep[d] = have_metal ? (mmax[d] - mmin[d]) / (mdim[d] - 1) : 1.0; // interp_init_dim, utils/interp.c:50-54
    }
    return S;
}

static void fetch_stats(CoolingEngine &E, hipStream_t st)
{
    unsigned long long h[ST_N];
    MPG_HIP(hipMemcpyAsync(h, E.d_stats.p, sizeof(h), hipMemcpyDeviceToHost, st));
    MPG_HIP(hipStreamSynchronize(st));
    for(int k = 0; k < ST_N; k++)
        E.stats[k] = (int64_t)h[k];
}

int64_t CoolingEngine::run(const mpg_cooling_arrays &A, const uint8_t *type, const float *mass, const mpg_sph_times &T, const mpg_cooling_step &step,
                           const int *d_active, int64_t nactive, int64_t n, hipStream_t st)
{
    MPG_CHECK(have_params, "cooling: mpg_set_cooling_params has not been called");
    const int64_t nlist = d_active ? nactive : n;
    const double redshift = 1 / T.atime - 1; // sfr_eff.c:211
    const bool jm = j21_mode(redshift);
    check_excursion_columns("cooling", redshift, n);
    d_stats.reserve(ST_N + 1); // (the last entry is the list position of the queue form)
    d_evals.reserve((size_t)n + 1);
    n_evals = n;
    MPG_HIP(hipMemsetAsync(d_stats.p, 0, (ST_N + 1) * sizeof(unsigned long long), st));
    if(n > 0)
        MPG_HIP(hipMemsetAsync(d_evals.p, 0xff, (size_t)n * sizeof(int), st));
    if(nlist > 0) {
        const Setup S = setup(step, redshift);
        CoolTimes CT;
        for(int b = 0; b < 47; b++) {
            CT.dtime[b] = T.dloga_bin[b] / T.hubble;
            CT.lastred[b] = step.lastred[b];
        }
        CT.a3inv = 1. / (T.atime * T.atime * T.atime); // sfr_eff.c:195
        const size_t lds = lds_tables ? (size_t)NRECOMBTAB * NNET * sizeof(double) : 0;
        const unsigned blocks = (unsigned)((nlist + COOL_BLOCK - 1) / COOL_BLOCK);
        // get_local_UVBG: the excursion set's columns above ExcursionSetZStop, else the table's zreion, else the global background
        const bool uvf = have_uvf && !jm;
        MPG_CHECK(!uvf || n_uvf == n, "cooling: the zreion column was not filled for this table");
        const double *zr = uvf ? uvf_z.p : nullptr;
        const J21View X = jm ? j21_view(redshift) : J21View{};
        if(form == 1) {
            // resident waves that pull from the list: no more blocks than keep every CU busy
            const unsigned cap = (unsigned)num_cus * 8u;
            const dim3 grid(blocks < cap ? blocks : cap);
            if(jm)
                hipLaunchKernelGGL(k_cooling_queue_j21, grid, dim3(COOL_BLOCK), lds, st, S, CT, A, type, mass, d_active, nlist, n, d_evals.p, d_stats.p,
                                   d_stats.p + ST_N, d_j21, d_zre, X, lds_tables);
            else if(uvf)
                hipLaunchKernelGGL(k_cooling_queue_uvf, grid, dim3(COOL_BLOCK), lds, st, S, CT, A, type, mass, d_active, nlist, n, d_evals.p, d_stats.p,
                                   d_stats.p + ST_N, zr, lds_tables);
            else
                hipLaunchKernelGGL(k_cooling_queue, grid, dim3(COOL_BLOCK), lds, st, S, CT, A, type, mass, d_active, nlist, n, d_evals.p, d_stats.p,
                                   d_stats.p + ST_N, lds_tables);
        }
        else if(jm)
            hipLaunchKernelGGL(k_cooling_j21, dim3(blocks), dim3(COOL_BLOCK), lds, st, S, CT, A, type, mass, d_active, nlist, n, d_evals.p, d_stats.p, d_j21,
                               d_zre, X, lds_tables);
        else if(uvf)
            hipLaunchKernelGGL(k_cooling_uvf, dim3(blocks), dim3(COOL_BLOCK), lds, st, S, CT, A, type, mass, d_active, nlist, n, d_evals.p, d_stats.p, zr,
                               lds_tables);
        else
            hipLaunchKernelGGL(k_cooling, dim3(blocks), dim3(COOL_BLOCK), lds, st, S, CT, A, type, mass, d_active, nlist, n, d_evals.p, d_stats.p,
                               lds_tables);
        MPG_HIP(hipGetLastError());
    }
    fetch_stats(*this, st);
    return stats[ST_ERRORS];
}

int64_t CoolingEngine::state(int64_t n, const double *rho, const double *u, double *ne, double *lambdanet, double *temp, double *nh0,
                             const mpg_cooling_step &step, hipStream_t st)
{
    MPG_CHECK(have_params, "cooling: mpg_set_cooling_params has not been called");
    d_stats.reserve(ST_N + 1);
    MPG_HIP(hipMemsetAsync(d_stats.p, 0, ST_N * sizeof(unsigned long long), st));
    if(n > 0) {
        const Setup S = setup(step, step.redshift);
        const double helium = step.helium > 0 ? step.helium : 1 - HYDROGEN_MASSFRAC;
        const size_t lds = lds_tables ? (size_t)NRECOMBTAB * NNET * sizeof(double) : 0;
        const unsigned blocks = (unsigned)((n + COOL_BLOCK - 1) / COOL_BLOCK);
        hipLaunchKernelGGL(k_cooling_state, dim3(blocks), dim3(COOL_BLOCK), lds, st, S, helium, n, rho, u, ne, lambdanet, temp, nh0, d_stats.p,
                           lds_tables);
        MPG_HIP(hipGetLastError());
    }
    unsigned long long h[ST_N];
    MPG_HIP(hipMemcpyAsync(h, d_stats.p, sizeof(h), hipMemcpyDeviceToHost, st));
    MPG_HIP(hipStreamSynchronize(st));
    return (int64_t)h[ST_ERRORS];
}

} // namespace mpg
