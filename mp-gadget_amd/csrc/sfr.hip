// sfr.hip -- the loop of cooling_and_starformation (sfr_eff.c:224-286) without the spawning, for gfx950, fp64; the model is sfr.h's, the
// network cooling.h's.  Three stages, each one lane per entry: the class of every listed row (k_sfr_classify), cooling_direct on the rows that
// do not form stars (CoolingEngine::run on their compacted list), starformation on the others (k_sfr_eeqos).  Both compactions keep the
// order of the active list: per-block counts, one scan, one push.  DESIGN 3.15.
#include "sfr.h"

namespace mpg {

using namespace sfr;

namespace {

constexpr int SFR_BLOCK = 256, SFR_WAVES = SFR_BLOCK / 64;
// words of the counters of k_sfr_eeqos
enum { SC_EVALS = 0, SC_ERRORS, SC_SPAWNED, SC_N };

struct SfrTimes {
    double dloga[47]; // get_dloga_for_bin
    double hubble, atime, a3inv;
};
struct SfrScalars {
    mpg_sfr_params p;
    mpg_wind_params w; // read by winds_evolve only, i.e. with a delaytime column
    const double *rnd; // RandTable.Table
    uint64_t rndsize;
};

// the rank of this lane among the lanes of its block for which `pred` holds, in thread order, and their number.  wc: SFR_WAVES words of LDS
// that belong to this call.  Every thread of the block calls it.
__device__ __forceinline__ unsigned block_rank(const bool pred, unsigned *wc, unsigned *total)
{
    const unsigned long long m = __ballot(pred);
    const int lane = __lane_id(), w = threadIdx.x >> 6;
    if(lane == 0)
        wc[w] = (unsigned)__popcll(m);
    __syncthreads();
    unsigned before = 0, tot = 0;
    for(int k = 0; k < SFR_WAVES; k++) {
        if(k < w)
            before += wc[k];
        tot += wc[k];
    }
    *total = tot;
    return before + (unsigned)__popcll(m & ((1ull << lane) - 1));
}

__device__ __forceinline__ double wave_sum(double v)
{
    for(int off = 32; off > 0; off >>= 1)
        v += __shfl_down(v, off);
    return v; // (lane 0 holds the sum; the order of the additions is fixed)
}
__device__ __forceinline__ unsigned wave_sum(unsigned v)
{
    for(int off = 32; off > 0; off >>= 1)
        v += __shfl_down(v, off);
    return v;
}

// the filter of sfr_eff.c:229, winds_evolve (:235) and the class (:237-240) of every list entry
__global__ __launch_bounds__(SFR_BLOCK) void k_sfr_classify(const double temp_to_u, const SfrTimes T, const SfrScalars P, const SfrView A,
                                                            const int *__restrict__ active, const int64_t nlist, uint8_t *__restrict__ cls,
                                                            uint8_t *__restrict__ rowclass, unsigned *__restrict__ blockcnt)
{
    __shared__ unsigned wc[2][SFR_WAVES];
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    int c = ROW_SKIPPED;
    if(t < nlist) {
        int64_t p = active ? (int64_t)active[t] : t;
        // a list entry outside the table is ignored; non-gas, garbage (type 7) and massless rows are skipped, as in k_cooling
        if(p < 0 || p >= A.n || (A.type ? A.type[p] : (uint8_t)1) != 0 || !(A.mass[p] > 0))
            p = -1;
        if(p >= 0) {
            const int bin = A.a.tb_hydro ? (A.a.tb_hydro[p] < 47 ? A.a.tb_hydro[p] : 46) : 0;
            const double density = A.a.density[p];
            double delay = 0;
            if(A.a.delaytime) {
                const double before = A.a.delaytime[p];
                delay = wind_evolve_delay(P.w, before, density, T.a3inv, T.dloga[bin] / T.hubble); // winds.h; a bin beyond 46 is read as 46 here
                if(delay != before)
                    A.a.delaytime[p] = delay;
            }
            int sf;
            if(P.p.QuickLymanAlphaProbability > 0)
                sf = quicklyastarformation(P.p, temp_to_u, density, A.a.entropy[p], T.a3inv, P.rnd[(A.a.id[p] + 1ull) % P.rndsize]);
            else
                sf = sfreff_on_eeqos(P.p, density, delay, T.a3inv);
            c = sf ? ROW_STARFORMING : ROW_COOLED;
            rowclass[p] = (uint8_t)c;
        }
        cls[t] = (uint8_t)c;
    }
    unsigned na, nb;
    block_rank(c == ROW_COOLED, wc[0], &na);
    block_rank(c == ROW_STARFORMING, wc[1], &nb);
    if(threadIdx.x == 0) {
        blockcnt[2 * blockIdx.x] = na;
        blockcnt[2 * blockIdx.x + 1] = nb;
    }
}

// one block: the two interleaved sequences of per-block counts become their exclusive prefix sums, totals[0 .. 1] their sums; and, when
// `partial` is given, the nb per-block partial sums of each of three quantities are added in a fixed order into sums[0 .. 2]
__global__ __launch_bounds__(SFR_BLOCK) void k_sfr_scan(unsigned *__restrict__ blockcnt, const int64_t nb, unsigned *__restrict__ totals,
                                                        const double *__restrict__ partial, double *__restrict__ sums)
{
    __shared__ unsigned sa[SFR_BLOCK], sb[SFR_BLOCK];
    __shared__ double sd[3][SFR_BLOCK];
    const int tid = threadIdx.x;
    const int64_t per = (nb + SFR_BLOCK - 1) / SFR_BLOCK, lo = tid * per, hi = lo + per < nb ? lo + per : nb;
    unsigned a = 0, b = 0;
    for(int64_t k = lo; k < hi; k++) {
        a += blockcnt[2 * k];
        b += blockcnt[2 * k + 1];
    }
    sa[tid] = a;
    sb[tid] = b;
    if(partial) {
        double d[3] = {0, 0, 0};
        for(int64_t k = lo; k < hi; k++)
            for(int j = 0; j < 3; j++)
                d[j] += partial[3 * k + j];
        for(int j = 0; j < 3; j++)
            sd[j][tid] = d[j];
    }
    __syncthreads();
    if(tid == 0) {
        unsigned ra = 0, rb = 0;
        for(int k = 0; k < SFR_BLOCK; k++) {
            const unsigned xa = sa[k], xb = sb[k];
            sa[k] = ra;
            sb[k] = rb;
            ra += xa;
            rb += xb;
        }
        totals[0] = ra;
        totals[1] = rb;
        if(partial)
            for(int j = 0; j < 3; j++) {
                double s = 0;
                for(int k = 0; k < SFR_BLOCK; k++)
                    s += sd[j][k];
                sums[j] = s;
            }
    }
    __syncthreads();
    a = sa[tid];
    b = sb[tid];
    for(int64_t k = lo; k < hi; k++) {
        const unsigned xa = blockcnt[2 * k], xb = blockcnt[2 * k + 1];
        blockcnt[2 * k] = a;
        blockcnt[2 * k + 1] = b;
        a += xa;
        b += xb;
    }
}

// the rows of the two classes into their lists, in list order
__global__ __launch_bounds__(SFR_BLOCK) void k_sfr_push(const uint8_t *__restrict__ cls, const int *__restrict__ active, const int64_t nlist,
                                                        const unsigned *__restrict__ blockoff, int *__restrict__ coollist, int *__restrict__ sflist)
{
    __shared__ unsigned wc[2][SFR_WAVES];
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int c = t < nlist ? cls[t] : ROW_SKIPPED;
    unsigned na, nb;
    const unsigned ra = block_rank(c == ROW_COOLED, wc[0], &na), rb = block_rank(c == ROW_STARFORMING, wc[1], &nb);
    if(c == ROW_SKIPPED)
        return;
    const int p = active ? active[t] : (int)t;
    if(c == ROW_COOLED)
        coollist[blockoff[2 * blockIdx.x] + ra] = p;
    else
        sflist[blockoff[2 * blockIdx.x + 1] + rb] = p;
}

// starformation (sfr_eff.c:731-800) for every row of the star-forming list: one lane per row, 2 .. 3 solves of the network.  UVF: under the
// row's own background (sfr_eff.c:745; zr by particle, cool::local_setup); a row whose zreion is NaN is an error row.  J21: under the
// background of the row's J21 and zreion (cool::j21_setup, X the model); a row that cool::j21_row_bad names is an error row.
template <bool UVF, bool J21>
__device__ __forceinline__ void sfr_eeqos_rows(const Setup &S, const SfrTimes &T, const SfrScalars &P, const SfrView &A, const int *__restrict__ sflist,
                                               const int64_t nsf, uint8_t *__restrict__ outcome, double *__restrict__ sfmass, int *__restrict__ sfevals,
                                               unsigned *__restrict__ blockcnt, double *__restrict__ partial, unsigned long long *__restrict__ ctr,
                                               const double *__restrict__ zr, const double *__restrict__ j21 = nullptr, const J21View *X = nullptr)
{
    __shared__ unsigned wc[2][SFR_WAVES];
    __shared__ double ws[3][SFR_WAVES];
    const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    int out = -1;
    double s[3] = {0, 0, 0}; // sum_sm, localsfr, sum_dtime
    unsigned evals = 0;
    if(q < nsf) {
        const int64_t p = sflist[q];
        const mpg_sfr_columns &a = A.a;
        const float mass = A.mass[p];
        if(P.p.QuickLymanAlphaProbability > 0) {
            // sfr_eff.c:247-251: the particle itself becomes the star; find_star_mass (:1006-1007)
            out = OUT_CONVERT;
            s[0] = mass;
            sfmass[q] = mass;
            sfevals[p] = 0;
        }
        else {
            Row r;
            r.density = a.density[p];
            r.entropy = a.entropy[p];
            r.ne = a.ne[p];
            r.metallicity = a.metallicity[p];
            r.delaytime = a.delaytime ? a.delaytime[p] : 0.0;
            r.hsml = a.hsml ? a.hsml[p] : 0.0;
            r.divvel = a.divvel ? a.divvel[p] : 0.0;
            r.curlvel = a.curlvel ? a.curlvel[p] : 0.0;
            r.gradrho_mag = a.gradrho_mag ? a.gradrho_mag[p] : 0.0;
            r.mass = mass;
            r.generation = a.generation ? a.generation[p] : 0;
            r.bhheated = a.bhheated ? a.bhheated[p] : 0;
            const int bin = a.tb_hydro ? (a.tb_hydro[p] < 47 ? a.tb_hydro[p] : 46) : 0;
            r.tb_hydro = bin;
            const unsigned long long id = a.id[p];
            Counters C;
            RowResult o;
            if constexpr(UVF) {
                const double zreion = zr[p];
                if(zreion != zreion) {
                    o = RowResult{};
                    o.outcome = OUT_ERROR;
                }
                else
                    o = starformation(local_setup(S, zreion), P.p, r, T.dloga[bin], T.hubble, T.atime, T.a3inv, P.rnd[id % P.rndsize],
                                      P.rnd[(id + 1ull) % P.rndsize], C);
            }
            else if constexpr(J21) {
                const double zreion = zr[p], local_J21 = j21[p];
                if(j21_row_bad(local_J21, zreion)) {
                    o = RowResult{};
                    o.outcome = OUT_ERROR;
                }
                else
                    o = starformation(j21_setup(S, *X, local_J21, zreion), P.p, r, T.dloga[bin], T.hubble, T.atime, T.a3inv, P.rnd[id % P.rndsize],
                                      P.rnd[(id + 1ull) % P.rndsize], C);
            }
            else
                o = starformation(S, P.p, r, T.dloga[bin], T.hubble, T.atime, T.a3inv, P.rnd[id % P.rndsize], P.rnd[(id + 1ull) % P.rndsize], C);
            out = o.outcome;
            evals = (unsigned)C.evals;
            sfevals[p] = C.evals;
            sfmass[q] = o.mass_of_star;
            if(out != OUT_ERROR) {
                a.entropy[p] = o.entropy;
                a.ne[p] = o.ne;
                a.sfr[p] = o.sfr;
                a.metallicity[p] = o.metallicity;
                if(a.bhheated && o.bhheated != r.bhheated)
                    a.bhheated[p] = (uint8_t)o.bhheated;
                if(a.stellarmass && out == OUT_NOSTAR)
                    a.stellarmass[p] = o.sm;
                s[0] = o.dM;
                s[1] = o.sfr;
                s[2] = o.dtime;
            }
        }
        outcome[q] = (uint8_t)out;
    }
    unsigned na, nb;
    block_rank(out == OUT_CONVERT || out == OUT_SPAWN, wc[0], &na);
    block_rank(out == OUT_NOSTAR, wc[1], &nb);
    const int lane = __lane_id(), w = threadIdx.x >> 6;
    for(int j = 0; j < 3; j++) {
        const double v = wave_sum(s[j]);
        if(lane == 0)
            ws[j][w] = v;
    }
    const unsigned ev = wave_sum(evals), er = wave_sum(out == OUT_ERROR ? 1u : 0u), sp = wave_sum(out == OUT_SPAWN ? 1u : 0u);
    if(lane == 0) {
        if(ev)
            atomicAdd(ctr + SC_EVALS, (unsigned long long)ev);
        if(er)
            atomicAdd(ctr + SC_ERRORS, (unsigned long long)er);
        if(sp)
            atomicAdd(ctr + SC_SPAWNED, (unsigned long long)sp);
    }
    __syncthreads();
    if(threadIdx.x == 0) {
        blockcnt[2 * blockIdx.x] = na;
        blockcnt[2 * blockIdx.x + 1] = nb;
        for(int j = 0; j < 3; j++) {
            double v = 0;
            for(int k = 0; k < SFR_WAVES; k++)
                v += ws[j][k];
            partial[3 * blockIdx.x + j] = v;
        }
    }
}

template <bool UVF>
__global__ __launch_bounds__(SFR_BLOCK) void k_sfr_eeqos(const Setup S, const SfrTimes T, const SfrScalars P, const SfrView A, const int *__restrict__ sflist,
                                                         const int64_t nsf, uint8_t *__restrict__ outcome, double *__restrict__ sfmass,
                                                         int *__restrict__ sfevals, unsigned *__restrict__ blockcnt, double *__restrict__ partial,
                                                         unsigned long long *__restrict__ ctr, const double *__restrict__ zr)
{
    sfr_eeqos_rows<UVF, false>(S, T, P, A, sflist, nsf, outcome, sfmass, sfevals, blockcnt, partial, ctr, zr);
}
__global__ __launch_bounds__(SFR_BLOCK) void k_sfr_eeqos_j21(const Setup S, const SfrTimes T, const SfrScalars P, const SfrView A, const int *__restrict__ sflist,
                                                             const int64_t nsf, uint8_t *__restrict__ outcome, double *__restrict__ sfmass,
                                                             int *__restrict__ sfevals, unsigned *__restrict__ blockcnt, double *__restrict__ partial,
                                                             unsigned long long *__restrict__ ctr, const double *__restrict__ j21,
                                                             const double *__restrict__ zr, const J21View X)
{
    sfr_eeqos_rows<false, true>(S, T, P, A, sflist, nsf, outcome, sfmass, sfevals, blockcnt, partial, ctr, zr, j21, &X);
}

// the new-star list and the MaybeWind list from the outcomes, in list order
__global__ __launch_bounds__(SFR_BLOCK) void k_sfr_lists(const uint8_t *__restrict__ outcome, const int *__restrict__ sflist, const double *__restrict__ sfmass,
                                                         const int64_t nsf, const unsigned *__restrict__ blockoff, int *__restrict__ ns_parent,
                                                         double *__restrict__ ns_mass, uint8_t *__restrict__ ns_spawn, int *__restrict__ maybewind)
{
    __shared__ unsigned wc[2][SFR_WAVES];
    const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int out = q < nsf ? outcome[q] : -1;
    const bool star = out == OUT_CONVERT || out == OUT_SPAWN;
    unsigned na, nb;
    const unsigned ra = block_rank(star, wc[0], &na), rb = block_rank(out == OUT_NOSTAR, wc[1], &nb);
    if(star) {
        const unsigned k = blockoff[2 * blockIdx.x] + ra;
        ns_parent[k] = sflist[q];
        ns_mass[k] = sfmass[q];
        ns_spawn[k] = out == OUT_SPAWN;
    }
    else if(out == OUT_NOSTAR && maybewind)
        maybewind[blockoff[2 * blockIdx.x + 1] + rb] = sflist[q];
}

} // namespace

void SfrEngine::set_params(const mpg_sfr_params &p, bool have_uvf_table, bool have_excursion_set)
{
    // what the engine does not carry is refused when it is set, so that a caller keeps its CPU path from the start
    MPG_CHECK(p.BHFeedbackUseTcool != 2, "star formation: BHFeedbackUseTcool == 2 is not carried (get_egyeff in sfreff_on_eeqos)");
    MPG_CHECK(p.BHFeedbackUseTcool >= 0 && p.BHFeedbackUseTcool <= 3, "star formation: BHFeedbackUseTcool mode not supported");
    MPG_CHECK(!p.UVFluctuationOn || have_uvf_table, "star formation: UVFluctuationOn without a UV-fluctuation table on this engine (mpg_set_uvf_table first)");
    MPG_CHECK(!p.ExcursionSetReion || have_excursion_set,
              "star formation: ExcursionSetReion (EXCUR_REION) without an excursion-set model on this engine (mpg_set_excursion_set first)");
    MPG_CHECK(p.NTask <= 1, "star formation: NTask > 1 is not carried; several ranks keep the CPU function");
    MPG_CHECK(p.Generations >= 1 && p.Generations <= 14, "star formation: Generations outside 1 .. 14");
    MPG_CHECK(p.PhysDensThresh > 0 && p.MaxSfrTimescale > 0, "star formation: PhysDensThresh and MaxSfrTimescale must be positive (after init_cooling_and_star_formation)");
    par = p;
    have_params = true;
}

int64_t SfrEngine::run(CoolingEngine &cooling, const SfrView &A, const mpg_wind_params *wind, const double *rnd, uint64_t rndsize, const mpg_sph_times &T,
                       const mpg_cooling_step &step, const int *d_active, int64_t nactive, hipStream_t st)
{
    const int64_t n = A.n, nlist = d_active ? nactive : n;
    const unsigned nb = nblk(nlist, SFR_BLOCK);
    cls.reserve(nlist + 1);
    coollist.reserve(nlist + 1);
    sflist.reserve(nlist + 1);
    rowclass.reserve(n + 1);
    sfevals.reserve(n + 1);
    blockcnt.reserve(2 * (size_t)nb + 2);
    totals.reserve(4);
    sums.reserve(4);
    n_rows = n;
    last = mpg_sfr_result{};
    for(int64_t &s : last_stats)
        s = 0;
    last_stats[0] = nlist;
    if(n > 0) {
        MPG_HIP(hipMemsetAsync(rowclass.p, 0, (size_t)n, st));
        MPG_HIP(hipMemsetAsync(sfevals.p, 0xff, (size_t)n * sizeof(int), st));
    }
    SfrTimes ST;
    for(int b = 0; b < 47; b++)
        ST.dloga[b] = T.dloga_bin[b];
    ST.hubble = T.hubble;
    ST.atime = T.atime;
    ST.a3inv = 1. / (T.atime * T.atime * T.atime); // sfr_eff.c:195
    SfrScalars P{};
    P.p = par;
    if(wind)
        P.w = *wind;
    P.rnd = rnd;
    P.rndsize = rndsize;
    unsigned tot[2] = {0, 0};
    const double redshift = 1 / T.atime - 1; // sfr_eff.c:211
    const bool jm = cooling.j21_mode(redshift);
    cooling.check_excursion_columns("cooling_and_starformation", redshift, n);
    const bool uvf = cooling.have_uvf && !jm;
    // the zreion of every listed gas row, cooled or star-forming, before either kernel reads it
    if(uvf)
        cooling.uvf_rows(A.pos, A.type, A.mass, d_active, nactive, n, st);
    if(nlist > 0) {
        hipLaunchKernelGGL(k_sfr_classify, dim3(nb), dim3(SFR_BLOCK), 0, st, cooling.par.temp_to_u, ST, P, A, d_active, nlist, cls.p, rowclass.p, blockcnt.p);
        hipLaunchKernelGGL(k_sfr_scan, dim3(1), dim3(SFR_BLOCK), 0, st, blockcnt.p, (int64_t)nb, totals.p, (const double *)nullptr, (double *)nullptr);
        hipLaunchKernelGGL(k_sfr_push, dim3(nb), dim3(SFR_BLOCK), 0, st, cls.p, d_active, nlist, blockcnt.p, coollist.p, sflist.p);
        MPG_HIP(hipGetLastError());
        MPG_HIP(hipMemcpyAsync(tot, totals.p, sizeof(tot), hipMemcpyDeviceToHost, st));
        MPG_HIP(hipStreamSynchronize(st));
    }
    const int64_t ncool = tot[0], nsf = tot[1];
    MPG_CHECK(ncool + nsf <= nlist, "star formation: the two lists are longer than the active list");
    last.cooled = ncool;
    last.sum_sf_part = nsf;
    last.treated = ncool + nsf;
    // cooling_direct for the rows that do not form stars: the cooling kernel of mpg_dev_cooling, whichever form was chosen, on their list
    mpg_cooling_arrays CA{};
    CA.density = A.a.density;
    CA.entropy = A.a.entropy;
    CA.ne = A.a.ne;
    CA.sfr = A.a.sfr;
    CA.metallicity = A.a.metallicity;
    CA.heiii_ionized = A.a.heiii_ionized;
    CA.tb_hydro = A.a.tb_hydro;
    const int64_t bad_cool = cooling.run(CA, A.type, A.mass, T, step, coollist.p, ncool, n, st);
    int64_t bad_sf = 0;
    if(nsf > 0) {
        const unsigned nb2 = nblk(nsf, SFR_BLOCK);
        outcome.reserve(nsf + 1);
        sfmass.reserve(nsf + 1);
        ns_parent.reserve(nsf + 1);
        ns_mass.reserve(nsf + 1);
        ns_spawn.reserve(nsf + 1);
        maybewind.reserve(nsf + 1);
        partial.reserve(3 * (size_t)nb2 + 3);
        ctr.reserve(SC_N);
        MPG_HIP(hipMemsetAsync(ctr.p, 0, SC_N * sizeof(unsigned long long), st));
        const Setup S = cooling.setup(step, redshift);
        if(jm)
            hipLaunchKernelGGL(k_sfr_eeqos_j21, dim3(nb2), dim3(SFR_BLOCK), 0, st, S, ST, P, A, sflist.p, nsf, outcome.p, sfmass.p, sfevals.p, blockcnt.p,
                               partial.p, ctr.p, cooling.d_j21, cooling.d_zre, cooling.j21_view(redshift));
        else
            hipLaunchKernelGGL(uvf ? k_sfr_eeqos<true> : k_sfr_eeqos<false>, dim3(nb2), dim3(SFR_BLOCK), 0, st, S, ST, P, A, sflist.p, nsf, outcome.p,
                               sfmass.p, sfevals.p, blockcnt.p, partial.p, ctr.p, uvf ? (const double *)cooling.uvf_z.p : (const double *)nullptr);
        hipLaunchKernelGGL(k_sfr_scan, dim3(1), dim3(SFR_BLOCK), 0, st, blockcnt.p, (int64_t)nb2, totals.p, (const double *)partial.p, sums.p);
        hipLaunchKernelGGL(k_sfr_lists, dim3(nb2), dim3(SFR_BLOCK), 0, st, outcome.p, sflist.p, sfmass.p, nsf, blockcnt.p, ns_parent.p, ns_mass.p, ns_spawn.p,
                           A.a.stellarmass ? maybewind.p : (int *)nullptr);
        MPG_HIP(hipGetLastError());
        unsigned long long c[SC_N];
        double s[3];
        MPG_HIP(hipMemcpyAsync(tot, totals.p, sizeof(tot), hipMemcpyDeviceToHost, st));
        MPG_HIP(hipMemcpyAsync(c, ctr.p, sizeof(c), hipMemcpyDeviceToHost, st));
        MPG_HIP(hipMemcpyAsync(s, sums.p, sizeof(s), hipMemcpyDeviceToHost, st));
        MPG_HIP(hipStreamSynchronize(st));
        last.newstars = tot[0];
        last.spawned = (int64_t)c[SC_SPAWNED];
        last.converted = last.newstars - last.spawned;
        last.maybewind = A.a.stellarmass ? tot[1] : 0;
        last.sum_sm = s[0];
        last.localsfr = s[1];
        last.sum_dtime = s[2];
        last_stats[4] = (int64_t)c[SC_EVALS];
        bad_sf = (int64_t)c[SC_ERRORS];
    }
    last.errors = bad_cool + bad_sf;
    last_stats[1] = last.treated;
    last_stats[2] = ncool;
    last_stats[3] = nsf;
    last_stats[5] = bad_sf;
    last_stats[6] = last.newstars;
    last_stats[7] = last.maybewind;
    return last.errors;
}

} // namespace mpg
