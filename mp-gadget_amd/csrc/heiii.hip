// heiii.hip -- helium reionisation by quasar bubbles: do_heiii_reionization / turn_on_quasars (cooling_qso_lightup.c:523-659) for one rank.
//
// The reference lights one bubble at a time: a tree walk around the chosen group, then a sum, then the next choice.  Here the sequence of
// choices and the radii are the host's (they depend on the random table and the candidate list alone, never on the counts), and the gas is
// scanned once per BATCH of the next B iterations: a lane per row keeps the FIRST bubble of the batch that covers it, a wave adds its rows
// into a histogram of the block, a block adds its non-zero words into B global counters.  The host reads the B counts, replays the
// reference's loop on them in the reference's order of double operations and finds where it stops; an apply pass then ionises and heats
// exactly the rows whose first cover lies before the stop.  No tree is read or built.  DESIGN 3.14 has the equivalence arguments.
#include "heiii.h"
#include <cmath>

namespace mpg {

// the rows of type 0 with the flag (gas_ionization_fraction, :372-376): ballot and popcount per wave, one atomic per block
__global__ void __launch_bounds__(256) k_heiii_count(const HeiiiView A, unsigned long long *__restrict__ out)
{
    __shared__ unsigned s_n;
    if(threadIdx.x == 0)
        s_n = 0;
    __syncthreads();
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const bool is = i < A.n && (A.type[i] & 7) == 0 && A.flag[i] != 0;
    const unsigned long long m = __ballot(is);
    if(m != 0 && (int)__lane_id() == __ffsll((long long)m) - 1)
        atomicAdd(&s_n, (unsigned)__popcll(m));
    __syncthreads();
    if(threadIdx.x == 0 && s_n != 0)
        atomicAdd(out, (unsigned long long)s_n);
}

// the flash branch (:539-548): every row of type 0 through ionize_single_particle; counted as above
__global__ void __launch_bounds__(256) k_heiii_flash(const HeiiiView A, double a3inv, double du, unsigned long long *__restrict__ out)
{
    __shared__ unsigned s_n;
    if(threadIdx.x == 0)
        s_n = 0;
    __syncthreads();
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    bool did = false;
    if(i < A.n && (A.type[i] & 7) == 0 && A.flag[i] == 0) {
        uint8_t f = 0;
        double e = A.entropy[i];
        did = heiii_ionize_row(f, e, A.density[i], a3inv, du) != 0;
        A.flag[i] = f;
        A.entropy[i] = e;
    }
    const unsigned long long m = __ballot(did);
    if(m != 0 && (int)__lane_id() == __ffsll((long long)m) - 1)
        atomicAdd(&s_n, (unsigned)__popcll(m));
    __syncthreads();
    if(threadIdx.x == 0 && s_n != 0)
        atomicAdd(out, (unsigned long long)s_n);
}

// the scan of a batch.  A row takes part if its type is 0 and its flag 0 (ionize_ngbiter :443, ionize_single_particle :392; garbage rows
// carry type 7).  The batch is a kernel argument and k is wave-uniform: the centres and radii arrive by scalar loads.
__global__ void __launch_bounds__(256) k_heiii_scan(const HeiiiView A, const HeiiiBatch bt, unsigned *__restrict__ first,
                                                    unsigned long long *__restrict__ counts)
{
    __shared__ unsigned s_hist[HEIII_MAXB];
    if(threadIdx.x < HEIII_MAXB)
        s_hist[threadIdx.x] = 0;
    __syncthreads();
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    unsigned f = HEIII_NONE;
    if(i < A.n && (A.type[i] & 7) == 0 && A.flag[i] == 0) {
        const double px = A.pos[3 * i], py = A.pos[3 * i + 1], pz = A.pos[3 * i + 2];
        for(int k = 0; k < bt.nb; k++)
            if(heiii_covers(px, py, pz, bt.b[k], bt.box)) {
                f = (unsigned)k;
                break;
            }
    }
    if(i < A.n)
        first[i] = f;
    // the wave's rows into the block's histogram: one LDS atomic per distinct bubble of the wave
    unsigned long long todo = __ballot(f != HEIII_NONE);
    while(todo != 0) {
        const int leader = __ffsll((long long)todo) - 1;
        const unsigned v = __shfl(f, leader);
        const unsigned long long same = __ballot(f == v);
        if((int)__lane_id() == leader)
            atomicAdd(&s_hist[v], (unsigned)__popcll(same));
        todo &= ~same;
    }
    __syncthreads();
    if((int)threadIdx.x < bt.nb && s_hist[threadIdx.x] != 0)
        atomicAdd(counts + threadIdx.x, (unsigned long long)s_hist[threadIdx.x]);
}

// ionise and heat the rows whose first cover is one of the `lit` first bubbles of the batch
__global__ void __launch_bounds__(256) k_heiii_apply(const HeiiiView A, const unsigned *__restrict__ first, unsigned lit, double a3inv, double du)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if(i >= A.n || first[i] >= lit)
        return;
    uint8_t f = A.flag[i];
    double e = A.entropy[i];
    if(heiii_ionize_row(f, e, A.density[i], a3inv, du)) {
        A.flag[i] = f;
        A.entropy[i] = e;
    }
}

// CM and MinID of the candidate groups into compact arrays (the group table itself stays on the device)
__global__ void __launch_bounds__(256) k_heiii_gather(int64_t nc, const int64_t *__restrict__ cand, const double *__restrict__ cm,
                                                      const uint64_t *__restrict__ minid, double *__restrict__ ocm, uint64_t *__restrict__ oid)
{
    const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if(k >= nc)
        return;
    const int64_t g = cand[k];
    for(int j = 0; j < 3; j++)
        ocm[3 * k + j] = cm[3 * g + j];
    oid[k] = minid[g];
}

void HeiiiEngine::gather_groups(const std::vector<int64_t> &cand, const double *d_cm, const uint64_t *d_minid, std::vector<double> &cm,
                                std::vector<uint64_t> &minid, hipStream_t st)
{
    const size_t nc = cand.size();
    cm.resize(3 * nc);
    minid.resize(nc);
    if(nc == 0)
        return;
    g_idx.reserve(nc);
    g_cm.reserve(3 * nc);
    g_minid.reserve(nc);
    MPG_HIP(hipMemcpyAsync(g_idx.p, cand.data(), nc * sizeof(int64_t), hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(k_heiii_gather, dim3(nblk((int64_t)nc)), dim3(256), 0, st, (int64_t)nc, g_idx.p, d_cm, d_minid, g_cm.p, g_minid.p);
    MPG_HIP(hipGetLastError());
    MPG_HIP(hipMemcpyAsync(cm.data(), g_cm.p, 3 * nc * sizeof(double), hipMemcpyDeviceToHost, st));
    MPG_HIP(hipMemcpyAsync(minid.data(), g_minid.p, nc * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
    MPG_HIP(hipStreamSynchronize(st));
}

static unsigned long long read_word(const unsigned long long *d, hipStream_t st)
{
    unsigned long long v = 0;
    MPG_HIP(hipMemcpyAsync(&v, d, sizeof(v), hipMemcpyDeviceToHost, st));
    MPG_HIP(hipStreamSynchronize(st));
    return v;
}

int64_t HeiiiEngine::count_ionized(const HeiiiView &A, hipStream_t st)
{
    counts.reserve(HEIII_MAXB + 2);
    MPG_HIP(hipMemsetAsync(counts.p + HEIII_MAXB, 0, sizeof(unsigned long long), st));
    if(A.n > 0 && A.type)
        hipLaunchKernelGGL(k_heiii_count, dim3(nblk(A.n)), dim3(256), 0, st, A, counts.p + HEIII_MAXB);
    MPG_HIP(hipGetLastError());
    return (int64_t)read_word(counts.p + HEIII_MAXB, st);
}

namespace {
struct Choice {
    int64_t position, group, slot;
    double radius;
};
double table_value(const std::vector<double> &t, uint64_t seed) { return t[seed % (uint64_t)t.size()]; } // get_random_number, system.c:55-61
} // namespace

void heiii_candidates(const mpg_heiii_params &par, const double *mass, int64_t ngroups, std::vector<int64_t> &cand)
{
    for(int64_t g = 0; g < ngroups; g++) {
        if(mass[g] < par.qso_candidate_min_mass)
            continue;
        if(mass[g] > par.qso_candidate_max_mass)
            continue;
        cand.push_back(g);
    }
}

void HeiiiEngine::run(const HeiiiView &A, double box, const mpg_heiii_step &S, const HeiiiGroups &groups, hipStream_t st)
{
    records.clear();
    last = mpg_heiii_result{};
    last_ms[0] = last_ms[1] = last_ms[2] = 0;
    const int B = batch > 0 ? batch : default_batch;
    const double n_gas_tot = (double)S.n_gas_tot, desired = S.desired_ion_frac;
    const double a3inv = 1 / pow(S.atime, 3);                                                  // :534
    const double nheperg = (1 - cool::HYDROGEN_MASSFRAC) / (cool::PROTONMASS * HEIII_HEMASS);   // :398
    const double du = S.qso_inst_heating * nheperg / S.uu_in_cgs;                               // :400, :406
    for(hipEvent_t &e : ev)
        if(!e)
            MPG_HIP(hipEventCreate(&e));
    counts.reserve(HEIII_MAXB + 2);
    first.reserve((size_t)A.n + 1);

    last.n_ionized_before = count_ionized(A, st);
    if(desired > par.heIIIreion_finish_frac) { // :539
        MPG_HIP(hipMemsetAsync(counts.p + HEIII_MAXB, 0, sizeof(unsigned long long), st));
        if(A.n > 0 && A.type)
            hipLaunchKernelGGL(k_heiii_flash, dim3(nblk(A.n)), dim3(256), 0, st, A, a3inv, du, counts.p + HEIII_MAXB);
        MPG_HIP(hipGetLastError());
        last.flash_ionized = (int64_t)read_word(counts.p + HEIII_MAXB, st);
    }
    // :555-556 (the flash ionises exactly the rows of type 0 without the flag: the count after it is the sum)
    double curionfrac = (double)(last.n_ionized_before + last.flash_ionized) / n_gas_tot;
    last.initionfrac = last.curionfrac = curionfrac;
    last.stop_reason = MPG_HEIII_NOTHING_TO_DO;
    if(!(curionfrac < desired)) // :559, :568
        return;

    // build_qso_candidate_list, :290-311: the groups inside the mass window in the order of fof.Group, with their CM and MinID
    std::vector<int64_t> cand;
    std::vector<double> cm;
    std::vector<uint64_t> minid;
    groups(par, cand, cm, minid);
    std::vector<int64_t> slot(cand.size()); // the list as the loop shortens it: rows of cand / cm / minid
    for(size_t k = 0; k < slot.size(); k++)
        slot[k] = (int64_t)k;
    last.stop_reason = MPG_HEIII_NO_CANDIDATES;
    if(cand.empty())
        return;

    // the choices of the whole loop (choose_QSO_halo :348-363 with ncand_before = 0, the removal of :624-627) and the radii (:280-286);
    // the sequence ends where ncand_tot reaches 0: that choice is consumed and never lit (:581-585)
    std::vector<Choice> seq;
    {
        int64_t ncand = (int64_t)cand.size(), ncand_tot = ncand;
        for(int64_t it = 0;; it++) {
            const double drand = table_value(rnd, (uint64_t)(S.TotNgroups + it));
            const int64_t qso = (int64_t)(drand * ncand_tot);
            ncand_tot--;
            const int64_t new_qso = (qso < 0 || qso >= ncand) ? -1 : qso;
            if(ncand_tot <= 0)
                break;
            Choice c{new_qso, -1, -1, 0.0};
            if(new_qso > 0) { // :505
                c.slot = slot[new_qso];
                c.group = cand[c.slot];
                const uint64_t id = minid[c.slot];
                const double u1 = table_value(rnd, id), u2 = table_value(rnd, id + 1);
                MPG_CHECK(u1 != 0, "heiii_reionization: the random table holds exactly 0 at a seed used as u1 (log(0))");
                const double z1 = sqrt(-2 * log(u1)) * cos(2 * M_PI * u2);
                c.radius = par.mean_bubble + sqrt(par.var_bubble) * z1;
                MPG_CHECK(std::isfinite(c.radius) && c.radius > 0, "heiii_reionization: a bubble radius is not positive and finite");
            }
            seq.push_back(c);
            if(new_qso >= 0) {
                slot.erase(slot.begin() + new_qso);
                ncand--;
            }
        }
    }

    int reason = -1;
    const int64_t nseq = (int64_t)seq.size();
    std::vector<unsigned long long> hc((size_t)HEIII_MAXB);
    for(int64_t it0 = 0; it0 < nseq && reason < 0; it0 += B) {
        if(!(curionfrac < desired)) { // (no scan for a loop that is over)
            reason = MPG_HEIII_REACHED;
            break;
        }
        HeiiiBatch bt;
        bt.nb = (int)std::min<int64_t>(B, nseq - it0);
        bt.box = box;
        for(int k = 0; k < bt.nb; k++) {
            const Choice &c = seq[it0 + k];
            for(int j = 0; j < 3; j++)
                bt.b[k][j] = c.group >= 0 ? cm[3 * c.slot + j] : 0.0;
            bt.b[k][3] = c.group >= 0 ? c.radius * c.radius : -1.0;
        }
        MPG_HIP(hipMemsetAsync(counts.p, 0, HEIII_MAXB * sizeof(unsigned long long), st));
        MPG_HIP(hipEventRecord(ev[0], st));
        if(A.n > 0)
            hipLaunchKernelGGL(k_heiii_scan, dim3(nblk(A.n)), dim3(256), 0, st, A, bt, first.p, counts.p);
        MPG_HIP(hipEventRecord(ev[1], st));
        MPG_HIP(hipGetLastError());
        MPG_HIP(hipMemcpyAsync(hc.data(), counts.p, bt.nb * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
        MPG_HIP(hipEventRecord(ev[2], st));
        MPG_HIP(hipStreamSynchronize(st));
        // the loop of :575-628 on the counts
        unsigned lit = 0;
        for(int k = 0; k < bt.nb; k++) {
            const int64_t it = it0 + k;
            if(!(curionfrac < desired)) {
                reason = MPG_HEIII_REACHED;
                break;
            }
            const int64_t count = (int64_t)hc[k];
            curionfrac += (double)count / n_gas_tot; // :591
            last.tot_n_ionized += count;
            records.push_back(HeiiiRecord{seq[it].position, seq[it].group, seq[it].radius, count, curionfrac});
            lit = (unsigned)k + 1;
            if((double)count < 0.01 * (double)S.non_overlapping_bubble_number && it > 10) { // :618
                reason = MPG_HEIII_INSUFFICIENT;
                break;
            }
        }
        MPG_HIP(hipEventRecord(ev[3], st));
        if(A.n > 0 && lit > 0)
            hipLaunchKernelGGL(k_heiii_apply, dim3(nblk(A.n)), dim3(256), 0, st, A, first.p, lit, a3inv, du);
        MPG_HIP(hipEventRecord(ev[4], st));
        MPG_HIP(hipGetLastError());
        MPG_HIP(hipEventSynchronize(ev[4]));
        for(int k = 0; k < 3; k++) { // scan (0, 1), copy (1, 2), apply (3, 4): the host's replay between 2 and 3 is in none
            float ms = 0;
            MPG_HIP(hipEventElapsedTime(&ms, ev[k == 2 ? 3 : k], ev[k == 2 ? 4 : k + 1]));
            last_ms[k] += ms;
        }
    }
    if(reason < 0) // the choice that empties the list is consumed, not lit (:581-585), unless the loop has ended before it (:575)
        reason = curionfrac < desired ? MPG_HEIII_EXHAUSTED : MPG_HEIII_REACHED;
    last.stop_reason = reason;
    last.iterations = (int64_t)records.size();
    last.curionfrac = curionfrac;
}

} // namespace mpg
