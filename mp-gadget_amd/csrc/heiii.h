// heiii.h -- helium reionisation by quasar bubbles (do_heiii_reionization, cooling_qso_lightup.c; see heiii.hip)
#pragma once
#include "../../include/mpgadget_hip.h"
#include "cooling_rates.h"
#include "mpg_common.h"
#include <functional>
#include <vector>

namespace mpg {

constexpr int HEIII_MAXB = 64;             // bubbles of a batch: they travel as a kernel argument (2 KB)
constexpr unsigned HEIII_NONE = 0xffffffffu; // first-cover word of a row that no bubble of the batch covers, or that takes no part
constexpr double HEIII_HEMASS = 4.002602;  // cooling_qso_lightup.c:46

// the next bubbles of the loop in iteration order: centre and radius squared; h2 < 0 for an inert iteration (new_qso <= 0)
struct HeiiiBatch {
    int nb;
    double box;
    double b[HEIII_MAXB][4];
};

// NEAREST, partmanager.h:99
MPG_HD double heiii_nearest(double x, double box) { return x > 0.5 * box ? x - box : (x < -0.5 * box ? x + box : x); }

// the pair test of treewalk.c:982-991 (centre minus particle, r2 <= h2; the early exit of :989 leaves the decision unchanged)
MPG_HD bool heiii_covers(double px, double py, double pz, const double *b, double box)
{
    const double dx = heiii_nearest(b[0] - px, box), dy = heiii_nearest(b[1] - py, box), dz = heiii_nearest(b[2] - pz, box);
    double r2 = dx * dx;
    r2 += dy * dy;
    r2 += dz * dz;
    return r2 <= b[3];
}

// ionize_single_particle, :388-408: the flag and the heat.  du = qso_inst_heating * nheperg / uu_in_cgs (the same for every row; the
// reference divides in this order).  Returns 1 if the row was ionised now.
MPG_HD int heiii_ionize_row(uint8_t &flag, double &entropy, double density, double a3inv, double du)
{
    if(flag)
        return 0;
    flag = 1;
    const double entropytou = pow(density * a3inv, cool::GAMMA_MINUS1) / cool::GAMMA_MINUS1;
    entropy += du / entropytou;
    return 1;
}

// device view of the call's columns (caller order, n entries)
struct HeiiiView {
    const double *pos;   // [n][3]
    const uint8_t *type; // current types; garbage rows carry 7.  null: every row is of type 1 (no gas)
    int64_t n;
    const double *density;
    double *entropy;
    uint8_t *flag; // P.HeIIIionized
};

// one iteration of the loop of turn_on_quasars, as mpg_heiii_export hands it out
struct HeiiiRecord {
    int64_t position; // new_qso: the position in the candidate list as it was at that iteration (-1: none on this rank)
    int64_t group;    // index into fof.Group, -1 when position <= 0 (nothing lit)
    double radius;    // 0 when position <= 0
    int64_t count;    // rows newly ionised
    double curionfrac;
};

// fills the candidate list: the indices into fof.Group, and per candidate CM[3] and MinID
using HeiiiGroups = std::function<void(const mpg_heiii_params &, std::vector<int64_t> &, std::vector<double> &, std::vector<uint64_t> &)>;
// build_qso_candidate_list (:296-306) on a host mass column
void heiii_candidates(const mpg_heiii_params &par, const double *mass, int64_t ngroups, std::vector<int64_t> &cand);

struct HeiiiEngine {
    mpg_heiii_params par{};
    bool have_par = false;
    std::vector<double> rnd; // the host's copy of the random table (mpg_set_random_table)
    int batch = 0;           // mpg_heiii_set_batch; 0: the default
    DevBuf<unsigned> first;  // per row: the first bubble of the batch that covers it
    DevBuf<unsigned long long> counts; // per bubble of the batch; [HEIII_MAXB]: the rows of type 0 with the flag set
    DevBuf<int64_t> g_idx;   // the candidates' group indices, their CM and MinID (gather_groups)
    DevBuf<double> g_cm;
    DevBuf<uint64_t> g_minid;
    std::vector<HeiiiRecord> records;
    mpg_heiii_result last{};
    hipEvent_t ev[5] = {}; // per batch: around the scan, behind the copy of the counts, around the apply pass
    double last_ms[3] = {0, 0, 0}; // summed over the batches of the last call: scan kernels, count copies, apply passes
    ~HeiiiEngine()
    {
        for(hipEvent_t e : ev)
            if(e)
                (void)hipEventDestroy(e);
    }
    static constexpr int default_batch = HEIII_MAXB;
    // gas_ionization_fraction, :367-382: the rows of type 0 with the flag
    int64_t count_ionized(const HeiiiView &A, hipStream_t st);
    // CM and MinID of the listed groups from the device group table
    void gather_groups(const std::vector<int64_t> &cand, const double *d_cm, const uint64_t *d_minid, std::vector<double> &cm,
                       std::vector<uint64_t> &minid, hipStream_t st);
    // the whole of turn_on_quasars on device columns; `groups` is asked for the candidates only when the loop is entered
    void run(const HeiiiView &A, double box, const mpg_heiii_step &S, const HeiiiGroups &groups, hipStream_t st);
};

} // namespace mpg
