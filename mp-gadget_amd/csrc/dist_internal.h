// dist_internal.h -- the object behind the mpg_dist handle and the helpers that more than one file of the multi-rank layer uses.  The layer
// is split by subject: dist.hip (the object, the communicator wrappers, plans and row exchange), dist_gravity.hip (slab PM, ghost import,
// local tree, walks, planes), dist_sph.hip, dist_domain.hip, dist_fof.hip and dist_host.hip (the host-pointer forms).  No kernel and no
// __device__ function lives here: every kernel stands in the file of the code that launches it, so no kernel is compiled twice.
#pragma once
#include "engine_internal.h"

struct Plan { // one personalised exchange: who gets which of my rows, and what I get
    DevBuf<int> idx;
    DevBuf<long long> d_sdsp;
    HostBuf<long long> h_sdsp;
    std::vector<int64_t> scnt, rcnt, sdsp, rdsp; // rows
    int64_t nsend = 0, nrecv = 0;
};

struct mpg_dist {
    mpg_engine *eng = nullptr;
    mpg_comm comm{};
    int me = 0, nt = 1;
    // the communicator runs device-buffer collectives as work on the engine's stream (mpg_comm.bind_stream: RCCL): no host
    // synchronisation before or after them
    bool stream_ordered = false;
    hipStream_t bound_stream = nullptr;
    // domain
    double box = 0, margin = 0;
    int La = 0;
    bool have_domain = false;
    DevBuf<unsigned long long> need; // [8^La] ranks that need the cell
    // work
    DevBuf<unsigned long long> mask, cnt;
    DevBuf<unsigned> tilecnt, tilepos; // build_plan: rows per (destination, tile of 1024 rows) and their exclusive scan
    DevBuf<char> tmp;
    DevBuf<char> sendbuf, recvbuf;
    HostBuf<char> hsend, hrecv;
    Plan pm, ghost;
    // PM side
    DevBuf<double> spos, sgrav, spot;
    DevBuf<float> smass;
    DevBuf<unsigned long long> scount;
    DevBuf<double> sendA, recvA, sendB, recvB, gsend, grecv;
    int64_t per_peer = 0, plane = 0;
    bool slab_ready = false;
    // tree side
    hipStream_t tree_stream = nullptr; // the local tree build beside the PM step (mpg_dist_gravity_step)
    DevBuf<double> lpos, top;
    DevBuf<float> lmass;
    DevBuf<int> targets, act_targets;
    DevBuf<uint8_t> actflag;
    DevBuf<unsigned> err;
    HostBuf<double> htop;
    int64_t ntarg = 0, n_own_tree = -1;
    // garbage / swallowed particles among the own rows (mpg_dist_dev_set_garbage): flags over n_skip_rows rows, n_skip of them set
    const unsigned char *d_skip = nullptr;
    DevBuf<unsigned char> skip_own; // (the library's copy of the caller's flags)
    int64_t n_skip = 0, n_skip_rows = -1;
    DevBuf<uint8_t> ltype, o_skip;
    const unsigned char *skip_for(int64_t n) const { return (n_skip > 0 && n == n_skip_rows) ? d_skip : nullptr; }
    // the types of the own rows for the hybrid-neutrino deposit mask (mpg_dist_dev_set_types): a copy, over n_type_rows rows
    DevBuf<uint8_t> type_own;
    int64_t n_type_rows = -1;
    const uint8_t *types_for(int64_t n) const { return n == n_type_rows ? type_own.p : nullptr; }
    HostBuf<unsigned long long> chk; // [0] own particles found in the local tree, [1] the two flags of the global top (pinned: read back without a wait)
    bool chk_pending = false;
    bool grav_tree_valid = false; // the engine's tree is the gravity tree of mpg_dist_dev_force_tree_build (the SPH loops and FOF replace it)
    double last_hmax = 0;         // largest smoothing length over all ranks after the last density loop
    int blackholes = 0;           // BlackHoleOn of density(): the own non-swallowed black holes are targets of the density loop too
    int64_t dom_max_part = 0;     // PartManager->MaxPart of domain_check_memory_bound (0: no bound)
    DevBuf<float> cost;
    // SPH loops on the local set: inputs and outputs over [own | ghosts]
    DevBuf<uint8_t> s_type, s_tbh, s_tbg;
    DevBuf<double> s_in[7];   // hsml, vel, entropy, gacc, gpm, hydroacc_in, dtentropy_in
    DevBuf<double> s_out[11]; // dthsml, density, egywtdensity, dhsmlegyfac, divvel, curlvel, gradrho, hydroacc_out, dtentropy_out, maxsignalvel
    DevBuf<int> gas;
    int64_t ngas = 0, sph_nl = -1, sph_n_own = -1;
    // domain decomposition (mpg_dist_domain_decompose): the global tree, its leaves, where every particle goes
    std::vector<mpg_topnode> dom_tree;
    std::vector<int> dom_leaf_task, dom_leaf_topnode, dom_start, dom_end;
    std::vector<int64_t> dom_leaf_count, dom_send_counts;
    int dom_size = 0, dom_nleaves = 0, dom_policy = 0;
    double dom_alloc_factor = 0.5;
    DevBuf<int> dom_topleaf, dom_task;
    DevBuf<double> dom_cost;
    int64_t dom_n = -1;
    Plan dom_plan;
    DevBuf<char> dom_out[16];
    // friends-of-friends over ranks
    DevBuf<unsigned long long> f_id, f_ext, f_keys, f_vals, f_keys2, f_vals2, f_ukeys, f_uvals, f_glab, f_minid;
    DevBuf<uint8_t> f_type, f_flag;
    DevBuf<long long> f_grnr_tab, f_pgrnr;
    struct GroupRec { // one (part of a) group: struct BaseGroup / Group (fof.h:14-49) with raw sums about FirstPos
        unsigned long long MinID;
        long long Length;
        int LenType[6];
        float FirstPos[3];
        int src;
        double acc[27]; // Mass, MassType[6], sum m x[3], sum m v[3], sum m (rel x v)[3], sum m rel rel^T [9]
    };
    std::vector<GroupRec> f_groups; // the complete groups this rank holds (MinID % NTask == ThisTask), finished
    std::vector<long long> f_group_grnr;
    int64_t f_total = 0;
    int64_t stats[8] = {};
    double times[8] = {};
    // host (drop-in) path: the rank's P[] staged on the device
    DevBuf<double> o_pos, o_gravpm, o_pot, o_acc, o_prev;
    DevBuf<float> o_mass;
    std::vector<double> hbuf;
    std::vector<float> hbuf_f;
    std::vector<uint8_t> hbuf_b;
    int64_t o_n = -1;
    DevBuf<int> o_act;        // ActiveParticle of the host drop-in walk
    DevBuf<double> o_sph[17]; // the double-valued fields of mpg_sph_arrays over the own particles (host SPH path)
    DevBuf<uint8_t> o_u8[3];  // type, tb_hydro, tb_grav
};

// ---- dist.hip
double now_ms();
void sync(mpg_dist *d);
void cb(int rc, const char *what);
// before a callback that takes device buffers: a stream-ordered communicator follows the engine's stream, a blocking one finds it idle
void comm_ready(mpg_dist *d);
void a2av(mpg_dist *d, const void *dsend, const std::vector<int64_t> &sb, const std::vector<int64_t> &sd, void *drecv,
          const std::vector<int64_t> &rb, const std::vector<int64_t> &rd, int64_t stot, int64_t rtot);
void a2a_uniform(mpg_dist *d, const void *dsend, void *drecv, int64_t bytes_per_peer);
void allreduce_i64(mpg_dist *d, int64_t *v, int64_t n, int op);
void allreduce_host_f64(mpg_dist *d, double *h, int64_t n, int op);
bool any_rank(mpg_dist *d, bool f);
void allgather_host(mpg_dist *d, const void *buf, int64_t nbytes, std::vector<std::vector<char>> &out);
void build_plan(mpg_dist *d, Plan &pl, int64_t n, const unsigned long long *mask);
void exchange_rows(mpg_dist *d, const Plan &pl, const void *dsend, void *drecv, bool reverse, int64_t rb_);
// Rows of `rb` bytes along a plan through d->sendbuf / d->recvbuf: pack(rows to fill) is called when this rank sends any, then the
// exchange; returns the rows received.  reverse: the answers travel back, out of d->recvbuf into d->sendbuf.
template <class Pack> const char *ship_rows(mpg_dist *d, const Plan &pl, int64_t rb, bool reverse, Pack pack)
{
    d->sendbuf.reserve((size_t)rb * pl.nsend + rb);
    d->recvbuf.reserve((size_t)rb * pl.nrecv + rb);
    char *out = reverse ? d->recvbuf.p : d->sendbuf.p, *in = reverse ? d->sendbuf.p : d->recvbuf.p;
    if((reverse ? pl.nrecv : pl.nsend) > 0)
        pack(out);
    exchange_rows(d, pl, out, in, reverse, rb);
    return in;
}
// ... and unpack(rows received) behind it when any arrived
template <class Pack, class Unpack> void ship_rows(mpg_dist *d, const Plan &pl, int64_t rb, bool reverse, Pack pack, Unpack unpack)
{
    const char *in = ship_rows(d, pl, rb, reverse, pack);
    if((reverse ? pl.nsend : pl.nrecv) > 0)
        unpack(in);
}
// rocPRIM's two calls: call(nullptr, bytes) asks for the size of the temporary storage, call(d->tmp, bytes) runs
template <class Call> void with_tmp(mpg_dist *d, Call call)
{
    size_t tb = 0;
    MPG_HIP(call(nullptr, tb));
    d->tmp.reserve(tb + 16);
    MPG_HIP(call((void *)d->tmp.p, tb));
}
// d->actflag[list[i]] = 1 for the m listed rows of n, queued on the engine's stream; an index outside [0, n) raises d->err[0], which the
// caller reads back at its next wait
void flag_active_list(mpg_dist *d, const int *d_list, int64_t m, int64_t n);

// ---- dist_gravity.hip
int64_t import_ghosts(mpg_dist *d, int64_t n, const double *pos, const float *mass);
void tree_build_local(mpg_dist *d, int64_t n_own, int64_t nl, hipStream_t st);
void tree_checks(mpg_dist *d);
void tree_finish(mpg_dist *d, int64_t n_own, int64_t nl);
