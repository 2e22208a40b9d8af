// host_forms.hip -- the host-pointer ("drop-in") entry points: the caller's particle table (mpg_particle_view) and host arrays are
// packed, uploaded, run through the mpg_dev_* calls of engine.hip, physics.hip and integrator.hip and the results written back, on top of host_table.h.  The calls on a
// device-resident table are resident.hip's.
#include "engine_internal.h"
#include <atomic>
#include <chrono>
#include <cstdio>

// MPG_HOST_TIMING=1: wall-clock marks of the host forms' phases on stderr (a diagnostic)
struct HostClock {
    bool on;
    const char *name;
    double t0;
    std::string line;
    static double now() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
    explicit HostClock(const char *n) : on(getenv("MPG_HOST_TIMING") != nullptr), name(n), t0(now()) {}
    void mark(const char *what)
    {
        if(!on)
            return;
        const double t = now();
        char buf[96];
        snprintf(buf, sizeof(buf), " %s %.2f", what, t - t0);
        line += buf;
        t0 = t;
    }
    ~HostClock()
    {
        if(on)
            fprintf(stderr, "HOST_TIMING %s:%s\n", name, line.c_str());
    }
};

// the stream of the overlapped transfers and the event that orders it behind the engine's stream
static void ensure_copy_stream(mpg_engine *eng)
{
    if(eng->copy_stream)
        return;
    MPG_HIP(hipStreamCreateWithFlags(&eng->copy_stream, hipStreamNonBlocking));
    MPG_HIP(hipEventCreateWithFlags(&eng->ev_pm_done, hipEventDisableTiming));
}

static void stage_particles_body(mpg_engine *eng, const mpg_particle_view *P, double BoxSize, bool on_prefetch_thread);
void stage_particles(mpg_engine *eng, const mpg_particle_view *P, double BoxSize)
{
    eng->prefetch_join(); // (a prefetch of this epoch ends here; the write-back thread of gravpm_force is waited for only if P[] is read again)
    if(!eng->prefetch_error.empty()) {
        const std::string e = eng->prefetch_error;
        eng->prefetch_error.clear();
        MPG_CHECK(false, "host path: the prefetch of the particle table failed: " + e);
    }
    stage_particles_body(eng, P, BoxSize, false);
}
static void stage_particles_body(mpg_engine *eng, const mpg_particle_view *P, double BoxSize, bool on_prefetch_thread)
{
    MPG_CHECK(P && (P->n == 0 || P->base), "null particle view");
    MPG_CHECK(P->off_pos >= 0 && P->off_mass >= 0, "particle view needs Pos and Mass");
    const int64_t n = P->n;
    if(eng->resident && eng->res_base == P->base) { // resident mode: the table is the device's
        MPG_CHECK(eng->res_n == n && eng->box == BoxSize && eng->d_pos == eng->s_pos.p,
                  "resident mode: the particle table changed size, box or binding (mpg_resident_end / _begin around anything that reorders P[])");
        return;
    }
    // positions, masses and types of this very table are on the device already (mpg_set_particle_epoch)
    if(eng->host_epoch != 0 && eng->staged_epoch == eng->host_epoch && eng->staged_base == P->base && eng->staged_n == n &&
       eng->staged_box == BoxSize && eng->d_pos == eng->s_pos.p)
        return;
    if(!on_prefetch_thread) // (mpg_host_prefetch joined before it started this thread)
        eng->host_join();   // a pending write-back of the last epoch's GravPM touches the records this pass reads
    eng->h_d.reserve(3 * (size_t)n + 1);
    eng->h_f.reserve((size_t)n + 1);
    eng->h_b.reserve((size_t)n + 1);
    eng->s_pos.reserve(3 * (size_t)n + 1);
    eng->s_mass.reserve((size_t)n + 1);
    eng->s_type.reserve((size_t)n + 1);
    double *hd = eng->h_d.p;
    float *hf = eng->h_f.p;
    uint8_t *hb = eng->h_b.p;
    const HostTable T(*P);
    const mpg_particle_view &V = T.V;
    // with overlap, the same pass also takes what the epoch's later calls would read from P[] again: Potential (gravpm_force accumulates
    // into it) and FullTreeGravAccel (the walk's opening criterion)
    const bool extras = eng->host_overlap && eng->host_epoch != 0 && V.off_accel >= 0;
    const bool xpot = extras && V.off_potential >= 0;
    double *hacc = nullptr, *hpot = nullptr;
    if(extras) {
        eng->h_acc.reserve(3 * (size_t)n + 1);
        eng->s_prevacc.reserve(3 * (size_t)n + 1);
        hacc = eng->h_acc.p;
        if(xpot) {
            eng->h_gpot.reserve((size_t)n + 1);
            eng->s_pot.reserve((size_t)n + 1);
            hpot = eng->h_gpot.p;
        }
    }
    std::atomic<int> any_dead{0};
    std::atomic<int> *dead_seen = &any_dead;
    for_each_chunk(n, [=](int64_t lo, int64_t hi) {
        parallel_for(hi - lo, [=](int64_t a0, int64_t a1) {
            for(int64_t i = lo + a0; i < lo + a1; i++) {
                const double *pp = T.pos(i);
                hd[3 * i + 0] = pp[0];
                hd[3 * i + 1] = pp[1];
                hd[3 * i + 2] = pp[2];
                hf[i] = T.mass(i);
                // garbage / swallowed-BH particles never enter the tree (forcetree.c:806): give them type 7 (no mask bit)
                uint8_t ty = T.type(i);
                if(not_in_tree(T.flags(i), ty))
                    ty = 7;
                hb[i] = ty;
                if(ty == 7)
                    dead_seen->store(1, std::memory_order_relaxed);
                if(hacc) {
                    const double *aa = T.vec(i, V.off_accel);
                    hacc[3 * i + 0] = aa[0];
                    hacc[3 * i + 1] = aa[1];
                    hacc[3 * i + 2] = aa[2];
                    if(hpot)
                        hpot[i] = T.scalar(i, V.off_potential);
                }
            }
        });
        MPG_HIP(hipMemcpyAsync(eng->s_pos.p + 3 * lo, hd + 3 * lo, 3 * (hi - lo) * sizeof(double), hipMemcpyHostToDevice, eng->stream));
        MPG_HIP(hipMemcpyAsync(eng->s_mass.p + lo, hf + lo, (hi - lo) * sizeof(float), hipMemcpyHostToDevice, eng->stream));
        MPG_HIP(hipMemcpyAsync(eng->s_type.p + lo, hb + lo, (hi - lo) * sizeof(uint8_t), hipMemcpyHostToDevice, eng->stream));
        if(hpot)
            MPG_HIP(hipMemcpyAsync(eng->s_pot.p + lo, hpot + lo, (hi - lo) * sizeof(double), hipMemcpyHostToDevice, eng->stream));
    });
    eng->staged_extra_epoch = extras ? eng->host_epoch : -1;
    eng->gravpm_epoch = -1;
    // garbage and swallowed particles are not deposited and receive no mesh force either (gravpm.c:176-179: region -2): the PM takes a
    // live flag per particle when the table holds any
    const bool dead = any_dead.load() != 0;
    eng->pm_live = nullptr;
    if(dead) {
        eng->s_live.reserve((size_t)n + 1);
        MPG_HIP(hipStreamSynchronize(eng->stream)); // (the type bytes have left the staging buffer, which now takes the flags)
        parallel_for(n, [=](int64_t lo, int64_t hi) {
            for(int64_t i = lo; i < hi; i++)
                hb[i] = hb[i] != 7;
        });
        MPG_HIP(hipMemcpyAsync(eng->s_live.p, hb, (size_t)n, hipMemcpyHostToDevice, eng->stream));
        eng->pm_live = eng->s_live.p;
    }
    MPG_HIP(hipStreamSynchronize(eng->stream));
    if(hacc) { // (needed by the walk only: on the copy stream it travels while the PM step computes; its staging buffer is its own)
        ensure_copy_stream(eng);
        if(!eng->ev_acc_up)
            MPG_HIP(hipEventCreateWithFlags(&eng->ev_acc_up, hipEventDisableTiming));
        MPG_HIP(hipMemcpyAsync(eng->s_prevacc.p, hacc, 3 * (size_t)n * sizeof(double), hipMemcpyHostToDevice, eng->copy_stream));
        MPG_HIP(hipEventRecord(eng->ev_acc_up, eng->copy_stream));
    }
    eng->n = n;
    eng->fof.cat_n = -1; // (a group catalogue belongs to the particles it was made of)
    eng->d_pos = eng->s_pos.p;
    eng->d_mass = eng->s_mass.p;
    eng->d_type = eng->s_type.p;
    eng->box = BoxSize;
    eng->staged_epoch = eng->host_epoch;
    eng->staged_base = P->base;
    eng->staged_n = n;
    eng->staged_box = BoxSize;
}

int mpg_set_particle_epoch(mpg_engine *eng, int64_t epoch)
{
    API_BEGIN
    MPG_CHECK(eng, "null engine");
    if(epoch != eng->host_epoch)
        eng->host_join(); // (a prefetch reads host_epoch on its own thread)
    eng->host_epoch = epoch;
    API_END
}

// The epoch's one packing pass and its uploads, started EARLY: a caller that knows P[] is final for the step - the end of
// drift_all_particles (drift.c:84-102), where nothing of run.c touches Pos / Mass / FullTreeGravAccel / Potential again before gravpm_force
// (run.c:420-522: domain_maintain reads them; an exchange or a garbage collection declares a new epoch, and this upload is then simply not used)
// - calls this after mpg_set_particle_epoch; the pass runs on a host thread of its own and the first entry point of the epoch joins it
// instead of packing.  Needs the overlap mode (the pass must also take Potential / FullTreeGravAccel); without it, or resident, a no-op.
int mpg_host_prefetch(mpg_engine *eng, const mpg_particle_view *P, double BoxSize)
{
    API_BEGIN
    MPG_CHECK(eng && P && BoxSize > 0, "mpg_host_prefetch: bad argument");
    MPG_HIP(hipSetDevice(eng->device));
    eng->host_join();
    if(eng->host_overlap && eng->host_epoch != 0 && !eng->resident && P->n != 0) {
        eng->prefetch_error.clear();
        eng->prefetch_view = *P;
        eng->prefetch_thread = std::thread([eng, BoxSize] {
            try {
                MPG_HIP(hipSetDevice(eng->device));
                stage_particles_body(eng, &eng->prefetch_view, BoxSize, true);
            }
            catch(const std::exception &e) {
                eng->prefetch_error = e.what();
            }
        });
    }
    API_END
}

int mpg_set_host_overlap(mpg_engine *eng, int on)
{
    API_BEGIN
    MPG_CHECK(eng, "null engine");
    eng->host_join();
    eng->host_overlap = on != 0;
    eng->host_slices = on > 1 ? on : 0; // (2 .. 8: that many slices of the walk whatever the size - the tests' way to the sliced path)
    API_END
}

int mpg_host_results_sync(mpg_engine *eng)
{
    API_BEGIN
    MPG_CHECK(eng, "null engine");
    eng->host_join();
    MPG_CHECK(eng->unpack_error.empty(), "host path: the write-back of GravPM failed: " + eng->unpack_error);
    API_END
}

// GravPM - and, p given, Potential - of the records [lo, hi) from the downloaded arrays
static void put_gravpm(const HostTable &T, int64_t lo, int64_t hi, const double *g, const double *p)
{
    for(int64_t i = lo; i < hi; i++) {
        double *d = T.vec_mut(i, T.V.off_gravpm);
        d[0] = g[3 * i + 0];
        d[1] = g[3 * i + 1];
        d[2] = g[3 * i + 2];
        if(p)
            T.scalar_mut(i, T.V.off_potential) = p[i];
    }
}

// mpg_gravpm_force on the resident table: the results stay in HBM, GravPM assigned, Potential accumulated (gravpm.c:499-501)
static void gravpm_force_resident(mpg_engine *eng, int64_t n)
{
    if(eng->pm_live) // (gravpm.c:88-92 zeroes GravPM of every particle; the readout reaches the live ones)
        MPG_HIP(hipMemsetAsync(eng->r_gravpm.p, 0, 3 * (size_t)n * sizeof(double), eng->stream));
    eng->pm.force(n, eng->d_pos, eng->pm.tracer_mass(n, eng->d_mass, eng->d_type, eng->stream), eng->pm_live, eng->r_gravpm.p, eng->r_pot.p,
                  eng->stream, &eng->timer);
}

// ... with overlap: the results leave on a copy stream behind the PM step and are written into P[] by a host thread, chunk by chunk, while
// the caller's thread returns and queues the tree build and the walk (the walk reads GravPM and the Potential it accumulates onto from the
// device buffers, which nothing overwrites before the next gravpm_force)
static void gravpm_results_overlapped(mpg_engine *eng, const HostTable &T, bool wantpot)
{
    const int64_t n = T.V.n;
    ensure_copy_stream(eng);
    eng->h_gpm.reserve(3 * (size_t)n + 1);
    double *ag = eng->h_gpm.p, *ap = nullptr;
    if(wantpot) {
        eng->h_gpot.reserve((size_t)n + 1);
        ap = eng->h_gpot.p;
    }
    const double *dg = eng->s_gravpm.p, *dp = eng->s_pot.p;
    hipStream_t cs = eng->copy_stream;
    MPG_HIP(hipEventRecord(eng->ev_pm_done, eng->stream));
    MPG_HIP(hipStreamWaitEvent(cs, eng->ev_pm_done, 0));
    for_each_chunk(
        n,
        [=](int64_t lo, int64_t hi) {
            MPG_HIP(hipMemcpyAsync(ag + 3 * lo, dg + 3 * lo, 3 * (hi - lo) * sizeof(double), hipMemcpyDeviceToHost, cs));
            if(wantpot)
                MPG_HIP(hipMemcpyAsync(ap + lo, dp + lo, (hi - lo) * sizeof(double), hipMemcpyDeviceToHost, cs));
        },
        eng->gchunk_ev, cs);
    eng->unpack_error.clear();
    const int device = eng->device;
    eng->unpack_thread = std::thread([=] {
        if(hipSetDevice(device) != hipSuccess) {
            eng->unpack_error = "hipSetDevice";
            return;
        }
        for(int c = 0; c < HOST_CHUNKS; c++) {
            int64_t lo, hi;
            chunk_range(n, c, lo, hi);
            if(hipEventSynchronize(eng->gchunk_ev[c]) != hipSuccess) {
                eng->unpack_error = "hipEventSynchronize";
                return;
            }
            if(hi > lo)
                parallel_for(hi - lo, [=](int64_t a0, int64_t a1) { put_gravpm(T, lo + a0, lo + a1, ag, ap); });
        }
    });
}

// ... synchronously: down and into P[] chunk by chunk before the call returns
static void gravpm_results_sync(mpg_engine *eng, const HostTable &T, bool wantpot)
{
    double *hg = eng->h_d2.p, *hp = eng->h_d3.p;
    const double *dg = eng->s_gravpm.p, *dp = eng->s_pot.p;
    hipStream_t st = eng->stream;
    download_chunks(
        eng->chunk_ev, st, T.V.n,
        [=](int64_t lo, int64_t hi) {
            MPG_HIP(hipMemcpyAsync(hg + 3 * lo, dg + 3 * lo, 3 * (hi - lo) * sizeof(double), hipMemcpyDeviceToHost, st));
            if(wantpot)
                MPG_HIP(hipMemcpyAsync(hp + lo, dp + lo, (hi - lo) * sizeof(double), hipMemcpyDeviceToHost, st));
        },
        [=](int64_t lo, int64_t hi) { put_gravpm(T, lo, hi, hg, wantpot ? hp : nullptr); });
}

// mpg_gravpm_force on a host table: Potential up (unless the epoch's packing pass took it), the PM step, the results down in one of the two ways
static void gravpm_force_host(mpg_engine *eng, const mpg_particle_view *P, HostClock &hc)
{
    const int64_t n = P->n;
    eng->s_gravpm.reserve(3 * (size_t)n + 1);
    const bool wantpot = P->off_potential >= 0;
    const HostTable T(*P);
    eng->h_d2.reserve(3 * (size_t)n + 1);
    eng->h_d3.reserve((size_t)n + 1);
    const bool overlap = eng->host_overlap && eng->host_epoch != 0;
    if(wantpot && !(overlap && eng->staged_extra_epoch == eng->host_epoch)) { // (with overlap the Potential went up with the positions)
        // readout_potential accumulates into P.Potential (gravpm.c:499-501), which is NOT zeroed first
        eng->s_pot.reserve((size_t)n + 1);
        double *hp = eng->h_d3.p;
        parallel_for(n, [=](int64_t lo, int64_t hi) {
            for(int64_t i = lo; i < hi; i++)
                hp[i] = T.scalar(i, T.V.off_potential);
        });
        MPG_HIP(hipMemcpyAsync(eng->s_pot.p, hp, n * sizeof(double), hipMemcpyHostToDevice, eng->stream));
    }
    if(eng->pm_live)
        MPG_HIP(hipMemsetAsync(eng->s_gravpm.p, 0, 3 * (size_t)n * sizeof(double), eng->stream));
    eng->pm.force(n, eng->d_pos, eng->pm.tracer_mass(n, eng->d_mass, eng->d_type, eng->stream), eng->pm_live, eng->s_gravpm.p,
                  wantpot ? eng->s_pot.p : nullptr, eng->stream, &eng->timer);
    eng->gravpm_epoch = eng->host_epoch;
    if(overlap) {
        gravpm_results_overlapped(eng, T, wantpot);
        hc.mark("queued");
    }
    else
        gravpm_results_sync(eng, T, wantpot);
}

int mpg_gravpm_force(mpg_engine *eng, const mpg_particle_view *P)
{
    API_BEGIN
    MPG_CHECK(eng && P, "null argument");
    MPG_HIP(hipSetDevice(eng->device));
    MPG_CHECK(eng->pm.nmesh > 0, "gravpm_force called before gravpm_init_periodic");
    MPG_CHECK(P->off_gravpm >= 0, "particle view needs GravPM");
    MPG_CHECK(!eng->pm.hybrid_tracer || P->off_type >= 0, "gravpm_force: the hybrid-neutrino deposit mask needs the particle type in the view");
    HostClock hc("gravpm_force");
    eng->host_join(); // (the write-back of an earlier call)
    MPG_CHECK(eng->unpack_error.empty(), "host path: the write-back of GravPM failed: " + eng->unpack_error);
    stage_particles(eng, P, eng->pm.box);
    hc.mark("stage");
    if(eng->resident && eng->res_base == P->base)
        gravpm_force_resident(eng, P->n);
    else
        gravpm_force_host(eng, P, hc);
    API_END
}

int mpg_force_tree_rebuild_mask(mpg_engine *eng, const mpg_particle_view *P, double BoxSize, int mask)
{
    API_BEGIN
    MPG_CHECK(eng && P, "null argument");
    MPG_HIP(hipSetDevice(eng->device));
    stage_particles(eng, P, BoxSize);
    wait_for_leaf_blocks(eng, eng->stream);
    eng->tree.build(eng->n, eng->d_pos, eng->d_mass, eng->d_type, mask, BoxSize, eng->stream, &eng->timer);
    eng->tree.calc_moments(nullptr, eng->stream, &eng->timer);
    eng->tree_allocated = true;
    eng->tree_mask = mask;
    eng->full_particle_tree = (eng->tree.npart == eng->n) || mask == 63;
    API_END
}

int mpg_force_tree_full(mpg_engine *eng, const mpg_particle_view *P, double BoxSize)
{
    return mpg_force_tree_rebuild_mask(eng, P, BoxSize, 63 /* ALLMASK, forcetree.h:22 */);
}

int mpg_force_tree_free(mpg_engine *eng)
{
    API_BEGIN
    MPG_CHECK(eng, "null engine");
    eng->tree_allocated = false;
    eng->full_particle_tree = false;
    eng->tree.has_moments = false;
    API_END
}

// the results of the targets [lo, hi) of the tree order, compacted in that order for a contiguous copy to the host
extern "C" __global__ void __launch_bounds__(256) k_gather_results(int64_t lo, int64_t hi, const int *__restrict__ order, const double *__restrict__ acc,
                                                        const double *__restrict__ pot, double *__restrict__ acc_t, double *__restrict__ pot_t)
{
    const int64_t j = lo + (int64_t)blockIdx.x * 256 + threadIdx.x;
    if(j >= hi)
        return;
    const int64_t i = order[j];
    acc_t[3 * j + 0] = acc[3 * i + 0];
    acc_t[3 * j + 1] = acc[3 * i + 1];
    acc_t[3 * j + 2] = acc[3 * i + 2];
    if(pot_t)
        pot_t[j] = pot[i];
}

// mpg_grav_short_tree on the resident table: OldAcc from the resident FullTreeGravAccel + GravPM (grav_get_abs_accel, gravshort.h:70-80),
// results into the resident FullTreeGravAccel / Potential in place: a target's old value is read before its new one is written, and no walk
// reads another target's acceleration.  AccelStore (host) receives a copy when given (timestep.c:454-456).
static void walk_resident(mpg_engine *eng, const mpg_particle_view *P, const int *ActiveParticle, int64_t NumActiveParticle, double (*AccelStore)[3],
                          double rho0)
{
    const int64_t n = P->n;
    const int *d_act = upload_active(eng->s_active, ActiveParticle, NumActiveParticle, eng->stream);
    const bool full = eng->full_particle_tree;
    double *out = eng->r_accel.p;
    if(!full) { // (a tree of a subset: results go to AccelStore only, gravshort.h:54-66)
        eng->s_accel.reserve(3 * (size_t)n + 1);
        MPG_HIP(hipMemsetAsync(eng->s_accel.p, 0, 3 * n * sizeof(double), eng->stream));
        out = eng->s_accel.p;
    }
    MPG_CALL(mpg_dev_grav_short_tree(eng, nullptr, eng->r_accel.p, eng->r_gravpm.p, d_act, NumActiveParticle, out, full ? eng->r_pot.p : nullptr, rho0));
    if(!AccelStore)
        return;
    eng->h_d2.reserve(3 * (size_t)n + 1);
    double *ha = eng->h_d2.p;
    MPG_HIP(hipMemcpyAsync(ha, out, 3 * n * sizeof(double), hipMemcpyDeviceToHost, eng->stream));
    MPG_HIP(hipStreamSynchronize(eng->stream));
    const HostTable T(*P);
    parallel_for(ActiveParticle ? NumActiveParticle : n, [=](int64_t lo, int64_t hi) {
        for(int64_t k = lo; k < hi; k++) {
            const int64_t i = ActiveParticle ? ActiveParticle[k] : k;
            store_walk_result(T, i, ha + 3 * i, nullptr, AccelStore, false);
        }
    });
}

// With overlap, all particles active, a tree of all of them: the walk in S SLICES of the tree order, the results of slice k copied down
// (compacted in tree order: one contiguous copy) and written into P[] by a host thread while slice k + 1 is walked.  The slices are cut
// at multiples of 8 targets, i.e. between the waves of the list kernel: every target's lists, and with them its sums, are those of the
// unsliced walk bit for bit.  What stays on the critical path is the last slice's copy and write-back.
static void walk_sliced(mpg_engine *eng, const HostTable &T, bool wantpot, int S, double rho0, HostClock &hc)
{
    const int64_t n = T.V.n, npart = eng->tree.npart;
    const int *d_order = (const int *)eng->tree.idx_b.p; // tree slot -> particle
    eng->h_order.reserve((size_t)npart + 1);
    eng->s_acc_t.reserve(3 * (size_t)npart + 1);
    eng->h_acc_t.reserve(3 * (size_t)npart + 1);
    if(wantpot) {
        eng->s_pot_t.reserve((size_t)npart + 1);
        eng->h_pot_t.reserve((size_t)npart + 1);
        eng->s_pot2.reserve((size_t)n + 1);
    }
    int *h_order = eng->h_order.p;
    double *hat = eng->h_acc_t.p, *hpt = wantpot ? eng->h_pot_t.p : nullptr;
    double *dat = eng->s_acc_t.p, *dpt = wantpot ? eng->s_pot_t.p : nullptr;
    for(int k = 0; k <= S; k++)
        if(!eng->slice_ev[k])
            MPG_HIP(hipEventCreateWithFlags(&eng->slice_ev[k], hipEventDisableTiming));
    // the tree order for the host thread (the tree is complete: force_tree_full waited for it)
    MPG_HIP(hipMemcpyAsync(h_order, d_order, (size_t)npart * sizeof(int), hipMemcpyDeviceToHost, eng->copy_stream));
    // (what nothing hides is the write-back that is still running when the last walk ends.  The writer needs about half as long for a slice's
    // results as the walk of that slice took, so slice k + 1 may be about half of slice k and still cover it: the slices shrink geometrically,
    // MPG_HOST_SLICE_RATIO per step, and the last - the one nothing covers - is the smallest.  1 = equal slices)
    static const double ratio_env = getenv("MPG_HOST_SLICE_RATIO") ? atof(getenv("MPG_HOST_SLICE_RATIO")) : 0.55;
    const double ratio = (ratio_env > 0.05 && ratio_env < 1.0) ? ratio_env : 1.0;
    int64_t cut[9];
    {
        double w = 1.0, tot = 0.0, acc = 0.0;
        for(int k = 0; k < S; k++, w *= ratio)
            tot += w;
        w = 1.0;
        for(int k = 0; k <= S; k++) {
            cut[k] = k == S ? npart : ((int64_t)((double)npart * (acc / tot)) & ~(int64_t)7);
            acc += w;
            w *= ratio;
        }
    }
    std::string therr;
    std::thread writer;
    std::atomic<int> issued{0}; // slices whose copies are queued and whose event is recorded (an event not yet recorded "is complete")
    std::atomic<bool> abandon{false};
    // (an error thrown below while the writer runs: tell it to stop and wait for it - a joinable std::thread must not be destroyed)
    struct JoinOnExit {
        std::thread &t;
        std::atomic<bool> &stop;
        ~JoinOnExit()
        {
            if(t.joinable()) {
                stop = true;
                t.join();
            }
        }
    } join_on_exit{writer, abandon};
    for(int k = 0; k < S; k++) {
        const int64_t lo = cut[k], hi = cut[k + 1];
        if(hi > lo) {
            MPG_CALL(mpg_dev_grav_short_tree(eng, nullptr, eng->s_prevacc.p, eng->s_gravpm.p, d_order + lo, hi - lo, eng->s_accel.p,
                                             wantpot ? eng->s_pot2.p : nullptr, rho0));
            hipLaunchKernelGGL(k_gather_results, dim3((unsigned)((hi - lo + 255) / 256)), dim3(256), 0, eng->stream, lo, hi, d_order, eng->s_accel.p,
                               wantpot ? eng->s_pot2.p : nullptr, dat, dpt);
        }
        MPG_HIP(hipEventRecord(eng->ev_pm_done, eng->stream)); // (re-used as "slice k gathered")
        MPG_HIP(hipStreamWaitEvent(eng->copy_stream, eng->ev_pm_done, 0));
        if(hi > lo) {
            MPG_HIP(hipMemcpyAsync(hat + 3 * lo, dat + 3 * lo, 3 * (size_t)(hi - lo) * sizeof(double), hipMemcpyDeviceToHost, eng->copy_stream));
            if(wantpot)
                MPG_HIP(hipMemcpyAsync(hpt + lo, dpt + lo, (size_t)(hi - lo) * sizeof(double), hipMemcpyDeviceToHost, eng->copy_stream));
        }
        MPG_HIP(hipEventRecord(eng->slice_ev[k], eng->copy_stream));
        issued = k + 1;
        if(k == 0) {
            // (the PM step's GravPM / Potential must be in P[] before the tree's Potential goes over it)
            eng->host_join();
            MPG_CHECK(eng->unpack_error.empty(), "host path: the write-back of GravPM failed: " + eng->unpack_error);
            const int device = eng->device;
            mpg_engine *e = eng;
            writer = std::thread([=, &therr, &issued, &abandon] {
                if(hipSetDevice(device) != hipSuccess) {
                    therr = "hipSetDevice";
                    return;
                }
                for(int q = 0; q < S; q++) {
                    while(issued.load() <= q) { // (the main thread is inside the walk of slice q)
                        if(abandon.load())
                            return;
                        std::this_thread::sleep_for(std::chrono::microseconds(50));
                    }
                    if(hipEventSynchronize(e->slice_ev[q]) != hipSuccess) {
                        therr = "hipEventSynchronize";
                        return;
                    }
                    const int64_t a = cut[q], b = cut[q + 1];
                    if(b > a)
                        parallel_for(b - a, [=](int64_t j0, int64_t j1) {
                            for(int64_t j = a + j0; j < a + j1; j++)
                                store_walk_result(T, h_order[j], hat + 3 * j, hpt ? hpt + j : nullptr, nullptr, true);
                        });
                }
            });
        }
    }
    hc.mark("walk (sliced)");
    writer.join();
    MPG_CHECK(therr.empty(), "host path: the write-back of the walk's results failed: " + therr);
    hc.mark("last slice down");
}

// One walk of all its targets, then the results down and into P[] / AccelStore.  dev_old: OldAcc is taken on the device.
static void walk_whole(mpg_engine *eng, const HostTable &T, const int *ActiveParticle, const int *d_act, int64_t NumActiveParticle,
                       double (*AccelStore)[3], bool dev_old, bool wantpot, double rho0, HostClock &hc)
{
    const int64_t n = T.V.n;
    const bool full = eng->full_particle_tree;
    // (with overlap the PM step's Potential may still be on its way down from s_pot: the tree's goes to a buffer of its own)
    double *d_treepot = eng->s_pot.p;
    if(eng->host_overlap && wantpot) {
        eng->s_pot2.reserve((size_t)n + 1);
        d_treepot = eng->s_pot2.p;
    }
    if(dev_old)
        MPG_CALL(mpg_dev_grav_short_tree(eng, nullptr, eng->s_prevacc.p, eng->s_gravpm.p, d_act, NumActiveParticle, eng->s_accel.p,
                                         wantpot ? d_treepot : nullptr, rho0));
    else
        MPG_CALL(mpg_dev_grav_short_tree(eng, eng->s_old.p, nullptr, nullptr, d_act, NumActiveParticle, eng->s_accel.p, wantpot ? d_treepot : nullptr,
                                         rho0));
    hc.mark("walk");
    // (the PM step's GravPM / Potential must be in P[] before this call's Potential - the tree's, gravshort.h:94-95 - goes over it)
    eng->host_join();
    hc.mark("join");
    MPG_CHECK(eng->unpack_error.empty(), "host path: the write-back of GravPM failed: " + eng->unpack_error);
    eng->h_d2.reserve(3 * (size_t)n + 1);
    eng->h_d3.reserve((size_t)n + 1);
    double *ha = eng->h_d2.p, *hp = eng->h_d3.p; // (OldAcc has been uploaded: its staging buffer is free again)
    // (garbage / swallowed particles are no walk targets, treewalk.c:234: their fields stay as they are.  eng->h_b holds the live flags
    // of the staged table whenever it has dead records: stage_particles)
    const uint8_t *liveflag = eng->pm_live ? eng->h_b.p : nullptr;
    auto put = [=](int64_t i) {
        if(!liveflag || liveflag[i])
            store_walk_result(T, i, ha + 3 * i, wantpot ? hp + i : nullptr, AccelStore, full);
    };
    const double *da = eng->s_accel.p, *dpot = d_treepot;
    hipStream_t st = eng->stream;
    if(!ActiveParticle) // all particles: unpack chunk by chunk while the later chunks are still on the bus
        download_chunks(
            eng->chunk_ev, st, n,
            [=](int64_t lo, int64_t hi) {
                MPG_HIP(hipMemcpyAsync(ha + 3 * lo, da + 3 * lo, 3 * (hi - lo) * sizeof(double), hipMemcpyDeviceToHost, st));
                if(wantpot)
                    MPG_HIP(hipMemcpyAsync(hp + lo, dpot + lo, (hi - lo) * sizeof(double), hipMemcpyDeviceToHost, st));
            },
            [=](int64_t lo, int64_t hi) {
                for(int64_t i = lo; i < hi; i++)
                    put(i);
            });
    else {
        MPG_HIP(hipMemcpyAsync(ha, da, 3 * n * sizeof(double), hipMemcpyDeviceToHost, st));
        if(wantpot)
            MPG_HIP(hipMemcpyAsync(hp, dpot, n * sizeof(double), hipMemcpyDeviceToHost, st));
        MPG_HIP(hipStreamSynchronize(st));
        parallel_for(NumActiveParticle, [=](int64_t lo, int64_t hi) {
            for(int64_t k = lo; k < hi; k++)
                put(ActiveParticle[k]);
        });
    }
    hc.mark("download+unpack");
}

// mpg_grav_short_tree on a host table
static void walk_host(mpg_engine *eng, const mpg_particle_view *P, const int *ActiveParticle, int64_t NumActiveParticle, double (*AccelStore)[3],
                      double rho0)
{
    const int64_t n = P->n;
    const HostTable T(*P);
    // OldAcc = |FullTreeGravAccel + GravPM| / G (grav_short_copy, gravshort.h:82-86).  With overlap, and when this epoch's first call
    // uploaded FullTreeGravAccel and this epoch's gravpm_force left GravPM on the device, it is taken there (k_oldacc / the list kernel:
    // the same arithmetic); otherwise from P[] on the host.
    HostClock hc("grav_short_tree");
    const bool dev_old = eng->host_overlap && eng->host_epoch != 0 && eng->staged_extra_epoch == eng->host_epoch &&
                         eng->gravpm_epoch == eng->host_epoch && eng->staged_base == P->base && eng->staged_n == n;
    eng->s_accel.reserve(3 * (size_t)n + 1);
    eng->s_pot.reserve((size_t)n + 1);
    if(!dev_old) {
        eng->host_join(); // (GravPM is read from P[])
        eng->h_d3.reserve((size_t)n + 1);
        double *old = eng->h_d3.p;
        const double G = eng->pm.G;
        parallel_for(n, [=](int64_t lo, int64_t hi) {
            for(int64_t i = lo; i < hi; i++) {
                const double *a = T.vec(i, T.V.off_accel), *g = T.vec(i, T.V.off_gravpm);
                double s2 = 0;
                for(int j = 0; j < 3; j++) {
                    const double ax = a[j] + g[j];
                    s2 += ax * ax;
                }
                old[i] = sqrt(s2) / G;
            }
        });
        eng->s_old.reserve((size_t)n + 1);
        MPG_HIP(hipMemcpyAsync(eng->s_old.p, old, n * sizeof(double), hipMemcpyHostToDevice, eng->stream));
    }
    const int *d_act = upload_active(eng->s_active, ActiveParticle, NumActiveParticle, eng->stream);
    const bool full = eng->full_particle_tree;
    const bool wantpot = full && P->off_potential >= 0;
    MPG_HIP(hipMemsetAsync(eng->s_accel.p, 0, 3 * n * sizeof(double), eng->stream));
    if(dev_old && eng->ev_acc_up) // (FullTreeGravAccel went up on the copy stream)
        MPG_HIP(hipStreamWaitEvent(eng->stream, eng->ev_acc_up, 0));
    static const int nslices_env = getenv("MPG_HOST_WALK_SLICES") ? atoi(getenv("MPG_HOST_WALK_SLICES")) : 5;
    const int64_t npart = eng->tree.npart;
    const int nslices = eng->host_slices > 1 ? eng->host_slices : (npart >= (1 << 20) ? nslices_env : 1); // (small walks: not worth the calls)
    if(eng->host_overlap && dev_old && !ActiveParticle && !AccelStore && full && eng->copy_stream && nslices > 1 && npart >= 8 * nslices)
        walk_sliced(eng, T, wantpot, nslices < 8 ? nslices : 8, rho0, hc);
    else
        walk_whole(eng, T, ActiveParticle, d_act, NumActiveParticle, AccelStore, dev_old, wantpot, rho0, hc);
    //  after a walk on a tree of all particles P[].FullTreeGravAccel holds THIS walk's result: the copy staged at the
    // epoch's first upload is no longer what grav_short_copy (gravshort.h:82-86) would read.  A second walk of the same epoch takes OldAcc
    // from P[] again.
    if(full)
        eng->staged_extra_epoch = -1;
}

int mpg_grav_short_tree(mpg_engine *eng, const mpg_particle_view *P, const int *ActiveParticle, int64_t NumActiveParticle,
                        double (*AccelStore)[3], double rho0)
{
    API_BEGIN
    MPG_CHECK(eng && P, "null argument");
    MPG_HIP(hipSetDevice(eng->device));
    MPG_CHECK(eng->tree_allocated && eng->tree.has_moments, "Gravtree called before tree moments computed!");
    MPG_CHECK(P->n == eng->n, "grav_short_tree: particle table changed size since the tree was built");
    MPG_CHECK(P->off_accel >= 0 && P->off_gravpm >= 0, "particle view needs FullTreeGravAccel and GravPM");
    if(eng->resident && eng->res_base == P->base)
        walk_resident(eng, P, ActiveParticle, NumActiveParticle, AccelStore, rho0);
    else
        walk_host(eng, P, ActiveParticle, NumActiveParticle, AccelStore, rho0);
    API_END
}

/* ---- potential planes on a host table (write_plane, plane.c:572-683; the kernels are planes.hip's) ----------------------------------- */
// IsGarbage / Swallowed of the records -> device bytes (null when the view has no flags).  In resident mode the host records are stale in
// every column the engine integrates, but nothing on the device sets or clears these two bits, so they are read from the host table.
static const uint8_t *stage_plane_flags(mpg_engine *eng, const mpg_particle_view *P)
{
    if(P->off_flags < 0 || P->n == 0)
        return nullptr;
    const int64_t n = P->n;
    // (not h_b: inside a declared epoch it holds the live flags the write-back of mpg_grav_short_tree reads)
    eng->h_plane_flags.reserve((size_t)n + 1);
    eng->plane_flags.reserve((size_t)n + 1);
    uint8_t *hb = eng->h_plane_flags.p;
    const HostTable T(*P);
    parallel_for(n, [=](int64_t lo, int64_t hi) {
        for(int64_t i = lo; i < hi; i++)
            hb[i] = T.flags(i) & 3;
    });
    MPG_HIP(hipMemcpyAsync(eng->plane_flags.p, hb, (size_t)n, hipMemcpyHostToDevice, eng->stream));
    MPG_HIP(hipStreamSynchronize(eng->stream));
    return eng->plane_flags.p;
}

void host_planes(mpg_engine *eng, const mpg_particle_view *P, const mpg_plane_params *par, double *planes, int64_t *npart)
{
    int64_t ncuts = 0;
    MPG_CALL(mpg_plane_count(eng, par, 0.0, &ncuts));
    MPG_CHECK(par->Resolution >= 1, "potential planes: Resolution must be at least 1");
    MPG_CHECK(par->Resolution <= 32768, "potential planes: Resolution above 32768");
    const size_t tot = (size_t)ncuts * (size_t)(par->nnormals > 0 ? par->nnormals : 0) * (size_t)par->Resolution * par->Resolution;
    MPG_CHECK(tot == 0 || (planes && npart), "potential planes: null output");
    eng->plane_out.reserve(tot + 1);
    const uint8_t *fl = stage_plane_flags(eng, P);
    planes_run(eng, par, fl, eng->plane_out.p, npart, nullptr);
    if(tot)
        MPG_HIP(hipMemcpyAsync(planes, eng->plane_out.p, tot * sizeof(double), hipMemcpyDeviceToHost, eng->stream));
    MPG_HIP(hipStreamSynchronize(eng->stream));
}

int mpg_potential_planes(mpg_engine *eng, const mpg_particle_view *P, double BoxSize, const mpg_plane_params *params, double *planes, int64_t *npart)
{
    API_BEGIN
    MPG_CHECK(eng && P && params, "null argument");
    MPG_CHECK(BoxSize > 0, "potential planes: BoxSize must be positive");
    MPG_HIP(hipSetDevice(eng->device));
    eng->host_join(); // (a running prefetch is joined, a write-back of the last PM step finished)
    MPG_CHECK(eng->unpack_error.empty(), "host path: the write-back of GravPM failed: " + eng->unpack_error);
    stage_particles(eng, P, BoxSize);
    host_planes(eng, P, params, planes, npart);
    API_END
}

int mpg_grav_short_pair(mpg_engine *eng, const mpg_particle_view *P, const int *ActiveParticle, int64_t NumActiveParticle, double Rcut, double rho0)
{
    API_BEGIN
    MPG_CHECK(eng && P, "null argument");
    MPG_HIP(hipSetDevice(eng->device));
    MPG_CHECK(eng->tree_allocated, "grav_short_pair: no tree");
    MPG_CHECK(P->n == eng->n, "grav_short_pair: particle table changed size since the tree was built");
    MPG_CHECK(P->off_accel >= 0, "particle view needs FullTreeGravAccel");
    const int64_t n = P->n;
    eng->s_accel.reserve(3 * (size_t)n + 1);
    eng->s_pot.reserve((size_t)n + 1);
    const int *d_act = upload_active(eng->s_active, ActiveParticle, NumActiveParticle, eng->stream);
    const bool full = eng->full_particle_tree;
    const bool wantpot = full && P->off_potential >= 0;
    MPG_HIP(hipMemsetAsync(eng->s_accel.p, 0, 3 * n * sizeof(double), eng->stream));
    MPG_CALL(mpg_dev_grav_short_pair(eng, d_act, NumActiveParticle, Rcut, eng->s_accel.p, wantpot ? eng->s_pot.p : nullptr, rho0));
    eng->h_d2.reserve(3 * (size_t)n + 1);
    eng->h_d3.reserve((size_t)n + 1);
    double *ha = eng->h_d2.p, *hp = eng->h_d3.p;
    MPG_HIP(hipMemcpyAsync(ha, eng->s_accel.p, 3 * n * sizeof(double), hipMemcpyDeviceToHost, eng->stream));
    if(wantpot)
        MPG_HIP(hipMemcpyAsync(hp, eng->s_pot.p, n * sizeof(double), hipMemcpyDeviceToHost, eng->stream));
    MPG_HIP(hipStreamSynchronize(eng->stream));
    if(full) { // the pair-wise result reaches the caller only through P (gravshort.h:54-66): priv.Accel is freed on return
        const HostTable T(*P);
        parallel_for(ActiveParticle ? NumActiveParticle : n, [=](int64_t lo, int64_t hi) {
            for(int64_t k = lo; k < hi; k++) {
                const int64_t i = ActiveParticle ? ActiveParticle[k] : k;
                store_walk_result(T, i, ha + 3 * i, wantpot ? hp + i : nullptr, nullptr, true);
            }
        });
    }
    API_END
}

int mpg_force_tree_active_moments(mpg_engine *eng, const mpg_particle_view *P, double BoxSize, const int *ActiveParticle,
                                  int64_t NumActiveParticle, int HybridNuTracer)
{
    API_BEGIN
    MPG_CHECK(eng && P, "null argument");
    MPG_HIP(hipSetDevice(eng->device));
    stage_particles(eng, P, BoxSize);
    const int *d_act = upload_active(eng->s_active, ActiveParticle, NumActiveParticle, eng->stream);
    MPG_CALL(mpg_dev_force_tree_active_moments(eng, d_act, NumActiveParticle, HybridNuTracer));
    API_END
}

/* host-pointer SPH path: stage every array of mpg_sph_arrays in HBM (doubles: hsml, dthsml, vel[3], gacc[3], gpm[3],
 * hydroacc_in[3], entropy, dtentropy_in, density, egywtdensity, dhsmlegyfac, divvel, curlvel, gradrho[3], hydroacc_out[3],
 * dtentropy_out, maxsignalvel; bytes: tb_hydro, tb_grav) */
void stage_sph(mpg_engine *eng, const mpg_sph_arrays *host, mpg_sph_arrays *dev, int64_t n)
{
    // (the staging buffers ARE the resident copies of a gas run: another array set must wait for mpg_resident_sph_end)
    MPG_CHECK(!eng->sph_resident, "SPH host call with arrays other than the resident gas run's (mpg_resident_sph_end first)");
    for(const SphField &F : SPH_FIELDS) {
        void *h = field_get(*host, F.off), *d = nullptr;
        if(h && F.width == 0) {
            eng->h_sph_u8[F.slot].reserve((size_t)n + 1);
            d = eng->h_sph_u8[F.slot].p;
            MPG_HIP(hipMemcpyAsync(d, h, (size_t)n, hipMemcpyHostToDevice, eng->stream));
        }
        else if(h) {
            eng->h_sph[F.slot].reserve((size_t)n * F.width + 1);
            d = eng->h_sph[F.slot].p;
            if(F.role & (SPH_IN | SPH_HYDRO_IN)) // (every call stages afresh: the hydro loop's inputs from the density loop too)
                MPG_HIP(hipMemcpyAsync(d, h, sph_field_bytes(F, n), hipMemcpyHostToDevice, eng->stream));
            else
                MPG_HIP(hipMemsetAsync(d, 0, sph_field_bytes(F, n), eng->stream));
        }
        field_set(*dev, F.off, d);
    }
}

// the results of the density loop (hydro false) or of the hydro loop into the host arrays
static void unstage_sph(mpg_engine *eng, const mpg_sph_arrays *host, const mpg_sph_arrays *dev, int64_t n, bool hydro)
{
    for(const SphField &F : SPH_FIELDS) {
        void *h = field_get(*host, F.off);
        if(h && (F.role & (hydro ? SPH_OUT_HYDRO : SPH_OUT_DENSITY)))
            MPG_HIP(hipMemcpyAsync(h, field_get(*dev, F.off), sph_field_bytes(F, n), hipMemcpyDeviceToHost, eng->stream));
    }
    MPG_HIP(hipStreamSynchronize(eng->stream));
}
// the host arrays of a resident gas run (mpg_resident_sph_begin): their device copies are current, nothing is staged
static bool sph_is_resident(mpg_engine *eng, const mpg_particle_view *P, const mpg_sph_arrays *A)
{
    return eng->sph_resident && eng->resident && eng->res_base == P->base && A->hsml == eng->res_sph_host.hsml;
}

int mpg_set_init_hsml(mpg_engine *eng, const mpg_particle_view *P, double BoxSize, const mpg_sph_arrays *A, double MeanGasSeparation)
{
    API_BEGIN
    MPG_CHECK(eng && P && A, "null argument");
    MPG_HIP(hipSetDevice(eng->device));
    stage_particles(eng, P, BoxSize);
    mpg_sph_arrays d;
    stage_sph(eng, A, &d, P->n);
    // the reference calls it on the GAS+BH tree with moments (init.c:485-511, test_density.c:86-87)
    MPG_CALL(mpg_dev_force_tree_rebuild_mask(eng, 1 + 32, 1));
    MPG_CALL(mpg_dev_set_init_hsml(eng, &d, MeanGasSeparation));
    MPG_HIP(hipMemcpyAsync(A->hsml, d.hsml, P->n * sizeof(double), hipMemcpyDeviceToHost, eng->stream));
    MPG_HIP(hipStreamSynchronize(eng->stream));
    API_END
}

int mpg_density(mpg_engine *eng, const mpg_particle_view *P, double BoxSize, const mpg_sph_arrays *A, const mpg_sph_times *T,
                const int *ActiveParticle, int64_t NumActiveParticle, int update_hsml, int DoEgyDensity, int BlackHoleOn)
{
    API_BEGIN
    MPG_CHECK(eng && P && A && T, "null argument");
    MPG_HIP(hipSetDevice(eng->device));
    stage_particles(eng, P, BoxSize);
    mpg_sph_arrays d;
    const bool res = sph_is_resident(eng, P, A); // a resident gas run: the arrays are in HBM already and stay there
    if(res)
        d = eng->res_sph_dev;
    else
        stage_sph(eng, A, &d, P->n);
    const int *d_act = upload_active(eng->s_active, ActiveParticle, NumActiveParticle, eng->stream);
    MPG_CALL(mpg_dev_force_tree_rebuild_mask(eng, 1 /* GASMASK */, 0));
    MPG_CALL(mpg_dev_density(eng, &d, T, d_act, NumActiveParticle, update_hsml, DoEgyDensity, BlackHoleOn));
    MPG_CALL(mpg_dev_force_tree_calc_hmax(eng)); // (update_hsml = 0: from the caller's Hsml, see SphEngine::density)
    if(!res)
        unstage_sph(eng, A, &d, P->n, false);
    API_END
}

int mpg_hydro_force(mpg_engine *eng, const mpg_particle_view *P, const mpg_sph_arrays *A, const mpg_sph_times *T,
                    const int *ActiveParticle, int64_t NumActiveParticle)
{
    API_BEGIN
    MPG_CHECK(eng && P && A && T, "null argument");
    MPG_HIP(hipSetDevice(eng->device));
    MPG_CHECK(eng->tree_allocated && eng->tree.has_hmax, "Hydro called before hmax computed"); // hydra.c:172-173
    MPG_CHECK(P->n == eng->n, "hydro_force: particle table changed size since density()");
    mpg_sph_arrays d;
    const bool res = sph_is_resident(eng, P, A);
    if(res)
        d = eng->res_sph_dev;
    else
        stage_sph(eng, A, &d, P->n);
    const int *d_act = upload_active(eng->s_active, ActiveParticle, NumActiveParticle, eng->stream);
    // the host DelayTime column of mpg_set_delaytime travels with the call and is the column in effect for it
    const double *const bound = eng->d_delaytime;
    if(eng->h_delaytime && P->n > 0) {
        // (a buffer of its own: s_delaytime may hold the column of mpg_resident_sph_set_delaytime, which comes back into effect below)
        eng->s_delaytime_call.reserve((size_t)P->n + 1);
        MPG_HIP(hipMemcpyAsync(eng->s_delaytime_call.p, eng->h_delaytime, (size_t)P->n * sizeof(double), hipMemcpyHostToDevice, eng->stream));
        eng->d_delaytime = eng->s_delaytime_call.p;
    }
    const int rc = mpg_dev_hydro_force(eng, &d, T, d_act, NumActiveParticle);
    if(eng->h_delaytime)
        eng->d_delaytime = bound;
    MPG_CHECK(rc == 0, mpg_last_error());
    if(!res)
        unstage_sph(eng, A, &d, P->n, true);
    API_END
}

int mpg_find_vel_disp(mpg_engine *eng, const mpg_particle_view *pv, double BoxSize, const mpg_veldisp_arrays *A, const mpg_sph_times *T,
                      const mpg_veldisp_params *par, const int *ActiveParticle, int64_t NumActiveParticle)
{
    API_BEGIN
    MPG_CHECK(eng && pv && A && T && par, "null argument");
    MPG_CHECK(A->vel && A->hsml && A->density && A->vdisp, "find_vel_disp: the arrays vel, hsml, density and vdisp are required");
    MPG_HIP(hipSetDevice(eng->device));
    stage_particles(eng, pv, BoxSize);
    mpg_veldisp_arrays d{};
    stage_fields(VDISP_FIELDS, *A, d, eng->vd_stage, pv->n, 0, "find_vel_disp", eng->stream);
    const int *d_act = upload_active(eng->s_active, ActiveParticle, NumActiveParticle, eng->stream);
    MPG_CALL(mpg_dev_find_vel_disp(eng, &d, T, par, d_act, NumActiveParticle));
    unstage_fields(VDISP_FIELDS, *A, d, pv->n, 0, eng->stream); // (vdisp alone)
    MPG_HIP(hipStreamSynchronize(eng->stream));
    API_END
}

// the host local_J21 / zreion columns of mpg_set_excursion_columns travel with a host-form call and are the columns in effect for it; the
// device columns bound before come back into effect when the guard ends (as DelayTime does in mpg_hydro_force)
struct ExcursionColumnsOfCall {
    CoolingEngine &E;
    const double *j21, *zre;
    int64_t n_exc;
    const bool swapped;
    ExcursionColumnsOfCall(mpg_engine *eng, int64_t n) : E(eng->cooling), j21(E.d_j21), zre(E.d_zre), n_exc(E.n_exc), swapped(E.h_j21 && n > 0)
    {
        if(!swapped)
            return;
        // (buffers of their own: s_j21 / s_zre may hold the columns of mpg_resident_sph_set_excursion_columns)
        E.s_j21_call.reserve((size_t)n + 1);
        E.s_zre_call.reserve((size_t)n + 1);
        MPG_HIP(hipMemcpyAsync(E.s_j21_call.p, E.h_j21, (size_t)n * sizeof(double), hipMemcpyHostToDevice, eng->stream));
        MPG_HIP(hipMemcpyAsync(E.s_zre_call.p, E.h_zre, (size_t)n * sizeof(double), hipMemcpyHostToDevice, eng->stream));
        E.d_j21 = E.s_j21_call.p;
        E.d_zre = E.s_zre_call.p;
        E.n_exc = n;
    }
    ~ExcursionColumnsOfCall()
    {
        if(swapped) {
            E.d_j21 = j21;
            E.d_zre = zre;
            E.n_exc = n_exc;
        }
    }
};

// cooling_direct for the listed particles of a host table (sfr_eff.c:463-514).  The results are copied back even when a particle hit an
// iteration limit: that particle's entries come back as they went up, all others are final.
int mpg_cooling(mpg_engine *eng, const mpg_particle_view *pv, double BoxSize, const mpg_cooling_arrays *A, const mpg_sph_times *T,
                const mpg_cooling_step *step, const int *ActiveParticle, int64_t NumActiveParticle)
{
    API_BEGIN
    MPG_CHECK(eng && pv && A && T && step, "null argument");
    MPG_CHECK(pv->n == 0 || (A->density && A->entropy && A->ne && A->sfr), "cooling: the arrays density, entropy, ne and sfr are required");
    MPG_HIP(hipSetDevice(eng->device));
    stage_particles(eng, pv, BoxSize);
    mpg_cooling_arrays d{};
    stage_fields(COOL_FIELDS, *A, d, eng->cl_stage, pv->n, 0, "cooling", eng->stream);
    const int *d_act = upload_active(eng->s_active, ActiveParticle, NumActiveParticle, eng->stream);
    int rc;
    {
        const ExcursionColumnsOfCall guard(eng, pv->n);
        rc = mpg_dev_cooling(eng, &d, T, step, d_act, NumActiveParticle);
    }
    const std::string err = rc ? mpg_last_error() : "";
    if(pv->n > 0)
        unstage_fields(COOL_FIELDS, *A, d, pv->n, 0, eng->stream);
    MPG_HIP(hipStreamSynchronize(eng->stream));
    MPG_CHECK(rc == 0, err);
    API_END
}

// cooling_and_starformation without the spawning for the listed particles of a host table (sfr_eff.c:224-286).  The columns are copied
// back even when a row hit an iteration limit: that row's entries come back as they went up, all others are final.
int mpg_cooling_and_starformation(mpg_engine *eng, const mpg_particle_view *pv, double BoxSize, const mpg_sfr_columns *A, const mpg_sph_times *T,
                                  const mpg_cooling_step *step, const int *ActiveParticle, int64_t NumActiveParticle)
{
    API_BEGIN
    MPG_CHECK(eng && pv && A && T && step, "null argument");
    MPG_HIP(hipSetDevice(eng->device));
    stage_particles(eng, pv, BoxSize);
    mpg_sfr_columns d{};
    if(pv->n > 0)
        stage_fields(SFR_FIELDS, *A, d, eng->sf_stage, pv->n, 0, "cooling_and_starformation", eng->stream);
    const int *d_act = upload_active(eng->s_active, ActiveParticle, NumActiveParticle, eng->stream);
    int rc;
    {
        const ExcursionColumnsOfCall guard(eng, pv->n);
        rc = mpg_dev_cooling_and_starformation(eng, &d, T, step, d_act, NumActiveParticle);
    }
    const std::string err = rc ? mpg_last_error() : "";
    if(pv->n > 0)
        unstage_fields(SFR_FIELDS, *A, d, pv->n, 0, eng->stream);
    MPG_HIP(hipStreamSynchronize(eng->stream));
    MPG_CHECK(rc == 0, err);
    API_END
}

// calculate_uvbg for a host table (uvbg.c:506-593): the four columns go through stage_fields / unstage_fields (host_table.h)
int mpg_calculate_uvbg(mpg_engine *eng, const mpg_particle_view *pv, double BoxSize, const mpg_uvbg_params *par, const mpg_uvbg_columns *A,
                       mpg_uvbg_result *result)
{
    API_BEGIN
    MPG_CHECK(eng && pv && par && A && result, "calculate_uvbg: null argument");
    MPG_HIP(hipSetDevice(eng->device));
    stage_particles(eng, pv, BoxSize);
    mpg_uvbg_columns d{};
    if(pv->n > 0)
        stage_fields(UVBG_FIELDS, *A, d, eng->uv_stage, pv->n, 0, "calculate_uvbg", eng->stream);
    const int rc = mpg_dev_calculate_uvbg(eng, par, &d, result);
    const std::string err = rc ? mpg_last_error() : "";
    if(pv->n > 0)
        unstage_fields(UVBG_FIELDS, *A, d, pv->n, 0, eng->stream);
    MPG_HIP(hipStreamSynchronize(eng->stream));
    MPG_CHECK(rc == 0, err);
    API_END
}

// metal_return for the listed particles of a host table: Mass is the records' column (staged with the table, written back into it), the
// other arrays go through stage_fields / unstage_fields (host_table.h)
int mpg_metal_return(mpg_engine *eng, const mpg_particle_view *pv, double BoxSize, const mpg_metal_arrays *A, const int *ActiveParticle,
                     int64_t NumActiveParticle)
{
    API_BEGIN
    MPG_CHECK(eng && pv && A, "null argument");
    MPG_HIP(hipSetDevice(eng->device));
    stage_particles(eng, pv, BoxSize);
    const int64_t n = pv->n;
    mpg_metal_arrays d{};
    stage_fields(METAL_FIELDS, *A, d, eng->mt_stage, n, ARR_TABLE, "metal_return", eng->stream);
    d.mass = eng->s_mass.p;
    const int *d_act = upload_active(eng->s_active, ActiveParticle, NumActiveParticle, eng->stream);
    // the tree of the call: the gas tree as mpg_density builds it.  (Built before the dev call, which demands it only when it has a target;
    // whether it has one is the device's knowledge, and a second queue pass here would cost what the build of a small tree costs.)
    MPG_CALL(mpg_dev_force_tree_rebuild_mask(eng, 1 /* GASMASK */, 0));
    MPG_CALL(mpg_dev_metal_return(eng, &d, d_act, NumActiveParticle));
    unstage_fields(METAL_FIELDS, *A, d, n, ARR_TABLE, eng->stream);
    if(eng->metals.ntargets > 0) {
        eng->mt_mass.reserve((size_t)n + 1);
        mass_to_records(*pv, eng->s_mass.p, eng->mt_mass.p, eng->stream);
    }
    MPG_HIP(hipStreamSynchronize(eng->stream));
    API_END
}

// blackhole_dynfric + blackhole_dfaccel for the listed particles of a host table: the arrays go through stage_fields / unstage_fields
// (host_table.h); nothing of the records is written.  The tree of the call's mask is built by the call itself once it has a target.
int mpg_blackhole_dynfric(mpg_engine *eng, const mpg_particle_view *pv, double BoxSize, const mpg_bh_dynfric_arrays *A, const mpg_sph_times *T,
                          const int *ActiveParticle, int64_t NumActiveParticle)
{
    API_BEGIN
    MPG_CHECK(eng && pv && A && T, "null argument");
    MPG_HIP(hipSetDevice(eng->device));
    stage_particles(eng, pv, BoxSize);
    const int64_t n = pv->n;
    const int *d_act = upload_active(eng->s_active, ActiveParticle, NumActiveParticle, eng->stream);
    // the queue pass first: without a listed black hole nothing travels, nothing is read and nothing is written
    if(dynfric_listed(eng, d_act, NumActiveParticle) == 0) {
        mpg_err_slot().clear();
        return 0;
    }
    mpg_bh_dynfric_arrays d{};
    stage_fields(DF_FIELDS, *A, d, eng->df_stage, n, 0, "blackhole_dynfric", eng->stream);
    dynfric_call(eng, &d, T, d_act, NumActiveParticle);
    unstage_fields(DF_FIELDS, *A, d, n, 0, eng->stream);
    MPG_HIP(hipStreamSynchronize(eng->stream));
    API_END
}

// blackhole() for the listed particles of a host table: Mass is the records' column (staged with the table, written back into it with
// the flags), the other arrays go through stage_fields / unstage_fields (host_table.h).  The tree of gas and black holes and its hmax are built
// by the call itself once it knows that it has a target.
int mpg_blackhole(mpg_engine *eng, const mpg_particle_view *pv, double BoxSize, const mpg_blackhole_arrays *A, const mpg_sph_times *T,
                  const int *ActiveParticle, int64_t NumActiveParticle)
{
    API_BEGIN
    MPG_CHECK(eng && pv && A && T, "null argument");
    MPG_HIP(hipSetDevice(eng->device));
    stage_particles(eng, pv, BoxSize);
    const int64_t n = pv->n;
    const int *d_act = upload_active(eng->s_active, ActiveParticle, NumActiveParticle, eng->stream);
    // the queue pass first: without a target nothing travels, nothing is read and nothing is written
    if(blackhole_targets(eng, d_act, NumActiveParticle) == 0) {
        mpg_err_slot().clear();
        return 0;
    }
    mpg_blackhole_arrays d{};
    stage_fields(BH_FIELDS, *A, d, eng->bh_stage, n, ARR_TABLE, "blackhole", eng->stream);
    d.mass = eng->s_mass.p;
    // (a tree that a previous call left is one of another table or another step: always rebuilt when there is a target)
    blackhole_call(eng, &d, T, d_act, NumActiveParticle, 2);
    unstage_fields(BH_FIELDS, *A, d, n, ARR_TABLE, eng->stream);
    if(eng->bh.ntargets > 0) {
        BlackholeEngine::retype(eng->s_type.p, d.flags, n, eng->stream);
        eng->bh_mass.reserve((size_t)n + 1);
        mass_to_records(*pv, eng->s_mass.p, eng->bh_mass.p, eng->stream);
        MPG_HIP(hipStreamSynchronize(eng->stream));
        flags_to_records(*pv, A->flags);
    }
    MPG_HIP(hipStreamSynchronize(eng->stream));
    API_END
}

// winds_and_feedback for the new stars of a host table: the arrays go through stage_fields / unstage_fields (host_table.h); nothing of the records
// is written.  Without a new star, or with the subgrid model, nothing travels and no tree is built (winds.c:302-306).
int mpg_winds_and_feedback(mpg_engine *eng, const mpg_particle_view *pv, double BoxSize, const mpg_wind_arrays *A, const int *NewStars,
                           int64_t NumNewStars, double atime)
{
    API_BEGIN
    MPG_CHECK(eng && pv && A, "null argument");
    MPG_CHECK(NumNewStars >= 0, "winds_and_feedback: negative list length");
    MPG_CHECK(eng->have_windpar, "winds_and_feedback: no parameters (mpg_set_wind_params first)");
    if((eng->windpar.WindModel & WIND_SUBGRID) != 0 || NumNewStars == 0) {
        mpg_err_slot().clear();
        return 0;
    }
    MPG_CHECK(NewStars, "winds_and_feedback: no list of new stars");
    MPG_HIP(hipSetDevice(eng->device));
    stage_particles(eng, pv, BoxSize);
    const int64_t n = pv->n;
    mpg_wind_arrays d{};
    stage_fields(WD_FIELDS, *A, d, eng->wd_stage, n, ARR_OTHER_CALL, "winds_and_feedback", eng->stream);
    const int *d_new = upload_active(eng->s_active, NewStars, NumNewStars, eng->stream);
    // the tree of the call: the gas tree as mpg_density builds it (winds_find_weights, winds.c:235-240)
    MPG_CALL(mpg_dev_force_tree_rebuild_mask(eng, 1 /* GASMASK */, 0));
    MPG_CALL(mpg_dev_winds_and_feedback(eng, &d, d_new, NumNewStars, atime));
    unstage_fields(WD_FIELDS, *A, d, n, ARR_OTHER_CALL, eng->stream);
    MPG_HIP(hipStreamSynchronize(eng->stream));
    API_END
}

// the candidate groups of the helium reionisation from HOST group columns (the dev form gathers them from the device table)
HeiiiGroups heiii_host_groups(const double *mass, const double *cm, const uint64_t *minid, int64_t ngroups)
{
    return [=](const mpg_heiii_params &par, std::vector<int64_t> &cand, std::vector<double> &ccm, std::vector<uint64_t> &cid) {
        MPG_CHECK(ngroups == 0 || (mass && cm && minid), "heiii_reionization: the group columns mass, cm and minid are required");
        heiii_candidates(par, mass, ngroups, cand);
        for(int64_t g : cand) {
            for(int j = 0; j < 3; j++)
                ccm.push_back(cm[3 * g + j]);
            cid.push_back(minid[g]);
        }
    };
}

// do_heiii_reionization on a host table: Density, Entropy and the flag go up, Entropy and the flag come back; the groups stay on the host.
// No tree is built.
int mpg_heiii_reionization(mpg_engine *eng, const mpg_particle_view *pv, double BoxSize, const mpg_heiii_step *step, const double *density,
                           double *entropy, uint8_t *heiii_ionized, const double *group_mass, const double *group_cm,
                           const uint64_t *group_minid, int64_t ngroups, mpg_heiii_result *result)
{
    API_BEGIN
    MPG_CHECK(eng && pv && step, "null argument");
    MPG_CHECK(ngroups >= 0, "heiii_reionization: negative group number");
    MPG_CHECK(pv->n == 0 || (density && entropy && heiii_ionized), "heiii_reionization: the arrays density, entropy and heiii_ionized are required");
    MPG_HIP(hipSetDevice(eng->device));
    stage_particles(eng, pv, BoxSize);
    const size_t n = (size_t)pv->n;
    eng->he_density.reserve(n + 1);
    eng->he_entropy.reserve(n + 1);
    eng->he_flag.reserve(n + 1);
    if(n > 0) {
        MPG_HIP(hipMemcpyAsync(eng->he_density.p, density, n * sizeof(double), hipMemcpyHostToDevice, eng->stream));
        MPG_HIP(hipMemcpyAsync(eng->he_entropy.p, entropy, n * sizeof(double), hipMemcpyHostToDevice, eng->stream));
        MPG_HIP(hipMemcpyAsync(eng->he_flag.p, heiii_ionized, n, hipMemcpyHostToDevice, eng->stream));
    }
    heiii_call(eng, step, eng->he_density.p, eng->he_entropy.p, eng->he_flag.p, heiii_host_groups(group_mass, group_cm, group_minid, ngroups), result);
    if(n > 0) {
        MPG_HIP(hipMemcpyAsync(entropy, eng->he_entropy.p, n * sizeof(double), hipMemcpyDeviceToHost, eng->stream));
        MPG_HIP(hipMemcpyAsync(heiii_ionized, eng->he_flag.p, n, hipMemcpyDeviceToHost, eng->stream));
    }
    MPG_HIP(hipStreamSynchronize(eng->stream));
    API_END
}
