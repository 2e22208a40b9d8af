// host_table.h -- the marshalling layer of the host-pointer ("drop-in") forms: everything that reads or writes the caller's records
// (mpg_particle_view) and host arrays: mpg_sph_arrays through SPH_FIELDS, whose staging has rules of its own (host_forms.hip), and the
// structs of the velocity dispersion, cooling, metal return, black holes, dynamical friction and winds through one ArrayField table each
// and stage_fields / unstage_fields.  Used by host_forms.hip, resident.hip and dist_host.hip; no engine state lives here.
#pragma once
#include "../../include/mpgadget_hip.h"
#include "mpg_common.h"
#include <condition_variable>
#include <cstddef>
#include <cstring>
#include <functional>
#include <iterator>
#include <mutex>
#include <thread>
#include <vector>

// a nested C-ABI call inside an entry point: its error becomes this call's
#define MPG_CALL(expr)                                 \
    do {                                               \
        if((expr) != 0)                                \
            throw ::mpg::Error(mpg_last_error());      \
    } while(0)

// Pinned, growable host buffer: transfers from / to pageable std::vector memory run at a fraction of the PCIe rate.
template <typename T> struct HostBuf {
    T *p = nullptr;
    size_t cap = 0;
    void reserve(size_t n)
    {
        if(n <= cap)
            return;
        release();
        const size_t want = n + n / 16 + 64;
        MPG_HIP(hipHostMalloc((void **)&p, want * sizeof(T), hipHostMallocDefault));
        cap = want;
    }
    void release()
    {
        if(p)
            (void)hipHostFree(p);
        p = nullptr;
        cap = 0;
    }
    ~HostBuf() { release(); }
    HostBuf() = default;
    HostBuf(const HostBuf &) = delete;
    HostBuf &operator=(const HostBuf &) = delete;
};

// f(lo, hi) over [0, n) on up to 32 host threads: packing 160-byte records into arrays (and back) is memory-bound and one
// thread moves ~2 GB/s of them; the reference's callers have the cores of the rank idle while the GPU works anyway.
// The threads are persistent (round 5): a pass over the table is cut into 8 chunks that overlap the PCIe transfers, i.e. 8 calls, and
// creating 32 threads per call cost 0.3 - 0.5 ms of each (three passes per step on the critical path of the host forms).  A second
// caller that finds the pool busy (the write-back thread of mpg_gravpm_force beside the main thread) starts its own threads as before.
class HostPool {
    std::vector<std::thread> th;
    std::mutex m, busy;
    std::condition_variable cv_work, cv_done;
    const std::function<void(int64_t, int64_t)> *job = nullptr;
    int64_t n = 0, chunk = 0;
    unsigned gen = 0, pending = 0;
    bool stop = false;
    void worker(unsigned t)
    {
        unsigned seen = 0;
        for(;;) {
            const std::function<void(int64_t, int64_t)> *f;
            int64_t lo, hi;
            {
                std::unique_lock<std::mutex> lk(m);
                cv_work.wait(lk, [&] { return stop || gen != seen; });
                if(stop)
                    return;
                seen = gen;
                f = job;
                lo = (int64_t)t * chunk;
                hi = lo + chunk < n ? lo + chunk : n;
            }
            if(lo < hi)
                (*f)(lo, hi);
            {
                std::lock_guard<std::mutex> lk(m);
                if(--pending == 0)
                    cv_done.notify_all();
            }
        }
    }

  public:
    explicit HostPool(unsigned T)
    {
        for(unsigned t = 0; t < T; t++)
            th.emplace_back([this, t] { worker(t); });
    }
    ~HostPool()
    {
        {
            std::lock_guard<std::mutex> lk(m);
            stop = true;
        }
        cv_work.notify_all();
        for(auto &x : th)
            x.join();
    }
    unsigned size() const { return (unsigned)th.size(); }
    // false: the pool is in use by another caller
    bool run(int64_t count, const std::function<void(int64_t, int64_t)> &f)
    {
        std::unique_lock<std::mutex> one(busy, std::try_to_lock);
        if(!one.owns_lock())
            return false;
        std::unique_lock<std::mutex> lk(m);
        job = &f;
        n = count;
        chunk = (count + size() - 1) / size();
        pending = size();
        gen++;
        cv_work.notify_all();
        cv_done.wait(lk, [&] { return pending == 0; });
        return true;
    }
};

inline HostPool &host_pool(unsigned T)
{
    static HostPool pool(T); // ONE pool per process (not one per instantiation of parallel_for); lives until the process ends
    return pool;
}

template <class F> inline void parallel_for(int64_t n, F f)
{
    static const unsigned cap = getenv("MPG_HOST_THREADS") ? (unsigned)atoi(getenv("MPG_HOST_THREADS")) : 32u;
    unsigned T = std::thread::hardware_concurrency();
    if(T > cap)
        T = cap;
    if(T < 2 || n < 131072) {
        f((int64_t)0, n);
        return;
    }
    static const bool use_pool = getenv("MPG_HOST_NO_POOL") == nullptr;
    if(use_pool) {
        const std::function<void(int64_t, int64_t)> fn = [&f](int64_t lo, int64_t hi) { f(lo, hi); };
        if(host_pool(T).run(n, fn))
            return;
    }
    const int64_t chunk = (n + T - 1) / T;
    std::vector<std::thread> th;
    th.reserve(T);
    for(unsigned t = 0; t < T; t++) {
        const int64_t lo = (int64_t)t * chunk, hi = lo + chunk < n ? lo + chunk : n;
        if(lo >= hi)
            break;
        th.emplace_back([=] { f(lo, hi); });
    }
    for(auto &x : th)
        x.join();
}

// ---- the caller's records ------------------------------------------------------------------------------------------------------
// Record i of a mpg_particle_view.  The one place that computes a record address; copied by value into the packing lambdas.
struct HostTable {
    mpg_particle_view V;
    explicit HostTable(const mpg_particle_view &v) : V(v) {}
    char *rec(int64_t i) const { return (char *)V.base + i * V.stride; }
    const double *vec(int64_t i, int64_t off) const { return (const double *)(rec(i) + off); } // a 3-vector (or scalar) column, read
    double *vec_mut(int64_t i, int64_t off) const { return (double *)(rec(i) + off); }         // ... written
    double scalar(int64_t i, int64_t off) const { return *vec(i, off); }
    double &scalar_mut(int64_t i, int64_t off) const { return *vec_mut(i, off); }
    const double *pos(int64_t i) const { return vec(i, V.off_pos); }
    float mass(int64_t i) const { return *(const float *)(rec(i) + V.off_mass); }
    uint8_t type(int64_t i) const { return V.off_type >= 0 ? (uint8_t)(*(const uint8_t *)(rec(i) + V.off_type) & 7) : (uint8_t)1; } // (no Type: dark matter)
    uint8_t flags(int64_t i) const { return V.off_flags >= 0 ? *(const uint8_t *)(rec(i) + V.off_flags) : (uint8_t)0; } // bit 0 IsGarbage, bit 1 Swallowed
};

// Three rules turn IsGarbage / Swallowed into "this record does not take part".  They differ for a swallowed particle that is no
// black hole; each caller keeps the one it has always had.
// Single GPU (stage_particles): garbage and swallowed BLACK HOLES never enter the tree (forcetree.c:806) and, through the same
// type 7, are not deposited and get no mesh force (gravpm.c:176-179) and are no walk targets (treewalk.c:234).
inline bool not_in_tree(uint8_t flags, uint8_t type) { return (flags & 1) || ((flags & 2) && type == 5); }
// Several ranks, gravity (stage_own, the active-only tree): garbage and swallowed particles of any type are skipped in place by every
// loop (treewalk.c:234, forcetree.c:806, gravpm.c:176-179).
inline bool skipped_in_place(uint8_t flags) { return (flags & 3) != 0; }
// Several ranks, SPH (stage_types): garbage and swallowed particles are no targets and no neighbours (density.c:521-530,
// forcetree.c:357-365); they get type 7.
inline bool no_sph_particle(uint8_t flags) { return (flags & 3) != 0; }

// a host index list (ActiveParticle; null: all particles) onto the device, queued on st: the device pointer, or null
inline const int *upload_active(mpg::DevBuf<int> &buf, const int *list, int64_t count, hipStream_t st)
{
    if(!list)
        return nullptr;
    buf.reserve((size_t)count + 1);
    if(count > 0)
        MPG_HIP(hipMemcpyAsync(buf.p, list, (size_t)count * sizeof(int), hipMemcpyHostToDevice, st));
    return buf.p;
}

// One walked particle's results into the caller's memory: AccelStore[i] when given and, when the tree held every particle (to_table;
// gravshort.h:54-66), P[i].FullTreeGravAccel and - pot not null - P[i].Potential.  Whether record i is written at all (garbage,
// swallowed) is the caller's rule.
inline void store_walk_result(const HostTable &T, int64_t i, const double *acc, const double *pot, double (*AccelStore)[3], bool to_table)
{
    if(AccelStore) {
        AccelStore[i][0] = acc[0];
        AccelStore[i][1] = acc[1];
        AccelStore[i][2] = acc[2];
    }
    if(!to_table)
        return;
    double *a = T.vec_mut(i, T.V.off_accel);
    a[0] = acc[0];
    a[1] = acc[1];
    a[2] = acc[2];
    if(pot)
        T.scalar_mut(i, T.V.off_potential) = *pot;
}

// ---- chunked transfers ---------------------------------------------------------------------------------------------------------
// The host <-> device staging of the AoS path is cut into chunks so that packing / unpacking on the host threads overlaps the
// PCIe transfers of the neighbouring chunks (pinned buffers: the copies are asynchronous).
constexpr int HOST_CHUNKS = 8;
inline void chunk_range(int64_t n, int c, int64_t &lo, int64_t &hi)
{
    lo = n * c / HOST_CHUNKS;
    hi = n * (c + 1) / HOST_CHUNKS;
}
// work(lo, hi) for every non-empty chunk in order - the host's pass over it and / or the copies queued for it - and then, when an
// event array is given, ev[c] (created on first use) recorded on st
template <class Work> inline void for_each_chunk(int64_t n, Work work, hipEvent_t *ev = nullptr, hipStream_t st = nullptr)
{
    for(int c = 0; c < HOST_CHUNKS; c++) {
        int64_t lo, hi;
        chunk_range(n, c, lo, hi);
        if(hi > lo)
            work(lo, hi);
        if(ev) {
            if(!ev[c])
                MPG_HIP(hipEventCreateWithFlags(&ev[c], hipEventDisableTiming));
            MPG_HIP(hipEventRecord(ev[c], st));
        }
    }
}
// unpack(lo, hi) runs on the host for each chunk as soon as the device -> host copies issue(lo, hi) queued for it on st have landed
template <class Issue, class Unpack> inline void download_chunks(hipEvent_t *ev, hipStream_t st, int64_t n, Issue issue, Unpack unpack)
{
    for_each_chunk(n, issue, ev, st);
    for(int c = 0; c < HOST_CHUNKS; c++) {
        int64_t lo, hi;
        chunk_range(n, c, lo, hi);
        MPG_HIP(hipEventSynchronize(ev[c]));
        if(hi > lo)
            parallel_for(hi - lo, [=](int64_t a, int64_t b) { unpack(lo + a, lo + b); });
    }
}

// ---- the host arrays of the SPH forms --------------------------------------------------------------------------------------------
// member `off` of a struct of array pointers, read and written as a pointer value (no cast of the struct to a pointer array)
template <class S> inline void *field_get(const S &A, size_t off)
{
    void *p;
    memcpy(&p, (const char *)&A + off, sizeof(p));
    return p;
}
template <class S> inline void field_set(S &A, size_t off, void *p) { memcpy((char *)&A + off, &p, sizeof(p)); }

enum SphRole : unsigned {
    SPH_IN = 1,          // input of the density loop and of the predictions
    SPH_HYDRO_IN = 2,    // result of the density loop that the hydro loop reads
    SPH_OUT_DENSITY = 4, // written by the density loop
    SPH_OUT_HYDRO = 8,   // written by the hydro loop
    SPH_TABLE_ALIAS = 16, // resident run: aliases a column of the resident table (Vel, FullTreeGravAccel, GravPM)
    SPH_PRED_ALIAS = 32,  // resident run: the prediction input aliases last step's output (HydroAccel, DtEntropy)
};
struct SphField {
    const char *name;
    size_t off;    // of the member in mpg_sph_arrays
    int width;     // doubles per particle; 0: one byte per particle
    int slot;      // ordinal among the double (or the byte) members: the staging buffer
    unsigned role; // SphRole bits
};
#define MPG_SPH_FIELD(m, width, slot, role) {#m, offsetof(mpg_sph_arrays, m), width, slot, role}
constexpr int SPH_NFIELDS = 19;
const SphField SPH_FIELDS[SPH_NFIELDS] = {
    MPG_SPH_FIELD(hsml, 1, 0, SPH_IN | SPH_OUT_DENSITY),
    MPG_SPH_FIELD(dthsml, 1, 1, SPH_OUT_DENSITY),
    MPG_SPH_FIELD(vel, 3, 2, SPH_IN | SPH_TABLE_ALIAS),
    MPG_SPH_FIELD(gacc, 3, 3, SPH_IN | SPH_TABLE_ALIAS),
    MPG_SPH_FIELD(gpm, 3, 4, SPH_IN | SPH_TABLE_ALIAS),
    MPG_SPH_FIELD(hydroacc_in, 3, 5, SPH_IN | SPH_PRED_ALIAS),
    MPG_SPH_FIELD(tb_hydro, 0, 0, SPH_IN),
    MPG_SPH_FIELD(tb_grav, 0, 1, SPH_IN),
    MPG_SPH_FIELD(entropy, 1, 6, SPH_IN),
    MPG_SPH_FIELD(dtentropy_in, 1, 7, SPH_IN | SPH_PRED_ALIAS),
    MPG_SPH_FIELD(density, 1, 8, SPH_HYDRO_IN | SPH_OUT_DENSITY),
    MPG_SPH_FIELD(egywtdensity, 1, 9, SPH_HYDRO_IN | SPH_OUT_DENSITY),
    MPG_SPH_FIELD(dhsmlegyfac, 1, 10, SPH_HYDRO_IN | SPH_OUT_DENSITY),
    MPG_SPH_FIELD(divvel, 1, 11, SPH_HYDRO_IN | SPH_OUT_DENSITY),
    MPG_SPH_FIELD(curlvel, 1, 12, SPH_HYDRO_IN | SPH_OUT_DENSITY),
    MPG_SPH_FIELD(gradrho, 3, 13, SPH_OUT_DENSITY),
    MPG_SPH_FIELD(hydroacc_out, 3, 14, SPH_OUT_HYDRO),
    MPG_SPH_FIELD(dtentropy_out, 1, 15, SPH_OUT_HYDRO),
    MPG_SPH_FIELD(maxsignalvel, 1, 16, SPH_OUT_HYDRO),
};
#undef MPG_SPH_FIELD
static_assert(sizeof(mpg_sph_arrays) == SPH_NFIELDS * sizeof(void *), "SPH_FIELDS describes every member of mpg_sph_arrays");
inline size_t sph_field_bytes(const SphField &F, int64_t n) { return F.width == 0 ? (size_t)n : (size_t)n * F.width * sizeof(double); }

// ---- the host arrays of the other calls ------------------------------------------------------------------------------------------
// One table per struct of array pointers, in the struct's member order, and one pair of functions that moves what a table describes.
// A new module's host arrays: (1) a table X_FIELDS here, with its static_assert; (2) `DevBuf<char> x_stage[std::size(X_FIELDS)]` in
// engine_internal.h; (3) stage_fields / the dev call / unstage_fields in its host form; (4) the tuple X_ARRAY_FIELDS, the dict
// X_ARRAY_DTYPES and the class XArraysC in engine.py, bound with _dev_arrays / _host_arrays; (5) the struct's name in STRUCTS of
// tests/test_array_structs.py, which holds the tuple and the dict against the header.
enum ArrayRole : unsigned {
    ARR_IN = 1,         // read by the call
    ARR_OUT = 2,        // comes back
    ARR_OPTIONAL = 4,   // may be NULL
    ARR_TABLE = 8,      // P.Mass: a column of the staged / resident table, never staged from the struct
    ARR_RES_ALIAS = 16, // resident gas run: aliases a resident column
    ARR_OTHER_CALL = 32 // read by another call that takes the same struct: never staged by this one
};
struct ArrayField {
    const char *name;
    size_t off;    // of the member in its struct
    size_t elem;   // bytes of one element: the sizeof of the member's pointee, as the header declares it
    int width;     // elements per particle
    unsigned role; // ArrayRole bits
};
#define MPG_ARRAY_FIELD(S, m, width, role) {#m, offsetof(S, m), sizeof(*S().m), width, role}
// the table names every member of S once and in S's order: entry f is the f-th pointer of the struct
template <class S, size_t N> constexpr bool describes_every_member(const ArrayField (&T)[N])
{
    for(size_t f = 0; f < N; f++)
        if(T[f].off != f * sizeof(void *))
            return false;
    return sizeof(S) == N * sizeof(void *);
}
// the index of the member at `off` (its entry, and its staging buffer); asked for a constant, a member the table lacks does not compile
template <size_t N> constexpr int field_index(const ArrayField (&T)[N], size_t off)
{
    for(size_t f = 0; f < N; f++)
        if(T[f].off == off)
            return (int)f;
    throw mpg::Error("field_index: no such member");
}

// the velocity dispersion: vdisp is in / out (mpg_find_vel_disp checks the required arrays itself, with a text of its own)
constexpr ArrayField VDISP_FIELDS[] = {
    MPG_ARRAY_FIELD(mpg_veldisp_arrays, vel, 3, ARR_IN),
    MPG_ARRAY_FIELD(mpg_veldisp_arrays, gacc, 3, ARR_IN | ARR_OPTIONAL),
    MPG_ARRAY_FIELD(mpg_veldisp_arrays, gpm, 3, ARR_IN | ARR_OPTIONAL),
    MPG_ARRAY_FIELD(mpg_veldisp_arrays, tb_grav, 1, ARR_IN | ARR_OPTIONAL),
    MPG_ARRAY_FIELD(mpg_veldisp_arrays, hsml, 1, ARR_IN),
    MPG_ARRAY_FIELD(mpg_veldisp_arrays, dthsml, 1, ARR_IN | ARR_OPTIONAL),
    MPG_ARRAY_FIELD(mpg_veldisp_arrays, density, 1, ARR_IN),
    MPG_ARRAY_FIELD(mpg_veldisp_arrays, vdisp, 1, ARR_IN | ARR_OUT),
};
static_assert(describes_every_member<mpg_veldisp_arrays>(VDISP_FIELDS), "VDISP_FIELDS follows mpg_veldisp_arrays");

// the cooling: entropy, ne and sfr go up and come back.  (ARR_OPTIONAL throughout: mpg_cooling checks density, entropy, ne and sfr itself,
// with a text of its own, and asks for none of them when the table is empty.)
constexpr ArrayField COOL_FIELDS[] = {
    MPG_ARRAY_FIELD(mpg_cooling_arrays, density, 1, ARR_IN | ARR_OPTIONAL),
    MPG_ARRAY_FIELD(mpg_cooling_arrays, entropy, 1, ARR_IN | ARR_OUT | ARR_OPTIONAL),
    MPG_ARRAY_FIELD(mpg_cooling_arrays, ne, 1, ARR_IN | ARR_OUT | ARR_OPTIONAL),
    MPG_ARRAY_FIELD(mpg_cooling_arrays, sfr, 1, ARR_IN | ARR_OUT | ARR_OPTIONAL),
    MPG_ARRAY_FIELD(mpg_cooling_arrays, metallicity, 1, ARR_IN | ARR_OPTIONAL),
    MPG_ARRAY_FIELD(mpg_cooling_arrays, heiii_ionized, 1, ARR_IN | ARR_OPTIONAL),
    MPG_ARRAY_FIELD(mpg_cooling_arrays, tb_hydro, 1, ARR_IN | ARR_OPTIONAL),
};
static_assert(describes_every_member<mpg_cooling_arrays>(COOL_FIELDS), "COOL_FIELDS follows mpg_cooling_arrays");

// the stellar mass and metal return.  `mass` is the table's column in both host forms (P.Mass of the records), `hsml` and `density` are
// resident columns on a resident gas run; everything else travels.
constexpr ArrayField METAL_FIELDS[] = {
    MPG_ARRAY_FIELD(mpg_metal_arrays, massgenerated, 1, ARR_IN),
    MPG_ARRAY_FIELD(mpg_metal_arrays, metalgenerated, 1, ARR_IN),
    MPG_ARRAY_FIELD(mpg_metal_arrays, speciesgenerated, 9, ARR_IN),
    MPG_ARRAY_FIELD(mpg_metal_arrays, stellarage, 1, ARR_IN),
    MPG_ARRAY_FIELD(mpg_metal_arrays, mass, 1, ARR_TABLE),
    MPG_ARRAY_FIELD(mpg_metal_arrays, hsml, 1, ARR_IN | ARR_OUT | ARR_RES_ALIAS),
    MPG_ARRAY_FIELD(mpg_metal_arrays, totalmassreturned, 1, ARR_IN | ARR_OUT),
    MPG_ARRAY_FIELD(mpg_metal_arrays, lastenrichment, 1, ARR_IN | ARR_OUT),
    MPG_ARRAY_FIELD(mpg_metal_arrays, density, 1, ARR_IN | ARR_OUT | ARR_RES_ALIAS),
    MPG_ARRAY_FIELD(mpg_metal_arrays, metallicity, 1, ARR_IN | ARR_OUT),
    MPG_ARRAY_FIELD(mpg_metal_arrays, metals, 9, ARR_IN | ARR_OUT),
    MPG_ARRAY_FIELD(mpg_metal_arrays, massreturned, 1, ARR_OUT | ARR_OPTIONAL),
    MPG_ARRAY_FIELD(mpg_metal_arrays, starvolume, 1, ARR_OUT | ARR_OPTIONAL),
};
static_assert(describes_every_member<mpg_metal_arrays>(METAL_FIELDS), "METAL_FIELDS follows mpg_metal_arrays");

// the black-hole call.  `mass` is the table's column in both host forms; on a resident gas run the SPH columns and the table's Vel /
// accelerations are resident too; everything else travels.
constexpr ArrayField BH_FIELDS[] = {
    MPG_ARRAY_FIELD(mpg_blackhole_arrays, id, 1, ARR_IN),
    MPG_ARRAY_FIELD(mpg_blackhole_arrays, gacc, 3, ARR_IN | ARR_RES_ALIAS),
    MPG_ARRAY_FIELD(mpg_blackhole_arrays, gpm, 3, ARR_IN | ARR_RES_ALIAS),
    MPG_ARRAY_FIELD(mpg_blackhole_arrays, hydroacc, 3, ARR_IN | ARR_RES_ALIAS),
    MPG_ARRAY_FIELD(mpg_blackhole_arrays, tb_hydro, 1, ARR_IN | ARR_RES_ALIAS),
    MPG_ARRAY_FIELD(mpg_blackhole_arrays, tb_grav, 1, ARR_IN | ARR_RES_ALIAS),
    MPG_ARRAY_FIELD(mpg_blackhole_arrays, hsml, 1, ARR_IN | ARR_RES_ALIAS),
    MPG_ARRAY_FIELD(mpg_blackhole_arrays, density, 1, ARR_IN | ARR_RES_ALIAS),
    MPG_ARRAY_FIELD(mpg_blackhole_arrays, delaytime, 1, ARR_IN),
    MPG_ARRAY_FIELD(mpg_blackhole_arrays, dfaccel, 3, ARR_IN),
    MPG_ARRAY_FIELD(mpg_blackhole_arrays, vdisp, 1, ARR_IN),
    MPG_ARRAY_FIELD(mpg_blackhole_arrays, active_hydro, 1, ARR_IN | ARR_OPTIONAL),
    MPG_ARRAY_FIELD(mpg_blackhole_arrays, mass, 1, ARR_TABLE),
    MPG_ARRAY_FIELD(mpg_blackhole_arrays, vel, 3, ARR_IN | ARR_OUT | ARR_RES_ALIAS),
    MPG_ARRAY_FIELD(mpg_blackhole_arrays, entropy, 1, ARR_IN | ARR_OUT | ARR_RES_ALIAS),
    MPG_ARRAY_FIELD(mpg_blackhole_arrays, flags, 1, ARR_IN | ARR_OUT),
    MPG_ARRAY_FIELD(mpg_blackhole_arrays, bh_mass, 1, ARR_IN | ARR_OUT),
    MPG_ARRAY_FIELD(mpg_blackhole_arrays, mtrack, 1, ARR_IN | ARR_OUT),
    MPG_ARRAY_FIELD(mpg_blackhole_arrays, kineticfdbkenergy, 1, ARR_IN | ARR_OUT),
    MPG_ARRAY_FIELD(mpg_blackhole_arrays, countprogs, 1, ARR_IN | ARR_OUT),
    MPG_ARRAY_FIELD(mpg_blackhole_arrays, mdot, 1, ARR_OUT),
    MPG_ARRAY_FIELD(mpg_blackhole_arrays, dragaccel, 3, ARR_OUT),
    MPG_ARRAY_FIELD(mpg_blackhole_arrays, encounter, 1, ARR_OUT),
    MPG_ARRAY_FIELD(mpg_blackhole_arrays, mintimebin, 1, ARR_OUT),
    MPG_ARRAY_FIELD(mpg_blackhole_arrays, swallowid, 1, ARR_OUT),
    MPG_ARRAY_FIELD(mpg_blackhole_arrays, swallowtime, 1, ARR_OUT),
    MPG_ARRAY_FIELD(mpg_blackhole_arrays, bhheated, 1, ARR_OUT),
    MPG_ARRAY_FIELD(mpg_blackhole_arrays, feedbackweightsum, 1, ARR_OUT | ARR_OPTIONAL),
    MPG_ARRAY_FIELD(mpg_blackhole_arrays, bh_entropy, 1, ARR_OUT | ARR_OPTIONAL),
    MPG_ARRAY_FIELD(mpg_blackhole_arrays, gasvel, 3, ARR_OUT | ARR_OPTIONAL),
    MPG_ARRAY_FIELD(mpg_blackhole_arrays, mgasenc, 1, ARR_OUT | ARR_OPTIONAL),
    MPG_ARRAY_FIELD(mpg_blackhole_arrays, keflag, 1, ARR_OUT | ARR_OPTIONAL),
    MPG_ARRAY_FIELD(mpg_blackhole_arrays, accreted_mass, 1, ARR_OUT | ARR_OPTIONAL),
    MPG_ARRAY_FIELD(mpg_blackhole_arrays, accreted_bhmass, 1, ARR_OUT | ARR_OPTIONAL),
    MPG_ARRAY_FIELD(mpg_blackhole_arrays, accreted_momentum, 3, ARR_OUT | ARR_OPTIONAL),
    MPG_ARRAY_FIELD(mpg_blackhole_arrays, sph_swallowid, 1, ARR_OUT | ARR_OPTIONAL),
    MPG_ARRAY_FIELD(mpg_blackhole_arrays, bh_swallowid, 1, ARR_OUT | ARR_OPTIONAL),
};
static_assert(describes_every_member<mpg_blackhole_arrays>(BH_FIELDS), "BH_FIELDS follows mpg_blackhole_arrays");

// the dynamical-friction call (ARR_OPTIONAL here: not read by every method, checked by the call itself).  On a resident gas run the
// table's Vel / accelerations / Potential and the SPH columns are resident; the per-black-hole members travel.
constexpr ArrayField DF_FIELDS[] = {
    MPG_ARRAY_FIELD(mpg_bh_dynfric_arrays, vel, 3, ARR_IN | ARR_RES_ALIAS),
    MPG_ARRAY_FIELD(mpg_bh_dynfric_arrays, gacc, 3, ARR_IN | ARR_OPTIONAL | ARR_RES_ALIAS),
    MPG_ARRAY_FIELD(mpg_bh_dynfric_arrays, gpm, 3, ARR_IN | ARR_OPTIONAL | ARR_RES_ALIAS),
    MPG_ARRAY_FIELD(mpg_bh_dynfric_arrays, hydroacc, 3, ARR_IN | ARR_OPTIONAL | ARR_RES_ALIAS),
    MPG_ARRAY_FIELD(mpg_bh_dynfric_arrays, tb_grav, 1, ARR_IN | ARR_OPTIONAL | ARR_RES_ALIAS),
    MPG_ARRAY_FIELD(mpg_bh_dynfric_arrays, tb_hydro, 1, ARR_IN | ARR_OPTIONAL | ARR_RES_ALIAS),
    MPG_ARRAY_FIELD(mpg_bh_dynfric_arrays, hsml, 1, ARR_IN | ARR_RES_ALIAS),
    MPG_ARRAY_FIELD(mpg_bh_dynfric_arrays, potential, 1, ARR_IN | ARR_RES_ALIAS),
    MPG_ARRAY_FIELD(mpg_bh_dynfric_arrays, bh_mass, 1, ARR_IN | ARR_OPTIONAL),
    MPG_ARRAY_FIELD(mpg_bh_dynfric_arrays, active_dynfric, 1, ARR_IN | ARR_OPTIONAL),
    MPG_ARRAY_FIELD(mpg_bh_dynfric_arrays, df_density, 1, ARR_IN | ARR_OUT | ARR_OPTIONAL),
    MPG_ARRAY_FIELD(mpg_bh_dynfric_arrays, df_vel, 3, ARR_IN | ARR_OUT | ARR_OPTIONAL),
    MPG_ARRAY_FIELD(mpg_bh_dynfric_arrays, df_rmsvel, 1, ARR_IN | ARR_OUT | ARR_OPTIONAL),
    MPG_ARRAY_FIELD(mpg_bh_dynfric_arrays, jumptominpot, 1, ARR_IN | ARR_OUT),
    MPG_ARRAY_FIELD(mpg_bh_dynfric_arrays, minpot, 1, ARR_OUT),
    MPG_ARRAY_FIELD(mpg_bh_dynfric_arrays, minpotpos, 3, ARR_OUT),
    MPG_ARRAY_FIELD(mpg_bh_dynfric_arrays, minpotvel, 3, ARR_OUT),
    MPG_ARRAY_FIELD(mpg_bh_dynfric_arrays, dfaccel, 3, ARR_OUT | ARR_OPTIONAL),
};
static_assert(describes_every_member<mpg_bh_dynfric_arrays>(DF_FIELDS), "DF_FIELDS follows mpg_bh_dynfric_arrays");

// winds_and_feedback.  tb_hydro is winds_evolve's alone and does not travel.
constexpr ArrayField WD_FIELDS[] = {
    MPG_ARRAY_FIELD(mpg_wind_arrays, id, 1, ARR_IN),
    MPG_ARRAY_FIELD(mpg_wind_arrays, hsml, 1, ARR_IN),
    MPG_ARRAY_FIELD(mpg_wind_arrays, vdisp, 1, ARR_IN),
    MPG_ARRAY_FIELD(mpg_wind_arrays, density, 1, ARR_IN),
    MPG_ARRAY_FIELD(mpg_wind_arrays, tb_hydro, 1, ARR_OTHER_CALL),
    MPG_ARRAY_FIELD(mpg_wind_arrays, vel, 3, ARR_IN | ARR_OUT),
    MPG_ARRAY_FIELD(mpg_wind_arrays, entropy, 1, ARR_IN | ARR_OUT),
    MPG_ARRAY_FIELD(mpg_wind_arrays, delaytime, 1, ARR_IN | ARR_OUT),
    MPG_ARRAY_FIELD(mpg_wind_arrays, totalweight, 1, ARR_OUT | ARR_OPTIONAL),
    MPG_ARRAY_FIELD(mpg_wind_arrays, kick_star, 1, ARR_OUT | ARR_OPTIONAL),
};
static_assert(describes_every_member<mpg_wind_arrays>(WD_FIELDS), "WD_FIELDS follows mpg_wind_arrays");

// cooling_and_starformation.  Density, Entropy, TimeBinHydro, Hsml, DivVel and CurlVel are resident columns on a resident gas run (the host
// copies are stale inside a stretch); everything else travels.
// (ARR_OPTIONAL where a criterion or the wind model decides: the call checks what it reads itself.)
constexpr ArrayField SFR_FIELDS[] = {
    MPG_ARRAY_FIELD(mpg_sfr_columns, id, 1, ARR_IN),
    MPG_ARRAY_FIELD(mpg_sfr_columns, generation, 1, ARR_IN | ARR_OPTIONAL),
    MPG_ARRAY_FIELD(mpg_sfr_columns, density, 1, ARR_IN | ARR_RES_ALIAS),
    MPG_ARRAY_FIELD(mpg_sfr_columns, hsml, 1, ARR_IN | ARR_OPTIONAL | ARR_RES_ALIAS),
    MPG_ARRAY_FIELD(mpg_sfr_columns, divvel, 1, ARR_IN | ARR_OPTIONAL | ARR_RES_ALIAS),
    MPG_ARRAY_FIELD(mpg_sfr_columns, curlvel, 1, ARR_IN | ARR_OPTIONAL | ARR_RES_ALIAS),
    MPG_ARRAY_FIELD(mpg_sfr_columns, gradrho_mag, 1, ARR_IN | ARR_OPTIONAL),
    MPG_ARRAY_FIELD(mpg_sfr_columns, tb_hydro, 1, ARR_IN | ARR_OPTIONAL | ARR_RES_ALIAS),
    MPG_ARRAY_FIELD(mpg_sfr_columns, heiii_ionized, 1, ARR_IN | ARR_OPTIONAL),
    MPG_ARRAY_FIELD(mpg_sfr_columns, vdisp, 1, ARR_IN | ARR_OPTIONAL),
    MPG_ARRAY_FIELD(mpg_sfr_columns, entropy, 1, ARR_IN | ARR_OUT | ARR_RES_ALIAS),
    MPG_ARRAY_FIELD(mpg_sfr_columns, ne, 1, ARR_IN | ARR_OUT),
    MPG_ARRAY_FIELD(mpg_sfr_columns, sfr, 1, ARR_IN | ARR_OUT),
    MPG_ARRAY_FIELD(mpg_sfr_columns, metallicity, 1, ARR_IN | ARR_OUT),
    MPG_ARRAY_FIELD(mpg_sfr_columns, delaytime, 1, ARR_IN | ARR_OUT | ARR_OPTIONAL),
    MPG_ARRAY_FIELD(mpg_sfr_columns, bhheated, 1, ARR_IN | ARR_OUT | ARR_OPTIONAL),
    MPG_ARRAY_FIELD(mpg_sfr_columns, vel, 3, ARR_IN | ARR_OUT | ARR_OPTIONAL),
    MPG_ARRAY_FIELD(mpg_sfr_columns, stellarmass, 1, ARR_OUT | ARR_OPTIONAL),
};
static_assert(describes_every_member<mpg_sfr_columns>(SFR_FIELDS), "SFR_FIELDS follows mpg_sfr_columns");

// calculate_uvbg: the halo mass goes up in escfrac and comes back converted; zreion is in / out; sfr is read with ReionUseParticleSFR (the call
// checks it)
constexpr ArrayField UVBG_FIELDS[] = {
    MPG_ARRAY_FIELD(mpg_uvbg_columns, sfr, 1, ARR_IN | ARR_OPTIONAL),
    MPG_ARRAY_FIELD(mpg_uvbg_columns, escfrac, 1, ARR_IN | ARR_OUT),
    MPG_ARRAY_FIELD(mpg_uvbg_columns, local_J21, 1, ARR_OUT),
    MPG_ARRAY_FIELD(mpg_uvbg_columns, zreion, 1, ARR_IN | ARR_OUT),
};
static_assert(describes_every_member<mpg_uvbg_columns>(UVBG_FIELDS), "UVBG_FIELDS follows mpg_uvbg_columns");

// Room for n particles of field F in its staging buffer and, when the host array `h` is given, its n entries on the way up (queued on
// st): the device pointer.  (512 bytes of slack: 64 spare elements of the widest type, and never an empty allocation.)
inline void *stage_field(const ArrayField &F, mpg::DevBuf<char> &buf, const void *h, int64_t n, hipStream_t st)
{
    const size_t bytes = (size_t)n * F.elem * F.width;
    buf.reserve(bytes + 512);
    if(h)
        MPG_HIP(hipMemcpyAsync(buf.p, h, bytes, hipMemcpyHostToDevice, st));
    return buf.p;
}
// The host arrays of `host` onto the device (bufs[f], one buffer per field) and `dev` filled with the device pointers; fields with a
// role in `skip` are left to the caller (dev keeps what it holds there).  A required array that is missing is an error in `who`'s name.
template <class S, size_t N>
inline void stage_fields(const ArrayField (&T)[N], const S &host, S &dev, mpg::DevBuf<char> *bufs, int64_t n, unsigned skip, const char *who,
                         hipStream_t st)
{
    for(size_t f = 0; f < N; f++) {
        const ArrayField &F = T[f];
        if(F.role & skip)
            continue;
        const void *h = field_get(host, F.off);
        MPG_CHECK(h || (F.role & ARR_OPTIONAL), std::string(who) + ": the array " + F.name + " is required");
        // (the outputs go up too: the call writes the entries of its targets only, the others come back as they were)
        field_set(dev, F.off, h ? stage_field(F, bufs[f], h, n, st) : nullptr);
    }
}
// ... and what the call wrote back into them (queued on st)
template <class S, size_t N> inline void unstage_fields(const ArrayField (&T)[N], const S &host, const S &dev, int64_t n, unsigned skip, hipStream_t st)
{
    for(const ArrayField &F : T) {
        void *h = field_get(host, F.off);
        if(h && (F.role & ARR_OUT) && !(F.role & skip))
            MPG_HIP(hipMemcpyAsync(h, field_get(dev, F.off), (size_t)n * F.elem * F.width, hipMemcpyDeviceToHost, st));
    }
}
// the flags byte of the records: IsGarbage and Swallowed as the call left them (`flags`: n host bytes)
inline void flags_to_records(const mpg_particle_view &V, const uint8_t *flags)
{
    const HostTable T(V);
    parallel_for(V.n, [=](int64_t lo, int64_t hi) {
        for(int64_t i = lo; i < hi; i++) {
            uint8_t *b = (uint8_t *)(T.rec(i) + T.V.off_flags);
            *b = (uint8_t)((*b & ~3) | (flags[i] & 3));
        }
    });
}
// the table's Mass column from the device into the records (`pinned`: n floats of pinned staging)
inline void mass_to_records(const mpg_particle_view &V, const float *d_mass, float *pinned, hipStream_t st)
{
    const int64_t n = V.n;
    if(n == 0)
        return;
    MPG_HIP(hipMemcpyAsync(pinned, d_mass, (size_t)n * sizeof(float), hipMemcpyDeviceToHost, st));
    MPG_HIP(hipStreamSynchronize(st));
    const HostTable T(V);
    parallel_for(n, [=](int64_t lo, int64_t hi) {
        for(int64_t i = lo; i < hi; i++)
            *(float *)(T.rec(i) + T.V.off_mass) = pinned[i];
    });
}
