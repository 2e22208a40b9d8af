// engine_internal.h -- the engine object behind the C-ABI handle (include/mpgadget_hip.h), shared by engine.hip, physics.hip, integrator.hip,
// host_forms.hip, resident.hip and the multi-rank layer (dist_internal.h, dist*.hip)
#pragma once
#include "../../include/mpgadget_hip.h"
#include "grav_walk.h"
#include "mpg_common.h"
#include "pm.h"
#include "sph.h"
#include "veldisp.h"
#include "cooling.h"
#include "sfr.h"
#include "metals.h"
#include "winds.h"
#include "heiii.h"
#include "blackhole.h"
#include "dynfric.h"
#include "timestep.h"
#include "peano.h"
#include "planes.h"
#include "domain.h"
#include "fof.h"
#include "fof_catalogue.h"
#include "uvbg.h"
#include "snapshot_io.h"
#include "tree_build.h"
#include "host_table.h"
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <string>
#include <thread>
#include <vector>

using namespace mpg;

std::string &mpg_err_slot(); // thread-local text of the last error (mpg_last_error)

struct mpg_engine {
    int device = 0;
    hipStream_t stream = nullptr;
    bool own_stream = false;
    // the tree build of a step has no data dependence on the step's PM force (both read the bound positions): when a PM
    // force has just been queued, force_tree_build runs on this second stream next to it (engine-internal; MPG_NO_TREE_OVERLAP=1
    // keeps everything on one stream)
    hipStream_t aux_stream = nullptr;
    hipEvent_t ev_inputs = nullptr, ev_tree_done = nullptr, ev_pad_done = nullptr;
    bool pad_pending = false; // the leaf blocks of the current tree were queued on aux_stream behind ev_tree_done (ev_pad_done)
    bool pm_queued = false;
    // module state (static variables of gravshort-tree.c:30-32, gravity.c:20, forcetree.c:30-37)
    mpg_gravshort_tree_params treepar{0.002, 0.175, 0.9, 2, 6.0, 1.0 / 30.};
    double GravitySoftening = 0;
    double TreeAllocFactor = 0.9;
    bool have_tab = false;
    double tab_dx = 0.02935420743639786;
    DevBuf<float> tab_force, tab_pot;
    // subsystems
    PMesh pm;
    TreeBuilder tree;
    bool tree_allocated = false;
    bool full_particle_tree = false;
    int tree_mask = 63;
    EventTimer timer;
    bool count = false;
    int walk_thresh = 16;
    // 1: lane-per-target while-while kernel (grav_walk.hip); 4: group-cooperative list kernel (grav_walk_coop.hip); 6: two-kernel walk
    // (grav_walk_split.hip); 0: 6 for large target sets, 1 for small ones
    int walk_variant = 0;
    int walk_choice = 0; // the kernel the default policy used last (0: no walk yet)
    int walks_since_tune = 0;
    WalkScratch w3;
    DevBuf<unsigned long long> counters;
    int64_t last_targets = 0;
    float *d_walk_cost = nullptr; // per-target work of the walks, caller order (mpg_dev_set_walk_cost; null: not recorded)
    // un-synchronised HIP event pairs around every walk launch (collected by mpg_walk_events_collect)
    std::vector<std::pair<hipEvent_t, hipEvent_t>> walk_events, free_events;
    // ... and, per walk, the event between the two kernels of a one-slice two-kernel walk (null otherwise)
    std::vector<hipEvent_t> walk_mid, free_mid;
    // SPH module state (static variables of density.c:20, hydra.c:26-34)
    mpg_density_params denspar{1.0, 2.0, 2.0, 99999., 2 /* quintic */, 0.006};
    mpg_hydro_params hydropar{1, 100.0, 0.75};
    SphEngine sph;
    // bound device particles (caller order)
    int64_t n = 0;
    const double *d_pos = nullptr;
    const float *d_mass = nullptr;
    const uint8_t *d_type = nullptr;
    double box = 0;
    DevBuf<double> w_old; // OldAcc of a walk that writes over its own opening input (mpg_dev_grav_short_tree)
    DevBuf<unsigned> ts_flag;
    DevBuf<uint8_t> tree_incl; // particles included in an active-particle tree
    // hierarchical gravity (timestep.c:239-599): active sublists (ping-pong), the per-level acceleration array, scratch
    DevBuf<int> hier_list[2], hier_val;
    DevBuf<uint8_t> hier_keep;
    DevBuf<double> hier_accel, hier_sp;
    DevBuf<unsigned long long> hier_cnt;
    DevBuf<char> hier_tmp;
    PeanoScratch peano;
    DomainScratch domain;
    FofEngine fof;
    CatalogueEngine cat; // the group catalogue on disk (fof_catalogue.hip): the order, the staging pair, the times of the last call
    PlaneEngine planes;
    VdispEngine vdisp; // DM velocity dispersion (veldisp.c): the loop's state
    // ---- everything below is the host-pointer ("drop-in") layer's: host_forms.hip and resident.hip (the engine only destroys it) ----
    // staging for the host SPH path: one device buffer per mpg_sph_arrays field
    DevBuf<double> h_sph[19];
    DevBuf<uint8_t> h_sph_u8[2];
    // staging for the host (AoS) path
    DevBuf<double> s_pos, s_accel, s_gravpm, s_pot, s_prev, s_old;
    DevBuf<float> s_mass;
    DevBuf<uint8_t> s_type, s_live;
    const uint8_t *pm_live = nullptr; // host path: 0 for garbage / swallowed particles when the staged table holds any (else null)
    DevBuf<int> s_active;
    DevBuf<uint8_t> plane_flags; // host forms of the potential planes: IsGarbage / Swallowed of the table ...
    HostBuf<uint8_t> h_plane_flags; // ... staged through a pinned buffer of their own (h_b holds the live flags of the staged epoch)
    DevBuf<double> plane_out;
    HostBuf<double> h_d, h_d2, h_d3; // pinned staging: positions / 3-vectors, scalars
    HostBuf<float> h_f;
    HostBuf<uint8_t> h_b;
    // host path: what is staged (mpg_set_particle_epoch) and the events of the chunked downloads
    int64_t host_epoch = 0, staged_epoch = 0, staged_n = -1;
    const void *staged_base = nullptr;
    // device-resident drop-in mode (mpg_resident_begin): the table at res_base lives in s_pos / s_mass / s_type and r_*; the host calls on
    // that table move no particle data
    bool resident = false, res_has_vel = false;
    const void *res_base = nullptr;
    int64_t res_n = -1;
    DevBuf<double> r_vel, r_accel, r_gravpm, r_pot;
    // ... and a gas run's SPH arrays (mpg_resident_sph_begin): the host set they were taken from, their device copies (h_sph / h_sph_u8,
    // with vel / gacc / gpm aliasing r_vel / r_accel / r_gravpm) and the garbage flags of the resident table for the integrator kernels
    bool sph_resident = false;
    mpg_sph_arrays res_sph_host{}, res_sph_dev{};
    DevBuf<uint8_t> r_flags;
    // ... and the device copy of the caller's StoredGravAccel of a resident split-gravity step (mpg_resident_hierarchical_*): the host array it
    // stands for (nullptr: none held), written back into it by mpg_resident_end
    DevBuf<double> r_stored;
    double (*r_stored_host)[3] = nullptr;
    double staged_box = 0;
    hipEvent_t chunk_ev[8] = {};
    // Host path with overlap (mpg_set_host_overlap): within one particle-table epoch Pos / Mass / Type, Potential AND the
    // previous FullTreeGravAccel go up in ONE pass over the records (the walk then takes OldAcc on the device from the uploaded
    // acceleration and the device's GravPM: no second host pass), and the results of gravpm_force travel down and into P[] on a copy
    // stream and a host thread while the tree build and the walk run.  host_join() waits for that thread.
    bool host_overlap = false;
    int host_slices = 0;
    hipStream_t copy_stream = nullptr;
    hipEvent_t ev_pm_done = nullptr, ev_acc_up = nullptr, gchunk_ev[8] = {};
    std::thread unpack_thread;
    std::string unpack_error;
    HostBuf<double> h_acc, h_gpm, h_gpot;
    DevBuf<double> s_prevacc, s_pot2, s_acc_t, s_pot_t; // ... the walk's results compacted in tree order, slice by slice
    HostBuf<double> h_acc_t, h_pot_t;
    HostBuf<int> h_order;
    hipEvent_t slice_ev[9] = {};
    int64_t staged_extra_epoch = -1; // the epoch whose Potential / FullTreeGravAccel are staged (s_pot, s_prevacc)
    int64_t gravpm_epoch = -1;       // the epoch whose GravPM sits in s_gravpm
    // mpg_host_prefetch (round 6): the epoch's packing pass + uploads on a host thread of their own, started by the caller as soon as P[] is
    // final for the step (the end of drift_all_particles) and joined by the first entry point that needs the staged columns
    std::thread prefetch_thread;
    std::string prefetch_error;
    mpg_particle_view prefetch_view{};
    // the staging of the velocity dispersion's host form (fields of mpg_veldisp_arrays)
    DevBuf<char> vd_stage[std::size(VDISP_FIELDS)];
    // radiative cooling (cooling.hip): parameters, tables and counters; the staging of its host forms (fields of mpg_cooling_arrays)
    CoolingEngine cooling;
    DevBuf<char> cl_stage[std::size(COOL_FIELDS)];
    // stellar mass and metal return (metals.hip): parameters and the loop's state; the staging of its host forms (fields of mpg_metal_arrays)
    mpg_metal_params metalpar{1, 2.0, 0.0};
    MetalsEngine metals;
    DevBuf<char> mt_stage[std::size(METAL_FIELDS)];
    HostBuf<float> mt_mass;
    // black-hole accretion, mergers and feedback (blackhole.hip): parameters, the walks' state and the random table; the staging of its
    // host forms (fields of mpg_blackhole_arrays)
    mpg_blackhole_params bhpar{};
    bool have_bhpar = false;
    BlackholeEngine bh;
    DevBuf<char> bh_stage[std::size(BH_FIELDS)];
    HostBuf<float> bh_mass;
    // black-hole dynamical friction and the potential minimum (dynfric.hip): parameters, the walk's state; the staging of its host forms
    mpg_bh_dynfric_params dfpar{};
    bool have_dfpar = false;
    DynfricEngine df;
    DevBuf<char> df_stage[std::size(DF_FIELDS)];
    // the wind model (winds.hip): parameters, the walks' state (the random table is the black holes'); the staging of its host form
    mpg_wind_params windpar{};
    bool have_windpar = false;
    WindsEngine winds;
    DevBuf<char> wd_stage[std::size(WD_FIELDS)];
    // ... and SphP.DelayTime for hydro_force's decoupling (WIND_DECOUPLE_SPH): the device column in effect (mpg_dev_set_delaytime, or
    // s_delaytime after mpg_resident_sph_set_delaytime), the host column mpg_hydro_force uploads per call (mpg_set_delaytime) into
    // s_delaytime_call
    const double *d_delaytime = nullptr;
    const double *h_delaytime = nullptr;
    DevBuf<double> s_delaytime, s_delaytime_call;
    // helium reionisation by quasar bubbles (heiii.hip): parameters, the host's random table, the loop's state; the staging of its host forms
    HeiiiEngine heiii;
    DevBuf<double> he_density, he_entropy;
    DevBuf<uint8_t> he_flag;
    // star formation (sfr.hip): parameters, the lists and counters of the last call; the staging of its host forms (fields of mpg_sfr_columns)
    SfrEngine sfr;
    DevBuf<char> sf_stage[std::size(SFR_FIELDS)];
    // excursion-set reionisation (uvbg.hip): meshes, plans and the float grids of the last call; the staging of its host form
    UvbgEngine uvbg;
    DevBuf<char> uv_stage[std::size(UVBG_FIELDS)];
    void prefetch_join()
    {
        if(prefetch_thread.joinable())
            prefetch_thread.join();
    }
    void host_join()
    {
        if(unpack_thread.joinable())
            unpack_thread.join();
        prefetch_join();
    }
};

extern "C" void engine_tree_build_on(mpg_engine *eng, int mask, hipStream_t st); // engine.hip
extern "C" void wait_for_leaf_blocks(mpg_engine *eng, hipStream_t st);            // engine.hip
// host_forms.hip, also used by resident.hip: Pos / Mass / Type of the table onto the device and bound (or, resident / same epoch: checked);
// the host arrays of the SPH forms staged, `dev` filled with their device copies; the planes of a staged or resident table
void stage_particles(mpg_engine *eng, const mpg_particle_view *P, double BoxSize);
void stage_sph(mpg_engine *eng, const mpg_sph_arrays *host, mpg_sph_arrays *dev, int64_t n);
// physics.hip, also used by host_forms.hip and resident.hip: the black-hole call on device arrays; when the call has a target, build == 1 builds
// the tree of gas and black holes with hmax (from A->hsml) if the current tree is not one, build == 2 builds it in any case
// ... and its queue pass alone: the number of targets the call would have (the host forms stage their arrays only when there is one)
extern "C" int64_t blackhole_targets(mpg_engine *eng, const int *d_active, int64_t nactive);
extern "C" void blackhole_call(mpg_engine *eng, const mpg_blackhole_arrays *A, const mpg_sph_times *T, const int *d_active, int64_t nactive, int build);
// ... the same of the dynamical-friction call: its queue pass without the dynfric bins (returns the number of listed black holes, 0 when
// the parameters switch the call off: then nothing would be read or written) and the call on device arrays, which builds the tree of its
// mask when it has a target
extern "C" int64_t dynfric_listed(mpg_engine *eng, const int *d_active, int64_t nactive);
extern "C" void dynfric_call(mpg_engine *eng, const mpg_bh_dynfric_arrays *A, const mpg_sph_times *T, const int *d_active, int64_t nactive);
// ... and the helium reionisation call on device particle columns with the groups wherever `groups` finds them (physics.hip)
extern "C" void heiii_call(mpg_engine *eng, const mpg_heiii_step *step, const double *d_density, double *d_entropy, uint8_t *d_flag, const HeiiiGroups &groups,
                mpg_heiii_result *result);
// ... the groups from HOST columns (host_forms.hip)
HeiiiGroups heiii_host_groups(const double *mass, const double *cm, const uint64_t *minid, int64_t ngroups);
void host_planes(mpg_engine *eng, const mpg_particle_view *P, const mpg_plane_params *par, double *planes, int64_t *npart);

// potential planes (planes.hip).  red: the sums over the ranks of the several-GPU form (dist_gravity.hip), or null; sum_device returns with the
// device array summed and usable on the engine's stream
struct PlaneReduce {
    void *ctx;
    int nt;
    void (*sum_device)(void *ctx, int64_t *d_v, int64_t count);
    void (*sum_host)(void *ctx, int64_t *v, int64_t count);
    void (*max_host)(void *ctx, int64_t *v, int64_t count);
};
void planes_run(mpg_engine *eng, const mpg_plane_params *par, const uint8_t *d_flags, double *d_planes, int64_t *npart, const PlaneReduce *red);

// the error word of a kernel, read back (synchronises the engine's stream)
inline unsigned read_flag(mpg_engine *eng, unsigned *d)
{
    unsigned e = 0;
    MPG_HIP(hipMemcpyAsync(&e, d, sizeof(e), hipMemcpyDeviceToHost, eng->stream));
    MPG_HIP(hipStreamSynchronize(eng->stream));
    return e;
}
// ... and its round trip: the word zeroed, launch(word), read back; a kernel that raised it fails the call with `message`
template <class Launch> inline void flagged_launch(mpg_engine *eng, const char *message, Launch &&launch)
{
    eng->ts_flag.reserve(4);
    MPG_HIP(hipMemsetAsync(eng->ts_flag.p, 0, sizeof(unsigned), eng->stream));
    launch(eng->ts_flag.p);
    MPG_CHECK(read_flag(eng, eng->ts_flag.p) == 0, message);
}

#define API_BEGIN try {
#define API_END_NORETURN             \
    }                                \
    catch(const std::exception &e) { \
        mpg_err_slot() = e.what();   \
        return 1;                    \
    }
#define API_END                      \
    }                                \
    catch(const std::exception &e) { \
        mpg_err_slot() = e.what();   \
        return 1;                    \
    }                                \
    mpg_err_slot().clear();          \
    return 0;

