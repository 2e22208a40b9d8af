// engine.hip -- C-ABI (include/mpgadget_hip.h) and host-side orchestration of the gfx950 TreePM engine.
//
// Host side mirrors the reference's call sequence: gravpm_force (gravpm.c:61-119), force_tree_full
// (forcetree.c:110-128), grav_short_tree (gravshort-tree.c:96-154) with fill / reduce / postprocess of
// gravshort.h:47-96.  Every entry point catches mpg::Error and returns non-zero (the reference has no
// return codes here; the in-tree shim maps failures to endrun()).  There is no CPU fallback anywhere:
// without a HIP device mpg_engine_create fails.  The entry points of the gas and subgrid physics are physics.hip's, the time integration
// is integrator.hip's, the host-pointer forms are host_forms.hip's and resident.hip's.
#include "engine_internal.h"
#include <cstdio>

static thread_local std::string g_err;
std::string &mpg_err_slot() { return g_err; }

extern "C" {

const char *mpg_last_error(void) { return g_err.c_str(); }
const char *mpg_version(void) { return "mpgadget_hip 0.1 (gfx950; TreePM gravity: PM + tree + short-range walk)"; }

int mpg_engine_create(mpg_engine **out, int device)
{
    API_BEGIN
    MPG_CHECK(out != nullptr, "mpg_engine_create: null output pointer");
    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if(e != hipSuccess || ndev <= 0)
        fail(__FILE__, __LINE__, "mpg_engine_create: no HIP device available (this engine has no CPU path)");
    MPG_CHECK(device >= 0 && device < ndev, "mpg_engine_create: bad device index");
    MPG_HIP(hipSetDevice(device));
    mpg_engine *eng = new mpg_engine();
    eng->device = device;
    MPG_HIP(hipStreamCreateWithFlags(&eng->stream, hipStreamNonBlocking));
    eng->own_stream = true;
    eng->counters.reserve(16);
    *out = eng;
    API_END
}

void mpg_engine_destroy(mpg_engine *eng)
{
    if(!eng)
        return;
    (void)hipSetDevice(eng->device);
    (void)hipStreamSynchronize(eng->stream);
    if(eng->w3.split_stream)
        (void)hipStreamSynchronize(eng->w3.split_stream);
    for(auto &v : {&eng->walk_events, &eng->free_events})
        for(auto &e : *v) {
            (void)hipEventDestroy(e.first);
            (void)hipEventDestroy(e.second);
        }
    for(auto &v : {&eng->walk_mid, &eng->free_mid})
        for(auto &e : *v)
            if(e)
                (void)hipEventDestroy(e);
    eng->host_join();
    for(auto &e : eng->chunk_ev)
        if(e)
            (void)hipEventDestroy(e);
    for(auto &e : eng->gchunk_ev)
        if(e)
            (void)hipEventDestroy(e);
    if(eng->ev_pm_done)
        (void)hipEventDestroy(eng->ev_pm_done);
    if(eng->ev_acc_up)
        (void)hipEventDestroy(eng->ev_acc_up);
    for(auto &e : eng->slice_ev)
        if(e)
            (void)hipEventDestroy(e);
    if(eng->copy_stream) {
        (void)hipStreamSynchronize(eng->copy_stream);
        (void)hipStreamDestroy(eng->copy_stream);
    }
    eng->pm.destroy();
    if(eng->aux_stream) {
        (void)hipStreamSynchronize(eng->aux_stream);
        (void)hipStreamDestroy(eng->aux_stream);
        (void)hipEventDestroy(eng->ev_inputs);
        (void)hipEventDestroy(eng->ev_tree_done);
        if(eng->ev_pad_done)
            (void)hipEventDestroy(eng->ev_pad_done);
    }
    if(eng->own_stream && eng->stream)
        (void)hipStreamDestroy(eng->stream);
    delete eng;
}

int mpg_engine_set_stream(mpg_engine *eng, void *hip_stream)
{
    API_BEGIN
    MPG_CHECK(eng, "null engine");
    if(eng->own_stream && eng->stream) {
        MPG_HIP(hipStreamSynchronize(eng->stream));
        MPG_HIP(hipStreamDestroy(eng->stream));
    }
    if(hip_stream) {
        eng->stream = (hipStream_t)hip_stream;
        eng->own_stream = false;
    }
    else {
        MPG_HIP(hipStreamCreateWithFlags(&eng->stream, hipStreamNonBlocking));
        eng->own_stream = true;
    }
    API_END
}

void *mpg_engine_get_stream(mpg_engine *eng) { return eng ? (void *)eng->stream : nullptr; }

int mpg_engine_synchronize(mpg_engine *eng)
{
    API_BEGIN
    MPG_CHECK(eng, "null engine");
    MPG_HIP(hipSetDevice(eng->device));
    MPG_HIP(hipStreamSynchronize(eng->stream));
    MPG_CHECK(walk_coop_error(eng->w3, eng->stream) == 0, "short-range walk aborted by its loop guard (corrupt tree?)");
    API_END
}

int mpg_set_gravshort_treepar(mpg_engine *eng, const mpg_gravshort_tree_params *par)
{
    API_BEGIN
    MPG_CHECK(eng && par, "null argument");
    eng->treepar = *par;
    API_END
}

int mpg_get_gravshort_treepar(mpg_engine *eng, mpg_gravshort_tree_params *par)
{
    API_BEGIN
    MPG_CHECK(eng && par, "null argument");
    *par = eng->treepar;
    API_END
}

int mpg_gravshort_set_softenings(mpg_engine *eng, double MeanSeparation)
{
    API_BEGIN
    MPG_CHECK(eng, "null engine");
    eng->GravitySoftening = eng->treepar.FractionalGravitySoftening * MeanSeparation; // gravshort-tree.c:47
    API_END
}

double mpg_force_softening(mpg_engine *eng) { return eng ? 2.8 * eng->GravitySoftening : 0.0; } // gravshort-tree.c:37-41

int mpg_gravshort_fill_ntab(mpg_engine *eng, int window_type, double Asmth, const double *table, int nrows)
{
    API_BEGIN
    MPG_CHECK(eng && table, "null argument");
    MPG_CHECK(nrows == NTAB, "gravshort_fill_ntab: the short-range table must have 512 rows");
    MPG_CHECK(window_type == 0 || window_type == 1, "gravshort_fill_ntab: unknown ShortRangeForceWindowType");
    if(window_type == 0 && Asmth != 1.5) // gravity.c:25-29
        fail(__FILE__, __LINE__, "The short range force window is calibrated for Asmth = 1.5, but running with " + std::to_string(Asmth));
    std::vector<float> f(NTAB), p(NTAB);
    for(int i = 0; i < NTAB; i++) {
        const double u = table[5 * i + 0] * 0.5 / Asmth;
        if(window_type == 0) {
            f[i] = (float)table[5 * i + 2];
            p[i] = (float)table[5 * i + 1];
        }
        else {
            f[i] = (float)(erfc(u) + 2.0 * u / sqrt(M_PI) * exp(-u * u));
            p[i] = (float)erfc(u);
        }
    }
    eng->tab_dx = table[5 * 1 + 0];
    eng->tab_force.reserve(NTAB);
    eng->tab_pot.reserve(NTAB);
    MPG_HIP(hipSetDevice(eng->device));
    MPG_HIP(hipMemcpy(eng->tab_force.p, f.data(), NTAB * sizeof(float), hipMemcpyHostToDevice));
    MPG_HIP(hipMemcpy(eng->tab_pot.p, p.data(), NTAB * sizeof(float), hipMemcpyHostToDevice));
    eng->have_tab = true;
    API_END
}

int mpg_gravpm_init_periodic(mpg_engine *eng, double BoxSize, double Asmth, int Nmesh, double G)
{
    API_BEGIN
    if(eng)
        eng->pm.kspace_force = getenv("MPG_PM_KSPACE_FORCE") != nullptr;
    MPG_CHECK(eng, "null engine");
    MPG_HIP(hipSetDevice(eng->device));
    eng->pm.init(BoxSize, Asmth, Nmesh, G, eng->stream);
    API_END
}

int mpg_petapm_destroy(mpg_engine *eng)
{
    API_BEGIN
    MPG_CHECK(eng, "null engine");
    MPG_HIP(hipSetDevice(eng->device));
    eng->pm.destroy();
    API_END
}

int mpg_init_forcetree_params(mpg_engine *eng, double TreeAllocFactor)
{
    API_BEGIN
    MPG_CHECK(eng, "null engine");
    eng->TreeAllocFactor = TreeAllocFactor;
    API_END
}

void mpg_particle_view_reference_layout(mpg_particle_view *v, void *P, int64_t NumPart)
{
    // struct particle_data, partmanager.h:9-71 (160 bytes; offsets as measured in SURVEY 8(a))
    v->base = P;
    v->n = NumPart;
    v->stride = 160;
    v->off_pos = 0;
    v->off_mass = 28;
    v->off_pi = 32;
    v->off_flags = 36;
    v->off_type = 39;
    v->off_vel = 40;
    v->off_accel = 64;
    v->off_gravpm = 88;
    v->off_hsml = 120;
    v->off_potential = 152;
}

/* ------------------------------ device-resident path ------------------------------ */

int mpg_dev_bind_particles(mpg_engine *eng, int64_t n, const double *d_pos, const float *d_mass, const uint8_t *d_type, double BoxSize)
{
    API_BEGIN
    MPG_CHECK(eng, "null engine");
    MPG_CHECK(n >= 0 && (n == 0 || (d_pos && d_mass)), "mpg_dev_bind_particles: null particle arrays");
    MPG_CHECK(BoxSize > 0, "mpg_dev_bind_particles: BoxSize must be positive");
    eng->host_join(); // (a prefetch or a write-back of the host-pointer calls still uses the binding and the stream)
    eng->n = n;
    eng->fof.cat_n = -1; // (a group catalogue belongs to the particles it was made of: mpg_dev_fof_subgrid asks for a new one)
    eng->d_pos = d_pos;
    eng->d_mass = d_mass;
    eng->d_type = d_type;
    eng->box = BoxSize;
    eng->pm_queued = false; // a tree build that follows sees new arrays: it stays behind everything on the main stream
    API_END
}

int mpg_dev_gravpm_force(mpg_engine *eng, double *d_gravpm, double *d_potential)
{
    API_BEGIN
    MPG_CHECK(eng && d_gravpm, "null argument");
    MPG_HIP(hipSetDevice(eng->device));
    MPG_CHECK(eng->pm.nmesh > 0, "gravpm_force called before gravpm_init_periodic");
    MPG_CHECK(eng->pm.box == eng->box, "gravpm_force: BoxSize of the mesh differs from the bound particles");
    static const bool no_overlap = getenv("MPG_NO_TREE_OVERLAP") != nullptr;
    if(!no_overlap && !eng->timer.enabled) {
        if(!eng->aux_stream) {
            MPG_HIP(hipStreamCreateWithFlags(&eng->aux_stream, hipStreamNonBlocking));
            MPG_HIP(hipEventCreateWithFlags(&eng->ev_inputs, hipEventDisableTiming));
            MPG_HIP(hipEventCreateWithFlags(&eng->ev_tree_done, hipEventDisableTiming));
            MPG_HIP(hipEventCreateWithFlags(&eng->ev_pad_done, hipEventDisableTiming));
        }
        MPG_HIP(hipEventRecord(eng->ev_inputs, eng->stream)); // everything queued so far: the particle arrays are final, the last walk is done
        eng->pm_queued = true;
    }
    MPG_CHECK(!eng->pm.hybrid_tracer || eng->d_type || eng->n == 0, "gravpm_force: the hybrid-neutrino deposit mask needs d_type in mpg_dev_bind_particles");
    const float *dep_mass = eng->pm.tracer_mass(eng->n, eng->d_mass, eng->d_type, eng->stream);
    eng->pm.force(eng->n, eng->d_pos, dep_mass, nullptr, d_gravpm, d_potential, eng->stream, &eng->timer);
    API_END
}

int mpg_dev_tree_top_partial(mpg_engine *eng, int La, int64_t n_own, double *d_out)
{
    API_BEGIN
    MPG_CHECK(eng && d_out, "null argument");
    MPG_CHECK(eng->tree_allocated, "no tree");
    MPG_HIP(hipSetDevice(eng->device));
    eng->tree.top_partial(La, n_own, d_out, eng->stream);
    API_END
}

int mpg_dev_tree_top_set(mpg_engine *eng, int La, const double *d_sums)
{
    API_BEGIN
    MPG_CHECK(eng && d_sums, "null argument");
    MPG_CHECK(eng->tree_allocated, "no tree");
    MPG_HIP(hipSetDevice(eng->device));
    eng->tree.top_set(La, d_sums, eng->stream);
    API_END
}

int mpg_dev_pm_slab_init(mpg_engine *eng, int rank, int world, int64_t *cplx_per_peer, int64_t *plane_doubles)
{
    API_BEGIN
    MPG_CHECK(eng, "null engine");
    MPG_HIP(hipSetDevice(eng->device));
    eng->pm.slab_init(rank, world);
    if(cplx_per_peer)
        *cplx_per_peer = (int64_t)eng->pm.slab_cplx_per_peer();
    if(plane_doubles)
        *plane_doubles = (int64_t)eng->pm.nmesh * eng->pm.nmesh;
    API_END
}

int mpg_dev_pm_slab_forward_a(mpg_engine *eng, double *sendA)
{
    API_BEGIN
    MPG_CHECK(eng && sendA, "null argument");
    MPG_HIP(hipSetDevice(eng->device));
    MPG_CHECK(eng->pm.box == eng->box, "gravpm_force: BoxSize of the mesh differs from the bound particles");
    eng->pm.slab_forward_a(eng->n, eng->d_pos, eng->d_mass, sendA, eng->stream);
    API_END
}

int mpg_dev_pm_slab_forward_b(mpg_engine *eng, double *recvA, double *sendB)
{
    API_BEGIN
    MPG_CHECK(eng && recvA && sendB, "null argument");
    MPG_HIP(hipSetDevice(eng->device));
    MPG_CHECK(!eng->pm.nu_fn, "mpg_dev_pm_slab_forward_b: the neutrino response needs the bins of all ranks between the two halves (use mpg_dist)");
    eng->pm.slab_forward_b(recvA, sendB, eng->stream);
    API_END
}

int mpg_dev_pm_slab_inverse_c(mpg_engine *eng, const double *recvB, double *ghost_send)
{
    API_BEGIN
    MPG_CHECK(eng && recvB && ghost_send, "null argument");
    MPG_HIP(hipSetDevice(eng->device));
    eng->pm.slab_inverse_c(recvB, ghost_send, eng->stream);
    API_END
}

int mpg_dev_pm_slab_readout(mpg_engine *eng, const double *ghost_recv, const int *d_targets, int64_t ntargets, double *d_gravpm,
                            double *d_potential)
{
    API_BEGIN
    MPG_CHECK(eng && ghost_recv && d_gravpm && (d_targets || ntargets == 0), "null argument");
    MPG_HIP(hipSetDevice(eng->device));
    eng->pm.slab_readout(ghost_recv, d_targets, ntargets, eng->d_pos, d_gravpm, d_potential, eng->stream);
    API_END
}

// tree of the bound particles + moments on the given stream (csrc/dist_gravity.hip: beside the PM step, from a second host thread)
// What the default walk kernels read beside the depth-first tree - the level-ordered copy and the leaves' particles in blocks of 8 - made
// with the tree, on the tree's stream (beside the PM force when one is queued), not at the start of the walk (rounds 1-5: 0.5 ms of every
// walk at 256^3).  Not when the phases are being timed (the tree's phases are its own) or another kernel was selected.
static bool tree_walk_copies(mpg_engine *eng, hipStream_t st, bool leaf_blocks = true)
{
    if(eng->timer.enabled || !(eng->walk_variant == 0 || eng->walk_variant == 6) || eng->tree.npart < 4096)
        return false;
    eng->tree.ensure_level_order(st);
    if(leaf_blocks)
        eng->tree.ensure_leaf_pad(st);
    return true;
}

// a tree build on `st` overwrites what a leaf-block kernel still running on the tree stream reads
void wait_for_leaf_blocks(mpg_engine *eng, hipStream_t st)
{
    if(eng->pad_pending && st != eng->aux_stream)
        MPG_HIP(hipStreamWaitEvent(st, eng->ev_pad_done, 0));
    eng->pad_pending = false;
}

void engine_tree_build_on(mpg_engine *eng, int mask, hipStream_t st)
{
    eng->pm_queued = false;
    wait_for_leaf_blocks(eng, st);
    eng->tree.build(eng->n, eng->d_pos, eng->d_mass, eng->d_type, mask, eng->box, st, nullptr);
    eng->tree.calc_moments(nullptr, st, nullptr);
    tree_walk_copies(eng, st);
    eng->tree_allocated = true;
    eng->tree_mask = mask;
    eng->full_particle_tree = (eng->tree.npart == eng->n);
}

int mpg_dev_force_tree_build(mpg_engine *eng, int mask)
{
    API_BEGIN
    MPG_CHECK(eng, "null engine");
    MPG_HIP(hipSetDevice(eng->device));
    if(eng->pm_queued && !eng->timer.enabled) {
        // next to the PM force queued on the main stream; whatever is queued on the main stream after this call waits for the tree
        eng->pm_queued = false;
        eng->pad_pending = false; // (a leaf-block kernel of the last tree runs on this same stream: ordered)
        MPG_HIP(hipStreamWaitEvent(eng->aux_stream, eng->ev_inputs, 0));
        eng->tree.build(eng->n, eng->d_pos, eng->d_mass, eng->d_type, mask, eng->box, eng->aux_stream, nullptr);
        eng->tree.calc_moments(nullptr, eng->aux_stream, nullptr);
        const bool copies = tree_walk_copies(eng, eng->aux_stream, false);
        MPG_HIP(hipEventRecord(eng->ev_tree_done, eng->aux_stream));
        MPG_HIP(hipStreamWaitEvent(eng->stream, eng->ev_tree_done, 0));
        if(copies) { // the leaf blocks are read by the walk's SECOND kernel only: made behind the event, beside the list kernel
            eng->tree.ensure_leaf_pad(eng->aux_stream);
            MPG_HIP(hipEventRecord(eng->ev_pad_done, eng->aux_stream));
            eng->pad_pending = true;
        }
    }
    else {
        eng->pm_queued = false;
        wait_for_leaf_blocks(eng, eng->stream);
        eng->tree.build(eng->n, eng->d_pos, eng->d_mass, eng->d_type, mask, eng->box, eng->stream, &eng->timer);
        eng->tree.calc_moments(nullptr, eng->stream, &eng->timer);
        tree_walk_copies(eng, eng->stream);
    }
    if(eng->timer.enabled)
        eng->timer.t.tree_total = eng->timer.t.tree_keys + eng->timer.t.tree_sort + eng->timer.t.tree_nodes + eng->timer.t.tree_moments;
    eng->tree_allocated = true;
    eng->tree_mask = mask;
    // full_particle_tree_flag (forcetree.c:127,164-165): all particle types are in the tree
    eng->full_particle_tree = (eng->tree.npart == eng->n);
    API_END
}

int mpg_dev_force_tree_rebuild_mask(mpg_engine *eng, int mask, int with_moments)
{
    API_BEGIN
    MPG_CHECK(eng, "null engine");
    MPG_HIP(hipSetDevice(eng->device));
    wait_for_leaf_blocks(eng, eng->stream);
    eng->tree.build(eng->n, eng->d_pos, eng->d_mass, eng->d_type, mask, eng->box, eng->stream, &eng->timer);
    if(with_moments)
        eng->tree.calc_moments(nullptr, eng->stream, &eng->timer);
    eng->tree_allocated = true;
    eng->tree_mask = mask;
    eng->full_particle_tree = (mask == 63) || (eng->tree.npart == eng->n);
    eng->sph.hmax_pending = false;
    API_END
}

__global__ void __launch_bounds__(256) k_mark_included(int64_t nact, const int *__restrict__ active, uint8_t *__restrict__ flags)
{
    const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if(k < nact)
        flags[active[k]] = 1;
}

int mpg_dev_force_tree_active_moments(mpg_engine *eng, const int *d_active, int64_t nactive, int HybridNuTracer)
{
    API_BEGIN
    MPG_CHECK(eng && (d_active || nactive == 0), "null argument");
    MPG_HIP(hipSetDevice(eng->device));
    const int mask = HybridNuTracer ? (1 + 2 + 16 + 32) : 63; // GASMASK + DMMASK + STARMASK + BHMASK, or ALLMASK (forcetree.c:139-141)
    const uint8_t *incl = nullptr;
    if(d_active) {
        eng->tree_incl.reserve((size_t)eng->n + 1);
        MPG_HIP(hipMemsetAsync(eng->tree_incl.p, 0, (size_t)eng->n, eng->stream));
        if(nactive > 0)
            hipLaunchKernelGGL(k_mark_included, dim3((unsigned)((nactive + 255) / 256)), dim3(256), 0, eng->stream, nactive, d_active,
                               eng->tree_incl.p);
        incl = eng->tree_incl.p;
    }
    wait_for_leaf_blocks(eng, eng->stream);
    eng->tree.build(eng->n, eng->d_pos, eng->d_mass, eng->d_type, mask, eng->box, eng->stream, &eng->timer, incl);
    eng->tree.calc_moments(nullptr, eng->stream, &eng->timer);
    eng->tree_allocated = true;
    eng->tree_mask = mask;
    eng->full_particle_tree = !d_active && eng->tree.npart == eng->n; // forcetree.c:146-147
    eng->sph.hmax_pending = false;
    API_END
}

int mpg_dev_force_tree_calc_hmax(mpg_engine *eng)
{
    API_BEGIN
    MPG_CHECK(eng && eng->tree_allocated, "force_tree_calc_moments: no tree");
    MPG_HIP(hipSetDevice(eng->device));
    eng->sph.calc_hmax(eng->tree, eng->stream);
    API_END
}

int mpg_dev_force_update_hmax(mpg_engine *eng, const double *d_hsml)
{
    API_BEGIN
    MPG_CHECK(eng && d_hsml && eng->tree_allocated, "force_update_hmax: no tree or no Hsml");
    MPG_HIP(hipSetDevice(eng->device));
    SphView v{};
    v.type = eng->d_type;
    v.hsml = const_cast<double *>(d_hsml);
    eng->sph.hsml_view = v;
    eng->sph.hmax_pending = true;
    eng->sph.calc_hmax(eng->tree, eng->stream);
    API_END
}

int mpg_dev_force_tree_set_min_leaf_level(mpg_engine *eng, int level)
{
    API_BEGIN
    MPG_CHECK(eng && level >= 0 && level <= 8, "mpg_dev_force_tree_set_min_leaf_level: level must be in [0, 8]");
    eng->tree.force_internal_above = level;
    API_END
}

static GravParams make_gp(mpg_engine *eng, double rho0)
{
    GravParams gp{};
    MPG_CHECK(eng->pm.nmesh > 0, "grav_short_tree needs gravpm_init_periodic first (cell size, Asmth, G)");
    MPG_CHECK(eng->have_tab, "grav_short_tree called before gravshort_fill_ntab");
    const double cellsize = eng->tree.box / eng->pm.nmesh;   // gravshort-tree.c:101
    gp.box = eng->tree.box;
    gp.invbox = 1.0 / gp.box;
    gp.rcut = eng->treepar.Rcut * eng->pm.Asmth * cellsize;  // :102
    gp.rcut2 = gp.rcut * gp.rcut;
    gp.h = 2.8 * eng->GravitySoftening;
    MPG_CHECK(gp.h > 0, "grav_short_tree called before gravshort_set_softenings");
    gp.hinv = 1.0 / gp.h;
    gp.h3inv = 1.0 / gp.h / gp.h / gp.h;
    gp.h2 = gp.h * gp.h;
    gp.inv_cell_dx = 1.0 / (cellsize * eng->tab_dx);
    gp.errtol = eng->treepar.ErrTolForceAcc;
    gp.use_bh = eng->treepar.TreeUseBH != 0;
    // gravshort-tree.c:266-270
    gp.bhangle2 = eng->treepar.BHOpeningAngle * eng->treepar.BHOpeningAngle;
    if(eng->treepar.TreeUseBH == 0)
        gp.bhangle2 = eng->treepar.MaxBHOpeningAngle * eng->treepar.MaxBHOpeningAngle;
    gp.G = eng->pm.G;
    gp.cbrtrho0 = pow(rho0, 1.0 / 3);
    gp.full_tree = eng->full_particle_tree ? 1 : 0;
    return gp;
}

int mpg_dev_set_walk_cost(mpg_engine *eng, float *d_cost)
{
    API_BEGIN
    MPG_CHECK(eng, "null engine");
    eng->d_walk_cost = d_cost;
    API_END
}

// OldAcc = |FullTreeGravAccel + GravPM| / G of every particle (grav_get_abs_accel, gravshort.h:70-80), the arithmetic of the walk kernels
// (rows: the targets of the walk, or all n when the list is NULL - only the targets' rows of prev / gravpm are read: under mpg_dist the
// engine is bound to own + ghost rows while the caller's arrays hold the own rows only)
__global__ void __launch_bounds__(256) k_oldacc(int64_t n, const int *__restrict__ list, const double *__restrict__ prev,
                                                const double *__restrict__ gravpm, double G, double *__restrict__ old)
{
    const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if(k >= n)
        return;
    const int64_t i = list ? (int64_t)list[k] : k;
    double s2 = 0;
    for(int j = 0; j < 3; j++) {
        const double a = prev[3 * i + j] + (gravpm ? gravpm[3 * i + j] : 0.0);
        s2 += a * a;
    }
    old[i] = sqrt(s2) / G;
}

int mpg_dev_grav_short_tree(mpg_engine *eng, const double *d_oldacc, const double *d_prev_accel, const double *d_gravpm,
                            const int *d_active, int64_t nactive, double *d_accel, double *d_potential, double rho0)
{
    API_BEGIN
    MPG_CHECK(eng && d_accel, "null argument");
    MPG_HIP(hipSetDevice(eng->device));
    MPG_CHECK(eng->tree_allocated && eng->tree.has_moments, "Gravtree called before tree moments computed!"); // gravshort-tree.c:113-114
    const GravParams gp = make_gp(eng, rho0);
    if(!d_oldacc && d_prev_accel && d_prev_accel == d_accel) {
        // Results written in place over the previous acceleration (resident mode, mpg_dist callers): the two-kernel walk may run its
        // list pass a second time with longer lists after the evaluation has stored new values for the targets that fitted, and the
        // fallback kernels run after it, so the opening input is taken once, before any kernel of this walk writes.
        // Taken for the walk's TARGETS only: with an active list the caller's arrays need not hold eng->n rows (mpg_dist binds the engine
        // to own + ghost particles and passes arrays of the own rows; its targets are own rows).
        const int64_t nrows = d_active ? nactive : eng->n;
        eng->w_old.reserve((size_t)eng->n + 1);
        if(nrows > 0)
            hipLaunchKernelGGL(k_oldacc, dim3((unsigned)((nrows + 255) / 256)), dim3(256), 0, eng->stream, nrows, d_active, d_prev_accel, d_gravpm,
                               gp.G, eng->w_old.p);
        d_oldacc = eng->w_old.p;
        d_prev_accel = nullptr;
    }
    WalkIO io;
    io.targets = d_active;
    if(d_active)
        io.ntargets = nactive;
    else {
        // ActiveParticle == NULL: all particles (timestep.c:77-84).  When the tree holds them all, walk in tree order.
        // (a tree of all types holds every LIVE particle: the garbage / swallowed records it leaves out are skipped by the reference's
        // queue as well, treewalk.c:92-96,234)
        MPG_CHECK(eng->tree.npart == eng->n || eng->full_particle_tree, "grav_short_tree with ActiveParticle == NULL needs a tree of all particles "
                                                                         "(pass the active list for masked trees)");
        io.ntargets = eng->tree.npart;
    }
    io.pos = eng->d_pos;
    io.mass = eng->d_mass;
    io.oldacc = d_oldacc;
    io.prev_accel = d_prev_accel;
    io.gravpm = d_gravpm;
    io.accel = d_accel;
    io.potential = eng->full_particle_tree ? d_potential : nullptr;
    io.tab_force = eng->tab_force.p;
    io.tab_pot = eng->tab_pot.p;
    io.counters = eng->counters.p;
    io.cost = eng->d_walk_cost;
    {
        static const int lp = getenv("MPG_LIST_PRIO") ? atoi(getenv("MPG_LIST_PRIO")) : 0, ep = getenv("MPG_EVAL_PRIO") ? atoi(getenv("MPG_EVAL_PRIO")) : 0;
        io.list_prio = lp;
        io.eval_prio = ep;
    }
    if(eng->count)
        MPG_HIP(hipMemsetAsync(eng->counters.p, 0, 16 * sizeof(unsigned long long), eng->stream));
    eng->timer.start(eng->stream);
    std::pair<hipEvent_t, hipEvent_t> ev{nullptr, nullptr};
    if(!eng->free_events.empty()) {
        ev = eng->free_events.back();
        eng->free_events.pop_back();
    }
    else {
        MPG_HIP(hipEventCreate(&ev.first));
        MPG_HIP(hipEventCreate(&ev.second));
    }
    MPG_HIP(hipEventRecord(ev.first, eng->stream));
    hipEvent_t mid = nullptr;
    if(!eng->free_mid.empty()) {
        mid = eng->free_mid.back();
        eng->free_mid.pop_back();
    }
    else
        MPG_HIP(hipEventCreate(&mid));
    eng->w3.ev_mid = mid;
    eng->w3.mid_recorded = false;
    //  a walk that throws - a loop guard, an overflow - must not leave w3.ev_mid pointing at an event nobody owns, nor
    // lose the three events: the guard hands them back unless the normal path below has filed them
    struct EventGuard {
        mpg_engine *e;
        std::pair<hipEvent_t, hipEvent_t> *ev;
        hipEvent_t *mid;
        bool filed = false;
        ~EventGuard()
        {
            if(filed)
                return;
            e->w3.ev_mid = nullptr;
            e->w3.mid_recorded = false;
            e->free_events.push_back(*ev);
            e->free_mid.push_back(*mid);
        }
    } ev_guard{eng, &ev, &mid};
    // hoisting the minimum-image wrap out of the pair loop is valid when every source range shares the image of its
    // node: Rcut + 1.5 * (largest leaf side) < Box/2, and Rcut well below Box/4 (see grav_walk_coop.hip)
    const double maxleaf = 1.001 * gp.box / (double)(1 << eng->tree.minleaflevel);
    const bool fastwrap = !getenv("MPG_NO_FASTWRAP") && (gp.rcut + 1.5 * maxleaf < 0.49 * gp.box) && (gp.rcut < 0.2 * gp.box);
    auto run_variant_io = [&](int v, const WalkIO &w) {
        if(v != 1)
            eng->tree.ensure_level_order(eng->stream); // variants 4 and 6 walk the level-ordered copy of the tree
        if(v == 6) {
            eng->tree.ensure_leaf_pad(eng->stream);    // ... and 6 the leaves' particles in blocks of 8 (both made with the tree as a rule)
            eng->w3.ev_before_eval = eng->pad_pending ? eng->ev_pad_done : nullptr;
        }
        if(v == 1)
            launch_grav_walk(eng->tree.view(), gp, w, w.potential != nullptr, eng->count, fastwrap, eng->walk_thresh, eng->stream);
        else if(v == 6)
            launch_grav_walk_split(eng->tree.view(), gp, w, w.potential != nullptr, eng->count, fastwrap, eng->w3, eng->stream);
        else
            launch_grav_walk_coop(eng->tree.view(), gp, w, w.potential != nullptr, eng->count, fastwrap, eng->w3, eng->stream);
    };
    auto run_variant = [&](int v) { run_variant_io(v, io); };
    int variant = eng->walk_variant;
    if(variant == 0) {
        // Default: the two-kernel walk (6) with the cooperative kernel (4) for the targets whose lists overflow; the lane-per-target
        // kernel (1) for small target sets (fewer than 4096), where launch count matters more than lane use.  (This used to be decided by timing
        // kernels 1, 4 and 6 on the first walk and every 64th.  On the measured sets - grid, Zel'dovich, clustered, 96^3 .. 256^3 -
        // kernel 6 now always wins, and the trial itself is unaffordable on clustered sets: 6.7 s for kernel 1 and 2 s for kernel 4
        // against 0.18 s for kernel 6 at 256^3; timing a sample of the targets instead misjudges kernel 6, whose fixed costs -
        // slices, two streams, the control-word read-back - weigh on a small sample.)
        // (round 3, with k_walk_lists8: 32 768 active targets of a 256^3 tree take 1.09 ms with kernel 6 against 4.6 ms with kernel 1;
        // the threshold was 65 536 when the list kernels needed that many targets to fill the chip)
        static const int64_t split_min = getenv("MPG_SPLIT_MIN_TARGETS") ? atoll(getenv("MPG_SPLIT_MIN_TARGETS")) : 4096;
        variant = io.ntargets >= split_min ? 6 : 1;
        eng->walk_choice = variant;
        eng->walks_since_tune++;
    }
    if(variant > 0)
        run_variant(variant);
    MPG_HIP(hipEventRecord(ev.second, eng->stream));
    ev_guard.filed = true;
    eng->walk_events.push_back(ev);
    eng->w3.ev_mid = nullptr;
    if(eng->w3.mid_recorded)
        eng->walk_mid.push_back(mid);
    else {
        eng->walk_mid.push_back(nullptr);
        eng->free_mid.push_back(mid);
    }
    if(eng->walk_events.size() > 4096) { // nobody is collecting: recycle the oldest
        eng->free_events.push_back(eng->walk_events.front());
        eng->walk_events.erase(eng->walk_events.begin());
        if(eng->walk_mid.front())
            eng->free_mid.push_back(eng->walk_mid.front());
        eng->walk_mid.erase(eng->walk_mid.begin());
    }
    eng->timer.lap(eng->stream, &eng->timer.t.walk);
    eng->timer.t.walk_launches = 1;
    eng->last_targets = io.ntargets;
    // TreeUseBH > 1: Barnes-Hut on the first walk only (gravshort-tree.c:148-151)
    if(eng->treepar.TreeUseBH > 1)
        eng->treepar.TreeUseBH = 0;
    API_END
}

int mpg_dev_grav_short_pair(mpg_engine *eng, const int *d_active, int64_t nactive, double Rcut, double *d_accel, double *d_potential, double rho0)
{
    API_BEGIN
    MPG_CHECK(eng && d_accel, "null argument");
    MPG_HIP(hipSetDevice(eng->device));
    MPG_CHECK(eng->tree_allocated, "grav_short_pair: no tree");
    const GravParams gp = make_gp(eng, rho0);
    WalkIO io;
    io.targets = d_active;
    if(d_active)
        io.ntargets = nactive;
    else {
        MPG_CHECK(eng->tree.npart == eng->n, "grav_short_pair with ActiveParticle == NULL needs a tree of all particles");
        io.ntargets = eng->tree.npart;
    }
    io.pos = eng->d_pos;
    io.mass = eng->d_mass;
    io.accel = d_accel;
    io.potential = eng->full_particle_tree ? d_potential : nullptr;
    io.tab_force = eng->tab_force.p;
    io.tab_pot = eng->tab_pot.p;
    eng->tree.ensure_level_order(eng->stream);
    const double rcut_abs = Rcut * eng->pm.Asmth * (eng->tree.box / eng->pm.nmesh); // gravshort-pair.c:27-28
    flagged_launch(eng, "grav_short_pair: neighbour-search stack overflow", [&](unsigned *err) {
        launch_grav_short_pair(eng->tree.view(), gp, io, rcut_abs, io.potential != nullptr, err, eng->stream);
    });
    API_END
}

int mpg_dev_peano_keys(mpg_engine *eng, int64_t n, const double *d_pos, double BoxSize, uint64_t *d_keys)
{
    API_BEGIN
    MPG_CHECK(eng && n >= 0 && (n == 0 || (d_pos && d_keys)) && BoxSize > 0, "peano_keys: bad argument");
    MPG_HIP(hipSetDevice(eng->device));
    launch_peano_keys(n, d_pos, BoxSize, d_keys, eng->stream);
    API_END
}

int mpg_dev_order_by_type_and_key(mpg_engine *eng, int64_t n, const unsigned char *d_type, const unsigned char *d_flags,
                                  const uint64_t *d_keys, int *d_perm, int64_t *n_live)
{
    API_BEGIN
    MPG_CHECK(eng && n >= 0 && n < ((int64_t)1 << 31) && (n == 0 || (d_keys && d_perm)) && n_live, "order_by_type_and_key: bad argument");
    MPG_HIP(hipSetDevice(eng->device));
    *n_live = order_by_type_and_key(n, d_type, d_flags, d_keys, d_perm, eng->peano, eng->stream);
    API_END
}

// ---- Peano-Hilbert domain decomposition (domain.hip) ------------------------------------------------------------------------
static_assert(sizeof(mpg_topnode) == sizeof(TopNode) && offsetof(mpg_topnode, Count) == offsetof(TopNode, Count), "mpg_topnode layout");

int mpg_dev_domain_sample(mpg_engine *eng, int64_t n, const double *d_pos, const unsigned char *d_garbage, double BoxSize, int PreSort,
                          int SubSampleDistance, uint64_t *keys_out, int64_t cap, int64_t *nsample)
{
    API_BEGIN
    MPG_CHECK(eng && n >= 0 && (n == 0 || d_pos) && BoxSize > 0 && keys_out && nsample, "domain_sample: bad argument");
    MPG_HIP(hipSetDevice(eng->device));
    *nsample = domain_sample(n, d_pos, d_garbage, BoxSize, PreSort, SubSampleDistance, keys_out, cap, eng->domain, eng->stream);
    API_END
}

int mpg_domain_local_refine(const uint64_t *keys, const int64_t *costs, int64_t nsample, mpg_topnode *tree, int *size, int MaxTopNodes, int *failed)
{
    API_BEGIN
    MPG_CHECK((keys || nsample == 0) && nsample >= 0 && tree && size && failed, "domain_local_refine: bad argument");
    *failed = toptree_local_refine(keys, costs, nsample, (TopNode *)tree, size, MaxTopNodes) ? 0 : 1;
    API_END
}

int mpg_domain_toptree_truncate(mpg_topnode *tree, int *size, int64_t countlimit, int64_t costlimit)
{
    API_BEGIN
    MPG_CHECK(tree && size && *size >= 1, "domain_toptree_truncate: bad argument");
    toptree_truncate((TopNode *)tree, size, countlimit, costlimit);
    API_END
}

int mpg_domain_toptree_merge(mpg_topnode *A, int *sizeA, const mpg_topnode *B, int sizeB, int MaxTopNodes, int *failed)
{
    API_BEGIN
    MPG_CHECK(A && sizeA && *sizeA >= 1 && (B || sizeB == 0) && sizeB >= 0 && failed, "domain_toptree_merge: bad argument");
    *failed = toptree_merge((TopNode *)A, sizeA, (const TopNode *)B, sizeB, MaxTopNodes) ? 0 : 1;
    API_END
}

int mpg_domain_global_refine(mpg_topnode *tree, int *size, int MaxTopNodes, int64_t countlimit, int64_t costlimit, int *failed)
{
    API_BEGIN
    MPG_CHECK(tree && size && *size >= 1 && failed, "domain_global_refine: bad argument");
    *failed = toptree_global_refine((TopNode *)tree, size, MaxTopNodes, countlimit, costlimit) ? 0 : 1;
    API_END
}

int mpg_domain_create_topleaves(mpg_topnode *tree, int size, int *leaf_topnode, int *nleaves)
{
    API_BEGIN
    MPG_CHECK(tree && size >= 1 && leaf_topnode && nleaves, "domain_create_topleaves: bad argument");
    *nleaves = toptree_create_leaves((TopNode *)tree, size, leaf_topnode);
    API_END
}

int mpg_domain_assign_topleaves_balanced(mpg_topnode *tree, int size, int *leaf_topnode, int nleaves, const int64_t *cost, int NTask,
                                         int NsegmentPerTask, int *leaf_task, int *StartLeaf, int *EndLeaf)
{
    API_BEGIN
    MPG_CHECK(tree && size >= 1 && leaf_topnode && nleaves >= 1 && cost && NTask >= 1 && NsegmentPerTask >= 1 && leaf_task && StartLeaf && EndLeaf,
              "domain_assign_topleaves_balanced: bad argument");
    toptree_assign_balanced((TopNode *)tree, size, leaf_topnode, nleaves, cost, NTask, NsegmentPerTask, leaf_task, StartLeaf, EndLeaf);
    API_END
}

int mpg_dev_domain_topleaves(mpg_engine *eng, int64_t n, const double *d_pos, const unsigned char *d_garbage, double BoxSize,
                             const mpg_topnode *tree, int size, int nleaves, const int *leaf_task, int NTask, int32_t *d_topleaf,
                             int32_t *d_task, int64_t *leaf_counts, int64_t *task_counts)
{
    API_BEGIN
    MPG_CHECK(eng && n >= 0 && (n == 0 || d_pos) && BoxSize > 0 && tree && NTask >= 1, "domain_topleaves: bad argument");
    MPG_HIP(hipSetDevice(eng->device));
    domain_topleaves(n, d_pos, d_garbage, BoxSize, (const TopNode *)tree, size, nleaves, leaf_task, NTask, d_topleaf, d_task, leaf_counts,
                     task_counts, eng->domain, eng->stream);
    API_END
}

__global__ void __launch_bounds__(256) k_include_live(int64_t n, const uint8_t *__restrict__ flags, uint8_t *__restrict__ incl)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if(i < n)
        incl[i] = (flags[i] & 3) ? 0 : 1; // garbage and swallowed particles are not in the tree (forcetree.c:357-365)
}

int mpg_dev_fof_fof(mpg_engine *eng, const mpg_fof_params *par, const uint64_t *d_id, const double *d_vel, const double *d_hsml,
                    const unsigned char *d_flags, int64_t *d_grnr, int64_t *ngroups)
{
    API_BEGIN
    MPG_CHECK(eng && par && ngroups && (eng->n == 0 || d_id), "fof_fof: null argument");
    MPG_CHECK(eng->d_pos || eng->n == 0, "fof_fof: no particles bound (mpg_dev_bind_particles)");
    MPG_CHECK(par->FOFHaloComovingLinkingLength > 0 && par->FOFHaloMinLength >= 1, "fof_fof: bad parameters");
    MPG_CHECK((par->FOFPrimaryLinkTypes & par->FOFSecondaryLinkTypes) == 0, "fof_fof: primary and secondary link types must be disjoint");
    MPG_HIP(hipSetDevice(eng->device));
    // the tree of the primary linking particles, no moments (fof.c:178-180)
    const uint8_t *incl = nullptr;
    if(d_flags && eng->n > 0) {
        eng->tree_incl.reserve((size_t)eng->n + 1);
        hipLaunchKernelGGL(k_include_live, dim3((unsigned)((eng->n + 255) / 256)), dim3(256), 0, eng->stream, eng->n, d_flags, eng->tree_incl.p);
        incl = eng->tree_incl.p;
    }
    wait_for_leaf_blocks(eng, eng->stream);
    eng->tree.build(eng->n, eng->d_pos, eng->d_mass, eng->d_type, par->FOFPrimaryLinkTypes, eng->box, eng->stream, &eng->timer, incl);
    eng->tree_allocated = true;
    eng->tree_mask = par->FOFPrimaryLinkTypes;
    eng->full_particle_tree = false;
    eng->sph.hmax_pending = false;
    FofInput in;
    in.n = eng->n;
    in.pos = eng->d_pos;
    in.vel = d_vel;
    in.mass = eng->d_mass;
    in.type = eng->d_type;
    in.flags = d_flags;
    in.id = (const unsigned long long *)d_id;
    in.hsml = d_hsml;
    in.box = eng->box;
    in.LL = par->FOFHaloComovingLinkingLength;
    in.minlen = par->FOFHaloMinLength;
    in.secondary_mask = par->FOFSecondaryLinkTypes;
    *ngroups = eng->fof.run(eng->tree, in, eng->stream);
    if(d_grnr && eng->n > 0)
        MPG_HIP(hipMemcpyAsync(d_grnr, eng->fof.p_grnr.p, (size_t)eng->n * sizeof(int64_t), hipMemcpyDeviceToDevice, eng->stream));
    API_END
}

int mpg_dev_fof_groups(mpg_engine *eng, const mpg_fof_groups *out)
{
    API_BEGIN
    MPG_CHECK(eng && out, "null argument");
    MPG_HIP(hipSetDevice(eng->device));
    FofTable t;
    t.MinID = (unsigned long long *)out->MinID;
    t.Length = out->Length;
    t.GrNr = out->GrNr;
    t.LenType = out->LenType;
    t.Mass = out->Mass;
    t.MassType = out->MassType;
    t.CM = out->CM;
    t.Vel = out->Vel;
    t.Jmom = out->Jmom;
    t.Imom = out->Imom;
    t.FirstPos = out->FirstPos;
    eng->fof.export_groups(t, eng->stream);
    API_END
}

// the sub-grid half of struct Group on the groups of the last mpg_dev_fof_fof (fof.c:647-676)
int mpg_dev_fof_subgrid(mpg_engine *eng, const mpg_fof_subgrid_columns *A, const mpg_fof_subgrid_groups *out)
{
    API_BEGIN
    MPG_CHECK(eng && A, "fof_subgrid: null argument");
    MPG_CHECK(eng->fof.cat_n >= 0, "fof_subgrid: no mpg_dev_fof_fof since the particles were bound");
    MPG_CHECK(eng->fof.cat_n == eng->n, "fof_subgrid: the bound particle count differs from that of the last mpg_dev_fof_fof");
    MPG_HIP(hipSetDevice(eng->device));
    const FofSubgridIn in{A->sfr, A->metallicity, A->metals, A->heiii_ionized, A->bh_mass, A->bh_mdot, A->density, A->delaytime, A->WindDecouple};
    FofSubgridTable t{};
    if(out)
        t = FofSubgridTable{out->Sfr, out->GasMetalMass, out->StellarMetalMass, out->GasMetalElemMass, out->StellarMetalElemMass, out->MassHeIonized,
                            out->BH_Mass, out->BH_Mdot, out->MaxDens, (long long *)out->seed_index};
    eng->fof.subgrid(eng->n, eng->d_mass, eng->d_type, in, t, eng->stream);
    API_END
}

// fof_set_escapefraction (fof.c:832-870) on the groups of the last mpg_dev_fof_fof
int mpg_dev_fof_set_escapefraction(mpg_engine *eng, double *d_escfrac)
{
    API_BEGIN
    MPG_CHECK(eng && (d_escfrac || eng->n == 0), "fof_set_escapefraction: null argument");
    MPG_CHECK(eng->fof.cat_n >= 0, "fof_set_escapefraction: no mpg_dev_fof_fof since the particles were bound");
    MPG_CHECK(eng->fof.cat_n == eng->n, "fof_set_escapefraction: the bound particle count differs from that of the last mpg_dev_fof_fof");
    MPG_HIP(hipSetDevice(eng->device));
    eng->fof.set_escapefraction(eng->n, eng->d_type, d_escfrac, eng->stream);
    API_END
}

// fof_seed (fof.c:1345-1449) with blackhole_make_one (blackhole.c:1056-1111) on the caller's columns
int mpg_dev_fof_seed(mpg_engine *eng, const mpg_fof_seed_params *par, double atime, const mpg_bh_seed_columns *cols, int64_t cap,
                     int64_t *d_seed_particle, int64_t *d_seed_group, int64_t *nseeds, int64_t *nwarn)
{
    API_BEGIN
    MPG_CHECK(eng && par && nseeds && cap >= 0, "fof_seed: bad argument");
    *nseeds = 0;
    MPG_CHECK(eng->fof.cat_n >= 0 && eng->fof.cat_n == eng->n && eng->fof.sub_done,
              "fof_seed: no mpg_dev_fof_subgrid since the last mpg_dev_fof_fof on the bound particles");
    const bool powerlaw = par->MaxSeedBlackHoleMass > 0;
    if(cols && powerlaw) {
        MPG_CHECK(eng->bh.rndsize > 0, "fof_seed: MaxSeedBlackHoleMass > 0 needs the random table (mpg_set_random_table first)");
        MPG_CHECK(cols->id, "fof_seed: MaxSeedBlackHoleMass > 0 needs the id column");
    }
    MPG_HIP(hipSetDevice(eng->device));
    FofSeedPar p{};
    p.MinFoFMass = par->MinFoFMassForNewSeed;
    p.MinMStar = par->MinMStarForNewSeed;
    p.SeedMass = par->SeedBlackHoleMass;
    p.MaxSeedMass = par->MaxSeedBlackHoleMass;
    p.SeedDynMass = par->SeedBHDynMass;
    if(powerlaw) { // the constants of bh_powerlaw_seed_mass (blackhole.c:1044-1051), once per call
        const double x1 = 1 + par->SeedBlackHoleMassIndex;
        p.pl_p0 = pow(par->SeedBlackHoleMass, x1);
        p.pl_norm = pow(par->MaxSeedBlackHoleMass, x1) - p.pl_p0;
        p.pl_inv = 1. / x1;
    }
    p.atime = atime;
    p.rnd = eng->bh.rnd.p;
    p.rndsize = (uint64_t)eng->bh.rndsize;
    FofSeedCols c{};
    if(cols) {
        c.id = (const unsigned long long *)cols->id;
        c.tb_hydro = cols->tb_hydro;
        c.pos = eng->d_pos;
        c.type_in = cols->type ? cols->type : eng->d_type;
        c.mass_in = cols->mass ? cols->mass : eng->d_mass;
        c.type = cols->type;
        c.mass = cols->mass;
        c.bh_mass = cols->bh_mass;
        c.mseed = cols->mseed;
        c.mdot = cols->mdot;
        c.formationtime = cols->formationtime;
        c.swallowid = (unsigned long long *)cols->swallowid;
        c.bh_density = cols->bh_density;
        c.tb_dynfric = cols->tb_dynfric;
        c.minpotpos = cols->minpotpos;
        c.dfaccel = cols->dfaccel;
        c.df_surroundingvel = cols->df_surroundingvel;
        c.dragaccel = cols->dragaccel;
        c.df_surroundingrmsvel = cols->df_surroundingrmsvel;
        c.df_surroundingdensity = cols->df_surroundingdensity;
        c.jumptominpot = cols->jumptominpot;
        c.countprogs = cols->countprogs;
        c.mtrack = cols->mtrack;
        c.kineticfdbkenergy = cols->kineticfdbkenergy;
        c.vdisp = cols->vdisp;
    }
    bool notgas = false;
    *nseeds = eng->fof.seed(p, cols ? &c : nullptr, cap, (long long *)d_seed_particle, (long long *)d_seed_group, nwarn, &notgas, eng->stream);
    MPG_CHECK(!notgas, "fof_seed: a seed row is no gas particle (only gas turns into black holes, blackhole.c:1057); nothing was converted");
    MPG_CHECK(*nseeds <= cap, "fof_seed: the seed list needs more room than cap (*nseeds is set; nothing was converted)");
    API_END
}

/* ------------------------------ matter power spectrum of the PM step ------------------------------ */
int mpg_gravpm_measure_power(mpg_engine *eng, int on)
{
    API_BEGIN
    MPG_CHECK(eng, "null engine");
    eng->pm.measure_power = on != 0;
    API_END
}

int mpg_gravpm_set_nu_response(mpg_engine *eng, mpg_nu_response_fn fn, void *ctx, double BoxSize_in_MPC)
{
    API_BEGIN
    MPG_CHECK(eng, "null engine");
    MPG_CHECK(!fn || (BoxSize_in_MPC > 0 && std::isfinite(BoxSize_in_MPC)), "mpg_gravpm_set_nu_response: BoxSize_in_MPC must be positive");
    eng->pm.nu_fn = fn;
    eng->pm.nu_ctx = fn ? ctx : nullptr;
    eng->pm.nu_box_mpc = fn ? BoxSize_in_MPC : 0;
    API_END
}

int mpg_gravpm_set_hybrid_nu_tracer(mpg_engine *eng, int on)
{
    API_BEGIN
    MPG_CHECK(eng, "null engine");
    eng->pm.hybrid_tracer = on != 0;
    API_END
}

int mpg_dev_gravpm_powerspectrum_raw(mpg_engine *eng, double *d_acc, int64_t *d_modes)
{
    API_BEGIN
    MPG_CHECK(eng && d_acc && d_modes, "null argument");
    MPG_CHECK(eng->pm.nmesh > 0 && eng->pm.ps_valid, "power spectrum: no PM step has been run with the measurement on");
    MPG_HIP(hipSetDevice(eng->device));
    const size_t nb = (size_t)eng->pm.nmesh;
    MPG_HIP(hipMemcpyAsync(d_acc, eng->pm.ps_acc.p, (2 * nb + 1) * sizeof(double), hipMemcpyDeviceToDevice, eng->stream));
    MPG_HIP(hipMemcpyAsync(d_modes, eng->pm.ps_modes.p, nb * sizeof(int64_t), hipMemcpyDeviceToDevice, eng->stream));
    API_END
}

int mpg_powerspectrum_sum(int nbins, const double *acc, const int64_t *modes, double BoxSize_in_MPC, double *kk, double *Power,
                          int64_t *Nmodes, int *nonzero)
{
    API_BEGIN
    MPG_CHECK(nbins > 0 && acc && modes && kk && Power && Nmodes && nonzero, "null argument");
    const double Norm = acc[2 * (size_t)nbins];
    int nz = 0;
    for(int i = 0; i < nbins; i++) { // powerspectrum.c:75-89
        if(modes[i] == 0)
            continue;
        double P = acc[i] / modes[i];
        P /= Norm;
        double k = acc[nbins + i] / modes[i];
        k *= 2 * M_PI / BoxSize_in_MPC;
        P *= pow(BoxSize_in_MPC, 3.0);
        Power[nz] = P;
        kk[nz] = k;
        Nmodes[nz] = modes[i];
        nz++;
    }
    *nonzero = nz;
    API_END
}

int mpg_gravpm_get_powerspectrum(mpg_engine *eng, double BoxSize_in_MPC, double *kk, double *Power, int64_t *Nmodes, int *nonzero)
{
    API_BEGIN
    MPG_CHECK(eng && kk && Power && Nmodes && nonzero, "null argument");
    MPG_CHECK(eng->pm.nmesh > 0 && eng->pm.ps_valid, "power spectrum: no PM step has been run with the measurement on");
    MPG_HIP(hipSetDevice(eng->device));
    const size_t nb = (size_t)eng->pm.nmesh;
    std::vector<double> acc(2 * nb + 1);
    std::vector<int64_t> modes(nb);
    MPG_HIP(hipMemcpyAsync(acc.data(), eng->pm.ps_acc.p, (2 * nb + 1) * sizeof(double), hipMemcpyDeviceToHost, eng->stream));
    MPG_HIP(hipMemcpyAsync(modes.data(), eng->pm.ps_modes.p, nb * sizeof(int64_t), hipMemcpyDeviceToHost, eng->stream));
    MPG_HIP(hipStreamSynchronize(eng->stream));
    MPG_CALL(mpg_powerspectrum_sum((int)nb, acc.data(), modes.data(), BoxSize_in_MPC, kk, Power, Nmodes, nonzero));
    API_END
}

int mpg_powerspectrum_save(const char *OutputDir, const char *filename, double Time, double D1, int nonzero, const double *kk,
                           const double *Power, const int64_t *Nmodes)
{
    API_BEGIN
    MPG_CHECK(OutputDir && filename && kk && Power && Nmodes && nonzero >= 0, "null argument");
    char fname[4096];
    if(Time <= 1e-4) // "avoid -0.0000.txt at high z" (powerspectrum.c:101-105)
        snprintf(fname, sizeof(fname), "%s/%s-%0.4e.txt", OutputDir, filename, Time);
    else
        snprintf(fname, sizeof(fname), "%s/%s-%0.4f.txt", OutputDir, filename, Time);
    FILE *fp = fopen(fname, "w");
    MPG_CHECK(fp != nullptr, std::string("Could not open ") + fname + " for writing");
    fprintf(fp, "# in Mpc/h Units \n");
    fprintf(fp, "# D1 = %g \n", D1);
    fprintf(fp, "# k P N P(z=0)\n");
    for(int i = 0; i < nonzero; i++)
        fprintf(fp, "%g %g %ld %g\n", kk[i], Power[i], (long)Nmodes[i], Power[i] / (D1 * D1));
    fclose(fp);
    API_END
}

/* ------------------------------ snapshot / IC wire format (host IO) ------------------------------ */
int mpg_bigfile_block_info(const char *file, const char *block, mpg_bigblock_info *info)
{
    API_BEGIN
    MPG_CHECK(info, "null argument");
    BigBlockInfo b;
    bigfile_block_info(file, block, &b);
    memcpy(info->dtype, b.dtype, 8);
    info->nmemb = b.nmemb;
    info->nfile = b.nfile;
    info->size = b.size;
    API_END
}

int mpg_bigfile_read_block(const char *file, const char *block, int64_t start, int64_t count, const char *want_dtype, void *out)
{
    API_BEGIN
    MPG_CHECK(out || count == 0, "null argument");
    bigfile_read_block(file, block, start, count, want_dtype, out);
    API_END
}

int mpg_bigfile_write_block(const char *file, const char *block, const char *dtype, int nmemb, int nfile, int64_t size, const char *src_dtype,
                            const void *data)
{
    API_BEGIN
    MPG_CHECK(data || size == 0, "null argument");
    bigfile_write_block(file, block, dtype, nmemb, nfile, size, src_dtype, data);
    API_END
}

int mpg_bigfile_get_attr(const char *file, const char *block, const char *name, const char *want_dtype, void *out, int nmemb)
{
    try {
        MPG_CHECK(name && out, "null argument");
        if(bigfile_get_attr(file, block, name, want_dtype, out, nmemb) != 0) {
            g_err = std::string("bigfile: no attribute `") + name + "'";
            return 2;
        }
    }
    catch(const std::exception &e) {
        g_err = e.what();
        return 1;
    }
    g_err.clear();
    return 0;
}

int mpg_bigfile_set_attr(const char *file, const char *block, const char *name, const char *dtype, const void *data, int nmemb)
{
    API_BEGIN
    MPG_CHECK(data || nmemb == 0, "null argument");
    bigfile_set_attr(file, block, name, dtype, data, nmemb);
    API_END
}

/* ------------------------------ introspection ------------------------------ */

int mpg_tree_get_stats(mpg_engine *eng, mpg_tree_stats *st)
{
    API_BEGIN
    MPG_CHECK(eng && st, "null argument");
    MPG_CHECK(eng->tree_allocated, "no tree");
    MPG_HIP(hipSetDevice(eng->device));
    const TreeBuilder &t = eng->tree;
    st->NumParticles = t.npart;
    st->numnodes = t.nnodes;
    st->maxlevel = t.maxlevel;
    std::vector<NodeLink> lk(t.nnodes);
    MPG_HIP(hipStreamSynchronize(eng->stream));
    MPG_HIP(hipMemcpy(lk.data(), t.link.p, t.nnodes * sizeof(NodeLink), hipMemcpyDeviceToHost));
    int64_t nl = 0;
    for(auto &l : lk)
        nl += l.pcount > 0;
    st->numleaves = nl;
    Src4 root{};
    if(t.has_moments)
        MPG_HIP(hipMemcpy(&root, t.src.p + t.npart, sizeof(Src4), hipMemcpyDeviceToHost));
    st->root_mass = root.m;
    st->root_cofm[0] = root.x;
    st->root_cofm[1] = root.y;
    st->root_cofm[2] = root.z;
    st->root_hmax = 0;
    if(t.has_hmax)
        MPG_HIP(hipMemcpy(&st->root_hmax, t.hmax.p, sizeof(double), hipMemcpyDeviceToHost));
    API_END
}

int mpg_tree_export(mpg_engine *eng, int32_t *level, double *center, double *len, double *cofm, double *mass, double *hmax,
                    int32_t *sibling, int32_t *pstart, int32_t *pcount)
{
    API_BEGIN
    MPG_CHECK(eng, "null engine");
    MPG_CHECK(eng->tree_allocated, "no tree");
    MPG_HIP(hipSetDevice(eng->device));
    const TreeBuilder &t = eng->tree;
    MPG_HIP(hipStreamSynchronize(eng->stream));
    std::vector<NodeLink> lk(t.nnodes);
    std::vector<NodeGeo> g(t.nnodes);
    std::vector<Src4> m(t.nnodes);
    MPG_HIP(hipMemcpy(lk.data(), t.link.p, t.nnodes * sizeof(NodeLink), hipMemcpyDeviceToHost));
    MPG_HIP(hipMemcpy(g.data(), t.geo.p, t.nnodes * sizeof(NodeGeo), hipMemcpyDeviceToHost));
    if(t.has_moments)
        MPG_HIP(hipMemcpy(m.data(), t.src.p + t.npart, t.nnodes * sizeof(Src4), hipMemcpyDeviceToHost));
    std::vector<double> hm;
    if(hmax && t.has_hmax) {
        hm.resize(t.nnodes);
        MPG_HIP(hipMemcpy(hm.data(), t.hmax.p, t.nnodes * sizeof(double), hipMemcpyDeviceToHost));
    }
    for(int64_t j = 0; j < t.nnodes; j++) {
        if(level)
            level[j] = lk[j].level;
        if(sibling)
            sibling[j] = lk[j].sibling;
        if(pstart)
            pstart[j] = lk[j].pstart;
        if(pcount)
            pcount[j] = lk[j].pcount;
        if(center) {
            center[3 * j + 0] = g[j].cx;
            center[3 * j + 1] = g[j].cy;
            center[3 * j + 2] = g[j].cz;
        }
        if(len)
            len[j] = g[j].len;
        if(cofm) {
            cofm[3 * j + 0] = m[j].x;
            cofm[3 * j + 1] = m[j].y;
            cofm[3 * j + 2] = m[j].z;
        }
        if(mass)
            mass[j] = m[j].m;
        if(hmax)
            hmax[j] = hm.empty() ? 0.0 : hm[j];
    }
    API_END
}

int mpg_tree_export_order(mpg_engine *eng, int32_t *order)
{
    API_BEGIN
    MPG_CHECK(eng && order, "null argument");
    MPG_CHECK(eng->tree_allocated, "no tree");
    MPG_HIP(hipSetDevice(eng->device));
    MPG_HIP(hipStreamSynchronize(eng->stream));
    MPG_HIP(hipMemcpy(order, eng->tree.idx_b.p, eng->tree.npart * sizeof(int32_t), hipMemcpyDeviceToHost));
    API_END
}

int mpg_tree_export_derived(mpg_engine *eng, int32_t *dfs_of_bfs, int32_t *linkB, double *geoB, double *momB, double *hmaxB, double *geoS,
                            double *hsmaxS, double *srcL, int32_t present[4])
{
    API_BEGIN
    MPG_CHECK(eng && present, "null argument");
    MPG_CHECK(eng->tree_allocated, "no tree");
    MPG_HIP(hipSetDevice(eng->device));
    TreeBuilder &t = eng->tree;
    t.ensure_level_order(eng->stream);
    MPG_HIP(hipStreamSynchronize(eng->stream));
    if(eng->pad_pending) // (leaf blocks being written on the tree's own stream)
        MPG_HIP(hipEventSynchronize(eng->ev_pad_done));
    const TreeView v = t.view();
    const size_t M = (size_t)t.nnodes;
    const auto out = [&](void *dst, const void *src, size_t bytes) {
        if(dst && src)
            MPG_HIP(hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost));
    };
    static_assert(sizeof(NodeLinkB) == 4 * sizeof(int32_t) && sizeof(NodeGeo) == 4 * sizeof(double) && sizeof(Src4) == 4 * sizeof(double),
                  "the read-out copies the records as they are");
    out(dfs_of_bfs, t.nid_b.p, M * sizeof(uint32_t));
    out(linkB, v.linkB, M * sizeof(NodeLinkB));
    out(geoB, v.geoB, M * sizeof(NodeGeo));
    out(momB, v.momB, M * sizeof(Src4));
    out(hmaxB, v.hmaxB, M * sizeof(double));
    out(geoS, v.geoS, M * sizeof(NodeGeo));
    out(hsmaxS, v.hsmaxS, M * sizeof(double));
    out(srcL, v.srcL, (M + 1) * 8 * sizeof(Src4));
    present[0] = v.hmaxB != nullptr;
    present[1] = v.geoS != nullptr;
    present[2] = v.hsmaxS != nullptr;
    present[3] = v.srcL != nullptr;
    API_END
}

int mpg_walk_get_counters(mpg_engine *eng, int64_t counters[10])
{
    API_BEGIN
    MPG_CHECK(eng && counters, "null argument");
    MPG_HIP(hipSetDevice(eng->device));
    MPG_HIP(hipStreamSynchronize(eng->stream));
    unsigned long long c[16] = {0};
    MPG_HIP(hipMemcpy(c, eng->counters.p, 16 * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    counters[0] = (int64_t)c[0];
    counters[1] = (int64_t)c[1];
    counters[2] = (int64_t)c[2];
    counters[3] = eng->last_targets;
    for(int k = 0; k < 6; k++)
        counters[4 + k] = (int64_t)c[3 + k];
    API_END
}

int mpg_walk_get_f32_stats(mpg_engine *eng, int64_t out[2])
{
    API_BEGIN
    MPG_CHECK(eng && out, "null argument");
    MPG_HIP(hipSetDevice(eng->device));
    MPG_HIP(hipStreamSynchronize(eng->stream));
    unsigned long long c[16] = {0};
    MPG_HIP(hipMemcpy(c, eng->counters.p, 16 * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    out[0] = (int64_t)c[12];
    out[1] = (int64_t)c[13];
    API_END
}

int mpg_get_phase_times(mpg_engine *eng, mpg_phase_times *t)
{
    API_BEGIN
    MPG_CHECK(eng && t, "null argument");
    *t = eng->timer.t;
    API_END
}

int mpg_set_instrumentation(mpg_engine *eng, int timing, int counters)
{
    API_BEGIN
    MPG_CHECK(eng, "null engine");
    eng->timer.enabled = timing != 0;
    eng->count = counters != 0;
    API_END
}

int mpg_walk_events_collect2(mpg_engine *eng, double *total_ms, int *count, double *lists_ms, double *eval_ms, int *count_split)
{
    API_BEGIN
    MPG_CHECK(eng && total_ms && count, "null argument");
    MPG_HIP(hipSetDevice(eng->device));
    MPG_HIP(hipStreamSynchronize(eng->stream));
    double tot = 0, tl = 0, te = 0;
    int c = 0, cs = 0;
    for(size_t k = 0; k < eng->walk_events.size(); k++) {
        auto &ev = eng->walk_events[k];
        float ms = 0;
        MPG_HIP(hipEventSynchronize(ev.second));
        MPG_HIP(hipEventElapsedTime(&ms, ev.first, ev.second));
        tot += ms;
        c++;
        if(hipEvent_t mid = k < eng->walk_mid.size() ? eng->walk_mid[k] : nullptr) {
            float a = 0, b = 0;
            MPG_HIP(hipEventElapsedTime(&a, ev.first, mid));
            MPG_HIP(hipEventElapsedTime(&b, mid, ev.second));
            tl += a;
            te += b;
            cs++;
            eng->free_mid.push_back(mid);
        }
        eng->free_events.push_back(ev);
    }
    eng->walk_events.clear();
    eng->walk_mid.clear();
    *total_ms = tot;
    *count = c;
    if(lists_ms)
        *lists_ms = tl;
    if(eval_ms)
        *eval_ms = te;
    if(count_split)
        *count_split = cs;
    API_END
}

int mpg_walk_events_collect(mpg_engine *eng, double *total_ms, int *count)
{
    return mpg_walk_events_collect2(eng, total_ms, count, nullptr, nullptr, nullptr);
}

const int *mpg_dev_tree_order(mpg_engine *eng) { return (eng && eng->tree_allocated) ? (const int *)eng->tree.idx_b.p : nullptr; }

/* tuning knob used by bench/tests: minimum number of walking lanes that keeps the node phase going */
int mpg_set_walk_split_mode(mpg_engine *eng, int overlap, int chunks_per_wave)
{
    API_BEGIN
    MPG_CHECK(eng && chunks_per_wave >= 0 && chunks_per_wave <= 1024, "bad argument");
    eng->w3.split_overlap = overlap != 0;
    eng->w3.split_chunks_per_wave = chunks_per_wave;
    API_END
}

int mpg_set_walk_offsets64(mpg_engine *eng, int on)
{
    API_BEGIN
    MPG_CHECK(eng, "null engine");
    eng->w3.split_offsets64 = on != 0;
    API_END
}

int mpg_set_walk_threshold(mpg_engine *eng, int thresh)
{
    API_BEGIN
    MPG_CHECK(eng, "null engine");
    eng->walk_thresh = thresh;
    API_END
}

int mpg_set_walk_list_capacity(mpg_engine *eng, int cap)
{
    API_BEGIN
    MPG_CHECK(eng && cap >= 16 && cap <= 65536, "walk list capacity must be in [16, 65536]");
    eng->w3.cap = cap;
    eng->w3.split_cap = (cap + 7) / 8 * 8;
    API_END
}

int mpg_get_walk_choice(mpg_engine *eng, int *variant, int *list_capacity, unsigned *last_overflow)
{
    API_BEGIN
    MPG_CHECK(eng && variant, "null argument");
    *variant = eng->walk_variant ? eng->walk_variant : eng->walk_choice;
    if(list_capacity)
        *list_capacity = eng->w3.split_cap;
    if(last_overflow)
        *last_overflow = eng->w3.split_last_overflow;
    API_END
}

int mpg_set_walk_variant(mpg_engine *eng, int variant)
{
    API_BEGIN
    MPG_CHECK(eng && (variant == 0 || variant == 1 || variant == 4 || variant == 6), "walk variant must be 0 (auto), 1, 4 or 6");
    eng->walk_variant = variant;
    eng->walk_choice = 0;
    API_END
}

} // extern "C"
