/* include/mpgadget_hip.h -- C-ABI of the MI355X (gfx950) TreePM + SPH force engine.
 *
 * The reference (MP-Gadget, plain C, statically linked) has no FFI: its "operator API" is the set of C
 * entry points run.c / timestep.c / init.c / runtests.c call.  Each function below replaces one of
 * those entry points (cited as libgadget/<file>:<line>) with plain pointers and sizes, so that a
 * 30-line shim compiled inside the reference tree can forward the reference symbols
 *   gravpm_init_periodic, gravpm_force, force_tree_full, force_tree_rebuild_mask, force_tree_free,
 *   grav_short_tree, gravshort_fill_ntab, gravshort_set_softenings, set_gravshort_treepar, FORCE_SOFTENING,
 *   density, hydro_force
 * to this library.  No torch / C++ types appear in any signature.
 * Around that path: drift / kicks / gravity time bins and the hierarchical gravity level loop, Peano-Hilbert keys
 * and the (type, key) particle order, friends-of-friends groups, the matter power spectrum of the PM step, and the snapshot / IC
 * wire format - each section below cites what it replaces.
 *
 * Conventions
 *   - every call returns 0 on success, non-zero on failure; mpg_last_error() gives the message
 *     (the shim maps it to endrun(), utils/endrun.h:4-7 -- the reference has no return codes on this path);
 *   - "host" calls take the reference's AoS particle table through an mpg_particle_view (base pointer,
 *     stride and byte offsets: the same idea as PetaPMParticleStruct, petapm.h:86-99), copy what they
 *     need to HBM, run, and scatter results back into the caller's structs;
 *   - "dev" calls take device pointers (SoA, fp64) already resident in HBM and leave results in HBM;
 *     they are what bench.py times;
 *   - all arithmetic on the path is fp64 (MyFloat = double, types.h:13-17); P.Mass is float
 *     (partmanager.h:15) and the short-range window tables are float (gravity.c:20).
 */
#ifndef MPGADGET_HIP_H
#define MPGADGET_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct mpg_engine mpg_engine;

/* ---- life cycle ------------------------------------------------------------------------------ */
/* Create an engine bound to HIP device `device` (one engine per GPU / MPI rank). */
int mpg_engine_create(mpg_engine **out, int device);
void mpg_engine_destroy(mpg_engine *eng);
/* Last error message of the calling thread ("" if none). */
const char *mpg_last_error(void);
/* Library / build identification string. */
const char *mpg_version(void);
/* Hash over the sources, headers and compiler flags this library was built from (build.py); the Python host side refuses a library
 * whose stamp differs from the sources next to it. */
const char *mpg_build_stamp(void);
/* Use an existing HIP stream (hipStream_t passed as void*) for all engine work; NULL = engine's own. */
int mpg_engine_set_stream(mpg_engine *eng, void *hip_stream);
void *mpg_engine_get_stream(mpg_engine *eng);
/* Block until all engine work is complete. */
int mpg_engine_synchronize(mpg_engine *eng);

/* ---- module parameters ----------------------------------------------------------------------- */
/* struct gravshort_tree_params, libgadget/gravity.h:9-22 (same fields, same order). */
typedef struct mpg_gravshort_tree_params {
    double ErrTolForceAcc;
    double BHOpeningAngle;
    double MaxBHOpeningAngle;
    int TreeUseBH;
    double Rcut;
    double FractionalGravitySoftening;
} mpg_gravshort_tree_params;

/* set_gravshort_treepar / get_gravshort_treepar, libgadget/gravshort-tree.c:53-61 */
int mpg_set_gravshort_treepar(mpg_engine *eng, const mpg_gravshort_tree_params *par);
int mpg_get_gravshort_treepar(mpg_engine *eng, mpg_gravshort_tree_params *par);
/* gravshort_set_softenings, libgadget/gravshort-tree.c:44-50 */
int mpg_gravshort_set_softenings(mpg_engine *eng, double MeanSeparation);
/* FORCE_SOFTENING, libgadget/gravshort-tree.c:37-41 (returns 2.8 * GravitySoftening) */
double mpg_force_softening(mpg_engine *eng);
/* gravshort_fill_ntab, libgadget/gravity.c:22-51.  window_type 0 = exact (needs Asmth == 1.5), 1 = erfc.
 * `table` = the calibrated 512 x 5 float64 table of libgadget/shortrange-kernel.c (row-major; carried as
 * data in mp-gadget_amd/data/shortrange_force_kernels.f64). */
int mpg_gravshort_fill_ntab(mpg_engine *eng, int window_type, double Asmth, const double *table, int nrows);
/* gravpm_init_periodic, libgadget/gravpm.c:51-54 (-> petapm_init, petapm.c:105-223): creates the mesh and FFT plans. */
int mpg_gravpm_init_periodic(mpg_engine *eng, double BoxSize, double Asmth, int Nmesh, double G);
/* petapm_destroy, libgadget/petapm.c:225-232 */
int mpg_petapm_destroy(mpg_engine *eng);
/* init_forcetree_params, libgadget/forcetree.c:39-44 (node pool = factor * NumPart; the engine grows it on demand) */
int mpg_init_forcetree_params(mpg_engine *eng, double TreeAllocFactor);

/* ---- particle table view (host AoS) ---------------------------------------------------------- */
/* Byte offsets into the caller's AoS record; -1 = field absent.  For struct particle_data
 * (libgadget/partmanager.h:9-71; 160 bytes) use mpg_particle_view_reference_layout(). */
typedef struct mpg_particle_view {
    void *base;        /* &P[0] */
    int64_t n;         /* PartManager->NumPart */
    int64_t stride;    /* sizeof(struct particle_data) */
    int32_t off_pos;   /* double[3]  Pos */
    int32_t off_mass;  /* float      Mass */
    int32_t off_flags; /* uint8 holding the bit-fields of partmanager.h:17-21: bit 0 IsGarbage, bit 1 Swallowed */
    int32_t off_type;  /* uint8 Type (partmanager.h:30) */
    int32_t off_accel; /* double[3]  FullTreeGravAccel */
    int32_t off_gravpm;    /* double[3]  GravPM */
    int32_t off_potential; /* double     Potential */
    int32_t off_hsml;      /* double     Hsml */
    int32_t off_vel;       /* double[3]  Vel */
    int32_t off_pi;        /* int32      PI (slot index) */
} mpg_particle_view;
/* Fill the offsets for the reference's struct particle_data (partmanager.h:9-71, offsets verified in SURVEY 8(a)). */
void mpg_particle_view_reference_layout(mpg_particle_view *v, void *particles, int64_t NumPart);

/* ---- host (drop-in) entry points ------------------------------------------------------------- */
/* Every host entry point that needs positions packs Pos / Mass / Type of P[] and uploads them, because P may have moved or
 * changed between calls.  A caller that knows better declares an EPOCH of its particle table: calls made with the same non-zero
 * epoch, the same &P[0], NumPart and BoxSize as the last upload reuse it (gravpm_force -> force_tree_full -> grav_short_tree of
 * one step, run.c:522-548).  Bump the epoch after anything that moves or reorders particles (drift, exchange, garbage collection);
 * 0 (the default) switches the reuse off. */
int mpg_set_particle_epoch(mpg_engine *eng, int64_t epoch);
/* Overlap of the host path's transfers with the device's work inside one epoch (default off).  When on - and only while a non-zero epoch is
 * declared - (a) the first call of an epoch packs Pos / Mass / Type, Potential and FullTreeGravAccel in ONE pass over the records, and
 * mpg_grav_short_tree takes OldAcc = |FullTreeGravAccel + GravPM| / G on the device from that upload and the device's own GravPM instead of
 * reading P[] again; (b) mpg_gravpm_force RETURNS once its results are on their way: GravPM and Potential are copied down and written into
 * P[] by a host thread while force_tree_full and grav_short_tree run, and are complete when the next call on the table that needs them
 * returns (mpg_grav_short_tree at the latest) or when mpg_host_results_sync returns.  A caller whose host code reads P[].GravPM /
 * P[].Potential between gravpm_force and grav_short_tree (energy_statistics, run.c:527) calls mpg_host_results_sync first.  (c) A walk of all
 * particles on a tree of all particles runs in slices of the tree order (5 from 2^20 particles on, each 0.55 of the one before it so that
 * the write-back nothing hides is the smallest; `on` = 2 .. 8 forces that many at any size), the results of a slice travelling down and into
 * P[] while the next is walked; results bit-identical to the unsliced walk. */
int mpg_set_host_overlap(mpg_engine *eng, int on);
/* The epoch's packing pass + uploads started early (round 6): call after mpg_set_particle_epoch as soon as P[] is final for the step - the
 * end of drift_all_particles (drift.c:84-102) - and the pass (Pos, Mass, Type, Potential, FullTreeGravAccel) runs on a host thread while the
 * caller goes on (run.c:420-522: domain_maintain, the active list); mpg_gravpm_force / mpg_density / ... of the same epoch and table join it
 * instead of packing.  A new epoch in between (an exchange, a garbage collection) simply leaves the upload unused.  Needs
 * mpg_set_host_overlap; a no-op without it or in resident mode.  P[] must not be written until the epoch's first entry point has returned,
 * and that entry point (or mpg_set_particle_epoch / mpg_host_results_sync, which wait for the pass) is the next call on this engine: the
 * pass uses the engine's stream. */
int mpg_host_prefetch(mpg_engine *eng, const mpg_particle_view *pv, double BoxSize);
int mpg_host_results_sync(mpg_engine *eng);
/* gravpm_force, libgadget/gravpm.c:61-119: zero GravPM, CIC deposit, r2c, Green's function, 4 x (transfer, c2r,
 * CIC readout).  Writes P[i].GravPM[3] (=) and P[i].Potential (+=, as readout_potential does). */
int mpg_gravpm_force(mpg_engine *eng, const mpg_particle_view *pv);
/* force_tree_full, libgadget/forcetree.c:110-128: tree of all particles with moments.  `mask` as ALLMASK etc.
 * (forcetree.h:22-27); particles whose type bit is clear are left out. */
int mpg_force_tree_full(mpg_engine *eng, const mpg_particle_view *pv, double BoxSize);
/* force_tree_rebuild_mask, libgadget/forcetree.c:151-166 */
int mpg_force_tree_rebuild_mask(mpg_engine *eng, const mpg_particle_view *pv, double BoxSize, int mask);
/* force_tree_free, libgadget/forcetree.c:1403-1413 */
int mpg_force_tree_free(mpg_engine *eng);
/* force_tree_active_moments (forcetree.c:129-148): a tree of the active particles only (ActiveParticle == NULL: all), with
 * moments; HybridNuTracer != 0 leaves neutrinos (type 2) out.  A walk over it takes the same active list as its targets. */
int mpg_force_tree_active_moments(mpg_engine *eng, const mpg_particle_view *pv, double BoxSize, const int *ActiveParticle,
                                  int64_t NumActiveParticle, int HybridNuTracer);
int mpg_dev_force_tree_active_moments(mpg_engine *eng, const int *d_active, int64_t nactive, int HybridNuTracer);
/* grav_short_tree, libgadget/gravshort-tree.c:96-154.  ActiveParticle == NULL means all particles
 * (timestep.c:77-84).  AccelStore may be NULL.  When the tree holds all particles (full_particle_tree_flag)
 * P[i].FullTreeGravAccel and P[i].Potential are updated as grav_short_postprocess does (gravshort.h:47-67).
 * After the call TreeUseBH > 1 is reset to 0 (gravshort-tree.c:148-151). */
int mpg_grav_short_tree(mpg_engine *eng, const mpg_particle_view *pv, const int *ActiveParticle, int64_t NumActiveParticle,
                        double (*AccelStore)[3], double rho0);

/* ---- device-resident drop-in mode ------------------------------------------------------------------------------------------
 * The host-pointer calls above upload Pos / Mass and download their results on every call, because the caller may have touched P[]
 * in between (run.c:392-548 drifts, kicks and exchanges on the host).  A caller that lets the engine integrate as well
 * (mpg_dev_drift_all_particles / mpg_dev_apply_pm_half_kick / mpg_dev_apply_half_kick, drift.c:18-102, timestep.c:873-1036, on the
 * arrays of mpg_resident_arrays) declares its table RESIDENT: mpg_resident_begin uploads Pos, Mass, Type / flags, Vel,
 * FullTreeGravAccel, GravPM and Potential once; from then on mpg_gravpm_force, mpg_force_tree_full / _rebuild_mask and
 * mpg_grav_short_tree called with the same view run on the device copies and leave their results there (P[] on the host goes stale:
 * AccelStore, when given, still receives its copy).  mpg_resident_fetch writes the named columns back into P[] for the host modules
 * that read them, mpg_resident_push takes columns the host changed, mpg_resident_end fetches everything and leaves the mode (and writes
 * a StoredGravAccel held for a split-gravity step back into the caller's array: mpg_resident_hierarchical_*, further down).
 * Anything that reorders or resizes P[] (domain_exchange, slots_gc) goes between _end and a new _begin. */
#define MPG_FIELD_POS 1u
#define MPG_FIELD_VEL 2u
#define MPG_FIELD_ACCEL 4u     /* FullTreeGravAccel */
#define MPG_FIELD_GRAVPM 8u
#define MPG_FIELD_POTENTIAL 16u
typedef struct mpg_resident_view {
    int64_t n;
    double *d_pos;            /* [n][3] */
    float *d_mass;            /* [n] */
    unsigned char *d_type;    /* [n] (7 = garbage / swallowed) */
    double *d_vel;            /* [n][3] or NULL when the view had no Vel */
    double *d_fulltree_accel; /* [n][3] */
    double *d_gravpm;         /* [n][3] */
    double *d_potential;      /* [n] */
} mpg_resident_view;
int mpg_resident_begin(mpg_engine *eng, const mpg_particle_view *pv, double BoxSize);
int mpg_resident_arrays(mpg_engine *eng, mpg_resident_view *out);
int mpg_resident_fetch(mpg_engine *eng, const mpg_particle_view *pv, unsigned fields);
int mpg_resident_push(mpg_engine *eng, const mpg_particle_view *pv, unsigned fields);
int mpg_resident_end(mpg_engine *eng, const mpg_particle_view *pv);

/* (a gas run stays resident too: mpg_resident_sph_begin and the integrator calls further down, behind the types they take) */

/* ---- device-resident entry points (inputs and outputs stay in HBM) ---------------------------- */
/* Bind device arrays in the caller's particle order: pos[n][3] f64, mass[n] f32, type[n] u8 (NULL = all type 1).
 * The arrays must stay valid until the next bind. */
int mpg_dev_bind_particles(mpg_engine *eng, int64_t n, const double *d_pos, const float *d_mass, const uint8_t *d_type,
                           double BoxSize);
/* gravpm_force on bound particles: d_gravpm[n][3] (=), d_potential[n] (+=; may be NULL). */
int mpg_dev_gravpm_force(mpg_engine *eng, double *d_gravpm, double *d_potential);
/* force_tree_full / force_tree_rebuild_mask on bound particles.  Called right after mpg_dev_gravpm_force (the order of run.c:522-548)
 * the build runs on an engine-internal second stream next to the PM force - neither depends on the other - and everything queued
 * afterwards waits for both.  The bound positions must not change between the two calls other than through this API
 * (mpg_dev_bind_particles / mpg_dev_drift_all_particles switch the overlap off for the next build); MPG_NO_TREE_OVERLAP=1 disables it. */
int mpg_dev_force_tree_build(mpg_engine *eng, int mask);
/* grav_short_tree on bound particles.  d_oldacc[n] = |FullTreeGravAccel + GravPM| / G (grav_get_abs_accel,
 * gravshort.h:70-80) or NULL to have it computed from d_prev_accel[n][3] + d_gravpm[n][3].
 * d_active: int32 target indices or NULL (all).  d_accel[n][3] receives G * Acc for every target;
 * d_potential[n] (may be NULL) receives the post-processed potential. */
int mpg_dev_grav_short_tree(mpg_engine *eng, const double *d_oldacc, const double *d_prev_accel, const double *d_gravpm,
                            const int *d_active, int64_t nactive, double *d_accel, double *d_potential, double rho0);

/* Work measure for the domain decomposition (the reference balances TopLeaves by cost, domain.c:611): while d_cost is set, the
 * two-kernel walk writes d_cost[i] = 8 x leaf-list entries + nodes used + 8 x traversal steps for every target i (caller order;
 * other entries untouched).  NULL switches it off. */
int mpg_dev_set_walk_cost(mpg_engine *eng, float *d_cost);

/* ---- SPH: density (with the smoothing-length iteration) and hydro force ----------------------------- */
/* struct density_params, libgadget/density.h:10-25 (same fields, same order; DensityKernelType is the enum value
 * 1 cubic / 2 quintic / 4 quartic of densitykernel.h:17-21). */
typedef struct mpg_density_params {
    double DensityResolutionEta;
    double MaxNumNgbDeviation;
    double BlackHoleNgbFactor;
    double BlackHoleMaxAccretionRadius;
    int DensityKernelType;
    double MinGasHsmlFractional;
} mpg_density_params;
/* struct hydro_params, libgadget/hydra.c:26-34 */
typedef struct mpg_hydro_params {
    int DensityIndependentSphOn;
    double DensityContrastLimit;
    double ArtBulkViscConst;
} mpg_hydro_params;
/* set_densitypar (density.c:22-27) / the hydro_params of set_hydro_params (hydra.c:36-48) */
int mpg_set_densitypar(mpg_engine *eng, const mpg_density_params *dp);
int mpg_set_hydropar(mpg_engine *eng, const mpg_hydro_params *hp);
/* GetNumNgb (density.c:53-59) for the current parameters */
double mpg_get_numngb(mpg_engine *eng);

/* Time-dependent scalars the reference derives from DriftKickTimes / Cosmology before the loops:
 * kick_factor_data (density.h:34-39, filled by init_kick_factor_data density.c:115-132), the per-bin density drift
 * factors of hydra.c:178-186, dloga_from_dti(Ti_Current - Ti_kick[bin]) used by SPH_EntVarPred (density.c:75),
 * get_dloga_for_bin (hydra.c:271,463), and atime / hubble_function(atime) (hydra.c:219-223).  Index = time bin, 0..46. */
typedef struct mpg_sph_times {
    double FgravkickB;
    double gravkicks[47];
    double hydrokicks[47];
    double drifts[47];
    double dloga_kick[47];
    double dloga_bin[47];
    double atime, hubble;
} mpg_sph_times;

/* Device arrays of the particle table in caller order (n = bound particles).  SPH slot fields (SphP[P[i].PI].X,
 * slotsmanager.h:93-129) are indexed by PARTICLE here; entries of non-gas particles are ignored.  NULL = absent/zero
 * for the optional inputs (gacc, gpm, hydroacc_in, tb_*, dtentropy_in) and optional outputs (dthsml, gradrho). */
typedef struct mpg_sph_arrays {
    double *hsml;                 /* in/out  P.Hsml */
    double *dthsml;               /* out     P.DtHsml */
    const double *vel;            /* [n][3]  P.Vel */
    const double *gacc;           /* [n][3]  P.FullTreeGravAccel */
    const double *gpm;            /* [n][3]  P.GravPM */
    const double *hydroacc_in;    /* [n][3]  SphP.HydroAccel (previous step, for the velocity prediction) */
    const uint8_t *tb_hydro;      /* P.TimeBinHydro */
    const uint8_t *tb_grav;       /* P.TimeBinGravity */
    const double *entropy;        /* SphP.Entropy */
    const double *dtentropy_in;   /* SphP.DtEntropy (previous step, for the entropy prediction) */
    double *density;              /* out SphP.Density (BHP.Density for type 5 targets) */
    double *egywtdensity;         /* out SphP.EgyWtDensity */
    double *dhsmlegyfac;          /* out SphP.DhsmlEgyDensityFactor */
    double *divvel;               /* out SphP.DivVel */
    double *curlvel;              /* out SphP.CurlVel */
    double *gradrho;              /* out [n][3] or NULL */
    double *hydroacc_out;         /* out [n][3] SphP.HydroAccel */
    double *dtentropy_out;        /* out SphP.DtEntropy */
    double *maxsignalvel;         /* out SphP.MaxSignalVel */
} mpg_sph_arrays;

/* force_tree_rebuild_mask without moments (forcetree.c:151-166) on the bound particles; with_moments != 0 also runs
 * force_tree_calc_moments (needed by set_init_hsml). */
int mpg_dev_force_tree_rebuild_mask(mpg_engine *eng, int mask, int with_moments);
/* set_init_hsml, libgadget/density.c:691-749 (tree with moments, mask GASMASK+BHMASK in the reference) */
int mpg_dev_set_init_hsml(mpg_engine *eng, const mpg_sph_arrays *A, double MeanGasSeparation);
/* density, libgadget/density.c:234-355.  d_active NULL = all particles.  Targets: gas and (non-swallowed) black holes. */
int mpg_dev_density(mpg_engine *eng, const mpg_sph_arrays *A, const mpg_sph_times *T, const int *d_active, int64_t nactive,
                    int update_hsml, int DoEgyDensity, int BlackHoleOn);
/* force_tree_calc_moments after density (run.c:477): propagates the leaf hmax of the final Hsml up the gas tree */
int mpg_dev_force_tree_calc_hmax(mpg_engine *eng);
/* force_update_hmax (forcetree.h:113, forcetree.c:1290-1340): the hmax moments of the current (gas) tree from the smoothing lengths in
 * d_hsml[n] (caller order; only gas and black holes count), without a density loop before it (test_forcetree.c:257-292) */
int mpg_dev_force_update_hmax(mpg_engine *eng, const double *d_hsml);
/* hydro_force, libgadget/hydra.c:153-245 (needs density() and the hmax moments of the same tree) */
int mpg_dev_hydro_force(mpg_engine *eng, const mpg_sph_arrays *A, const mpg_sph_times *T, const int *d_active, int64_t nactive);
/* Host-pointer forms of the four calls above: `P` supplies Pos / Mass / Type / flags (the reference AoS table), `A` holds HOST
 * arrays in particle order (the in-tree shim gathers SphP[P[i].PI].X into them).  Inputs are copied to HBM,
 * outputs copied back; the gas tree is (re)built inside, as force_tree_rebuild_mask does in run.c:466. */
int mpg_set_init_hsml(mpg_engine *eng, const mpg_particle_view *pv, double BoxSize, const mpg_sph_arrays *A, double MeanGasSeparation);
int mpg_density(mpg_engine *eng, const mpg_particle_view *pv, double BoxSize, const mpg_sph_arrays *A, const mpg_sph_times *T,
                const int *ActiveParticle, int64_t NumActiveParticle, int update_hsml, int DoEgyDensity, int BlackHoleOn);
int mpg_hydro_force(mpg_engine *eng, const mpg_particle_view *pv, const mpg_sph_arrays *A, const mpg_sph_times *T,
                    const int *ActiveParticle, int64_t NumActiveParticle);
/* statistics of the last SPH call: [0] density iterations, [1] targets summed over iterations,
 * [2] successful distance tests / hydro pairs evaluated, [3] candidates distance-tested */
int mpg_sph_get_stats(mpg_engine *eng, int64_t stats[4]);

/* ---- DM velocity dispersion of gas and black holes: winds_find_vel_disp, libgadget/veldisp.c:375-466 (run.c:646-647) ---------
 * For every active gas particle that may form stars during the next PM step (winds_veldisp_haswork, veldisp.c:348-371:
 * Density / densfac^3 >= 0.1 sfr_density_threshold, densfac = min(1, (Hsml + DtHsml ddrift) / Hsml)) the radius loop of
 * treewalk_do_hsml_loop finds the 40 +- 1 nearest DM particles - five trial radii per pass, ngb_narrow_down between the passes - and
 * stores their one-dimensional velocity dispersion, Hubble flow included, in vdisp; every active black hole receives the dispersion
 * of the DM inside its Hsml (blackhole_veldisp, one pass).  The engine does not evaluate the star-formation model: the caller passes
 * sfr_density_threshold(Time) and ddrift = get_exact_drift_factor(Ti_Current, Ti_Current + PM_length).  The kick factors of
 * DM_VelPred (density.c:106-112) are FgravkickB and gravkicks[] of mpg_sph_times; its other members are not read.
 * Garbage and swallowed particles carry type 7 (as everywhere in the dev calls); the host forms derive it from the flags.
 * vdisp is in/out, in particle order: entries of gas targets are SphP.VDisp, of black-hole targets BHP.VDisp; an entry is written
 * only where the reference writes it (a positive variance; a black hole with at least one DM neighbour), every other entry is
 * left as it was.  vel, hsml, density and vdisp are required; NULL for gacc, gpm, tb_grav, dthsml means zero.
 * THE TREE: when a gas particle qualifies or the table holds a black hole, the call rebuilds the engine's current tree as the tree
 * of the DM particles (DMMASK, no moments), as the reference does (veldisp.c:414); that is the current tree when the call returns,
 * so a density / hydro loop after it needs its gas tree rebuilt (mpg_dev_force_tree_rebuild_mask; the host forms mpg_density /
 * mpg_set_init_hsml rebuild it themselves).  When nothing qualifies and there is no black hole, no tree is built or demanded,
 * nothing is written and the current tree stays.  More than 400 iterations (the reference's endrun(1155)) is an error return.
 * One rank only: there is no mpg_dist_* form. */
typedef struct mpg_veldisp_params {
    double Time;                  /* scale factor a */
    double hubble;                /* hubble_function(a) */
    double ddrift;                /* drift factor over the next PM step */
    double sfr_density_threshold; /* sfr_density_threshold(Time); the engine takes a tenth of it */
} mpg_veldisp_params;
typedef struct mpg_veldisp_arrays {
    const double *vel;            /* [n][3]  P.Vel */
    const double *gacc;           /* [n][3]  P.FullTreeGravAccel */
    const double *gpm;            /* [n][3]  P.GravPM */
    const uint8_t *tb_grav;       /* P.TimeBinGravity */
    const double *hsml;           /* P.Hsml */
    const double *dthsml;         /* P.DtHsml */
    const double *density;        /* SphP.Density */
    double *vdisp;                /* in/out  SphP.VDisp / BHP.VDisp */
} mpg_veldisp_arrays;
/* on the bound particles; d_active NULL = all particles */
int mpg_dev_find_vel_disp(mpg_engine *eng, const mpg_veldisp_arrays *A, const mpg_sph_times *T, const mpg_veldisp_params *par, const int *d_active,
                          int64_t nactive);
/* host form: `pv` supplies Pos / Mass / Type / flags, `A` holds HOST arrays in particle order (the shim gathers SphP / BHP into them) */
int mpg_find_vel_disp(mpg_engine *eng, const mpg_particle_view *pv, double BoxSize, const mpg_veldisp_arrays *A, const mpg_sph_times *T,
                      const mpg_veldisp_params *par, const int *ActiveParticle, int64_t NumActiveParticle);
/* on a resident gas run (mpg_resident_sph_begin): Vel, FullTreeGravAccel, GravPM, TimeBinGravity, Hsml, DtHsml and Density are the
 * resident ones; only `vdisp` (a HOST array of n entries, in/out) travels */
int mpg_resident_sph_find_vel_disp(mpg_engine *eng, const mpg_particle_view *pv, const mpg_sph_times *T, const mpg_veldisp_params *par,
                                   const int *ActiveParticle, int64_t NumActiveParticle, double *vdisp);
/* statistics of the last call: [0] iterations of the gas loop, [1] gas targets summed over the iterations, [2] candidates found inside
 * the search radius (gas and black-hole passes), [3] candidates distance-tested, [4] gas targets that ended through the tight bracket
 * (Right - Left <= 5e-6 Left) with a count outside 39 .. 41 */
int mpg_veldisp_get_stats(mpg_engine *eng, int64_t stats[5]);
/* the loop's per-target results of the last call into host arrays of n entries (each may be NULL): the trial radius the final sums were
 * taken at (a black hole: its Hsml), the passes the target took (-1: not a target), its final count and maxcmpte; and the queue length
 * of the first queue_capacity iterations (0 beyond the last) */
int mpg_veldisp_export(mpg_engine *eng, int64_t n, double *radius, int32_t *iterations, int32_t *numngb, int32_t *maxcmpte, int64_t *queue_lengths,
                       int64_t queue_capacity);

/* ---- radiative cooling of gas: cooling_direct, libgadget/sfr_eff.c:463-514 (cooling_and_starformation, run.c:663-664) ---------
 * For every listed gas particle (Type == 0, not garbage, Mass > 0; sfr_eff.c:229) DoCooling (cooling.c:57-138) finds the internal energy
 * after the particle's hydro step dtime = dloga_bin[TimeBinHydro] / hubble by bracketing (x 1.1, / 1.1) and bisecting
 * u - u_old - LambdaNet(u) dt; every LambdaNet solves the ionisation network of cooling_rates.c (get_heatingcooling_rate :1248-1310,
 * get_equilib_ne / scipy_optimize_fixed_point :779-827, ne_internal :755-765) with the fits recomb = Cen92 / Verner96 / Badnell06 and
 * cooling = KWH92 / Enzo2Nyx / Sherwood, tabulated in 13 tables of 1000 entries exactly as init_cooling_rates does (:1153-1171) and
 * evaluated directly outside them.  The particle gets Ne, Entropy = unew / entropy_to_u(Density, a3inv) and Sfr = 0; one that was
 * reionised during its step (HIReionTemp > 0, zreion in [redshift, lastred[bin]), sfr_eff.c:488-501) is set to HIReionTemp instead.
 * The engine reads no files and evaluates no star-formation criterion: the caller decides who is listed (the particles for which
 * cooling_and_starformation takes the `else cooling_direct` branch, sfr_eff.c:270-271) and passes the step's UV background
 * (get_global_UVBG, cooling_rates.c:365-397), get_long_mean_free_path_heating(redshift) (cooling_qso_lightup.c:258) and per hydro bin
 * lastred = 1 / exp(loga_from_ti(Ti_Current - dti_from_timebin(bin))) - 1 (sfr_eff.c:483-484).
 * With a UV-fluctuation table loaded (mpg_set_uvf_table below) every row takes the background of get_local_UVBG_from_global at its own
 * position, and the HIReionTemp test reads the row's own zreion.
 * With an excursion-set model loaded and its two columns bound (mpg_set_excursion_set below) every row takes the background of
 * get_local_UVBG_from_J21 while redshift > ExcursionSetZStop.
 * Not carried: cooling_relaxed, star formation and winds (mpg_dev_cooling_and_starformation has them);
 * several ranks each call this form on their own gas (the loop is per particle).
 * Every loop is bounded: the two limits of 1000 are the reference's (cooling.c:32, cooling_rates.c:768); the two bracketing loops, which the
 * reference leaves unbounded, stop after 8192 steps.  A particle that hits a limit, or whose electron abundance is not finite, keeps its
 * Entropy / Ne / Sfr, counts in stats[5], and makes the call return non-zero after all other particles are done (the reference: endrun). */
/* struct UVBG, cooling.h:9-19 (same members, same order) */
typedef struct mpg_uvbg {
    double J_UV, gJH0, gJHep, gJHe0, epsH0, epsHep, epsHe0, self_shield_dens, zreion;
} mpg_uvbg;
typedef struct mpg_cooling_params {
    /* struct cooling_params, cooling_rates.h:23-58 (PhotoIonizationOn, PhotoIonizeFactor, UVRedshiftThreshold and HydrogenHeatAmp act in
     * get_global_UVBG / load_treecool only, i.e. on the caller's side; they are carried for completeness and not read) */
    int recomb;  /* enum RecombType: 0 Cen92, 1 Verner96, 2 Badnell06 */
    int cooling; /* enum CoolingType: 0 KWH92, 1 Enzo2Nyx, 2 Sherwood */
    int SelfShieldingOn;
    int PhotoIonizationOn;
    double fBar;
    double PhotoIonizeFactor;
    double CMBTemperature;
    double MinGasTemp;
    double UVRedshiftThreshold;
    double HydrogenHeatAmp;
    int HeliumHeatOn;
    double HeliumHeatThresh;
    double HeliumHeatAmp;
    double HeliumHeatExp;
    double rho_crit_baryon;
    /* struct cooling_units, cooling.h:32-44 */
    int CoolingOn;
    double density_in_phys_cgs;
    double uu_in_cgs;
    double tt_in_s;
    double units_rho_crit_baryon; /* cooling_units.rho_crit_baryon */
    /* of sfr_params (sfr_eff.c:69-71, 498, 505) */
    double sfr_MinGasTemp;
    double temp_to_u;
    double HIReionTemp;
    /* tests only: a limit for the fixed-point iteration of the network in place of its 1000; 0 = the reference's */
    int test_network_maxiter;
} mpg_cooling_params;
typedef struct mpg_cooling_step {
    mpg_uvbg uvbg;                      /* get_global_UVBG(redshift) */
    double long_mean_free_path_heating; /* get_long_mean_free_path_heating(redshift), erg/s/cm^3 */
    double lastred[47];                 /* per hydro time bin: the redshift at the start of the particle's step */
    double redshift;                    /* mpg_dev_cooling_state only (mpg_dev_cooling takes 1 / T->atime - 1) */
    double helium;                      /* mpg_dev_cooling_state only: helium mass fraction; 0 = 1 - HYDROGEN_MASSFRAC */
} mpg_cooling_step;
typedef struct mpg_cooling_arrays {
    const double *density;        /* SphP.Density */
    double *entropy;              /* in/out SphP.Entropy */
    double *ne;                   /* in/out SphP.Ne */
    double *sfr;                  /* in/out SphP.Sfr (set to 0 for every treated particle) */
    const double *metallicity;    /* SphP.Metallicity; NULL = 0 */
    const uint8_t *heiii_ionized; /* P.HeIIIionized; NULL = 0 */
    const uint8_t *tb_hydro;      /* P.TimeBinHydro; NULL = 0 */
} mpg_cooling_arrays;
/* set_coolpar / init_cooling (cooling_rates.c:1071, cooling.c:22-30): stores the parameters and fills the 13 rate tables */
int mpg_set_cooling_params(mpg_engine *eng, const mpg_cooling_params *par);
/* InitMetalCooling (cooling_uvfluc.c:265-305): the three bin vectors (of which, as in the reference, only the ends and the lengths
 * count) and NetCoolingRate[nz][nnh][nt] from HOST memory; zbins == NULL removes the table (MetalCoolFile == "") */
int mpg_set_metal_cooling_table(mpg_engine *eng, int nz, const double *zbins, int nnh, const double *nhbins, int nt, const double *tbins,
                                const double *rate);
/* on the bound particles (types from the bound table, garbage as type 7); arrays in particle order; d_active NULL = all particles;
 * atime, hubble and dloga_bin of T are read */
int mpg_dev_cooling(mpg_engine *eng, const mpg_cooling_arrays *A, const mpg_sph_times *T, const mpg_cooling_step *step, const int *d_active,
                    int64_t nactive);
/* host form: `pv` supplies Mass / Type / flags, `A` holds HOST arrays in particle order (the shim gathers SphP into them) */
int mpg_cooling(mpg_engine *eng, const mpg_particle_view *pv, double BoxSize, const mpg_cooling_arrays *A, const mpg_sph_times *T,
                const mpg_cooling_step *step, const int *ActiveParticle, int64_t NumActiveParticle);
/* on a resident gas run (mpg_resident_sph_begin): Density, Entropy and TimeBinHydro are the resident columns; `ne` (HOST, n entries,
 * in/out) travels, as do the optional HOST inputs metallicity and heiii_ionized (NULL = 0).  Sfr is not a resident column: the caller
 * zeroes it for the listed gas. */
int mpg_resident_sph_cooling(mpg_engine *eng, const mpg_particle_view *pv, const mpg_sph_times *T, const mpg_cooling_step *step,
                             const int *ActiveParticle, int64_t NumActiveParticle, double *ne, const double *metallicity,
                             const uint8_t *heiii_ionized);
/* the network alone, in physical cgs units (density in protons/cm^3, energy in erg/g), for n independent points on the device:
 * get_heatingcooling_rate with zero metallicity (erg/s/g), the temperature (get_temp, K) and the neutral hydrogen fraction
 * (get_neutral_fraction_phys_cgs) at the equilibrium; d_ne_inout holds ne / nH as the start value and returns the equilibrium.  The three
 * outputs may each be NULL.  GetNeutralFraction (cooling.c:166-176) of a snapshot is this call on density_in_phys_cgs / PROTONMASS *
 * rho and uu_in_cgs * u. */
int mpg_dev_cooling_state(mpg_engine *eng, int64_t n, const double *d_rho, const double *d_u, double *d_ne_inout, double *d_lambdanet,
                          double *d_temp, double *d_nh0, const mpg_cooling_step *step);
/* statistics of the last mpg_dev_cooling: [0] particles treated, [1] evaluations of the network (ne_internal) summed, [2] bisection steps
 * summed, [3] particles that ended on the energy floor, [4] particles in the HIReionTemp branch, [5] particles that hit a limit */
int mpg_cooling_get_stats(mpg_engine *eng, int64_t stats[6]);
/* the evaluations of the network of every particle in the last mpg_dev_cooling (host array of n entries; -1: not treated) */
int mpg_cooling_export(mpg_engine *eng, int64_t n, int32_t *evaluations);

/* ---- patchy reionisation: the UV-fluctuation table, libgadget/cooling_uvfluc.c:115-197 ------------------------------------------
 * UVFluctuationFile's Zreion_Table gives the reionisation redshift as a function of position.  With a table loaded, mpg_dev_cooling,
 * mpg_cooling and mpg_resident_sph_cooling (and the three forms of cooling_and_starformation) first evaluate it at the position of every
 * listed gas row (the bound positions; on a resident run the resident Pos) minus the offset below, into an engine-owned column
 * (mpg_uvf_export), and then give every row the background of get_local_UVBG_from_global: zreion < redshift: every rate of struct UVBG 0
 * and self_shield_dens the global one; otherwise the step's background; uvbg.zreion the local value in both cases, which is what the
 * HIReionTemp test reads.  The read is interp_eval_periodic (utils/interp.c:134-170) with interp_init_dim(0, BoxSize): trilinear, the
 * cells BoxSize / (Nside - 1) wide and wrapped after Nside of them, so the table's period is BoxSize Nside / (Nside - 1) as in the
 * reference.  A row whose position is not finite, or 2^31 cells or more from the origin (the reference: undefined), gets zreion = NaN
 * without a read of the table, keeps Entropy / Ne / Sfr, counts in stats[5] and makes the call return non-zero after all other rows are
 * done.  Without a table every call is bit for bit what it is without this section.  The excursion set (EXCUR_REION) is a
 * different model: its producer is mpg_dev_calculate_uvbg below, its consumer in this loop mpg_set_excursion_set. */
/* init_uvf_table (cooling_uvfluc.c:115-167) without the file: Zreion_Table[Nside][Nside][Nside], C order, from HOST memory; table == NULL
 * removes it.  Refused: Nside < 2, BoxSize <= 0, a non-finite entry, Table[0] outside [0.01, 100] (:164). */
int mpg_set_uvf_table(mpg_engine *eng, int64_t Nside, const double *table, double BoxSize);
/* PartManager->CurrentParticleOffset for the calls that follow; {0,0,0} until set */
int mpg_set_uvf_offset(mpg_engine *eng, const double offset[3]);
/* zreion of n arbitrary points on the device ([n][3] in, [n] out): interp_eval_periodic(&UVF.interp, pos - offset, UVF.Table).  What
 * get_neutral_fraction_sfreff (sfr_eff.c:580, 613) and stats.c:271 need before mpg_dev_cooling_state, which keeps taking one background:
 * the caller splits its points by zreion < redshift.  A point that cannot be evaluated (above) gets NaN, and the call returns non-zero
 * after all other points are done. */
int mpg_dev_uvf_zreion(mpg_engine *eng, int64_t n, const double *d_pos, double *d_zreion);
/* the zreion of every particle in the last cooling or cooling_and_starformation call with a table (host array of n entries; NaN: the row
 * was not evaluated, or could not be) */
int mpg_uvf_export(mpg_engine *eng, int64_t n, double *zreion);

/* ---- the excursion set's J21 in cooling and star formation: get_local_UVBG_from_J21 / get_local_UVBG, cooling_uvfluc.c:199-246 --------
 * The consumer of SphP.local_J21 / SphP.zreion, which mpg_dev_calculate_uvbg makes.  With a model loaded and redshift > ExcursionSetZStop,
 * the three forms of cooling and of cooling_and_starformation give every listed gas row the background
 *   J_UV = J21, zreion the row's, gJH0 = c.gJH0 J21, epsH0 = c.epsH0 J21 1.60218e-12, gJHe0 and epsHe0 likewise, gJHep = epsHep = 0,
 *   self_shield_dens = get_self_shield_dens(redshift) of the row's gJH0 (cooling_rates.c:345-361; 1e10 where gJH0 == 0),
 * and the HIReionTemp test (sfr_eff.c:488) reads the row's zreion.  At or below ExcursionSetZStop, with ExcursionSetReionOn == 0 and
 * without a model every call is bit for bit what it is without this section: the global background, or the UV-fluctuation table's.
 * A row whose J21 is NaN or negative, or whose zreion is NaN, keeps Entropy / Ne / Sfr, counts in stats[5] and makes the call return
 * non-zero after all other rows are done.  Not carried: several ranks, BHFeedbackUseTcool == 2. */
typedef struct mpg_excursion_set_params {
    /* struct UVFparams, cooling_uvfluc.c:25-30 (AlphaUV is recorded and not read: the caller has evaluated the coefficients at it) */
    int ExcursionSetReionOn;
    double ExcursionSetZStop;
    double AlphaUV;
    /* get_J21_coeffs(AlphaUV) as the reference returns it (cooling_rates.c:419-430): after pow(10, .) * PhotoIonizeFactor, the eps in
     * eV/s.  The two Hep members are carried for completeness and not read. */
    double gJH0, gJHe0, gJHep, epsH0, epsHe0, epsHep;
} mpg_excursion_set_params;
/* par == NULL removes the model.  The engine reads no file: the caller interpolates J21CoeffFile.  Refused: a coefficient that is not
 * finite or is negative, an ExcursionSetZStop that is not finite. */
int mpg_set_excursion_set(mpg_engine *eng, const mpg_excursion_set_params *par);
/* the two columns, doubles in particle order, for the calls that follow: the pointers mpg_dev_calculate_uvbg wrote local_J21 and zreion
 * through, so producer and consumer chain on the device.  They are bound for the particle table bound at this moment; a call on a table
 * of another size is refused.  NULL, NULL unbinds.  A call in the J21 mode with no columns bound is refused. */
int mpg_dev_set_excursion_columns(mpg_engine *eng, const double *d_local_J21, const double *d_zreion);
/* ... HOST arrays for the host forms (mpg_cooling, mpg_cooling_and_starformation): they travel with every such call, as DelayTime does */
int mpg_set_excursion_columns(mpg_engine *eng, const double *local_J21, const double *zreion);
/* ... HOST arrays of a resident gas run, uploaded now and in effect until the next call or the end of the stretch, as ne travels */
int mpg_resident_sph_set_excursion_columns(mpg_engine *eng, const double *local_J21, const double *zreion);
/* get_local_UVBG for n arbitrary points on the device: d_out[n] from d_J21[n] and d_zreion[n] at `redshift` with the background of
 * `global` below ExcursionSetZStop or without a model (the UV-fluctuation table is not read here: mpg_dev_uvf_zreion has it).  What
 * get_neutral_fraction_sfreff and stats.c:271 need before mpg_dev_cooling_state.  A point whose J21 is NaN or negative or whose zreion is
 * NaN gets a struct of NaNs, and the call returns non-zero after all other points are done. */
int mpg_dev_excursion_uvbg(mpg_engine *eng, int64_t n, const double *d_J21, const double *d_zreion, double redshift, const mpg_uvbg *global,
                           mpg_uvbg *d_out);

/* ---- return of stellar mass and metals to the gas: metal_return, libgadget/metal_return.c (run.c:613) ----------------------------
 * For every active star (Type == 4, not garbage) with massgenerated >= 1e-3 (Mass + TotalMassReturned) (metals_haswork, :714-724):
 *   stellar_density (:930-1006)  the radius loop of treewalk_do_hsml_loop over the GAS around the star, ten trial radii per pass (effhsml
 *       :778-804) and ngb_narrow_down between the passes, until the kernel-weighted neighbour number Ngb = sum wk kernel_volume is within
 *       GetNumNgb +- MaxNgbDeviation (the kernel and eta of mpg_set_densitypar, i.e. mpg_get_numngb) or Right - Left < 1e-4 Left.  Hsml
 *       is assigned on every pass; StarVolumeSPH = sum (Mass_j / Density_j) (x wk with SPHWeighting) is the one of the trial radius
 *       closest to the wanted number, as in the reference (:848).
 *   the return walk (:637-709)  every gas particle with 0 < r < Hsml receives returnfraction = wk (Mass_j / Density_j) / StarVolumeSPH
 *       (wk = 1 without SPHWeighting) of massgenerated, metalgenerated and speciesgenerated[9]; the star loses what was accepted, adds
 *       it to TotalMassReturned and takes LastEnrichmentMyr = stellarage (:623-631).
 * The yields of a stellar population over its step (metal_return_init, metal_yield: quadrature over yield tables) are the caller's: per
 * star the engine receives massgenerated (priv->MassReturn), metalgenerated and speciesgenerated as metal_return_copy leaves them
 * (:581-611: scaled by the initial mass, negatives clamped) and stellarage.
 * THE CAP.  The reference lets a gas particle take a contribution iff P.Mass + thismass <= MaxGasMass on the RUNNING mass, under a
 * spinlock per particle: when several contributions of one call would each fit alone but not together, which of them it accepts depends
 * on the order its threads arrive in.  The engine tests every contribution against the mass at CALL ENTRY and sums the accepted ones per
 * gas particle (Mass / Density is invariant under the reference's update, so every returnfraction is the reference's):
 *     Mnew = M + dM, Metals_k = (Metals_k M + dMetals_k) / Mnew, Metallicity likewise, Density *= Mnew / M, Mass = (float)Mnew.
 * That equals the reference's sequential update in exact arithmetic wherever the reference's own result does not depend on thread order.
 * ERRORS: a target with Hsml <= 0 (the reference repairs it from a tree node the star is not in, :786-791: the caller repairs Hsml
 * before the call), a target that ends with StarVolumeSPH == 0 (endrun(3)), more than 400 iterations (endrun(1155)).
 * THE TREE: the call runs on the engine's CURRENT tree, which must contain the gas (it is the tree hydro_force has just used); it builds
 * no tree and leaves this one in place - the gas tree carries no moment that depends on a mass.  The engine's tree-order copies of the
 * masses are those of the last build: the next tree build refreshes them.  With no target nothing is read beyond the queue pass, nothing
 * is written and no tree is demanded.  Garbage and swallowed rows carry type 7 (as in every dev call); black holes in the tree are skipped.
 * One rank only: there is no mpg_dist_* form. */
typedef struct mpg_metal_params {
    int SPHWeighting;       /* MetalParams.SPHWeighting */
    double MaxNgbDeviation; /* MetalParams.MaxNgbDeviation */
    double MaxGasMass;      /* 4 * AvgGasMass (metal_return.c:535) */
} mpg_metal_params;
/* all arrays in particle order, n entries (x 9 where noted); every one is required except the two outputs */
typedef struct mpg_metal_arrays {
    const double *massgenerated;    /* stars: mass returned by the population this step (priv->MassReturn) */
    const double *metalgenerated;   /* stars: InitialMass * total_z_yield, >= 0 */
    const double *speciesgenerated; /* stars: [n][9] InitialMass * MetalSpeciesGenerated, >= 0 */
    const double *stellarage;       /* stars: priv->StellarAges (Myr) */
    float *mass;                    /* in/out P.Mass (float, as in the reference) of stars and gas */
    double *hsml;                   /* in/out P.Hsml of the stars */
    double *totalmassreturned;      /* in/out STARP.TotalMassReturned */
    double *lastenrichment;         /* in/out STARP.LastEnrichmentMyr */
    double *density;                /* in/out SphP.Density */
    double *metallicity;            /* in/out SphP.Metallicity */
    double *metals;                 /* in/out [n][9] SphP.Metals */
    double *massreturned;           /* out, optional: what every target star actually returned */
    double *starvolume;             /* out, optional: StarVolumeSPH of every target star */
} mpg_metal_arrays;
int mpg_set_metal_params(mpg_engine *eng, const mpg_metal_params *par);
/* on the bound particles and the current tree; d_active NULL = all particles */
int mpg_dev_metal_return(mpg_engine *eng, const mpg_metal_arrays *A, const int *d_active, int64_t nactive);
/* host form: `pv` supplies Pos / Mass / Type / flags and receives the new Mass (A->mass is not read); the other members of `A` are HOST
 * arrays in particle order.  The gas tree is (re)built as mpg_density builds it, before the call knows whether it has a target: in this
 * form a call without one still pays the build of the gas tree ("no tree is demanded" above holds for the dev and resident forms). */
int mpg_metal_return(mpg_engine *eng, const mpg_particle_view *pv, double BoxSize, const mpg_metal_arrays *A, const int *ActiveParticle,
                     int64_t NumActiveParticle);
/* on a resident gas run (mpg_resident_sph_begin), on its current tree: Pos, Mass, Hsml and Density are the resident columns and are updated
 * there (A->mass and A->density are not read); the new Mass is also written into the records of `pv`, which the end of the resident
 * stretch does not fetch.  The metal columns and the per-star members of `A` (HOST arrays) travel.  The STARS' Hsml is read and written by
 * this call alone, so A->hsml (HOST, optional) carries it both ways: its rows of type 4 replace the resident column's before the call (a
 * caller's repair of Hsml == 0 arrives so) and the whole resident column comes back into it afterwards; NULL: the resident column as it is. */
int mpg_resident_sph_metal_return(mpg_engine *eng, const mpg_particle_view *pv, const mpg_metal_arrays *A, const int *ActiveParticle,
                                  int64_t NumActiveParticle);
/* statistics of the last call: [0] iterations of the radius loop, [1] targets summed over the iterations, [2] gas candidates found inside
 * the search radius (both walks), [3] candidates distance-tested, [4] contributions refused by the cap, [5] targets that ended through
 * the tight bracket with a neighbour number outside the window */
int mpg_metals_get_stats(mpg_engine *eng, int64_t stats[6]);
/* device time of the last call (zeros when it had no target), in ms, from events on the engine's stream: [0] the radius loop (all iterations, with
 * its read-backs), [1] the return walk with the clearing of its accumulators, [2] the apply pass */
int mpg_metals_get_times(mpg_engine *eng, double ms[3]);
/* the loop's per-target results of the last call into host arrays of n entries (each may be NULL): the trial radius the final sums were
 * taken at, the passes the target took (-1: not a target), its final maxcmpte and `close`; and the queue length of the first
 * queue_capacity iterations (0 beyond the last) */
int mpg_metals_export(mpg_engine *eng, int64_t n, double *radius, int32_t *iterations, int32_t *maxcmpte, int32_t *close, int64_t *queue_lengths,
                      int64_t queue_capacity);

/* ---- black-hole accretion, mergers and feedback: blackhole(), libgadget/blackhole.c:215-370 (run.c:660) ----------------------------
 * Everything of blackhole() between its dynamical-friction calls and its file output, for the active, not swallowed black holes
 * (blackhole_haswork, :185-188), on the engine's CURRENT tree, which must hold gas AND black holes and carry the hmax moments of the Hsml
 * passed here (the search is the symmetric one: a pair interacts inside max(Hsml_i, Hsml_j)):
 *   the accretion walk (:471-649)  per target the kernel-weighted sums SmoothedEntropy, GasVel (SPH_VelPred), FeedbackWeightSum, MgasEnc
 *       and `encounter`; every gas particle inside Hsml with table[ID_gas % size] < (BH_Mass - BHPartMass) wk / Density is marked for the
 *       target, every black hole closer than 2 FORCE_SOFTENING / 2.8 that passes check_grav_bound (unless MergeGravBound == 0 or
 *       repositioning is on) likewise when the target is eligible (larger ID than the marked one, or the marked one is inactive).  A mark
 *       is the LARGEST ID + 1 over the candidates (64-bit atomic maximum), whatever the order of arrival.  For gas that is the
 *       reference's result.  For black holes the reference compares the stored ID + 1 with the newcomer's ID (:548), so two candidate
 *       swallowers with CONSECUTIVE IDs leave its result to the order its threads arrive in; the engine keeps the larger.
 *   its post-process (:373-468)  Bondi Mdot with the Eddington cap, Mass += Mdot dtime, DragAccel (BH_DRAG 0 / 1 / 2), the bookkeeping of
 *       the kinetic channel (KEflag, KineticFdbkEnergy).
 *   the feedback walk (:746-902) for the targets that are not themselves marked: marked black holes and marked gas are swallowed
 *       (Swallowed / IsGarbage in `flags`, SwallowID, SwallowTime, the swallower's sums of mass, momentum, BHP.Mass and CountProgs), the
 *       unmarked gas inside Hsml gives minTimeBin and receives thermal energy or a kick.  Energy and kicks are summed per gas particle
 *       with fp64 atomics; ONE apply pass per call turns the energy sum into entropy, u = min(u + sum e / Mass, u(5e8 K)) - in exact
 *       arithmetic the reference's capped additions in any order, all additions being positive - and adds the velocity sum.
 *   its post-process (:955-990)  BHP.Mass, the momentum-conserving velocity, the Mtrack / P.Mass rule, KineticFdbkEnergy reset.
 * NOT CARRIED (an error return naming the setting; the shim keeps the CPU walks): BlackHoleFeedbackMethod with BH_FEEDBACK_OPTTHIN,
 * BHFeedbackUseTcool == 2.  Dynamical friction and repositioning (bhdynfric.c) are not part of this call: DFAccel arrives as data, from
 * mpg_dev_blackhole_dynfric (below), which blackhole() calls first.
 * With no target nothing is read beyond the queue pass, nothing is written and no tree is demanded.  Garbage and swallowed rows carry
 * type 7 (as in every dev call).  One rank only: there is no mpg_dist_* form. */
typedef struct mpg_blackhole_params {
    double BlackHoleAccretionFactor, BlackHoleFeedbackFactor, BlackHoleEddingtonFactor; /* struct BlackholeParams, blackhole.c:28-54 */
    int BlackHoleFeedbackMethod; /* enum BlackHoleFeedbackMethod, blackhole.h:47-53: SPLINE 0x4, MASS 0x8, OPTTHIN 0x20 */
    int BlackHoleKineticOn;
    double BHKE_EddingtonThrFactor, BHKE_EddingtonMFactor, BHKE_EddingtonMPivot, BHKE_EddingtonMIndex, BHKE_EffRhoFactor, BHKE_EffCap,
        BHKE_InjEnergyThr, BHKE_SfrCritOverDensity;
    int MergeGravBound, BH_DRAG;
    double SeedBHDynMass;
    int BlackHoleRepositionEnabled; /* BHGetRepositionEnabled(): mergers skip check_grav_bound */
    int WindDecouple;               /* HAS(wind_params.WindModel, WIND_DECOUPLE_SPH): gas with DelayTime > 0 is skipped */
    int StarformationOn, BHFeedbackUseTcool;
    double PhysDensThresh, OverDensThresh; /* sfr_params, for sfreff_on_eeqos (sfr_eff.c:535-551) */
    double ForceSoftening;                 /* FORCE_SOFTENING(); <= 0: the engine's (mpg_force_softening) */
    double GravInternal, HubbleParam, OmegaBaryon, Hubble; /* Cosmology */
    double UnitTime_in_s, UnitVelocity_in_cm_per_s, uu_in_cgs; /* UnitSystem; uu_in_cgs = UnitEnergy_in_cgs / UnitMass_in_g */
} mpg_blackhole_params;
/* all arrays in particle order, n entries (x 3 where noted).  Slot members (SphP / BHP) are indexed by PARTICLE; entries of rows of other
 * types are ignored.  Required unless marked optional. */
typedef struct mpg_blackhole_arrays {
    /* read */
    const uint64_t *id;          /* P.ID */
    const double *gacc;          /* [n][3] P.FullTreeGravAccel */
    const double *gpm;           /* [n][3] P.GravPM */
    const double *hydroacc;      /* [n][3] SphP.HydroAccel */
    const uint8_t *tb_hydro;     /* P.TimeBinHydro */
    const uint8_t *tb_grav;      /* P.TimeBinGravity */
    const double *hsml;          /* P.Hsml of gas and black holes */
    const double *density;       /* SphP.Density / BHP.Density */
    const double *delaytime;     /* SphP.DelayTime */
    const double *dfaccel;       /* [n][3] BHP.DFAccel */
    const double *vdisp;         /* BHP.VDisp */
    const uint8_t *active_hydro; /* optional: is_timebin_active(TimeBinHydro, Ti_drift) of the black holes; NULL: all active */
    /* in / out */
    float *mass;                 /* P.Mass (float, as in the reference) */
    double *vel;                 /* [n][3] P.Vel */
    double *entropy;             /* SphP.Entropy */
    uint8_t *flags;              /* bit 0 IsGarbage, bit 1 Swallowed */
    double *bh_mass;             /* BHP.Mass */
    double *mtrack;              /* BHP.Mtrack */
    double *kineticfdbkenergy;   /* BHP.KineticFdbkEnergy */
    int32_t *countprogs;         /* BHP.CountProgs */
    /* out: written for the targets (swallowid / swallowtime / encounter also for the black holes swallowed, bhheated for heated gas) */
    double *mdot;                /* BHP.Mdot */
    double *dragaccel;           /* [n][3] BHP.DragAccel */
    int32_t *encounter;          /* BHP.encounter */
    int32_t *mintimebin;         /* BHP.minTimeBin (targets of the feedback walk) */
    uint64_t *swallowid;         /* BHP.SwallowID */
    double *swallowtime;         /* BHP.SwallowTime */
    uint8_t *bhheated;           /* P.BHHeated: set to 1, never cleared */
    /* out, optional: the walks' private arrays (struct BHPriv), what collect_BH_info writes and the tests read */
    double *feedbackweightsum, *bh_entropy, *gasvel /* [n][3] */, *mgasenc;
    int32_t *keflag;
    double *accreted_mass, *accreted_bhmass, *accreted_momentum /* [n][3] */;
    uint64_t *sph_swallowid, *bh_swallowid; /* the marks of every gas particle / black hole of the tree (others 0) */
} mpg_blackhole_arrays;
/* the step's RandTable (set_random_numbers, run.c:582-584) as data: get_random_number(id) = table[id % size] (system.c:55-61).  Copied. */
int mpg_set_random_table(mpg_engine *eng, const double *table, int64_t size);
int mpg_set_blackhole_params(mpg_engine *eng, const mpg_blackhole_params *par);
/* on the bound particles and the current tree; d_active NULL = all particles.  T supplies FgravkickB, gravkicks, hydrokicks, dloga_bin,
 * atime and hubble.  An error when the tree lacks gas, black holes or hmax, and before mpg_set_random_table / mpg_set_blackhole_params. */
int mpg_dev_blackhole(mpg_engine *eng, const mpg_blackhole_arrays *A, const mpg_sph_times *T, const int *d_active, int64_t nactive);
/* host form: `pv` supplies Pos / Mass / Type / flags and receives the new Mass and flags (A->mass is not read); the members of `A` are
 * HOST arrays in particle order, A->flags in / out like the records'.  The queue pass runs first: without a target no array travels; with
 * one, the tree of gas and black holes and its hmax moments (from A->hsml) are built. */
int mpg_blackhole(mpg_engine *eng, const mpg_particle_view *pv, double BoxSize, const mpg_blackhole_arrays *A, const mpg_sph_times *T,
                  const int *ActiveParticle, int64_t NumActiveParticle);
/* on a resident gas run (mpg_resident_sph_begin): Pos, Mass, Vel, the accelerations (HydroAccel: the resident hydroacc_out), the time bins,
 * Hsml, Density and Entropy are the resident columns and are updated in place (those members of `A` are not read); the type column takes 7
 * for the rows swallowed; flags and the new Mass are also written into the records of `pv`.  Every other member of `A` (HOST arrays)
 * travels, and only when the queue pass found a target.  When the call has a target and the current tree is not one of gas and black holes with hmax (find_vel_disp leaves the DM tree),
 * that tree is built. */
int mpg_resident_sph_blackhole(mpg_engine *eng, const mpg_particle_view *pv, const mpg_blackhole_arrays *A, const mpg_sph_times *T,
                               const int *ActiveParticle, int64_t NumActiveParticle);
/* statistics of the last call: [0] gas swallowed, [1] black holes swallowed, [2] candidates distance-tested and [3] neighbours found by the
 * accretion walk, [4], [5] the same of the feedback walk, [6] targets of the accretion walk, [7] of the feedback walk */
int mpg_blackhole_get_stats(mpg_engine *eng, int64_t stats[8]);
/* device time of the last call (zeros when it had no target), in ms, from events on the engine's stream: [0] the accretion walk with its
 * post-process, [1] the feedback walk with its post-process and the clearing of the accumulators, [2] the apply pass.  The queue pass of
 * the feedback walk and the read-back of its length (a host round trip between [0] and [1]) are in none of the three. */
int mpg_blackhole_get_times(mpg_engine *eng, double ms[3]);

/* ---- black-hole dynamical friction and the potential minimum: blackhole_dynfric + blackhole_dfaccel, libgadget/bhdynfric.c
 * (blackhole.c:254-256, the first two calls of blackhole()) -----------------------------------------------------------------------------
 * THE TREE: the call builds the tree of its type mask itself, without moments - stars and black holes, with the DM when
 * BH_DynFrictionMethod > 1, with the gas when it is 3, every type when BlackHoleRepositionEnabled (blackhole_dynfric_treemask, :66-81) -
 * and that tree is the engine's current tree when the call returns, as after find_vel_disp.  With method 0 and no repositioning nothing is
 * read or written and no tree is built; with no target no tree is built either.
 * Targets: the listed, not swallowed black holes; with method > 0 those whose active_dynfric byte is set (the caller's
 * is_timebin_active(BHP.TimeBinDynFric, Ti_Current); NULL: all); with method 0 and repositioning every listed black hole, and only the
 * potential minimum is searched (blackhole_minpot).  One pass per target over every particle of the tree with r^2 < Hsml^2 (asymmetric):
 *   the potential minimum   the particle of smallest Potential, starting from the target's own Potential and position; a neighbour wins
 *       only when strictly lower.  minpot / minpotpos are always written for a target; minpotvel (the neighbour's raw Vel) and
 *       jumptominpot = BlackHoleRepositionEnabled only when a lower neighbour exists.  THE ONE DEFINED DIFFERENCE: among neighbours of
 *       EQUAL lowest potential the reference keeps the one it visits first; the engine keeps the one of smaller particle index.
 *   the friction sums (method > 0) over the stars, the DM (method > 1) and the gas (method 3): sum m wk, sum m wk v[k], sum m wk v[k]^2
 *       with wk = density_kernel_wk(r / Hsml) and v = DM_VelPred / SPH_VelPred (gas); then rms = sqrt(rms / density), vel /= density, or,
 *       for density == 0, the target is counted in ZeroDF.  df_density / df_vel / df_rmsvel are overwritten for targets and untouched
 *       for every other row.
 * Then, with method > 0, blackhole_compute_dfaccel (:86-145) for EVERY listed black hole, target or not, from the stored sums; a
 * non-finite relative velocity (the reference's endrun(6)) is an error return.  One rank only: there is no mpg_dist_* form. */
typedef struct mpg_bh_dynfric_params {
    int BH_DynFrictionMethod; /* 0 off, 1 stars, 2 + DM, 3 + gas */
    int BH_DFBoostFactor;
    double BH_DFbmax;
    int BlackHoleRepositionEnabled;
    double GravInternal;
    int DensityKernelType;    /* GetDensityKernelType() */
} mpg_bh_dynfric_params;
/* all arrays in particle order, n entries (x 3 where noted); entries of rows that are no black holes are ignored in the BHP members */
typedef struct mpg_bh_dynfric_arrays {
    /* read */
    const double *vel;             /* [n][3] P.Vel */
    const double *gacc;            /* [n][3] P.FullTreeGravAccel (method > 0) */
    const double *gpm;             /* [n][3] P.GravPM (method > 0) */
    const double *hydroacc;        /* [n][3] SphP.HydroAccel (method 3) */
    const uint8_t *tb_grav;        /* P.TimeBinGravity (method > 0) */
    const uint8_t *tb_hydro;       /* P.TimeBinHydro (method 3) */
    const double *hsml;            /* P.Hsml of the black holes */
    const double *potential;       /* P.Potential */
    const double *bh_mass;         /* BHP.Mass (method > 0: ZeroDFMass) */
    const uint8_t *active_dynfric; /* optional: is_timebin_active(BHP.TimeBinDynFric, Ti_Current); NULL: all */
    /* in / out (method > 0; jumptominpot always) */
    double *df_density;            /* BHP.DF_SurroundingDensity */
    double *df_vel;                /* [n][3] BHP.DF_SurroundingVel */
    double *df_rmsvel;             /* BHP.DF_SurroundingRmsVel */
    int32_t *jumptominpot;         /* BHP.JumpToMinPot */
    /* out */
    double *minpot;                /* BHP.MinPot */
    double *minpotpos;             /* [n][3] BHP.MinPotPos */
    double *minpotvel;             /* [n][3] BHP.MinPotVel */
    double *dfaccel;               /* [n][3] BHP.DFAccel (method > 0) */
} mpg_bh_dynfric_arrays;
int mpg_set_bh_dynfric_params(mpg_engine *eng, const mpg_bh_dynfric_params *par);
/* on the bound particles; d_active NULL = all particles.  T supplies FgravkickB, gravkicks, hydrokicks and atime. */
int mpg_dev_blackhole_dynfric(mpg_engine *eng, const mpg_bh_dynfric_arrays *A, const mpg_sph_times *T, const int *d_active, int64_t nactive);
/* host form: `pv` supplies Pos / Mass / Type; the members of `A` are HOST arrays.  The queue pass runs first: without a target (and, for
 * method > 0, without a listed black hole) no array travels. */
int mpg_blackhole_dynfric(mpg_engine *eng, const mpg_particle_view *pv, double BoxSize, const mpg_bh_dynfric_arrays *A, const mpg_sph_times *T,
                          const int *ActiveParticle, int64_t NumActiveParticle);
/* on a resident gas run: Pos, Mass, Vel, the accelerations (HydroAccel: the resident hydroacc_out), the time bins, Hsml and Potential are
 * the resident columns (those members of `A` are not read); the per-black-hole members (HOST arrays) travel.  mpg_resident_sph_blackhole
 * after this call finds another tree than its own and builds it. */
int mpg_resident_sph_blackhole_dynfric(mpg_engine *eng, const mpg_particle_view *pv, const mpg_bh_dynfric_arrays *A, const mpg_sph_times *T,
                                       const int *ActiveParticle, int64_t NumActiveParticle);
/* statistics of the last call: [0] targets, [1] candidates distance-tested, [2] neighbours found, [3] ZeroDF (targets with no density),
 * [4] listed black holes; *zerodfmass their summed BHP.Mass (may be NULL) */
int mpg_bh_dynfric_get_stats(mpg_engine *eng, int64_t stats[5], double *zerodfmass);
/* device time of the last call in ms from events on the engine's stream: [0] the walk with its post-process, [1] the DFAccel pass */
int mpg_bh_dynfric_get_times(mpg_engine *eng, double ms[2]);
/* the walk's per-target state of the last call, n entries each (any may be NULL): the raw sums before the post-process ([n][5]: sum m wk,
 * sum m wk v[3], sum m wk v^2), the particle of the potential minimum (-1: none lower than the target), the tree particles inside Hsml.
 * Rows that were no targets hold -1 in minidx and numngb. */
int mpg_bh_dynfric_export(mpg_engine *eng, int64_t n, double *rawsums, int32_t *minidx, int32_t *numngb);

/* ---- the wind model: winds_and_feedback, winds_subgrid, winds_evolve, libgadget/winds.c (sfr_eff.c:235, 283, 391-392) --------------
 * winds_and_feedback (:298-371) for the NEW STARS of a step, given as a list of rows, on the engine's CURRENT tree, which must contain the
 * gas.  No hmax is needed: both searches are asymmetric inside the star's Hsml.  With WIND_SUBGRID set or an empty list nothing is read,
 * nothing is written and no tree is demanded.
 *   the weight walk (:414-450)    TotalWeight = sum of P.Mass over the gas with r <= Hsml and DelayTime <= 0.  A candidate is a row of the
 *       tree whose CURRENT type is 0: black holes in the tree, type-7 rows and gas converted since the tree was built are skipped.  Mass is
 *       the column bound with mpg_dev_bind_particles as it is NOW, not the tree-order copy of the last build.  The walk counts the eligible
 *       neighbours (the reference's nvisited), which sizes the list of potential kicks.
 *   the feedback walk (:513-569)  same search, same eligibility; no candidate when TotalWeight == 0 or Vdisp <= 0.  get_wind_params
 *       (:493-511) once per star; p = windeff Mass_star / TotalWeight; a pair is a potential kick iff
 *       table[(ID_star + ID_gas) % size] < p and v > 0 (the sum wraps as unsigned 64-bit; the table of mpg_set_random_table).
 *   the nearest-star rule (:207-224, :338-356)  a gas particle takes the kick of the candidate of smallest r = sqrt(r2); ties go to the
 *       smaller star ID.  Taken with two 64-bit atomic minima (the bits of r, then the star ID among the entries at that r) and one apply
 *       pass over the list: the result does not depend on the order of arrival and no lane waits for another.
 *   the kick (:453-490)  Vel += v dir with theta = acos(2 t[(ID_gas + 3) % size] - 1), phi = 2 pi t[(ID_gas + 4) % size];
 *       Entropy += therm / enttou, enttou = pow(Density / atime^3, GAMMA_MINUS1) / GAMMA_MINUS1; with MaxWindFreeTravelTime > 0
 *       DelayTime = min(WindFreeTravelLength / (v / atime), MaxWindFreeTravelTime).
 * ERRORS: a listed row outside the table or not of type 4 (endrun(5), :406-407), no random table, no parameters, a tree without the gas, a
 * search that overflowed its stack, a kick list without room (endrun(5), :559-561): all of these are found before Vel, Entropy or
 * DelayTime is written.  A non-finite kick velocity or DelayTime ("Odd v", endrun(5), :350-355) is found AFTER the kicks have been
 * applied, as in the reference, which then ends the run: Vel, Entropy and DelayTime are undefined after this error.
 * One rank only: there is no mpg_dist_* form, and no form on a resident gas run. */
typedef struct mpg_wind_params {
    int WindModel;               /* enum WindModel, winds.h:13-20: SUBGRID 1, DECOUPLE_SPH 2, USE_HALO 4, FIXED_EFFICIENCY 8, ISOTROPIC 512 */
    double WindEfficiency, WindSigma0, WindSpeedFactor, MinWindVelocity, WindThermalFactor, WindFreeTravelLength;
    double WindSpeed;            /* after init_winds: already divided by sqrt(WindEfficiency) for WIND_FIXED_EFFICIENCY */
    double MaxWindFreeTravelTime;/* in internal units (after init_winds) */
    double WindFreeTravelDensThresh;
} mpg_wind_params;
/* all arrays in particle order, n entries (x 3 where noted).  Slot members are indexed by PARTICLE. */
typedef struct mpg_wind_arrays {
    /* read */
    const uint64_t *id;      /* P.ID */
    const double *hsml;      /* P.Hsml of the stars (winds_and_feedback only) */
    const double *vdisp;     /* STARP.VDisp of the stars (winds_and_feedback); SPHP.VDisp of the gas (winds_subgrid) */
    const double *density;   /* SPHP.Density */
    const uint8_t *tb_hydro; /* P.TimeBinHydro (winds_evolve only) */
    /* in / out */
    double *vel;             /* [n][3] P.Vel */
    double *entropy;         /* SPHP.Entropy */
    double *delaytime;       /* SPHP.DelayTime */
    /* out, optional (winds_and_feedback) */
    double *totalweight;     /* TotalWeight of every listed star */
    uint64_t *kick_star;     /* ID + 1 of the star whose kick a gas particle received, 0 for every other row (all n are written) */
} mpg_wind_arrays;
/* an error (the reference's endrun(1)) for a model with neither WIND_FIXED_EFFICIENCY nor WIND_USE_HALO */
int mpg_set_wind_params(mpg_engine *eng, const mpg_wind_params *par);
/* on the bound particles and the current tree; d_newstars: nnew rows (device).  Required: id, hsml, vdisp, density, vel, entropy, delaytime */
int mpg_dev_winds_and_feedback(mpg_engine *eng, const mpg_wind_arrays *A, const int *d_newstars, int64_t nnew, double atime);
/* host form: `pv` supplies Pos / Mass / Type / flags, the members of `A` and NewStars are HOST arrays.  The gas tree is built as
 * mpg_density builds it unless the list is empty or WIND_SUBGRID is set: then nothing travels. */
int mpg_winds_and_feedback(mpg_engine *eng, const mpg_particle_view *pv, double BoxSize, const mpg_wind_arrays *A, const int *NewStars,
                           int64_t NumNewStars, double atime);
/* winds_subgrid / winds_make_after_sf (:275-295, :571-589): one lane per listed gas particle (d_maybewind NULL: rows 0 .. n - 1, as the
 * reference's NULL list); prob = 1 - exp(-windeff sm / Mass), sm = d_stellarmass[row] (by PARTICLE, not by slot); kicked when
 * table[(ID + 2) % size] < prob, with the kick above and the particle's own vdisp.  Nothing unless WIND_SUBGRID is set.  Required: id,
 * vdisp, density, vel, entropy, delaytime. */
int mpg_dev_winds_subgrid(mpg_engine *eng, const mpg_wind_arrays *A, const int *d_maybewind, int64_t n, const double *d_stellarmass, double atime);
/* winds_evolve (:374-391) for the listed rows of type 0 (d_active NULL: every row): DelayTime = 0 when DelayTime > 0 and
 * Density / atime^3 < WindFreeTravelDensThresh; else the clamp to MaxWindFreeTravelTime and
 * DelayTime = max(DelayTime - dloga_bin[TimeBinHydro] / hubble, 0).  T supplies atime, hubble and dloga_bin.  Required: density,
 * tb_hydro, delaytime. */
int mpg_dev_winds_evolve(mpg_engine *eng, const mpg_wind_arrays *A, const mpg_sph_times *T, const int *d_active, int64_t nactive);
/* statistics of the last mpg_dev_winds_and_feedback: [0] stars, [1] candidates distance-tested by the weight walk, [2] eligible neighbours
 * (nvisited), [3] potential kicks, [4] kicks applied, [5] kicks discarded; *maxvel (may be NULL) the velocity of the kick applied to the
 * lowest particle index, which is what the reference prints as "Vel" (0 without a kick).  After mpg_dev_winds_subgrid: [0] listed rows,
 * [4] kicks applied. */
int mpg_winds_get_stats(mpg_engine *eng, int64_t stats[6], double *maxvel);
/* DECOUPLED WIND GAS IN hydro_force.  With WIND_DECOUPLE_SPH in the WindModel of mpg_set_wind_params AND a DelayTime column, gas with
 * DelayTime > 0 (winds_is_particle_decoupled, :113-120) takes no part in the hydro forces:
 *   as a source (hydra.c:360-363) it contributes nothing to any target: no acceleration, no DtEntropy, no MaxSignalVel;
 *   as a target (hydro_postprocess -> winds_decoupled_hydro, :122-136) its walk still runs; it then gets HydroAccel = 0, DtEntropy = 0 and
 *       MaxSignalVel = hsml_c max(2 windspeed, MaxSignalVel), windspeed = WindSpeed atime fac_mu, fac_mu = atime^(3 (GAMMA - 1) / 2) / atime,
 *       hsml_c = cbrt(WindFreeTravelDensThresh / Density) atime.
 * Without the bit or without a column hydro_force launches the kernels it launched before there was such a rule.  The column (SphP.DelayTime
 * by particle, n entries) arrives through one of three setters; NULL unbinds:
 *   mpg_dev_set_delaytime           a device array, read by mpg_dev_hydro_force (the caller keeps it alive)
 *   mpg_set_delaytime               a host array, uploaded by every mpg_hydro_force (staged or resident) and in effect for that call
 *   mpg_resident_sph_set_delaytime  a host array, uploaded NOW into the engine and in effect for the mpg_hydro_force calls of the resident gas
 *                                   run until the next such call or mpg_resident_sph_end (the kicks of winds_and_feedback change DelayTime
 *                                   on the host: the caller hands the column over again after them)
 * The density loop's rule for black-hole targets (density.c:455) is not carried. */
int mpg_dev_set_delaytime(mpg_engine *eng, const double *d_delaytime);
int mpg_set_delaytime(mpg_engine *eng, const double *delaytime);
int mpg_resident_sph_set_delaytime(mpg_engine *eng, const double *delaytime);
/* the potential kicks of the last mpg_dev_winds_and_feedback, star by star in list order, while the tree of that call is
 * still the engine's: the rows of the star and of the gas particle of the first `capacity` entries into host arrays (either may be NULL),
 * *count the length of the list */
int mpg_winds_export(mpg_engine *eng, int64_t capacity, int32_t *star, int32_t *gas, int64_t *count);
/* device time of the last mpg_dev_winds_and_feedback in ms (zeros when it had nothing to do), from events on the engine's stream: [0] the
 * weight walk, [1] the feedback walk with the clearing of its per-particle words, [2] the resolve and apply passes.  The read-back of
 * the neighbour count that sizes the list (a host round trip between [0] and [1]) is in none of the three. */
int mpg_winds_get_times(mpg_engine *eng, double ms[3]);

/* ---- helium reionisation by quasar bubbles: do_heiii_reionization, libgadget/cooling_qso_lightup.c (run.c:622, 632-635) -------------
 * turn_on_quasars (:523-638) for ONE rank, after the caller's guards of :641-659.  The engine reads no file: the caller interpolates the
 * history table (desired_ion_frac), evaluates Q_inst and the rhobar arithmetic of :550-554 (non_overlapping_bubble_number).
 *   flash (:539-548)   with desired_ion_frac > heIIIreion_finish_frac every row of type 0 goes through ionize_single_particle (:388-408):
 *       a row with the flag is left alone; otherwise flag = 1 and Entropy += deltau / uu_in_cgs / entropytou,
 *       deltau = qso_inst_heating (1 - HYDROGEN_MASSFRAC) / (PROTONMASS HEMASS), entropytou = pow(Density / atime^3, GAMMA_MINUS1) / GAMMA_MINUS1.
 *   the fraction (:367-382)  initionfrac = curionfrac = (rows of type 0 with the flag) / n_gas_tot.
 *   the candidates (:290-311)  the groups with min <= Mass <= max in the order of the group table; only with curionfrac < desired.
 *   the loop (:575-628), iteration = 0, 1, ... while curionfrac < desired:
 *       choice   qso = (int64)(table[(TotNgroups + iteration) % size] * ncand_tot), ncand_tot--; position = qso, or -1 outside the list;
 *                when ncand_tot <= 0 now the loop ends BEFORE the bubble: the last remaining candidate is never lit.
 *       bubble   only for position > 0 (:505): the candidate at list position 0 ionises nothing and is consumed all the same.  Centre =
 *                CM of the group, radius = mean_bubble + sqrt(var_bubble) sqrt(-2 log u1) cos(2 pi u2), u1 = table[MinID % size],
 *                u2 = table[(MinID + 1) % size], computed on the host in double.  Every row of CURRENT type 0 without the flag whose
 *                nearest image lies within r2 <= radius^2 is ionised as above; count = the rows newly ionised.
 *       then     curionfrac += count / n_gas_tot; the loop ends when count < 0.01 non_overlapping_bubble_number and iteration > 10;
 *                otherwise the candidate leaves the list.
 * The device scans the gas once per BATCH of iterations and keeps, per row, the first bubble that covers it; the host replays the loop on
 * the counts (same doubles, same order) and an apply pass ionises the rows of the bubbles before the stop: flags, counts and curionfrac
 * are those of the sequential loop for every batch size.  No tree is read, built or changed.  Garbage rows carry type 7 in
 * the bound type column.
 * ERRORS (returned; the reference would endrun or divide by zero): no parameters, no random table (mpg_set_random_table), n_gas_tot <= 0,
 * no type column; and, found when the candidate list is drawn, before any bubble is scanned (a flash has been applied by then): a radius
 * that is not positive and finite, a table value of exactly 0 at a seed used as u1. */
typedef struct mpg_heiii_params {
    double qso_candidate_min_mass, qso_candidate_max_mass; /* QSOMinMass, QSOMaxMass */
    double mean_bubble, var_bubble;                        /* QSOMeanBubble, QSOVarBubble */
    double heIIIreion_finish_frac;                         /* QSOHeIIIReionFinishFrac */
} mpg_heiii_params;
typedef struct mpg_heiii_step {
    double atime;
    double desired_ion_frac;   /* XHeIII(atime), :530 */
    double qso_inst_heating;   /* Q_inst of the table's header, in erg */
    double uu_in_cgs;          /* UnitInternalEnergy_in_cgs */
    int64_t n_gas_tot;         /* SlotsManager->info[0].size */
    int64_t non_overlapping_bubble_number; /* :550-554 */
    int64_t TotNgroups;        /* fof.TotNgroups: the seed of the choices */
} mpg_heiii_step;
enum { MPG_HEIII_NOTHING_TO_DO = 0, MPG_HEIII_NO_CANDIDATES = 1, MPG_HEIII_REACHED = 2, MPG_HEIII_EXHAUSTED = 3, MPG_HEIII_INSUFFICIENT = 4 };
typedef struct mpg_heiii_result {
    int64_t n_ionized_before;  /* rows of type 0 with the flag on entry */
    int64_t flash_ionized;     /* rows the flash branch ionised (0 without it) */
    int64_t iterations;        /* iterations that reached the bookkeeping of :587-621 (the entries of mpg_heiii_export) */
    int64_t tot_n_ionized;     /* summed counts of the bubbles */
    double initionfrac, curionfrac;
    int stop_reason;           /* MPG_HEIII_*: curionfrac >= desired on entry; no group in the mass window; desired reached; the list
                                * ran out (:581-585); insufficient ionisation (:618-621) */
} mpg_heiii_result;
int mpg_set_heiii_params(mpg_engine *eng, const mpg_heiii_params *par);
/* gas_ionization_fraction on the bound particles: *n_ionized = rows of type 0 with the flag, *fraction = n_ionized / n_gas_tot (either may be
 * NULL).  need_change_helium_ionization_fraction (:661-669) is fraction < desired. */
int mpg_dev_heiii_ionization_fraction(mpg_engine *eng, const uint8_t *d_heiii_ionized, int64_t n_gas_tot, int64_t *n_ionized, double *fraction);
/* on the bound particles (Pos and Type; Type is required).  Device columns of n entries: density (read), entropy and heiii_ionized (in / out);
 * device group columns of ngroups entries as mpg_dev_fof_groups fills them: d_group_mass, d_group_cm [ngroups][3], d_group_minid.  Mass is
 * read back whole, CM and MinID for the candidates only.  The group columns may be NULL with ngroups == 0. */
int mpg_dev_heiii_reionization(mpg_engine *eng, const mpg_heiii_step *step, const double *d_density, double *d_entropy, uint8_t *d_heiii_ionized,
                               const double *d_group_mass, const double *d_group_cm, const uint64_t *d_group_minid, int64_t ngroups,
                               mpg_heiii_result *result);
/* host form: `pv` supplies Pos / Type / flags; all arrays are HOST arrays.  entropy and heiii_ionized come back. */
int mpg_heiii_reionization(mpg_engine *eng, const mpg_particle_view *pv, double BoxSize, const mpg_heiii_step *step, const double *density,
                           double *entropy, uint8_t *heiii_ionized, const double *group_mass, const double *group_cm,
                           const uint64_t *group_minid, int64_t ngroups, mpg_heiii_result *result);
/* on a resident gas run: Density and Entropy are the resident columns; the flag (HOST array) travels in and out, the groups are HOST arrays */
int mpg_resident_sph_heiii_reionization(mpg_engine *eng, const mpg_particle_view *pv, const mpg_heiii_step *step, uint8_t *heiii_ionized,
                                        const double *group_mass, const double *group_cm, const uint64_t *group_minid, int64_t ngroups,
                                        mpg_heiii_result *result);
/* the iterations of the last call, `capacity` entries at most into host arrays (any may be NULL); *count their number.  position: new_qso,
 * the position in the candidate list as it stood; group: the index into the group table, or -1 when position <= 0 (nothing was lit; radius
 * is 0 then); count: rows newly ionised; curionfrac after the iteration.  The shim writes FdHelium from these. */
int mpg_heiii_export(mpg_engine *eng, int64_t capacity, int64_t *position, int64_t *group, double *radius, int64_t *count, double *curionfrac,
                     int64_t *n);
/* bubbles per scan, 1 .. 64; 0: the default (64).  The result does not depend on it. */
int mpg_heiii_set_batch(mpg_engine *eng, int batch);
/* device time of the last call in ms, from events on the engine's stream, summed over its batches: [0] the scan kernels, [1] the copies of
 * the counts, [2] the apply passes.  The host's replay between [1] and [2], the fraction count and the flash are in none. */
int mpg_heiii_get_times(mpg_engine *eng, double ms[3]);

/* ---- star formation on the effective equation of state: cooling_and_starformation, libgadget/sfr_eff.c:186-394 (run.c:663-664) --------
 * Everything in cooling_and_starformation that changes neither the number of rows nor a row's type: the loop of :224-272, the subgrid winds
 * of :280-286 and the sums of :343-350, for ONE rank with StarformationOn.  For every listed row that passes the filter of :229:
 *   winds_evolve (winds.c:374-391) when a `delaytime` column is given (mpg_set_wind_params is then required; NULL: DelayTime == 0);
 *   the class: sfreff_on_eeqos (:534-566), or quicklyastarformation (:706-725) when QuickLymanAlphaProbability > 0;
 *   a row that does not form stars: cooling_direct through the cooling kernel of mpg_dev_cooling on the compacted list of these rows;
 *   a row on the effective equation of state: starformation (:731-800) without the spawning - get_sfr_eeqos (:804-841, one GetCoolingTime),
 *       get_starformation_rate_full (:843-862) with the H2 (:1041-1077) and self-gravity (:1079-1112) factors, Sfr, Ne, both Metallicity
 *       increments, cooling_relaxed (:666-701, with the BHFeedbackUseTcool 1 / 3 branch, its second GetCoolingTime and the clearing of
 *       BHHeated), find_star_mass (:1002-1023), the draw table[(ID + 1) % size] < prob with w = table[ID % size], and the rule
 *       Mass >= 1.1 mass_of_star that tells a spawned star from a converted particle.  With QuickLymanAlphaProbability > 0 a star-forming
 *       row is converted as it is (:247-251): none of its columns changes.
 * RESULTS besides the columns, all in the order of the active list (what gadget_compact_thread_arrays gives under the static schedule):
 *   the new-star list: parent row, mass_of_star, spawn (1) or convert (0).  The kernel writes neither Mass, Generation, Type nor ID:
 *       slots_split_particle, slots_convert, make_particle_star and the rest of :288-393 stay the caller's;
 *   the MaybeWind list (:264-268), when a `stellarmass` column is given: the star-forming rows without a new star, StellarMass by particle;
 *   sum_sm, localsfr, sum_dtime, sum_sf_part: summed in a fixed order, so two calls give the same bits.
 * With WindOn and WIND_SUBGRID in the WindModel the call ends with winds_subgrid on the MaybeWind list (:280-286), as mpg_dev_winds_subgrid.
 * A list entry outside the table is ignored and a time bin beyond 46 is read as 46, as in mpg_dev_cooling.  A row whose network hits its
 * iteration limit keeps all its columns but DelayTime (winds_evolve has run before the row's class is known, as in the reference; for a
 * star-forming row it can only have written 0), forms no star, enters no list and no sum but sum_sf_part, and makes the call return non-zero
 * after every other row is done.  The lists on the device stay valid until the next call (mpg_sfr_dev_lists). */
typedef struct mpg_sfr_params {
    /* the members of struct SFRParams (sfr_eff.c:36-90) the loop reads, AFTER init_cooling_and_star_formation (the threshold is the caller's) */
    int StarformationCriterion; /* enum StarformationCriterion, sfr_eff.h:16-23 */
    int BoostSFDenseGas;
    double BoostSFOverDenseFactor;
    double FactorSN, FactorEVP, MaxSfrTimescale;
    int Generations;
    int BHFeedbackUseTcool;     /* 0, 1 or 3; 2 is refused (it needs get_egyeff in the classification) */
    double QuickLymanAlphaProbability, QuickLymanAlphaTempThresh;
    double EgySpecSN, EgySpecCold, PhysDensThresh, OverDensThresh;
    double UnitSfr_in_solar_per_year, avg_baryon_mass, tau_fmol_unit, GravInternal;
    int WindOn;
    /* UVF.enabled: must agree with the engine's table (mpg_set_uvf_table): refused when set without one, and every
     * cooling_and_starformation call is refused while the two disagree */
    int UVFluctuationOn;
    /* built with EXCUR_REION: refused on an engine without an excursion-set model (mpg_set_excursion_set comes first) */
    int ExcursionSetReion;
    /* what is refused when it is set, so that a caller keeps its CPU path from the start */
    int NTask;           /* ranks of the run; 0 is read as 1 */
} mpg_sfr_params;
/* arrays in particle order, n entries (x 3 where noted); slot members are indexed by PARTICLE */
typedef struct mpg_sfr_columns {
    /* read */
    const uint64_t *id;           /* P.ID */
    const uint8_t *generation;    /* P.Generation; NULL = 0 */
    const double *density;        /* SPHP.Density */
    const double *hsml;           /* P.Hsml (SFR_CRITERION_MOLECULAR_H2) */
    const double *divvel;         /* SPHP.DivVel (SFR_CRITERION_SELFGRAVITY) */
    const double *curlvel;        /* SPHP.CurlVel (SFR_CRITERION_SELFGRAVITY) */
    const double *gradrho_mag;    /* GradRho_mag (SFR_CRITERION_MOLECULAR_H2) */
    const uint8_t *tb_hydro;      /* P.TimeBinHydro; NULL = 0 */
    const uint8_t *heiii_ionized; /* P.HeIIIionized (cooling_direct); NULL = 0 */
    const double *vdisp;          /* SPHP.VDisp (winds_subgrid) */
    /* in / out */
    double *entropy;              /* SPHP.Entropy */
    double *ne;                   /* SPHP.Ne */
    double *sfr;                  /* SPHP.Sfr */
    double *metallicity;          /* SPHP.Metallicity */
    double *delaytime;            /* SPHP.DelayTime; NULL = 0 everywhere, no winds_evolve */
    uint8_t *bhheated;            /* P.BHHeated; NULL = 0 */
    double *vel;                  /* [n][3] P.Vel (winds_subgrid) */
    /* out */
    double *stellarmass;          /* StellarMass of the rows of the MaybeWind list; NULL: no such list */
} mpg_sfr_columns;
typedef struct mpg_sfr_result {
    int64_t treated;      /* listed rows that passed the filter */
    int64_t cooled;       /* ... that went through cooling_direct */
    int64_t sum_sf_part;  /* ... that were star-forming */
    int64_t newstars, converted, spawned;
    int64_t maybewind;
    int64_t errors;       /* rows that hit an iteration limit: cooled and star-forming */
    double sum_sm, localsfr, sum_dtime;
} mpg_sfr_result;
/* an error that names the setting for BHFeedbackUseTcool == 2, UVFluctuationOn without a table on this engine (mpg_set_uvf_table comes
 * first), EXCUR_REION without an excursion-set model on this engine (mpg_set_excursion_set comes first) and several ranks.  A fifth refusal belongs to one form: mpg_resident_sph_cooling_and_starformation with WindOn and
 * WIND_SUBGRID (below).  With a table, starformation takes the row's own background (sfr_eff.c:745) in both GetCoolingTime calls, and the
 * cooled rows theirs as in mpg_dev_cooling; a star-forming row whose position cannot be evaluated is an error row. */
int mpg_set_sfr_params(mpg_engine *eng, const mpg_sfr_params *par);
/* on the bound particles (types from the bound table, garbage as type 7, Mass the bound column); d_active NULL = all particles.  Required:
 * id, density, entropy, ne, sfr, metallicity and what the criterion reads; with WindOn and WIND_SUBGRID also vdisp, vel, delaytime and
 * stellarmass.  The random table is that of mpg_set_random_table, the cooling parameters those of mpg_set_cooling_params. */
int mpg_dev_cooling_and_starformation(mpg_engine *eng, const mpg_sfr_columns *A, const mpg_sph_times *T, const mpg_cooling_step *step,
                                      const int *d_active, int64_t nactive);
/* host form: `pv` supplies Mass / Type / flags, `A` holds HOST arrays in particle order (the shim gathers P and SphP into them) */
int mpg_cooling_and_starformation(mpg_engine *eng, const mpg_particle_view *pv, double BoxSize, const mpg_sfr_columns *A, const mpg_sph_times *T,
                                  const mpg_cooling_step *step, const int *ActiveParticle, int64_t NumActiveParticle);
/* on a resident gas run (mpg_resident_sph_begin): Density, Entropy and TimeBinHydro are the resident columns, and so are Hsml, DivVel and
 * CurlVel, which the density loop of the stretch left there and whose host copies are stale (these six members of `A` are not read); every
 * other member of `A` is a HOST array that travels.  REFUSED here: WindOn with WIND_SUBGRID, whose kicks would have to
 * reach the resident Vel.  A caller with subgrid winds sets WindOn = 0 for this form, gives a `stellarmass` column, and runs winds_subgrid on
 * the exported MaybeWind list after the stretch has ended (shim/cooling-hip.c does). */
int mpg_resident_sph_cooling_and_starformation(mpg_engine *eng, const mpg_particle_view *pv, const mpg_sfr_columns *A, const mpg_sph_times *T,
                                               const mpg_cooling_step *step, const int *ActiveParticle, int64_t NumActiveParticle);
/* counts, sums and errors of the last call */
int mpg_sfr_get_result(mpg_engine *eng, mpg_sfr_result *result);
/* the two lists of the last call into host arrays (any may be NULL): the first `capacity` new stars (parent row, mass_of_star, 1 = spawn /
 * 0 = convert), *nnew their number; the first `wcapacity` rows of the MaybeWind list, *nmaybewind its length */
int mpg_sfr_export(mpg_engine *eng, int64_t capacity, int32_t *parent, double *mass_of_star, uint8_t *spawn, int64_t *nnew, int64_t wcapacity,
                   int32_t *maybewind, int64_t *nmaybewind);
/* ... and where they are on the device until the next call (any may be NULL; lengths in mpg_sfr_get_result) */
int mpg_sfr_dev_lists(mpg_engine *eng, const int **d_parent, const double **d_mass_of_star, const uint8_t **d_spawn, const int **d_maybewind);
/* per particle of the last call (host arrays of n entries, either may be NULL): the class (0 not treated, 1 cooled, 2 star-forming) and
 * the network evaluations of a star-forming row (-1 for every other row; those of the cooled rows: mpg_cooling_export) */
int mpg_sfr_export_rows(mpg_engine *eng, int64_t n, uint8_t *rowclass, int32_t *evaluations);
/* statistics of the last call: [0] list entries, [1] rows treated, [2] cooled, [3] star-forming, [4] network evaluations of the
 * star-forming rows summed, [5] star-forming rows that hit a limit, [6] new stars, [7] rows of the MaybeWind list.  After the call
 * mpg_cooling_get_stats / mpg_cooling_export describe the cooled rows as after mpg_dev_cooling. */
int mpg_sfr_get_stats(mpg_engine *eng, int64_t stats[8]);

/* ---- introspection (tests, bench roofline accounting) ----------------------------------------- */
typedef struct mpg_tree_stats {
    int64_t NumParticles; /* particles in the tree */
    int64_t numnodes;     /* live nodes */
    int64_t numleaves;
    int32_t maxlevel;
    double root_mass, root_cofm[3], root_hmax;
} mpg_tree_stats;
int mpg_tree_get_stats(mpg_engine *eng, mpg_tree_stats *st);
/* Copy the node table to host arrays (each may be NULL): level[i], center[i][3], len[i], cofm[i][3], mass[i],
 * hmax[i], sibling[i] (-1 = none), pstart[i], pcount[i] (0 for internal nodes).  Nodes are in depth-first
 * pre-order, children in octant order x | y<<1 | z<<2 (forcetree.c:278-284). */
int mpg_tree_export(mpg_engine *eng, int32_t *level, double *center, double *len, double *cofm, double *mass, double *hmax,
                    int32_t *sibling, int32_t *pstart, int32_t *pcount);
/* Tree-order permutation: order[k] = caller index of the k-th particle in tree order (n entries). */
int mpg_tree_export_order(mpg_engine *eng, int32_t *order);
/* Diagnostic read-out of what the build derives from the node table for the kernels that walk it (each array may be NULL; M = numnodes).
 * The level-ordered copy is made if it does not exist yet; the search geometry of the SPH loops and the leaf blocks of the two-kernel
 * gravity walk are copied only where a loop or a walk has made them for the current tree, and never created here:
 *   dfs_of_bfs[M]      pre-order number of the i-th node in level order (a stable sort by level)
 *   linkB[M][4]        firstchild (a leaf: the merge counts of its sibling leaves, pair | quad << 4 | all << 8), nchild, pstart, pcount
 *   geoB[M][4], momB[M][4]   (centre, len) and (cofm, mass) in level order;  hmaxB[M]: present[0]
 *   geoS[M][4]         cube around each node's particles: present[1];  hsmaxS[M] largest smoothing length of its SPH sources: present[2]
 *   srcL[(M+1)*8][4]   the leaves' particles in blocks of 8 (x, y, z, mass) by level-order node number: present[3] */
int mpg_tree_export_derived(mpg_engine *eng, int32_t *dfs_of_bfs, int32_t *linkB, double *geoB, double *momB, double *hmaxB, double *geoS,
                            double *hsmaxS, double *srcL, int32_t present[4]);
/* Walk counters of the last grav_short_tree: [0] particle-particle interactions (= the reference's Ninteractions,
 * treewalk.c:904-912), [1] nodes visited, [2] nodes used unopened, [3] targets, [4..7] phase statistics of the
 * cooperative kernel: phase-A group steps, nodes consumed by them (of 8 tested each), phase-B lane-steps issued, of which active; [8],[9] wave clock cycles spent in phase A / phase B (summed over waves). */
int mpg_walk_get_counters(mpg_engine *eng, int64_t counters[10]);
/* ... and of the list kernel's fp32 pre-classification of the node tests (MPG_LISTS_F32=1; counting walks only): [0] target passes that fell
 * back to the fp64 tests, [1] waves (8 targets) whose main loop ran the fp32 form */
int mpg_walk_get_f32_stats(mpg_engine *eng, int64_t out[2]);
/* Per-phase device times (ms, HIP events on the engine stream) of the last call of each phase. */
typedef struct mpg_phase_times {
    float pm_deposit, pm_fft, pm_transfer, pm_readout, pm_total;
    float tree_keys, tree_sort, tree_nodes, tree_moments, tree_total;
    float walk;
    int32_t walk_launches;
} mpg_phase_times;
int mpg_get_phase_times(mpg_engine *eng, mpg_phase_times *t);
/* Enable (1) / disable (0) event timing + walk counters (counters cost a few % in the walk kernel). */
int mpg_set_instrumentation(mpg_engine *eng, int timing, int counters);
/* HIP events are recorded (without synchronising) on the engine stream around every walk-kernel launch.  This call
 * synchronises the stream, returns the summed duration (ms) and number of launches since the last collect. */
int mpg_walk_events_collect(mpg_engine *eng, double *total_ms, int *count);
/* ... and, of the walks that ran as ONE list kernel + ONE evaluation kernel, the two kernels' times (an event between them) */
int mpg_walk_events_collect2(mpg_engine *eng, double *total_ms, int *count, double *lists_ms, double *eval_ms, int *count_split);
/* Device pointer to the tree-order permutation (int32 [NumParticles]: tree slot -> caller index) of the current tree;
 * a contiguous slice of it is a spatially compact active list (used to shard targets over GPUs). */
const int *mpg_dev_tree_order(mpg_engine *eng);
/* grav_short_pair (gravshort-pair.c:21-57): the exact pair-wise short-range force over all particles within Rcut * Asmth * cell
 * size of each target (a sphere, not the tree walk's cube), same softening spline and window; runtests.c:131 checks the tree force
 * against it.  Needs a tree (any walk order); results as for grav_short_tree: FullTreeGravAccel and Potential when the tree holds
 * every particle. */
int mpg_grav_short_pair(mpg_engine *eng, const mpg_particle_view *pv, const int *ActiveParticle, int64_t NumActiveParticle, double Rcut,
                        double rho0);
int mpg_dev_grav_short_pair(mpg_engine *eng, const int *d_active, int64_t nactive, double Rcut, double *d_accel, double *d_potential,
                            double rho0);

/* ---- time integration on device-resident arrays: the streaming loops the reference runs between force
 * steps.  Arrays are in particle order with n entries; flags[i] is the bit-field byte of struct particle_data (bit 0 IsGarbage,
 * bit 1 Swallowed; may be NULL).  Results are bit-identical to the reference's loops (no FMA contraction).
 * Black-hole repositioning (drift.c:31-53) and the dynamic-friction / drag kicks of type 5 (timestep.c:1007-1013) are calls of their own:
 * mpg_dev_reposition_blackholes before the drift, mpg_dev_apply_bh_subgrid_kick after a half kick. */
#define MPG_TIMEBINS 46 /* timebinmgr.h:8 */
typedef struct mpg_kick_factors_s {
    double gravkick[MPG_TIMEBINS + 1];  /* get_exact_gravkick_factor(Ti_kick[bin], Ti_kick[bin] + dti/2); 0 for inactive bins */
    double hydrokick[MPG_TIMEBINS + 1]; /* get_exact_hydrokick_factor, same interval (timestep.c:878-890) */
    double dt_entr[MPG_TIMEBINS + 1];   /* dloga_from_dti(dti_from_timebin(bin) / 2, Ti_Current)  (timestep.c:917) */
    unsigned char bin_active[MPG_TIMEBINS + 1]; /* is_timebin_active(bin, Ti_Current) */
    double atime, MaxGasVel;            /* TimestepParams.MaxGasVel (timestep.c:1026) */
} mpg_kick_factors;
/* drift_all_particles (drift.c:84-102): Pos += Vel * ddrift + random_shift, wrapped into (0, BoxSize]; gas Hsml += DtHsml *
 * ddrift, capped at BoxSize/2.  Returns non-zero (the reference's endrun(5)) for Hsml <= 0 or a non-finite position.
 * d_type, d_flags, d_hsml, d_dthsml may be NULL (then no smoothing lengths are drifted). */
int mpg_dev_drift_all_particles(mpg_engine *eng, int64_t n, double *d_pos, const double *d_vel, const unsigned char *d_type,
                                const unsigned char *d_flags, double *d_hsml, const double *d_dthsml, double ddrift, double BoxSize,
                                const double random_shift[3]);
/* apply_PM_half_kick (timestep.c:964-985): Vel += GravPM * Fgravkick */
int mpg_dev_apply_pm_half_kick(mpg_engine *eng, int64_t n, double *d_vel, const double *d_gravpm, const unsigned char *d_flags, double Fgravkick);
/* apply_half_kick (timestep.c:873-929): short-range gravity kick of the particles in active gravity bins and the hydro kick
 * (velocity, gas velocity limit, entropy) of gas.  d_active == NULL: all n particles.  d_tb_grav / d_tb_hydro NULL: bin 0. */
int mpg_dev_apply_half_kick(mpg_engine *eng, int64_t n, const int *d_active, int64_t nactive, double *d_vel, const double *d_gravaccel,
                            const unsigned char *d_type, const unsigned char *d_flags, const unsigned char *d_tb_grav,
                            const unsigned char *d_tb_hydro, const double *d_hydroaccel, double *d_entropy, const double *d_dtentropy,
                            const mpg_kick_factors *K);
/* apply_hydro_half_kick (timestep.c:930-968): the hydro kick of do_hydro_kick (timestep.c:1004-1036) alone - Vel += HydroAccel *
 * hydrokick[TimeBinHydro], the gas velocity limit MaxGasVel * atime, Entropy += DtEntropy * dt_entr[TimeBinHydro] - for the gas among the
 * listed particles (d_active == NULL: all n), bit-identical to the reference; no gravity kick (K->gravkick is not read), other types
 * unchanged.  d_tb_hydro NULL: bin 0.  A hydro bin above MPG_TIMEBINS is an error. */
int mpg_dev_apply_hydro_half_kick(mpg_engine *eng, int64_t n, const int *d_active, int64_t nactive, double *d_vel, const unsigned char *d_type,
                                  const unsigned char *d_flags, const unsigned char *d_tb_hydro, const double *d_hydroaccel, double *d_entropy,
                                  const double *d_dtentropy, const mpg_kick_factors *K);
/* the kicks of do_hydro_kick for black holes (timestep.c:1007-1013): for the live type-5 rows among the listed particles (d_active == NULL:
 * all n) Vel += DFAccel * K->gravkick[TimeBinHydro], then Vel += DragAccel * K->gravkick[TimeBinHydro] - two additions per component, in that
 * order.  Called after mpg_dev_apply_half_kick or mpg_dev_apply_hydro_half_kick (which leave type 5 alone), a black hole's velocity is
 * bit-identical to the reference's.  d_tb_hydro NULL: bin 0.  A hydro bin above MPG_TIMEBINS is an error. */
int mpg_dev_apply_bh_subgrid_kick(mpg_engine *eng, int64_t n, const int *d_active, int64_t nactive, double *d_vel, const unsigned char *d_type,
                                  const unsigned char *d_flags, const unsigned char *d_tb_hydro, const double *d_dfaccel, const double *d_dragaccel,
                                  const mpg_kick_factors *K);
/* the jump of the black holes to their potential minimum (real_drift_particle, drift.c:31-53), to be called BEFORE
 * mpg_dev_drift_all_particles when BlackHoleRepositionEnabled: a live black hole whose JumpToMinPot is set takes MinPotPos / MinPotVel; the
 * flag of every live black hole is cleared.  Returns non-zero (the reference's endrun(1)) when NEAREST(Pos - MinPotPos) exceeds
 * 0.1 BoxSize along an axis - the reference's signed test - and leaves that black hole where it is. */
int mpg_dev_reposition_blackholes(mpg_engine *eng, int64_t n, double *d_pos, double *d_vel, const unsigned char *d_type, const unsigned char *d_flags,
                                  int32_t *d_jumptominpot, const double *d_minpotpos, const double *d_minpotvel, double BoxSize);

/* get_timestep_gravity_dloga (timestep.c:1039-1074) for every particle: dloga = H * sqrt(2 ErrTolIntAccuracy a (FORCE_SOFTENING/2.8)
 * / |a_phys|), a_phys = (FullTreeGravAccel + GravPM) / a^2.  Uses the softening set by mpg_gravshort_set_softenings. */
int mpg_dev_timestep_gravity_dloga(mpg_engine *eng, int64_t n, const double *d_gravaccel, const double *d_gravpm, double atime, double hubble,
                                   double ErrTolIntAccuracy, double *d_dloga);

/* get_timestep_hydro_dloga (timestep.c:1076-1118) for every particle: gas takes the Courant criterion 2 CourantFac a Hsml / (fac3
 * MaxSignalVel), fac3 = a^(3 (1 - GAMMA) / 2), or, when shorter, the Gadget-4 criterion on the change of the smoothing length CourantFac
 * a^2 |Hsml / (DtHsml + 1e-20)|; a black hole the step of the bin above the shortest of its gas neighbours (d_bh_mintimebin = BHP().minTimeBin
 * per particle and dloga_for_bin[b] = get_dloga_for_bin(b, Ti_Current), a host array of MPG_TIMEBINS + 1 entries; both NULL: no limiter);
 * every other type dt = 1.  d_titype (may be NULL) receives enum TimeStepType (timestep.c:89-96: 0 ACCEL, 1 COURANT, 3 NEIGH, 4 HSML).
 * d_type NULL: no gas; d_dthsml NULL: zero. */
int mpg_dev_timestep_hydro_dloga(mpg_engine *eng, int64_t n, const unsigned char *d_type, const double *d_hsml, const double *d_dthsml,
                                 const double *d_maxsignalvel, const unsigned char *d_bh_mintimebin, const double *dloga_for_bin, double atime,
                                 double hubble, double CourantFac, double *d_dloga, unsigned char *d_titype);

/* ---- hierarchical gravity (SplitGravityTimestepsOn, the default): the level loop of timestep.c:239-599 on
 * device-resident arrays.  Per level it builds the tree of the particles active at that level (force_tree_active_moments),
 * walks it for exactly those particles into a separate acceleration array (grav_short_tree with AccelStore) and applies the
 * hierarchical half kick; the first half of a step also assigns the gravity time bins.  The integer timeline, the kick times
 * and the kick integrals stay with the caller: it passes its sync points, its DriftKickTimes and a callback for
 * get_exact_gravkick_factor.  Not carried here: get_PM_timestep_ti (the caller passes the PM step length it found), the hydro
 * bins (find_hydro_timesteps), star / black-hole particles created during the step. */
typedef struct {            /* the integer timeline: SyncPoints[i].loga (timebinmgr.c:18, 372-417); host array, nsync >= 2 */
    int64_t nsync;
    const double *loga;
} mpg_timeline;
typedef struct {            /* DriftKickTimes, timestep.h:10-27 (same fields, same order) */
    int mintimebin, maxtimebin, mingravtimebin;
    int64_t Ti_kick[MPG_TIMEBINS + 1];
    int64_t Ti_lastactivedrift[MPG_TIMEBINS + 1];
    int64_t Ti_Current;
    int64_t PM_length, PM_start, PM_kick;
} mpg_drift_kick_times;
typedef double (*mpg_gravkick_fn)(void *ctx, int64_t ti0, int64_t ti1); /* get_exact_gravkick_factor(CP, ti0, ti1), timefac.c:65-68 */
typedef struct {            /* device arrays in particle order (the particles bound with mpg_dev_bind_particles) */
    double *d_vel;                  /* P[].Vel              [n][3] */
    const double *d_gravpm;         /* P[].GravPM           [n][3] */
    double *d_fulltree_accel;       /* P[].FullTreeGravAccel[n][3] */
    double *d_potential;            /* P[].Potential        [n] (written by walks over a full tree; may be NULL) */
    unsigned char *d_tb_grav;       /* P[].TimeBinGravity   [n] */
    const unsigned char *d_flags;   /* bit 0 IsGarbage, bit 1 Swallowed; may be NULL */
    double *d_stored_accel;         /* StoredGravAccel.GravAccel [n][3], or NULL: FullTreeGravAccel plays its part */
} mpg_hiergrav_arrays;
typedef struct {            /* TimestepParams (timestep.c:40-60) as far as this path reads them */
    double ErrTolIntAccuracy, MinSizeTimestep;
} mpg_timestep_params;
/* hierarchical_gravity_and_timesteps (timestep.c:293-490).  d_active: the active list (NULL = all n particles), with
 * NumActiveGravity of them gravitationally active.  On a PM step (Ti_Current == PM_start + PM_length) dti_max_pm is the
 * caller's get_PM_timestep_ti and times->PM_length / PM_start are updated as the reference does.  rho0 = the mean density
 * of grav_short_tree.  Returns in *badstepsizecount the number of particles print_bad_timebin would have reported. */
int mpg_dev_hierarchical_gravity_and_timesteps(mpg_engine *eng, const mpg_hiergrav_arrays *A, const int *d_active, int64_t NumActiveParticle,
                                               int64_t NumActiveGravity, mpg_drift_kick_times *times, const mpg_timeline *timeline,
                                               const mpg_timestep_params *par, double atime, double hubble, int64_t dti_max_pm, double rho0,
                                               int HybridNuGrav, mpg_gravkick_fn gravkick, void *gravkick_ctx, int64_t *badstepsizecount);
/* hierarchical_gravity_accelerations (timestep.c:495-599): the second half of the step. */
int mpg_dev_hierarchical_gravity_accelerations(mpg_engine *eng, const mpg_hiergrav_arrays *A, const int *d_active, int64_t NumActiveParticle,
                                               int64_t NumActiveGravity, mpg_drift_kick_times *times, double rho0, int HybridNuGrav,
                                               mpg_gravkick_fn gravkick, void *gravkick_ctx);
/* find_hydro_timesteps (timestep.c:617-733), the assignment of the hydro time bins of the active gas / black-hole particles, in its two
 * halves: the particle loop on the device (new bin from get_timestep_hydro_dloga through convert_timestep_to_ti and get_timebin_from_dti,
 * never above the particle's gravity bin, written to TimeBinHydro when old and new bin are active), and - after the caller's MPI_Allreduce of
 * the smallest bin and the counts, where it has ranks - the update of times->mintimebin (host).  The dynamic-friction bins of the
 * black holes (timestep.c:676-695) are mpg_dev_find_dynfric_timesteps, called after this.  Uses the particles bound with mpg_dev_bind_particles for n. */
typedef struct {
    const unsigned char *d_type;          /* P[].Type; NULL: no gas */
    const unsigned char *d_flags;         /* bit 0 IsGarbage, bit 1 Swallowed; may be NULL */
    const double *d_hsml, *d_dthsml;      /* P[].Hsml, P[].DtHsml (may be NULL: zero) */
    const double *d_maxsignalvel;         /* SPHP().MaxSignalVel (hydro_force) */
    const unsigned char *d_tb_grav;       /* P[].TimeBinGravity; NULL: no cap */
    unsigned char *d_tb_hydro;            /* P[].TimeBinHydro, updated */
    const unsigned char *d_bh_mintimebin; /* BHP().minTimeBin per particle, or NULL */
} mpg_hydrostep_arrays;
typedef struct {
    int mTimeBin;               /* the smallest new bin among this rank's particles (MPG_TIMEBINS if it has none): MPI_MIN over the ranks */
    int64_t ntitype[5];         /* particles by criterion: TI_ACCEL, TI_COURANT, TI_ACCRETE, TI_NEIGH, TI_HSML (MPI_SUM) */
    int64_t badstepsizecount;   /* bin_hydro < 1 (MPI_SUM; the function's return value in the reference) */
    int64_t badtimebins;        /* print_bad_timebin cases: dti <= 1 or > TIMEBASE */
} mpg_hydrostep_result;
int mpg_dev_find_hydro_timesteps(mpg_engine *eng, const mpg_hydrostep_arrays *A, const int *d_active, int64_t NumActiveParticle,
                                 const mpg_drift_kick_times *times, const mpg_timeline *timeline, const mpg_timestep_params *par, double CourantFac,
                                 double atime, double hubble, mpg_hydrostep_result *out);
/* the dynamic-friction bins of the black holes (timestep.c:676-691): get_timestep_dynfric_dloga (timestep.c:1119-1145) through
 * convert_timestep_to_ti and get_timebin_from_dti (with BHP.TimeBinDynFric as the old bin), clamped into [TimeBinHydro, TimeBinGravity] and
 * written to d_tb_dynfric, for the live black holes among the listed particles.  Call it AFTER mpg_dev_find_hydro_timesteps: it reads the
 * new hydro bin.  Returns the sum and the maximum of bin - TimeBinHydro and the number of black holes (the reference's message). */
typedef struct {
    const unsigned char *d_type;
    const unsigned char *d_flags;     /* bit 0 IsGarbage, bit 1 Swallowed; may be NULL */
    const double *d_vel;              /* [n][3] P[].Vel */
    const double *d_df_vel;           /* [n][3] BHP().DF_SurroundingVel */
    const double *d_hsml, *d_dthsml;  /* P[].Hsml, P[].DtHsml (may be NULL: zero) */
    const unsigned char *d_tb_grav;   /* P[].TimeBinGravity; NULL: no cap */
    const unsigned char *d_tb_hydro;  /* P[].TimeBinHydro, as mpg_dev_find_hydro_timesteps left it */
    unsigned char *d_tb_dynfric;      /* BHP().TimeBinDynFric per particle, updated */
} mpg_dynfricstep_arrays;
typedef struct {
    int64_t dynratio; /* sum of bin_dynfric - TimeBinHydro (MPI_SUM) */
    int maxdyndiff;   /* its maximum */
    int64_t nbh;      /* black holes (MPI_SUM) */
} mpg_dynfricstep_result;
int mpg_dev_find_dynfric_timesteps(mpg_engine *eng, const mpg_dynfricstep_arrays *A, const int *d_active, int64_t NumActiveParticle,
                                   const mpg_drift_kick_times *times, const mpg_timeline *timeline, const mpg_timestep_params *par, double CourantFac,
                                   double atime, double hubble, mpg_dynfricstep_result *out);
/* the tail of find_hydro_timesteps (timestep.c:709-733) with the all-reduced smallest bin: the rule for a bin without active particles,
 * set_bh_first_timestep on the first step (d_type / d_tb_hydro of n particles; may be NULL when isFirstTimeStep == 0), times->mintimebin */
int mpg_dev_hydro_timesteps_finish(mpg_engine *eng, int mTimeBin_global, int isFirstTimeStep, int64_t n, const unsigned char *d_type,
                                   unsigned char *d_tb_hydro, mpg_drift_kick_times *times);
/* find_timesteps (timestep.c:739-849): the step assignment of a run WITHOUT SplitGravityTimestepsOn (run.c:756) - gravity step from
 * FullTreeGravAccel + GravPM (get_timestep_gravity_dloga), for gas / black holes the hydro step where it is shorter, TimeBinHydro and
 * TimeBinGravity both set to the new bin when old and new bin are active.  On a PM step (Ti_Current == PM_start + PM_length) dti_max_pm is the
 * caller's get_PM_timestep_ti and times->PM_length / PM_start are updated as the reference does; the finish call (after the caller's
 * MPI_Allreduce of mTimeBin (MIN), maxTimeBin (MAX) and the counts, where it has ranks) shrinks the PM step onto the longest tree step and
 * sets times->mintimebin / maxtimebin.  Not carried: ForceEqualTimesteps, set_bh_first_timestep (the caller keeps both). */
typedef struct {
    int mTimeBin, maxTimeBin;   /* smallest / largest new bin among this rank's active particles (MPG_TIMEBINS / 0 if it has none) */
    int isPM;                   /* this was a PM step */
    int64_t ntitype[5];         /* particles by criterion: TI_ACCEL, TI_COURANT, TI_ACCRETE, TI_NEIGH, TI_HSML */
    int64_t badstepsizecount;   /* bin < 1 (the function's return value in the reference) */
    int64_t badtimebins;        /* print_bad_timebin cases: dti <= 1 or > TIMEBASE */
} mpg_timestep_result;
int mpg_dev_find_timesteps(mpg_engine *eng, const mpg_hydrostep_arrays *A, const double *d_fulltree_accel, const double *d_gravpm,
                           unsigned char *d_tb_grav, const int *d_active, int64_t NumActiveParticle, mpg_drift_kick_times *times,
                           const mpg_timeline *timeline, const mpg_timestep_params *par, double CourantFac, double atime, double hubble,
                           int64_t dti_max_pm, mpg_timestep_result *out);
int mpg_find_timesteps_finish(int mTimeBin_global, int maxTimeBin_global, int isPM, mpg_drift_kick_times *times);
/* A GAS run stays resident too (round 5).  mpg_resident_sph_begin, on a resident table, uploads every array of `A` (host arrays in
 * particle order, as the host forms mpg_density / mpg_hydro_force take them) ONCE; its vel / gacc / gpm then alias the resident
 * P[].Vel / FullTreeGravAccel / GravPM, and the *_in arrays of the velocity / entropy prediction alias the *_out arrays (SphP.HydroAccel,
 * SphP.DtEntropy: one field each in the reference).  From then on mpg_density / mpg_hydro_force called with the same `A` run on the device
 * copies and leave their results there, and the integrator between the force steps runs on the device as well:
 *   mpg_resident_drift_all_particles   drift_all_particles (drift.c:84-102): Pos, and Hsml += DtHsml * ddrift for gas
 *   mpg_resident_apply_pm_half_kick    apply_PM_half_kick (timestep.c:964-985)
 *   mpg_resident_apply_half_kick       apply_half_kick (timestep.c:873-929): gravity kick, hydro kick, gas velocity limit, entropy
 *   mpg_resident_find_timesteps        find_timesteps (timestep.c:739-849): the step assignment of run.c:756 (no SplitGravityTimestepsOn)
 *   mpg_resident_apply_hydro_half_kick apply_hydro_half_kick (timestep.c:930-968): the hydro kick alone (SplitGravityTimestepsOn)
 *   mpg_resident_hierarchical_gravity_accelerations / _and_timesteps
 *                                      the level loop of SplitGravityTimestepsOn (timestep.c:293-599, run.c:536-540, 766-767)
 *   mpg_resident_find_hydro_timesteps  find_hydro_timesteps (timestep.c:617-733) on TimeBinHydro (both halves, one rank; several ranks:
 *                                      mpg_dev_find_hydro_timesteps + the caller's MPI_Allreduce + mpg_dev_hydro_timesteps_finish on
 *                                      mpg_resident_sph_arrays)
 * mpg_resident_sph_end writes every array back to `A` (Entropy and the time bins included: the kicks and the bin assignment changed them)
 * and leaves the mode; mpg_resident_end does the same for the table.  shim/timestep-hip.c forwards the reference's own entry points. */
int mpg_resident_sph_begin(mpg_engine *eng, const mpg_particle_view *pv, const mpg_sph_arrays *A);
int mpg_resident_sph_arrays(mpg_engine *eng, mpg_sph_arrays *device_arrays_out);
int mpg_resident_sph_end(mpg_engine *eng, const mpg_sph_arrays *A);
/* the resident time bins into host arrays of n bytes (either may be NULL): build_active_particles (timestep.c:1333-1420) reads
 * P[].TimeBinHydro / TimeBinGravity on the host at the top of every step, so the shim copies them into P[] after every bin assignment */
int mpg_resident_fetch_timebins(mpg_engine *eng, unsigned char *tb_hydro, unsigned char *tb_grav);
int mpg_resident_drift_all_particles(mpg_engine *eng, const mpg_particle_view *pv, double ddrift, const double random_shift[3]);
int mpg_resident_apply_pm_half_kick(mpg_engine *eng, const mpg_particle_view *pv, double Fgravkick);
int mpg_resident_apply_half_kick(mpg_engine *eng, const mpg_particle_view *pv, const int *ActiveParticle, int64_t NumActiveParticle,
                                 const mpg_kick_factors *K);

/* find_timesteps on a resident gas run, one rank (both halves): accelerations, Hsml, DtHsml, MaxSignalVel and the time bins are the resident ones */
int mpg_resident_find_timesteps(mpg_engine *eng, const mpg_particle_view *pv, const int *ActiveParticle, int64_t NumActiveParticle,
                                mpg_drift_kick_times *times, const mpg_timeline *timeline, const mpg_timestep_params *par, double CourantFac,
                                double atime, double hubble, int64_t dti_max_pm, mpg_timestep_result *out);
/* both halves on a resident gas run (mpg_resident_sph_begin), one rank: Hsml, DtHsml, MaxSignalVel and the time bins are the resident ones */
int mpg_resident_find_hydro_timesteps(mpg_engine *eng, const mpg_particle_view *pv, const int *ActiveParticle, int64_t NumActiveParticle,
                                      mpg_drift_kick_times *times, const mpg_timeline *timeline, const mpg_timestep_params *par, double CourantFac,
                                      double atime, double hubble, int isFirstTimeStep, mpg_hydrostep_result *out);

int mpg_resident_apply_hydro_half_kick(mpg_engine *eng, const mpg_particle_view *pv, const int *ActiveParticle, int64_t NumActiveParticle,
                                       const mpg_kick_factors *K);
/* The branch of run.c WITH SplitGravityTimestepsOn (the default) on a resident run, one rank: mpg_dev_hierarchical_gravity_accelerations /
 * _and_timesteps on the resident table.  Vel, GravPM, FullTreeGravAccel and Potential are the table's columns, TimeBinGravity is the resident
 * gas run's tb_grav (so, as for mpg_resident_find_timesteps, mpg_resident_sph_begin comes first), the flags are the table's; the host active
 * list is uploaded (NULL: all n particles active, whatever NumActiveParticle says), the level trees are built from the resident positions.  rho0, the timeline, the PM step length on a PM step and the
 * gravkick callback are as for the dev forms.
 * StoredGravAccel (run.c:533-540: filled by the first call, read by the second) lives on the device for the caller's host array of
 * [n][3] (the first n rows of struct grav_accel_store's GravAccel):
 *   - a call naming a host array the engine does not hold yet uploads its first n rows and holds it from then on;
 *   - mpg_resident_end writes the device copy back into the held array (n rows) and releases it, so the stretch may end and a new one begin
 *     between the two calls (cooling, star formation, FOF, a snapshot) and the second call then takes the array up again;
 *   - _and_timesteps releases the array once it has used it (the reference frees it there, timestep.c:417-418);
 *   - NULL: no stored array, FullTreeGravAccel plays its part (timestep.c:352, 417).
 * Not carried: several ranks (the dev forms on mpg_dist state are the multi-rank path), black holes (mpg_shim_resident_begin refuses
 * them), and star particles created during the step (only n rows are kept).  The trees of the levels replace the engine's tree. */
int mpg_resident_hierarchical_gravity_accelerations(mpg_engine *eng, const mpg_particle_view *pv, const int *ActiveParticle, int64_t NumActiveParticle,
                                                    int64_t NumActiveGravity, mpg_drift_kick_times *times, double rho0, int HybridNuGrav,
                                                    mpg_gravkick_fn gravkick, void *gravkick_ctx, double (*StoredGravAccel)[3]);
int mpg_resident_hierarchical_gravity_and_timesteps(mpg_engine *eng, const mpg_particle_view *pv, const int *ActiveParticle, int64_t NumActiveParticle,
                                                    int64_t NumActiveGravity, mpg_drift_kick_times *times, const mpg_timeline *timeline,
                                                    const mpg_timestep_params *par, double atime, double hubble, int64_t dti_max_pm, double rho0,
                                                    int HybridNuGrav, mpg_gravkick_fn gravkick, void *gravkick_ctx, double (*StoredGravAccel)[3],
                                                    int64_t *badstepsizecount);

/* build_active_sublist (timestep.c:1435-1478): the entries of d_active (NULL = all n) that are not garbage, whose gravity bin
 * is <= maxtimebin and active at Ti_Current, order preserved.  d_out must hold NumActiveParticle entries. */
int mpg_dev_build_active_sublist(mpg_engine *eng, const int *d_active, int64_t NumActiveParticle, const unsigned char *d_tb_grav,
                                 const unsigned char *d_flags, int maxtimebin, int64_t Ti_Current, int *d_out, int64_t *n_out);

/* ---- particle order: Peano-Hilbert keys and the (type, key) sort the reference keeps its particles in
 * (slots_gc_sorted after every full domain decomposition, domain.c:247).  Keys are bit-identical to the reference's. */
/* ---- Peano-Hilbert domain decomposition (libgadget/domain.c) -------------------------------------------------------------
 * The reference's domain_decompose_full (domain.c:153-258) in the pieces its MPI code is made of: the device passes over a
 * rank's particles, the arithmetic on the top-level tree (host; no GPU needed), and - left to the caller, where the reference
 * calls MPI - the sums, the pairwise hand-over of trees and the all-to-all of particle records (INTEGRATION.md shows the
 * sequence; mp-gadget_amd/domain_peano.py is that caller over torch.distributed). */
typedef struct mpg_topnode {            /* struct local_topnode_data, domain.c:60-70, + Leaf of struct topnode_data, domain.h:12-18 */
    uint64_t StartKey;
    int32_t Shift, Daughter, Parent, Leaf;
    int64_t Count, Cost;
} mpg_topnode;
/* the rank's sample of keys for the local refinement, sorted (domain.c:1031-1083 with DomainUseGlobalSorting = 0; for the
 * global sort the caller gathers the ranks' samples and sorts them): every SubSampleDistance-th particle, after a key sort
 * that drops garbage if PreSort.  keys_out: HOST array of `cap` entries; d_garbage: device bytes (IsGarbage) or NULL */
int mpg_dev_domain_sample(mpg_engine *eng, int64_t n, const double *d_pos, const unsigned char *d_garbage, double BoxSize, int PreSort,
                          int SubSampleDistance, uint64_t *keys_out, int64_t cap, int64_t *nsample);
/* domain_check_for_local_refine_subsample from the sorted sample on (domain.c:1085-1180); costs NULL: 1 per sample.
 * *failed = 1: MaxTopNodes too small (the caller enlarges TopNodeAllocFactor and retries, domain.c:182-194) */
int mpg_domain_local_refine(const uint64_t *keys, const int64_t *costs, int64_t nsample, mpg_topnode *tree, int *size, int MaxTopNodes, int *failed);
/* domain_toptree_truncate, domain.c:954-967 */
int mpg_domain_toptree_truncate(mpg_topnode *tree, int *size, int64_t countlimit, int64_t costlimit);
/* one receive step of domain_nonrecursively_combine_topTree (domain.c:1232-1247): tree B of rank ThisTask + sep merged into A */
int mpg_domain_toptree_merge(mpg_topnode *A, int *sizeA, const mpg_topnode *B, int sizeB, int MaxTopNodes, int *failed);
/* domain_global_refine, domain.c:1344-1395 */
int mpg_domain_global_refine(mpg_topnode *tree, int *size, int MaxTopNodes, int64_t countlimit, int64_t costlimit, int *failed);
/* domain_create_topleaves, domain.c:810-824: sets tree[].Leaf, fills leaf_topnode[*nleaves] */
int mpg_domain_create_topleaves(mpg_topnode *tree, int size, int *leaf_topnode, int *nleaves);
/* domain_assign_topleaves_balanced + domain_set_task_leafs (domain.c:610-786): reorders the leaves by (Task, Key) - leaf_topnode
 * and tree[].Leaf are rewritten - and fills leaf_task[nleaves], StartLeaf[NTask], EndLeaf[NTask] */
int mpg_domain_assign_topleaves_balanced(mpg_topnode *tree, int size, int *leaf_topnode, int nleaves, const int64_t *cost, int NTask,
                                         int NsegmentPerTask, int *leaf_task, int *StartLeaf, int *EndLeaf);
/* one pass over the rank's particles: P[].TopLeaf (domain.c:216-225, -1 for garbage) into d_topleaf, the destination task
 * (domain_layoutfunc, domain.c:794-802) into d_task, particles per leaf (domain_compute_costs, domain.c:1398-1457, before the
 * Allreduce) into leaf_counts[nleaves] and per destination task into task_counts[NTask] (host arrays).  leaf_task, d_topleaf,
 * d_task, leaf_counts, task_counts may be NULL. */
int mpg_dev_domain_topleaves(mpg_engine *eng, int64_t n, const double *d_pos, const unsigned char *d_garbage, double BoxSize,
                             const mpg_topnode *tree, int size, int nleaves, const int *leaf_task, int NTask, int32_t *d_topleaf,
                             int32_t *d_task, int64_t *leaf_counts, int64_t *task_counts);

/* PEANO(Pos, BoxSize), libgadget/utils/peano.h:15-21 + peano_hilbert_key, peano.c:117-140: d_keys[n] */
int mpg_dev_peano_keys(mpg_engine *eng, int64_t n, const double *d_pos, double BoxSize, uint64_t *d_keys);
/* the order of slots_gc_sorted (slotsmanager.c:404-452): d_perm[k] = index of the k-th particle by (Type, Key), garbage
 * (flags bit 0) last; *n_live = the particles that are not garbage.  d_type NULL: one type.  Equal (type, key) keep their
 * input order (the reference's qsort leaves it unspecified). */
int mpg_dev_order_by_type_and_key(mpg_engine *eng, int64_t n, const unsigned char *d_type, const unsigned char *d_flags,
                                  const uint64_t *d_keys, int *d_perm, int64_t *n_live);

/* ---- friends-of-friends groups (libgadget/fof.c) on the bound particles: primary linking of the
 * FOFPrimaryLinkTypes at the comoving linking length, secondary particles attached to the nearest primary one, groups of at
 * least FOFHaloMinLength members numbered by (Length descending, MinID).  A group is labelled by its smallest particle ID.
 * The sub-grid half of struct Group (Sfr, metal masses, MassHeIonized, black-hole masses, MaxDens / seed_index) and fof_seed are
 * the calls mpg_dev_fof_subgrid / mpg_dev_fof_seed below, on ONE rank: groups that span ranks (mpg_dist_dev_fof_fof) keep the
 * table they have, without the sub-grid members and without seeding.  fof_set_escapefraction (EXCUR_REION) is
 * mpg_dev_fof_set_escapefraction below, on one rank as well. */
typedef struct mpg_fof_params {     /* struct FOFParams, fof.c:37-48, as far as this path reads it */
    int FOFPrimaryLinkTypes;        /* bit mask of particle types, default 2 (dark matter) */
    int FOFSecondaryLinkTypes;      /* default 1 + 16 + 32 (gas, stars, black holes); disjoint from the primary types */
    double FOFHaloComovingLinkingLength; /* FOFHaloLinkingLength * mean DM separation (fof_init, fof.c:83-86) */
    int FOFHaloMinLength;
} mpg_fof_params;
typedef struct mpg_fof_groups {     /* struct Group / BaseGroup, fof.h:14-49: device arrays of *ngroups entries; NULL = not wanted */
    uint64_t *MinID;
    int *Length, *GrNr, *LenType;   /* LenType[g][6] */
    double *Mass, *MassType;        /* MassType[g][6] */
    double *CM, *Vel, *Jmom;        /* [g][3] */
    double *Imom;                   /* [g][3][3] */
    float *FirstPos;                /* [g][3] */
} mpg_fof_groups;
/* fof_fof (fof.c:157-253) with StoreGrNr: d_id[n] = P[].ID, d_vel[n][3] (may be NULL: zero), d_hsml[n] (may be NULL: no radius hint
 * for gas), d_flags (may be NULL).  d_grnr[n] (may be NULL) receives P[].GrNr (-1: in no group); *ngroups = fof.TotNgroups.
 * Builds the tree of the primary types itself (force_tree_rebuild_mask) and leaves it in place. */
int mpg_dev_fof_fof(mpg_engine *eng, const mpg_fof_params *par, const uint64_t *d_id, const double *d_vel, const double *d_hsml,
                    const unsigned char *d_flags, int64_t *d_grnr, int64_t *ngroups);
/* the group table of the last mpg_dev_fof_fof, in MinID order (the order of fof.Group) */
int mpg_dev_fof_groups(mpg_engine *eng, const mpg_fof_groups *out);

/* ---- the sub-grid half of add_particle_to_group (fof.c:647-676) and fof_seed (fof.c:1345-1449, blackhole.c:1039-1111) on the groups
 * of the last mpg_dev_fof_fof.  Membership, Mass and Type are those of that call and of the bound particles; garbage and swallowed
 * rows enter the sums exactly where the FOF call made them members of a group (as in the reference, which does not test them again).
 * Columns are device arrays in particle order, slot members (SphP / StarP / BHP) indexed by PARTICLE; entries of rows of other types
 * are not read.  Any column may be NULL: its terms are 0, and without `density` no group gets a seed.
 *   gas          Sfr += Sfr, GasMetalMass += Metallicity Mass, GasMetalElemMass[j] += Metals[j] Mass, MassHeIonized += Mass HeIIIionized
 *   stars        StellarMetalMass += Metallicity Mass, StellarMetalElemMass[j] += Metals[j] Mass
 *   black holes  BH_Mass += BHP.Mass, BH_Mdot += BHP.Mdot
 * Every sum is fp64 with exact terms widened from the columns' types.  The reference keeps GasMetalElemMass, StellarMetalElemMass and
 * MassHeIonized in float accumulators (fof.h:47-54); the engine returns the fp64 sums.
 * MaxDens / seed_index: the largest Density > 0 among the gas rows of the group that are not decoupled (WindDecouple && DelayTime > 0,
 * winds.c:114-120), and the row that has it.  THE ONE DEFINED DIFFERENCE: among rows of EQUAL largest density the reference keeps the
 * one its qsort puts first (unspecified); the engine keeps the one of smaller particle index, whatever the order of arrival (a 64-bit
 * atomic maximum of the density's bits, then a 64-bit atomic minimum of the index among the rows that equal it).  A group
 * without such a row has MaxDens = 0 and seed_index = -1. */
typedef struct mpg_fof_subgrid_columns {
    const double *sfr;            /* SphP.Sfr */
    const double *metallicity;    /* SphP.Metallicity of gas rows, StarP.Metallicity of star rows: one column */
    const float *metals;          /* [n][9] SphP.Metals / StarP.Metals */
    const uint8_t *heiii_ionized; /* P.HeIIIionized */
    const double *bh_mass;        /* BHP.Mass */
    const double *bh_mdot;        /* BHP.Mdot */
    const double *density;        /* SphP.Density */
    const double *delaytime;      /* SphP.DelayTime */
    int WindDecouple;             /* HAS(wind_params.WindModel, WIND_DECOUPLE_SPH) */
} mpg_fof_subgrid_columns;
typedef struct mpg_fof_subgrid_groups { /* device arrays of ngroups entries in MinID order (as mpg_fof_groups); NULL = not wanted */
    double *Sfr, *GasMetalMass, *StellarMetalMass;
    double *GasMetalElemMass, *StellarMetalElemMass; /* [g][9] */
    double *MassHeIonized, *BH_Mass, *BH_Mdot, *MaxDens;
    int64_t *seed_index;                             /* particle index, -1: none */
} mpg_fof_subgrid_groups;
/* ERRORS (returned): no mpg_dev_fof_fof since the particles were last bound; the bound count differs from the FOF's.  `out` may be NULL:
 * the sums are then only kept for mpg_dev_fof_seed. */
int mpg_dev_fof_subgrid(mpg_engine *eng, const mpg_fof_subgrid_columns *A, const mpg_fof_subgrid_groups *out);

typedef struct mpg_fof_seed_params {
    double MinFoFMassForNewSeed, MinMStarForNewSeed;                        /* fof_params, fof.c:37-48 */
    double SeedBlackHoleMass, MaxSeedBlackHoleMass, SeedBlackHoleMassIndex; /* blackhole_params, blackhole.c:28-54 */
    double SeedBHDynMass;
} mpg_fof_seed_params;
/* the columns blackhole_make_one (blackhole.c:1056-1111) reads and writes, in particle order; slots_convert is type = 5 here.  A NULL
 * output column is skipped.  Pos is the bound one. */
typedef struct mpg_bh_seed_columns {
    /* read */
    const uint64_t *id;             /* P.ID: the power-law seed mass draws table[(ID + 23) % size], the sum wrapping as unsigned 64-bit */
    const uint8_t *tb_hydro;        /* P.TimeBinHydro */
    /* in / out */
    uint8_t *type;                  /* P.Type: must be 0 for every seed (endrun 7772), becomes 5; NULL: the bound column is checked */
    float *mass;                    /* P.Mass: becomes SeedBHDynMass when that is > 0; NULL: the bound column is read */
    /* out */
    double *bh_mass, *mseed;        /* BHP.Mass, BHP.Mseed */
    double *mdot;                   /* BHP.Mdot = 0 */
    double *formationtime;          /* BHP.FormationTime = atime */
    uint64_t *swallowid;            /* BHP.SwallowID = (uint64) -1 */
    double *bh_density;             /* BHP.Density = 0 */
    uint8_t *tb_dynfric;            /* BHP.TimeBinDynFric = P.TimeBinHydro */
    double *minpotpos;              /* [n][3] BHP.MinPotPos = P.Pos */
    double *dfaccel, *df_surroundingvel, *dragaccel; /* [n][3] = 0 */
    double *df_surroundingrmsvel, *df_surroundingdensity; /* = 0 */
    int32_t *jumptominpot;          /* = 0 */
    int32_t *countprogs;            /* = 1 */
    double *mtrack;                 /* BHP.Mtrack = the old P.Mass when SeedBHDynMass > 0, else -1 */
    double *kineticfdbkenergy, *vdisp; /* = 0 */
} mpg_bh_seed_columns;
/* fof_seed on the groups of the last mpg_dev_fof_subgrid: a group is marked when Mass >= MinFoFMassForNewSeed && MassType[4] >=
 * MinMStarForNewSeed && LenType[5] == 0 && seed_index >= 0 (fof.c:1356-1365); the marked groups, in group (MinID) order, give the list
 * d_seed_group[k] / d_seed_particle[k] (device arrays of `cap` entries, either may be NULL), *nseeds its length.  With `cols` every
 * listed particle becomes a black hole (blackhole_make_one); cols == NULL: the list only.  *nwarn (may be NULL) counts the rows for
 * which the reference prints its mass warning (blackhole.c:1105).
 * ERRORS (returned): no mpg_dev_fof_subgrid since the last mpg_dev_fof_fof; MaxSeedBlackHoleMass > 0 with `cols` and without a random
 * table (mpg_set_random_table) or without cols->id; a listed row that is no gas (endrun 7772): found before anything is written; cap smaller
 * than the list: *nseeds is set, no list is written and nothing is converted, the caller repeats with room. */
int mpg_dev_fof_seed(mpg_engine *eng, const mpg_fof_seed_params *par, double atime, const mpg_bh_seed_columns *cols, int64_t cap,
                     int64_t *d_seed_particle, int64_t *d_seed_group, int64_t *nseeds, int64_t *nwarn);

/* fof_set_escapefraction (fof.c:832-870, EXCUR_REION) on the groups of the last mpg_dev_fof_fof: d_escfrac[n] (device, particle order)
 * receives Group.Mass for every gas or star row that is a member of a group and 0 for every other gas or star row; rows of other types
 * are left untouched.  The value is the Mass column of mpg_dev_fof_groups bit for bit.  mpg_dev_calculate_uvbg converts it.
 * ERRORS (returned): those of mpg_dev_fof_subgrid. */
int mpg_dev_fof_set_escapefraction(mpg_engine *eng, double *d_escfrac);

/* ---- the group catalogue on disk: fof_save_groups / fof_save_particles (fof.c:1157-1163, fofpetaio.c:38-159) on ONE rank, from device
 * columns in particle order.  The file holds `Header` (twelve attributes, fofpetaio.c:448-459), the FOFGroups blocks in GrNr order
 * (fofpetaio.c:538-568; the getters of :464-536) and, with SaveParticles, one block "<ptype>/<name>" per descriptor holding the selected
 * rows of that type sorted by GrNr (register_io_blocks with WriteGroupID, petaio.c:986-1080).
 *   selected:   GrNr >= 0, type < 6, flag bit 0 (IsGarbage) and bit 1 (Swallowed) clear (fofpetaio.c:33-36, petaio.c:117-154)
 *   in_group:   GrNr >= 0 and type < 6, whatever the flags: NumPartInGroupTotal of the header (fofpetaio.c:432-436)
 * THE ONE DEFINED DIFFERENCE: rows of equal (type, GrNr) keep ascending particle index; the reference's qsort_openmp with
 * order_by_type_and_grnr (fofpetaio.c:202-218, :389) leaves their order unspecified.
 * GrNr counts from 1 here as in fof.c:1127-1134: the FOFGroups blocks are scattered to row GrNr - 1, GroupID holds GrNr itself.
 * The wraps of the position getters are the reference's two loops of repeated addition (the bits match), each bounded at 64 trips: a value
 * that is not finite or lies further out fails the call with the block and the row named, and nothing of that block is written. */
enum { MPG_DT_F8 = 0, MPG_DT_F4 = 1, MPG_DT_U1 = 2, MPG_DT_U4 = 3, MPG_DT_U8 = 4, MPG_DT_I4 = 5, MPG_DT_I8 = 6 };
enum {
    MPG_CONV_NONE = 0,     /* SIMPLE_GETTER: out = (block type) column */
    MPG_CONV_POSITION = 1, /* GTPosition, petaio.c:744-753: f64 [3] - CurrentParticleOffset, wrapped into (0, BoxSize]; f8 */
    MPG_CONV_VELOCITY = 2, /* GTVelocity, petaio.c:803-817: (float)(fac * Vel), fac = 1 / atime with UsePeculiarVelocity, else 1 */
    MPG_CONV_GROUPID = 3   /* GTGroupID, petaio.c:887: the int64 GrNr column as u4; d_data NULL: the GrNr of the last mpg_dev_fof_fof */
};
typedef struct mpg_fof_catalogue_params {
    double atime;
    double CurrentParticleOffset[3];
    int UsePeculiarVelocity, MetalReturnOn, SaveParticles;
    int nfile;                 /* files per non-empty block; an empty block gets NFILE: 0 (petaio.c:673-676) */
    double hubble;             /* hubble_function(CP, atime): RSDFactor = 1 / (atime hubble), / atime again without peculiar velocities */
    double MassTable[6];
    double OmegaLambda, Omega0, HubbleParam, CMBTemperature, OmegaBaryon;
} mpg_fof_catalogue_params;    /* (BoxSize is that of the bound particles) */
typedef struct mpg_catalogue_block {
    const char *name;          /* the block is "<ptype>/<name>" */
    int ptype;                 /* 0..5 */
    const void *d_data;        /* device column [n][nmemb] in PARTICLE order, n the bound particles */
    int src_dtype;             /* MPG_DT_F8, F4, U1, U8, I4 or I8: the column's element type */
    int nmemb;
    int dtype;                 /* MPG_DT_F8, F4, U1, U4, U8 or I4: the block's type in the file */
    int conv;                  /* MPG_CONV_* */
} mpg_catalogue_block;
/* fof_select_func + petaio_build_selection + order_by_type_and_grnr: d_perm[n] (device; the first count[0] + ... + count[5] entries are
 * the order, type by type, the rest are the rows not selected), count[6] the selected rows per type, in_group[6].  d_grnr NULL: the GrNr of
 * the last mpg_dev_fof_fof (ERRORS: those of mpg_dev_fof_subgrid); else an int64 column of the bound particles, values below 2^32, and no
 * FOF call is needed.  d_flags may be NULL. */
int mpg_dev_fof_pig_order(mpg_engine *eng, const int64_t *d_grnr, const unsigned char *d_flags, int *d_perm, int64_t count[6], int64_t in_group[6]);
/* the gather of one block, device to device: d_out[j][k] = getter(column[d_perm[j]][k]) for j < count; block->ptype and name only label
 * errors.  ERRORS (returned, d_out untouched by a POSITION block): a d_perm[j] outside the bound particles; a POSITION value that is not
 * finite or more than 64 boxes outside - the first such row j is named. */
int mpg_dev_gather_block(mpg_engine *eng, const int *d_perm, int64_t count, const mpg_catalogue_block *block, const mpg_fof_catalogue_params *params,
                         void *d_out);
/* the whole of fof_save_particles on the groups of the last mpg_dev_fof_fof (and, for the sub-grid members of the FOFGroups blocks, of the
 * last mpg_dev_fof_subgrid; zeros without one): Header, the FOFGroups blocks (the four metal blocks only with MetalReturnOn), and with
 * SaveParticles the `nblocks` particle blocks, each of count[ptype] rows (a type without members gets blocks of size 0).  Every block is
 * gathered into one device buffer, copied into one pinned host buffer and written from there.
 * ERRORS (returned, the block named): those of mpg_dev_fof_subgrid and every fault of a descriptor are found before anything is written and
 * create no file; a refused POSITION row ends the call at its block. */
int mpg_dev_fof_save_groups(mpg_engine *eng, const char *path, const mpg_fof_catalogue_params *params, const mpg_catalogue_block *blocks, int nblocks,
                            const unsigned char *d_flags);
/* device times in ms of the last calls: the order (keys + sort); the sum of the gathers; the FOFGroups scatters */
int mpg_fof_catalogue_get_times(mpg_engine *eng, double ms[3]);

/* ---- excursion-set reionisation (EXCUR_REION; libgadget/uvbg.c:471-594 through petapm_reion, petapm.c:381-577) on the bound particles
 * of ONE rank: the producer of SphP.local_J21 / SphP.zreion.  The consumer (get_local_UVBG_from_J21 in cooling and star formation) is
 * mpg_set_excursion_set above: the two output columns of this call are what mpg_dev_set_excursion_columns binds.
 *   1. init_particle_uvbg: local_J21 = 0 for gas; escfrac (the halo mass of mpg_dev_fof_set_escapefraction) becomes
 *      min(1, EscapeFractionNorm (M UnitMass_in_g / SOLAR_MASS / 1e10 / HubbleParam)^EscapeFractionScaling) for stars with escfrac != 0
 *      and, only with ReionUseParticleSFR, for such gas (the reference's `continue`, uvbg.c:483)
 *   2. three CIC deposits on a UVBGdim^3 mesh: Mass of every row; Mass fesc of stars; Sfr fesc of gas (with ReionUseParticleSFR)
 *   3. forward transforms, divided by UVBGdim^3
 *   4. the radii R = min(ReionRBubbleMax, Box), R / ReionDeltaRFactor, ... down to the last, unfiltered step at R = Box / UVBGdim
 *      (petapm_reion_c2r): per radius one filter pass over the modes, one batched inverse transform, one pass over the cells
 *      (reion_loop_pm) on the float grids J21 / xHI, which stay on the device
 *   5. the volume- and mass-weighted neutral fractions of the last step, summed in a fixed order (equal input, equal numbers)
 *   6. readout_J21: a gas row takes the largest J21 of its 8 CIC corners when that exceeds its local_J21; zreion becomes 1 / Time - 1
 *      where it was -1 and the row took a value
 * DEFINED DIFFERENCES: rows of type 7 (the engine's garbage / swallowed convention) are not deposited, the reference deposits
 * such stale rows; the real-space top hat W(kR) is evaluated in fp64 where the reference calls sinf / cosf / powf on the double kR; the
 * transforms are divided by UVBGdim^3 as a double, the reference's int overflows above 1290, which is refused here. */
typedef struct mpg_uvbg_params {
    int ReionFilterType;              /* 0 real-space top hat, 1 k-space top hat, 2 Gaussian (uvbg.c:215-248) */
    int RtoMFilterType;               /* 0 top hat, 1 Gaussian (uvbg.c:155-173) */
    double ReionRBubbleMax, ReionRBubbleMin, ReionDeltaRFactor;
    double ReionNionPhotPerBary, AlphaUV, EscapeFractionNorm, EscapeFractionScaling;
    int ReionUseParticleSFR;
    double ReionSFRTimescale;
    int UVBGdim;
    double Time, Omega0, OmegaBaryon, RhoCrit, HubbleParam; /* the step: atime and CP's members */
    double hubble;                    /* hubble_function(CP, Time) */
    double UnitLength_in_cm, UnitMass_in_g, UnitTime_in_s;
    int NTask;                        /* several ranks are refused */
} mpg_uvbg_params;
typedef struct mpg_uvbg_columns {     /* device (mpg_dev_*) or host (mpg_calculate_uvbg) arrays in particle order; rows of other types are not touched */
    double *sfr;                      /* in: SphP.Sfr; required with ReionUseParticleSFR, else may be NULL */
    double *escfrac;                  /* in / out: SphP / StarP.EscapeFraction, one column: the halo mass comes back converted */
    double *local_J21;                /* out: SphP.local_J21 */
    double *zreion;                   /* in / out: SphP.zreion */
} mpg_uvbg_columns;
typedef struct mpg_uvbg_result {
    double volume_weighted_global_xHI, mass_weighted_global_xHI;
    int64_t nradii;                   /* filter steps taken, the last (unfiltered) one included */
    int64_t radii_cap;                /* in: room in radii (0: none wanted) */
    double *radii;                    /* out, host: the first min(nradii, radii_cap) radii */
} mpg_uvbg_result;
/* ERRORS (returned, each names the setting): unknown ReionFilterType / RtoMFilterType; ReionDeltaRFactor <= 1; ReionRBubbleMax or
 * ReionRBubbleMin not positive; UVBGdim < 4 or > 1290; ReionUseParticleSFR without an sfr column; NTask > 1; a negative escape fraction
 * (found at the end of the call: the columns are then as the reference's endrun would leave them, converted up to that row). */
int mpg_dev_calculate_uvbg(mpg_engine *eng, const mpg_uvbg_params *par, const mpg_uvbg_columns *cols, mpg_uvbg_result *result);
/* the grids of the last mpg_dev_calculate_uvbg, x slowest: d_J21 / d_xHI float[dim^3] (UVBGgrids, what save_uvbg_grids writes),
 * d_deposit double[3][dim^3] = the mass, star and SFR grids as deposited (the third is zero without ReionUseParticleSFR).  Device
 * arrays; any may be NULL.  `dim` must be the UVBGdim of that call. */
int mpg_dev_uvbg_grids(mpg_engine *eng, int dim, float *d_J21, float *d_xHI, double *d_deposit);
/* calculate_uvbg for a host table: Pos / Mass / Type from the records (garbage and swallowed black holes are type 7), the columns host
 * arrays of pv->n entries */
int mpg_calculate_uvbg(mpg_engine *eng, const mpg_particle_view *pv, double BoxSize, const mpg_uvbg_params *par, const mpg_uvbg_columns *cols,
                       mpg_uvbg_result *result);

/* ---- snapshot / IC wire format: the "bigfile" blocks petaio.c reads and writes (libgadget/petaio.c:986-1120;
 * format: depends/bigfile/src/bigfile.c).  `file` is the snapshot directory (PART_000, an MP-GenIC output), `block` a column such
 * as "1/Position" or "Header".  dtypes are bigfile's: "f8", "f4", "i8", "u8", "i4", "u4", "u1", "S1" (little-endian).  Host IO only;
 * files written here are read by the reference library and vice versa (tests/test_snapshot_io.py). */
typedef struct mpg_bigblock_info {
    char dtype[8];   /* normalised, e.g. "<f8" */
    int nmemb;       /* values per element (3 for Position) */
    int nfile;       /* physical files of the block */
    int64_t size;    /* elements */
} mpg_bigblock_info;
int mpg_bigfile_block_info(const char *file, const char *block, mpg_bigblock_info *info);            /* big_file_open_block */
/* big_block_read with a cast: `count` elements from element `start`, converted to want_dtype, into out */
int mpg_bigfile_read_block(const char *file, const char *block, int64_t start, int64_t count, const char *want_dtype, void *out);
/* big_file_create_block + big_block_write: `size` elements of `nmemb` values stored as `dtype`, split evenly over nfile files
 * (bigfile-mpi.c:106-111); data holds src_dtype values (NULL: dtype) */
int mpg_bigfile_write_block(const char *file, const char *block, const char *dtype, int nmemb, int nfile, int64_t size, const char *src_dtype,
                            const void *data);
/* big_block_get_attr / big_block_set_attr; get returns 2 when the attribute does not exist */
int mpg_bigfile_get_attr(const char *file, const char *block, const char *name, const char *want_dtype, void *out, int nmemb);
int mpg_bigfile_set_attr(const char *file, const char *block, const char *name, const char *dtype, const void *data, int nmemb);

/* ---- matter power spectrum of the PM density field: gravpm_force measures it on every PM step (measure_power_spectrum /
 * powerspectrum_add_mode, gravpm.c:331-382: |delta_k|^2 with the CIC window removed once, weight 2 off the kz = 0 / Nyquist planes,
 * Nmesh logarithmic bins) and writes powerspectrum-<a>.txt (powerspectrum_sum / powerspectrum_save, powerspectrum.c:55-122).
 * The engine accumulates the raw sums during mpg_(dev_)gravpm_force and mpg_dev_pm_slab_forward_b.  With the neutrino linear response
 * on (mpg_gravpm_set_nu_response below) the spectrum is the total-matter one of gravpm.c:436-446. */
int mpg_gravpm_measure_power(mpg_engine *eng, int on);   /* default on, as in the reference */
/* raw sums of the last PM step into caller device arrays: d_acc[2 Nmesh + 1] = Power[Nmesh], kk[Nmesh], Norm; d_modes[Nmesh].
 * One process per GPU: sum them over the ranks (the MPI_Allreduce of powerspectrum_sum) before mpg_powerspectrum_sum. */
int mpg_dev_gravpm_powerspectrum_raw(mpg_engine *eng, double *d_acc, int64_t *d_modes);
/* powerspectrum_sum (powerspectrum.c:55-91) on host arrays: averages, normalises by Norm, converts to Mpc/h units with BoxSize_in_MPC
 * and drops empty bins; kk, Power, Nmodes hold nbins entries, *nonzero of which are filled. */
int mpg_powerspectrum_sum(int nbins, const double *acc, const int64_t *modes, double BoxSize_in_MPC, double *kk, double *Power,
                          int64_t *Nmodes, int *nonzero);
/* both steps for one GPU */
int mpg_gravpm_get_powerspectrum(mpg_engine *eng, double BoxSize_in_MPC, double *kk, double *Power, int64_t *Nmodes, int *nonzero);
/* ---- massive-neutrino linear response (MassiveNuLinRespOn: gravpm.c:72-79, 303-326, 418-446; petapm.c:311-315).
 * The reference measures P(k) of the CDM field after the r2c transform (measure_power_spectrum, gravpm.c:365-382), then
 * compute_neutrino_power (gravpm.c:308-326) runs delta_nu_from_power (neutrinos_lra.c:134-232) on delta_cdm = sqrt(Power), and
 * potential_transfer (gravpm.c:418-446) multiplies every k2 > 0 mode by nufac = 1 + nu_prefac * delta_nu_ratio(log k) (linear
 * interpolation in logknu; a log k within log 2 below logknu[0] is clamped to it, one above logknu[nonzero-1] to that), measures it
 * again (the total-matter spectrum) and multiplies Norm by MtotbyMcdm^2.  The LRA integral stays on the host: the engine calls `fn`
 * at that point of every PM step, with the normalised Mpc/h bins mpg_powerspectrum_sum gives (kk, delta_cdm = sqrt(Power), Nmodes;
 * `nonzero` entries each).  fn fills logknu[nonzero], delta_nu_ratio[nonzero], *nu_prefac, *MtotbyMcdm and returns 0; a non-zero
 * return fails the PM call ("neutrino response callback ...").  The table must have nonzero >= 2, logknu strictly increasing and every
 * value finite, else the call fails.  The measurement is made while the response is on even with mpg_gravpm_measure_power(eng, 0);
 * mpg_(dist_)gravpm_get_powerspectrum then return the total-matter spectrum.  The callback runs on the calling thread, once per PM
 * step and rank (in the several-GPU form after the bins are summed over the ranks, as powerspectrum_sum's MPI_Allreduce does: every
 * rank gets the same inputs and must return the same table).  Honoured by mpg_gravpm_force, mpg_dev_gravpm_force,
 * mpg_dist_gravpm_force, mpg_dist_dev_gravpm_force and mpg_dist_gravity_step; mpg_dev_pm_slab_forward_b refuses while it is on.
 * fn = NULL (the default) turns it off: the one-pass transfer, no host wait. */
typedef int (*mpg_nu_response_fn)(void *ctx, int nonzero, const double *kk, const double *delta_cdm, const int64_t *Nmodes, double *logknu,
                                  double *delta_nu_ratio, double *nu_prefac, double *MtotbyMcdm);
int mpg_gravpm_set_nu_response(mpg_engine *eng, mpg_nu_response_fn fn, void *ctx, double BoxSize_in_MPC);
/* hybrid neutrinos as passive tracers (hybrid_nu_tracer, gravpm.c:84-85, 469-474; petapm.c:1138-1143): while on, particles of type 2
 * are left out of the mass deposit and still receive GravPM / Potential.  mpg_gravpm_force reads the type from the particle view,
 * mpg_dev_gravpm_force from the d_type of mpg_dev_bind_particles (an error if it is NULL); for the mpg_dist forms see
 * mpg_dist_dev_set_types.  Default off. */
int mpg_gravpm_set_hybrid_nu_tracer(mpg_engine *eng, int on);
/* powerspectrum_save (powerspectrum.c:93-122): OutputDir/filename-<Time>.txt with the reference's columns "k P N P(z=0)" */
int mpg_powerspectrum_save(const char *OutputDir, const char *filename, double Time, double D1, int nonzero, const double *kk,
                           const double *Power, const int64_t *Nmodes);

/* ---- lensing potential planes (write_plane, libgadget/plane.c:572-683, called from run.c:727 at the sync points that ask for it).
 * For every cut point and every normal, in the loop order of plane.c:633-634: the active particles of the slab
 * [cut - Thickness/2, cut + Thickness/2) along the normal are COUNTED (nearest grid point, not mass) on a Resolution^2 image
 * (cutPlaneGaussianGrid / grid3d_ngb / find_bin, lenstools.c:68-124, 233-319), the counts are normalised to the density contrast and the
 * 2-D Poisson equation is solved for the lensing potential (calculate_lensing_potential, lenstools.c:168-231).  The image axes are
 * projectDensity's (lenstools.c:126-166): normal 0 -> (y, z), normal 1 -> (x, z), normal 2 -> (x, y), the first one is the row.
 * Active is lenstools_particle_is_active (lenstools.c:18-26): not Swallowed, and not type 2 while the hybrid-neutrino tracer switch
 * (mpg_gravpm_set_hybrid_nu_tracer) is on; rows with IsGarbage are skipped as well, as in every other loop of the engine (the reference
 * does not test that bit here because write_plane runs after the table has been collected).  The counters are 32-bit integers: a call
 * with 2^32 or more active rows on one rank is refused.  The pixel index is the reference's arithmetic operation for operation, so the
 * counts equal the reference's exactly.
 * With fn != NULL the massive-neutrino correction of PlaneMassiveNuCorrection (plane_pm_grid_init_neutrino_correction,
 * cutPlanePMNeutrinoCorrection, plane_add_periodic_bilinear, plane.c:313-478) is added: the active particles' mass on the engine's PM
 * mesh, its spectrum, the callback (called once per planes call with the inputs documented at mpg_nu_response_fn; its MtotbyMcdm is
 * ignored; this is NOT the callback registered with mpg_gravpm_set_nu_response: the reference runs delta_nu_from_power a second time
 * here and its state is the caller's business), every mode times nufac - 1, the mesh projected onto an Nmesh^2 image whose axes are
 * plane_directions[] = (normal + 1) % 3, (normal + 2) % 3 (plane.c:399, 421-425) - for normal 1 that is (z, x), the TRANSPOSE of the
 * particle plane's (x, z); restated as the reference has it - solved, and resampled bilinearly onto the plane.  The PM meshes are scratch
 * during the call; the spectrum of the last PM step, the registered response and the deposit tuner come out unchanged. */
typedef struct mpg_plane_params {
    int Resolution;                  /* PlaneResolution >= 1 (>= 2 with a correction, plane.c:618) */
    double Thickness;                /* PlaneThickness in internal length units; <= 0: BoxSize (plane.c:581-584) */
    int ncuts;                       /* <= 1024; 0: CutPoints[i] = (i + 1/2) Thickness, i < (int64) (BoxSize / Thickness) (plane.c:587-591) */
    const double *CutPoints;
    int nnormals;                    /* <= 3 */
    const int *Normals;              /* each 0, 1 or 2 */
    double left_corner[3];           /* the reference passes zeros (plane.c:637) */
    double atime;
    double comoving_distance;        /* compute_comoving_distance(CP, atime, 1., UnitVelocity_in_cm_per_s), internal length units */
    double HubbleParam;
    double omega_source;             /* plane_particle_omega_source (plane.c:65-74); <= 0 is an error */
    double CurrentParticleOffset[3]; /* PartManager->CurrentParticleOffset */
    mpg_nu_response_fn fn;           /* NULL: no correction */
    void *ctx;
    double BoxSize_in_MPC;           /* BoxSize * UnitLength_in_cm / CM_PER_MPC (plane.c:337), for the correction */
} mpg_plane_params;
/* the number of cut points a call with these parameters makes (the first dimension of its outputs).  BoxSize <= 0: the box of the
 * particles bound to eng (mpg_dev_bind_particles, the resident table), which is what the device and resident calls use. */
int mpg_plane_count(mpg_engine *eng, const mpg_plane_params *params, double BoxSize, int64_t *ncuts);
/* Counter memory of a planes call: ncuts x nnormals x R^2 x 4 bytes (12 with the 64-bit copy of the several-rank form).  When that
 * exceeds the budget the counting pass runs once per batch of planes.  bytes = 0 (the default): a quarter of the device memory free at
 * the call; one plane is always held. */
int mpg_set_plane_counter_budget(mpg_engine *eng, int64_t bytes);
/* On the particles of mpg_dev_bind_particles; d_flags: device bytes with bit 0 IsGarbage, bit 1 Swallowed (as mpg_dev_fof_fof takes
 * them), or NULL.  d_planes[ncuts][nnormals][R][R] doubles on the device, npart[ncuts][nnormals] on the host (num_particles_plane). */
int mpg_dev_potential_planes(mpg_engine *eng, const mpg_plane_params *params, const unsigned char *d_flags, double *d_planes, int64_t *npart);
/* the counting pass alone (grid3d_ngb + projectDensity): d_counts[ncuts][nnormals][R][R] 32-bit counters on the device, *n_active =
 * plane_count_active_particles of the bound rows (may be NULL).  For tests and measurements. */
int mpg_dev_plane_counts(mpg_engine *eng, const mpg_plane_params *params, const unsigned char *d_flags, uint32_t *d_counts, int64_t *n_active);
/* On the records of a particle view (host pointers in and out; joins a running prefetch like the other host-path calls, reuses the
 * upload of a declared epoch; on the resident table it runs on the device copies). */
int mpg_potential_planes(mpg_engine *eng, const mpg_particle_view *pv, double BoxSize, const mpg_plane_params *params, double *planes,
                         int64_t *npart);
/* On the resident table (mpg_resident_begin): positions, masses and types are the device's; IsGarbage / Swallowed are read from the
 * host records, which nothing on the device changes.  planes / npart are host arrays. */
int mpg_resident_potential_planes(mpg_engine *eng, const mpg_particle_view *pv, const mpg_plane_params *params, double *planes, int64_t *npart);

/* ---- long-range PM over several GPUs, one process per GPU (petapm.c:584-885 exchanges region meshes with 2-D pencils and lets
 * PFFT transpose; here: x-slabs of Nmesh/world planes, two all-to-all transposes per PM step and one neighbour plane).  The
 * engine does the local stages; the caller (one rank per GPU) does the collectives between them on the engine's stream:
 *
 *   mpg_dev_pm_slab_init(rank, world)        after mpg_gravpm_init_periodic; Nmesh % world == 0.  Outputs the number of complex
 *                                            values per peer block (P * Py * (Nmesh/2+1)) and the doubles of one mesh plane.
 *   mpg_dev_pm_slab_forward_a(sendA)         deposit the bound particles onto this rank's planes, 2-D r2c, pack:
 *                                            sendA[world][cplx_per_peer] complex      -> all-to-all -> recvA
 *   mpg_dev_pm_slab_forward_b(recvA, sendB)  1-D c2c along x, potential_transfer, inverse 1-D c2c of the potential:
 *                                            sendB[world][cplx_per_peer] complex      -> all-to-all -> recvB
 *   mpg_dev_pm_slab_inverse_c(recvB, ghost_send)  2-D c2r: the potential on this rank's planes; ghost_send[5][plane] = its first 3
 *                                            planes (for the previous rank) and its last 2 (for the next rank)
 *   mpg_dev_pm_slab_readout(ghost_recv, targets, n, GravPM, Potential)   ghost_recv[5][plane] = the next rank's first 3 planes, then
 *                                            the previous rank's last 2.  Forces = 4-point differences of the potential (the
 *                                            real-space form of force_transfer, gravpm.c:456-489), then readout_force_* /
 *                                            readout_potential (gravpm.c:499-510) for the listed particles, whose base cell must
 *                                            lie in this rank's slab.
 * Every rank binds the same particle set (mpg_dev_bind_particles); a particle's CIC cloud is deposited by the owners of the
 * planes it touches, so no region exchange is needed.  world == 1 reproduces mpg_dev_gravpm_force to FFT round-off (measured: 2e-14
 * of the mean force; tests/test_gpu_pm_forms.py drives the five calls with 1 - 4 engines of one process as ranks, slabs of 3 planes
 * included).  Restrictions of the stage calls: EVERY bound particle deposits with its bound mass - they take no mask of garbage /
 * swallowed records and do not apply the hybrid-neutrino tracer mask of mpg_gravpm_set_hybrid_nu_tracer (a caller compacts its set
 * or zeroes those masses first, as mpg_dist_* does); Nmesh / world >= 3; no neutrino response (forward_b refuses).  Positions may
 * lie outside [0, BoxSize]: the base cell folds by whole boxes as in the single-mesh step. */
int mpg_dev_pm_slab_init(mpg_engine *eng, int rank, int world, int64_t *cplx_per_peer, int64_t *plane_doubles);

/* ---- particles distributed over ranks (the reference: Peano-Hilbert domains, a replicated top-tree whose leaves carry the
 * moments of remote sub-trees, forcetree.c:1106-1290; here: x-slab domains, ghosts imported in whole columns of level-La
 * cells).  The bound particle set is [own particles | ghosts]; the tree built from it equals the global tree at levels >= La;
 * the nodes above get their moments from sums over all ranks:
 *   mpg_dev_tree_top_partial(La, n_own, out)  out[8^(La-1)][4] = (sum m, sum m x, sum m y, sum m z) of the OWN particles
 *                                             (caller index < n_own) per level-(La-1) cell, cells numbered by octant path
 *   -> all-reduce over ranks; coarser levels by summing 8 children
 *   mpg_dev_tree_top_set(La, sums)            sums[(8^La - 1)/7][4]: levels 0 .. La-1 concatenated; sets the moments of
 *                                             every local node above level La (error if such a node is a leaf) */
int mpg_dev_tree_top_partial(mpg_engine *eng, int La, int64_t n_own, double *d_out);
int mpg_dev_tree_top_set(mpg_engine *eng, int La, const double *d_sums);
int mpg_dev_pm_slab_forward_a(mpg_engine *eng, double *sendA);
int mpg_dev_pm_slab_forward_b(mpg_engine *eng, double *recvA, double *sendB);
int mpg_dev_pm_slab_inverse_c(mpg_engine *eng, const double *recvB, double *ghost_send);
int mpg_dev_pm_slab_readout(mpg_engine *eng, const double *ghost_recv, const int *d_targets, int64_t ntargets, double *d_gravpm,
                            double *d_potential);

/* ---- the force step on several ranks behind the CALLER's communicator ------------------------------------------------------
 * The reference's entry points are collective over MPI_COMM_WORLD (gravity.h:40,55; forcetree.h:115-148; treewalk.c:801-902;
 * petapm.c:584-885; domain.c:153-258; exchange.c).  This library links neither MPI nor RCCL: the caller hands it the three
 * collectives the path needs as callbacks over its own communicator (run.c: MPI_Allreduce / MPI_Alltoall / MPI_Alltoallv;
 * the Python host side: torch.distributed = RCCL over xGMI), and every rank calls the mpg_dist_* functions collectively, as it
 * calls gravpm_force / force_tree_full / grav_short_tree today.  All choreography (what is sent where, in which order) is in
 * the library (csrc/dist.hip and the csrc/dist_*.hip beside it); a callback only moves bytes.
 *
 * Particles live on the rank that owns their Peano-Hilbert TopLeaf (domain_decompose_full).  Per force step:
 *   PM     every particle's {Pos, Mass} goes to the rank(s) owning the x-planes its CIC cloud touches (32 B per particle: an
 *          eighth of what the reference's region meshes cost at Nmesh = 2 N^(1/3)); slab FFT with two all-to-all transposes;
 *          GravPM / Potential return to the owners.
 *   tree   a rank imports, as ghosts, the particles of every level-La tree cell within Rcut of its TopLeaves (whole cells: the
 *          local tree equals the global one at levels >= La); the nodes above get their moments from an all-reduce and are
 *          kept internal down to level La, the counterpart of the reference's replicated top-tree with pseudo nodes
 *          (forcetree.c:654-723, 1145-1284).  Ghost import replaces the export of walk targets (treewalk.c:325-793): the
 *          interaction sets are the same, there is no return trip.
 * Callback contract: return 0 on success; `on_device` says whether the buffers are device pointers (only if device_buffers
 * was set; otherwise the library stages through pinned host memory).  Counts and displacements are in BYTES. */
typedef struct mpg_comm {
    void *ctx;                 /* handed back to every callback (e.g. the MPI_Comm) */
    int ThisTask, NTask;       /* NTask <= 64 */
    int device_buffers;        /* 1: alltoallv / allreduce accept device pointers (RCCL, GPU-aware MPI) */
    /* MPI_Allreduce(MPI_IN_PLACE, buf, count, dtype ? MPI_INT64_T : MPI_DOUBLE, op ? MPI_MAX : MPI_SUM) */
    int (*allreduce)(void *ctx, void *buf, int64_t count, int dtype, int op, int on_device);
    /* MPI_Alltoall of ONE int64 per peer, host memory */
    int (*alltoall_i64)(void *ctx, const int64_t *send, int64_t *recv);
    /* MPI_Alltoallv of bytes */
    int (*alltoallv)(void *ctx, const void *send, const int64_t *sendbytes, const int64_t *sdispls, void *recv, const int64_t *recvbytes,
                     const int64_t *rdispls, int on_device);
    /* Optional (NULL: every call blocks until its data has arrived, as MPI does).  A communicator whose device-buffer collectives are
     * stream-ordered work (RCCL) sets bind_stream: mpg_dist_create calls it once with the engine's hipStream_t.  From then on a callback
     * that is handed device pointers ENQUEUES on that stream and returns at once, and the library does not synchronise around it:
     * kernels and collectives of a force step run back to back.  Calls with host pointers stay blocking. */
    int (*bind_stream)(void *ctx, void *hip_stream);
} mpg_comm;

/* ---- mpg_comm on a native RCCL communicator (csrc/rccl_comm.hip) --------------------------------------------------------------
 * Stands where the reference has MPI on this path: the query export / import of the tree walks (treewalk.c:586-655: MPI_Alltoall of
 * counts, MPI_Isend / MPI_Irecv per peer) and the PM mesh exchanges (petapm.c:751,815,869: MPI_Alltoallv) become ncclGroupStart +
 * ncclSend / ncclRecv per peer + ncclGroupEnd and ncclAllReduce on the engine's stream, device memory to device memory over xGMI.
 * librccl is opened at run time (the library does not link it).  Bootstrap: rank 0 obtains the 128-byte id, the CALLER hands it to
 * every rank (MPI_Bcast: shim/mpg_rccl_mpi.c; torch.distributed: bench.py; shared memory: tests/c/test_cabi.c), then every rank calls
 * mpg_rccl_create (collective: ncclCommInitRank) on ITS device and passes the callbacks of mpg_rccl_comm to mpg_dist_create.
 * mpg_rccl_selftest runs every collective once on a known pattern (collective) and fails if a byte differs. */
#define MPG_RCCL_ID_BYTES 128
typedef struct mpg_rccl mpg_rccl;
int mpg_rccl_available(void);                 /* 1 if librccl could be opened */
int mpg_rccl_get_unique_id(void *id128);
int mpg_rccl_create(mpg_rccl **out, int ThisTask, int NTask, const void *id128, int device);
int mpg_rccl_comm(mpg_rccl *r, mpg_comm *out);
int mpg_rccl_selftest(mpg_rccl *r, int64_t bytes_per_peer);
/* calls3: allreduce, alltoall_i64, alltoallv calls so far; bytes sent to OTHER ranks; the RCCL version code (any may be NULL) */
int mpg_rccl_stats(mpg_rccl *r, int64_t *calls3, int64_t *bytes_sent, int *version);
/* what RCCL reports for the communicator: ncclCommCount, ncclCommUserRank, and the HIP device it was created on (any may be NULL) */
int mpg_rccl_comm_info(mpg_rccl *r, int *nranks, int *rank, int *device);
const char *mpg_rccl_last_error(mpg_rccl *r); /* detail of the last failed callback */
void mpg_rccl_destroy(mpg_rccl *r);

typedef struct mpg_dist mpg_dist;
/* eng: configured as for one rank (mpg_gravpm_init_periodic with the GLOBAL Nmesh, tables, tree parameters, softening);
 * Nmesh % NTask == 0.  The comm struct is copied. */
int mpg_dist_create(mpg_dist **out, mpg_engine *eng, const mpg_comm *comm);
void mpg_dist_destroy(mpg_dist *d);
/* domain_decompose_full (domain.c:153-258) over the communicator: policies, the rank's key sample, local refinement, the pairwise
 * combination of the ranks' trees, global refinement, the TopLeaves and their balanced assignment (by particle number, or by the
 * per-particle work d_cost[n] when given: mpg_dist_walk_cost), P[].TopLeaf and the destination task of every particle.  d_garbage:
 * device bytes (IsGarbage) or NULL.  Then mpg_dist_domain_exchange moves the particles (domain_exchange, exchange.c): ncols <= 16
 * columns of col_bytes[j] bytes per particle each (device arrays over the n particles); on return *n_new particles live on this
 * rank and d_new_cols[j] point to their columns in library-owned device buffers (valid until the next exchange), the particles that
 * stayed and those that arrived in source-rank order; garbage is dropped.  mpg_dist_domain_get copies the decomposition out (arrays
 * sized by the counts mpg_dist_domain_decompose returned; any may be NULL); mpg_dist_use_decomposition hands it to the force step
 * (= mpg_dist_set_domain with it). */
int mpg_dist_domain_decompose(mpg_dist *d, int64_t n, const double *d_pos, const unsigned char *d_garbage, double BoxSize,
                              int DomainOverDecompositionFactor, int DomainUseGlobalSorting, const float *d_cost, int *NTopNodes,
                              int *NTopLeaves);
int mpg_dist_domain_get(mpg_dist *d, mpg_topnode *TopNodes, int *leaf_task, int *StartLeaf, int *EndLeaf, int64_t *TopLeafCount);
int mpg_dist_domain_exchange(mpg_dist *d, int64_t n, int ncols, const void *const *d_cols, const int *col_bytes, int64_t *n_new,
                             void **d_new_cols);
int mpg_dist_use_decomposition(mpg_dist *d, double BoxSize, double margin, int La);
/* domain_maintain (domain.c:262-319) after a drift: the decomposition is kept, TopLeaf and destination task of every particle are
 * found again; *n_leaving (may be NULL) = the particles that mpg_dist_domain_exchange will now move to other ranks */
int mpg_dist_domain_maintain(mpg_dist *d, int64_t n, const double *d_pos, const unsigned char *d_garbage, double BoxSize, int64_t *n_leaving);
/* The domain the ranks' particles were distributed by: the TopNodes of domain_decompose_full (same on every rank) and the Task
 * of every TopLeaf (DomainDecomp.TopNodes / TopLeaves, domain.h:12-43).  margin: at least Rcut in length units (the walk's
 * cut-off, gravshort-tree.c:102) and, for SPH, the largest smoothing length; La = 0 picks the level whose cells are
 * [margin, 2 margin) wide. */
int mpg_dist_set_domain(mpg_dist *d, double BoxSize, const mpg_topnode *TopNodes, int NTopNodes, const int *leaf_task, int NTopLeaves,
                        double margin, int La);
/* gravpm_force + force_tree_full + grav_short_tree for the rank's OWN particles (device arrays, n_own rows; all active).
 * d_prev_accel (may be NULL): last step's FullTreeGravAccel for the relative opening criterion, else d_oldacc (|a|/G per
 * particle, may be NULL -> Barnes-Hut walk if TreeUseBH says so).  Outputs: d_gravpm[n_own][3] assigned, d_accel[n_own][3]
 * assigned, d_potential[n_own] (may be NULL) = PM + tree potential as the reference leaves it in P[].Potential. */
int mpg_dist_gravity_step(mpg_dist *d, int64_t n_own, const double *d_pos, const float *d_mass, const double *d_oldacc,
                          const double *d_prev_accel, double *d_accel, double *d_gravpm, double *d_potential, double rho0);
/* The three entry points separately, in the reference's order (run.c:522-548) - gravity_step is exactly this sequence:
 *   gravpm_force (gravity.h:55)          -> GravPM assigned, Potential accumulated (readout_potential, gravpm.c:499-501)
 *   force_tree_full (forcetree.h:115)    -> ghost import, local tree with the global top
 *   grav_short_tree (gravity.h:40)       -> accelerations of all own particles (and the tree potential, assigned) */
int mpg_dist_dev_gravpm_force(mpg_dist *d, int64_t n_own, const double *d_pos, const float *d_mass, double *d_gravpm, double *d_potential);
/* The types of the own rows (n_own device bytes, caller order) for the hybrid-neutrino deposit mask (mpg_gravpm_set_hybrid_nu_tracer on
 * the rank's engine): the typed form of mpg_dist_dev_gravpm_force and mpg_dist_gravity_step.  While the mask is on, those two calls fail
 * unless types for the same n_own were set; stays in force until the next call (NULL clears it).  The host forms read the type of the
 * particle view themselves. */
int mpg_dist_dev_set_types(mpg_dist *d, int64_t n_own, const uint8_t *d_type);
/* Garbage and swallowed particles among the own rows (P[].IsGarbage, P[].Swallowed: star formation and black-hole mergers leave them in
 * the table until the next domain_decompose_full collects them).  The reference skips them in place in every loop of this path
 * (treewalk.c:234, forcetree.c:806, gravpm.c:176-179); so do the mpg_dist_dev_* calls that follow on a table of n_own rows: such rows are
 * shipped nowhere, are not in the local tree, are no targets; their GravPM is zeroed, their other outputs are left alone.
 * d_garbage: n_own device bytes (non-zero = skip) or NULL for none; stays in force until the next call.  The host forms
 * (mpg_dist_gravpm_force, ...) read the flag byte of the particle view themselves. */
int mpg_dist_dev_set_garbage(mpg_dist *d, int64_t n_own, const unsigned char *d_garbage);
int mpg_dist_dev_force_tree_build(mpg_dist *d, int64_t n_own, const double *d_pos, const float *d_mass);
int mpg_dist_dev_grav_short_tree(mpg_dist *d, const double *d_oldacc, const double *d_prev_accel, const double *d_gravpm, double *d_accel,
                                 double *d_potential, double rho0);
/* Hierarchical gravity (timestep.c: hierarchical_gravity_accelerations; force_tree_active_moments, forcetree.c:129-148): the short-range
 * force of the ACTIVE particles on each other, on the tree of the active particles only.  d_pos / d_mass / d_oldacc hold the rank's
 * n_act active particles (compacted by the caller), d_accel[n_act][3] is assigned; d_potential is not touched (the tree is not the full
 * particle tree: gravshort.h:57-67 leaves P[].Potential and FullTreeGravAccel alone then).  Such sets are sparse and small: every rank receives the whole set (one all-gather of
 * 28 bytes per particle), builds the tree one GPU would build and walks its own members, so the results are those of one GPU.  The
 * local tree of mpg_dist_dev_force_tree_build is replaced (build it again before the next walk on all particles). */
int mpg_dist_dev_grav_short_tree_active_tree(mpg_dist *d, int64_t n_act, const double *d_pos, const float *d_mass, const double *d_oldacc,
                                             double *d_accel, double *d_potential, double rho0);
/* ... as a drop-in call: the active particles are gathered from the rank's P[] (OldAcc from P[].FullTreeGravAccel + GravPM), their
 * AccelStore[i] is assigned, P[] is left alone.  ActiveParticle == NULL: all particles of the table. */
int mpg_dist_grav_short_tree_active_tree(mpg_dist *d, const mpg_particle_view *pv, const int *ActiveParticle, int64_t NumActiveParticle,
                                         double (*AccelStore)[3], double rho0);
/* the same for a subset of the own particles: d_active[nactive] = their indices (device array, no duplicates), the ActiveParticle list of a
 * sub-step (run.c:392-470: the tree holds every particle, the active ones are walked).  Only their entries of d_accel / d_potential are
 * written.  d_active == NULL: all own particles. */
int mpg_dist_dev_grav_short_tree_active(mpg_dist *d, const int *d_active, int64_t nactive, const double *d_oldacc, const double *d_prev_accel,
                                        const double *d_gravpm, double *d_accel, double *d_potential, double rho0);
/* density() and hydro_force() (density.h:42, hydra.h) for the rank's own gas on the particle set of the last
 * mpg_dist_dev_force_tree_build (own + ghosts; the domain margin must cover the largest smoothing length: checked).  d_type and the
 * arrays of A are device arrays over the n_own own particles (mpg_sph_arrays; optional inputs may be NULL); the ghosts' columns
 * travel along the ghost plan, and between the two loops the ghosts' Hsml / Density / EgyWtDensity / DhsmlEgyDensityFactor / DivVel /
 * CurlVel are refreshed from their owners. */
int mpg_dist_dev_density(mpg_dist *d, int64_t n_own, const uint8_t *d_type, const mpg_sph_arrays *A, const mpg_sph_times *T, int update_hsml,
                         int DoEgyDensity);
int mpg_dist_dev_hydro_force(mpg_dist *d, int64_t n_own, const mpg_sph_arrays *A, const mpg_sph_times *T);
/* ... for a sub-step: only the own gas among d_active[nactive] (device array of own-particle indices; NULL = all) is treated; the arrays
 * of A must then hold, for the other particles, the results of their last loops (they are read: the hydro loop and the ghosts need the
 * inactive particles' Density ... CurlVel) and those entries come back unchanged, as the reference leaves SphP of inactive particles */
int mpg_dist_dev_density_active(mpg_dist *d, int64_t n_own, const uint8_t *d_type, const mpg_sph_arrays *A, const mpg_sph_times *T,
                                const int *d_active, int64_t nactive, int update_hsml, int DoEgyDensity);
int mpg_dist_dev_hydro_force_active(mpg_dist *d, int64_t n_own, const mpg_sph_arrays *A, const mpg_sph_times *T, const int *d_active,
                                    int64_t nactive);
/* fof_fof (fof.c:157-253) with the particles on their owners: groups may span ranks.  Device arrays over the n_own own particles
 * (d_type NULL: all type 1; d_vel NULL: zero); the linking length must not exceed the domain margin.  d_grnr[n_own] (may be NULL)
 * receives P[].GrNr with GLOBAL group numbers (length descending, then MinID); *ngroups_total = fof.TotNgroups; this rank keeps the
 * *ngroups_here groups with MinID % NTask == ThisTask: mpg_dist_fof_groups copies their table into HOST arrays. */
int mpg_dist_dev_fof_fof(mpg_dist *d, int64_t n_own, const double *d_pos, const float *d_mass, const uint8_t *d_type, const uint64_t *d_id,
                         const double *d_vel, const mpg_fof_params *par, int64_t *d_grnr, int64_t *ngroups_total, int64_t *ngroups_here);
int mpg_dist_fof_groups(mpg_dist *d, const mpg_fof_groups *out);
/* ... and as drop-in calls on the rank's particle table in host memory (what libgadget's callers hand over; shim/gravity-hip.c):
 * Pos / Mass are read from P[], GravPM / FullTreeGravAccel / Potential (and AccelStore, may be NULL) are written as the reference's
 * functions write them; OldAcc of the walk comes from P[].FullTreeGravAccel + P[].GravPM.  All particles active (a PM step). */
int mpg_dist_gravpm_force(mpg_dist *d, const mpg_particle_view *pv);
int mpg_dist_force_tree_full(mpg_dist *d, const mpg_particle_view *pv);
int mpg_dist_grav_short_tree(mpg_dist *d, const mpg_particle_view *pv, double (*AccelStore)[3], double rho0);
/* ... for the sub-steps: ActiveParticle[NumActiveParticle] (host array of indices into P[], NULL = all) are walked, their
 * FullTreeGravAccel / Potential / AccelStore entries updated (the tree of mpg_dist_force_tree_full holds every particle) */
int mpg_dist_grav_short_tree_active(mpg_dist *d, const mpg_particle_view *pv, const int *ActiveParticle, int64_t NumActiveParticle,
                                    double (*AccelStore)[3], double rho0);
/* density() / hydro_force() as drop-in calls on the same table (after mpg_dist_force_tree_full on it): A holds HOST arrays in particle
 * order, as for mpg_density / mpg_hydro_force (the shim gathers SphP[P[i].PI].X into them); inputs are read, outputs written.
 * ActiveParticle[NumActiveParticle]: host array of indices into P[] (NULL = all), see mpg_dist_dev_density_active */
/* BlackHoleOn of density() (density.c:234) for the following mpg_dist_(dev_)density calls.  The own black holes that are not swallowed
 * are targets of the density loop next to the gas in any case (density_haswork, density.c:521-530: Hsml, Density and DivVel of BHP);
 * BlackHoleOn gives them BlackHoleNgbFactor times the neighbours and caps their radius (density.c:598-600, 667-670).  The smoothing
 * lengths of both must lie within the domain margin.  Swallowed black holes and garbage carry type 7 in d_type (the host form reads
 * the flag bits). */
int mpg_dist_set_sph_options(mpg_dist *d, int BlackHoleOn);
/* the largest smoothing length over all ranks at the end of the last mpg_dist_(dev_)density loop.  When that call failed because it
 * exceeds the domain margin (the neighbours of such a particle are not all local), set the domain again with a margin above this
 * value, rebuild the local tree and repeat the call: the inputs were not modified. */
double mpg_dist_last_max_hsml(mpg_dist *d);
/* PartManager->MaxPart for domain_check_memory_bound (domain.c:378-424): a decomposition that gives one task more particles is retried
 * with the next policy (domain.c:199-201).  0 (default): no bound. */
int mpg_dist_domain_set_maxpart(mpg_dist *d, int64_t MaxPart);
/* the matter power spectrum of the last mpg_dist_(dev_)gravpm_force over all ranks (gravpm.c:110-118; powerspectrum_sum's
 * MPI_Allreduce, powerspectrum.c:55-91).  Collective; arrays of Nmesh entries, *nonzero of which are filled on every rank. */
int mpg_dist_gravpm_get_powerspectrum(mpg_dist *d, double BoxSize_in_MPC, double *kk, double *Power, int64_t *Nmodes, int *nonzero);
/* write_plane over the ranks (plane.c:572-683), collective: every rank passes its OWN rows (device arrays; d_mass / d_type / d_flags may
 * be NULL) and the parameters of mpg_dev_potential_planes, and receives the planes and npart of the whole box.  Each rank counts its rows;
 * the counters are widened to 64-bit integers and summed with the communicator's allreduce, as are the active-particle number and
 * npart.  (The reference reduces the finished potentials, plane.c:654; the solve is linear, so summing the integer counts first is the
 * same plane with one solve instead of one per rank.)  The call leaves the rows bound to the engine.  With params->fn != NULL and more
 * than one rank it fails with "the massive-neutrino correction on several ranks is not implemented" on every rank, before any collective.
 * The number of planes per batch is agreed on over the ranks (the smallest any rank's budget holds), and a refusal of one rank's counting
 * pass (a position that cannot be wrapped, 2^32 active rows) is all-reduced, so every rank returns that error together.  Errors of the
 * parameters are the same on every rank by construction.  NOT collective-safe: a failed device allocation or a HIP error on one rank. */
int mpg_dist_potential_planes(mpg_dist *d, int64_t n_own, const double *d_pos, const float *d_mass, const uint8_t *d_type,
                              const unsigned char *d_flags, double BoxSize, const mpg_plane_params *params, double *d_planes, int64_t *npart);
int mpg_dist_density(mpg_dist *d, const mpg_particle_view *pv, const mpg_sph_arrays *A, const mpg_sph_times *T, const int *ActiveParticle,
                     int64_t NumActiveParticle, int update_hsml, int DoEgyDensity);
int mpg_dist_hydro_force(mpg_dist *d, const mpg_particle_view *pv, const mpg_sph_arrays *A, const mpg_sph_times *T, const int *ActiveParticle,
                         int64_t NumActiveParticle);
/* per-particle work of the last mpg_dist walk for the rank's own particles (device pointer, n_own floats, caller order):
 * the cost the next domain decomposition balances (mpg_dev_set_walk_cost) */
const float *mpg_dist_walk_cost(mpg_dist *d);
/* what the last step moved: [0] ghosts imported, [1] particles shipped to PM slabs, [2] local tree particles (own + ghosts),
 * [3] decomposition level La, [4] bytes sent in personalised exchanges, [5] bytes sent in transposes */
int mpg_dist_get_stats(mpg_dist *d, int64_t stats[8]);
/* phase times of the last step in ms (host clock around stream synchronisations): [0] PM shipping + slab PM, [1] ghost import,
 * [2] tree build + global top, [3] walk.  After mpg_dist_gravity_step, which builds the local tree on a second stream beside the PM
 * step (MPG_DIST_NO_OVERLAP=1: one after the other): [0] PM with the tree build beside it, [2] global top + targets, [4] the tree build
 * on its own stream */
int mpg_dist_get_times(mpg_dist *d, double ms[8]);
/* cells of the tree above this level are kept internal (never leaves) by the next tree builds; 0 restores forcetree.c's rule.
 * Used by the distributed step; exposed for tests. */
int mpg_dev_force_tree_set_min_leaf_level(mpg_engine *eng, int level);

/* Tuning knobs of the walk; results do not depend on any of them.
 *   variant   0 = auto (default): kernel 6 for 4096 targets or more, kernel 1 below that;
 *             1 = lane-per-target while-while kernel (grav_walk.hip); 4 = group-cooperative list kernel (grav_walk_coop.hip);
 *             6 = two kernels, list construction then evaluation (grav_walk_split.hip)
 *   threshold (kernel 1) the node phase keeps running while at least that many lanes of a wave still search (default 16)
 *   list capacity (kernels 4, 6) interaction-list entries per target (default 512): kernel 4 drains its lists when they are
 *             full; kernel 6 hands targets with longer lists to kernel 1 and doubles its capacity when > 2 % of them do */
int mpg_set_walk_threshold(mpg_engine *eng, int thresh);
/* kernel 6: overlap != 0 builds the lists of slice k+1 on a second stream while slice k is evaluated (default on);
 * chunks_per_wave = 0 uses persistent grids, > 0 that many 8-target chunks per wave (default 2) */
int mpg_set_walk_split_mode(mpg_engine *eng, int overlap, int chunks_per_wave);
int mpg_set_walk_list_capacity(mpg_engine *eng, int cap);
/* kernel 6: on != 0 takes the kernels' 64-bit-offset variants whatever the array sizes (default: only when the source and node arrays exceed
 * 4 GiB, i.e. from about 512^3 particles in one tree); results do not depend on it */
int mpg_set_walk_offsets64(mpg_engine *eng, int on);
int mpg_set_walk_variant(mpg_engine *eng, int variant);
/* kernel in use (the explicit variant, or the default policy's pick: 6 for >= 4096 targets, else 1; 0 = no walk yet), kernel 6's current list capacity and
 * the number of targets its last walk handed to the fallback kernel (either output may be NULL) */
int mpg_get_walk_choice(mpg_engine *eng, int *variant, int *list_capacity, unsigned *last_overflow);

#ifdef __cplusplus
}
#endif
#endif /* MPGADGET_HIP_H */
