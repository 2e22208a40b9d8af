// resident.hip -- the host-pointer entry points on a device-RESIDENT particle table (mpg_resident_*): the table, a gas run's SPH arrays and
// time bins, the integrator forwards, hierarchical gravity, planes, the velocity dispersion, the cooling and the metal return.
#include "engine_internal.h"

/* ---- device-resident drop-in mode ------------------------------------------------------------------------------------------
 * The host-pointer calls of host_forms.hip move Pos / Mass up and GravPM / FullTreeGravAccel / Potential down on every call because the caller
 * may have changed P[] in between: at 256^3 that is half of a step (bench.py host_path).  A caller that lets the engine integrate -
 * mpg_dev_drift_all_particles, mpg_dev_apply_pm_half_kick, mpg_dev_apply_half_kick on the arrays of mpg_resident_arrays - declares
 * the table resident: one upload, then gravpm_force / force_tree_* / grav_short_tree on the same mpg_particle_view run on the device
 * copies and leave their results there; the host asks for the columns its other modules read (mpg_resident_fetch) and hands back
 * what they changed (mpg_resident_push).  Anything that reorders or resizes P[] (domain exchange, garbage collection) goes between
 * mpg_resident_end and a new mpg_resident_begin. */
namespace {
// one column of the AoS table <-> a device array of w doubles per particle
void column_to_device(mpg_engine *eng, const mpg_particle_view &V, int64_t off, int w, double *dev)
{
    const int64_t n = V.n;
    eng->h_d.reserve((size_t)w * n + 1);
    double *h = eng->h_d.p;
    const HostTable T(V);
    hipStream_t st = eng->stream;
    for_each_chunk(n, [=](int64_t lo, int64_t hi) {
        parallel_for(hi - lo, [=](int64_t a0, int64_t a1) {
            for(int64_t i = lo + a0; i < lo + a1; i++)
                for(int k = 0; k < w; k++)
                    h[w * i + k] = T.vec(i, off)[k];
        });
        MPG_HIP(hipMemcpyAsync(dev + w * lo, h + w * lo, (size_t)w * (hi - lo) * sizeof(double), hipMemcpyHostToDevice, st));
    });
    MPG_HIP(hipStreamSynchronize(st));
}

void column_to_host(mpg_engine *eng, const mpg_particle_view &V, int64_t off, int w, const double *dev)
{
    const int64_t n = V.n;
    eng->h_d.reserve((size_t)w * n + 1);
    double *h = eng->h_d.p;
    const HostTable T(V);
    hipStream_t st = eng->stream;
    download_chunks(
        eng->chunk_ev, st, n,
        [=](int64_t lo, int64_t hi) { MPG_HIP(hipMemcpyAsync(h + w * lo, dev + w * lo, (size_t)w * (hi - lo) * sizeof(double), hipMemcpyDeviceToHost, st)); },
        [=](int64_t lo, int64_t hi) {
            for(int64_t i = lo; i < hi; i++)
                for(int k = 0; k < w; k++)
                    T.vec_mut(i, off)[k] = h[w * i + k];
        });
}

void resident_check(mpg_engine *eng, const mpg_particle_view *P)
{
    MPG_CHECK(eng && P, "null argument");
    MPG_CHECK(eng->resident && eng->res_base == P->base && eng->res_n == P->n, "not the resident particle table (mpg_resident_begin first)");
    MPG_HIP(hipSetDevice(eng->device));
}
} // namespace

int mpg_resident_begin(mpg_engine *eng, const mpg_particle_view *P, double BoxSize)
{
    API_BEGIN
    MPG_CHECK(eng && P, "null argument");
    MPG_CHECK(P->off_accel >= 0 && P->off_gravpm >= 0 && P->off_potential >= 0, "resident mode needs FullTreeGravAccel, GravPM and Potential in the view");
    MPG_HIP(hipSetDevice(eng->device));
    eng->host_join(); // (a prefetch in flight writes the staging state set below)
    eng->resident = false;
    eng->staged_epoch = -1; // (force the upload whatever epoch the caller declared)
    stage_particles(eng, P, BoxSize);
    const size_t n = (size_t)P->n;
    eng->r_accel.reserve(3 * n + 3);
    eng->r_gravpm.reserve(3 * n + 3);
    eng->r_pot.reserve(n + 1);
    column_to_device(eng, *P, P->off_accel, 3, eng->r_accel.p);
    column_to_device(eng, *P, P->off_gravpm, 3, eng->r_gravpm.p);
    column_to_device(eng, *P, P->off_potential, 1, eng->r_pot.p);
    eng->res_has_vel = P->off_vel >= 0;
    if(eng->res_has_vel) {
        eng->r_vel.reserve(3 * n + 3);
        column_to_device(eng, *P, P->off_vel, 3, eng->r_vel.p);
    }
    eng->resident = true;
    eng->res_base = P->base;
    eng->res_n = P->n;
    API_END
}

int mpg_resident_arrays(mpg_engine *eng, mpg_resident_view *out)
{
    API_BEGIN
    MPG_CHECK(eng && out && eng->resident, "mpg_resident_arrays: no resident table");
    out->n = eng->res_n;
    out->d_pos = eng->s_pos.p;
    out->d_mass = eng->s_mass.p;
    out->d_type = eng->s_type.p;
    out->d_vel = eng->res_has_vel ? eng->r_vel.p : nullptr; // (a buffer left by an earlier session is not this table's Vel)
    out->d_fulltree_accel = eng->r_accel.p;
    out->d_gravpm = eng->r_gravpm.p;
    out->d_potential = eng->r_pot.p;
    API_END
}

int mpg_resident_fetch(mpg_engine *eng, const mpg_particle_view *P, unsigned fields)
{
    API_BEGIN
    resident_check(eng, P);
    if(fields & MPG_FIELD_POS)
        column_to_host(eng, *P, P->off_pos, 3, eng->s_pos.p);
    if((fields & MPG_FIELD_VEL) && P->off_vel >= 0 && eng->res_has_vel)
        column_to_host(eng, *P, P->off_vel, 3, eng->r_vel.p);
    if(fields & MPG_FIELD_ACCEL)
        column_to_host(eng, *P, P->off_accel, 3, eng->r_accel.p);
    if(fields & MPG_FIELD_GRAVPM)
        column_to_host(eng, *P, P->off_gravpm, 3, eng->r_gravpm.p);
    if(fields & MPG_FIELD_POTENTIAL)
        column_to_host(eng, *P, P->off_potential, 1, eng->r_pot.p);
    API_END
}

int mpg_resident_push(mpg_engine *eng, const mpg_particle_view *P, unsigned fields)
{
    API_BEGIN
    resident_check(eng, P);
    if(fields & MPG_FIELD_POS) {
        column_to_device(eng, *P, P->off_pos, 3, eng->s_pos.p);
        eng->pm_queued = false;
    }
    if((fields & MPG_FIELD_VEL) && P->off_vel >= 0) {
        eng->r_vel.reserve(3 * (size_t)P->n + 3);
        column_to_device(eng, *P, P->off_vel, 3, eng->r_vel.p);
        eng->res_has_vel = true;
    }
    if(fields & MPG_FIELD_ACCEL)
        column_to_device(eng, *P, P->off_accel, 3, eng->r_accel.p);
    if(fields & MPG_FIELD_GRAVPM)
        column_to_device(eng, *P, P->off_gravpm, 3, eng->r_gravpm.p);
    if(fields & MPG_FIELD_POTENTIAL)
        column_to_device(eng, *P, P->off_potential, 1, eng->r_pot.p);
    API_END
}

int mpg_resident_end(mpg_engine *eng, const mpg_particle_view *P)
{
    API_BEGIN
    resident_check(eng, P);
    MPG_CALL(mpg_resident_fetch(eng, P, MPG_FIELD_POS | MPG_FIELD_VEL | MPG_FIELD_ACCEL | MPG_FIELD_GRAVPM | MPG_FIELD_POTENTIAL));
    MPG_CHECK(!eng->sph_resident, "mpg_resident_end: the gas arrays are still resident (mpg_resident_sph_end first)");
    if(eng->r_stored_host) { // the StoredGravAccel of a split-gravity step left between its two halves goes back to the caller's array
        MPG_HIP(hipMemcpyAsync(eng->r_stored_host, eng->r_stored.p, 3 * (size_t)P->n * sizeof(double), hipMemcpyDeviceToHost, eng->stream));
        MPG_HIP(hipStreamSynchronize(eng->stream));
        eng->r_stored_host = nullptr;
    }
    eng->resident = false;
    eng->res_has_vel = false;
    eng->res_base = nullptr;
    eng->res_n = -1;
    eng->staged_epoch = -1;
    API_END
}

int mpg_resident_potential_planes(mpg_engine *eng, const mpg_particle_view *P, const mpg_plane_params *params, double *planes, int64_t *npart)
{
    API_BEGIN
    resident_check(eng, P);
    MPG_CHECK(params, "null argument");
    MPG_CHECK(eng->d_pos == eng->s_pos.p && eng->n == P->n, "resident mode: the binding changed (mpg_resident_end / _begin)");
    host_planes(eng, P, params, planes, npart);
    API_END
}

/* ---- a resident gas run: the SPH arrays stay in HBM between the calls, the integrator runs there (include/mpgadget_hip.h) ---- */
namespace {
__global__ void __launch_bounds__(256) k_flags_from_type(int64_t n, const uint8_t *__restrict__ type, uint8_t *__restrict__ flags)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if(i < n)
        flags[i] = (type[i] & 7) == 7 ? 1 : 0; // (stage_particles gave garbage and swallowed particles type 7)
}
// the garbage flags of the resident table for the integrator kernels
void resident_flags(mpg_engine *eng, int64_t n)
{
    eng->r_flags.reserve((size_t)n + 1);
    if(n > 0)
        hipLaunchKernelGGL(k_flags_from_type, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, eng->stream, n, eng->s_type.p, eng->r_flags.p);
}
void resident_sph_check(mpg_engine *eng, const mpg_particle_view *P)
{
    resident_check(eng, P);
    MPG_CHECK(eng->sph_resident, "no resident gas arrays (mpg_resident_sph_begin first)");
}
// the arrays of the time-step searches on a resident gas run
mpg_hydrostep_arrays resident_hydrostep_arrays(mpg_engine *eng)
{
    const mpg_sph_arrays &d = eng->res_sph_dev;
    mpg_hydrostep_arrays H{};
    H.d_type = eng->s_type.p;
    H.d_flags = eng->r_flags.p;
    H.d_hsml = d.hsml;
    H.d_dthsml = d.dthsml;
    H.d_maxsignalvel = d.maxsignalvel;
    H.d_tb_grav = d.tb_grav;
    H.d_tb_hydro = (unsigned char *)d.tb_hydro;
    return H;
}
} // namespace

int mpg_resident_sph_begin(mpg_engine *eng, const mpg_particle_view *P, const mpg_sph_arrays *A)
{
    API_BEGIN
    MPG_CHECK(eng && P && A, "null argument");
    resident_check(eng, P);
    MPG_CHECK(eng->res_has_vel, "mpg_resident_sph_begin: the resident table has no Vel column (the view's off_vel)");
    MPG_CHECK(A->hsml && A->entropy && A->density && A->dhsmlegyfac && A->divvel && A->curlvel && A->hydroacc_out && A->dtentropy_out &&
                  A->maxsignalvel,
              "mpg_resident_sph_begin: hsml, entropy, density, dhsmlegyfac, divvel, curlvel, hydroacc_out, dtentropy_out and maxsignalvel are required");
    const int64_t n = P->n;
    mpg_sph_arrays d;
    stage_sph(eng, A, &d, n);
    // the arrays stage_sph only clears hold state of the previous step that the predictions and the drift read: DtHsml, HydroAccel, DtEntropy
    for(const SphField &F : SPH_FIELDS) {
        void *h = field_get(*A, F.off);
        if(h && F.width > 0 && !(F.role & (SPH_IN | SPH_HYDRO_IN)))
            MPG_HIP(hipMemcpyAsync(field_get(d, F.off), h, sph_field_bytes(F, n), hipMemcpyHostToDevice, eng->stream));
    }
    // one field each in the reference: SphP.HydroAccel and SphP.DtEntropy are what the next step's predictions read; P[].Vel,
    // FullTreeGravAccel and GravPM are the resident table's
    d.hydroacc_in = d.hydroacc_out;
    d.dtentropy_in = d.dtentropy_out;
    d.vel = eng->r_vel.p;
    d.gacc = eng->r_accel.p;
    d.gpm = eng->r_gravpm.p;
    resident_flags(eng, n);
    MPG_HIP(hipStreamSynchronize(eng->stream));
    eng->res_sph_host = *A;
    eng->res_sph_dev = d;
    eng->sph_resident = true;
    API_END
}

int mpg_resident_sph_arrays(mpg_engine *eng, mpg_sph_arrays *out)
{
    API_BEGIN
    MPG_CHECK(eng && out && eng->sph_resident, "mpg_resident_sph_arrays: no resident gas arrays");
    *out = eng->res_sph_dev;
    API_END
}

int mpg_resident_sph_end(mpg_engine *eng, const mpg_sph_arrays *A)
{
    API_BEGIN
    MPG_CHECK(eng && A && eng->sph_resident, "mpg_resident_sph_end: no resident gas arrays");
    MPG_CHECK(A->hsml == eng->res_sph_host.hsml, "mpg_resident_sph_end: not the arrays mpg_resident_sph_begin took");
    MPG_HIP(hipSetDevice(eng->device));
    const int64_t n = eng->res_n;
    for(const SphField &F : SPH_FIELDS) {
        // everything the device may have changed: the outputs, Entropy (kicks), the time bins; not the aliases of the table's columns
        // nor the prediction inputs that alias the outputs
        void *h = field_get(*A, F.off);
        if(h && !(F.role & (SPH_TABLE_ALIAS | SPH_PRED_ALIAS)))
            MPG_HIP(hipMemcpyAsync(h, field_get(eng->res_sph_dev, F.off), sph_field_bytes(F, n), hipMemcpyDeviceToHost, eng->stream));
    }
    MPG_HIP(hipStreamSynchronize(eng->stream));
    eng->sph_resident = false;
    if(eng->d_delaytime == eng->s_delaytime.p) // the column of mpg_resident_sph_set_delaytime ends with the stretch
        eng->d_delaytime = nullptr;
    if(eng->cooling.d_j21 && eng->cooling.d_j21 == eng->cooling.s_j21.p) { // ... and so do those of mpg_resident_sph_set_excursion_columns
        eng->cooling.d_j21 = eng->cooling.d_zre = nullptr;
        eng->cooling.n_exc = 0;
    }
    API_END
}

// SphP.local_J21 / SphP.zreion of a resident gas run for the cooling and star formation of the stretch: uploaded now, in effect until the
// next call or the end of the stretch
int mpg_resident_sph_set_excursion_columns(mpg_engine *eng, const double *local_J21, const double *zreion)
{
    API_BEGIN
    MPG_CHECK(eng && eng->sph_resident, "mpg_resident_sph_set_excursion_columns: no resident gas arrays");
    MPG_CHECK((local_J21 == nullptr) == (zreion == nullptr), "mpg_resident_sph_set_excursion_columns: local_J21 and zreion go together");
    MPG_HIP(hipSetDevice(eng->device));
    CoolingEngine &E = eng->cooling;
    const int64_t n = eng->res_n;
    if(!local_J21 || n <= 0) {
        if(E.d_j21 && E.d_j21 == E.s_j21.p) {
            E.d_j21 = E.d_zre = nullptr;
            E.n_exc = 0;
        }
    }
    else {
        E.s_j21.reserve((size_t)n + 1);
        E.s_zre.reserve((size_t)n + 1);
        MPG_HIP(hipMemcpyAsync(E.s_j21.p, local_J21, (size_t)n * sizeof(double), hipMemcpyHostToDevice, eng->stream));
        MPG_HIP(hipMemcpyAsync(E.s_zre.p, zreion, (size_t)n * sizeof(double), hipMemcpyHostToDevice, eng->stream));
        MPG_HIP(hipStreamSynchronize(eng->stream));
        E.d_j21 = E.s_j21.p;
        E.d_zre = E.s_zre.p;
        E.n_exc = n;
    }
    API_END
}

// SphP.DelayTime of a resident gas run for hydro_force's decoupling: uploaded now, in effect until the next call or the end of the stretch
int mpg_resident_sph_set_delaytime(mpg_engine *eng, const double *delaytime)
{
    API_BEGIN
    MPG_CHECK(eng && eng->sph_resident, "mpg_resident_sph_set_delaytime: no resident gas arrays");
    MPG_HIP(hipSetDevice(eng->device));
    const int64_t n = eng->res_n;
    if(!delaytime || n <= 0) {
        if(eng->d_delaytime == eng->s_delaytime.p)
            eng->d_delaytime = nullptr;
    }
    else {
        eng->s_delaytime.reserve((size_t)n + 1);
        MPG_HIP(hipMemcpyAsync(eng->s_delaytime.p, delaytime, (size_t)n * sizeof(double), hipMemcpyHostToDevice, eng->stream));
        MPG_HIP(hipStreamSynchronize(eng->stream));
        eng->d_delaytime = eng->s_delaytime.p;
    }
    API_END
}

// the resident time bins into host arrays (n bytes each; either may be NULL): build_active_particles (timestep.c:1333-1420) reads
// P[].TimeBinHydro / TimeBinGravity on the host at the top of every step
int mpg_resident_fetch_timebins(mpg_engine *eng, unsigned char *tb_hydro, unsigned char *tb_grav)
{
    API_BEGIN
    MPG_CHECK(eng && eng->sph_resident, "mpg_resident_fetch_timebins: no resident gas arrays");
    MPG_HIP(hipSetDevice(eng->device));
    const int64_t n = eng->res_n;
    const mpg_sph_arrays &d = eng->res_sph_dev;
    MPG_CHECK((!tb_hydro || d.tb_hydro) && (!tb_grav || d.tb_grav), "mpg_resident_fetch_timebins: the resident arrays have no such bins");
    if(tb_hydro)
        MPG_HIP(hipMemcpyAsync(tb_hydro, d.tb_hydro, (size_t)n, hipMemcpyDeviceToHost, eng->stream));
    if(tb_grav)
        MPG_HIP(hipMemcpyAsync(tb_grav, d.tb_grav, (size_t)n, hipMemcpyDeviceToHost, eng->stream));
    MPG_HIP(hipStreamSynchronize(eng->stream));
    API_END
}

int mpg_resident_drift_all_particles(mpg_engine *eng, const mpg_particle_view *P, double ddrift, const double random_shift[3])
{
    API_BEGIN
    MPG_CHECK(eng && P && random_shift, "null argument");
    resident_check(eng, P);
    MPG_CHECK(eng->res_has_vel, "resident drift: the resident table has no Vel column");
    const bool gas = eng->sph_resident;
    if(!gas) // (a gas run made them at mpg_resident_sph_begin)
        resident_flags(eng, P->n);
    MPG_CALL(mpg_dev_drift_all_particles(eng, P->n, eng->s_pos.p, eng->r_vel.p, eng->s_type.p, eng->r_flags.p, gas ? eng->res_sph_dev.hsml : nullptr,
                                         gas ? eng->res_sph_dev.dthsml : nullptr, ddrift, eng->box, random_shift));
    API_END
}

int mpg_resident_apply_pm_half_kick(mpg_engine *eng, const mpg_particle_view *P, double Fgravkick)
{
    API_BEGIN
    MPG_CHECK(eng && P, "null argument");
    resident_check(eng, P);
    MPG_CHECK(eng->res_has_vel, "resident kick: the resident table has no Vel column");
    if(!eng->sph_resident)
        resident_flags(eng, P->n);
    MPG_CALL(mpg_dev_apply_pm_half_kick(eng, P->n, eng->r_vel.p, eng->r_gravpm.p, eng->r_flags.p, Fgravkick));
    API_END
}

int mpg_resident_apply_half_kick(mpg_engine *eng, const mpg_particle_view *P, const int *ActiveParticle, int64_t NumActiveParticle,
                                 const mpg_kick_factors *K)
{
    API_BEGIN
    MPG_CHECK(eng && P && K, "null argument");
    resident_sph_check(eng, P);
    const mpg_sph_arrays &d = eng->res_sph_dev;
    const int *d_act = upload_active(eng->s_active, ActiveParticle, NumActiveParticle, eng->stream);
    MPG_CALL(mpg_dev_apply_half_kick(eng, P->n, d_act, NumActiveParticle, eng->r_vel.p, eng->r_accel.p, eng->s_type.p, eng->r_flags.p, d.tb_grav, d.tb_hydro,
                                     d.hydroacc_out, (double *)d.entropy, d.dtentropy_out, K));
    API_END
}

int mpg_resident_find_hydro_timesteps(mpg_engine *eng, const mpg_particle_view *P, const int *ActiveParticle, int64_t NumActiveParticle,
                                      mpg_drift_kick_times *times, const mpg_timeline *timeline, const mpg_timestep_params *par, double CourantFac,
                                      double atime, double hubble, int isFirstTimeStep, mpg_hydrostep_result *out)
{
    API_BEGIN
    MPG_CHECK(eng && P && times && out, "null argument");
    resident_sph_check(eng, P);
    const mpg_sph_arrays &d = eng->res_sph_dev;
    MPG_CHECK(d.tb_hydro, "resident find_hydro_timesteps: the gas arrays have no TimeBinHydro");
    const int *d_act = upload_active(eng->s_active, ActiveParticle, NumActiveParticle, eng->stream);
    const mpg_hydrostep_arrays H = resident_hydrostep_arrays(eng);
    MPG_CALL(mpg_dev_find_hydro_timesteps(eng, &H, d_act, NumActiveParticle, times, timeline, par, CourantFac, atime, hubble, out));
    MPG_CALL(mpg_dev_hydro_timesteps_finish(eng, out->mTimeBin, isFirstTimeStep, P->n, eng->s_type.p, (unsigned char *)d.tb_hydro, times));
    API_END
}

int mpg_resident_find_timesteps(mpg_engine *eng, const mpg_particle_view *P, const int *ActiveParticle, int64_t NumActiveParticle,
                                mpg_drift_kick_times *times, const mpg_timeline *timeline, const mpg_timestep_params *par, double CourantFac,
                                double atime, double hubble, int64_t dti_max_pm, mpg_timestep_result *out)
{
    API_BEGIN
    MPG_CHECK(eng && P && times && out, "null argument");
    resident_sph_check(eng, P);
    const mpg_sph_arrays &d = eng->res_sph_dev;
    MPG_CHECK(d.tb_hydro && d.tb_grav, "resident find_timesteps: the gas arrays have no time bins");
    const int *d_act = upload_active(eng->s_active, ActiveParticle, NumActiveParticle, eng->stream);
    const mpg_hydrostep_arrays H = resident_hydrostep_arrays(eng);
    MPG_CALL(mpg_dev_find_timesteps(eng, &H, eng->r_accel.p, eng->r_gravpm.p, (unsigned char *)d.tb_grav, d_act, NumActiveParticle, times, timeline, par,
                                    CourantFac, atime, hubble, dti_max_pm, out));
    MPG_CALL(mpg_find_timesteps_finish(out->mTimeBin, out->maxTimeBin, out->isPM, times));
    API_END
}

int mpg_resident_apply_hydro_half_kick(mpg_engine *eng, const mpg_particle_view *P, const int *ActiveParticle, int64_t NumActiveParticle,
                                       const mpg_kick_factors *K)
{
    API_BEGIN
    MPG_CHECK(eng && P && K, "null argument");
    resident_sph_check(eng, P);
    const mpg_sph_arrays &d = eng->res_sph_dev;
    const int *d_act = upload_active(eng->s_active, ActiveParticle, NumActiveParticle, eng->stream);
    MPG_CALL(mpg_dev_apply_hydro_half_kick(eng, P->n, d_act, NumActiveParticle, eng->r_vel.p, eng->s_type.p, eng->r_flags.p, d.tb_hydro, d.hydroacc_out,
                                           (double *)d.entropy, d.dtentropy_out, K));
    API_END
}

/* The branch of run.c WITH SplitGravityTimestepsOn (run.c:497-499, 536-540, 766-775) on a resident run: the level loop of
 * mpg_dev_hierarchical_* on the resident table - Vel, GravPM, FullTreeGravAccel and Potential are its columns, TimeBinGravity the resident gas
 * run's tb_grav (mpg_resident_sph_begin, as for mpg_resident_find_timesteps), the flags those of the resident table.  The trees of the levels
 * are built from the resident positions.  StoredGravAccel: the device copy r_stored stands for the caller's host array (include/mpgadget_hip.h).
 * Carried: one rank, dark matter and gas.  Not carried: several ranks (the level loop's trees are local), black holes, and star particles
 * created during the step (the reference's extra StoredGravAccel rows, run.c:537-538: only the first n rows exist here). */
namespace {
void resident_hier_arrays(mpg_engine *eng, const mpg_particle_view *P, double (*StoredGravAccel)[3], mpg_hiergrav_arrays *A)
{
    resident_sph_check(eng, P);
    MPG_CHECK(eng->res_has_vel, "resident hierarchical gravity: the resident table has no Vel column");
    const mpg_sph_arrays &d = eng->res_sph_dev;
    MPG_CHECK(d.tb_grav, "resident hierarchical gravity: the gas arrays have no TimeBinGravity");
    stage_particles(eng, P, eng->box); // (resident: checks that the device binding is still the table's)
    const int64_t n = P->n;
    A->d_vel = eng->r_vel.p;
    A->d_gravpm = eng->r_gravpm.p;
    A->d_fulltree_accel = eng->r_accel.p;
    A->d_potential = eng->r_pot.p;
    A->d_tb_grav = (unsigned char *)d.tb_grav;
    A->d_flags = eng->r_flags.p;
    A->d_stored_accel = nullptr;
    if(!StoredGravAccel)
        return; // FullTreeGravAccel plays the part of the stored array
    if(StoredGravAccel != eng->r_stored_host) {
        MPG_CHECK(!eng->r_stored_host, "resident hierarchical gravity: another StoredGravAccel array is still held (hierarchical_gravity_and_timesteps "
                                       "or mpg_resident_end releases it)");
        eng->r_stored.reserve(3 * (size_t)n + 3);
        if(n > 0) { // (a host array the engine does not hold yet: its first n rows)
            MPG_HIP(hipMemcpyAsync(eng->r_stored.p, StoredGravAccel, 3 * (size_t)n * sizeof(double), hipMemcpyHostToDevice, eng->stream));
            MPG_HIP(hipStreamSynchronize(eng->stream));
        }
        eng->r_stored_host = StoredGravAccel;
    }
    A->d_stored_accel = eng->r_stored.p;
}
} // namespace

int mpg_resident_hierarchical_gravity_accelerations(mpg_engine *eng, const mpg_particle_view *P, const int *ActiveParticle, int64_t NumActiveParticle,
                                                    int64_t NumActiveGravity, mpg_drift_kick_times *times, double rho0, int HybridNuGrav,
                                                    mpg_gravkick_fn gravkick, void *gravkick_ctx, double (*StoredGravAccel)[3])
{
    API_BEGIN
    MPG_CHECK(eng && P && times && gravkick && NumActiveParticle >= 0 && NumActiveGravity >= 0, "null argument");
    MPG_CHECK(!ActiveParticle || NumActiveParticle <= P->n, "resident hierarchical gravity: more active particles than particles");
    mpg_hiergrav_arrays A;
    resident_hier_arrays(eng, P, StoredGravAccel, &A);
    const int *d_act = upload_active(eng->s_active, ActiveParticle, NumActiveParticle, eng->stream);
    if(!ActiveParticle) // every particle is active (build_active_particles on a PM step: NumActiveParticle = NumPart)
        NumActiveParticle = P->n;
    MPG_CALL(mpg_dev_hierarchical_gravity_accelerations(eng, &A, d_act, NumActiveParticle, NumActiveGravity, times, rho0, HybridNuGrav, gravkick, gravkick_ctx));
    API_END
}

int mpg_resident_hierarchical_gravity_and_timesteps(mpg_engine *eng, const mpg_particle_view *P, const int *ActiveParticle, int64_t NumActiveParticle,
                                                    int64_t NumActiveGravity, mpg_drift_kick_times *times, const mpg_timeline *timeline,
                                                    const mpg_timestep_params *par, double atime, double hubble, int64_t dti_max_pm, double rho0,
                                                    int HybridNuGrav, mpg_gravkick_fn gravkick, void *gravkick_ctx, double (*StoredGravAccel)[3],
                                                    int64_t *badstepsizecount)
{
    API_BEGIN
    MPG_CHECK(eng && P && times && timeline && par && gravkick && badstepsizecount && NumActiveParticle >= 0 && NumActiveGravity >= 0, "null argument");
    MPG_CHECK(!ActiveParticle || NumActiveParticle <= P->n, "resident hierarchical gravity: more active particles than particles");
    mpg_hiergrav_arrays A;
    resident_hier_arrays(eng, P, StoredGravAccel, &A);
    const int *d_act = upload_active(eng->s_active, ActiveParticle, NumActiveParticle, eng->stream);
    if(!ActiveParticle)
        NumActiveParticle = P->n;
    MPG_CALL(mpg_dev_hierarchical_gravity_and_timesteps(eng, &A, d_act, NumActiveParticle, NumActiveGravity, times, timeline, par, atime, hubble, dti_max_pm,
                                                        rho0, HybridNuGrav, gravkick, gravkick_ctx, badstepsizecount));
    // the step has consumed the stored accelerations: the reference frees the array here (timestep.c:417-418)
    if(StoredGravAccel)
        eng->r_stored_host = nullptr;
    API_END
}

int mpg_resident_sph_find_vel_disp(mpg_engine *eng, const mpg_particle_view *pv, const mpg_sph_times *T, const mpg_veldisp_params *par,
                                   const int *ActiveParticle, int64_t NumActiveParticle, double *vdisp)
{
    API_BEGIN
    MPG_CHECK(eng && pv && T && par && vdisp, "null argument");
    resident_sph_check(eng, pv);
    const size_t n = (size_t)pv->n;
    const mpg_sph_arrays &r = eng->res_sph_dev;
    mpg_veldisp_arrays d;
    d.vel = r.vel;
    d.gacc = r.gacc;
    d.gpm = r.gpm;
    d.tb_grav = r.tb_grav;
    d.hsml = r.hsml;
    d.dthsml = r.dthsml;
    d.density = r.density;
    constexpr int VDISP = field_index(VDISP_FIELDS, offsetof(mpg_veldisp_arrays, vdisp));
    d.vdisp = (double *)stage_field(VDISP_FIELDS[VDISP], eng->vd_stage[VDISP], vdisp, pv->n, eng->stream);
    const int *d_act = upload_active(eng->s_active, ActiveParticle, NumActiveParticle, eng->stream);
    MPG_CALL(mpg_dev_find_vel_disp(eng, &d, T, par, d_act, NumActiveParticle));
    MPG_HIP(hipMemcpyAsync(vdisp, d.vdisp, n * sizeof(double), hipMemcpyDeviceToHost, eng->stream));
    MPG_HIP(hipStreamSynchronize(eng->stream));
    API_END
}

// cooling_direct on a resident gas run: Density, Entropy and TimeBinHydro are the resident columns, so the new entropies are where the
// next density / hydro loop and the integrator read them; ne travels (as vdisp does above), with the two optional inputs
int mpg_resident_sph_cooling(mpg_engine *eng, const mpg_particle_view *pv, const mpg_sph_times *T, const mpg_cooling_step *step,
                             const int *ActiveParticle, int64_t NumActiveParticle, double *ne, const double *metallicity,
                             const uint8_t *heiii_ionized)
{
    API_BEGIN
    MPG_CHECK(eng && pv && T && step && ne, "null argument");
    resident_sph_check(eng, pv);
    const size_t n = (size_t)pv->n;
    const mpg_sph_arrays &r = eng->res_sph_dev;
    MPG_CHECK(r.density && r.entropy, "resident cooling: the gas arrays have no Density / Entropy");
    mpg_cooling_arrays d{};
    d.density = r.density;
    d.entropy = (double *)r.entropy;
    d.tb_hydro = r.tb_hydro;
    constexpr int NE = field_index(COOL_FIELDS, offsetof(mpg_cooling_arrays, ne)), SFR = field_index(COOL_FIELDS, offsetof(mpg_cooling_arrays, sfr)),
                  METALLICITY = field_index(COOL_FIELDS, offsetof(mpg_cooling_arrays, metallicity)),
                  HEIII = field_index(COOL_FIELDS, offsetof(mpg_cooling_arrays, heiii_ionized));
    d.ne = (double *)stage_field(COOL_FIELDS[NE], eng->cl_stage[NE], ne, pv->n, eng->stream);
    // Sfr is no resident column: a scratch column, reserved and not uploaded, takes the zeros
    d.sfr = (double *)stage_field(COOL_FIELDS[SFR], eng->cl_stage[SFR], nullptr, pv->n, eng->stream);
    if(metallicity)
        d.metallicity = (const double *)stage_field(COOL_FIELDS[METALLICITY], eng->cl_stage[METALLICITY], metallicity, pv->n, eng->stream);
    if(heiii_ionized)
        d.heiii_ionized = (const uint8_t *)stage_field(COOL_FIELDS[HEIII], eng->cl_stage[HEIII], heiii_ionized, pv->n, eng->stream);
    const int *d_act = upload_active(eng->s_active, ActiveParticle, NumActiveParticle, eng->stream);
    const int rc = mpg_dev_cooling(eng, &d, T, step, d_act, NumActiveParticle);
    const std::string err = rc ? mpg_last_error() : "";
    MPG_HIP(hipMemcpyAsync(ne, d.ne, n * sizeof(double), hipMemcpyDeviceToHost, eng->stream));
    MPG_HIP(hipStreamSynchronize(eng->stream));
    MPG_CHECK(rc == 0, err);
    API_END
}

// cooling_and_starformation without the spawning on a resident gas run: Density, Entropy, TimeBinHydro, Hsml, DivVel and CurlVel are the
// resident columns, so
// the new entropies are where the next density / hydro loop and the integrator read them; every other column travels (host_table.h).
// The caller ends the stretch only when the new-star list is not empty.
int mpg_resident_sph_cooling_and_starformation(mpg_engine *eng, const mpg_particle_view *pv, const mpg_sfr_columns *A, const mpg_sph_times *T,
                                               const mpg_cooling_step *step, const int *ActiveParticle, int64_t NumActiveParticle)
{
    API_BEGIN
    MPG_CHECK(eng && pv && A && T && step, "null argument");
    resident_sph_check(eng, pv);
    const mpg_sph_arrays &r = eng->res_sph_dev;
    MPG_CHECK(r.density && r.entropy, "resident cooling_and_starformation: the gas arrays have no Density / Entropy");
    MPG_CHECK(!(eng->sfr.have_params && eng->sfr.par.WindOn && eng->have_windpar && (eng->windpar.WindModel & WIND_SUBGRID)),
              "resident cooling_and_starformation: WindOn with WIND_SUBGRID is not carried on a resident gas run (the kicks change the resident Vel)");
    mpg_sfr_columns d{};
    stage_fields(SFR_FIELDS, *A, d, eng->sf_stage, pv->n, ARR_RES_ALIAS, "cooling_and_starformation", eng->stream);
    d.density = r.density;
    d.entropy = (double *)r.entropy;
    d.tb_hydro = r.tb_hydro;
    d.hsml = r.hsml; // (of the density loop of this stretch: the criteria read them)
    d.divvel = r.divvel;
    d.curlvel = r.curlvel;
    const int *d_act = upload_active(eng->s_active, ActiveParticle, NumActiveParticle, eng->stream);
    const int rc = mpg_dev_cooling_and_starformation(eng, &d, T, step, d_act, NumActiveParticle);
    const std::string err = rc ? mpg_last_error() : "";
    unstage_fields(SFR_FIELDS, *A, d, pv->n, ARR_RES_ALIAS, eng->stream);
    MPG_HIP(hipStreamSynchronize(eng->stream));
    MPG_CHECK(rc == 0, err);
    API_END
}

// metal_return on a resident gas run, on the run's current tree (the one hydro_force has just used): Mass, Hsml and Density are resident
// columns; the new masses also go into the records, which mpg_resident_end does not fetch.  The STARS' Hsml belongs to this call alone (no
// SPH loop reads or writes it): when A->hsml is given, its rows of type 4 replace the resident column's before the call - the caller's
// repair of a zero Hsml arrives that way - and the whole column comes back into it afterwards.
int mpg_resident_sph_metal_return(mpg_engine *eng, const mpg_particle_view *pv, const mpg_metal_arrays *A, const int *ActiveParticle,
                                  int64_t NumActiveParticle)
{
    API_BEGIN
    MPG_CHECK(eng && pv && A, "null argument");
    resident_sph_check(eng, pv);
    const int64_t n = pv->n;
    const mpg_sph_arrays &r = eng->res_sph_dev;
    mpg_metal_arrays d{};
    stage_fields(METAL_FIELDS, *A, d, eng->mt_stage, n, ARR_TABLE | ARR_RES_ALIAS, "metal_return", eng->stream);
    d.mass = eng->s_mass.p;
    d.hsml = r.hsml;
    d.density = r.density;
    if(A->hsml && n > 0) {
        constexpr int HSML = field_index(METAL_FIELDS, offsetof(mpg_metal_arrays, hsml));
        const double *up = (const double *)stage_field(METAL_FIELDS[HSML], eng->mt_stage[HSML], A->hsml, n, eng->stream);
        MetalsEngine::take_star_hsml(d.hsml, up, eng->s_type.p, n, eng->stream);
    }
    const int *d_act = upload_active(eng->s_active, ActiveParticle, NumActiveParticle, eng->stream);
    MPG_CALL(mpg_dev_metal_return(eng, &d, d_act, NumActiveParticle));
    unstage_fields(METAL_FIELDS, *A, d, n, ARR_TABLE | ARR_RES_ALIAS, eng->stream);
    if(A->hsml && n > 0)
        MPG_HIP(hipMemcpyAsync(A->hsml, d.hsml, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, eng->stream));
    if(eng->metals.ntargets > 0) {
        eng->mt_mass.reserve((size_t)n + 1);
        mass_to_records(*pv, eng->s_mass.p, eng->mt_mass.p, eng->stream);
    }
    MPG_HIP(hipStreamSynchronize(eng->stream));
    API_END
}

// blackhole_dynfric + blackhole_dfaccel on a resident gas run: Pos, Mass, Vel, the accelerations, the bins, Hsml and Potential are the
// resident columns; the per-black-hole members travel, and only when the list holds a black hole.  Nothing resident is written.  The call
// leaves the tree of its own mask: mpg_resident_sph_blackhole, next in blackhole(), builds the tree of gas and black holes again.
int mpg_resident_sph_blackhole_dynfric(mpg_engine *eng, const mpg_particle_view *pv, const mpg_bh_dynfric_arrays *A, const mpg_sph_times *T,
                                       const int *ActiveParticle, int64_t NumActiveParticle)
{
    API_BEGIN
    MPG_CHECK(eng && pv && A && T, "null argument");
    resident_sph_check(eng, pv);
    const int64_t n = pv->n;
    const mpg_sph_arrays &r = eng->res_sph_dev;
    MPG_CHECK(r.vel && r.gacc && r.gpm && r.hydroacc_out && r.tb_hydro && r.tb_grav && r.hsml,
              "resident blackhole_dynfric: the gas arrays lack one of vel, gacc, gpm, hydroacc_out, tb_hydro, tb_grav, hsml");
    const int *d_act = upload_active(eng->s_active, ActiveParticle, NumActiveParticle, eng->stream);
    if(dynfric_listed(eng, d_act, NumActiveParticle) == 0) {
        mpg_err_slot().clear();
        return 0;
    }
    mpg_bh_dynfric_arrays d{};
    stage_fields(DF_FIELDS, *A, d, eng->df_stage, n, ARR_RES_ALIAS, "blackhole_dynfric", eng->stream);
    d.vel = r.vel;
    d.gacc = r.gacc;
    d.gpm = r.gpm;
    d.hydroacc = r.hydroacc_out;
    d.tb_hydro = r.tb_hydro;
    d.tb_grav = r.tb_grav;
    d.hsml = r.hsml;
    d.potential = eng->r_pot.p;
    dynfric_call(eng, &d, T, d_act, NumActiveParticle);
    unstage_fields(DF_FIELDS, *A, d, n, ARR_RES_ALIAS, eng->stream);
    MPG_HIP(hipStreamSynchronize(eng->stream));
    API_END
}

// blackhole() on a resident gas run: the table's and the gas arrays' columns are the resident ones and are updated in place; the type
// column and the integrator's flags take the rows swallowed; Mass and flags also go into the records, which the end of the resident
// stretch does not fetch.  The per-black-hole members and ID / DelayTime travel.
int mpg_resident_sph_blackhole(mpg_engine *eng, const mpg_particle_view *pv, const mpg_blackhole_arrays *A, const mpg_sph_times *T,
                               const int *ActiveParticle, int64_t NumActiveParticle)
{
    API_BEGIN
    MPG_CHECK(eng && pv && A && T, "null argument");
    resident_sph_check(eng, pv);
    const int64_t n = pv->n;
    const mpg_sph_arrays &r = eng->res_sph_dev;
    MPG_CHECK(r.vel && r.gacc && r.gpm && r.hydroacc_out && r.tb_hydro && r.tb_grav && r.hsml && r.density && r.entropy,
              "resident blackhole: the gas arrays lack one of vel, gacc, gpm, hydroacc_out, tb_hydro, tb_grav, hsml, density, entropy");
    const int *d_act = upload_active(eng->s_active, ActiveParticle, NumActiveParticle, eng->stream);
    // the queue pass first: without a target nothing travels, nothing is read and nothing is written
    if(blackhole_targets(eng, d_act, NumActiveParticle) == 0) {
        mpg_err_slot().clear();
        return 0;
    }
    mpg_blackhole_arrays d{};
    stage_fields(BH_FIELDS, *A, d, eng->bh_stage, n, ARR_TABLE | ARR_RES_ALIAS, "blackhole", eng->stream);
    d.mass = eng->s_mass.p;
    d.vel = (double *)r.vel;
    d.gacc = r.gacc;
    d.gpm = r.gpm;
    d.hydroacc = r.hydroacc_out;
    d.tb_hydro = r.tb_hydro;
    d.tb_grav = r.tb_grav;
    d.hsml = r.hsml;
    d.density = r.density;
    d.entropy = (double *)r.entropy;
    blackhole_call(eng, &d, T, d_act, NumActiveParticle, 1);
    unstage_fields(BH_FIELDS, *A, d, n, ARR_TABLE | ARR_RES_ALIAS, eng->stream);
    if(eng->bh.ntargets > 0) {
        BlackholeEngine::retype(eng->s_type.p, d.flags, n, eng->stream);
        resident_flags(eng, n);
        eng->bh_mass.reserve((size_t)n + 1);
        mass_to_records(*pv, eng->s_mass.p, eng->bh_mass.p, eng->stream);
        MPG_HIP(hipStreamSynchronize(eng->stream));
        flags_to_records(*pv, A->flags);
    }
    MPG_HIP(hipStreamSynchronize(eng->stream));
    API_END
}

// do_heiii_reionization on a resident gas run: Density and Entropy are the resident columns, so the heat is where the next cooling call
// and the integrator read it; the flag travels in and out, the groups stay on the host.  The run's tree is neither read nor changed.
int mpg_resident_sph_heiii_reionization(mpg_engine *eng, const mpg_particle_view *pv, const mpg_heiii_step *step, uint8_t *heiii_ionized,
                                        const double *group_mass, const double *group_cm, const uint64_t *group_minid, int64_t ngroups,
                                        mpg_heiii_result *result)
{
    API_BEGIN
    MPG_CHECK(eng && pv && step, "null argument");
    MPG_CHECK(ngroups >= 0, "heiii_reionization: negative group number");
    resident_sph_check(eng, pv);
    const size_t n = (size_t)pv->n;
    const mpg_sph_arrays &r = eng->res_sph_dev;
    MPG_CHECK(r.density && r.entropy, "resident heiii_reionization: the gas arrays have no Density / Entropy");
    MPG_CHECK(heiii_ionized || n == 0, "heiii_reionization: the array heiii_ionized is required");
    eng->he_flag.reserve(n + 1);
    if(n > 0)
        MPG_HIP(hipMemcpyAsync(eng->he_flag.p, heiii_ionized, n, hipMemcpyHostToDevice, eng->stream));
    heiii_call(eng, step, r.density, (double *)r.entropy, eng->he_flag.p, heiii_host_groups(group_mass, group_cm, group_minid, ngroups), result);
    if(n > 0)
        MPG_HIP(hipMemcpyAsync(heiii_ionized, eng->he_flag.p, n, hipMemcpyDeviceToHost, eng->stream));
    MPG_HIP(hipStreamSynchronize(eng->stream));
    API_END
}
