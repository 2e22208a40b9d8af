// dist_host.hip -- the host-pointer forms of the multi-rank layer (dist.hip has the overview): every mpg_dist_* call that takes an
// mpg_particle_view.  They stage the rank's table on the device, call the device forms and write the results back; no kernel is theirs.
#include "dist_internal.h"
#include <algorithm>

/* ---- the drop-in (host pointer) forms: the rank's P[] in host memory, results written back into it ------------------------ */
namespace {
// Pos / Mass of the rank's particle table onto the device (d->o_pos, d->o_mass)
void stage_own(mpg_dist *d, const mpg_particle_view *P)
{
    MPG_CHECK(P && (P->n == 0 || P->base), "null particle view");
    MPG_CHECK(P->off_pos >= 0 && P->off_mass >= 0, "particle view needs Pos and Mass");
    const int64_t n = P->n;
    hipStream_t st = d->eng->stream;
    d->hbuf.resize(3 * (size_t)n + 3);
    d->hbuf_f.resize((size_t)n + 1);
    const HostTable T(*P);
    double *hd = d->hbuf.data();
    float *hf = d->hbuf_f.data();
    // IsGarbage (bit 0) and Swallowed (bit 1) of the flag byte (partmanager.h:24-44): such particles stay where they are in P[] and are
    // skipped in place by every loop of this path (treewalk.c:234, forcetree.c:806, gravpm.c:176-179) - after star formation and black
    // hole mergers every sub-step sees some until the next domain_decompose_full collects them
    d->hbuf_b.resize((size_t)n + 1);
    uint8_t *hb = d->hbuf_b.data();
    std::vector<int> bad(64, 0);
    parallel_for(n, [=, &bad](int64_t lo, int64_t hi) {
        int any = 0;
        for(int64_t i = lo; i < hi; i++) {
            const double *pp = T.pos(i);
            hd[3 * i] = pp[0];
            hd[3 * i + 1] = pp[1];
            hd[3 * i + 2] = pp[2];
            hf[i] = T.mass(i);
            hb[i] = skipped_in_place(T.flags(i)) ? 1 : 0;
            any |= hb[i];
        }
        if(any)
            bad[0] = 1;
    });
    if(bad[0]) {
        d->o_skip.reserve((size_t)n + 1);
        MPG_HIP(hipMemcpyAsync(d->o_skip.p, hb, (size_t)n, hipMemcpyHostToDevice, st));
        MPG_CALL(mpg_dist_dev_set_garbage(d, n, d->o_skip.p));
    }
    else
        MPG_CALL(mpg_dist_dev_set_garbage(d, n, nullptr));
    d->o_pos.reserve(3 * (size_t)n + 3);
    d->o_mass.reserve((size_t)n + 1);
    d->o_gravpm.reserve(3 * (size_t)n + 3);
    d->o_pot.reserve((size_t)n + 1);
    d->o_acc.reserve(3 * (size_t)n + 3);
    d->o_prev.reserve(3 * (size_t)n + 3);
    if(n > 0) {
        MPG_HIP(hipMemcpyAsync(d->o_pos.p, hd, 3 * (size_t)n * sizeof(double), hipMemcpyHostToDevice, st));
        MPG_HIP(hipMemcpyAsync(d->o_mass.p, hf, (size_t)n * sizeof(float), hipMemcpyHostToDevice, st));
    }
    sync(d);
    d->o_n = n;
}

// one 3-vector (or scalar) column of P[] <-> a device array
void column_up(mpg_dist *d, const mpg_particle_view *P, int64_t off, int w, double *dev)
{
    const int64_t n = P->n;
    d->hbuf.resize((size_t)w * n + 3);
    const HostTable T(*P);
    double *hd = d->hbuf.data();
    parallel_for(n, [=](int64_t lo, int64_t hi) {
        for(int64_t i = lo; i < hi; i++)
            for(int k = 0; k < w; k++)
                hd[w * i + k] = T.vec(i, off)[k];
    });
    if(n > 0)
        MPG_HIP(hipMemcpyAsync(dev, hd, (size_t)w * n * sizeof(double), hipMemcpyHostToDevice, d->eng->stream));
    sync(d);
}

template <class F> void column_down(mpg_dist *d, int64_t n, int w, const double *dev, F put)
{
    d->hbuf.resize((size_t)w * n + 3);
    double *hd = d->hbuf.data();
    if(n > 0)
        MPG_HIP(hipMemcpyAsync(hd, dev, (size_t)w * n * sizeof(double), hipMemcpyDeviceToHost, d->eng->stream));
    sync(d);
    parallel_for(n, [=](int64_t lo, int64_t hi) {
        for(int64_t i = lo; i < hi; i++)
            put(i, hd + (size_t)w * i);
    });
}

/* ---- the SPH loops as drop-in calls: the rank's table and the SPH fields in HOST arrays (what shim/sph-hip.c gathers from the
 * slots), after mpg_dist_force_tree_full on the same table ------------------------------------------------------------------ */
// device copy of the host arrays (SPH_FIELDS, host_table.h): inputs uploaded, outputs allocated; returns the device-side struct
mpg_sph_arrays stage_sph(mpg_dist *d, const mpg_sph_arrays *A, int64_t n, bool upload, bool upload_density_out, bool upload_hydro_out)
{
    hipStream_t st = d->eng->stream;
    mpg_sph_arrays D;
    for(const SphField &F : SPH_FIELDS) {
        void *h = field_get(*A, F.off), *dv = nullptr;
        bool up = upload && (F.role & SPH_IN);
        if(h && F.width == 0) {
            d->o_u8[1 + F.slot].reserve((size_t)n + 1);
            dv = d->o_u8[1 + F.slot].p;
        }
        else if(h) {
            d->o_sph[F.slot].reserve((size_t)F.width * n + 3);
            dv = d->o_sph[F.slot].p;
            up = up || (upload_density_out && (F.role & SPH_OUT_DENSITY)) || (upload_hydro_out && (F.role & SPH_OUT_HYDRO));
        }
        if(dv && up && n > 0)
            MPG_HIP(hipMemcpyAsync(dv, h, sph_field_bytes(F, n), hipMemcpyHostToDevice, st));
        field_set(D, F.off, dv);
    }
    sync(d);
    return D;
}

void download_sph(mpg_dist *d, const mpg_sph_arrays *A, int64_t n, bool hydro)
{
    hipStream_t st = d->eng->stream;
    for(const SphField &F : SPH_FIELDS) {
        void *h = field_get(*A, F.off);
        if(h && n > 0 && (F.role & (hydro ? SPH_OUT_HYDRO : SPH_OUT_DENSITY)))
            MPG_HIP(hipMemcpyAsync(h, d->o_sph[F.slot].p, sph_field_bytes(F, n), hipMemcpyDeviceToHost, st));
    }
    sync(d);
}

// P[].Type (garbage has been refused by mpg_dist_force_tree_full) onto the device
const uint8_t *stage_types(mpg_dist *d, const mpg_particle_view *P)
{
    const int64_t n = P->n;
    std::vector<uint8_t> ty((size_t)n + 1);
    const HostTable T(*P);
    uint8_t *t = ty.data();
    parallel_for(n, [=](int64_t lo, int64_t hi) {
        for(int64_t i = lo; i < hi; i++)
            t[i] = no_sph_particle(T.flags(i)) ? (uint8_t)7 : T.type(i);
    });
    d->o_u8[0].reserve((size_t)n + 1);
    if(n > 0)
        MPG_HIP(hipMemcpy(d->o_u8[0].p, ty.data(), (size_t)n, hipMemcpyHostToDevice));
    return d->o_u8[0].p;
}

} // namespace

extern "C" {

int mpg_dist_gravpm_force(mpg_dist *d, const mpg_particle_view *P)
{
    API_BEGIN
    MPG_CHECK(d && P, "null argument");
    MPG_CHECK(P->off_gravpm >= 0, "particle view needs GravPM");
    MPG_HIP(hipSetDevice(d->eng->device));
    stage_own(d, P);
    const int64_t n = P->n;
    if(d->eng->pm.hybrid_tracer) { // the types for the deposit mask (hybrid_nu_gravpm_is_active, gravpm.c:469-474)
        MPG_CHECK(P->off_type >= 0, "gravpm_force: the hybrid-neutrino deposit mask needs the particle type in the view");
        std::vector<uint8_t> ht((size_t)n + 1); // (not hbuf_b: it keeps the garbage flags of stage_own for the walk)
        uint8_t *hb = ht.data();
        const HostTable T(*P);
        parallel_for(n, [=](int64_t lo, int64_t hi) {
            for(int64_t i = lo; i < hi; i++)
                hb[i] = T.type(i);
        });
        d->o_u8[0].reserve((size_t)n + 1);
        if(n > 0)
            MPG_HIP(hipMemcpyAsync(d->o_u8[0].p, hb, (size_t)n, hipMemcpyHostToDevice, d->eng->stream));
        MPG_CALL(mpg_dist_dev_set_types(d, n, d->o_u8[0].p));
        sync(d);
    }
    if(n > 0)
        MPG_HIP(hipMemsetAsync(d->o_pot.p, 0, (size_t)n * sizeof(double), d->eng->stream));
    MPG_CALL(mpg_dist_dev_gravpm_force(d, n, d->o_pos.p, d->o_mass.p, d->o_gravpm.p, d->o_pot.p));
    const HostTable T(*P);
    column_down(d, n, 3, d->o_gravpm.p, [=](int64_t i, const double *v) {
        double *g = T.vec_mut(i, T.V.off_gravpm);
        g[0] = v[0];
        g[1] = v[1];
        g[2] = v[2];
    });
    if(P->off_potential >= 0)
        column_down(d, n, 1, d->o_pot.p, [=](int64_t i, const double *v) { T.scalar_mut(i, T.V.off_potential) += v[0]; });
    API_END
}

int mpg_dist_force_tree_full(mpg_dist *d, const mpg_particle_view *P)
{
    API_BEGIN
    MPG_CHECK(d && P, "null argument");
    MPG_HIP(hipSetDevice(d->eng->device));
    stage_own(d, P);
    MPG_CALL(mpg_dist_dev_force_tree_build(d, P->n, d->o_pos.p, d->o_mass.p));
    API_END
}

int mpg_dist_grav_short_tree(mpg_dist *d, const mpg_particle_view *P, double (*AccelStore)[3], double rho0)
{
    return mpg_dist_grav_short_tree_active(d, P, nullptr, 0, AccelStore, rho0);
}

int mpg_dist_grav_short_tree_active(mpg_dist *d, const mpg_particle_view *P, const int *ActiveParticle, int64_t NumActiveParticle,
                                    double (*AccelStore)[3], double rho0)
{
    API_BEGIN
    MPG_CHECK(d && P, "null argument");
    MPG_CHECK(P->off_accel >= 0 && P->off_gravpm >= 0, "particle view needs FullTreeGravAccel and GravPM");
    MPG_CHECK(d->o_n == P->n && d->n_own_tree == P->n, "mpg_dist_grav_short_tree: call mpg_dist_force_tree_full on this table first");
    MPG_CHECK(!ActiveParticle || (NumActiveParticle >= 0 && NumActiveParticle <= P->n), "bad NumActiveParticle");
    MPG_HIP(hipSetDevice(d->eng->device));
    const int64_t n = P->n;
    // OldAcc = |FullTreeGravAccel + GravPM| / G of the table as it stands (grav_get_abs_accel, gravshort.h:70-80)
    column_up(d, P, P->off_accel, 3, d->o_prev.p);
    column_up(d, P, P->off_gravpm, 3, d->o_gravpm.p);
    const int *d_act = upload_active(d->o_act, ActiveParticle, NumActiveParticle, d->eng->stream);
    const bool pot = P->off_potential >= 0;
    MPG_CALL(mpg_dist_dev_grav_short_tree_active(d, d_act, NumActiveParticle, nullptr, d->o_prev.p, d->o_gravpm.p, d->o_acc.p,
                                                 pot ? d->o_pot.p : nullptr, rho0));
    // results of the walked particles into the table: P[i].FullTreeGravAccel (full particle tree, gravshort.h:57-62), AccelStore[i],
    // P[i].Potential
    const HostTable T(*P);
    d->hbuf.resize(4 * (size_t)n + 4);
    double *ha = d->hbuf.data(), *hp = ha + 3 * (size_t)n;
    if(n > 0) {
        MPG_HIP(hipMemcpyAsync(ha, d->o_acc.p, 3 * (size_t)n * sizeof(double), hipMemcpyDeviceToHost, d->eng->stream));
        if(pot)
            MPG_HIP(hipMemcpyAsync(hp, d->o_pot.p, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, d->eng->stream));
    }
    sync(d);
    const int64_t m = ActiveParticle ? NumActiveParticle : n;
    const uint8_t *dead = (d->n_skip > 0 && (int64_t)d->hbuf_b.size() > n) ? d->hbuf_b.data() : nullptr; // (flags of this table: stage_own)
    parallel_for(m, [=](int64_t lo, int64_t hi) {
        for(int64_t k = lo; k < hi; k++) {
            const int64_t i = ActiveParticle ? ActiveParticle[k] : k;
            if(dead && dead[i])
                continue; // garbage / swallowed: not walked, nothing to write (treewalk.c:234)
            store_walk_result(T, i, ha + 3 * i, pot ? hp + i : nullptr, AccelStore, true);
        }
    });
    API_END
}

int mpg_dist_density(mpg_dist *d, const mpg_particle_view *P, const mpg_sph_arrays *A, const mpg_sph_times *T, const int *ActiveParticle,
                     int64_t NumActiveParticle, int update_hsml, int DoEgyDensity)
{
    API_BEGIN
    MPG_CHECK(d && P && A && T, "null argument");
    MPG_CHECK(d->o_n == P->n && d->n_own_tree == P->n, "mpg_dist_density: call mpg_dist_force_tree_full on this table first");
    MPG_HIP(hipSetDevice(d->eng->device));
    const uint8_t *ty = stage_types(d, P);
    // (a sub-step also uploads the density-loop results the inactive particles hold)
    const mpg_sph_arrays D = stage_sph(d, A, P->n, true, ActiveParticle != nullptr, false);
    const int *act = upload_active(d->o_act, ActiveParticle, NumActiveParticle, d->eng->stream);
    sync(d); // (on the device before the call returns to a caller that may reuse the list)
    MPG_CALL(mpg_dist_dev_density_active(d, P->n, ty, &D, T, act, NumActiveParticle, update_hsml, DoEgyDensity));
    download_sph(d, A, P->n, false);
    API_END
}

int mpg_dist_hydro_force(mpg_dist *d, const mpg_particle_view *P, const mpg_sph_arrays *A, const mpg_sph_times *T, const int *ActiveParticle,
                         int64_t NumActiveParticle)
{
    API_BEGIN
    MPG_CHECK(d && P && A && T, "null argument");
    MPG_CHECK(d->sph_n_own == P->n, "mpg_dist_hydro_force: call mpg_dist_density on this table first");
    MPG_HIP(hipSetDevice(d->eng->device));
    // (the inputs are the library's from the density call; a sub-step uploads the hydro results the inactive particles hold)
    const mpg_sph_arrays D = stage_sph(d, A, P->n, false, false, ActiveParticle != nullptr);
    const int *act = upload_active(d->o_act, ActiveParticle, NumActiveParticle, d->eng->stream);
    sync(d); // (on the device before the call returns to a caller that may reuse the list)
    MPG_CALL(mpg_dist_dev_hydro_force_active(d, P->n, &D, T, act, NumActiveParticle));
    download_sph(d, A, P->n, true);
    API_END
}

/* the drop-in form: the active particles are gathered from the rank's table, AccelStore[i] of the active particles is assigned
 * (grav_short_reduce / _postprocess with a tree that is not the full particle tree: P[] itself is left alone) */
extern "C" int mpg_dist_grav_short_tree_active_tree(mpg_dist *d, const mpg_particle_view *P, const int *ActiveParticle, int64_t NumActiveParticle,
                                                    double (*AccelStore)[3], double rho0)
{
    API_BEGIN
    MPG_CHECK(d && P && AccelStore, "null argument (the walk on an active-only tree returns its result in AccelStore)");
    MPG_CHECK(P->off_pos >= 0 && P->off_mass >= 0 && P->off_accel >= 0 && P->off_gravpm >= 0, "particle view needs Pos, Mass, FullTreeGravAccel, GravPM");
    const int64_t nlist = ActiveParticle ? NumActiveParticle : P->n;
    MPG_CHECK(nlist >= 0 && nlist <= P->n, "bad NumActiveParticle");
    MPG_HIP(hipSetDevice(d->eng->device));
    hipStream_t st = d->eng->stream;
    // the live members of the list (garbage and swallowed particles are skipped in place: treewalk.c:234, forcetree.c:806)
    const HostTable T(*P);
    std::vector<int64_t> live;
    live.reserve((size_t)nlist);
    for(int64_t k = 0; k < nlist; k++) {
        const int64_t i = ActiveParticle ? ActiveParticle[k] : k;
        MPG_CHECK(i >= 0 && i < P->n, "ActiveParticle index out of range");
        if(skipped_in_place(T.flags(i)))
            continue;
        live.push_back(i);
    }
    const int64_t n = (int64_t)live.size();
    const int64_t *lv = live.data();
    std::vector<double> hp(3 * (size_t)n + 3), ho((size_t)n + 1);
    std::vector<float> hm((size_t)n + 1);
    const double G = d->eng->pm.G;
    double *pp = hp.data(), *po = ho.data();
    float *pm = hm.data();
    parallel_for(n, [=](int64_t lo, int64_t hi) {
        for(int64_t k = lo; k < hi; k++) {
            const int64_t i = lv[k];
            const double *x = T.pos(i), *a = T.vec(i, T.V.off_accel), *g = T.vec(i, T.V.off_gravpm);
            double s2 = 0;
            for(int j = 0; j < 3; j++) {
                pp[3 * k + j] = x[j];
                s2 += (a[j] + g[j]) * (a[j] + g[j]);
            }
            pm[k] = T.mass(i);
            po[k] = sqrt(s2) / G; // grav_get_abs_accel, gravshort.h:70-80
        }
    });
    DevBuf<double> dp, dold, dacc;
    DevBuf<float> dm;
    dp.reserve(3 * (size_t)n + 3);
    dold.reserve((size_t)n + 1);
    dacc.reserve(3 * (size_t)n + 3);
    dm.reserve((size_t)n + 1);
    if(n > 0) {
        MPG_HIP(hipMemcpyAsync(dp.p, pp, 3 * (size_t)n * sizeof(double), hipMemcpyHostToDevice, st));
        MPG_HIP(hipMemcpyAsync(dold.p, po, (size_t)n * sizeof(double), hipMemcpyHostToDevice, st));
        MPG_HIP(hipMemcpyAsync(dm.p, pm, (size_t)n * sizeof(float), hipMemcpyHostToDevice, st));
    }
    sync(d);
    MPG_CALL(mpg_dist_dev_grav_short_tree_active_tree(d, n, dp.p, dm.p, dold.p, dacc.p, nullptr, rho0));
    if(n > 0)
        MPG_HIP(hipMemcpyAsync(pp, dacc.p, 3 * (size_t)n * sizeof(double), hipMemcpyDeviceToHost, st));
    sync(d);
    parallel_for(n, [=](int64_t lo, int64_t hi) {
        for(int64_t k = lo; k < hi; k++) {
            const int64_t i = lv[k];
            for(int j = 0; j < 3; j++)
                AccelStore[i][j] = pp[3 * k + j];
        }
    });
    API_END
}

} // extern "C"
