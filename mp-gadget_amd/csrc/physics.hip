// physics.hip -- C-ABI (include/mpgadget_hip.h) of the gas and subgrid physics on device arrays: SPH, DM velocity dispersion, radiative
// cooling and the UV-fluctuation table, metal return, black holes, winds, star formation, helium reionisation and dynamical friction.
// Host code only: the kernels are the modules' (sph.hip, veldisp.hip, cooling.hip, ...), the trees these calls build are engine.hip's,
// reached through the C ABI.
#include "engine_internal.h"
#include <algorithm>
#include <cstdio>

/* ------------------------------ what the entry points share ------------------------------ */

// a call on an active list of the bound particles, after its own refusals (they come first: this touches the engine): the last
// refusal, the device, the flags of the listed particles (null: every particle)
static const uint8_t *active_call(mpg_engine *eng, const char *who, const int *d_active, int64_t nactive)
{
    MPG_CHECK(eng->d_pos || eng->n == 0, std::string(who) + ": no particles bound");
    MPG_HIP(hipSetDevice(eng->device));
    return eng->sph.mark_active(d_active, nactive, eng->n, eng->stream);
}

// the searches for gas neighbours run on the current tree (treewalk.c:941-945)
static void require_gas_tree(const mpg_engine *eng, const char *who)
{
    MPG_CHECK(eng->tree_allocated && (eng->tree_mask & 1) != 0, std::string(who) + ": the current tree does not contain the gas (GASMASK)");
}

// an export of per-particle results: n is the particle number they were written for, and the call that wrote them has finished ...
static void export_begin(mpg_engine *eng, int64_t n, int64_t n_state, const char *message)
{
    MPG_CHECK(n == n_state, message);
    MPG_HIP(hipSetDevice(eng->device));
    MPG_HIP(hipStreamSynchronize(eng->stream));
}

// ... and one column of it, when the caller asked for it
template <class T> static void copy_down(T *host, const T *dev, int64_t count)
{
    if(host && count > 0)
        MPG_HIP(hipMemcpy(host, dev, (size_t)count * sizeof(T), hipMemcpyDeviceToHost));
}

// the counters and the device times (float or double) of a module's last call
static void copy_stats(int64_t *stats, const int64_t *last, int n) { std::copy_n(last, n, stats); }
template <class T> static void copy_times(double *ms, const T *last, int n) { std::copy_n(last, n, ms); }

// the targets of every iteration of a radius loop, zero beyond the last
static void copy_queue_lengths(int64_t *out, int64_t capacity, const std::vector<int64_t> &lengths)
{
    for(int64_t k = 0; out && k < capacity; k++)
        out[k] = k < (int64_t)lengths.size() ? lengths[k] : 0;
}

extern "C" {

/* ------------------------------ SPH ------------------------------ */

int mpg_set_densitypar(mpg_engine *eng, const mpg_density_params *dp)
{
    API_BEGIN
    MPG_CHECK(eng && dp, "null argument");
    MPG_CHECK(dp->DensityKernelType == 1 || dp->DensityKernelType == 2 || dp->DensityKernelType == 4, "Density Kernel type is unknown");
    eng->denspar = *dp;
    API_END
}

int mpg_set_hydropar(mpg_engine *eng, const mpg_hydro_params *hp)
{
    API_BEGIN
    MPG_CHECK(eng && hp, "null argument");
    eng->hydropar = *hp;
    API_END
}

double mpg_get_numngb(mpg_engine *eng) { return eng ? sph_desnumngb(eng->denspar) : 0.0; }

static SphView make_sph_view(mpg_engine *eng, const mpg_sph_arrays *A)
{
    MPG_CHECK(A, "null SPH arrays");
    MPG_CHECK(A->hsml && A->vel && A->entropy && A->density && A->dhsmlegyfac && A->divvel && A->curlvel,
              "SPH arrays: hsml, vel, entropy, density, dhsmlegyfac, divvel, curlvel are required");
    SphView v{};
    v.pos = eng->d_pos;
    v.mass = eng->d_mass;
    v.type = eng->d_type;
    v.hsml = A->hsml;
    v.dthsml = A->dthsml;
    v.vel = A->vel;
    v.gacc = A->gacc;
    v.gpm = A->gpm;
    v.hydroacc_in = A->hydroacc_in;
    v.tb_hydro = A->tb_hydro;
    v.tb_grav = A->tb_grav;
    v.entropy = A->entropy;
    v.dtentropy_in = A->dtentropy_in;
    v.density = A->density;
    v.egywtdensity = A->egywtdensity;
    v.dhsmlegyfac = A->dhsmlegyfac;
    v.divvel = A->divvel;
    v.curlvel = A->curlvel;
    v.gradrho = A->gradrho;
    v.hydroacc_out = A->hydroacc_out;
    v.dtentropy_out = A->dtentropy_out;
    v.maxsignalvel = A->maxsignalvel;
    return v;
}

int mpg_dev_set_init_hsml(mpg_engine *eng, const mpg_sph_arrays *A, double MeanGasSeparation)
{
    API_BEGIN
    MPG_CHECK(eng && eng->tree_allocated, "set_init_hsml: no tree");
    MPG_HIP(hipSetDevice(eng->device));
    const SphView v = make_sph_view(eng, A);
    eng->sph.set_init_hsml(eng->tree, v, eng->denspar, MeanGasSeparation, eng->stream);
    API_END
}

int mpg_dev_density(mpg_engine *eng, const mpg_sph_arrays *A, const mpg_sph_times *T, const int *d_active, int64_t nactive,
                    int update_hsml, int DoEgyDensity, int BlackHoleOn)
{
    API_BEGIN
    MPG_CHECK(eng && T, "null argument");
    MPG_CHECK(eng->tree_allocated, "density: no tree (force_tree_rebuild_mask first)");
    MPG_CHECK((eng->tree_mask & 1) != 0, "density: the tree does not contain gas (GASMASK)"); // treewalk.c:942-943
    MPG_CHECK(!DoEgyDensity || A->egywtdensity, "density: DoEgyDensity needs the egywtdensity array");
    MPG_HIP(hipSetDevice(eng->device));
    const SphView v = make_sph_view(eng, A);
    eng->sph.density(eng->tree, v, *T, eng->denspar, 2.8 * eng->GravitySoftening, d_active, nactive, eng->n, update_hsml, DoEgyDensity,
                     BlackHoleOn, (eng->tree_mask & 32) != 0, eng->stream);
    API_END
}

int mpg_dev_hydro_force(mpg_engine *eng, const mpg_sph_arrays *A, const mpg_sph_times *T, const int *d_active, int64_t nactive)
{
    API_BEGIN
    MPG_CHECK(eng && T, "null argument");
    MPG_CHECK(eng->tree_allocated, "hydro_force: no tree");
    MPG_CHECK(A->hydroacc_out && A->dtentropy_out && A->maxsignalvel, "hydro_force: output arrays are required");
    MPG_CHECK(!eng->hydropar.DensityIndependentSphOn || A->egywtdensity, "hydro_force: pressure-entropy SPH needs egywtdensity");
    MPG_HIP(hipSetDevice(eng->device));
    const SphView v = make_sph_view(eng, A);
    // decoupled wind gas: only with the model's bit AND a DelayTime column; otherwise the loop without the rule, as before there was one
    const bool decouple = eng->d_delaytime && eng->have_windpar && (eng->windpar.WindModel & WIND_DECOUPLE_SPH) != 0;
    const HydroWind W{eng->d_delaytime, eng->windpar.WindSpeed, eng->windpar.WindFreeTravelDensThresh, T->atime};
    eng->sph.hydro_force(eng->tree, v, *T, eng->denspar, eng->hydropar, d_active, nactive, eng->n, eng->stream, decouple ? &W : nullptr);
    API_END
}

int mpg_dev_set_delaytime(mpg_engine *eng, const double *d_delaytime)
{
    API_BEGIN
    MPG_CHECK(eng, "null argument");
    eng->d_delaytime = d_delaytime;
    API_END
}

int mpg_set_delaytime(mpg_engine *eng, const double *delaytime)
{
    API_BEGIN
    MPG_CHECK(eng, "null argument");
    eng->h_delaytime = delaytime;
    API_END
}

int mpg_sph_get_stats(mpg_engine *eng, int64_t stats[4])
{
    API_BEGIN
    MPG_CHECK(eng && stats, "null argument");
    const int64_t last[4] = {eng->sph.last_iterations, eng->sph.last_targets, eng->sph.last_interactions, eng->sph.last_candidates};
    copy_stats(stats, last, 4);
    API_END
}

/* ------------------------------ DM velocity dispersion (veldisp.c) ------------------------------ */

int mpg_dev_find_vel_disp(mpg_engine *eng, const mpg_veldisp_arrays *A, const mpg_sph_times *T, const mpg_veldisp_params *par, const int *d_active,
                          int64_t nactive)
{
    API_BEGIN
    MPG_CHECK(eng && A && T && par, "null argument");
    MPG_CHECK(A->vel && A->hsml && A->density && A->vdisp, "find_vel_disp: the arrays vel, hsml, density and vdisp are required");
    const uint8_t *flags = active_call(eng, "find_vel_disp", d_active, nactive);
    VdispView v{};
    v.pos = eng->d_pos;
    v.type = eng->d_type;
    v.vel = A->vel;
    v.gacc = A->gacc;
    v.gpm = A->gpm;
    v.tb_grav = A->tb_grav;
    v.hsml = A->hsml;
    v.dthsml = A->dthsml;
    v.density = A->density;
    v.vdisp = A->vdisp;
    VdispScalars S;
    S.box = eng->box;
    S.hubble_a2 = par->hubble * par->Time * par->Time; // veldisp.c:265
    S.ddrift = par->ddrift;
    S.dens_threshold = 0.1 * par->sfr_density_threshold; // veldisp.c:362
    // nothing qualifies and the table holds no black hole: nothing is built, nothing is written (veldisp.c:413)
    if(eng->vdisp.make_queues(v, S, flags, eng->n, eng->stream)) {
        // force_tree_rebuild_mask(tree, ddecomp, DMMASK, NULL), veldisp.c:414: the engine's current tree is, from here on, the tree of the
        // DM particles without moments
        MPG_CALL(mpg_dev_force_tree_rebuild_mask(eng, 2 /* DMMASK */, 0));
        if(eng->vdisp.nbh > 0 || eng->vdisp.ngas > 0)
            eng->vdisp.search(eng->tree, v, *T, S, eng->stream);
    }
    API_END
}

int mpg_veldisp_get_stats(mpg_engine *eng, int64_t stats[5])
{
    API_BEGIN
    MPG_CHECK(eng && stats, "null argument");
    const VdispEngine &V = eng->vdisp;
    const int64_t last[5] = {V.last_iterations, V.last_targets, V.last_neighbours, V.last_candidates, V.last_tight};
    copy_stats(stats, last, 5);
    API_END
}

int mpg_veldisp_export(mpg_engine *eng, int64_t n, double *radius, int32_t *iterations, int32_t *numngb, int32_t *maxcmpte, int64_t *queue_lengths,
                       int64_t queue_capacity)
{
    API_BEGIN
    MPG_CHECK(eng, "null argument");
    VdispEngine &V = eng->vdisp;
    export_begin(eng, n, V.n_state, "mpg_veldisp_export: n is not the particle number of the last find_vel_disp call");
    copy_down(radius, V.evalradius.p, n);
    copy_down(iterations, V.niter.p, n);
    copy_down(numngb, V.ngb.p, n);
    copy_down(maxcmpte, V.maxcmpte.p, n);
    copy_queue_lengths(queue_lengths, queue_capacity, V.queue_lengths);
    API_END
}

/* ------------------------------ radiative cooling (cooling.c, cooling_rates.c, sfr_eff.c:463-514) ------------------------------ */

int mpg_set_cooling_params(mpg_engine *eng, const mpg_cooling_params *par)
{
    API_BEGIN
    MPG_CHECK(eng && par, "null argument");
    MPG_HIP(hipSetDevice(eng->device));
    eng->cooling.set_params(*par, eng->stream);
    API_END
}

int mpg_set_metal_cooling_table(mpg_engine *eng, int nz, const double *zbins, int nnh, const double *nhbins, int nt, const double *tbins,
                                const double *rate)
{
    API_BEGIN
    MPG_CHECK(eng, "null argument");
    MPG_HIP(hipSetDevice(eng->device));
    MPG_HIP(hipStreamSynchronize(eng->stream)); // (a kernel in flight may still read the table this call replaces)
    eng->cooling.set_metal_table(nz, zbins, nnh, nhbins, nt, tbins, rate, eng->stream);
    API_END
}

int mpg_dev_cooling(mpg_engine *eng, const mpg_cooling_arrays *A, const mpg_sph_times *T, const mpg_cooling_step *step, const int *d_active,
                    int64_t nactive)
{
    API_BEGIN
    MPG_CHECK(eng && A && T && step, "null argument");
    MPG_CHECK(nactive >= 0, "cooling: negative list length");
    MPG_CHECK(eng->n == 0 || (A->density && A->entropy && A->ne && A->sfr), "cooling: the arrays density, entropy, ne and sfr are required");
    MPG_CHECK(eng->d_mass || eng->n == 0, "cooling: no particles bound");
    MPG_HIP(hipSetDevice(eng->device));
    const bool jm = eng->cooling.j21_mode(1 / T->atime - 1);
    eng->cooling.check_excursion_columns("cooling", 1 / T->atime - 1, eng->n);
    if(eng->cooling.have_uvf && !jm) // the zreion of every listed gas row from the bound positions (get_local_UVBG_from_global)
        eng->cooling.uvf_rows(eng->d_pos, eng->d_type, eng->d_mass, d_active, nactive, eng->n, eng->stream);
    const int64_t bad = eng->cooling.run(*A, eng->d_type, eng->d_mass, *T, *step, d_active, nactive, eng->n, eng->stream);
    // the reference's endrun(1 / 10): every other particle of the call has been treated
    MPG_CHECK(bad == 0, "cooling: " + std::to_string(bad) + " particle(s) hit an iteration limit of DoCooling or of the ionisation network, or reached an "
                                                           "electron abundance that is not finite" +
                            (jm                      ? ", or have a local_J21 that is NaN or negative or a zreion that is NaN"
                             : eng->cooling.have_uvf ? ", or have a position at which the UV-fluctuation table cannot be read (not finite)"
                                                     : "") +
                            "; they keep their Entropy and Ne");
    API_END
}

/* ------------------------------ the excursion set's J21 (cooling_uvfluc.c:199-246) ------------------------------ */

int mpg_set_excursion_set(mpg_engine *eng, const mpg_excursion_set_params *par)
{
    API_BEGIN
    MPG_CHECK(eng, "null argument");
    eng->cooling.set_excursion_set(par);
    API_END
}

int mpg_dev_set_excursion_columns(mpg_engine *eng, const double *d_local_J21, const double *d_zreion)
{
    API_BEGIN
    MPG_CHECK(eng, "null argument");
    MPG_CHECK((d_local_J21 == nullptr) == (d_zreion == nullptr), "mpg_dev_set_excursion_columns: local_J21 and zreion go together");
    eng->cooling.d_j21 = d_local_J21;
    eng->cooling.d_zre = d_zreion;
    eng->cooling.n_exc = d_local_J21 ? eng->n : 0;
    API_END
}

int mpg_set_excursion_columns(mpg_engine *eng, const double *local_J21, const double *zreion)
{
    API_BEGIN
    MPG_CHECK(eng, "null argument");
    MPG_CHECK((local_J21 == nullptr) == (zreion == nullptr), "mpg_set_excursion_columns: local_J21 and zreion go together");
    eng->cooling.h_j21 = local_J21;
    eng->cooling.h_zre = zreion;
    API_END
}

int mpg_dev_excursion_uvbg(mpg_engine *eng, int64_t n, const double *d_J21, const double *d_zreion, double redshift, const mpg_uvbg *global,
                           mpg_uvbg *d_out)
{
    API_BEGIN
    MPG_CHECK(eng && global && n >= 0, "null argument");
    MPG_CHECK(n == 0 || (d_J21 && d_zreion && d_out), "mpg_dev_excursion_uvbg: J21, zreion and out are required");
    MPG_HIP(hipSetDevice(eng->device));
    const int64_t bad = eng->cooling.excursion_points(n, d_J21, d_zreion, redshift, *global, d_out, eng->stream);
    MPG_CHECK(bad == 0, "mpg_dev_excursion_uvbg: " + std::to_string(bad) + " point(s) have a J21 that is NaN or negative or a zreion that is NaN; "
                                                                          "their background is NaN");
    API_END
}

/* ------------------------------ the UV-fluctuation table (cooling_uvfluc.c:115-197) ------------------------------ */

int mpg_set_uvf_table(mpg_engine *eng, int64_t Nside, const double *table, double BoxSize)
{
    API_BEGIN
    MPG_CHECK(eng, "null argument");
    MPG_HIP(hipSetDevice(eng->device));
    MPG_HIP(hipStreamSynchronize(eng->stream)); // (a kernel in flight may still read the table this call replaces)
    eng->cooling.set_uvf_table(Nside, table, BoxSize, eng->stream);
    API_END
}

int mpg_set_uvf_offset(mpg_engine *eng, const double offset[3])
{
    API_BEGIN
    MPG_CHECK(eng && offset, "null argument");
    MPG_CHECK(offset[0] - offset[0] == 0 && offset[1] - offset[1] == 0 && offset[2] - offset[2] == 0, "mpg_set_uvf_offset: offset is not finite");
    for(int d = 0; d < 3; d++)
        eng->cooling.uvf_off[d] = offset[d];
    API_END
}

int mpg_dev_uvf_zreion(mpg_engine *eng, int64_t n, const double *d_pos, double *d_zreion)
{
    API_BEGIN
    MPG_CHECK(eng && n >= 0, "null argument");
    MPG_CHECK(n == 0 || (d_pos && d_zreion), "mpg_dev_uvf_zreion: pos and zreion are required");
    MPG_HIP(hipSetDevice(eng->device));
    const int64_t bad = eng->cooling.uvf_points(n, d_pos, d_zreion, eng->stream);
    // (the reference: undefined behaviour) every other point of the call has its value
    MPG_CHECK(bad == 0, "mpg_dev_uvf_zreion: " + std::to_string(bad) + " point(s) have a coordinate that is not finite or lies 2^31 cells or more "
                                                                      "from the table's origin; their zreion is NaN");
    API_END
}

int mpg_uvf_export(mpg_engine *eng, int64_t n, double *zreion)
{
    API_BEGIN
    MPG_CHECK(eng && zreion, "null argument");
    export_begin(eng, n, eng->cooling.n_uvf, "mpg_uvf_export: n is not the particle number of the last cooling call with a UV-fluctuation table");
    copy_down(zreion, eng->cooling.uvf_z.p, n);
    API_END
}

int mpg_dev_cooling_state(mpg_engine *eng, int64_t n, const double *d_rho, const double *d_u, double *d_ne_inout, double *d_lambdanet,
                          double *d_temp, double *d_nh0, const mpg_cooling_step *step)
{
    API_BEGIN
    MPG_CHECK(eng && step && n >= 0, "null argument");
    MPG_CHECK(n == 0 || (d_rho && d_u && d_ne_inout), "cooling_state: rho, u and ne are required");
    MPG_HIP(hipSetDevice(eng->device));
    const int64_t bad = eng->cooling.state(n, d_rho, d_u, d_ne_inout, d_lambdanet, d_temp, d_nh0, *step, eng->stream);
    MPG_CHECK(bad == 0, "cooling_state: the ionisation network did not converge for " + std::to_string(bad) + " point(s)");
    API_END
}

int mpg_cooling_get_stats(mpg_engine *eng, int64_t stats[6])
{
    API_BEGIN
    MPG_CHECK(eng && stats, "null argument");
    copy_stats(stats, eng->cooling.stats, 6);
    API_END
}

int mpg_cooling_export(mpg_engine *eng, int64_t n, int32_t *evaluations)
{
    API_BEGIN
    MPG_CHECK(eng && evaluations, "null argument");
    export_begin(eng, n, eng->cooling.n_evals, "mpg_cooling_export: n is not the particle number of the last cooling call");
    copy_down(evaluations, eng->cooling.d_evals.p, n);
    API_END
}

/* ------------------------------ stellar mass and metal return (metal_return.c) ------------------------------ */

int mpg_set_metal_params(mpg_engine *eng, const mpg_metal_params *par)
{
    API_BEGIN
    MPG_CHECK(eng && par, "null argument");
    MPG_CHECK(par->MaxNgbDeviation >= 0 && par->MaxGasMass > 0, "metal parameters: MaxNgbDeviation >= 0 and MaxGasMass > 0 are required");
    eng->metalpar = *par;
    API_END
}

int mpg_dev_metal_return(mpg_engine *eng, const mpg_metal_arrays *A, const int *d_active, int64_t nactive)
{
    API_BEGIN
    MPG_CHECK(eng && A, "null argument");
    MPG_CHECK(nactive >= 0, "metal_return: negative list length");
    MPG_CHECK(A->massgenerated && A->metalgenerated && A->speciesgenerated && A->stellarage && A->mass && A->hsml && A->totalmassreturned &&
                  A->lastenrichment && A->density && A->metallicity && A->metals,
              "metal_return: every array but massreturned and starvolume is required");
    MPG_CHECK(eng->metalpar.MaxGasMass > 0, "metal_return: no parameters (mpg_set_metal_params first)");
    const uint8_t *flags = active_call(eng, "metal_return", d_active, nactive);
    MetalView v{};
    v.pos = eng->d_pos;
    v.type = eng->d_type;
    v.massgenerated = A->massgenerated;
    v.metalgenerated = A->metalgenerated;
    v.speciesgenerated = A->speciesgenerated;
    v.stellarage = A->stellarage;
    v.mass = A->mass;
    v.hsml = A->hsml;
    v.totalmassreturned = A->totalmassreturned;
    v.lastenrichment = A->lastenrichment;
    v.density = A->density;
    v.metallicity = A->metallicity;
    v.metals = A->metals;
    v.massreturned = A->massreturned;
    v.starvolume = A->starvolume;
    MetalScalars S;
    S.box = eng->box;
    S.desnumngb = sph_desnumngb(eng->denspar); // GetNumNgb(GetDensityKernelType()), metal_return.c:960
    S.maxdev = eng->metalpar.MaxNgbDeviation;
    S.maxgasmass = eng->metalpar.MaxGasMass;
    S.sphweight = eng->metalpar.SPHWeighting != 0;
    S.ktype = kernel_index(eng->denspar.DensityKernelType);
    // no target: nothing further is read, nothing is written, no tree is demanded
    if(eng->metals.make_queue(v, S, flags, eng->n, eng->stream) > 0) {
        require_gas_tree(eng, "metal_return");
        eng->metals.run(eng->tree, v, S, eng->n, eng->stream);
    }
    API_END
}

int mpg_metals_get_stats(mpg_engine *eng, int64_t stats[6])
{
    API_BEGIN
    MPG_CHECK(eng && stats, "null argument");
    const MetalsEngine &M = eng->metals;
    const int64_t last[6] = {M.last_iterations, M.last_targets, M.last_neighbours, M.last_candidates, M.last_refused, M.last_tight};
    copy_stats(stats, last, 6);
    API_END
}

int mpg_metals_get_times(mpg_engine *eng, double ms[3])
{
    API_BEGIN
    MPG_CHECK(eng && ms, "null argument");
    copy_times(ms, eng->metals.last_ms, 3);
    API_END
}

int mpg_metals_export(mpg_engine *eng, int64_t n, double *radius, int32_t *iterations, int32_t *maxcmpte, int32_t *close, int64_t *queue_lengths,
                      int64_t queue_capacity)
{
    API_BEGIN
    MPG_CHECK(eng, "null argument");
    MetalsEngine &M = eng->metals;
    export_begin(eng, n, M.n_state, "mpg_metals_export: n is not the particle number of the last metal_return call");
    copy_down(radius, M.evalradius.p, n);
    copy_down(iterations, M.niter.p, n);
    copy_down(maxcmpte, M.maxcmpte.p, n);
    copy_down(close, M.close.p, n);
    copy_queue_lengths(queue_lengths, queue_capacity, M.queue_lengths);
    API_END
}

/* ------------------------------ black-hole accretion, mergers and feedback (blackhole.c) ------------------------------ */

int mpg_set_random_table(mpg_engine *eng, const double *table, int64_t size)
{
    API_BEGIN
    MPG_CHECK(eng && table && size > 0, "random table: a table of at least one entry is required");
    MPG_HIP(hipSetDevice(eng->device));
    eng->bh.set_random_table(table, size, eng->stream);
    eng->heiii.rnd.assign(table, table + size); // the choices and radii of the helium reionisation are the host's
    API_END
}

int mpg_set_blackhole_params(mpg_engine *eng, const mpg_blackhole_params *par)
{
    API_BEGIN
    MPG_CHECK(eng && par, "null argument");
    // what the engine does not carry is refused when it is set, so that a caller keeps its CPU path from the start
    MPG_CHECK((par->BlackHoleFeedbackMethod & 0x20) == 0, "blackhole: BlackHoleFeedbackMethod with BH_FEEDBACK_OPTTHIN is not carried (get_neutral_fraction_sfreff)");
    MPG_CHECK(par->BHFeedbackUseTcool != 2, "blackhole: BHFeedbackUseTcool == 2 is not carried (get_egyeff)");
    MPG_CHECK(par->GravInternal > 0 && par->HubbleParam > 0 && par->UnitTime_in_s > 0 && par->UnitVelocity_in_cm_per_s > 0 && par->uu_in_cgs > 0,
              "blackhole parameters: GravInternal, HubbleParam and the units must be positive");
    eng->bhpar = *par;
    eng->have_bhpar = true;
    API_END
}

void blackhole_call(mpg_engine *eng, const mpg_blackhole_arrays *A, const mpg_sph_times *T, const int *d_active, int64_t nactive, int build)
{
    MPG_CHECK(eng && A && T, "null argument");
    MPG_CHECK(nactive >= 0, "blackhole: negative list length");
    MPG_CHECK(eng->have_bhpar, "blackhole: no parameters (mpg_set_blackhole_params first)");
    MPG_CHECK(eng->bh.rndsize > 0, "blackhole: no random table (mpg_set_random_table first)");
    for(const ArrayField &F : BH_FIELDS)
        MPG_CHECK(field_get(*A, F.off) || (F.role & ARR_OPTIONAL) || eng->n == 0, std::string("blackhole: the array ") + F.name + " is required");
    const uint8_t *flags = active_call(eng, "blackhole", d_active, nactive);
    const mpg_blackhole_params &P = eng->bhpar;
    BhView v{eng->d_pos, eng->d_type, *A};
    BhScalars S;
    S.p = P;
    S.merge_dist = 2 * (P.ForceSoftening > 0 ? P.ForceSoftening : 2.8 * eng->GravitySoftening) / 2.8; // blackhole.c:503
    S.a3inv = 1. / (T->atime * T->atime * T->atime);
    // blackhole.c:379-380, physconst.h
    S.meddington_fac = (4 * M_PI * 6.672e-8 * 2.99792458e10 * 1.6726e-24 / (0.1 * 2.99792458e10 * 2.99792458e10 * 6.65245e-25)) * P.UnitTime_in_s / P.HubbleParam;
    S.c2 = pow(2.99792458e10 / P.UnitVelocity_in_cm_per_s, 2);
    S.rho_sfr = P.BHKE_SfrCritOverDensity * (P.OmegaBaryon * 3 * P.Hubble * P.Hubble / (8 * M_PI * P.GravInternal)); // :450-451
    S.ucap = 5.0e8 / ((4 / (8 - 5 * (1 - 0.76))) * 1.6726e-24 / 1.38066e-16 * (5.0 / 3.0 - 1) * P.uu_in_cgs);           // :722-725
    S.ktype = kernel_index(eng->denspar.DensityKernelType);
    S.rnd = eng->bh.rnd.p;
    S.rndsize = (uint64_t)eng->bh.rndsize;
    // no target: nothing further is read, nothing is written, no tree is demanded
    if(eng->bh.make_queue(eng->d_type, flags, eng->n, eng->stream) > 0) {
        const bool fits = eng->tree_allocated && (eng->tree_mask & 33) == 33 && eng->tree.has_hmax;
        if(build == 2 || (!fits && build == 1)) {
            MPG_CALL(mpg_dev_force_tree_rebuild_mask(eng, 33 /* GASMASK + BHMASK */, 0));
            MPG_CALL(mpg_dev_force_update_hmax(eng, A->hsml));
        }
        // blackhole.c:237-238, treewalk.c:941-945
        require_gas_tree(eng, "blackhole");
        MPG_CHECK((eng->tree_mask & 32) != 0, "blackhole: the current tree does not contain the black holes (BHMASK)");
        MPG_CHECK(eng->tree.has_hmax, "blackhole: symmetric search on a tree without hmax (force_tree_calc_moments first)");
        MPG_CHECK(S.merge_dist > 0, "blackhole: no force softening");
        eng->bh.run(eng->tree, v, *T, S, eng->n, eng->stream);
    }
}

int64_t blackhole_targets(mpg_engine *eng, const int *d_active, int64_t nactive)
{
    MPG_CHECK(eng && nactive >= 0, "blackhole: null engine or negative list length");
    return eng->bh.make_queue(eng->d_type, active_call(eng, "blackhole", d_active, nactive), eng->n, eng->stream);
}

int mpg_dev_blackhole(mpg_engine *eng, const mpg_blackhole_arrays *A, const mpg_sph_times *T, const int *d_active, int64_t nactive)
{
    API_BEGIN
    blackhole_call(eng, A, T, d_active, nactive, 0);
    API_END
}

int mpg_blackhole_get_stats(mpg_engine *eng, int64_t stats[8])
{
    API_BEGIN
    MPG_CHECK(eng && stats, "null argument");
    copy_stats(stats, eng->bh.last_stats, BH_NSTATS);
    API_END
}

int mpg_blackhole_get_times(mpg_engine *eng, double ms[3])
{
    API_BEGIN
    MPG_CHECK(eng && ms, "null argument");
    copy_times(ms, eng->bh.last_ms, 3);
    API_END
}

/* ------------------------------ the wind model (winds.c) ------------------------------ */

int mpg_set_wind_params(mpg_engine *eng, const mpg_wind_params *par)
{
    API_BEGIN
    MPG_CHECK(eng && par, "null argument");
    char model[32];
    snprintf(model, sizeof(model), "0x%X", (unsigned)par->WindModel);
    // init_winds, winds.c:98-101
    MPG_CHECK((par->WindModel & (WIND_FIXED_EFFICIENCY | WIND_USE_HALO)) != 0, std::string("WindModel = ") + model + " is strange. This shall not happen.");
    eng->windpar = *par;
    eng->have_windpar = true;
    API_END
}

// the view and the scalars of a wind call on the bound particles
static void winds_setup(mpg_engine *eng, const mpg_wind_arrays *A, double atime, const char *who, WindView &v, WindScalars &S)
{
    MPG_CHECK(eng->have_windpar, std::string(who) + ": no parameters (mpg_set_wind_params first)");
    MPG_CHECK(eng->d_pos || eng->n == 0, std::string(who) + ": no particles bound");
    MPG_HIP(hipSetDevice(eng->device));
    v = WindView{eng->d_pos, eng->d_mass, eng->d_type, eng->n, *A};
    S.p = eng->windpar;
    S.atime = atime;
    S.rnd = eng->bh.rnd.p;
    S.rndsize = (uint64_t)eng->bh.rndsize;
}

int mpg_dev_winds_and_feedback(mpg_engine *eng, const mpg_wind_arrays *A, const int *d_newstars, int64_t nnew, double atime)
{
    API_BEGIN
    MPG_CHECK(eng && A, "null argument");
    MPG_CHECK(nnew >= 0, "winds_and_feedback: negative list length");
    WindView v;
    WindScalars S;
    winds_setup(eng, A, atime, "winds_and_feedback", v, S);
    eng->winds.reset();
    // winds.c:302-306: the subgrid model does nothing here; without a new star nothing is read, nothing is written, no tree is demanded
    if((eng->windpar.WindModel & WIND_SUBGRID) == 0 && nnew > 0) {
        MPG_CHECK(d_newstars, "winds_and_feedback: no list of new stars");
        MPG_CHECK(eng->bh.rndsize > 0, "winds_and_feedback: no random table (mpg_set_random_table first)");
        MPG_CHECK(A->id && A->hsml && A->vdisp && A->density && A->vel && A->entropy && A->delaytime,
                  "winds_and_feedback: the arrays id, hsml, vdisp, density, vel, entropy and delaytime are required");
        eng->winds.check_stars(v, d_newstars, nnew, eng->stream);
        require_gas_tree(eng, "winds_and_feedback");
        eng->winds.run(eng->tree, v, S, d_newstars, nnew, eng->stream);
    }
    API_END
}

int mpg_dev_winds_subgrid(mpg_engine *eng, const mpg_wind_arrays *A, const int *d_maybewind, int64_t n, const double *d_stellarmass, double atime)
{
    API_BEGIN
    MPG_CHECK(eng && A, "null argument");
    MPG_CHECK(n >= 0, "winds_subgrid: negative list length");
    WindView v;
    WindScalars S;
    winds_setup(eng, A, atime, "winds_subgrid", v, S);
    eng->winds.reset();
    if((eng->windpar.WindModel & WIND_SUBGRID) != 0 && n > 0) { // winds.c:279-283
        MPG_CHECK(eng->bh.rndsize > 0, "winds_subgrid: no random table (mpg_set_random_table first)");
        MPG_CHECK(d_stellarmass && A->id && A->vdisp && A->density && A->vel && A->entropy && A->delaytime && eng->d_mass,
                  "winds_subgrid: the stellar masses and the arrays id, vdisp, density, vel, entropy and delaytime are required");
        eng->winds.subgrid(v, S, d_maybewind, n, d_stellarmass, eng->stream);
    }
    API_END
}

int mpg_dev_winds_evolve(mpg_engine *eng, const mpg_wind_arrays *A, const mpg_sph_times *T, const int *d_active, int64_t nactive)
{
    API_BEGIN
    MPG_CHECK(eng && A && T, "null argument");
    MPG_CHECK(nactive >= 0, "winds_evolve: negative list length");
    WindView v;
    WindScalars S;
    winds_setup(eng, A, T->atime, "winds_evolve", v, S);
    const int64_t nlist = d_active ? nactive : eng->n;
    if(nlist > 0) {
        MPG_CHECK(A->density && A->tb_hydro && A->delaytime, "winds_evolve: the arrays density, tb_hydro and delaytime are required");
        eng->winds.evolve(v, S, *T, d_active, nlist, eng->stream);
    }
    API_END
}

int mpg_winds_get_stats(mpg_engine *eng, int64_t stats[6], double *maxvel)
{
    API_BEGIN
    MPG_CHECK(eng && stats, "null argument");
    copy_stats(stats, eng->winds.last_stats, WD_NSTATS);
    if(maxvel)
        *maxvel = eng->winds.last_maxvel;
    API_END
}

int mpg_winds_export(mpg_engine *eng, int64_t capacity, int32_t *star, int32_t *gas, int64_t *count)
{
    API_BEGIN
    MPG_CHECK(eng && count && capacity >= 0, "null argument");
    const int64_t nk = eng->winds.last_stats[3], m = eng->winds.last_capacity;
    *count = nk;
    if(m > 0 && (star || gas)) {
        MPG_HIP(hipSetDevice(eng->device));
        MPG_HIP(hipStreamSynchronize(eng->stream));
        const TreeView tv = eng->tree.view();
        std::vector<WindKick> k((size_t)m);
        std::vector<int> order((size_t)tv.npart);
        MPG_HIP(hipMemcpy(k.data(), eng->winds.kicks.p, (size_t)m * sizeof(WindKick), hipMemcpyDeviceToHost));
        MPG_HIP(hipMemcpy(order.data(), tv.order, (size_t)tv.npart * sizeof(int), hipMemcpyDeviceToHost));
        int64_t out = 0;
        for(int64_t e = 0; e < m && out < capacity; e++) {
            if(k[e].star < 0) // an unused entry of a star's segment
                continue;
            MPG_CHECK(k[e].slot >= 0 && k[e].slot < tv.npart, "mpg_winds_export: the tree of the last call is gone");
            if(star)
                star[out] = k[e].star;
            if(gas)
                gas[out] = order[k[e].slot];
            out++;
        }
    }
    API_END
}

int mpg_winds_get_times(mpg_engine *eng, double ms[3])
{
    API_BEGIN
    MPG_CHECK(eng && ms, "null argument");
    copy_times(ms, eng->winds.last_ms, 3);
    API_END
}

/* ------------------------------ star formation (sfr_eff.c:186-394) ------------------------------ */

int mpg_set_sfr_params(mpg_engine *eng, const mpg_sfr_params *par)
{
    API_BEGIN
    MPG_CHECK(eng && par, "null argument");
    eng->sfr.set_params(*par, eng->cooling.have_uvf, eng->cooling.have_exc);
    API_END
}

int mpg_dev_cooling_and_starformation(mpg_engine *eng, const mpg_sfr_columns *A, const mpg_sph_times *T, const mpg_cooling_step *step,
                                      const int *d_active, int64_t nactive)
{
    API_BEGIN
    MPG_CHECK(eng && A && T && step, "null argument");
    MPG_CHECK(nactive >= 0, "cooling_and_starformation: negative list length");
    MPG_CHECK(eng->sfr.have_params, "cooling_and_starformation: no parameters (mpg_set_sfr_params first)");
    MPG_CHECK(eng->bh.rndsize > 0, "cooling_and_starformation: no random table (mpg_set_random_table first)");
    MPG_CHECK(eng->d_mass || eng->n == 0, "cooling_and_starformation: no particles bound");
    const mpg_sfr_params &P = eng->sfr.par;
    // starformation and cooling_direct take the background get_local_UVBG gives: the setting and the table go together
    MPG_CHECK((P.UVFluctuationOn != 0) == eng->cooling.have_uvf,
              P.UVFluctuationOn ? "cooling_and_starformation: UVFluctuationOn is set but the engine holds no UV-fluctuation table (mpg_set_uvf_table)"
                                : "cooling_and_starformation: the engine holds a UV-fluctuation table but UVFluctuationOn is 0 (mpg_set_sfr_params)");
    MPG_CHECK(!P.ExcursionSetReion || eng->cooling.have_exc,
              "cooling_and_starformation: ExcursionSetReion (EXCUR_REION) is set but the engine holds no excursion-set model (mpg_set_excursion_set)");
    const bool jm = eng->cooling.j21_mode(1 / T->atime - 1);
    eng->cooling.check_excursion_columns("cooling_and_starformation", 1 / T->atime - 1, eng->n);
    MPG_CHECK(!(P.WindOn || A->delaytime) || eng->have_windpar, "cooling_and_starformation: no wind parameters (mpg_set_wind_params first)");
    const bool subgrid = P.WindOn && (eng->windpar.WindModel & WIND_SUBGRID) != 0; // winds_are_subgrid, sfr_eff.c:205, 280
    if(eng->n > 0) {
        MPG_CHECK(A->id && A->density && A->entropy && A->ne && A->sfr && A->metallicity,
                  "cooling_and_starformation: the columns id, density, entropy, ne, sfr and metallicity are required");
        if(!(P.QuickLymanAlphaProbability > 0)) {
            MPG_CHECK(!mpg::sfr::has(P.StarformationCriterion, mpg::sfr::CRIT_MOLECULAR_H2) || (A->hsml && A->gradrho_mag),
                      "cooling_and_starformation: SFR_CRITERION_MOLECULAR_H2 needs the columns hsml and gradrho_mag");
            MPG_CHECK(!mpg::sfr::has(P.StarformationCriterion, mpg::sfr::CRIT_SELFGRAVITY) || (A->divvel && A->curlvel),
                      "cooling_and_starformation: SFR_CRITERION_SELFGRAVITY needs the columns divvel and curlvel");
        }
        MPG_CHECK(!subgrid || (A->vdisp && A->vel && A->delaytime && A->stellarmass),
                  "cooling_and_starformation: WIND_SUBGRID needs the columns vdisp, vel, delaytime and stellarmass");
    }
    MPG_HIP(hipSetDevice(eng->device));
    const SfrView v{eng->d_type, eng->d_mass, eng->n, *A, eng->d_pos};
    const int64_t bad = eng->sfr.run(eng->cooling, v, A->delaytime ? &eng->windpar : nullptr, eng->bh.rnd.p, (uint64_t)eng->bh.rndsize, *T, *step, d_active,
                                     nactive, eng->stream);
    if(subgrid) { // sfr_eff.c:280-286
        mpg_wind_arrays W{};
        W.id = A->id;
        W.vdisp = A->vdisp;
        W.density = A->density;
        W.vel = A->vel;
        W.entropy = A->entropy;
        W.delaytime = A->delaytime;
        WindView wv;
        WindScalars S;
        winds_setup(eng, &W, T->atime, "cooling_and_starformation", wv, S);
        eng->winds.reset();
        if(eng->sfr.last.maybewind > 0)
            eng->winds.subgrid(wv, S, eng->sfr.maybewind.p, eng->sfr.last.maybewind, A->stellarmass, eng->stream);
    }
    // the reference's endrun(1 / 10): every other row of the call has been treated
    MPG_CHECK(bad == 0, "cooling_and_starformation: " + std::to_string(bad) + " row(s) hit an iteration limit of DoCooling or of the ionisation network, or reached "
                                                                             "an electron abundance that is not finite" +
                            (jm                      ? ", or have a local_J21 that is NaN or negative or a zreion that is NaN"
                             : eng->cooling.have_uvf ? ", or have a position at which the UV-fluctuation table cannot be read (not finite)"
                                                     : "") +
                            "; they keep their columns and form no star");
    API_END
}

int mpg_sfr_get_result(mpg_engine *eng, mpg_sfr_result *result)
{
    API_BEGIN
    MPG_CHECK(eng && result, "null argument");
    *result = eng->sfr.last;
    API_END
}

int mpg_sfr_export(mpg_engine *eng, int64_t capacity, int32_t *parent, double *mass_of_star, uint8_t *spawn, int64_t *nnew, int64_t wcapacity,
                   int32_t *maybewind, int64_t *nmaybewind)
{
    API_BEGIN
    MPG_CHECK(eng && capacity >= 0 && wcapacity >= 0, "mpg_sfr_export: null engine or negative capacity");
    const SfrEngine &E = eng->sfr;
    MPG_HIP(hipSetDevice(eng->device));
    MPG_HIP(hipStreamSynchronize(eng->stream));
    const int64_t m = capacity < E.last.newstars ? capacity : E.last.newstars, mw = wcapacity < E.last.maybewind ? wcapacity : E.last.maybewind;
    copy_down(parent, E.ns_parent.p, m);
    copy_down(mass_of_star, E.ns_mass.p, m);
    copy_down(spawn, E.ns_spawn.p, m);
    copy_down(maybewind, E.maybewind.p, mw);
    if(nnew)
        *nnew = E.last.newstars;
    if(nmaybewind)
        *nmaybewind = E.last.maybewind;
    API_END
}

int mpg_sfr_dev_lists(mpg_engine *eng, const int **d_parent, const double **d_mass_of_star, const uint8_t **d_spawn, const int **d_maybewind)
{
    API_BEGIN
    MPG_CHECK(eng, "null argument");
    if(d_parent)
        *d_parent = eng->sfr.ns_parent.p;
    if(d_mass_of_star)
        *d_mass_of_star = eng->sfr.ns_mass.p;
    if(d_spawn)
        *d_spawn = eng->sfr.ns_spawn.p;
    if(d_maybewind)
        *d_maybewind = eng->sfr.maybewind.p;
    API_END
}

int mpg_sfr_export_rows(mpg_engine *eng, int64_t n, uint8_t *rowclass, int32_t *evaluations)
{
    API_BEGIN
    MPG_CHECK(eng, "null argument");
    export_begin(eng, n, eng->sfr.n_rows, "mpg_sfr_export_rows: n is not the particle number of the last call");
    copy_down(rowclass, eng->sfr.rowclass.p, n);
    copy_down(evaluations, eng->sfr.sfevals.p, n);
    API_END
}

int mpg_sfr_get_stats(mpg_engine *eng, int64_t stats[8])
{
    API_BEGIN
    MPG_CHECK(eng && stats, "null argument");
    copy_stats(stats, eng->sfr.last_stats, SFR_NSTATS);
    API_END
}

/* ------------------------------ helium reionisation by quasar bubbles (cooling_qso_lightup.c) ------------------------------ */

int mpg_set_heiii_params(mpg_engine *eng, const mpg_heiii_params *par)
{
    API_BEGIN
    MPG_CHECK(eng && par, "null argument");
    MPG_CHECK(par->var_bubble >= 0, "heiii parameters: var_bubble is a variance");
    eng->heiii.par = *par;
    eng->heiii.have_par = true;
    API_END
}

int mpg_heiii_set_batch(mpg_engine *eng, int batch)
{
    API_BEGIN
    MPG_CHECK(eng, "null argument");
    MPG_CHECK(batch >= 0 && batch <= HEIII_MAXB, "mpg_heiii_set_batch: 0 (the default) or 1 .. 64 bubbles per scan");
    eng->heiii.batch = batch;
    API_END
}

static HeiiiView heiii_view(mpg_engine *eng, const char *who, const double *d_density, double *d_entropy, uint8_t *d_flag)
{
    MPG_CHECK(eng->d_pos || eng->n == 0, std::string(who) + ": no particles bound");
    MPG_CHECK(eng->d_type || eng->n == 0, std::string(who) + ": the bound particles have no type column");
    MPG_CHECK(d_flag || eng->n == 0, std::string(who) + ": the array heiii_ionized is required");
    return HeiiiView{eng->d_pos, eng->d_type, eng->n, d_density, d_entropy, d_flag};
}

int mpg_dev_heiii_ionization_fraction(mpg_engine *eng, const uint8_t *d_heiii_ionized, int64_t n_gas_tot, int64_t *n_ionized, double *fraction)
{
    API_BEGIN
    MPG_CHECK(eng, "null argument");
    MPG_CHECK(n_gas_tot > 0, "heiii_ionization_fraction: n_gas_tot must be positive");
    MPG_HIP(hipSetDevice(eng->device));
    const HeiiiView v = heiii_view(eng, "heiii_ionization_fraction", nullptr, nullptr, (uint8_t *)d_heiii_ionized);
    const int64_t c = eng->heiii.count_ionized(v, eng->stream);
    if(n_ionized)
        *n_ionized = c;
    if(fraction)
        *fraction = (double)c / (double)n_gas_tot; // :381
    API_END
}

void heiii_call(mpg_engine *eng, const mpg_heiii_step *step, const double *d_density, double *d_entropy, uint8_t *d_flag, const HeiiiGroups &groups,
                mpg_heiii_result *result)
{
    MPG_CHECK(eng && step, "null argument");
    MPG_CHECK(eng->heiii.have_par, "heiii_reionization: no parameters (mpg_set_heiii_params first)");
    MPG_CHECK(!eng->heiii.rnd.empty(), "heiii_reionization: no random table (mpg_set_random_table first)");
    MPG_CHECK(step->n_gas_tot > 0, "heiii_reionization: n_gas_tot must be positive");
    MPG_CHECK(step->atime > 0 && step->uu_in_cgs > 0, "heiii_reionization: atime and uu_in_cgs must be positive");
    MPG_HIP(hipSetDevice(eng->device));
    const HeiiiView v = heiii_view(eng, "heiii_reionization", d_density, d_entropy, d_flag);
    MPG_CHECK((d_density && d_entropy) || eng->n == 0, "heiii_reionization: the arrays density and entropy are required");
    try {
        eng->heiii.run(v, eng->box, *step, groups, eng->stream);
    } catch(...) {
        if(result)
            *result = eng->heiii.last;
        throw;
    }
    if(result)
        *result = eng->heiii.last;
}

int mpg_dev_heiii_reionization(mpg_engine *eng, const mpg_heiii_step *step, const double *d_density, double *d_entropy, uint8_t *d_heiii_ionized,
                               const double *d_group_mass, const double *d_group_cm, const uint64_t *d_group_minid, int64_t ngroups,
                               mpg_heiii_result *result)
{
    API_BEGIN
    MPG_CHECK(eng && ngroups >= 0, "heiii_reionization: null engine or negative group number");
    // the groups when the loop asks for them: Mass whole, CM and MinID of the candidates
    const HeiiiGroups groups = [=](const mpg_heiii_params &par, std::vector<int64_t> &cand, std::vector<double> &ccm, std::vector<uint64_t> &cid) {
        MPG_CHECK(ngroups == 0 || (d_group_mass && d_group_cm && d_group_minid), "heiii_reionization: the group columns mass, cm and minid are required");
        std::vector<double> mass((size_t)ngroups);
        if(ngroups > 0) {
            MPG_HIP(hipMemcpyAsync(mass.data(), d_group_mass, (size_t)ngroups * sizeof(double), hipMemcpyDeviceToHost, eng->stream));
            MPG_HIP(hipStreamSynchronize(eng->stream));
        }
        heiii_candidates(par, mass.data(), ngroups, cand);
        eng->heiii.gather_groups(cand, d_group_cm, d_group_minid, ccm, cid, eng->stream);
    };
    heiii_call(eng, step, d_density, d_entropy, d_heiii_ionized, groups, result);
    API_END
}

int mpg_heiii_export(mpg_engine *eng, int64_t capacity, int64_t *position, int64_t *group, double *radius, int64_t *count, double *curionfrac,
                     int64_t *n)
{
    API_BEGIN
    MPG_CHECK(eng && n && capacity >= 0, "null argument");
    const std::vector<HeiiiRecord> &R = eng->heiii.records;
    *n = (int64_t)R.size();
    for(int64_t k = 0; k < (int64_t)R.size() && k < capacity; k++) {
        if(position)
            position[k] = R[k].position;
        if(group)
            group[k] = R[k].group;
        if(radius)
            radius[k] = R[k].radius;
        if(count)
            count[k] = R[k].count;
        if(curionfrac)
            curionfrac[k] = R[k].curionfrac;
    }
    API_END
}

int mpg_heiii_get_times(mpg_engine *eng, double ms[3])
{
    API_BEGIN
    MPG_CHECK(eng && ms, "null argument");
    copy_times(ms, eng->heiii.last_ms, 3);
    API_END
}

/* ------------------------------ black-hole dynamical friction and the potential minimum (bhdynfric.c) ------------------------------ */

int mpg_set_bh_dynfric_params(mpg_engine *eng, const mpg_bh_dynfric_params *par)
{
    API_BEGIN
    MPG_CHECK(eng && par, "null argument");
    MPG_CHECK(par->BH_DynFrictionMethod >= 0 && par->BH_DynFrictionMethod <= 3, "dynamical friction parameters: BH_DynFrictionMethod is 0, 1, 2 or 3");
    MPG_CHECK(par->BH_DynFrictionMethod == 0 || par->GravInternal > 0, "dynamical friction parameters: GravInternal must be positive");
    (void)kernel_index(par->DensityKernelType); // (an unknown kernel type is an error here, not at the first call)
    eng->dfpar = *par;
    eng->have_dfpar = true;
    API_END
}

// blackhole_dynfric_treemask, bhdynfric.c:66-81
static int dynfric_treemask(const mpg_bh_dynfric_params &P)
{
    int mask = 16 + 32; // STARMASK + BHMASK
    if(P.BH_DynFrictionMethod > 1)
        mask += 2; // DMMASK
    if(P.BH_DynFrictionMethod > 2)
        mask += 1; // GASMASK
    if(P.BlackHoleRepositionEnabled)
        mask = 63; // ALLMASK
    return mask;
}

// what dynfric_listed and dynfric_call begin with.  False: the parameters switch the call off (bhdynfric.c:356-362) - nothing is read,
// nothing is written, no tree is built, and no flags are made
static bool dynfric_begin(mpg_engine *eng, const int *d_active, int64_t nactive, const uint8_t *&flags)
{
    MPG_CHECK(eng->have_dfpar, "blackhole_dynfric: no parameters (mpg_set_bh_dynfric_params first)");
    const bool on = eng->dfpar.BH_DynFrictionMethod != 0 || eng->dfpar.BlackHoleRepositionEnabled;
    flags = active_call(eng, "blackhole_dynfric", on ? d_active : nullptr, nactive);
    eng->df.reset();
    return on;
}

int64_t dynfric_listed(mpg_engine *eng, const int *d_active, int64_t nactive)
{
    MPG_CHECK(eng && nactive >= 0, "blackhole_dynfric: null engine or negative list length");
    const uint8_t *flags;
    if(!dynfric_begin(eng, d_active, nactive, flags))
        return 0;
    eng->df.make_queues(eng->d_type, flags, nullptr, 0, eng->n, eng->stream);
    return eng->df.nlisted;
}

void dynfric_call(mpg_engine *eng, const mpg_bh_dynfric_arrays *A, const mpg_sph_times *T, const int *d_active, int64_t nactive)
{
    MPG_CHECK(eng && A && T, "null argument");
    MPG_CHECK(nactive >= 0, "blackhole_dynfric: negative list length");
    const uint8_t *flags;
    if(!dynfric_begin(eng, d_active, nactive, flags))
        return;
    const mpg_bh_dynfric_params &P = eng->dfpar;
    const int method = P.BH_DynFrictionMethod;
    DfView v{eng->d_pos, eng->d_mass, eng->d_type, *A};
    DfScalars S;
    S.p = P;
    S.ktype = kernel_index(P.DensityKernelType);
    const int64_t ntargets = eng->df.make_queues(eng->d_type, flags, method > 0 ? A->active_dynfric : nullptr, method, eng->n, eng->stream);
    if(eng->df.nlisted == 0)
        return;
    // what this method reads and writes
    MPG_CHECK(A->vel && A->hsml && A->potential && A->jumptominpot && A->minpot && A->minpotpos && A->minpotvel,
              "blackhole_dynfric: the arrays vel, hsml, potential, jumptominpot, minpot, minpotpos and minpotvel are required");
    if(method > 0) {
        MPG_CHECK(A->gacc && A->gpm && A->tb_grav && A->bh_mass && A->df_density && A->df_vel && A->df_rmsvel && A->dfaccel,
                  "blackhole_dynfric: dynamical friction needs the arrays gacc, gpm, tb_grav, bh_mass, df_density, df_vel, df_rmsvel and dfaccel");
        MPG_CHECK(method < 3 || (A->hydroacc && A->tb_hydro), "blackhole_dynfric: BH_DynFrictionMethod 3 needs the arrays hydroacc and tb_hydro");
    }
    if(ntargets > 0) {
        // force_tree_rebuild_mask(tree, ddecomp, treemask, NULL), bhdynfric.c:295 / :372: the engine's current tree is, from here on, the
        // tree of this mask without moments
        MPG_CALL(mpg_dev_force_tree_rebuild_mask(eng, dynfric_treemask(P), 0));
        eng->df.walk(eng->tree, v, *T, S, eng->n, eng->stream);
    }
    if(method > 0) // blackhole_dfaccel: every listed black hole, target or not
        eng->df.dfaccel(v, *T, S, eng->stream);
}

int mpg_dev_blackhole_dynfric(mpg_engine *eng, const mpg_bh_dynfric_arrays *A, const mpg_sph_times *T, const int *d_active, int64_t nactive)
{
    API_BEGIN
    dynfric_call(eng, A, T, d_active, nactive);
    API_END
}

int mpg_bh_dynfric_get_stats(mpg_engine *eng, int64_t stats[5], double *zerodfmass)
{
    API_BEGIN
    MPG_CHECK(eng && stats, "null argument");
    copy_stats(stats, eng->df.last_stats, DF_NSTATS);
    if(zerodfmass)
        *zerodfmass = eng->df.last_zeromass;
    API_END
}

int mpg_bh_dynfric_get_times(mpg_engine *eng, double ms[2])
{
    API_BEGIN
    MPG_CHECK(eng && ms, "null argument");
    copy_times(ms, eng->df.last_ms, 2);
    API_END
}

int mpg_bh_dynfric_export(mpg_engine *eng, int64_t n, double *rawsums, int32_t *minidx, int32_t *numngb)
{
    API_BEGIN
    MPG_CHECK(eng, "null argument");
    DynfricEngine &D = eng->df;
    export_begin(eng, n, D.n_state, "mpg_bh_dynfric_export: n is not the particle number of the last blackhole_dynfric walk");
    copy_down(rawsums, D.raw.p, DF_NRAW * n);
    copy_down(minidx, D.minidx.p, n);
    copy_down(numngb, D.numngb.p, n);
    API_END
}

} // extern "C"
