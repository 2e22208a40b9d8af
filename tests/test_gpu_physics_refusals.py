"""The refusals of the gas and subgrid physics entry points (csrc/physics.hip: SPH, velocity dispersion, cooling, the UV-fluctuation table,
metal return, black holes, winds, star formation, helium reionisation, dynamical friction), pinned by their TEXT: every check that arguments
and setter state alone can make fail is driven once, through the library handle engine.py holds, and mpg_last_error() up to the last " ["
(the file:line suffix) is compared with a literal written from the source.  The checks guard the order "refuse, then touch the engine", so a
few steps also look at what a refused call left behind: the statistics of every module, and mpg_tree_get_stats still refusing "no tree"
after a refused find_vel_disp (which would otherwise have built the DM tree).

One engine, driven through a script whose order matters (a setter cannot be undone): a fresh engine with nothing bound (every "no
parameters" refusal, every null pointer, every wrong n of an export), 8 particles without a type column, 8 particles with one (4 gas,
2 DM, 1 star, 1 black hole), then trees of masks 2, 1 and 33.  The columns handed to the calls are one buffer of 512 doubles equal to 1: no
case reaches a kernel that reads more than 8 * 3 of them.  A second engine serves the one refusal that cannot coexist with another on the
first: "no wind parameters" of star formation needs a random table and no wind parameters, "no random table" of the winds the opposite.

Of the 149 MPG_CHECK lines these entry points had while they were part of engine.hip (153 between its SPH and introspection banners, 4 of
them in the tree functions that stayed there), 134 are driven here.  Left out, because no argument or setter reaches them:
 * the 8 "<who>: no particles bound" checks (find_vel_disp, cooling, metal_return, blackhole, the winds' setup, cooling_and_starformation,
   the helium view, blackhole_dynfric): mpg_dev_bind_particles refuses n > 0 without positions and masses, the host forms bind their own;
 * the 3 iteration-limit reports (cooling, cooling_state, cooling_and_starformation): a kernel would have to fail to converge;
 * "mpg_winds_export: the tree of the last call is gone": needs the kicks of a completed call and another tree;
 * the 3 checks of blackhole_targets and dynfric_listed, which only the host forms call, after binding a table and uploading its list;
 * "mpg_dev_uvf_zreion: ... not finite ..." IS driven: the kernel does what it should with a NaN coordinate."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

I64, F64 = C.c_int64, C.c_double
NOARG = "null argument"
STEPS = []   # (id, kind, expected text or None, function of the context)


def refuse(name, want, fn):
    STEPS.append((name, "refuse", want, fn))


def setup(name, fn):
    STEPS.append((name, "setup", None, fn))


def observe(name, fn):
    STEPS.append((name, "observe", None, fn))


class Context:
    def __init__(self, pkg):
        import torch
        self.E = E = pkg.engine
        self.eng, self.eng2 = pkg.Engine(0), pkg.Engine(0)
        self.lib, self.h, self.h2 = self.eng.lib, self.eng.h, self.eng2.h
        rng = np.random.default_rng(7)
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
        self.ones, self.zeros = torch.ones(512, dtype=torch.float64, device="cuda"), torch.zeros(512, dtype=torch.uint8, device="cuda")
        self.pos, self.mass = up(rng.random((8, 3))), up(np.ones(8, np.float32))
        self.type = up(np.array([0, 0, 0, 0, 1, 1, 4, 5], np.uint8))
        self.nan = up(np.full(4, np.nan))   # a point and the place of its result
        self.rows = up(np.arange(8, dtype=np.int32))
        self.star = up(np.array([6], np.int32))
        torch.cuda.synchronize()
        self.B, self.Z = self.ones.data_ptr(), self.zeros.data_ptr()
        self.T = E.SphTimes()
        self.T.atime = 1.0
        self.step = E.CoolingStep()
        self.hstep = E.HeiiiStep(atime=1.0, desired_ion_frac=0.5, qso_inst_heating=1.0, uu_in_cgs=1.0, n_gas_tot=4, non_overlapping_bubble_number=0, TotNgroups=2)
        self.i64, self.f64 = (I64 * 16)(), (F64 * 16)()
        self.snapshot = None

    def close(self):
        self.eng.close()
        self.eng2.close()

    def arrays(self, cls, **over):
        """the struct of array pointers with every member on the buffer of ones, but those named (None: NULL)"""
        a = cls()
        for k, _ in cls._fields_:
            setattr(a, k, over.get(k, self.B))
        return a

    def bind(self, h, type):
        return self.lib.mpg_dev_bind_particles(h, I64(8), C.c_void_p(self.pos.data_ptr()), C.c_void_p(self.mass.data_ptr()),
                                               None if type is None else C.c_void_p(type.data_ptr()), F64(1.0))

    def stats(self):
        """the statistics every module hands out"""
        L, h, out = self.lib, self.h, []
        for fn, n, extra in ((L.mpg_sph_get_stats, 4, 0), (L.mpg_veldisp_get_stats, 5, 0), (L.mpg_cooling_get_stats, 6, 0), (L.mpg_metals_get_stats, 6, 0),
                             (L.mpg_blackhole_get_stats, 8, 0), (L.mpg_winds_get_stats, 6, 1), (L.mpg_sfr_get_stats, 8, 0), (L.mpg_bh_dynfric_get_stats, 5, 1)):
            c, v = (I64 * 8)(), F64(0.0)
            assert (fn(h, c, C.byref(v)) if extra else fn(h, c)) == 0
            out.append(tuple(c[:n]) + (v.value,))
        return out


def p(x):
    return C.c_void_p(x)


# parameter sets that their setters accept
def bhpar(E, **over):
    d = dict(GravInternal=1.0, HubbleParam=0.7, UnitTime_in_s=1.0, UnitVelocity_in_cm_per_s=1e5, uu_in_cgs=1e10)
    d.update(over)
    return E.BlackholeParams(**d)


def sfrpar(E, **over):
    d = dict(StarformationCriterion=E.SFR_CRITERION_DENSITY, Generations=2, PhysDensThresh=1.0, MaxSfrTimescale=1.0, NTask=1)
    d.update(over)
    return E.SfrParams(**d)


def dfpar(E, method, **over):
    d = dict(BH_DynFrictionMethod=method, BH_DFBoostFactor=1, BH_DFbmax=20.0, GravInternal=1.0, DensityKernelType=E.DENSITY_KERNEL_QUINTIC_SPLINE)
    d.update(over)
    return E.BhDynfricParams(**d)


def set_sfr(X, h=None, **over):
    par = sfrpar(X.E, **over)
    return X.lib.mpg_set_sfr_params(h or X.h, C.byref(par))


def set_wind(X, model):
    par = X.E.WindParams(WindModel=model)
    return X.lib.mpg_set_wind_params(X.h, C.byref(par))


def set_df(X, method, **over):
    par = dfpar(X.E, method, **over)
    return X.lib.mpg_set_bh_dynfric_params(X.h, C.byref(par))


def uvf_table(X, on):
    t = np.full((2, 2, 2), 8.0)
    return X.lib.mpg_set_uvf_table(X.h, I64(2 if on else 0), t.ctypes.data_as(C.c_void_p) if on else None, F64(1.0 if on else 0.0))


# the calls, each with keyword overrides of what it is given
def density(X, A="sph", T=True, egy=0, **over):
    a = X.arrays(X.E.SphArraysC, **over) if A == "sph" else None
    return X.lib.mpg_dev_density(X.h, None if a is None else C.byref(a), C.byref(X.T) if T else None, None, I64(0), 1, egy, 0)


def hydro(X, T=True, **over):
    a = X.arrays(X.E.SphArraysC, **over)
    return X.lib.mpg_dev_hydro_force(X.h, C.byref(a), C.byref(X.T) if T else None, None, I64(0))


def veldisp(X, par=True, **over):
    a, q = X.arrays(X.E.VelDispArraysC, **over), X.E.VelDispParams(1.0, 1.0, 0.0, 1.0)
    return X.lib.mpg_dev_find_vel_disp(X.h, C.byref(a), C.byref(X.T), C.byref(q) if par else None, None, I64(0))


def cooling(X, step=True, nactive=0, **over):
    a = X.arrays(X.E.CoolingArraysC, **over)
    return X.lib.mpg_dev_cooling(X.h, C.byref(a), C.byref(X.T), C.byref(X.step) if step else None, None, I64(nactive))


def metals(X, A=True, nactive=0, **over):
    a = X.arrays(X.E.MetalArraysC, **over)
    return X.lib.mpg_dev_metal_return(X.h, C.byref(a) if A else None, None, I64(nactive))


def blackhole(X, T=True, nactive=0, **over):
    a = X.arrays(X.E.BlackholeArraysC, **over)
    return X.lib.mpg_dev_blackhole(X.h, C.byref(a), C.byref(X.T) if T else None, None, I64(nactive))


def winds_feedback(X, A=True, stars="star", nnew=1, **over):
    a = X.arrays(X.E.WindArraysC, **over)
    return X.lib.mpg_dev_winds_and_feedback(X.h, C.byref(a) if A else None, p(X.star.data_ptr()) if stars else None, I64(nnew), F64(1.0))


def winds_subgrid(X, A=True, n=1, stellarmass=True, **over):
    a = X.arrays(X.E.WindArraysC, **over)
    return X.lib.mpg_dev_winds_subgrid(X.h, C.byref(a) if A else None, None, I64(n), p(X.B) if stellarmass else None, F64(1.0))


def winds_evolve(X, T=True, nactive=0, **over):
    a = X.arrays(X.E.WindArraysC, **over)
    return X.lib.mpg_dev_winds_evolve(X.h, C.byref(a), C.byref(X.T) if T else None, None, I64(nactive))


def starformation(X, h=None, step=True, nactive=0, **over):
    a = X.arrays(X.E.SfrColumnsC, **over)
    return X.lib.mpg_dev_cooling_and_starformation(h or X.h, C.byref(a), C.byref(X.T), C.byref(X.step) if step else None, None, I64(nactive))


def heiii_fraction(X, h="h", flag=True, n_gas_tot=4):
    return X.lib.mpg_dev_heiii_ionization_fraction(X.h if h else None, p(X.Z) if flag else None, I64(n_gas_tot), None, None)


def heiii(X, h="h", step=True, density=True, flag=True, ngroups=0, **over):
    s = X.E.HeiiiStep.from_buffer_copy(X.hstep)
    for k, v in over.items():
        setattr(s, k, v)
    return X.lib.mpg_dev_heiii_reionization(X.h if h else None, C.byref(s) if step else None, p(X.B) if density else None, p(X.B), p(X.Z) if flag else None,
                                            None, None, None, I64(ngroups), None)


def dynfric(X, T=True, nactive=0, **over):
    a = X.arrays(X.E.BhDynfricArraysC, **over)
    return X.lib.mpg_dev_blackhole_dynfric(X.h, C.byref(a), C.byref(X.T) if T else None, None, I64(nactive))


def rebuild(X, mask):
    return X.lib.mpg_dev_force_tree_rebuild_mask(X.h, mask, 0)


def keep_stats(X):
    X.snapshot = X.stats()
    return 0


# ---------------------------------------------------------------- a fresh engine: nothing bound, no tree, no parameters, no tables
setup("fresh.stats", keep_stats)
refuse("densitypar.null", NOARG, lambda X: X.lib.mpg_set_densitypar(X.h, None))
refuse("densitypar.kernel", "Density Kernel type is unknown", lambda X: X.lib.mpg_set_densitypar(X.h, C.byref(X.E.DensityParams(1.0, 2.0, 2.0, 99999., 3, 0.006))))
refuse("hydropar.null", NOARG, lambda X: X.lib.mpg_set_hydropar(X.h, None))
refuse("init_hsml.notree", "set_init_hsml: no tree", lambda X: X.lib.mpg_dev_set_init_hsml(X.h, None, F64(1.0)))
refuse("density.null", NOARG, lambda X: density(X, T=False))
refuse("density.notree", "density: no tree (force_tree_rebuild_mask first)", density)
refuse("hydro.null", NOARG, lambda X: hydro(X, T=False))
refuse("hydro.notree", "hydro_force: no tree", hydro)
refuse("dev_delaytime.null", NOARG, lambda X: X.lib.mpg_dev_set_delaytime(None, None))
refuse("delaytime.null", NOARG, lambda X: X.lib.mpg_set_delaytime(None, None))
refuse("sph_stats.null", NOARG, lambda X: X.lib.mpg_sph_get_stats(X.h, None))

refuse("veldisp.null", NOARG, lambda X: veldisp(X, par=False))
refuse("veldisp.arrays", "find_vel_disp: the arrays vel, hsml, density and vdisp are required", lambda X: veldisp(X, vdisp=None))
refuse("veldisp.built_no_tree", "no tree", lambda X: X.lib.mpg_tree_get_stats(X.h, C.byref(X.E.TreeStats())))
refuse("veldisp_stats.null", NOARG, lambda X: X.lib.mpg_veldisp_get_stats(X.h, None))
refuse("veldisp_export.null", NOARG, lambda X: X.lib.mpg_veldisp_export(None, I64(0), None, None, None, None, None, I64(0)))
refuse("veldisp_export.n", "mpg_veldisp_export: n is not the particle number of the last find_vel_disp call",
       lambda X: X.lib.mpg_veldisp_export(X.h, I64(3), None, None, None, None, None, I64(0)))

refuse("cooling_params.null", NOARG, lambda X: X.lib.mpg_set_cooling_params(X.h, None))
refuse("metal_table.null", NOARG, lambda X: X.lib.mpg_set_metal_cooling_table(None, 0, None, 0, None, 0, None, None))
refuse("cooling.null", NOARG, lambda X: cooling(X, step=False))
refuse("cooling.negative", "cooling: negative list length", lambda X: cooling(X, nactive=-1))
refuse("uvf_table.null", NOARG, lambda X: X.lib.mpg_set_uvf_table(None, I64(0), None, F64(0.0)))
refuse("uvf_offset.null", NOARG, lambda X: X.lib.mpg_set_uvf_offset(X.h, None))
refuse("uvf_offset.nan", "mpg_set_uvf_offset: offset is not finite", lambda X: X.lib.mpg_set_uvf_offset(X.h, (F64 * 3)(0.0, float("nan"), 0.0)))
refuse("uvf_zreion.null", NOARG, lambda X: X.lib.mpg_dev_uvf_zreion(X.h, I64(-1), None, None))
refuse("uvf_zreion.arrays", "mpg_dev_uvf_zreion: pos and zreion are required", lambda X: X.lib.mpg_dev_uvf_zreion(X.h, I64(1), None, p(X.B)))
refuse("uvf_export.null", NOARG, lambda X: X.lib.mpg_uvf_export(X.h, I64(0), None))
refuse("uvf_export.n", "mpg_uvf_export: n is not the particle number of the last cooling call with a UV-fluctuation table",
       lambda X: X.lib.mpg_uvf_export(X.h, I64(3), X.f64))
refuse("cooling_state.null", NOARG, lambda X: X.lib.mpg_dev_cooling_state(X.h, I64(-1), None, None, None, None, None, None, C.byref(X.step)))
refuse("cooling_state.arrays", "cooling_state: rho, u and ne are required",
       lambda X: X.lib.mpg_dev_cooling_state(X.h, I64(1), None, p(X.B), p(X.B), None, None, None, C.byref(X.step)))
refuse("cooling_stats.null", NOARG, lambda X: X.lib.mpg_cooling_get_stats(X.h, None))
refuse("cooling_export.null", NOARG, lambda X: X.lib.mpg_cooling_export(X.h, I64(0), None))
refuse("cooling_export.n", "mpg_cooling_export: n is not the particle number of the last cooling call", lambda X: X.lib.mpg_cooling_export(X.h, I64(3), X.i64))

refuse("metal_params.null", NOARG, lambda X: X.lib.mpg_set_metal_params(X.h, None))
refuse("metal_params.range", "metal parameters: MaxNgbDeviation >= 0 and MaxGasMass > 0 are required",
       lambda X: X.lib.mpg_set_metal_params(X.h, C.byref(X.E.MetalParams(1, 2.0, 0.0))))
refuse("metals.null", NOARG, lambda X: metals(X, A=False))
refuse("metals.negative", "metal_return: negative list length", lambda X: metals(X, nactive=-1))
refuse("metals.arrays", "metal_return: every array but massreturned and starvolume is required", lambda X: metals(X, metals=None))
refuse("metals.nopar", "metal_return: no parameters (mpg_set_metal_params first)", metals)
refuse("metals_stats.null", NOARG, lambda X: X.lib.mpg_metals_get_stats(X.h, None))
refuse("metals_times.null", NOARG, lambda X: X.lib.mpg_metals_get_times(X.h, None))
refuse("metals_export.null", NOARG, lambda X: X.lib.mpg_metals_export(None, I64(0), None, None, None, None, None, I64(0)))
refuse("metals_export.n", "mpg_metals_export: n is not the particle number of the last metal_return call",
       lambda X: X.lib.mpg_metals_export(X.h, I64(3), None, None, None, None, None, I64(0)))

refuse("random_table.empty", "random table: a table of at least one entry is required", lambda X: X.lib.mpg_set_random_table(X.h, X.f64, I64(0)))
refuse("bh_params.null", NOARG, lambda X: X.lib.mpg_set_blackhole_params(X.h, None))
refuse("bh_params.optthin", "blackhole: BlackHoleFeedbackMethod with BH_FEEDBACK_OPTTHIN is not carried (get_neutral_fraction_sfreff)",
       lambda X: X.lib.mpg_set_blackhole_params(X.h, C.byref(bhpar(X.E, BlackHoleFeedbackMethod=0x20))))
refuse("bh_params.tcool", "blackhole: BHFeedbackUseTcool == 2 is not carried (get_egyeff)",
       lambda X: X.lib.mpg_set_blackhole_params(X.h, C.byref(bhpar(X.E, BHFeedbackUseTcool=2))))
refuse("bh_params.units", "blackhole parameters: GravInternal, HubbleParam and the units must be positive",
       lambda X: X.lib.mpg_set_blackhole_params(X.h, C.byref(bhpar(X.E, uu_in_cgs=0.0))))
refuse("bh.null", NOARG, lambda X: blackhole(X, T=False))
refuse("bh.negative", "blackhole: negative list length", lambda X: blackhole(X, nactive=-1))
refuse("bh.nopar", "blackhole: no parameters (mpg_set_blackhole_params first)", blackhole)
refuse("bh_stats.null", NOARG, lambda X: X.lib.mpg_blackhole_get_stats(X.h, None))
refuse("bh_times.null", NOARG, lambda X: X.lib.mpg_blackhole_get_times(X.h, None))

refuse("wind_params.null", NOARG, lambda X: X.lib.mpg_set_wind_params(X.h, None))
refuse("wind_params.model", "WindModel = 0x1 is strange. This shall not happen.", lambda X: set_wind(X, X.E.WIND_SUBGRID))
refuse("winds_feedback.null", NOARG, lambda X: winds_feedback(X, A=False))
refuse("winds_feedback.negative", "winds_and_feedback: negative list length", lambda X: winds_feedback(X, nnew=-1))
refuse("winds_feedback.nopar", "winds_and_feedback: no parameters (mpg_set_wind_params first)", winds_feedback)
refuse("winds_subgrid.null", NOARG, lambda X: winds_subgrid(X, A=False))
refuse("winds_subgrid.negative", "winds_subgrid: negative list length", lambda X: winds_subgrid(X, n=-1))
refuse("winds_subgrid.nopar", "winds_subgrid: no parameters (mpg_set_wind_params first)", winds_subgrid)
refuse("winds_evolve.null", NOARG, lambda X: winds_evolve(X, T=False))
refuse("winds_evolve.negative", "winds_evolve: negative list length", lambda X: winds_evolve(X, nactive=-1))
refuse("winds_evolve.nopar", "winds_evolve: no parameters (mpg_set_wind_params first)", winds_evolve)
refuse("winds_stats.null", NOARG, lambda X: X.lib.mpg_winds_get_stats(X.h, None, None))
refuse("winds_export.null", NOARG, lambda X: X.lib.mpg_winds_export(X.h, I64(0), None, None, None))
refuse("winds_times.null", NOARG, lambda X: X.lib.mpg_winds_get_times(X.h, None))

refuse("sfr_params.null", NOARG, lambda X: X.lib.mpg_set_sfr_params(X.h, None))
refuse("sfr.null", NOARG, lambda X: starformation(X, step=False))
refuse("sfr.negative", "cooling_and_starformation: negative list length", lambda X: starformation(X, nactive=-1))
refuse("sfr.nopar", "cooling_and_starformation: no parameters (mpg_set_sfr_params first)", starformation)
refuse("sfr_result.null", NOARG, lambda X: X.lib.mpg_sfr_get_result(X.h, None))
refuse("sfr_export.negative", "mpg_sfr_export: null engine or negative capacity",
       lambda X: X.lib.mpg_sfr_export(X.h, I64(-1), None, None, None, None, I64(0), None, None))
refuse("sfr_dev_lists.null", NOARG, lambda X: X.lib.mpg_sfr_dev_lists(None, None, None, None, None))
refuse("sfr_export_rows.null", NOARG, lambda X: X.lib.mpg_sfr_export_rows(None, I64(0), None, None))
refuse("sfr_export_rows.n", "mpg_sfr_export_rows: n is not the particle number of the last call", lambda X: X.lib.mpg_sfr_export_rows(X.h, I64(3), None, None))
refuse("sfr_stats.null", NOARG, lambda X: X.lib.mpg_sfr_get_stats(X.h, None))

refuse("heiii_params.null", NOARG, lambda X: X.lib.mpg_set_heiii_params(X.h, None))
refuse("heiii_params.variance", "heiii parameters: var_bubble is a variance",
       lambda X: X.lib.mpg_set_heiii_params(X.h, C.byref(X.E.HeiiiParams(1.0, 2.0, 1.0, -1.0, 0.95))))
refuse("heiii_batch.null", NOARG, lambda X: X.lib.mpg_heiii_set_batch(None, 0))
refuse("heiii_batch.range", "mpg_heiii_set_batch: 0 (the default) or 1 .. 64 bubbles per scan", lambda X: X.lib.mpg_heiii_set_batch(X.h, 65))
refuse("heiii_fraction.null", NOARG, lambda X: heiii_fraction(X, h=None))
refuse("heiii_fraction.ngas", "heiii_ionization_fraction: n_gas_tot must be positive", lambda X: heiii_fraction(X, n_gas_tot=0))
refuse("heiii.negative", "heiii_reionization: null engine or negative group number", lambda X: heiii(X, ngroups=-1))
refuse("heiii.null", NOARG, lambda X: heiii(X, step=False))
refuse("heiii.nopar", "heiii_reionization: no parameters (mpg_set_heiii_params first)", heiii)
refuse("heiii_export.null", NOARG, lambda X: X.lib.mpg_heiii_export(X.h, I64(0), None, None, None, None, None, None))
refuse("heiii_times.null", NOARG, lambda X: X.lib.mpg_heiii_get_times(X.h, None))

refuse("df_params.null", NOARG, lambda X: X.lib.mpg_set_bh_dynfric_params(X.h, None))
refuse("df_params.method", "dynamical friction parameters: BH_DynFrictionMethod is 0, 1, 2 or 3", lambda X: set_df(X, 4))
refuse("df_params.gravity", "dynamical friction parameters: GravInternal must be positive", lambda X: set_df(X, 1, GravInternal=0.0))
refuse("df.null", NOARG, lambda X: dynfric(X, T=False))
refuse("df.negative", "blackhole_dynfric: negative list length", lambda X: dynfric(X, nactive=-1))
refuse("df.nopar", "blackhole_dynfric: no parameters (mpg_set_bh_dynfric_params first)", dynfric)
refuse("df_stats.null", NOARG, lambda X: X.lib.mpg_bh_dynfric_get_stats(X.h, None, None))
refuse("df_times.null", NOARG, lambda X: X.lib.mpg_bh_dynfric_get_times(X.h, None))
refuse("df_export.null", NOARG, lambda X: X.lib.mpg_bh_dynfric_export(None, I64(0), None, None, None))
refuse("df_export.n", "mpg_bh_dynfric_export: n is not the particle number of the last blackhole_dynfric walk",
       lambda X: X.lib.mpg_bh_dynfric_export(X.h, I64(3), None, None, None))
observe("fresh.stats_unchanged", lambda X: X.stats() == X.snapshot)

# ---------------------------------------------------------------- parameters without a random table
setup("set.heiii_params", lambda X: X.lib.mpg_set_heiii_params(X.h, C.byref(X.E.HeiiiParams(1.0, 2.0, 1.0, 0.0, 0.95))))
refuse("heiii.notable", "heiii_reionization: no random table (mpg_set_random_table first)", heiii)
setup("set.bh_params", lambda X: X.lib.mpg_set_blackhole_params(X.h, C.byref(bhpar(X.E))))
refuse("bh.notable", "blackhole: no random table (mpg_set_random_table first)", blackhole)
setup("set.sfr_params", set_sfr)
refuse("sfr.notable", "cooling_and_starformation: no random table (mpg_set_random_table first)", starformation)
setup("set.wind_params", lambda X: set_wind(X, X.E.WIND_FIXED_EFFICIENCY))
refuse("winds_feedback.nolist", "winds_and_feedback: no list of new stars", lambda X: winds_feedback(X, stars=None))
refuse("winds_feedback.notable", "winds_and_feedback: no random table (mpg_set_random_table first)", winds_feedback)
setup("set.wind_params_subgrid", lambda X: set_wind(X, X.E.WIND_FIXED_EFFICIENCY | X.E.WIND_SUBGRID))
refuse("winds_subgrid.notable", "winds_subgrid: no random table (mpg_set_random_table first)", winds_subgrid)
# (the second engine: a random table and star-formation parameters with WindOn, no wind parameters)
setup("set2.random_table", lambda X: X.lib.mpg_set_random_table(X.h2, (F64 * 16)(*[0.5] * 16), I64(16)))
setup("set2.sfr_params", lambda X: set_sfr(X, X.h2, WindOn=1))
refuse("sfr.nowindpar", "cooling_and_starformation: no wind parameters (mpg_set_wind_params first)", lambda X: starformation(X, X.h2))

# ---------------------------------------------------------------- with the random table: what the calls ask of their arguments
setup("set.random_table", lambda X: X.lib.mpg_set_random_table(X.h, (F64 * 16)(*[0.5] * 16), I64(16)))
refuse("heiii.ngas", "heiii_reionization: n_gas_tot must be positive", lambda X: heiii(X, n_gas_tot=0))
refuse("heiii.atime", "heiii_reionization: atime and uu_in_cgs must be positive", lambda X: heiii(X, uu_in_cgs=0.0))
setup("set.uvf_table", lambda X: uvf_table(X, True))
refuse("sfr.table_without_setting", "cooling_and_starformation: the engine holds a UV-fluctuation table but UVFluctuationOn is 0 (mpg_set_sfr_params)", starformation)
refuse("uvf_zreion.nan", "mpg_dev_uvf_zreion: 1 point(s) have a coordinate that is not finite or lies 2^31 cells or more from the table's origin; their zreion is NaN",
       lambda X: X.lib.mpg_dev_uvf_zreion(X.h, I64(1), p(X.nan.data_ptr()), p(X.nan.data_ptr() + 24)))
setup("set.sfr_params_uvf", lambda X: set_sfr(X, UVFluctuationOn=1))
setup("unset.uvf_table", lambda X: uvf_table(X, False))
refuse("sfr.setting_without_table", "cooling_and_starformation: UVFluctuationOn is set but the engine holds no UV-fluctuation table (mpg_set_uvf_table)", starformation)

# ---------------------------------------------------------------- 8 particles without a type column, then with one
setup("bind.untyped", lambda X: X.bind(X.h, None))
refuse("heiii_fraction.notype", "heiii_ionization_fraction: the bound particles have no type column", heiii_fraction)
refuse("heiii.notype", "heiii_reionization: the bound particles have no type column", heiii)
setup("bind.typed", lambda X: X.bind(X.h, X.type))
refuse("heiii_fraction.flag", "heiii_ionization_fraction: the array heiii_ionized is required", lambda X: heiii_fraction(X, flag=False))
refuse("heiii.flag", "heiii_reionization: the array heiii_ionized is required", lambda X: heiii(X, flag=False))
refuse("heiii.arrays", "heiii_reionization: the arrays density and entropy are required", lambda X: heiii(X, density=False))
refuse("heiii.groups", "heiii_reionization: the group columns mass, cm and minid are required", lambda X: heiii(X, ngroups=2))
refuse("cooling.arrays", "cooling: the arrays density, entropy, ne and sfr are required", lambda X: cooling(X, ne=None))
refuse("bh.arrays", "blackhole: the array mdot is required", lambda X: blackhole(X, mdot=None))
setup("set.sfr_params_h2", lambda X: set_sfr(X, StarformationCriterion=X.E.SFR_CRITERION_MOLECULAR_H2))
refuse("sfr.columns", "cooling_and_starformation: the columns id, density, entropy, ne, sfr and metallicity are required", lambda X: starformation(X, metallicity=None))
refuse("sfr.h2", "cooling_and_starformation: SFR_CRITERION_MOLECULAR_H2 needs the columns hsml and gradrho_mag", lambda X: starformation(X, gradrho_mag=None))
setup("set.sfr_params_selfgravity", lambda X: set_sfr(X, StarformationCriterion=X.E.SFR_CRITERION_SELFGRAVITY))
refuse("sfr.selfgravity", "cooling_and_starformation: SFR_CRITERION_SELFGRAVITY needs the columns divvel and curlvel", lambda X: starformation(X, curlvel=None))
setup("set.sfr_params_wind", lambda X: set_sfr(X, WindOn=1))
refuse("sfr.subgrid", "cooling_and_starformation: WIND_SUBGRID needs the columns vdisp, vel, delaytime and stellarmass", lambda X: starformation(X, stellarmass=None))
refuse("winds_subgrid.arrays", "winds_subgrid: the stellar masses and the arrays id, vdisp, density, vel, entropy and delaytime are required",
       lambda X: winds_subgrid(X, stellarmass=False))
refuse("winds_evolve.arrays", "winds_evolve: the arrays density, tb_hydro and delaytime are required", lambda X: winds_evolve(X, tb_hydro=None))
setup("set.wind_params_stars", lambda X: set_wind(X, X.E.WIND_FIXED_EFFICIENCY))
refuse("winds_feedback.arrays", "winds_and_feedback: the arrays id, hsml, vdisp, density, vel, entropy and delaytime are required", lambda X: winds_feedback(X, id=None))
setup("set.df_params_1", lambda X: set_df(X, 1))
refuse("df.arrays", "blackhole_dynfric: the arrays vel, hsml, potential, jumptominpot, minpot, minpotpos and minpotvel are required", lambda X: dynfric(X, minpot=None))
refuse("df.friction_arrays", "blackhole_dynfric: dynamical friction needs the arrays gacc, gpm, tb_grav, bh_mass, df_density, df_vel, df_rmsvel and dfaccel",
       lambda X: dynfric(X, dfaccel=None))
setup("set.df_params_3", lambda X: set_df(X, 3))
refuse("df.method3_arrays", "blackhole_dynfric: BH_DynFrictionMethod 3 needs the arrays hydroacc and tb_hydro", lambda X: dynfric(X, hydroacc=None))
setup("set.metal_params", lambda X: X.lib.mpg_set_metal_params(X.h, C.byref(X.E.MetalParams(1, 2.0, 1.0))))
refuse("metals.notree", "metal_return: the current tree does not contain the gas (GASMASK)", metals)
refuse("bh.notree", "blackhole: the current tree does not contain the gas (GASMASK)", blackhole)
refuse("winds_feedback.notree", "winds_and_feedback: the current tree does not contain the gas (GASMASK)", winds_feedback)

# ---------------------------------------------------------------- trees that lack what a call needs
setup("tree.dm", lambda X: rebuild(X, 2))
refuse("density.nogas", "density: the tree does not contain gas (GASMASK)", density)
refuse("metals.nogas", "metal_return: the current tree does not contain the gas (GASMASK)", metals)
refuse("bh.nogas", "blackhole: the current tree does not contain the gas (GASMASK)", blackhole)
refuse("winds_feedback.nogas", "winds_and_feedback: the current tree does not contain the gas (GASMASK)", winds_feedback)
setup("tree.gas", lambda X: rebuild(X, 1))
refuse("bh.noblackholes", "blackhole: the current tree does not contain the black holes (BHMASK)", blackhole)
refuse("init_hsml.arrays_null", "null SPH arrays", lambda X: X.lib.mpg_dev_set_init_hsml(X.h, None, F64(1.0)))
refuse("density.arrays_null", "null SPH arrays", lambda X: density(X, A=None))
refuse("density.arrays", "SPH arrays: hsml, vel, entropy, density, dhsmlegyfac, divvel, curlvel are required", lambda X: density(X, divvel=None))
refuse("density.egy", "density: DoEgyDensity needs the egywtdensity array", lambda X: density(X, egy=1, egywtdensity=None))
refuse("hydro.outputs", "hydro_force: output arrays are required", lambda X: hydro(X, maxsignalvel=None))
refuse("hydro.egy", "hydro_force: pressure-entropy SPH needs egywtdensity", lambda X: hydro(X, egywtdensity=None))
setup("tree.gas_and_blackholes", lambda X: rebuild(X, 33))
refuse("bh.nohmax", "blackhole: symmetric search on a tree without hmax (force_tree_calc_moments first)", blackhole)
setup("tree.hmax", lambda X: X.lib.mpg_dev_force_update_hmax(X.h, p(X.B)))
refuse("bh.nosoftening", "blackhole: no force softening", blackhole)

IDS = [s[0] for s in STEPS]
assert len(set(IDS)) == len(IDS)


@pytest.fixture(scope="module")
def results(pkg):
    """the whole script, run once in its order: id -> (return value, text of mpg_last_error)"""
    X = Context(pkg)
    X.lib.mpg_last_error.restype = C.c_char_p
    out = {}
    for name, kind, want, fn in STEPS:
        rc = fn(X)
        out[name] = (rc, X.lib.mpg_last_error().decode())
    X.eng.synchronize()
    X.close()
    return out


@pytest.mark.parametrize("name,kind,want", [s[:3] for s in STEPS], ids=IDS)
def test_refusal(results, name, kind, want):
    rc, text = results[name]
    print(name, rc, repr(text))
    if kind == "refuse":
        assert rc != 0, "%s was not refused" % name
        assert text.rsplit(" [", 1)[0] == want
    elif kind == "setup":
        assert rc == 0, text
    else:
        assert rc is True

