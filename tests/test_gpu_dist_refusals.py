"""The refusals of the multi-rank layer's entry points (mpg_dist_*, csrc/dist*.hip) that arguments and call order can reach on ONE rank with
LocalComm (no callbacks, hence no collective), pinned by their TEXT: mpg_last_error() up to the last " [" (the file:line suffix) against a
literal written from the source.  Calls that fail two checks at once pin WHICH one reports: every check stays before the first side effect
and in its place among the other checks.  One rank only, never under a launcher: a refusal on one rank of several leaves the others waiting.

One engine (Nmesh 16, box 8), one mpg_dist, 64 particles (16 of them gas), driven through a script whose order matters:
a fresh handle (nulls, "mpg_dist_set_domain first", the ordering checks of the walk, the SPH loops and the host forms, the planes, the domain
calls), then with a domain (too many particles, the mesh-box mismatch, the FOF parameters), then with the local tree of
mpg_dist_force_tree_full (the active counts, "an active index is not an own particle", "the active list holds duplicates"), then after a
density loop ("the local tree was replaced", the active lists of the SPH loops).  Every refusal is a host-side check, and all but four fail
before the call has launched anything.  The four: the two active-list verdicts of the walk and the two of the SPH loops come from
k_flag_list, which tests an index against [0, n) BEFORE it uses it (the bad index is never dereferenced; every array the calls get is a
real one of 64 rows).

Not driven, because nothing reaches them on one rank without callbacks: the "mpg_comm: ... callback missing" / "callback failed" /
"bind_stream failed" checks; "Nmesh must be a multiple of the number of ranks" and "gravpm_init_periodic first" of the slab set-up (the
mesh-box check reports first); "more than 2^31 rows in one exchange"; the three deferred checks of the tree (cells above the decomposition
level, own particles missing: they need a particle set that fails them); the hybrid-neutrino deposit mask; "corrupt Peano-Hilbert key"
(every digit has an octant); "the largest smoothing length exceeds the domain margin" (needs a density loop that ends so); "the labels do
not converge"; "TopNodeAllocFactor unreasonably large", "too many TopLeaves for the cost pass" and the send-count invariant of
domain_exchange; "the active set is not small"; the massive-neutrino correction of the planes on several ranks; mpg_dist_density on a
table whose tree call is missing is driven, its "bad NumActiveParticle" twin of the host walk as well."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

I64, F64 = C.c_int64, C.c_double
NOARG = "null argument"
NODOMAIN = "mpg_dist: mpg_dist_set_domain first"
TOOMANY = "mpg_dist: too many particles on one rank"
MESHBOX = "mpg_dist: BoxSize of the mesh differs from the domain's"
WALK_FIRST = "mpg_dist_dev_grav_short_tree: mpg_dist_dev_force_tree_build first"
WALK_REPLACED = ("mpg_dist_dev_grav_short_tree: the local tree was replaced since mpg_dist_dev_force_tree_build (the density loop "
                 "builds a gas tree, FOF a tree of the primary types): build the gravity tree again")
WALK_COUNT = "mpg_dist_dev_grav_short_tree_active: bad number of active particles"
DENSITY_FIRST = "mpg_dist_dev_density: mpg_dist_dev_force_tree_build of this particle set first"
HYDRO_FIRST = "mpg_dist_dev_hydro_force: mpg_dist_dev_density of this particle set first"
N, NMESH, BOX, MARGIN = 64, 16, 8.0, 3.5
STEPS = []   # (id, kind, expected text or None, function of the context)


def refuse(name, want, fn):
    STEPS.append((name, "refuse", want, fn))


def setup(name, fn):
    STEPS.append((name, "setup", None, fn))


def p(x):
    return None if x is None else C.c_void_p(x)


class Context:
    def __init__(self, pkg):
        import torch
        self.pkg, self.E, self.D = pkg, pkg.engine, pkg.dist
        self.eng = eng = pkg.Engine(0)
        self.lib = eng.lib
        eng.gravshort_fill_ntab(0, 1.5)
        eng.set_gravshort_treepar()
        eng.gravshort_set_softenings(BOX / 4)
        eng.set_densitypar(1.0, 2.0, 2.0, 99999., pkg.engine.DENSITY_KERNEL_QUINTIC_SPLINE, 0.006)
        eng.set_hydropar(0, 100.0, 0.75)
        self.mesh(BOX)
        self.df = self.D.DistForce(eng, self.D.LocalComm())
        self.h = self.df.h
        rng = np.random.default_rng(11)
        self.hpos, self.hmass = rng.random((N, 3)) * BOX, np.ones(N, np.float32)
        self.htyp = np.ones(N, np.uint8)
        self.htyp[::4] = 0
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
        f8 = dict(dtype=torch.float64, device="cuda")
        self.pos, self.mass, self.typ = up(self.hpos), up(self.hmass), up(self.htyp)
        self.ones = torch.ones(512, **f8)
        self.B = self.ones.data_ptr()
        z1 = lambda: torch.zeros(N, **f8)
        self.sph = dict(hsml=torch.full((N,), 2.0, **f8), dthsml=z1(), vel=torch.zeros(N, 3, **f8), entropy=torch.ones(N, **f8), density=z1(),
                        egywtdensity=z1(), dhsmlegyfac=z1(), divvel=z1(), curlvel=z1(), hydroacc_out=torch.zeros(N, 3, **f8), dtentropy_out=z1(),
                        maxsignalvel=z1())
        self.lists = {k: up(np.array(v, np.int32)) for k, v in dict(ok=[0, 4, 8], outside=[0, 4, N], twice=[0, 0, 4]).items()}
        self.T = pkg.SphTimes()
        self.T.atime, self.T.hubble = 0.5, 0.3
        for i in range(47):
            self.T.dloga_bin[i] = 0.01
        self.P = pkg.make_particles(self.hpos, self.hmass, type=self.htyp)
        self.hsph = {k: np.ascontiguousarray(v.cpu().numpy()) for k, v in self.sph.items()}
        self.store = np.zeros((N, 3))
        self.hact = {k: np.array(v, np.int32) for k, v in dict(ok=[0, 4], outside=[0, N]).items()}
        self.root = (self.D.TopNode * 1)(self.D.TopNode(0, 63, -1, -1, 0, N, N))     # one TopNode: the whole box, a leaf
        self.fof = self.E.FofParams(2, 1 + 16 + 32, 0.2, 8)
        self.planes_out = torch.zeros(3 * 16 * 16, **f8)
        self.npart = np.zeros(3, np.int64)
        torch.cuda.synchronize()

    def mesh(self, box):
        self.eng.gravpm_init_periodic(box, 1.5, NMESH, 43.0071)
        return 0

    def close(self):
        self.df.close()
        self.eng.close()

    def view(self, **over):
        v = self.eng._view(self.P)
        for k, val in over.items():
            setattr(v, k, val)
        return v

    def arrays(self, **over):
        """mpg_sph_arrays with every member on the buffer of ones, but those named (None: NULL)"""
        a = self.E.SphArraysC()
        for k, _ in self.E.SphArraysC._fields_:
            setattr(a, k, over.get(k, self.B))
        return a

    def ok(self, fn):
        try:
            fn()
            return 0
        except self.E.EngineError:
            return 1


# the calls, each with keyword overrides of what it is given
def set_domain(X, d="h", nodes=True, box=BOX, margin=MARGIN, La=0, task=0, leaves=1, leaf=0):
    X.root[0].Leaf = leaf
    return X.lib.mpg_dist_set_domain(X.h if d else None, F64(box), X.root if nodes else None, 1, (C.c_int * 1)(task), leaves, F64(margin), La)


def pm(X, n=N, gravpm=True, pos=True):
    return X.lib.mpg_dist_dev_gravpm_force(X.h, I64(n), p(X.pos.data_ptr() if pos else None), p(X.mass.data_ptr()), p(X.B if gravpm else None), None)


def tree(X, n=N, pos=True):
    return X.lib.mpg_dist_dev_force_tree_build(X.h, I64(n), p(X.pos.data_ptr() if pos else None), p(X.mass.data_ptr()))


def step(X, n=N, accel=True, gravpm=True):
    return X.lib.mpg_dist_gravity_step(X.h, I64(n), p(X.pos.data_ptr()), p(X.mass.data_ptr()), None, None, p(X.B if accel else None),
                                       p(X.B if gravpm else None), None, F64(0.0))


def walk(X, accel=True, active=None, nactive=None):
    a = None if active is None else X.lists[active]
    return X.lib.mpg_dist_dev_grav_short_tree_active(X.h, p(None if a is None else a.data_ptr()), I64((0 if a is None else len(a)) if nactive is None else nactive),
                                                     None, None, None, p(X.B if accel else None), None, F64(0.0))


def density(X, n=N, active=None, nactive=None, real=False, **over):
    a = X.eng._sph_arrays(X.sph) if real else X.arrays(**over)
    l = None if active is None else X.lists[active]
    return X.lib.mpg_dist_dev_density_active(X.h, I64(n), p(X.typ.data_ptr()), C.byref(a), C.byref(X.T), p(None if l is None else l.data_ptr()),
                                             I64((0 if l is None else len(l)) if nactive is None else nactive), 0, 0)


def hydro(X, n=N, active=None, real=False, **over):
    a = X.eng._sph_arrays(X.sph) if real else X.arrays(**over)
    l = None if active is None else X.lists[active]
    return X.lib.mpg_dist_dev_hydro_force_active(X.h, I64(n), C.byref(a), C.byref(X.T), p(None if l is None else l.data_ptr()), I64(0 if l is None else len(l)))


def fof(X, par=True, ids=True, **over):
    q = X.E.FofParams.from_buffer_copy(X.fof)
    for k, v in over.items():
        setattr(q, k, v)
    X.lib.mpg_dist_dev_fof_fof.argtypes = [C.c_void_p, C.c_int64] + [C.c_void_p] * 7 + [C.POINTER(C.c_int64)] * 2
    return X.lib.mpg_dist_dev_fof_fof(X.h, I64(N), p(X.pos.data_ptr()), p(X.mass.data_ptr()), None, p(X.B if ids else None), None,
                                      C.cast(C.pointer(q), C.c_void_p) if par else None, None, None, None)


def powerspectrum(X, kk=True):
    out = (F64 * NMESH)()
    return X.lib.mpg_dist_gravpm_get_powerspectrum(X.h, F64(BOX), out if kk else None, (F64 * NMESH)(), (I64 * NMESH)(), C.byref(C.c_int(0)))


def active_tree(X, n=4, pos=True, d="h"):
    return X.lib.mpg_dist_dev_grav_short_tree_active_tree(X.h if d else None, I64(n), p(X.pos.data_ptr() if pos else None), p(X.mass.data_ptr()), None, p(X.B),
                                                          None, F64(0.0))


def planes(X, par=True, pos=True, box=BOX, out=True, **over):
    pp, keep, nc, nn, thunk = X.eng._plane_params(box if box > 0 else BOX, 16, [0, 1, 2], atime=0.5, comoving_distance=2.5e5, HubbleParam=0.7, omega_source=0.27)
    for k, v in over.items():
        setattr(pp, k, v)
    return X.lib.mpg_dist_potential_planes(X.h, I64(N), p(X.pos.data_ptr() if pos else None), p(X.mass.data_ptr()), None, None, F64(box),
                                           C.byref(pp) if par else None, p(X.planes_out.data_ptr() if out else None), X.npart.ctypes.data_as(C.c_void_p))


def decompose(X, n=N):
    X.lib.mpg_dist_domain_decompose.argtypes = None
    return X.lib.mpg_dist_domain_decompose(X.h, I64(n), p(X.pos.data_ptr()), None, F64(BOX), 4, 1, None, None, None)


def exchange(X, n=N, ncols=1):
    X.lib.mpg_dist_domain_exchange.argtypes = None
    return X.lib.mpg_dist_domain_exchange(X.h, I64(n), ncols, (C.c_void_p * 1)(X.pos.data_ptr()), (C.c_int * 1)(24), C.byref(I64(0)), (C.c_void_p * 1)())


def host_walk(X, v, active=None, nactive=None):
    a = None if active is None else X.hact[active]
    return X.lib.mpg_dist_grav_short_tree_active(X.h, None if v is None else C.byref(v), None if a is None else a.ctypes.data_as(C.c_void_p),
                                                 I64((0 if a is None else len(a)) if nactive is None else nactive), None, F64(0.0))


def host_active_tree(X, v, active="ok", nactive=None, store=True):
    a = None if active is None else X.hact[active]
    return X.lib.mpg_dist_grav_short_tree_active_tree(X.h, C.byref(v), None if a is None else a.ctypes.data_as(C.c_void_p),
                                                      I64((0 if a is None else len(a)) if nactive is None else nactive),
                                                      X.store.ctypes.data_as(C.c_void_p) if store else None, F64(0.0))


def host_sph(X, fn, v, T=True, **extra):
    a = X.eng._sph_host_arrays(X.hsph)
    return fn(X.h, None if v is None else C.byref(v), C.byref(a), C.byref(X.T) if T else None, None, I64(0), *extra.get("tail", ()))


# ---------------------------------------------------------------- a fresh handle: no domain, no tree, no density loop, no decomposition
refuse("create.null", NOARG, lambda X: X.lib.mpg_dist_create(None, X.eng.h, C.byref(X.D.LocalComm().struct)))
refuse("create.ntask", "mpg_dist_create: bad ThisTask / NTask",
       lambda X: X.lib.mpg_dist_create(C.byref(C.c_void_p()), X.eng.h, C.byref(X.D.MpgComm(None, 0, 65, 0, X.D.ALLREDUCE_FN(), X.D.A2A_I64_FN(), X.D.A2AV_FN()))))
refuse("set_domain.null", NOARG, lambda X: set_domain(X, nodes=False))
refuse("set_domain.null_and_box", NOARG, lambda X: set_domain(X, nodes=False, box=0.0))
refuse("set_domain.box", "mpg_dist_set_domain: BoxSize and margin must be positive", lambda X: set_domain(X, box=0.0))
refuse("set_domain.box_and_narrow", "mpg_dist_set_domain: BoxSize and margin must be positive", lambda X: set_domain(X, margin=-1.0, La=3))
refuse("set_domain.narrow", "mpg_dist_set_domain: cells of level La are narrower than the margin", lambda X: set_domain(X, La=3))
refuse("set_domain.leaf", "mpg_dist_set_domain: TopNode without a valid Leaf", lambda X: set_domain(X, leaf=1))
refuse("set_domain.task", "mpg_dist_set_domain: Task of a TopLeaf out of range", lambda X: set_domain(X, task=1))
refuse("set_domain.leaves", "mpg_dist_set_domain: the TopNodes do not hold NTopLeaves leaves", lambda X: set_domain(X, leaves=2))
refuse("set_garbage.null", NOARG, lambda X: X.lib.mpg_dist_dev_set_garbage(X.h, I64(-1), None))
refuse("set_types.null", NOARG, lambda X: X.lib.mpg_dist_dev_set_types(X.h, I64(-1), None))
refuse("set_sph_options.null", NOARG, lambda X: X.lib.mpg_dist_set_sph_options(None, 0))
refuse("set_maxpart.null", NOARG, lambda X: X.lib.mpg_dist_domain_set_maxpart(X.h, I64(-1)))
refuse("get_stats.null", NOARG, lambda X: X.lib.mpg_dist_get_stats(X.h, None))
refuse("get_times.null", NOARG, lambda X: X.lib.mpg_dist_get_times(X.h, None))
refuse("fof_groups.null", NOARG, lambda X: X.lib.mpg_dist_fof_groups(X.h, None))

refuse("pm.null", NOARG, lambda X: pm(X, gravpm=False))
refuse("pm.null_positions", NOARG, lambda X: pm(X, pos=False))
refuse("pm.nodomain", NODOMAIN, pm)
refuse("pm.nodomain_and_toomany", NODOMAIN, lambda X: pm(X, n=1 << 31))
refuse("tree.null", NOARG, lambda X: tree(X, pos=False))
refuse("tree.nodomain", NODOMAIN, tree)
refuse("step.null", NOARG, lambda X: step(X, accel=False))
refuse("step.null_gravpm", NOARG, lambda X: step(X, gravpm=False))
refuse("step.nodomain", NODOMAIN, step)
refuse("walk.null", NOARG, lambda X: walk(X, accel=False))
refuse("walk.notree", WALK_FIRST, walk)
refuse("walk.notree_and_count", WALK_FIRST, lambda X: walk(X, active="ok", nactive=-1))
refuse("density.null", NOARG, lambda X: density(X, divvel=None))
refuse("density.notree", DENSITY_FIRST, density)
refuse("hydro.null", NOARG, lambda X: hydro(X, maxsignalvel=None))
refuse("hydro.null_and_nodensity", NOARG, lambda X: hydro(X, hydroacc_out=None))
refuse("hydro.nodensity", HYDRO_FIRST, hydro)
refuse("fof.null", "mpg_dist_dev_fof_fof: null argument", lambda X: fof(X, par=False))
refuse("fof.null_ids", "mpg_dist_dev_fof_fof: null argument", lambda X: fof(X, ids=False))
refuse("fof.nodomain", "mpg_dist_dev_fof_fof: mpg_dist_set_domain first", fof)
refuse("fof.nodomain_and_parameters", "mpg_dist_dev_fof_fof: mpg_dist_set_domain first", lambda X: fof(X, FOFHaloMinLength=0))
refuse("powerspectrum.null", NOARG, lambda X: powerspectrum(X, kk=False))
refuse("powerspectrum.nostep", "power spectrum: no PM step has been run with the measurement on", powerspectrum)
refuse("active_tree.null", NOARG, lambda X: active_tree(X, pos=False))
refuse("active_tree.nodomain", "mpg_dist: mpg_dist_set_domain first (the box size)", active_tree)
refuse("planes.null", NOARG, lambda X: planes(X, par=False))
refuse("planes.positions", "mpg_dist_potential_planes: null positions", lambda X: planes(X, pos=False))
refuse("planes.positions_and_box", "mpg_dist_potential_planes: null positions", lambda X: planes(X, pos=False, box=0.0))
refuse("planes.box", "mpg_dist_potential_planes: BoxSize must be positive", lambda X: planes(X, box=0.0))
refuse("planes.resolution", "potential planes: Resolution must be at least 1", lambda X: planes(X, Resolution=0))
refuse("planes.resolution_and_omega", "potential planes: Resolution must be at least 1", lambda X: planes(X, Resolution=0, omega_source=0.0))
refuse("planes.omega", "potential planes: non-positive particle matter density (omega_source <= 0)", lambda X: planes(X, omega_source=0.0))
refuse("planes.output", "potential planes: null output", lambda X: planes(X, out=False))

refuse("decompose.argument", "mpg_dist_domain_decompose: bad argument", lambda X: decompose(X, n=-1))
refuse("maintain.none", "mpg_dist_domain_maintain: no decomposition / bad argument",
       lambda X: X.lib.mpg_dist_domain_maintain(X.h, I64(N), p(X.pos.data_ptr()), None, F64(BOX), None))
refuse("domain_get.none", "mpg_dist_domain_get: no decomposition", lambda X: X.lib.mpg_dist_domain_get(X.h, None, None, None, None, None))
refuse("exchange.argument", "mpg_dist_domain_exchange: bad argument", lambda X: exchange(X, ncols=17))
refuse("exchange.argument_and_none", "mpg_dist_domain_exchange: bad argument", lambda X: exchange(X, n=N + 1, ncols=0))
refuse("exchange.none", "mpg_dist_domain_exchange: mpg_dist_domain_decompose of this particle set first", exchange)

refuse("host_pm.null", NOARG, lambda X: X.lib.mpg_dist_gravpm_force(X.h, None))
refuse("host_pm.gravpm", "particle view needs GravPM", lambda X: X.lib.mpg_dist_gravpm_force(X.h, C.byref(X.view(off_gravpm=-1))))
refuse("host_pm.gravpm_and_positions", "particle view needs GravPM", lambda X: X.lib.mpg_dist_gravpm_force(X.h, C.byref(X.view(off_gravpm=-1, off_pos=-1))))
refuse("host_pm.view", "null particle view", lambda X: X.lib.mpg_dist_gravpm_force(X.h, C.byref(X.view(base=None))))
refuse("host_pm.positions", "particle view needs Pos and Mass", lambda X: X.lib.mpg_dist_gravpm_force(X.h, C.byref(X.view(off_mass=-1))))
refuse("host_tree.null", NOARG, lambda X: X.lib.mpg_dist_force_tree_full(X.h, None))
refuse("host_tree.positions", "particle view needs Pos and Mass", lambda X: X.lib.mpg_dist_force_tree_full(X.h, C.byref(X.view(off_pos=-1))))
refuse("host_walk.null", NOARG, lambda X: host_walk(X, None))
refuse("host_walk.fields", "particle view needs FullTreeGravAccel and GravPM", lambda X: host_walk(X, X.view(off_accel=-1)))
refuse("host_walk.fields_and_notree", "particle view needs FullTreeGravAccel and GravPM", lambda X: host_walk(X, X.view(off_gravpm=-1)))
refuse("host_walk.notree", "mpg_dist_grav_short_tree: call mpg_dist_force_tree_full on this table first", lambda X: host_walk(X, X.view()))
refuse("host_walk.notree_and_count", "mpg_dist_grav_short_tree: call mpg_dist_force_tree_full on this table first",
       lambda X: host_walk(X, X.view(), active="ok", nactive=N + 1))
refuse("host_density.null", NOARG, lambda X: host_sph(X, X.lib.mpg_dist_density, X.view(), T=False, tail=(0, 0)))
refuse("host_density.notree", "mpg_dist_density: call mpg_dist_force_tree_full on this table first",
       lambda X: host_sph(X, X.lib.mpg_dist_density, X.view(), tail=(0, 0)))
refuse("host_hydro.null", NOARG, lambda X: host_sph(X, X.lib.mpg_dist_hydro_force, None))
refuse("host_hydro.nodensity", "mpg_dist_hydro_force: call mpg_dist_density on this table first", lambda X: host_sph(X, X.lib.mpg_dist_hydro_force, X.view()))
refuse("host_active_tree.null", "null argument (the walk on an active-only tree returns its result in AccelStore)", lambda X: host_active_tree(X, X.view(), store=False))
refuse("host_active_tree.fields", "particle view needs Pos, Mass, FullTreeGravAccel, GravPM", lambda X: host_active_tree(X, X.view(off_accel=-1)))
refuse("host_active_tree.fields_and_count", "particle view needs Pos, Mass, FullTreeGravAccel, GravPM", lambda X: host_active_tree(X, X.view(off_pos=-1), nactive=-1))
refuse("host_active_tree.count", "bad NumActiveParticle", lambda X: host_active_tree(X, X.view(), nactive=N + 1))
refuse("host_active_tree.index", "ActiveParticle index out of range", lambda X: host_active_tree(X, X.view(), active="outside"))

# ---------------------------------------------------------------- with a domain (one TopLeaf, the whole box)
setup("set_domain", set_domain)
refuse("pm.toomany", TOOMANY, lambda X: pm(X, n=1 << 31))
refuse("tree.toomany", TOOMANY, lambda X: tree(X, n=1 << 31))
refuse("step.toomany", TOOMANY, lambda X: step(X, n=1 << 31))
setup("mesh.other_box", lambda X: X.mesh(4.0))
refuse("pm.meshbox", MESHBOX, pm)
refuse("step.meshbox", MESHBOX, step)
refuse("pm.toomany_and_meshbox", TOOMANY, lambda X: pm(X, n=1 << 31))
refuse("step.toomany_and_meshbox", TOOMANY, lambda X: step(X, n=1 << 31))
refuse("step.null_and_meshbox", NOARG, lambda X: step(X, accel=False))
setup("mesh.box", lambda X: X.mesh(BOX))
refuse("fof.parameters", "fof_fof: bad parameters", lambda X: fof(X, FOFHaloMinLength=0))
refuse("fof.parameters_and_disjoint", "fof_fof: bad parameters", lambda X: fof(X, FOFHaloComovingLinkingLength=0.0, FOFSecondaryLinkTypes=2))
refuse("fof.disjoint", "fof_fof: primary and secondary link types must be disjoint", lambda X: fof(X, FOFSecondaryLinkTypes=2))
refuse("fof.disjoint_and_margin", "fof_fof: primary and secondary link types must be disjoint", lambda X: fof(X, FOFSecondaryLinkTypes=2, FOFHaloComovingLinkingLength=4.0))
refuse("fof.margin", "mpg_dist_dev_fof_fof: the domain margin must cover the linking length (6.4 linking lengths with secondary link types)",
       lambda X: fof(X, FOFHaloComovingLinkingLength=1.0))
refuse("walk.notree_with_domain", WALK_FIRST, walk)

# ---------------------------------------------------------------- with the local tree of the table (host form: it stages the table too)
setup("host_force_tree_full", lambda X: X.ok(lambda: X.df.host_force_tree_full(X.P)))
refuse("walk.count_negative", WALK_COUNT, lambda X: walk(X, active="ok", nactive=-1))
refuse("walk.count_above", WALK_COUNT, lambda X: walk(X, active="ok", nactive=N + 1))
refuse("walk.null_and_count", NOARG, lambda X: walk(X, accel=False, active="ok", nactive=-1))
refuse("walk.index", "mpg_dist_dev_grav_short_tree_active: an active index is not an own particle", lambda X: walk(X, active="outside"))
refuse("walk.duplicates", "mpg_dist_dev_grav_short_tree_active: the active list holds duplicates", lambda X: walk(X, active="twice"))
refuse("density.other_n", DENSITY_FIRST, lambda X: density(X, n=N - 1))
refuse("host_walk.count", "bad NumActiveParticle", lambda X: host_walk(X, X.view(), active="ok", nactive=N + 1))

# ---------------------------------------------------------------- after a density loop: the gas tree has replaced the gravity tree
setup("density", lambda X: density(X, real=True))
refuse("walk.replaced", WALK_REPLACED, walk)
refuse("walk.replaced_and_count", WALK_REPLACED, lambda X: walk(X, active="ok", nactive=-1))
refuse("hydro.other_n", HYDRO_FIRST, lambda X: hydro(X, n=N - 1))
refuse("density.count", "mpg_dist SPH loop: bad number of active particles", lambda X: density(X, real=True, active="ok", nactive=N + 1))
refuse("density.index", "mpg_dist SPH loop: an active index is not an own particle", lambda X: density(X, real=True, active="outside"))
setup("density.again", lambda X: density(X, real=True))
refuse("hydro.index", "mpg_dist SPH loop: an active index is not an own particle", lambda X: hydro(X, real=True, active="outside"))

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
    else:
        assert rc == 0, text
