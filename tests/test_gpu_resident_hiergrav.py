"""The resident integrator on the branch of run.c WITH SplitGravityTimestepsOn (the default): the hydro-only half kick
(mpg_dev_apply_hydro_half_kick / mpg_resident_apply_hydro_half_kick, timestep.c:930-968) and the resident forms of the hierarchical
gravity level loop (mpg_resident_hierarchical_gravity_accelerations / _and_timesteps, timestep.c:293-599), driven in run.c's own order
against the CPU restatements (oracle/hiergrav_oracle.py for gravity and the time bins, the oracle's SPH loops, and the NumPy
restatement of apply_hydro_half_kick below)."""
import numpy as np
import pytest

from oracle import oracle as O
from oracle import hiergrav_oracle as H
from test_gpu_gravity import G
from test_gpu_hiergrav import to_struct, from_struct, update_kick_times
from test_gpu_timestep import _gas_run_setup, make_times_like

pytestmark = pytest.mark.gpu

TIMEBINS = H.TIMEBINS


def dev(torch, a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def hydro_half_kick(vel, entropy, typ, tb_hydro, hydroaccel, dtentropy, K, active=None, flags=None):
    """apply_hydro_half_kick (timestep.c:930-968) with do_hydro_kick (timestep.c:1004-1036), gas part, in place: for the listed gas
    particles that are not garbage / swallowed, Vel += HydroAccel * hydrokick[bin], the velocity limit MaxGasVel * atime, Entropy +=
    DtEntropy * dt_entr[bin] - the same IEEE operations in the same order (the factor of an inactive bin is 0 and is applied all the same)."""
    idx = np.arange(len(vel)) if active is None else np.asarray(active, np.int64)
    keep = typ[idx] == 0
    if flags is not None:
        keep &= (flags[idx] & 3) == 0
    i = idx[keep]
    b = tb_hydro[i].astype(np.int64)
    hk = np.asarray(K.hydrokick)[b]
    de = np.asarray(K.dt_entr)[b]
    v = vel[i].copy()
    for j in range(3):
        v[:, j] = v[:, j] + hydroaccel[i, j] * hk
    vv = np.sqrt(((0.0 + v[:, 0] * v[:, 0]) + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2])
    lim = (vv > 0) & (vv / K.atime > K.MaxGasVel)
    for j in range(3):
        v[lim, j] = v[lim, j] * (K.MaxGasVel * K.atime / vv[lim])
    vel[i] = v
    entropy[i] = entropy[i] + dtentropy[i] * de


def kick_factors(KF, times, atime, MaxGasVel, ckick, centr):
    """the per-bin factors of apply_half_kick / apply_hydro_half_kick (timestep.c:936-945) with linear kick integrals: the factors of the bins
    from mintimebin that are active, dt_entr for every bin"""
    K = KF()
    for b in range(TIMEBINS + 1):
        K.bin_active[b] = int(H.is_timebin_active(b, times["Ti_Current"]))
        K.dt_entr[b] = (H.dti_from_timebin(b) // 2) * centr
        if b < times["mintimebin"] or not K.bin_active[b]:
            continue
        newkick = times["Ti_kick"][b] + H.dti_from_timebin(b) // 2
        K.gravkick[b] = (newkick - times["Ti_kick"][b]) * ckick
        K.hydrokick[b] = (newkick - times["Ti_kick"][b]) * ckick
    K.atime, K.MaxGasVel = atime, MaxGasVel
    return K


def test_dev_apply_hydro_half_kick_bitwise(pkg, engine):
    import torch
    rng = np.random.RandomState(17)
    n = 50021
    typ = rng.choice(np.array([0, 1], np.uint8), n)
    flags = ((rng.random_sample(n) < 0.04) * rng.randint(1, 4, n)).astype(np.uint8)
    tbh = rng.randint(0, 9, n).astype(np.uint8)                       # bins 0 .. 8
    vel = rng.standard_normal((n, 3))
    fast = rng.random_sample(n) < 0.05
    vel[fast] *= 40.0                                                   # these exceed MaxGasVel * atime
    hacc, dte = rng.standard_normal((n, 3)), rng.standard_normal(n)
    ent = 1.0 + rng.random_sample(n)
    times = dict(Ti_Current=3 << 4, mintimebin=2, Ti_kick=[int(x) for x in rng.randint(0, 1 << 20, TIMEBINS + 1)])
    assert sorted({H.is_timebin_active(b, times["Ti_Current"]) for b in range(9)}) == [False, True]
    Kd = kick_factors(pkg.KickFactors, times, 0.5, 9.0, 1e-6, 3e-7)
    Kd.gravkick[3] = 1e300                                              # (must not be read)
    assert max(np.sqrt((vel ** 2).sum(1))[typ == 0] / 0.5) > 9.0
    half = np.sort(rng.choice(n, n // 2, replace=False)).astype(np.int32)
    for act in (half, None):
        v_o, e_o = vel.copy(), ent.copy()
        hydro_half_kick(v_o, e_o, typ, tbh, hacc, dte, Kd, active=act, flags=flags)
        d_vel, d_ent = dev(torch, vel), dev(torch, ent)
        engine.dev_apply_hydro_half_kick(d_vel, Kd, dev(torch, typ), dev(torch, hacc), d_ent, dev(torch, dte), active=dev(torch, act),
                                         flags=dev(torch, flags), tb_hydro=dev(torch, tbh))
        engine.synchronize()
        v_d, e_d = d_vel.cpu().numpy(), d_ent.cpu().numpy()
        assert np.array_equal(v_d, v_o) and np.array_equal(e_d, e_o)
        listed = np.zeros(n, bool)
        listed[np.arange(n) if act is None else act] = True
        untouched = ~listed | (typ != 0) | ((flags & 3) != 0)
        assert np.array_equal(v_d[untouched], vel[untouched]) and np.array_equal(e_d[untouched], ent[untouched])
        changed = listed & (typ == 0) & ((flags & 3) == 0)
        kicked = changed & (np.asarray(Kd.hydrokick)[tbh] != 0)                          # (bins active at Ti_Current, from mintimebin)
        assert kicked.sum() > n // 20 and (v_d[kicked] != vel[kicked]).any(axis=1).all()
        speed = np.sqrt((v_d[changed] ** 2).sum(1))
        assert np.isclose(speed, 9.0 * 0.5, rtol=1e-12).sum() > 100 and speed.max() <= 9.0 * 0.5 * (1 + 1e-12)   # (the limit did act)
    with pytest.raises(pkg.EngineError, match="hydro time bin"):
        bad = tbh.copy()
        bad[np.nonzero(typ == 0)[0][0]] = TIMEBINS + 1
        engine.dev_apply_hydro_half_kick(dev(torch, vel), Kd, dev(torch, typ), dev(torch, hacc), dev(torch, ent), dev(torch, dte),
                                         tb_hydro=dev(torch, bad))


# ---- the split-gravity branch of run.c (run.c:436-565, 754-794) on the resident table, against the oracle
def _setup(pkg, orc, gas):
    """initial state and parameters: positions, velocities, GravPM and FullTreeGravAccel of a full tree (the oracle's), the timeline, a
    Hubble rate that spreads the gravity steps over several bins below the PM step"""
    if gas:
        s = _gas_run_setup(pkg, n=10)
        pos, mass, typ, box, n = s["pos"], s["mass"], s["typ"].astype(np.uint8), s["box"], s["n"]
        vel = s["vel"] * 1e-2
        nmesh = 2 * n
    else:
        n, nmesh = 14, 28
        pos, mass, box = pkg.ics.s_clust(n)
        typ = np.ones(len(pos), np.uint8)
        vel = np.random.RandomState(11).standard_normal((len(pos), 3)) * 1e-2
        s = {}
    N = len(pos)
    par = O.make_grav_params(box, nmesh, npart_cbrt=n, G=G)
    par.TreeUseBH = 0
    gpm, _ = O.gravpm_force(pos, mass, box, nmesh, 1.5, G)
    tr = orc.tree(pos, mass, box)
    full, _, _, _ = tr.grav_short_tree(par, oldacc=np.sqrt((gpm ** 2).sum(1)) / G)
    tr.free()
    soft = 2.8 * (box / n) / 30.
    atime, ErrTol = 0.1, 0.025
    dl1 = O.timestep_gravity_dloga(orc, full, gpm, atime, 1.0, ErrTol, soft)
    c = dict(gas=gas, n=n, nmesh=nmesh, N=N, pos=pos, mass=mass, typ=typ, box=box, vel=vel, gpm=gpm, full=full, par=par, soft=soft, atime=atime,
             ErrTol=ErrTol, MinSize=0.0, hubble=6e-3 / np.median(dl1), loga=[np.log(0.1), np.log(0.5), np.log(1.0)], dti_max_pm=1 << 40,
             ckick=1e-3 / float(1 << 40), centr=1e-4 / float(1 << 40), MaxGasVel=1e30, courant=0.15, pe=1, nsteps=6)
    if gas:
        c["ent"] = s["ent"] / 4 ** 7                                                     # (sound speed: hydro steps near the gravity steps)
        c["hsml0"] = np.full(N, 2.5 * box / n)
    return c


def _active(c, tb_grav, tb_hydro, times):
    """build_active_particles (timestep.c:1333-1420): all on a PM step (NULL list), else the gas that is hydro-active and every particle
    that is gravity-active, in particle order"""
    N, ti = c["N"], times["Ti_Current"]
    if ti == times["PM_start"] + times["PM_length"]:
        return None, N
    ga = np.array([H.is_timebin_active(int(b), ti) for b in tb_grav])
    ha = np.array([H.is_timebin_active(int(b), ti) for b in tb_hydro]) & (c["typ"] == 0)
    return np.nonzero(ga | ha)[0].astype(np.int32), int(ga.sum())


def _sph_times(c, times):
    f = [0.0] + [c["ckick"] * H.dti_from_timebin(b) * 0.5 for b in range(1, TIMEBINS + 1)]
    return dict(atime=c["atime"], hubble=c["hubble"], FgravkickB=0.0, gravkicks=f, hydrokicks=f, drifts=[2 * x for x in f],
                dloga_kick=[x * 0.1 for x in f], dloga_bin=[x * 0.2 for x in f])


class _Oracle:
    """the oracle's side of one run: state S (hiergrav_oracle's dict) and, for gas, the SPH arrays sharing its Pos / Vel / bins"""

    def __init__(self, orc, c):
        self.orc, self.c = orc, c
        N = c["N"]
        S = dict(pos=c["pos"].copy(), mass=c["mass"].copy(), box=c["box"], vel=c["vel"].copy(), gravpm=c["gpm"].copy(), fulltree=c["full"].copy(),
                 tb_grav=np.zeros(N, np.uint8), flags=None, stored=None)
        self.S = S
        self.tb_hydro = np.zeros(N, np.uint8)
        if c["gas"]:
            A = O.SphArrays(S["pos"], S["mass"], type=c["typ"].astype(np.int32), hsml=c["hsml0"], vel=S["vel"], entropy=c["ent"].copy())
            S["pos"], S["vel"], A.tb_grav, A.tb_hydro = A.pos, A.vel, S["tb_grav"], self.tb_hydro
            O.sph_set_softening(orc, c["soft"])
            self.A = A

    def sph(self, act, times):
        c, A, S = self.c, self.A, self.S
        N = c["N"]
        A.gacc[:], A.gpm[:] = S["fulltree"], S["gravpm"]
        A.hydroacc_in[:], A.dtentropy_in[:] = A.hydroacc_out, A.dtentropy_out
        hact = np.zeros(N, np.uint8)
        hact[np.arange(N) if act is None else act] = 1
        to = O.sph_times(**_sph_times(c, times))
        dp = O.DensityParams(1.0, 2.0, 2.0, 99999., 2, 0.006)
        trg = self.orc.tree(A.pos, S["mass"], c["box"], type=A.type, hsml=A.hsml, hydro_active=hact, mask=1, moments=False)
        O.sph_density(self.orc, trg, dp, A, to, active=act, DoEgyDensity=c["pe"])
        trg.calc_moments()
        O.sph_hydro_force(self.orc, trg, dp, O.HydroParams(c["pe"], 100.0, 0.75), A, to, active=act)

    def hydro_kick(self, act, K):
        A = self.A
        hydro_half_kick(A.vel, A.entropy, self.c["typ"], self.tb_hydro, A.hydroacc_out, A.dtentropy_out, K, active=act)

    def gravpm(self):
        c, S = self.c, self.S
        S["gravpm"][:], _ = O.gravpm_force(S["pos"], S["mass"], c["box"], c["nmesh"], 1.5, G)

    def accelerations(self, act, nag, times, stored):
        self.S["stored"] = stored
        H.hierarchical_gravity_accelerations(self.orc, self.S, act, nag, times, self.c["par"], G, self._gk)

    def and_timesteps(self, act, nag, times, stored):
        c = self.c
        self.S["stored"] = stored
        return H.hierarchical_gravity_and_timesteps(self.orc, self.S, act, nag, times, H.Timeline(c["loga"]), c["ErrTol"], c["MinSize"], c["atime"],
                                                    c["hubble"], c["dti_max_pm"], c["par"], G, c["soft"], self._gk)

    def find_hydro(self, act, times, first):
        c, A = self.c, self.A
        S = dict(type=c["typ"], hsml=A.hsml, dthsml=A.dthsml, maxsignalvel=A.maxsignalvel, tb_grav=self.S["tb_grav"], tb_hydro=self.tb_hydro)
        r = H.find_hydro_timesteps(S, act, times, H.Timeline(c["loga"]), c["MinSize"], c["courant"], c["atime"], c["hubble"], isFirstTimeStep=first)
        return r["badstepsizecount"]

    def pm_kick(self, F):
        S = self.S
        O.apply_pm_half_kick(self.orc, S["vel"], S["gravpm"], F)

    def drift(self, ddrift):
        c, S = self.c, self.S
        if c["gas"]:
            assert O.drift_all_particles(self.orc, S["pos"], S["vel"], ddrift, c["box"], type=c["typ"], hsml=self.A.hsml, dthsml=self.A.dthsml) == 0
        else:
            assert O.drift_all_particles(self.orc, S["pos"], S["vel"], ddrift, c["box"]) == 0

    def bins(self):
        return self.tb_hydro.copy(), self.S["tb_grav"].copy()

    _gk = None


class _Engine:
    """the engine's side: a resident table P (struct particle_data) and the resident SPH arrays, driven through the Python mirror"""

    def __init__(self, pkg, c):
        self.pkg, self.c = pkg, c
        N, box, n = c["N"], c["box"], c["n"]
        eng = pkg.Engine(0)
        eng.gravshort_fill_ntab(0, 1.5)
        eng.gravpm_init_periodic(box, 1.5, c["nmesh"], G)
        eng.set_gravshort_treepar(TreeUseBH=0)
        eng.gravshort_set_softenings(box / n)
        eng.set_densitypar(1.0, 2.0, 2.0, 99999., pkg.engine.DENSITY_KERNEL_QUINTIC_SPLINE, 0.006)
        eng.set_hydropar(c["pe"], 100.0, 0.75)
        P = pkg.make_particles(c["pos"], c["mass"], type=c["typ"])
        P["Vel"], P["GravPM"], P["FullTreeGravAccel"] = c["vel"], c["gpm"], c["full"]
        z = lambda *sh: np.zeros(sh)
        hsml = c["hsml0"].copy() if c["gas"] else z(N)
        ent = c["ent"].copy() if c["gas"] else z(N)
        self.a = dict(hsml=hsml, dthsml=z(N), vel=z(N, 3), gacc=z(N, 3), gpm=z(N, 3), hydroacc_in=z(N, 3), tb_hydro=np.zeros(N, np.uint8),
                      tb_grav=np.zeros(N, np.uint8), entropy=ent, dtentropy_in=z(N), density=z(N), egywtdensity=z(N), dhsmlegyfac=z(N), divvel=z(N),
                      curlvel=z(N), hydroacc_out=z(N, 3), dtentropy_out=z(N), maxsignalvel=z(N))
        self.eng, self.P = eng, P
        self.begin()

    def begin(self):
        self.eng.resident_begin(self.P, self.c["box"])
        self.eng.resident_sph_begin(self.P, self.a)

    def end(self):
        self.eng.resident_sph_end(self.a)
        self.eng.resident_end(self.P)

    def sph(self, act, times):
        t = make_times_like(self.pkg, **_sph_times(self.c, times))
        self.eng.density(self.P, self.c["box"], self.a, t, ActiveParticle=act, DoEgyDensity=self.c["pe"])
        self.eng.hydro_force(self.P, self.a, t, ActiveParticle=act)

    def hydro_kick(self, act, K):
        self.eng.resident_apply_hydro_half_kick(self.P, K, ActiveParticle=act)

    def gravpm(self):
        self.eng.gravpm_force(self.P)

    def accelerations(self, act, nag, times, stored):
        ts = to_struct(self.pkg, times)
        self.eng.resident_hierarchical_gravity_accelerations(self.P, ts, 0.0, self._gk, ActiveParticle=act, NumActiveGravity=nag, StoredGravAccel=stored)
        from_struct(ts, times)

    def and_timesteps(self, act, nag, times, stored):
        c = self.c
        ts = to_struct(self.pkg, times)
        isPM = times["Ti_Current"] == times["PM_start"] + times["PM_length"]
        bad = self.eng.resident_hierarchical_gravity_and_timesteps(self.P, ts, c["loga"], c["ErrTol"], c["MinSize"], c["atime"], c["hubble"],
                                                                   c["dti_max_pm"] if isPM else 0, 0.0, self._gk, ActiveParticle=act,
                                                                   NumActiveGravity=nag, StoredGravAccel=stored)
        from_struct(ts, times)
        return bad

    def find_hydro(self, act, times, first):
        c = self.c
        ts = to_struct(self.pkg, times)
        r = self.eng.resident_find_hydro_timesteps(self.P, ts, c["loga"], c["MinSize"], c["courant"], c["atime"], c["hubble"], ActiveParticle=act,
                                                   isFirstTimeStep=first)
        from_struct(ts, times)
        return r["badstepsizecount"]

    def pm_kick(self, F):
        self.eng.resident_apply_pm_half_kick(self.P, F)

    def drift(self, ddrift):
        self.eng.resident_drift_all_particles(self.P, ddrift)

    def bins(self):
        return self.eng.resident_fetch_timebins(self.c["N"])          # (what the shim's fetch_timebins copies into P[])

    _gk = None


def _drive(side, c, interrupt_at=None):
    """run.c:436-565, 754-794 with HierarchicalGravity, c["nsteps"] sub-steps; returns the record of every bin assignment.  interrupt_at: the
    sub-step in which the resident stretch ends and a new one begins between the two halves of the gravity step (engine side only)."""
    gk = lambda t0, t1: (t1 - t0) * c["ckick"]
    side._gk = gk
    N = c["N"]
    times = dict(mintimebin=0, maxtimebin=0, mingravtimebin=0, Ti_kick=[0] * (TIMEBINS + 1), Ti_Current=0, PM_length=0, PM_start=0, PM_kick=0)
    tb_hydro, tb_grav = np.zeros(N, np.uint8), np.zeros(N, np.uint8)
    rec = []
    for step in range(c["nsteps"]):
        isPM = times["Ti_Current"] == times["PM_start"] + times["PM_length"]
        act, nag = _active(c, tb_grav, tb_hydro, times)
        if c["gas"]:
            side.sph(act, times)                                                         # run.c:472, 489
            side.hydro_kick(act, kick_factors(side.K, times, c["atime"], c["MaxGasVel"], c["ckick"], c["centr"]))   # run.c:498-499
        if isPM:
            side.gravpm()                                                                # run.c:522
        stored = np.zeros((N + 5, 3))                                                    # (run.c:538: NumPart + room for new stars)
        if nag:                                                                          # run.c:531-540 (totgravactive)
            side.accelerations(act, nag, times, stored)
        if interrupt_at == step:
            side.end()
            held = stored.copy()
            side.begin()
        update_kick_times(times)                                                         # run.c:563
        if isPM:                                                                         # run.c:565, apply_PM_half_kick timestep.c:964-985
            F = gk(times["PM_kick"], times["PM_kick"] + times["PM_length"] // 2)
            side.pm_kick(F)
            times["PM_kick"] += times["PM_length"] // 2
        bad = side.and_timesteps(act, nag, times, stored) if nag else 0                 # run.c:766-767
        if c["gas"]:
            bad += side.find_hydro(act, times, step == 0)                                # run.c:770
            side.hydro_kick(act, kick_factors(side.K, times, c["atime"], c["MaxGasVel"], c["ckick"], c["centr"]))   # run.c:773
        tb_hydro, tb_grav = side.bins()
        rec.append(dict(step=step, isPM=isPM, act=act, nact=N if act is None else len(act), nag=nag, bad=bad, tb_hydro=tb_hydro, tb_grav=tb_grav,
                        times=dict(times, Ti_kick=list(times["Ti_kick"])), held=held if interrupt_at == step else None, stored=stored))
        update_kick_times(times)                                                         # run.c:788
        if isPM:                                                                         # run.c:794
            F = gk(times["PM_kick"], times["PM_kick"] + times["PM_length"] // 2)
            side.pm_kick(F)
            times["PM_kick"] += times["PM_length"] // 2
        ti_next = times["Ti_Current"] + H.dti_from_timebin(times["mintimebin"])          # find_next_kick, timestep.c:1324-1328
        side.drift((ti_next - times["Ti_Current"]) * c["ckick"])                         # run.c:392-420
        times["Ti_Current"] = ti_next
    return rec


def _oracle_run(orc, c):
    o = _Oracle(orc, c)
    o.K = O.KickFactors
    rec = _drive(o, c)
    return o, rec


def _check_record(c, rec_o):
    """what the run must have exercised"""
    assert len(rec_o) >= 3
    assert any(not r["isPM"] and 0 < r["nag"] < c["N"] for r in rec_o), [(r["isPM"], r["nag"]) for r in rec_o]
    assert all(r["bad"] == 0 for r in rec_o)
    if not c["gas"]:
        assert max(len(np.unique(r["tb_grav"])) for r in rec_o) >= 3


@pytest.mark.parametrize("case", ["dm", "gas"])
def test_resident_steps_in_run_c_order_with_split_gravity(pkg, orc, case):
    c = _setup(pkg, orc, case == "gas")
    o, rec_o = _oracle_run(orc, c)
    _check_record(c, rec_o)
    e = _Engine(pkg, c)
    e.K = pkg.KickFactors
    pos0, vel0 = e.P["Pos"].copy(), e.P["Vel"].copy()
    rec_d = _drive(e, c)
    assert np.array_equal(e.P["Pos"], pos0) and np.array_equal(e.P["Vel"], vel0)            # (the host copies stayed stale: still resident)
    e.end()
    e.eng.close()
    for rd, ro in zip(rec_d, rec_o):
        k = rd["step"]
        assert rd["times"] == ro["times"], (k, rd["times"], ro["times"])
        assert rd["bad"] == ro["bad"] == 0, k
        assert np.array_equal(rd["tb_grav"], ro["tb_grav"]), (k, np.nonzero(rd["tb_grav"] != ro["tb_grav"])[0][:10])
        if c["gas"]:
            gas = c["typ"] == 0
            assert np.array_equal(rd["tb_hydro"][gas], ro["tb_hydro"][gas]), (k, np.nonzero(rd["tb_hydro"] != ro["tb_hydro"])[0][:10])
    S, box, sp = o.S, c["box"], c["box"] / c["n"]
    dpos = np.abs(np.mod(e.P["Pos"] - S["pos"] + box / 2, box) - box / 2).max()
    assert dpos <= 1e-9 * sp, dpos
    assert np.abs(e.P["Vel"] - S["vel"]).max() <= 1e-9 * np.abs(S["vel"]).max()
    moved = np.abs(np.mod(S["pos"] - c["pos"] + box / 2, box) - box / 2).max()
    assert moved > 0
    if c["gas"]:
        gas = c["typ"] == 0
        for key in ("entropy", "hsml", "density"):
            g, r = e.a[key][gas], getattr(o.A, key)[gas]
            assert np.abs(g - r).max() <= 1e-9 * np.abs(r).max(), (key, np.abs(g - r).max() / np.abs(r).max())
        assert np.abs(o.A.entropy[gas] / c["ent"][gas] - 1).max() > 0                      # (the hydro kicks changed the entropies)


def test_resident_stored_accel_survives_end_begin(pkg, orc):
    c = _setup(pkg, orc, False)
    c["nsteps"] = 4
    runs = []
    for interrupt in (None, 2):
        e = _Engine(pkg, c)
        e.K = pkg.KickFactors
        rec = _drive(e, c, interrupt_at=interrupt)
        e.end()
        e.eng.close()
        runs.append((rec, e.P.copy()))
    (rec_a, P_a), (rec_b, P_b) = runs
    for ra, rb in zip(rec_a, rec_b):
        assert ra["times"] == rb["times"] and np.array_equal(ra["tb_grav"], rb["tb_grav"])
    # (the walks of the level trees are not bitwise reproducible from one run to the next - two uninterrupted runs differ by a few ulp in
    # the velocities - so the interrupted run is held to that, with the time bins and kick times exact)
    assert np.abs(P_a["Vel"] - P_b["Vel"]).max() <= 1e-12 * np.abs(P_a["Vel"]).max()
    assert np.abs(P_a["Pos"] - P_b["Pos"]).max() <= 1e-12 * c["box"]
    # after resident_end between the halves the host StoredGravAccel holds the device copy: the accelerations of the active particles (as
    # the oracle's) and, in the rows the step did not write, the zeros the first call uploaded
    r = rec_b[2]
    held, act = r["held"], r["act"]
    idx = np.arange(c["N"]) if act is None else act
    assert not r["isPM"] and len(idx) < c["N"]
    _, rec_o = _oracle_run(orc, c)
    so = rec_o[2]["stored"][idx]
    assert np.abs(held[idx] - so).max() <= 1e-8 * np.abs(so).max()
    rest = np.ones(len(held), bool)
    rest[idx] = False
    assert not held[rest].any()


def test_resident_hierarchical_errors(pkg, orc):
    c = _setup(pkg, orc, False)
    N = c["N"]
    eng = pkg.Engine(0)
    eng.gravshort_fill_ntab(0, 1.5)
    eng.gravpm_init_periodic(c["box"], 1.5, c["nmesh"], G)
    eng.gravshort_set_softenings(c["box"] / c["n"])
    P = pkg.make_particles(c["pos"], c["mass"])
    gk = lambda t0, t1: 0.0
    times = dict(mintimebin=0, maxtimebin=0, mingravtimebin=0, Ti_kick=[0] * (TIMEBINS + 1), Ti_Current=0, PM_length=0, PM_start=0, PM_kick=0)
    K = kick_factors(pkg.KickFactors, times, 1.0, 1e30, 0.0, 0.0)
    calls = lambda Q: [lambda: eng.resident_hierarchical_gravity_accelerations(Q, to_struct(pkg, times), 0.0, gk),
                       lambda: eng.resident_hierarchical_gravity_and_timesteps(Q, to_struct(pkg, times), c["loga"], 0.025, 0.0, 0.1, 1.0, 1 << 40,
                                                                               0.0, gk),
                       lambda: eng.resident_apply_hydro_half_kick(Q, K)]
    for f in calls(P):                                                    # no resident table
        with pytest.raises(pkg.EngineError, match="resident"):
            f()
    P["Vel"] = c["vel"]
    eng.resident_begin(P, c["box"])
    for f in calls(P):                                                    # no resident_sph_begin
        with pytest.raises(pkg.EngineError, match="mpg_resident_sph_begin"):
            f()
    z = lambda *sh: np.zeros(sh)
    a = dict(hsml=z(N), dthsml=z(N), vel=z(N, 3), gacc=z(N, 3), gpm=z(N, 3), hydroacc_in=z(N, 3), tb_hydro=np.zeros(N, np.uint8),
             tb_grav=np.zeros(N, np.uint8), entropy=z(N), dtentropy_in=z(N), density=z(N), egywtdensity=z(N), dhsmlegyfac=z(N), divvel=z(N),
             curlvel=z(N), hydroacc_out=z(N, 3), dtentropy_out=z(N), maxsignalvel=z(N))
    eng.resident_sph_begin(P, a)
    for f in calls(P[: N - 7].copy()):                                   # a view of the wrong size
        with pytest.raises(pkg.EngineError, match="not the resident particle table"):
            f()
    with pytest.raises(pkg.EngineError, match="StoredGravAccel"):
        eng.resident_hierarchical_gravity_accelerations(P, to_struct(pkg, times), 0.0, gk, StoredGravAccel=np.zeros((N - 1, 3)))
    eng.resident_sph_end(a)
    eng.resident_end(P)
    eng.close()
