"""GPU parity of the sub-grid group sums (mpg_dev_fof_subgrid: k_fof_subgrid, k_fof_seed_index) and of black-hole seeding (mpg_dev_fof_seed:
k_fof_seed_mark, k_blackhole_make_one; csrc/fof.hip) with the restatement of fof.c:631-676, :1356-1365 and blackhole.c:1039-1111
(tests/fof_subgrid_restated.py) on the membership of the FOF oracle.

Bounds: integers (seed_index, the seed list, type, countprogs, tb_dynfric, swallowid, nwarn) and MaxDens exact; every column blackhole_make_one
writes bit-identical, except the power-law bh_mass / mseed; every sum within L 2^-52 sum|term| of the long-double sum (L the group's length:
any order of L - 1 fp64 additions of terms that are exact, or rounded once, errs by at most L 2^-53 sum|term| to first order).
The power-law mass has one device pow() against libm's (its three constants are taken on the host): measured largest relative difference
over the sets of this file 4.44e-16 = 2 ulp; asserted 8 x that."""
import numpy as np
import pytest

import fof_subgrid_restated as R
import fof_subgrid_scenes as S

pytestmark = pytest.mark.gpu

POW_MEASURED = 4.44e-16
POW_BOUND = min(8 * POW_MEASURED, 1e-12)
ATIME = 0.3125
TORCH_VIEW = {"uint64": np.int64}                     # (torch has no uint64: the same bits)


def dev(a):
    import torch
    if a is None:
        return None
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(TORCH_VIEW.get(a.dtype.name, a.dtype)).copy()).cuda()


def run_fof(engine, T, minlen=None):
    """binds the set and finds its groups -> (tensors kept alive, grnr, group table)"""
    import torch
    keep = dict(pos=dev(T["pos"]), mass=dev(T["mass"]), type=dev(T["type"]), ids=dev(T["ids"]), flags=dev(T["flags"]))
    engine.dev_bind_particles(keep["pos"], keep["mass"], T["box"], type=keep["type"])
    grnr = torch.zeros(T["n"], dtype=torch.int64, device="cuda")
    ng = engine.dev_fof_fof(keep["ids"], T["LL"], T["minlen"] if minlen is None else minlen, flags=keep["flags"], grnr=grnr)
    G = {k: v.cpu().numpy() for k, v in engine.dev_fof_groups(ng).items()}
    G["MinID"] = G["MinID"].view(np.uint64)
    return keep, grnr.cpu().numpy(), G


def run_subgrid(engine, T, ng, wind_decouple, leave_out=()):
    cols = {k: dev(v) for k, v in T["P"].items() if k not in leave_out}
    sub = engine.dev_fof_subgrid(ng, WindDecouple=wind_decouple, **cols)
    engine.synchronize()
    return {k: v.cpu().numpy() for k, v in sub.items()}


def check(engine, orc, T, wind_decouple, minlen=None, leave_out=()):
    """FOF + sub-grid sums of the set on the engine against the restatement on the oracle's membership -> (engine's, restated)"""
    grnr_o, Go, group = S.membership(orc, T, minlen)
    keep, grnr, G = run_fof(engine, T, minlen)
    assert np.array_equal(grnr, grnr_o) and np.array_equal(G["MinID"], Go["MinID"]) and np.array_equal(G["GrNr"], Go["GrNr"])
    ng = len(Go["MinID"])
    sub = run_subgrid(engine, T, ng, wind_decouple, leave_out)
    P = {k: v for k, v in T["P"].items() if k not in leave_out}
    want = R.group_sums(group, ng, T["mass"], T["type"], P, wind_decouple, "ld")
    assert np.array_equal(sub["seed_index"], want["seed_index"])
    assert np.array_equal(sub["MaxDens"], want["MaxDens"])
    for k in R.SUMS:
        err = np.abs(sub[k].astype(np.longdouble) - want[k])
        bound = R.sum_bound(want["Length"], want["abs_" + k])
        worst = float((err[bound > 0] / bound[bound > 0]).max()) if (bound > 0).any() else 0.0
        print("%s %s wd %d: %s error / bound %.3g" % (T["name"], leave_out, wind_decouple, k, worst))
        assert np.all(err <= bound), k
        assert np.all(sub[k][want["abs_" + k] == 0] == 0), k
    del keep
    return sub, want


@pytest.mark.parametrize("wd", [0, 1])
@pytest.mark.parametrize("scene", S.SUM_SCENES, ids=lambda s: "%s-%s%s" % (s[0], s[1], "-highids" if s[2] else ""))
def test_sums_and_seed_rows(engine, orc, scene, wd):
    """Many groups per wave with rows of no group between them; a 64-row group on a wave boundary; a 700-row group across blocks; a group
    ending on the last row; a group of dark matter only; IDs above 2^63."""
    T = S.particles(*scene)
    sub, want = check(engine, orc, T, wd)
    assert (want["seed_index"] >= 0).sum() >= 2
    if scene[0] == "big700":
        _, Go, _ = S.membership(orc, T)
        dm = np.nonzero(Go["LenType"][:, 1] == Go["Length"])[0]
        assert len(dm) >= 1 and np.all(sub["seed_index"][dm] == -1) and np.all(sub["MaxDens"][dm] == 0)
        assert all(np.all(sub[k][dm] == 0) for k in R.SUMS)


def test_all_gas_decoupled(engine, orc):
    T = S.particles("minlen2")
    T = S.variant(T, delaytime=np.full(T["n"], 0.5))
    sub, _ = check(engine, orc, T, 1)
    assert np.all(sub["seed_index"] == -1) and np.all(sub["MaxDens"] == 0)
    sub, _ = check(engine, orc, T, 0)                                        # without WIND_DECOUPLE_SPH DelayTime is not looked at
    assert (sub["seed_index"] >= 0).sum() >= 20


def test_density_zero_is_no_seed(engine, orc):
    T = S.particles("minlen2")
    dens = T["P"]["density"].copy()
    dens[T["cluster"] % 2 == 0] = 0.0
    T = S.variant(T, density=dens)
    sub, _ = check(engine, orc, T, 0)
    _, _, group = S.membership(orc, T)
    even = np.unique(group[(T["cluster"] % 2 == 0) & (group >= 0)])
    assert len(even) >= 10 and np.all(sub["seed_index"][even] == -1) and (sub["seed_index"] >= 0).sum() >= 10


def test_equal_maxima_in_one_wave(engine, orc):
    T, (a, b) = S.with_ties(S.particles("big700", "shuffle"), far=False)
    sub, _ = check(engine, orc, T, 1)
    _, _, group = S.membership(orc, T)
    assert group[a] == group[b] and sub["seed_index"][group[a]] == min(a, b) and sub["MaxDens"][group[a]] == 77.25


@pytest.mark.parametrize("order", ["label", "reverse", "shuffle"])
def test_equal_maxima_in_different_blocks(engine, orc, order):
    """The smaller particle index wins whatever block finishes first, under three particle orders of the same IDs."""
    T, (a, b) = S.with_ties(S.particles("big700", order), far=True)
    sub, _ = check(engine, orc, T, 1)
    _, _, group = S.membership(orc, T)
    assert group[a] == group[b] and sub["seed_index"][group[a]] == min(a, b) and sub["MaxDens"][group[a]] == 77.25


@pytest.mark.parametrize("minlen", [1, 2])
def test_garbage_and_swallowed_rows(engine, orc, minlen):
    """Flagged rows link to nothing: with FOFHaloMinLength 2 they are in no group, with 1 each is a group of its own (as in the reference)."""
    T = S.with_flags(S.particles("minlen2"))
    check(engine, orc, T, 1, minlen=minlen)


@pytest.mark.parametrize("column", list(R.COLUMNS) + ["all"])
def test_every_column_may_be_null(engine, orc, column):
    T = S.particles("seeds")
    out = R.COLUMNS if column == "all" else (column,)
    sub, _ = check(engine, orc, T, 1, leave_out=out)
    if column in ("density", "all"):
        assert np.all(sub["seed_index"] == -1) and np.all(sub["MaxDens"] == 0)


# ---- seeding ----
FLOAT_COLS = ("bh_mass", "mseed", "mdot", "formationtime", "bh_density", "df_surroundingrmsvel", "df_surroundingdensity", "mtrack",
              "kineticfdbkenergy", "vdisp")
VEC_COLS = ("minpotpos", "dfaccel", "df_surroundingvel", "dragaccel")


def seed_columns(T):
    """blackhole_make_one's columns with values that no rule writes, so that every write and every row left alone shows"""
    n = T["n"]
    rng = np.random.RandomState(77)
    cols = dict(id=np.array(T["ids"]), tb_hydro=np.array(T["tb_hydro"]), type=np.array(T["type"]), mass=np.array(T["mass"]))
    for k in FLOAT_COLS:
        cols[k] = rng.random_sample(n) + 40
    for k in VEC_COLS:
        cols[k] = rng.random_sample((n, 3)) + 40
    cols.update(swallowid=rng.randint(1, 1000, n).astype(np.uint64), tb_dynfric=np.full(n, 3, np.uint8), jumptominpot=np.full(n, 42, np.int32),
                countprogs=np.full(n, 42, np.int32))
    return cols


def seed_setup(engine, orc, T=None):
    """FOF and sub-grid sums of the "seeds" set on the engine; thresholds that put one group exactly AT the mass threshold and one just
    below the stellar one -> (tensors kept alive, oracle table, restated sums, parameters)"""
    T = S.particles("seeds") if T is None else T
    _, Go, group = S.membership(orc, T)
    keep, _, _ = run_fof(engine, T)
    ng = len(Go["MinID"])
    run_subgrid(engine, T, ng, 1)
    want = R.group_sums(group, ng, T["mass"], T["type"], T["P"], 1, "ld")
    cand = np.nonzero((Go["LenType"][:, 5] == 0) & (want["seed_index"] >= 0) & (Go["MassType"][:, 4] > 0))[0]
    assert len(cand) >= 5
    masses = np.sort(Go["Mass"][cand])
    heavy = cand[Go["Mass"][cand] >= masses[1]]
    mstars = np.sort(Go["MassType"][heavy, 4])
    par = dict(MinFoFMassForNewSeed=float(masses[1]), MinMStarForNewSeed=float(np.nextafter(mstars[0], np.inf)), SeedBlackHoleMass=0.05,
               MaxSeedBlackHoleMass=0.0, SeedBlackHoleMassIndex=-1.5, SeedBHDynMass=0.0)
    marked = R.seed_marks(Go["Mass"], Go["MassType"], Go["LenType"], want["seed_index"], par)
    at = cand[Go["Mass"][cand] == masses[1]]
    below = heavy[Go["MassType"][heavy, 4] == mstars[0]]
    assert len(marked) >= 3 and np.isin(at, marked).all()                                      # exactly at the mass threshold: kept
    assert len(below) >= 1 and not np.isin(below, marked).any()                                # heavy enough, dropped for its stars alone
    with_bh = np.nonzero((Go["LenType"][:, 5] > 0) & (Go["Mass"] >= par["MinFoFMassForNewSeed"]) & (want["seed_index"] >= 0))[0]
    assert len(with_bh) >= 1 and not np.isin(with_bh, marked).any()
    assert (Go["Mass"][cand] < par["MinFoFMassForNewSeed"]).any()
    return T, keep, Go, want, par


def engine_params(pkg, par):
    return pkg.engine.FofSeedParams(*[par[k] for k, _ in pkg.engine.FofSeedParams._fields_])


TABLE = np.random.RandomState(99).random_sample(1013)


@pytest.mark.parametrize("dynmass", [0.0, 2.0, 0.125])
@pytest.mark.parametrize("case", ["constant", "powerlaw", "powerlaw-highids"])
def test_seeding(engine, orc, pkg, case, dynmass):
    """Constant and power-law seed mass (also on IDs whose ID + 23 wraps), SeedBHDynMass 0, above every mass and below the particles' (the
    reference's warning for every seed): the list, every column, every row that is no seed bit-identical."""
    powerlaw = case != "constant"
    T, keep, Go, want, par = seed_setup(engine, orc, S.particles("seeds", "shuffle", True) if case == "powerlaw-highids" else None)
    par = dict(par, SeedBHDynMass=dynmass, MaxSeedBlackHoleMass=0.9 if powerlaw else 0.0)
    engine.set_random_table(TABLE)
    cols = seed_columns(T)
    ref = {k: v.copy() for k, v in cols.items()}
    parts_o, groups_o, nwarn_o = R.fof_seed(Go["Mass"], Go["MassType"], Go["LenType"], want["seed_index"], ref, np.array(T["pos"]), ATIME, TABLE, par)
    d = {k: dev(v) for k, v in cols.items()}
    parts, groups, nwarn = engine.dev_fof_seed(engine_params(pkg, par), ATIME, d)
    engine.synchronize()
    assert np.array_equal(parts.cpu().numpy(), parts_o) and np.array_equal(groups.cpu().numpy(), groups_o) and nwarn == nwarn_o
    assert len(parts_o) >= 3
    if case == "powerlaw-highids":
        assert ((T["ids"][parts_o] + np.uint64(23)) < np.uint64(23)).any()                    # a seed whose ID + 23 wraps
    if case == "powerlaw" and dynmass == 0.0:
        assert 0 < nwarn_o < len(parts_o)                                                     # seed masses above some particles' masses
    if dynmass > 0:
        assert nwarn_o == (len(parts_o) if dynmass == 0.125 else 0)
    for k, v in d.items():
        got = v.cpu().numpy().view(ref[k].dtype)
        if powerlaw and k in ("bh_mass", "mseed"):
            rel = np.abs(got[parts_o] / ref[k][parts_o] - 1).max()
            print("power-law %s: largest relative difference %.3g" % (k, rel))
            assert rel <= POW_BOUND
            rest = np.ones(T["n"], bool)
            rest[parts_o] = False
            assert np.array_equal(got[rest], ref[k][rest]), k
        else:
            assert np.array_equal(got, ref[k]), k
    assert np.all(ref["type"][parts_o] == 5) and np.all(ref["countprogs"][parts_o] == 1)
    del keep


def test_seed_list_alone_and_too_little_room(engine, orc, pkg):
    T, keep, Go, want, par = seed_setup(engine, orc)
    parts_o, groups_o, _ = R.fof_seed(Go["Mass"], Go["MassType"], Go["LenType"], want["seed_index"], None, None, ATIME, None, par)
    parts, groups, nwarn = engine.dev_fof_seed(engine_params(pkg, par), ATIME, None)           # cols = NULL: the list only
    assert np.array_equal(parts.cpu().numpy(), parts_o) and np.array_equal(groups.cpu().numpy(), groups_o) and nwarn == 0
    cols = seed_columns(T)
    d = {k: dev(v) for k, v in cols.items()}
    with pytest.raises(pkg.EngineError, match="more room") as e:
        engine.dev_fof_seed(engine_params(pkg, par), ATIME, d, cap=len(parts_o) - 1)
    engine.synchronize()
    assert e.value.nseeds == len(parts_o)
    for k, v in d.items():                                                                      # nothing was converted
        assert np.array_equal(v.cpu().numpy().view(cols[k].dtype), cols[k]), k
    # NULL output columns are skipped: type alone
    parts, _, _ = engine.dev_fof_seed(engine_params(pkg, par), ATIME, dict(type=d["type"]))
    engine.synchronize()
    t = cols["type"].copy()
    t[parts_o] = 5
    assert np.array_equal(d["type"].cpu().numpy(), t)
    # ... and now these rows are no gas any more: the reference's endrun(7772), before anything is written
    with pytest.raises(pkg.EngineError, match="no gas"):
        engine.dev_fof_seed(engine_params(pkg, par), ATIME, d)
    engine.synchronize()
    for k, v in d.items():
        if k != "type":
            assert np.array_equal(v.cpu().numpy().view(cols[k].dtype), cols[k]), k
    del keep


def test_error_returns(orc, pkg):
    """On an engine of its own (no random table yet)."""
    eng = pkg.Engine(0)
    try:
        T = S.particles("seeds")
        par = dict(MinFoFMassForNewSeed=0.0, MinMStarForNewSeed=0.0, SeedBlackHoleMass=0.05, MaxSeedBlackHoleMass=0.0, SeedBlackHoleMassIndex=-1.5,
                   SeedBHDynMass=0.0)
        keep = dict(pos=dev(T["pos"]), mass=dev(T["mass"]), type=dev(T["type"]))
        eng.dev_bind_particles(keep["pos"], keep["mass"], T["box"], type=keep["type"])
        with pytest.raises(pkg.EngineError, match="no mpg_dev_fof_fof since the particles were bound"):
            eng.dev_fof_subgrid(1)
        keep2, _, G = run_fof(eng, T)
        ng = len(G["MinID"])
        with pytest.raises(pkg.EngineError, match="no mpg_dev_fof_subgrid since the last mpg_dev_fof_fof"):
            eng.dev_fof_seed(engine_params(pkg, par), ATIME, None)
        run_subgrid(eng, T, ng, 1)
        cols = {k: dev(v) for k, v in seed_columns(T).items()}
        with pytest.raises(pkg.EngineError, match="random table"):
            eng.dev_fof_seed(engine_params(pkg, dict(par, MaxSeedBlackHoleMass=0.9)), ATIME, cols)
        assert np.array_equal(cols["type"].cpu().numpy(), T["type"])
        parts, _, _ = eng.dev_fof_seed(engine_params(pkg, par), ATIME, None)
        assert len(parts) >= 3
        # a new FOF: the sums of the old one are gone
        keep3, _, _ = run_fof(eng, T)
        with pytest.raises(pkg.EngineError, match="no mpg_dev_fof_subgrid"):
            eng.dev_fof_seed(engine_params(pkg, par), ATIME, None)
        # particles bound again, with the same count or another: the catalogue belongs to the ones it was made of
        eng.dev_bind_particles(keep["pos"], keep["mass"], T["box"], type=keep["type"])
        with pytest.raises(pkg.EngineError, match="fof_subgrid"):
            eng.dev_fof_subgrid(ng)
        eng.dev_bind_particles(keep["pos"][:-1], keep["mass"][:-1], T["box"], type=keep["type"][:-1])
        with pytest.raises(pkg.EngineError, match="fof_subgrid"):
            eng.dev_fof_subgrid(ng)
        eng.synchronize()
        del keep2, keep3
    finally:
        eng.close()
