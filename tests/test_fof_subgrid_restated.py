"""The restatement of the sub-grid group sums and of black-hole seeding (tests/fof_subgrid_restated.py) on the CPU: hand-made groups with
hand-computed answers; the reference's own order and types against the long-double sums within the bounds the GPU tests assert, on every
set those tests use (so the reference alone stays inside them); the seed rule of both modes on distinct densities."""
import numpy as np
import pytest

import fof_subgrid_restated as R
import fof_subgrid_scenes as S


def hand_made():
    # particle:        0    1    2    3    4    5    6    7    8
    group = np.array([0, 0, 0, 1, 1, -1, 1, 0, 1])
    ptype = np.array([1, 0, 0, 0, 4, 0, 5, 4, 5])
    mass = np.array([1, 0.5, 0.25, 2, 4, 8, 1, 0.5, 1], np.float32)
    met = np.zeros((9, 9), np.float32)
    met[:, 0] = [0, 0.5, 0.25, 0.125, 0.5, 1, 0, 0.25, 0]
    met[:, 8] = [0, 1, 1, 1, 2, 1, 0, 4, 0]
    P = dict(sfr=np.array([9, 1, 2, 4, 9, 8, 9, 9, 9.]), metallicity=np.array([9, 0.5, 0.25, 0.125, 0.5, 1, 9, 0.25, 9]), metals=met,
             heiii_ionized=np.array([1, 1, 0, 1, 1, 1, 1, 1, 1], np.uint8), bh_mass=np.array([9, 9, 9, 9, 9, 9, 0.5, 9, 0.25]),
             bh_mdot=np.array([9, 9, 9, 9, 9, 9, 2, 9, 4.]), density=np.array([99, 3, 3, 7, 99, 50, 99, 99, 99.]),
             delaytime=np.array([0, 0, 0, 1, 0, 0, 0, 0, 0.]))
    return group, ptype, mass, P


@pytest.mark.parametrize("mode", ["ld", "ref"])
def test_hand_made_groups(mode):
    group, ptype, mass, P = hand_made()
    r = R.group_sums(group, 2, mass, ptype, P, wind_decouple=1, mode=mode)
    assert r["Length"].tolist() == [4, 4]
    assert r["Sfr"].tolist() == [3, 4]                                       # gas rows 1, 2 | 3 (row 5 is in no group)
    assert r["GasMetalMass"].tolist() == [0.5 * 0.5 + 0.25 * 0.25, 0.125 * 2]
    assert r["GasMetalElemMass"][:, 0].tolist() == [0.3125, 0.25] and r["GasMetalElemMass"][:, 8].tolist() == [0.75, 2.0]
    assert r["GasMetalElemMass"][:, 1:8].max() == 0
    assert r["MassHeIonized"].tolist() == [0.5, 2.0]                         # row 2 is not ionised
    assert r["StellarMetalMass"].tolist() == [0.125, 2.0]
    assert r["StellarMetalElemMass"][:, 0].tolist() == [0.125, 2.0] and r["StellarMetalElemMass"][:, 8].tolist() == [2.0, 8.0]
    assert r["BH_Mass"].tolist() == [0, 0.75] and r["BH_Mdot"].tolist() == [0, 6]
    # group 0: rows 1 and 2 tie at 3: the smaller index (and the first strict maximum in particle order); group 1: its one gas row is decoupled
    assert r["MaxDens"].tolist() == [3, 0] and r["seed_index"].tolist() == [1, -1]
    r = R.group_sums(group, 2, mass, ptype, P, wind_decouple=0, mode=mode)
    assert r["MaxDens"].tolist() == [3, 7] and r["seed_index"].tolist() == [1, 3]
    # the reference's tie follows the order of arrival; the defined rule does not
    md, si = R.first_strict_maximum([2, 1, 0, 3, 4, 5, 6, 7, 8], group, 2, ptype, P)
    assert md.tolist() == [3, 7] and si.tolist() == [2, 3]
    # absent columns read as zeros; without density no group has a seed
    r = R.group_sums(group, 2, mass, ptype, dict(sfr=P["sfr"]), mode=mode)
    assert r["Sfr"].tolist() == [3, 4] and r["seed_index"].tolist() == [-1, -1] and r["MaxDens"].tolist() == [0, 0]
    assert all(np.all(r[k] == 0) for k in R.SUMS if k != "Sfr")


def test_hand_made_seeding():
    par = dict(MinFoFMassForNewSeed=5.0, MinMStarForNewSeed=1.0, SeedBlackHoleMass=1e-3, MaxSeedBlackHoleMass=0.0, SeedBlackHoleMassIndex=-2.0,
               SeedBHDynMass=0.0)
    mass = np.array([5.0, 4.999, 9, 9, 9])
    mtype = np.zeros((5, 6))
    mtype[:, 4] = [1.0, 3, np.nextafter(1.0, 0), 2, 2]
    ltype = np.zeros((5, 6), np.int32)
    ltype[3, 5] = 1
    seed = np.array([3, 1, 2, 0, -1])
    assert R.seed_marks(mass, mtype, ltype, seed, par).tolist() == [0]      # at the mass threshold: kept; below it, too few stars, a black
    #                                                                         hole, no seed row: dropped
    n = 6
    cols = dict(id=np.array([10, 11, 12, (1 << 64) - 10, 14, 15], np.uint64), tb_hydro=np.arange(n, dtype=np.uint8) + 30, type=np.zeros(n, np.uint8),
                mass=np.full(n, 0.5, np.float32))
    for k in ("bh_mass", "mseed", "mdot", "formationtime", "bh_density", "df_surroundingrmsvel", "df_surroundingdensity", "mtrack",
              "kineticfdbkenergy", "vdisp"):
        cols[k] = np.full(n, 42.0)
    for k in ("minpotpos", "dfaccel", "df_surroundingvel", "dragaccel"):
        cols[k] = np.full((n, 3), 42.0)
    cols.update(swallowid=np.zeros(n, np.uint64), tb_dynfric=np.zeros(n, np.uint8), jumptominpot=np.full(n, 42, np.int32),
                countprogs=np.full(n, 42, np.int32))
    pos = np.arange(18.).reshape(6, 3)
    before = {k: v.copy() for k, v in cols.items()}
    parts, groups, nwarn = R.fof_seed(mass, mtype, ltype, seed, cols, pos, 0.25, None, par)
    assert parts.tolist() == [3] and groups.tolist() == [0] and nwarn == 0
    assert cols["type"].tolist() == [0, 0, 0, 5, 0, 0] and cols["bh_mass"][3] == 1e-3 == cols["mseed"][3] and cols["mdot"][3] == 0
    assert cols["formationtime"][3] == 0.25 and cols["swallowid"][3] == np.uint64((1 << 64) - 1) and cols["tb_dynfric"][3] == 33
    assert cols["minpotpos"][3].tolist() == [9, 10, 11] and cols["countprogs"][3] == 1 and cols["mtrack"][3] == -1 and cols["mass"][3] == 0.5
    for k, v in cols.items():                                                # every other row untouched
        assert np.array_equal(np.delete(v, 3, axis=0), np.delete(before[k], 3, axis=0)), k
    # SeedBHDynMass: the old mass is tracked, the new one is a float; the warning when the dynamic mass is below either
    cols = {k: v.copy() for k, v in before.items()}
    par2 = dict(par, SeedBHDynMass=0.1)
    _, _, nwarn = R.fof_seed(mass, mtype, ltype, seed, cols, pos, 0.25, None, par2)
    assert cols["mtrack"][3] == 0.5 and cols["mass"][3] == np.float32(0.1) and nwarn == 1
    # the power law: w = table[(ID + 23) % size] with the sum wrapped: (2^64 - 10 + 23) % 2^64 = 13 -> table[13 % 7 = 6]
    table = np.array([0.1, 0.2, 0.3, 0.4, 0.5, 0.6, 0.75])
    par3 = dict(par, MaxSeedBlackHoleMass=4e-3)
    cols = {k: v.copy() for k, v in before.items()}
    R.fof_seed(mass, mtype, ltype, seed, cols, pos, 0.25, table, par3)
    # index -2: M = 1 / (1 / M0 - w (1 / M0 - 1 / M1)) = 1 / (1000 - 0.75 * 750)
    assert abs(cols["bh_mass"][3] / (1 / 437.5) - 1) < 1e-14
    # a seed row that is no gas: the reference ends the run
    cols = {k: v.copy() for k, v in before.items()}
    cols["type"][3] = 4
    with pytest.raises(R.SeedError):
        R.fof_seed(mass, mtype, ltype, seed, cols, pos, 0.25, None, par)
    assert all(np.array_equal(cols[k], before[k]) for k in cols if k != "type")


@pytest.mark.parametrize("scene", S.SUM_SCENES, ids=lambda s: "%s-%s%s" % (s[0], s[1], "-highids" if s[2] else ""))
def test_reference_types_stay_inside_the_bounds(orc, scene):
    """The reference's sequential fp64 sums within L 2^-52 sum|term| of the long-double sums; its three float members within the same bound at
    float's precision, L 2^-23 sum|term| (the engine's fp64 sums of them are held to 2^-52)."""
    T = S.particles(*scene)
    _, G, group = S.membership(orc, T)
    ng = len(G["MinID"])
    assert ng >= 3
    for wd in (0, 1):
        ld = R.group_sums(group, ng, T["mass"], T["type"], T["P"], wd, "ld")
        ref = R.group_sums(group, ng, T["mass"], T["type"], T["P"], wd, "ref")
        assert np.array_equal(ld["Length"], G["Length"])
        for k in R.SUMS:
            eps = 2.0 ** -23 if k in R.FLOAT_MEMBERS else 2.0 ** -52
            err = np.abs(ref[k].astype(np.longdouble) - ld[k])
            assert np.all(err <= R.sum_bound(ld["Length"], ld["abs_" + k], eps)), (k, wd)
        # the densities of a set are distinct (a continuous draw): both modes, and the reference under any order of arrival, agree
        assert np.array_equal(ld["MaxDens"], ref["MaxDens"]) and np.array_equal(ld["seed_index"], ref["seed_index"])
        gas = T["type"] == 0
        assert len(np.unique(T["P"]["density"][gas])) == gas.sum()
        for seed in (1, 2):
            md, si = R.first_strict_maximum(np.random.RandomState(seed).permutation(T["n"]), group, ng, T["type"], T["P"], wd)
            assert np.array_equal(md, ld["MaxDens"]) and np.array_equal(si, ld["seed_index"])
    assert (ld["seed_index"] >= 0).sum() >= 2


def test_the_sets_have_the_shapes_they_are_for(orc):
    """Where the groups lie among the 64-row waves and 256-row blocks of the catalogue's label order."""
    def rows(T):
        _, G, group = S.membership(orc, T)
        label = np.where(group >= 0, G["MinID"][np.maximum(group, 0)], T["ids"])
        order = np.argsort(label, kind="stable")
        return G, group[order]
    for name in ("minlen1", "minlen2"):
        G, g = rows(S.particles(name))
        per_wave = [len(np.unique(g[w:w + 64][g[w:w + 64] >= 0])) for w in range(0, len(g), 64)]
        assert max(per_wave) >= 8
        assert (g < 0).any() == (name == "minlen2") and G["Length"].min() == (1 if name == "minlen1" else 2)
    G, g = rows(S.particles("wave64", "label"))
    assert np.all(g[:64] < 0) and len(set(g[64:128])) == 1 and g[64] >= 0 and g[128] != g[64] and G["Length"][g[64]] == 64
    assert g[-1] >= 0                                                          # a group ends on the last row
    T = S.particles("big700", "label")
    G, g = rows(T)
    big = np.argmax(G["Length"])
    at = np.nonzero(g == big)[0]
    assert len(at) == 700 and at[0] % 64 != 0 and at[-1] // 256 - at[0] // 256 >= 2 and g[-1] >= 0
    assert ((G["LenType"][:, 1] == G["Length"]) & (G["Length"] == 40)).any()   # a group of dark matter only
    H = S.particles("big700", "shuffle", True)
    assert H["ids"].min() > np.uint64(1 << 63) and (H["ids"] + np.uint64(23)).min() < np.uint64(23)
    F = S.with_flags(S.particles("minlen2"))
    _, group = rows(F)[0], S.membership(orc, F)[2]
    assert np.all(group[F["flags"] != 0] < 0) and (F["flags"] & 1).sum() >= 5 and (F["flags"] & 2).sum() >= 5
