"""GPU tests of the group catalogue on disk (csrc/fof_catalogue.hip: k_cat_keys + the radix sort, k_cat_gather, k_cat_group_block;
mpg_dev_fof_pig_order, mpg_dev_gather_block, mpg_dev_fof_save_groups) against the numpy restatement of fofpetaio.c / petaio.c
(tests/fof_catalogue_restated.py, held to its edges by tests/test_fof_catalogue_restated.py).

Bounds: EVERYTHING is bit for bit.  Every operation of the order, of the getters and of the header is a comparison, a cast, one subtraction,
one product or a repeated addition of the same operand in the same order, so no tolerance is owed.  The one check with a bound is the one
that does not use the restatement (test_catalogue_is_consistent_with_itself): the fp64 sum of a group's run of the f4 Mass block against the
f4 MassByType, within 2^-23 relative - the table's sum is fp64 over the same widened floats (any order: L 2^-53 relative, L <= 400) and is
then cast once to f4 (2^-24 relative)."""
import hashlib
import os

import numpy as np
import pytest

import fof_catalogue_restated as R

pytestmark = pytest.mark.gpu

BOX, LL, MINLEN = 1000.0, 1.0, 8
ATIME, HUBBLE = 0.3125, 0.7
OFFSET = (123.5, -77.25, 300.0)
HEADER = dict(MassTable=(0.0, 0.0321, 0.0, 0.0, 0.0, 0.0), OmegaLambda=0.7186, Omega0=0.2814, HubbleParam=0.697, CMBTemperature=2.7255, OmegaBaryon=0.0464)
TORCH_VIEW = {"uint64": np.int64, "uint32": np.int32}                     # (torch has no unsigned 32- and 64-bit types: the same bits)


def dev(a):
    import torch
    if a is None:
        return None
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(TORCH_VIEW.get(a.dtype.name, a.dtype)).copy()).cuda()


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype.itemsize == b.dtype.itemsize and a.tobytes() == b.tobytes()


def bind(engine, n, ptype, rng):
    keep = (dev(rng.uniform(0, BOX, (n, 3))), dev(np.ones(n, np.float32)), dev(ptype))
    engine.dev_bind_particles(keep[0], keep[1], BOX, type=keep[2])
    return keep


# ---- 1. the order --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["mixed", "one_group", "no_group", "flagged"])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257, 4097])
def test_order(engine, n, case):
    """explicit GrNr, no FOF run: count, in_group and perm exact; equal (type, GrNr) in ascending index; rows of type 7 skipped; flagged rows
    inside groups out of count and in in_group; no row in any group: all counts 0 and an empty perm"""
    rng = np.random.default_rng(1000 * n + len(case))
    ptype = rng.choice([0, 1, 4, 5, 7], n, p=[0.25, 0.4, 0.15, 0.1, 0.1]).astype(np.uint8)
    grnr = rng.choice([-1, 0, 1, 2 ** 16, 2 ** 31 - 2], n).astype(np.int64)
    flags = np.zeros(n, np.uint8)
    if case == "one_group":
        grnr[:] = 1
    elif case == "no_group":
        grnr[:] = -1
    elif case == "flagged":
        flags = rng.choice([0, 1, 2, 3], n, p=[0.55, 0.15, 0.15, 0.15]).astype(np.uint8)
    keep = bind(engine, n, ptype, rng)
    perm, count, ing = engine.dev_fof_pig_order(grnr=dev(grnr), flags=dev(flags) if case == "flagged" else None)
    want, wcount, wing = R.pig_order(grnr, ptype, flags)
    assert count.tolist() == wcount.tolist() and ing.tolist() == wing.tolist()
    assert perm.cpu().numpy().tolist() == want.tolist()
    if case == "no_group":
        assert count.sum() == 0 and ing.sum() == 0 and perm.shape[0] == 0
    if case == "flagged" and n >= 257:
        assert (ing - count).sum() > 0
    if n >= 63 and case != "no_group":                                     # equal keys are there, and they ascend
        p = want
        key = ptype[p].astype(np.int64) * 2 ** 32 + grnr[p]
        assert (np.diff(key) == 0).any() and np.all(np.diff(p)[np.diff(key) == 0] > 0)
    del keep


def test_order_refuses_a_group_number_that_does_not_fit(engine):
    rng = np.random.default_rng(3)
    grnr = np.array([0, 5, 2 ** 32, 1, 2 ** 32], np.int64)
    keep = bind(engine, 5, np.ones(5, np.uint8), rng)
    with pytest.raises(Exception, match="GrNr of row 2 does not fit 32 bits"):
        engine.dev_fof_pig_order(grnr=dev(grnr))
    del keep


# ---- 2. the gather -------------------------------------------------------------------------------------------------------------------------
NSRC = 5000
GOFF = (0.5, -0.25, 0.0)


def gather_sources():
    rng = np.random.default_rng(11)
    wide = lambda shape: rng.standard_normal(shape) * 10.0 ** rng.uniform(-30, 30, shape)
    ids = rng.integers(0, 2 ** 63, NSRC, dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, NSRC, dtype=np.uint64)
    ids[::3] |= np.uint64(2 ** 63)
    grnr = rng.choice([-1, 0, 1, 2 ** 16, 2 ** 31 - 2, 2 ** 32 - 1], NSRC).astype(np.int64)
    pos = rng.uniform(-5 * BOX, 6 * BOX, (NSRC, 3))
    ulp_up = np.nextafter(BOX, np.inf)
    pos[0] = GOFF                                                            # - offset: exactly 0 -> Box
    pos[1] = [BOX + GOFF[0], BOX + GOFF[1], BOX]                             # exactly Box -> Box
    pos[2] = [GOFF[0], GOFF[1], -0.0]                                        # -0.0 - 0.0 = -0.0 -> Box
    pos[3] = [ulp_up + 0.5, GOFF[1], ulp_up]                                 # Box + ulp -> ulp
    pos[4] = [-5 * BOX + 0.5, 5 * BOX - 0.25, -4.999 * BOX]
    return dict(f64=wide(NSRC), f32=(rng.standard_normal(NSRC) * 10.0 ** rng.uniform(-20, 20, NSRC)).astype(np.float32),
                f64x3=wide((NSRC, 3)), f64x9=wide((NSRC, 9)), f32x9=(rng.standard_normal((NSRC, 9)) * 10.0 ** rng.uniform(-20, 20, (NSRC, 9))).astype(np.float32),
                u64=ids, i64=grnr, u8=rng.integers(0, 256, NSRC).astype(np.uint8), i32=rng.integers(-2 ** 31, 2 ** 31, NSRC).astype(np.int32), pos=pos)


# every (source, destination) pair the two tables use, with the member counts 1, 3 and 9
PAIRS = [("f32", "f4", "NONE"), ("f64", "f4", "NONE"), ("f64x9", "f4", "NONE"), ("f32x9", "f4", "NONE"), ("f64x3", "f8", "NONE"), ("u64", "u8", "NONE"),
         ("i64", "u4", "GROUPID"), ("u8", "u1", "NONE"), ("u8", "u4", "NONE"), ("i32", "i4", "NONE"), ("f64x3", "f4", "VELOCITY"), ("pos", "f8", "POSITION")]


def make_perm(count, rng):
    """reversed runs (the first holds the rows of the edge values), repeats, random rows"""
    if count == 0:
        return np.zeros(0, np.int32)
    parts = [np.arange(min(count, 70))[::-1], np.full(9, 7), np.arange(2000, 2100)[::-1], rng.integers(0, NSRC, count), np.full(3, NSRC - 1)]
    p = np.concatenate(parts)[:count]
    if count > 200:
        p[-3:] = NSRC - 1
    return p.astype(np.int32)


@pytest.fixture(scope="module")
def sources():
    src = gather_sources()
    return src, {k: dev(v) for k, v in src.items()}


@pytest.mark.parametrize("count", [0, 1, 63, 64, 65, 4097])
def test_gather(engine, pkg, sources, count):
    src, dsrc = sources
    rng = np.random.default_rng(count)
    keep = bind(engine, NSRC, np.ones(NSRC, np.uint8), rng)
    perm = make_perm(count, rng)
    dperm = dev(perm)
    for pec in (1, 0):
        par = pkg.engine.fof_catalogue_params(ATIME, HUBBLE, CurrentParticleOffset=GOFF, UsePeculiarVelocity=pec)
        for name, dtype, conv in PAIRS:
            if pec == 0 and conv != "VELOCITY":
                continue
            got = engine.dev_gather_block(dperm, dsrc[name], dtype, conv, par, src_dtype="u8" if name == "u64" else None).cpu().numpy()
            want = R.gather(perm, src[name], dtype, conv, GOFF, BOX, ATIME, pec)
            assert same_bits(got, want), (name, dtype, conv, count, pec)
    if count >= 5:                                                           # the edge rows went through the POSITION gather as stated
        want = R.gather(perm, src["pos"], "f8", "POSITION", GOFF, BOX)
        j = {int(r): k for k, r in enumerate(perm[:70])}
        assert want[j[0]].tolist() == [BOX] * 3 and want[j[1]].tolist() == [BOX] * 3 and want[j[2]][2] == BOX and not np.signbit(want[j[2]][2])
        assert want[j[3]][2] == np.nextafter(BOX, np.inf) - BOX and np.all((want > 0) & (want <= BOX))
    del keep


@pytest.mark.parametrize("bad", [100.5 * BOX, -100.5 * BOX, np.nan, np.inf])
def test_gather_refuses_a_position_it_cannot_wrap(engine, pkg, sources, bad):
    """a value 100 boxes out, or not finite: the error return names the first such row of the block and d_out is untouched"""
    import torch
    src, _ = sources
    rng = np.random.default_rng(5)
    keep = bind(engine, NSRC, np.ones(NSRC, np.uint8), rng)
    pos = src["pos"].copy()
    pos[77, 1] = bad
    perm = make_perm(300, rng)
    perm[[41, 130, 299]] = 77
    assert 77 not in perm[:41]
    out = torch.full((300, 3), 7.0, dtype=torch.float64, device="cuda")
    par = pkg.engine.fof_catalogue_params(ATIME, HUBBLE, CurrentParticleOffset=GOFF)
    with pytest.raises(pkg.EngineError, match=r"block 0/Position: row 41 is not finite or lies more than 64 boxes"):
        engine.dev_gather_block(dev(perm), dev(pos), "f8", "POSITION", par, out=out, name="Position")
    assert np.all(out.cpu().numpy() == 7.0)
    with pytest.raises(R.WrapError) as e:
        R.gather(perm, pos, "f8", "POSITION", GOFF, BOX)
    assert e.value.row == 41
    perm[5] = NSRC                                                          # an index outside the bound particles is refused too, nothing read
    with pytest.raises(pkg.EngineError, match=r"row 5 of the order names a particle outside"):
        engine.dev_gather_block(dev(perm), dev(src["pos"]), "f8", "POSITION", par, out=out, name="Position")
    assert np.all(out.cpu().numpy() == 7.0)
    del keep


# ---- 3. the whole catalogue ----------------------------------------------------------------------------------------------------------------
def make_scene():
    """~6000 rows in a box of 1000: 40 clumps of dark matter (8 .. 300 members within a ball of 0.4 linking lengths: every pair links), one
    of exactly 8 and one of 7 members (no group); gas, stars and a black hole in some clumps and not in others; an unlinked background of
    every type; clumps across the periodic boundary; rows shuffled so that particle order says nothing about groups"""
    rng = np.random.default_rng(20)
    sizes = [8, 7] + [int(x) for x in np.geomspace(9, 300, 38)]
    pos, typ, clump = [], [], []

    def ball(c, k):
        v = rng.standard_normal((k, 3))
        v *= (0.4 * LL * rng.uniform(0, 1, (k, 1)) ** (1 / 3)) / np.linalg.norm(v, axis=1, keepdims=True)
        return (c + v) % BOX

    for c, size in enumerate(sizes):
        centre = np.array([(c % 4) * 250.0 + 0.2, ((c // 4) % 4) * 250.0 + 0.1, (c // 16) * 333.0 + 0.3])
        members = [(1, size)]
        if c >= 2 and c % 3 == 0:
            members += [(0, size // 4 + 1), (4, size // 8 + 1), (5, 1 + (c % 2))]
        elif c >= 2 and c % 3 == 1:
            members += [(0, size // 3 + 2)]
        for t, k in members:
            pos.append(ball(centre, k))
            typ += [t] * k
            clump += [c] * k
    for t, k in ((1, 900), (0, 400), (4, 150), (5, 20)):
        pos.append(rng.uniform(0, BOX, (k, 3)))
        typ += [t] * k
        clump += [-1] * k
    pos, typ, clump = np.concatenate(pos), np.array(typ, np.uint8), np.array(clump)
    n = len(typ)
    sh = rng.permutation(n)
    pos, typ, clump = pos[sh], typ[sh], clump[sh]
    ids = rng.permutation(4 * n)[:n].astype(np.uint64) + np.uint64(1)
    ids[::2] += np.uint64(2 ** 63)
    f = lambda lo, hi, shape=n: rng.uniform(lo, hi, shape)
    mass = np.where(typ == 1, np.float32(0.0321), f(0.004, 0.008).astype(np.float32)).astype(np.float32)
    T = dict(n=n, clump=clump, sizes=sizes, pos=pos, vel=rng.standard_normal((n, 3)) * 200.0, mass=mass, type=typ, ids=ids)
    T["cols"] = dict(Mass=mass, Position=pos, Velocity=T["vel"], ID=ids, Potential=f(-5e4, 0), Generation=rng.integers(0, 4, n).astype(np.uint8),
                     SmoothingLength=f(0.1, 30), Density=f(1e-9, 1e-3), EgyWtDensity=f(1e-9, 1e-3), InternalEnergy=f(1, 1e4), ElectronAbundance=f(0, 1.2),
                     HeIIIIonized=rng.integers(0, 2, n).astype(np.uint8), StarFormationRate=f(0, 3) * (rng.uniform(0, 1, n) < 0.3),
                     Metallicity=f(0, 0.04), Metals=f(0, 0.01, (n, 9)).astype(np.float32), StarFormationTime=f(0.05, ATIME),
                     BlackholeMass=f(1e-5, 1e-2), BlackholeDensity=f(1e-9, 1e-3), BlackholeAccretionRate=f(0, 1e-3),
                     BlackholeProgenitors=rng.integers(1, 9, n).astype(np.int32), BlackholeMinPotPos=f(0, BOX, (n, 3)),
                     BlackholeJumpToMinPot=rng.integers(0, 2, n).astype(np.int32), BlackholeMtrack=f(-1, 1), Swallowed=np.zeros(n, np.uint8),
                     BlackholeSwallowID=np.full(n, 2 ** 64 - 1, np.uint64))
    c = T["cols"]
    T["sub"] = dict(sfr=c["StarFormationRate"], metallicity=c["Metallicity"], metals=c["Metals"], heiii_ionized=c["HeIIIIonized"], bh_mass=c["BlackholeMass"],
                    bh_mdot=c["BlackholeAccretionRate"], density=c["Density"], delaytime=np.zeros(n))
    return T


@pytest.fixture(scope="module")
def scene():
    T = make_scene()
    T["dcols"] = {k: dev(v) for k, v in T["cols"].items()}
    T["dsub"] = {k: dev(v) for k, v in T["sub"].items()}
    T["dbind"] = (dev(T["pos"]), dev(T["mass"]), dev(T["type"]), dev(T["ids"]), dev(T["vel"]))
    return T


def find_groups(engine, T, ll=LL, subgrid=True):
    """bind, dev_fof_fof (without flags: flagged rows are members), dev_fof_subgrid -> GrNr per row, the two tables (numpy, MinID order)"""
    import torch
    p, m, t, ids, vel = T["dbind"]
    engine.dev_bind_particles(p, m, BOX, type=t)
    grnr = torch.zeros(T["n"], dtype=torch.int64, device="cuda")
    ng = engine.dev_fof_fof(ids, ll, MINLEN, vel=vel, grnr=grnr)
    G = engine.dev_fof_groups(ng)
    sub = engine.dev_fof_subgrid(ng, **T["dsub"]) if subgrid else None
    engine.synchronize()                                                      # (the tables are written on the engine's stream)
    G = {k: v.cpu().numpy() for k, v in G.items()}
    G["MinID"] = G["MinID"].view(np.uint64)
    sub = {k: v.cpu().numpy() for k, v in sub.items()} if subgrid else None
    return grnr.cpu().numpy(), G, sub, ng


def expected(pkg, T, grnr, G, sub, flags, nfile, SaveParticles, metal, pec):
    """the restated catalogue: {block: (array, nfile)} and the header"""
    F = pkg.fof_catalogue
    out = {"FOFGroups/" + k: v for k, v in R.group_blocks(G, sub, OFFSET, BOX, ATIME, pec, metal).items()}
    perm, count, ing = R.pig_order(grnr, T["type"], flags)
    off = np.concatenate([[0], np.cumsum(count)])
    if SaveParticles:
        for b in F.pig_blocks(MetalReturnOn=metal):
            col = grnr if b.name == "GroupID" else T["cols"].get(b.name)
            if col is not None:
                out["%d/%s" % (b.ptype, b.name)] = R.gather(perm[off[b.ptype]:off[b.ptype + 1]], col, b.dtype, b.conv, OFFSET, BOX, ATIME, pec)
    hdr = R.header(ing, len(G["GrNr"]), BOX, ATIME, HUBBLE, pec, **HEADER)
    return {k: (v, nfile if len(v) else 0) for k, v in out.items()}, hdr


def save(engine, pkg, T, path, flags=None, nfile=1, SaveParticles=1, metal=1, pec=1):
    cols = {k: v for k, v in T["dcols"].items() if metal or k != "Metals"}
    pkg.fof_catalogue.save_fof_catalogue(engine, path, cols, ATIME, HUBBLE, flags=dev(flags), CurrentParticleOffset=OFFSET, UsePeculiarVelocity=pec,
                                         SaveParticles=SaveParticles, nfile=nfile, header=HEADER, MetalReturnOn=metal)


def check_against_restatement(pkg, path, want, hdr):
    F = pkg.fof_catalogue
    info = F.block_info(path)
    assert sorted(info) == sorted(want)
    header, groups, parts = F.read_fof_catalogue(path)
    for name, (arr, nfile) in want.items():
        i = info[name]
        assert (i["size"], i["nfile"], i["nmemb"]) == (len(arr), nfile, 1 if arr.ndim == 1 else arr.shape[1]), name
        assert np.dtype(i["dtype"]) == arr.dtype, name
        sub, b = name.split("/")
        got = groups[b] if sub == "FOFGroups" else parts[int(sub)][b]
        assert same_bits(got, arr), name
    assert sorted(header) == sorted(hdr) and len(header) == 12
    for k, v in hdr.items():
        assert same_bits(np.asarray(header[k]), np.asarray(v, np.asarray(header[k]).dtype)), k


def scene_flags(T, grnr):
    """3 garbage rows (2 of dark matter, 1 of gas) and 2 swallowed black holes, all inside groups"""
    flags = np.zeros(T["n"], np.uint8)
    inside = np.nonzero(grnr >= 0)[0]
    flags[inside[T["type"][inside] == 1][[3, 700]]] = 1
    flags[inside[T["type"][inside] == 0][5]] |= 1
    flags[inside[T["type"][inside] == 5][[1, 4]]] = 2
    return flags


@pytest.mark.parametrize("variant", ["nfile1", "nfile3_flags", "no_particles", "no_metals_comoving_velocity"])
def test_whole_catalogue(engine, pkg, scene, tmp_path, variant):
    T = scene
    grnr, G, sub, ng = find_groups(engine, T)
    assert ng == 39 and T["n"] > 5500                                         # the clump of 7 is no group, the clump of 8 is one
    assert G["Length"].min() == 8 and not np.any(grnr[T["clump"] == 1] >= 0) and np.all(grnr[T["clump"] == 0] >= 0)
    assert (grnr[T["clump"] < 0] >= 0).sum() == 0 and sorted(G["GrNr"].tolist()) == list(range(1, ng + 1))
    flags = scene_flags(T, grnr) if variant == "nfile3_flags" else None
    kw = dict(nfile1=dict(), nfile3_flags=dict(nfile=3), no_particles=dict(SaveParticles=0), no_metals_comoving_velocity=dict(metal=0, pec=0))[variant]
    path = str(tmp_path / "cat")
    save(engine, pkg, T, path, flags=flags, **kw)
    want, hdr = expected(pkg, T, grnr, G, sub, flags, kw.get("nfile", 1), kw.get("SaveParticles", 1), kw.get("metal", 1), kw.get("pec", 1))
    check_against_restatement(pkg, path, want, hdr)
    blocks = set(want)
    assert ("FOFGroups/GasMetalElemMass" in blocks) == (variant != "no_metals_comoving_velocity")
    if variant == "no_particles":
        assert sorted(os.listdir(path)) == ["FOFGroups", "Header"] and len(blocks) == 18
    else:
        assert {"2/Mass", "3/GroupID", "5/BlackholeMinPotPos", "0/Density", "4/Metallicity"} <= blocks
        assert want["2/Mass"][1] == 0 and len(want["2/Mass"][0]) == 0          # a type without members: blocks of size 0 with NFILE: 0
    if flags is not None:
        assert (hdr["NumPartInGroupTotal"].sum() - sum(len(want["%d/Mass" % t][0]) for t in range(6))) == 5
    t = engine.fof_catalogue_times()
    assert t["group_ms"] > 0 and (t["order_ms"] > 0) and (t["gather_ms"] > 0) == (variant != "no_particles")


def test_catalogue_without_subgrid_call_has_zero_subgrid_blocks(engine, pkg, scene, tmp_path):
    T = scene
    grnr, G, _, ng = find_groups(engine, T, subgrid=False)
    path = str(tmp_path / "cat")
    save(engine, pkg, T, path)
    want, hdr = expected(pkg, T, grnr, G, None, None, 1, 1, 1, 1)
    check_against_restatement(pkg, path, want, hdr)
    for b in R.SUBGRID_OF:
        assert not want["FOFGroups/" + b][0].any()


def test_catalogue_without_any_group(engine, pkg, scene, tmp_path):
    """a linking length so small that nothing links: every block is there with size 0 and NFILE: 0"""
    T = scene
    grnr, G, sub, ng = find_groups(engine, T, ll=1e-7)
    assert ng == 0 and np.all(grnr == -1)
    path = str(tmp_path / "cat")
    save(engine, pkg, T, path)
    want, hdr = expected(pkg, T, grnr, G, sub, None, 1, 1, 1, 1)
    check_against_restatement(pkg, path, want, hdr)
    info = pkg.fof_catalogue.block_info(path)
    assert len(info) > 60 and all(i["size"] == 0 and i["nfile"] == 0 for i in info.values())
    assert hdr["NumFOFGroupsTotal"] == 0 and not hdr["NumPartInGroupTotal"].any()


# ---- 4. independent of the restatement -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flagged", [False, True])
def test_catalogue_is_consistent_with_itself(engine, pkg, scene, tmp_path, flagged):
    T = scene
    grnr, G, sub, ng = find_groups(engine, T)
    flags = scene_flags(T, grnr) if flagged else None
    path = str(tmp_path / "cat")
    save(engine, pkg, T, path, flags=flags)
    header, groups, parts = pkg.fof_catalogue.read_fof_catalogue(path)
    assert groups["GroupID"].tolist() == list(range(1, ng + 1))
    short = np.zeros((ng, 6), np.int64)
    if flagged:
        for i in np.nonzero(flags)[0]:
            short[grnr[i] - 1, T["type"][i]] += 1
        assert short.sum() == 5 and short[:, 5].sum() == 2
    for t in range(6):
        gid = parts[t]["GroupID"].astype(np.int64)
        assert np.all(np.diff(gid) >= 0)
        runs = np.bincount(gid - 1, minlength=ng)[:ng] if len(gid) else np.zeros(ng, np.int64)
        assert np.array_equal(runs, groups["LengthByType"][:, t].astype(np.int64) - short[:, t]), t
        if not flagged and len(gid):
            msum = np.bincount(gid - 1, weights=parts[t]["Mass"].astype(np.float64), minlength=ng)[:ng]
            tab = groups["MassByType"][:, t].astype(np.float64)
            assert np.all(np.abs(msum - tab) <= 2.0 ** -23 * np.abs(msum)), t
    assert header["NumPartInGroupTotal"].tolist() == groups["LengthByType"].astype(np.int64).sum(0).tolist()
    assert len(parts[2]["GroupID"]) == 0 and len(parts[5]["GroupID"]) > 10 and len(parts[0]["GroupID"]) > 200


# ---- 5. repeatability ----------------------------------------------------------------------------------------------------------------------
def tree_hash(path):
    h = {}
    for d, _, files in os.walk(path):
        for f in files:
            with open(os.path.join(d, f), "rb") as fh:
                h[os.path.relpath(os.path.join(d, f), path)] = hashlib.sha256(fh.read()).hexdigest()
    return h


def test_two_calls_write_identical_trees(engine, pkg, scene, tmp_path):
    T = scene
    grnr, _, _, _ = find_groups(engine, T)
    flags = scene_flags(T, grnr)
    save(engine, pkg, T, str(tmp_path / "a"), flags=flags, nfile=3)
    save(engine, pkg, T, str(tmp_path / "b"), flags=flags, nfile=3)
    a, b = tree_hash(str(tmp_path / "a")), tree_hash(str(tmp_path / "b"))
    assert len(a) > 200 and a == b


# ---- 6. errors -----------------------------------------------------------------------------------------------------------------------------
def test_no_catalogue_no_file(pkg, scene, tmp_path):
    """an engine without a FOF run, and one whose particles were bound again with another count: the error return of mpg_dev_fof_subgrid
    from the order (GrNr of the engine) and from the writer, and no file"""
    T = scene
    eng = pkg.Engine(0)
    try:
        p, m, t, ids, vel = T["dbind"]
        eng.dev_bind_particles(p, m, BOX, type=t)
        path = str(tmp_path / "cat")
        with pytest.raises(pkg.EngineError, match="fof_pig_order: no mpg_dev_fof_fof since the particles were bound"):
            eng.dev_fof_pig_order()
        with pytest.raises(pkg.EngineError, match="fof_save_groups: no mpg_dev_fof_fof since the particles were bound"):
            save(eng, pkg, T, path)
        assert not os.path.exists(path)
        eng.dev_fof_fof(ids, LL, MINLEN, vel=vel)
        half = T["n"] // 2
        eng.dev_bind_particles(p[:half].contiguous(), m[:half].contiguous(), BOX, type=t[:half].contiguous())
        with pytest.raises(pkg.EngineError, match="no mpg_dev_fof_fof since the particles were bound|the bound particle count differs"):
            eng.dev_fof_pig_order()
        with pytest.raises(pkg.EngineError, match="no mpg_dev_fof_fof since the particles were bound|the bound particle count differs"):
            save(eng, pkg, T, path)
        assert not os.path.exists(path)
    finally:
        eng.close()
