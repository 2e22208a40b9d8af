"""GPU parity of the excursion-set reionisation model (mpg_dev_calculate_uvbg: k_uvbg_init, k_uvbg_deposit, k_uvbg_filter, k_uvbg_cells,
k_uvbg_readout; csrc/uvbg.hip) and of mpg_dev_fof_set_escapefraction (csrc/fof.hip) with the long-double restatement of uvbg.c:471-594 and
petapm.c:381-577 (tests/uvbg_restated.py).

Bounds, from the formats: the deposited grids within 1e-13 of the largest cell (fp64 sums of a cell's terms in the engine's order); the radii exact; the decisions
(xHI == 0) exact in every cell that has one (tests/test_uvbg_restated.py holds the scenes to having next to no others); J21 within 2 float
ulps (2.4e-7 relative), the partial xHI within 2.4e-7 absolute; local_J21 bit for bit the largest of the 8 corners of the engine's own J21
grid; zreion exact; escfrac within 1e-13 relative, its clamp at 1 exact; rows of other types bit-identical; the neutral fractions within
5e-7 relative (a float ulp per cell of xHI) and identical on two calls."""
import numpy as np
import pytest

import fof_subgrid_scenes as FS
import uvbg_restated as U

pytestmark = pytest.mark.gpu

ULP2 = 2.4e-7
MARGIN, CAP = 1e-9, 1e-3
CONFIGS = ((0, 0, 0), (1, 0, 0), (2, 0, 0), (0, 1, 0), (0, 0, 1))      # (ReionFilterType, RtoMFilterType, ReionUseParticleSFR)


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).copy()).cuda()


def bind(engine, S):
    keep = dict(pos=dev(S["pos"]), mass=dev(np.asarray(S["mass"], np.float32)), type=dev(S["type"]))
    engine.dev_bind_particles(keep["pos"], keep["mass"], S["box"], type=keep["type"])
    return keep


def columns(S, with_sfr=True):
    n = len(S["type"])
    c = dict(escfrac=np.array(S["escfrac"], np.float64), local_J21=np.full(n, -5.0), zreion=np.array(S["zreion"], np.float64))
    if with_sfr:
        c["sfr"] = np.array(S["sfr"], np.float64)
    return c


def run_dev(engine, S, with_sfr=True, bound=None):
    """mpg_dev_calculate_uvbg on the scene -> (result dict, columns as numpy, grids as numpy)"""
    import torch
    keep = bind(engine, S) if bound is None else bound
    cols = {k: dev(v) for k, v in columns(S, with_sfr).items()}
    torch.cuda.synchronize()
    res = engine.dev_calculate_uvbg(S["par"], cols)
    grids = engine.dev_uvbg_grids(S["par"]["UVBGdim"], deposits=True)
    engine.synchronize()
    del keep
    return res, {k: v.cpu().numpy() for k, v in cols.items()}, {k: v.cpu().numpy() for k, v in grids.items()}


def compare(S, r, res, cols, grids, capped=True):
    """every check of the module's docstring: the engine's results (res, cols, grids) against the restatement's r on the scene S"""
    par, dim = S["par"], S["par"]["UVBGdim"]
    ptype = np.asarray(S["type"])
    gas, star = ptype == 0, ptype == 4
    # radii
    assert list(res["radii"]) == list(r["radii"])
    # deposited grids
    for k, name in enumerate(("mass", "star", "sfr")):
        if k < len(r["deposit"]):
            want = r["deposit"][k]
            err = np.abs(grids[name].astype(np.longdouble) - want).max()
            print("%s: deposit %s error %.3g of the largest cell" % (S["name"], name, float(err / np.abs(want).max())))
            assert err <= 1e-13 * np.abs(want).max()
        else:
            assert not grids[name].any()
    # decisions
    have = ~r["degenerate"] & ~(r["margin"] < MARGIN)
    if capped:
        assert (~have).sum() <= CAP * have.size
    ion_e, ion_r = grids["xHI"] == 0, r["xHI"] == 0
    print("%s: %d cells, %d ionised, %d left out; smallest margin %.3g" % (S["name"], have.size, ion_r.sum(), (~have).sum(), r["margin"][have].min()))
    assert np.array_equal(ion_e[have], ion_r[have])
    assert np.isfinite(grids["J21"]).all()
    # J21 where ionised, the partial xHI elsewhere
    sel = have & ion_r
    dj = np.abs(grids["J21"][sel].astype(np.float64) - r["J21"][sel])
    print("%s: J21 error %.3g relative" % (S["name"], (dj / np.abs(r["J21"][sel])).max() if sel.any() else 0.0))
    assert np.all(dj <= ULP2 * np.abs(r["J21"][sel]))
    assert not grids["J21"][have & ~ion_r].any()
    sel = have & ~ion_r
    dx = np.abs(grids["xHI"][sel].astype(np.float64) - r["xHI"][sel])
    print("%s: partial xHI error %.3g" % (S["name"], dx.max() if sel.any() else 0.0))
    assert np.all(dx <= ULP2)
    assert not capped or (sel.any() and (have & ion_r).any())
    # local_J21: the largest corner of the engine's OWN grid, bit for bit; and the restatement's value
    best = U.max_of_corners(grids["J21"], S["pos"], S["box"], dim)
    took = gas & (best > 0)
    assert np.array_equal(cols["local_J21"][gas], np.where(took, best, 0.0)[gas])
    if capped:
        assert np.all(np.abs(cols["local_J21"][gas] - r["local_J21"][gas]) <= ULP2 * np.abs(r["local_J21"][gas]))
        assert took.sum() >= 100
    # zreion
    assert np.array_equal(cols["zreion"], U.zreion_rule(S["zreion"], took, par["Time"]))
    if capped:
        assert np.array_equal(cols["zreion"], r["zreion"])
    # escfrac
    conv = gas | star
    want = r["escfrac"]
    assert np.all(np.abs(cols["escfrac"][conv].astype(np.longdouble) - want[conv]) <= 1e-13 * np.abs(want[conv]))
    assert np.array_equal(cols["escfrac"][conv] == 1, want[conv] == 1) and np.array_equal(cols["escfrac"][conv] == 0, want[conv] == 0)
    # untouched rows
    other = ~gas
    assert np.array_equal(cols["escfrac"][~conv], np.asarray(S["escfrac"])[~conv])
    assert np.all(cols["local_J21"][other] == -5.0) and np.array_equal(cols["zreion"][other], np.asarray(S["zreion"])[other])
    if "sfr" in cols:
        assert np.array_equal(cols["sfr"], S["sfr"])


@pytest.mark.parametrize("cfg", CONFIGS, ids=lambda c: "f%d-m%d-sfr%d" % c)
@pytest.mark.parametrize("name", ["d16", "d24"])
def test_scene(engine, name, cfg):
    """UVBGdim 16 and 24 (no power of two: the Nz / 2 + 1 padding), the three filters, both RtoM forms, with and without the particles' SFR"""
    S = U.scene(name, ReionFilterType=cfg[0], RtoMFilterType=cfg[1], ReionUseParticleSFR=cfg[2])
    r = U.reference(name, *cfg)
    res, cols, grids = run_dev(engine, S, with_sfr=bool(cfg[2]) or cfg[0] == 2)
    compare(S, r, res, cols, grids)
    assert (cols["escfrac"][S["type"] == 4] == 1).sum() >= 5             # the clamp is exercised
    gas_kept = np.array_equal(cols["escfrac"][S["type"] == 0], S["escfrac"][S["type"] == 0])
    assert gas_kept == (not cfg[2])                                       # the reference's `continue`
    for k in ("volume_weighted_global_xHI", "mass_weighted_global_xHI"):
        print("%s %s: %s %.17g (restated %.17g)" % (name, cfg, k, res[k], float(r[k])))
        assert abs(res[k] - float(r[k])) <= 5e-7 * float(r[k])
    res2, cols2, grids2 = run_dev(engine, S, with_sfr=bool(cfg[2]) or cfg[0] == 2)
    assert res2["volume_weighted_global_xHI"] == res["volume_weighted_global_xHI"]
    assert res2["mass_weighted_global_xHI"] == res["mass_weighted_global_xHI"]


def test_void_scene(engine):
    """an empty octant: x / 0 and 0 / 0 stay what C makes of them; the call returns, J21 is finite, every cell that has a decision agrees"""
    S, r = U.scene("void"), U.reference("void")
    res, cols, grids = run_dev(engine, S)
    assert r["degenerate"].sum() >= 100
    compare(S, r, res, cols, grids, capped=False)


def group_mass_of_rows(grnr, G):
    """Mass of the group of every row (0: in no group) from P.GrNr and the group table"""
    mass_of_grnr = np.zeros(int(G["GrNr"].max()) + 1 if len(G["GrNr"]) else 1)
    mass_of_grnr[G["GrNr"]] = G["Mass"]
    return np.where(grnr > 0, mass_of_grnr[np.maximum(grnr, 0)], 0.0)


def test_set_escapefraction_and_the_pair(engine):
    """fof_set_escapefraction after mpg_dev_fof_fof on a clustered set with gas and stars inside and outside groups: the Mass of the row's
    group bit for bit, 0 outside, other types untouched; then calculate_uvbg on that column, end to end"""
    import torch
    T = FS.particles("minlen2")
    typ = np.array(T["type"])
    lone = np.nonzero((np.bincount(T["cluster"])[T["cluster"]] == 1) & (typ == 1))[0]
    typ[lone[::2]] = 4                                                    # stars on their own: in no group
    keep = dict(pos=dev(T["pos"]), mass=dev(T["mass"]), type=dev(typ), ids=dev(np.array(T["ids"]).view(np.int64)))
    engine.dev_bind_particles(keep["pos"], keep["mass"], T["box"], type=keep["type"])
    with pytest.raises(Exception, match="fof_set_escapefraction: no mpg_dev_fof_fof since the particles were bound"):
        engine.dev_fof_set_escapefraction(dev(np.zeros(T["n"])))
    grnr = torch.zeros(T["n"], dtype=torch.int64, device="cuda")
    ng = engine.dev_fof_fof(keep["ids"], T["LL"], T["minlen"], grnr=grnr)
    G = {k: v.cpu().numpy() for k, v in engine.dev_fof_groups(ng).items()}
    esc = dev(np.full(T["n"], -7.0))
    torch.cuda.synchronize()
    engine.dev_fof_set_escapefraction(esc)
    engine.synchronize()
    esc, grnr = esc.cpu().numpy(), grnr.cpu().numpy()
    want = group_mass_of_rows(grnr, G)
    conv = (typ == 0) | (typ == 4)
    assert np.array_equal(esc[conv], want[conv]) and np.all(esc[~conv] == -7.0)
    for t in (0, 4):
        assert ((typ == t) & (grnr > 0)).sum() >= 5 and ((typ == t) & (grnr <= 0)).sum() >= 5
        assert np.all(esc[(typ == t) & (grnr <= 0)] == 0) and np.all(esc[(typ == t) & (grnr > 0)] > 0)
    # a changed particle count
    engine.dev_bind_particles(keep["pos"][:-1], keep["mass"][:-1], T["box"], type=keep["type"][:-1])
    engine.dev_bind_particles(keep["pos"], keep["mass"], T["box"], type=keep["type"])
    with pytest.raises(Exception, match="no mpg_dev_fof_fof since the particles were bound"):
        engine.dev_fof_set_escapefraction(dev(np.zeros(T["n"])))
    # the pair: the halo masses into calculate_uvbg
    par = dict(U.PAR, UVBGdim=16, ReionRBubbleMax=100.0, ReionRBubbleMin=5.0, ReionUseParticleSFR=1, ReionNionPhotPerBary=4.0)
    S = dict(name="fof-pair", pos=np.array(T["pos"]), mass=np.array(T["mass"]), type=typ, sfr=np.array(T["P"]["sfr"]), escfrac=esc,
             zreion=np.full(T["n"], -1.0), box=T["box"], par=par)
    r = U.run(S)
    res, cols, grids = run_dev(engine, S, bound=keep)
    compare(S, r, res, cols, grids, capped=False)
    assert (grids["xHI"] == 0).sum() >= 10 and (cols["local_J21"][typ == 0] > 0).sum() >= 10


def test_host_form(pkg):
    """mpg_calculate_uvbg on a host table equals the device form bit for bit: the deposit gathers in an order the input fixes, so nothing
    depends on the order of arrival (with a deposit by atomics the issue's bound for the grids would be 1e-13 of the largest cell)"""
    S = U.scene("d16", ReionUseParticleSFR=1)
    engine = pkg.Engine(0)
    res, cols, grids = run_dev(engine, S)
    dead = S["type"] == 7
    P = pkg.make_particles(S["pos"], S["mass"], type=np.where(dead, 1, S["type"]))
    P["Flags"][dead] = 1                                                  # garbage: type 7 on the device
    h = columns(S)
    hres = engine.calculate_uvbg(P, S["box"], S["par"], h)
    hg = {k: v.cpu().numpy() for k, v in engine.dev_uvbg_grids(16, deposits=True).items()}
    assert list(hres["radii"]) == list(res["radii"])
    for k in ("sfr", "escfrac", "local_J21", "zreion"):
        assert np.array_equal(h[k], cols[k]), k
    for k in ("mass", "star", "sfr", "J21", "xHI"):
        assert np.array_equal(hg[k], grids[k]), k
    for k in ("volume_weighted_global_xHI", "mass_weighted_global_xHI"):
        assert hres[k] == res[k]
    engine.close()


REFUSALS = ((dict(ReionFilterType=3), "ReionFilterType 3 is undefined"), (dict(ReionFilterType=-1), "ReionFilterType"),
            (dict(RtoMFilterType=2), "RtoMFilterType 2"), (dict(ReionDeltaRFactor=1.0), "ReionDeltaRFactor"),
            (dict(ReionDeltaRFactor=0.9), "ReionDeltaRFactor"), (dict(ReionRBubbleMax=0.0), "ReionRBubbleMax"),
            (dict(ReionRBubbleMin=-1.0), "ReionRBubbleMin"), (dict(UVBGdim=3), "UVBGdim must be at least 4"),
            (dict(UVBGdim=1291), "UVBGdim above 1290"), (dict(NTask=2), "NTask"))


def test_refusals(engine, pkg):
    """every refusal returns its message and names the setting; nothing is written"""
    S = U.scene("d16")
    keep = bind(engine, S)
    for over, text in REFUSALS:
        cols = {k: dev(v) for k, v in columns(S).items()}
        with pytest.raises(pkg.EngineError, match=text):
            engine.dev_calculate_uvbg(dict(S["par"], **over), cols)
        engine.synchronize()
        assert np.array_equal(cols["escfrac"].cpu().numpy(), S["escfrac"])
    cols = {k: dev(v) for k, v in columns(S, with_sfr=False).items()}
    with pytest.raises(pkg.EngineError, match="ReionUseParticleSFR needs the sfr column"):
        engine.dev_calculate_uvbg(dict(S["par"], ReionUseParticleSFR=1), cols)
    with pytest.raises(pkg.EngineError, match="negative escape fraction"):
        engine.dev_calculate_uvbg(dict(S["par"], EscapeFractionNorm=-0.3), cols)
    engine.dev_calculate_uvbg(S["par"], cols)
    with pytest.raises(pkg.EngineError, match="dim differs from the UVBGdim of the last"):
        engine.dev_uvbg_grids(24)
    del keep
