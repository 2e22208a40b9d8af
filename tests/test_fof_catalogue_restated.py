"""The block tables of the FOF group catalogue (mp-gadget_amd/fof_catalogue.py) against the list of names read off the reference's two
registrations (tests/golden/fof_catalogue_blocks.txt: petaio.c:986-1080, fofpetaio.c:538-568), the wraps of the restatement the GPU tests
compare with (tests/fof_catalogue_restated.py) at their edges, and the refusals of save_fof_catalogue that need no engine.  No GPU."""
import os

import numpy as np
import pytest

import fof_catalogue_restated as R

HERE = os.path.dirname(os.path.abspath(__file__))
BOX = 1000.0


def golden():
    rows = []
    with open(os.path.join(HERE, "golden", "fof_catalogue_blocks.txt")) as f:
        for line in f:
            if line.strip() and not line.startswith("#"):
                t, name, dtype, nmemb, required, cond = line.split()
                rows.append((t, name, dtype, int(nmemb), int(required), cond))
    return rows


def as_rows(blocks):
    return [(str(b.ptype), b.name, b.dtype, b.nmemb, b.required, b.cond) for b in blocks]


def test_tables_equal_the_golden_list(pkg):
    F = pkg.fof_catalogue
    g = golden()
    assert as_rows(F.PIG_BLOCKS) == [r for r in g if r[0] != "FOFGroups"]
    assert as_rows(F.GROUP_BLOCKS) == [r for r in g if r[0] == "FOFGroups"]
    assert len(F.GROUP_BLOCKS) == 18 and len({(b.ptype, b.name) for b in F.PIG_BLOCKS}) == len(F.PIG_BLOCKS)
    assert {r[5] for r in g} <= set(F.CONDITIONS)


@pytest.mark.parametrize("metal", [0, 1])
def test_registered_blocks_by_metal_return(pkg, metal):
    """what the reference registers with MetalReturnOn 0 and 1, the other switches at the reference's defaults: the golden lines whose
    condition holds, by type and then by registration"""
    F = pkg.fof_catalogue
    opt = dict(F.DEFAULT_OPTIONS, MetalReturnOn=metal)
    g = [r for r in golden() if r[5] == "always" or opt[r[5]]]
    pig = [r for r in g if r[0] != "FOFGroups"]
    want = sorted(pig, key=lambda r: (int(r[0]), pig.index(r)))
    assert as_rows(F.pig_blocks(MetalReturnOn=metal)) == want
    assert as_rows(F.group_blocks(MetalReturnOn=metal)) == [r for r in g if r[0] == "FOFGroups"]
    names = {b.name for b in F.group_blocks(MetalReturnOn=metal)}
    assert ({"GasMetalMass", "StellarMetalMass", "GasMetalElemMass", "StellarMetalElemMass"} <= names) == bool(metal)
    assert (("0", "Metals", "f4", 9, 0, "MetalReturnOn") in as_rows(F.pig_blocks(MetalReturnOn=metal))) == bool(metal)
    assert len(F.group_blocks(MetalReturnOn=metal)) == (18 if metal else 14)


def test_wrap_edges():
    ulp = np.nextafter(BOX, np.inf) - BOX
    assert R.wrap_double_one(0.0, BOX) == (BOX, True)
    assert R.wrap_double_one(BOX, BOX) == (BOX, True)
    x, ok = R.wrap_double_one(-0.0, BOX)
    assert ok and x == BOX and not np.signbit(x)
    x, ok = R.wrap_double_one(BOX + ulp, BOX)
    assert ok and x == ulp and 0 < x < 1e-12
    for k in range(-5, 6):
        for frac in (0.0, 0.25, 1e-9, 0.999999):
            x, ok = R.wrap_double_one((k + frac) * BOX, BOX)
            assert ok and 0 < x <= BOX
            y, ok = R.wrap_float_one(np.float32((k + frac) * BOX), BOX)
            assert ok and 0 < float(y) <= BOX and isinstance(y, np.float32)
    # the bound: 64 trips bring a value 64 boxes out home, not one 100 boxes out; nothing that is not finite passes
    assert R.wrap_double_one(64.5 * BOX, BOX) == (0.5 * BOX, True) and R.wrap_double_one(-63.5 * BOX, BOX) == (0.5 * BOX, True)
    for bad in (100.5 * BOX, -100.5 * BOX, np.nan, np.inf, -np.inf):
        assert not R.wrap_double_one(bad, BOX)[1] and not R.wrap_float_one(np.float32(bad), BOX)[1]
    pos = np.array([[1.0, 2.0, 3.0], [4.0, np.nan, 5.0], [100.5 * BOX, 0.0, 0.0]])
    with pytest.raises(R.WrapError) as e:
        R.get_position(pos, (0.0, 0.0, 0.0), BOX)
    assert e.value.row == 1


def test_firstpos_wrap_is_in_float_not_in_double():
    """GTFirstPos wraps its FLOAT out (fofpetaio.c:479-481): rounding to float before the loop and after every step is not rounding once at
    the end.  A value on which the two differ (found by search, kept here) guards against restating the getter in double."""
    first, off = np.float32(511.8216247558594), 1351.391
    f = R.get_firstpos(np.array([[first] * 3], np.float32), (off,) * 3, BOX)[0, 0]
    d = np.float32(R.wrap_double_one(np.float64(first) - off, BOX)[0])
    assert f.dtype == np.float32 and f != d
    assert float(f) == 160.43060302734375 and float(d) == 160.4306182861328


def test_order_restated_keeps_equal_keys_in_index_order():
    grnr = np.array([3, -1, 3, 0, 3, 0, 7, 3], np.int64)
    ptype = np.array([1, 1, 0, 1, 1, 7, 1, 1], np.uint8)
    flags = np.array([0, 0, 0, 0, 1, 0, 2, 0], np.uint8)
    perm, count, ing = R.pig_order(grnr, ptype, flags)
    assert perm.tolist() == [2, 3, 0, 7] and count.tolist() == [1, 3, 0, 0, 0, 0] and ing.tolist() == [1, 5, 0, 0, 0, 0]


class NoEngine:
    """stands where the engine would: any use of it fails the test"""

    def __getattr__(self, name):
        raise AssertionError("the engine was touched (%s)" % name)


def columns_of(pkg, ptypes, **options):
    """a stand-in column (no tensor is looked at before the checks) for every required block"""
    F = pkg.fof_catalogue
    return {b.name: object() for b in F.pig_blocks(**options) if b.ptype in ptypes and b.required and not b.derived}


def test_save_refuses_unknown_and_missing_columns_without_the_engine(pkg, tmp_path):
    F = pkg.fof_catalogue
    path = str(tmp_path / "cat")
    cols = columns_of(pkg, range(6))
    with pytest.raises(pkg.EngineError, match="no block of the table takes the column.*Entropy"):
        F.save_fof_catalogue(NoEngine(), path, dict(cols, Entropy=object()), 0.5, 1.0)
    with pytest.raises(pkg.EngineError, match=r"no block of the table takes the column.*1/Density"):
        F.save_fof_catalogue(NoEngine(), path, {**cols, (1, "Density"): object()}, 0.5, 1.0)
    with pytest.raises(pkg.EngineError, match="no block of the table takes the column.*Metals"):     # (not registered without MetalReturnOn)
        F.save_fof_catalogue(NoEngine(), path, dict(cols, Metals=object()), 0.5, 1.0, MetalReturnOn=0)
    short = {k: v for k, v in cols.items() if k not in ("ID", "BlackholeMass")}
    with pytest.raises(pkg.EngineError, match="required block.*left out: 0/ID, 1/ID, 2/ID, 3/ID, 4/ID, 5/ID, 5/BlackholeMass"):
        F.save_fof_catalogue(NoEngine(), path, short, 0.5, 1.0)
    # optional and derived blocks may be left out, GroupID needs no column: the descriptors of a DM-only catalogue
    dm = columns_of(pkg, (1,))
    assert set(dm) == {"Mass", "Position", "Velocity", "ID"}
    with pytest.raises(pkg.EngineError, match="unknown option"):
        F.build_descriptors(dm, ptypes=(1,), NoSuchSwitch=1)
    assert not os.path.exists(path)
