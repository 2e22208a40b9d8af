"""The Peano-Hilbert state machine generated for the device (mp-gadget_amd/csrc/peano_tables.h, made by tools/gen_peano_tables.py)
against golden vectors taken from the reference function (tests/golden/peano_keys.npz, make_peano_golden.py, and the random
triplets of every bit count in tests/golden/reference_leaf.npz, make_reference_golden.py).  CPU only: the tables are parsed from the header."""
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def load_tables():
    txt = open(os.path.join(ROOT, "mp-gadget_amd", "csrc", "peano_tables.h")).read()
    out = {}
    for name in ("MPG_PEANO_SUBPIX", "MPG_PEANO_NEXT"):
        body = txt.split("#define " + name)[1].split("}\n")[0]
        rows = re.findall(r"\{([0-9, ]+)\}", body)
        out[name] = np.array([[int(v) for v in r.split(",")] for r in rows], np.int64)
    n = int(re.search(r"MPG_PEANO_NSTATES (\d+)", txt).group(1))
    assert out["MPG_PEANO_SUBPIX"].shape == (n, 8) and out["MPG_PEANO_NEXT"].shape == (n, 8)
    return out["MPG_PEANO_SUBPIX"], out["MPG_PEANO_NEXT"]


def keys_from_tables(xyz, bits=21):
    sub, nxt = load_tables()
    xyz = np.asarray(xyz, np.int64)
    state = np.zeros(len(xyz), np.int64)
    key = np.zeros(len(xyz), np.uint64)
    for bit in range(bits - 1, -1, -1):
        pix = 4 * ((xyz[:, 0] >> bit) & 1) + 2 * ((xyz[:, 1] >> bit) & 1) + ((xyz[:, 2] >> bit) & 1)
        key = (key << np.uint64(3)) | sub[state, pix].astype(np.uint64)
        state = nxt[state, pix]
    return key


def test_tables_are_a_bijection_per_state():
    sub, nxt = load_tables()
    assert all(sorted(r) == list(range(8)) for r in sub.tolist())       # every orientation numbers its 8 octants 0..7
    assert nxt.min() >= 0 and nxt.max() < len(sub)


def test_golden_keys():
    g = np.load(os.path.join(ROOT, "tests", "golden", "peano_keys.npz"))
    assert np.array_equal(keys_from_tables(g["xyz"]), g["keys"])
    box = float(g["box"])
    fac = 1.0 / (box * 1.001) * float(1 << 21)
    ip = ((g["pos"] + box / 2000) * fac).astype(np.int32)
    assert np.array_equal(keys_from_tables(ip), g["pkeys"])
    # the curve is continuous: consecutive keys of a small cube are face neighbours
    side = 8
    c = np.array([[x, y, z] for x in range(side) for y in range(side) for z in range(side)])
    k = keys_from_tables(c, bits=3)
    assert sorted(k.tolist()) == list(range(side ** 3))
    path = c[np.argsort(k)]
    assert np.all(np.abs(np.diff(path, axis=0)).sum(1) == 1)


def test_against_reference_function_when_built():
    """peano_hilbert_key of the reference's utils/peano.c, as its in-place build (oracle/_ref/libref_leaf.so) computes it on random
    triplets of 1, 2, 5, 13 and 21 bits, recorded in tests/golden/reference_leaf.npz (make_reference_golden.py)."""
    g = np.load(os.path.join(ROOT, "tests", "golden", "reference_leaf.npz"))
    assert g["peano_bits"].tolist() == [1, 2, 5, 13, 21]
    for bits in g["peano_bits"].tolist():
        xyz, ref = g["peano_xyz_%d" % bits], g["peano_keys_%d" % bits]
        assert xyz.shape == (3000, 3) and xyz.min() >= 0 and xyz.max() < (1 << bits)
        assert np.array_equal(keys_from_tables(xyz, bits), ref), bits
