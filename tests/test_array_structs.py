"""The Python mirrors of the structs of array pointers follow include/mpgadget_hip.h: member names in order, and element types.

A transposed name in a *_ARRAY_FIELDS tuple hands the library the wrong pointer; this reads the header's text, so it needs no GPU."""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# struct of the header -> (tuple of member names, dict of the element types that are not float64), both in engine.py.
# A new module's struct of host arrays is one more row here.
STRUCTS = {
    "mpg_sph_arrays": ("SPH_ARRAY_FIELDS", "SPH_ARRAY_DTYPES"),
    "mpg_veldisp_arrays": ("VELDISP_ARRAY_FIELDS", "VELDISP_ARRAY_DTYPES"),
    "mpg_cooling_arrays": ("COOLING_ARRAY_FIELDS", "COOLING_ARRAY_DTYPES"),
    "mpg_metal_arrays": ("METAL_ARRAY_FIELDS", "METAL_ARRAY_DTYPES"),
    "mpg_blackhole_arrays": ("BLACKHOLE_ARRAY_FIELDS", "BLACKHOLE_ARRAY_DTYPES"),
    "mpg_bh_dynfric_arrays": ("BH_DYNFRIC_ARRAY_FIELDS", "BH_DYNFRIC_ARRAY_DTYPES"),
    "mpg_wind_arrays": ("WIND_ARRAY_FIELDS", "WIND_ARRAY_DTYPES"),
}
C_TO_NUMPY = {"double": "float64", "float": "float32", "uint8_t": "uint8", "uint64_t": "uint64", "int32_t": "int32"}
DECLARATION = re.compile(r"(?:const\s+)?(\w+)\s*\*\s*(\w+(?:\s*,\s*\*\s*\w+)*)$")   # [const] T *a, *b, *c


def struct_members(name):
    """[(member, numpy type name)] of `typedef struct <name> { ... }` in declaration order"""
    txt = open(os.path.join(ROOT, "include", "mpgadget_hip.h")).read()
    txt = re.sub(r"/\*.*?\*/", " ", txt, flags=re.S)
    txt = re.sub(r"//[^\n]*", " ", txt)
    body = re.search(r"typedef\s+struct\s+%s\s*\{(.*?)\}\s*%s\s*;" % (name, name), txt, flags=re.S)
    assert body, "no struct %s in the header" % name
    members = []
    for decl in body.group(1).split(";"):
        decl = " ".join(decl.split())
        if not decl:
            continue
        m = DECLARATION.match(decl)
        assert m, "%s: not a declaration of array pointers: %r" % (name, decl)
        assert m.group(1) in C_TO_NUMPY, "%s: element type %s" % (name, m.group(1))
        members += [(v.strip(" *"), C_TO_NUMPY[m.group(1)]) for v in m.group(2).split(",")]
    return members


@pytest.mark.parametrize("struct", sorted(STRUCTS))
def test_python_mirror_follows_the_header(pkg, struct):
    fields, dtypes = (getattr(pkg.engine, k) for k in STRUCTS[struct])
    members = struct_members(struct)
    assert tuple(k for k, _ in members) == tuple(fields)
    assert {k: t for k, t in members if t != "float64"} == dict(dtypes)


def test_every_struct_of_arrays_is_listed():
    txt = open(os.path.join(ROOT, "include", "mpgadget_hip.h")).read()
    assert sorted(re.findall(r"typedef\s+struct\s+(mpg_\w+_arrays)\s*\{", txt)) == sorted(STRUCTS)
