"""The drop-in's gravpm_force carries the massive-neutrino linear response (gravpm.c:72-79, 303-326) and the hybrid-neutrino deposit
mask (gravpm.c:84-85): it installs the engine callback that runs the reference's own LRA code (delta_nu_from_power, neutrinos_lra.c),
MtotbyMcdm from get_omega_nu_nopart (omega_nu_single.c), and writes powerspectrum-nu through powerspectrum_nu_save."""
import ctypes as C
import os
import re
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LRA = ("delta_nu_from_power", "get_omega_nu_nopart", "powerspectrum_nu_save")


def _gravpm_force_body():
    src = open(os.path.join(ROOT, "shim", "gravity-hip.c")).read()
    i = src.index("void gravpm_force(PetaPM *pm")
    return src, src[i:src.index("\n}\n", i)]


def test_shim_installs_the_response():
    src, body = _gravpm_force_body()
    assert "(void)CP" not in body and "(void)TimeIC" not in body      # the two arguments the model needs are used
    for call in ("mpg_gravpm_set_nu_response(", "mpg_gravpm_set_hybrid_nu_tracer(", "hybrid_nu_tracer(CP, Time)",
                 "CP->MassiveNuLinRespOn", "powerspectrum_nu_save("):
        assert call in body, call
    cb = src[src.index("static int nu_response("):src.index("void gravpm_force(PetaPM *pm")]
    for call in ("powerspectrum_alloc(", "delta_nu_from_power(", "get_omega_nu_nopart("):
        assert call in cb, call


def test_library_exports_the_response_api(pkg):
    L = pkg.engine.load_library()
    for name in ("mpg_gravpm_set_nu_response", "mpg_gravpm_set_hybrid_nu_tracer", "mpg_dist_dev_set_types"):
        assert hasattr(L, name), name
    # the setters take a null engine as an error, not a crash
    assert L.mpg_gravpm_set_nu_response(None, None, None, C.c_double(1.0)) != 0
    assert L.mpg_gravpm_set_hybrid_nu_tracer(None, 1) != 0


def test_shim_object_references_the_lra():
    """shim/gravity-hip.c compiled with tools/link_audit.py's stand-ins against an MP-Gadget checkout (MPG_REFERENCE_TREE): its object
    references the three LRA functions, and the audit finds nothing defined twice and nothing unaccounted."""
    ref = os.environ.get("MPG_REFERENCE_TREE", "")
    if not ref or not os.path.isdir(os.path.join(ref, "libgadget")) or not shutil.which("gcc") or not shutil.which("nm"):
        pytest.skip("MPG_REFERENCE_TREE does not name an MP-Gadget checkout")
    import tempfile
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import link_audit
    with tempfile.TemporaryDirectory() as work:
        rep = link_audit.audit(ref, work)
        obj = os.path.join(work, "obj", "shim_gravity-hip.o")
        und = subprocess.run(["nm", "-u", obj], capture_output=True, text=True).stdout
        names = set(re.findall(r"\bU\s+(\S+)", und))
    for f in LRA:
        assert f in names, f
    assert not rep["duplicates"] and not rep["unaccounted"], (rep["duplicates"], rep["unaccounted"])
