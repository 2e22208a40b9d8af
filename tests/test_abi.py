"""The C-ABI library loads on a CPU-only box and exports every symbol include/*.h declares (no compute calls)."""
import ctypes as C
import glob
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def declared_symbols():
    syms = []
    for h in glob.glob(os.path.join(ROOT, "include", "*.h")):
        txt = open(h).read()
        txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
        syms += re.findall(r"\b(mpg_[a-z0-9_]+)\s*\(", txt)
    return sorted(set(syms))


def test_library_exports_every_declared_symbol(pkg):
    L = pkg.engine.load_library()
    syms = declared_symbols()
    assert len(syms) >= 25
    missing = [s for s in syms if not hasattr(L, s)]
    assert not missing, missing


def test_version_and_error_string(pkg):
    L = pkg.engine.load_library()
    assert b"gfx950" in L.mpg_version()
    assert L.mpg_last_error() is not None


def test_reference_particle_layout(pkg):
    """struct particle_data is 160 bytes with the offsets of partmanager.h:9-71."""
    dt = pkg.PARTICLE_DTYPE
    assert dt.itemsize == 160
    off = {k: dt.fields[k][1] for k in dt.names}
    assert off["Pos"] == 0 and off["TopLeaf"] == 24 and off["Mass"] == 28 and off["PI"] == 32 and off["Type"] == 39
    assert off["Vel"] == 40 and off["FullTreeGravAccel"] == 64 and off["GravPM"] == 88 and off["Ti_drift"] == 112
    assert off["Hsml"] == 120 and off["DtHsml"] == 128 and off["ID"] == 136 and off["GrNr"] == 144 and off["Potential"] == 152
    v = pkg.engine.ParticleView()
    P = np.zeros(3, dtype=dt)
    pkg.engine.load_library().mpg_particle_view_reference_layout(C.byref(v), C.c_void_p(P.ctypes.data), C.c_int64(3))
    assert (v.stride, v.off_pos, v.off_mass, v.off_type, v.off_accel, v.off_gravpm, v.off_potential, v.off_hsml) == \
        (160, 0, 28, 39, 64, 88, 152, 120)


def test_no_cpu_fallback(pkg):
    """Without a GPU the engine must fail loudly, never fall back to a CPU path."""
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    with pytest.raises(pkg.EngineError, match="no HIP device"):
        pkg.Engine(0)


def test_product_never_imports_oracle():
    """oracle/ is test infrastructure: nothing under mp-gadget_amd/ may reference it."""
    for path in glob.glob(os.path.join(ROOT, "mp-gadget_amd", "**", "*"), recursive=True):
        if os.path.isfile(path) and path.endswith((".py", ".hip", ".h", ".cpp")):
            txt = open(path).read()
            for needle in ("import oracle", "from oracle", "liboracle", "oracle/"):
                assert needle not in txt, (path, needle)


def test_mpi_comm_shim_compiles():
    """shim/mpg_mpi_comm.c (mpg_comm on an MPI communicator) against the MPI-3 headers of this image, when they are there"""
    import shutil
    import subprocess
    inc = "/opt/conda/include"
    if not os.path.exists(os.path.join(inc, "mpi.h")) or not shutil.which("gcc"):
        pytest.skip("no mpi.h in this image")
    r = subprocess.run(["gcc", "-std=gnu11", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), "-I", inc,
                        os.path.join(ROOT, "shim", "mpg_mpi_comm.c"), os.path.join(ROOT, "shim", "mpg_rccl_mpi.c")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_shim_epoch_bookkeeping(tmp_path):
    """shim/mpg_shim_epoch.h - when mpg_shim_sync declares a new particle-table epoch - compiled and RUN on 160-byte records
    (tests/c/test_shim_epoch.c): one epoch per step, a new one for a new Ti_Current, moved / reordered / resized / relocated tables,
    the explicit hook, callers without a Ti_Current; and the documented limit of the 64-record sample."""
    import shutil
    import subprocess
    if not shutil.which("gcc"):
        pytest.skip("no gcc")
    exe = str(tmp_path / "test_shim_epoch")
    r = subprocess.run(["gcc", "-O2", "-std=gnu11", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "shim"),
                        os.path.join(ROOT, "tests", "c", "test_shim_epoch.c"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and r.stdout.strip().splitlines()[-1].startswith("PASS"), r.stdout[-2000:]


def test_shim_mpi_communicator_runs(tmp_path):
    """shim/mpg_mpi_comm.c under a REAL MPI on the CPU (tests/c/test_mpi_comm.c, mpiexec -n 1 / 3 / 4): all-reduce (double / int64, sum /
    max, a count beyond INT_MAX refused), the all-to-all of counts, and the byte all-to-all-v on ragged, empty and gapped blocks - also
    with a displacement beyond 2^31 bytes, where the shim switches every rank to 8-byte units, and a block those units cannot express.
    (The same file carries the library's collectives on the GPU box: tests/test_gpu_cabi.py::test_c_caller_real_mpi.)"""
    import shutil
    import subprocess
    root = os.environ.get("MPG_MPI_ROOT", "/opt/conda")
    inc, libmpi, mpiexec = os.path.join(root, "include"), os.path.join(root, "lib", "libmpi.so.12"), os.path.join(root, "bin", "mpiexec")
    if not (os.path.exists(os.path.join(inc, "mpi.h")) and os.path.exists(libmpi) and os.path.exists(mpiexec) and shutil.which("gcc")):
        pytest.skip("no MPI in this image")
    links = tmp_path / "mpilib"
    links.mkdir()
    for f in ("libmpi.so.12", "libgfortran.so.4", "libquadmath.so.0"):     # libmpi and its private dependencies only (tests/test_gpu_cabi.py)
        if os.path.exists(os.path.join(root, "lib", f)):
            os.symlink(os.path.join(root, "lib", f), str(links / f))
    exe = str(tmp_path / "test_mpi_comm")
    r = subprocess.run(["gcc", "-O2", "-std=gnu11", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "shim"),
                        "-I", inc, os.path.join(ROOT, "tests", "c", "test_mpi_comm.c"), os.path.join(ROOT, "shim", "mpg_mpi_comm.c"), "-o", exe,
                        libmpi, "-Wl,-rpath," + str(links)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    env = dict(os.environ, MPICH_INTERFACE_HOSTNAME="127.0.0.1")
    for nt in (1, 3, 4):
        r = subprocess.run([mpiexec, "-launcher", "fork", "-hosts", "127.0.0.1", "-n", str(nt), exe], capture_output=True, text=True, timeout=300, env=env)
        assert r.returncode == 0 and ("PASS mpg_mpi_comm on %d MPI processes" % nt) in r.stdout, (r.stdout[-2000:], r.stderr[-2000:])


def test_stale_library_is_refused(monkeypatch):
    """The library carries the hash of the sources it was built from (mpg_build_stamp, build.py); the host side refuses one that does
    not match the tree instead of running old kernels silently."""
    import importlib
    pkg = importlib.import_module("mp-gadget_amd")
    E = pkg.engine
    E.load_library()                                           # the in-tree library matches its sources
    assert E.load_library().mpg_build_stamp().decode() == pkg.build.source_stamp()
    monkeypatch.setattr(E, "_lib", None)
    monkeypatch.setattr(pkg.build, "source_stamp", lambda: "0" * 32)
    with pytest.raises(E.EngineError, match="stale"):
        E.load_library()


def test_rank_repeat_is_limited_to_device_faults_in_foreign_kernels():
    """tests/conftest.py::run_ranks repeats a multi-rank helper ONCE only for the failure caught at the end of round 6 (several processes on
    one GPU: an HSA queue abort inside PyTorch's own fill kernel, profiles/r06b_flake_stress/hsa_abort_in_torch_fill.log); a fault in a kernel
    of this library, a fault without a named kernel, an invariant or a wrong number are never repeated."""
    from conftest import _foreign_device_fault
    seen = ("GPU core dump created: gpucore.31797\n"
            "Kernel Name: _ZN2at6native29vectorized_elementwise_kernelILi4ENS0_11FillFunctorIdEESt5arrayIPcLm1EEEEviT0_T1_\n"
            ":0:rocdevice.cpp :3676: Callback: Queue 0x7f3e68c00000 aborting with error : HSA_STATUS_ERROR_ILLEGAL_INSTRUCTION: "
            "The agent attempted to execute an illegal shader instruction. code: 0x2a\n")
    assert _foreign_device_fault(seen)
    assert not _foreign_device_fault(seen.replace("_ZN2at6native29vectorized_elementwise_kernel", "_ZN3mpg9k_density"))
    assert not _foreign_device_fault("HSA_STATUS_ERROR_ILLEGAL_INSTRUCTION")           # (no kernel named: not repeated)
    assert not _foreign_device_fault("mpg_dist_domain_exchange: plan counts and decomposition counts differ")
    assert not _foreign_device_fault("AssertionError: max relative difference 3e-9")
    on_disk = os.path.join(ROOT, "profiles", "r06b_flake_stress", "hsa_abort_in_torch_fill.log")
    assert _foreign_device_fault(open(on_disk).read())


def test_run_ranks_repeat_paths(tmp_path, monkeypatch):
    """run_ranks on a stand-in helper: a first run that dies with the foreign-kernel device fault is repeated once (with a warning); the same
    death with one of this library's kernels named, or any other failure, fails at once."""
    import sys
    from conftest import run_ranks
    monkeypatch.delenv("MPG_TEST_RETRY", raising=False)
    helper = tmp_path / "helper.py"
    helper.write_text(
        "import os, sys\n"
        "marker, kernel = sys.argv[1], sys.argv[2]\n"
        "if os.path.exists(marker):\n"
        "    sys.exit(0)\n"
        "open(marker, 'w').close()\n"
        "print('Kernel Name: ' + kernel)\n"
        "sys.stderr.write('Queue aborting with error : HSA_STATUS_ERROR_ILLEGAL_INSTRUCTION: illegal shader instruction\\n')\n"
        "sys.exit(134)\n")
    foreign = "_ZN2at6native29vectorized_elementwise_kernelILi4ENS0_11FillFunctorIdEEEEviT0_T1_"
    with pytest.warns(UserWarning, match="device fault in a foreign kernel"):
        r = run_ranks([sys.executable, str(helper), str(tmp_path / "m1"), foreign], os.environ, tmp_path / "log1")
    assert r.returncode == 0 and os.path.exists(str(tmp_path / "log1") + ".failed.log")
    with pytest.raises(AssertionError):
        run_ranks([sys.executable, str(helper), str(tmp_path / "m2"), "_ZN3mpg9k_densityENS_8TreeViewE"], os.environ, tmp_path / "log2")
    with pytest.raises(AssertionError):
        run_ranks([sys.executable, "-c", "import sys; sys.exit(3)"], os.environ, tmp_path / "log3")
