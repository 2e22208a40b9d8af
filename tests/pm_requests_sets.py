"""Input sets of the PM request tests (test_gpu_pm_requests.py on the GPU, test_pm_requests_inputs.py for their fp64 conditioning), on
top of pm_restated.py.  Not a test module.

Two kernels are concerned (csrc/pm.hip): the plain deposit with two lanes per particle, and the fused x-pass solve (k_xpass_solve)
that Nmesh 64 .. 1024 take by default.  The sets:

  deposit pairs   pm_restated.sweep("one" | "runs", N, Nmesh), N = 1, 31, 32, 33 (half a pair-wave: 32 particles are 64 lanes), 63, 64, 65,
                  127, 128, 129 (a 256-thread block holds 128 particles) and 3001, at Nmesh 8 - an eighth of the particles sit in the
                  last z-plane, where the two lanes of a pair write cells a row apart - and 40; the pile with dead records and the pile
                  moved whole boxes out (pm_restated's "pile-live", "pile-shift")
  x-pass          a clustered and a Zel'dovich-like set of 27^3 = 19683 particles at Nmesh 64 (33 kz columns: four tiles of 8 and a
                  ragged one when counted from kz = 0; the kernel cuts a row at the 128-byte lines of memory, so rows with ky mod 8 != 0
                  start with a ragged tile too) and Nmesh 128"""
import functools

import numpy as np

import pm_restated as R

PAIR_N = (1, 31, 32, 33, 63, 64, 65, 127, 128, 129, 3001)
PAIR_NMESH = (8, 40)
PAIR_SETS = tuple("%s-%d-%d" % (k, n, m) for k in ("one", "runs") for n in PAIR_N for m in PAIR_NMESH)
XPASS_SETS = tuple("x%s-%d" % (k, m) for k in ("clust", "zel") for m in (64, 128))
FALLBACK_SETS = ("xclust-64", "clust-72")
ALL_SETS = tuple(dict.fromkeys(PAIR_SETS + ("pile-live", "pile-shift") + XPASS_SETS + FALLBACK_SETS))


@functools.lru_cache(maxsize=None)
def input_set(name):
    """(pos, mass, box, nmesh) by name: the x-pass sets here, every other name is pm_restated's"""
    part = name.split("-")
    if part[0] == "xclust":
        pos, _, box = R._ics().s_clust(27, box=100.0, seed=4)
        return pos, R._masses(np.random.RandomState(5), len(pos)), box, int(part[1])
    if part[0] == "xzel":
        return R._ics().s_zel(27) + (int(part[1]),)
    return R.input_set(name)


@functools.lru_cache(maxsize=None)
def reference(name):
    """long-double (GravPM, Potential) of a named set, computed once per process"""
    if name[0] != "x":
        return R.reference(name)
    pos, mass, box, nmesh = input_set(name)
    return R.gravpm_force_ld(pos, mass, box, nmesh, 1.5, R.G)


def force_scale(name):
    """pm_restated.force_scale for the sets of this module"""
    pos, _, box, nmesh = input_set(name)
    g, p = reference(name)
    ps = np.abs(p).mean()
    return (ps * nmesh / box if len(pos) == 1 else np.abs(g).mean()), ps


@functools.lru_cache(maxsize=None)
def spectrum(name):
    """pm_restated.power_spectrum_ld of a named set with BoxSize_in_MPC = box / 1000"""
    pos, mass, box, nmesh = input_set(name)
    return R.power_spectrum_ld(pos, mass, box, nmesh, box / 1000.0)
