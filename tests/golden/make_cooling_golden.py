"""Generates tests/golden/cooling_kat.npz: the numbers the reference's own cooling tests check against, and the UV background table they
load.  Only numbers are recorded.  Run with the path of a reference checkout:  python tests/golden/make_cooling_golden.py <checkout>

cooling_kat.npz
  treecool                   the seven columns of examples/TREECOOL_ep_2018p (comment lines dropped): log10(1+z), Gamma_HI, Gamma_HeI,
                             Gamma_HeII, Qdot_HI, Qdot_HeI, Qdot_HeII, shape (7, N)
  unew_table, tcool_table    the two 20 x 20 tables of libgadget/tests/test_cooling.c (DoCooling and GetCoolingTime on the grid of
                             test_cooling.c:210-239; density index major)
  docooling_single           (u, rho, dt, unew) and coolingtime_single (u, rho, tcool) of test_cooling.c:215-218
  uvbg_z0, uvbg_z3           epsH0, epsHe0, epsHep, gJH0, gJHe0, gJHep, self_shield_dens of test_cooling_rates.c:98-115
  tcool_kwh                  4.68906e-06 (:230);  lambdanet (-0.0410059, -1.64834) (:241, :252)
  temp_window                (9500, 9510) (:145-146);  nh0_slope 0.3113 (:156)
  equilib_ne                 rows (density, helium, tolerance) of :138-141
"""
import os
import re
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))


def c_array(text, name):
    m = re.search(r"%s\s*\[[^\]]*\]\s*=\s*\{(.*?)\};" % name, text, re.S)
    return np.array([float(x) for x in m.group(1).replace("\n", " ").split(",") if x.strip()])


def main(ref):
    rows = []
    for line in open(os.path.join(ref, "examples", "TREECOOL_ep_2018p")):
        f = line.split()
        if not f or f[0].startswith("#"):
            continue
        rows.append([float(x) for x in f[:7]])
    treecool = np.array(rows).T.copy()
    txt = open(os.path.join(ref, "libgadget", "tests", "test_cooling.c")).read()
    unew, tcool = c_array(txt, "unew_table"), c_array(txt, "tcool_table")
    assert unew.shape == (400,) and tcool.shape == (400,) and treecool.shape[0] == 7
    np.savez_compressed(
        os.path.join(HERE, "cooling_kat.npz"), treecool=treecool, unew_table=unew, tcool_table=tcool,
        docooling_single=np.array([9828.44, 7.07946e-06, 0.2, 531.724]), coolingtime_single=np.array([949.755, 7.07946e-06, 0.0172379]),
        uvbg_z0=np.array([3.65296e-25, 3.98942e-25, 3.33253e-26, 6.06e-14, 3.03e-14, 1.1e-15, 0.0010114161149989826]),
        uvbg_z3=np.array([5.96570906168362e-24, 4.466976578202419e-24, 2.758535690259892e-26, 1.0549960730284017e-12, 4.759025257653999e-13,
                          2.270599708640625e-16, 0.007691709693529007]),
        tcool_kwh=np.array(4.68906e-06), lambdanet=np.array([-0.0410059, -1.64834]), temp_window=np.array([9500.0, 9510.0]),
        nh0_slope=np.array(0.3113), equilib_ne=np.array([[1e-6, 0.24, 3e-5], [1e-6, 0.12, 3e-5], [1e-5, 0.24, 3e-4], [1e-4, 0.24, 2e-3]]))
    print("wrote cooling_kat.npz: %d TREECOOL rows, %d + %d table entries" % (treecool.shape[1], len(unew), len(tcool)))


if __name__ == "__main__":
    main(sys.argv[1])
