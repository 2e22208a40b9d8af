/* The filter radii of the excursion-set reionisation model as a C loop in fp64 (the loop of petapm_reion_c2r: start at min(Rmax, Box),
 * divide by Rdelta, stop - with one last, unfiltered step at the cell size - as soon as the next radius would fall below Rmin or below the
 * cell size, or after MAX_R_ITERATIONS).  tests/test_uvbg_restated.py compiles it and holds tests/uvbg_restated.py::radii to its output,
 * bit for bit (the radii are printed as hexadecimal floats).
 * usage: uvbg_radii Rmax Rmin Rdelta Box dim */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>

#define MAX_R_ITERATIONS 10000

int main(int argc, char **argv)
{
    if(argc != 6)
        return 2;
    const double R_max = strtod(argv[1], NULL), R_min = strtod(argv[2], NULL), R_delta = strtod(argv[3], NULL), BoxSize = strtod(argv[4], NULL);
    const int Nmesh = atoi(argv[5]);
    const double CellSize = BoxSize / Nmesh;
    double R = fmin(R_max, BoxSize);
    int last_step = 0, f_count = 0;
    while(!last_step) {
        f_count++;
        if(R / R_delta < R_min || R / R_delta < CellSize || f_count > MAX_R_ITERATIONS) {
            last_step = 1;
            R = CellSize;
        }
        printf("%a\n", R);
        R = R / R_delta;
    }
    return 0;
}
