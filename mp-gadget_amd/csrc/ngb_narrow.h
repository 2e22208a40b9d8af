// ngb_narrow.h -- ngb_narrow_down (treewalk.c:1371-1434), the step between two passes of a radius loop with several trial radii per pass
// (treewalk_do_hsml_loop): written once for the velocity dispersion (veldisp.hip: 5 radii, 40 neighbours) and the stellar density
// (metals.hip: 10 radii, GetNumNgb neighbours).
#pragma once
#include "mpg_common.h"
#include <cmath>

namespace mpg {

// a[k] of a register array without a dynamic index (k beyond the end reads the last entry)
template <int NR> __device__ __forceinline__ double ngb_pick(const double (&a)[NR], const int k)
{
    double v = a[NR - 1];
#pragma unroll
    for(int j = NR - 2; j >= 0; j--)
        v = k == j ? a[j] : v;
    return v;
}

// NR trial radii of which the first maxcmpt carry complete neighbour numbers.  desnumngb is an int, as the reference's parameter is: a
// caller with a fractional neighbour number (GetNumNgb) has it truncated here and nowhere else.  With maxcmpt == 1 the reference reads
// radius[1] and numNgb[1], which nothing defines (:1418-1419), and then overwrites what it computed from them (:1421-1422): the defined
// outcome is dngbdv = numNgb[0] / radius[0]^3.  The growth branch (:1400) uses the last two entries only when maxcmpt > 1.
template <int NR>
__device__ __forceinline__ double ngb_narrow_down(double &right, double &left, const double (&radius)[NR], const double (&num)[NR], const int maxcmpt,
                                                  const int desnumngb_int, const double box, int &closeidx)
{
    const double desnumngb = desnumngb_int;
    int close = 0;
    double ngbdist = fabs(num[0] - desnumngb);
#pragma unroll
    for(int j = 1; j < NR; j++) {
        const double newdist = fabs(num[j] - desnumngb);
        if(j < maxcmpt && newdist < ngbdist) {
            ngbdist = newdist;
            close = j;
        }
    }
    closeidx = close;
    bool stop = false;
#pragma unroll
    for(int j = 0; j < NR; j++) {
        if(j < maxcmpt && !stop) {
            if(num[j] < desnumngb)
                left = radius[j];
            if(num[j] > desnumngb) {
                right = radius[j];
                stop = true;
            }
        }
    }
    double hsml = ngb_pick(radius, close);
    if(right > 0.99 * box) {
        double dngbdv = 0;
        const double nlast = ngb_pick(num, maxcmpt - 1);
        if(maxcmpt > 1) {
            const double r1 = ngb_pick(radius, maxcmpt - 1), r0 = ngb_pick(radius, maxcmpt - 2);
            if(r1 > r0)
                dngbdv = (nlast - ngb_pick(num, maxcmpt - 2)) / (pow(r1, 3) - pow(r0, 3));
        }
        double newhsml = 4 * hsml; // "Increase hsml by a maximum factor to avoid madness"
        if(dngbdv > 0) {
            const double dngb = desnumngb - nlast;
            const double newvolume = pow(hsml, 3) + dngb / dngbdv;
            if(pow(newvolume, 1. / 3) < newhsml)
                newhsml = pow(newvolume, 1. / 3);
        }
        hsml = newhsml;
    }
    if(hsml > right)
        hsml = right;
    if(left == 0) { // extrapolate using volume, i.e. locally constant density
        double dngbdv = 0;
        if(maxcmpt > 1) {
            if(radius[1] > radius[0])
                dngbdv = (num[1] - num[0]) / (pow(radius[1], 3) - pow(radius[0], 3));
        }
        else if(radius[0] > 0)
            dngbdv = num[0] / pow(radius[0], 3);
        if(dngbdv > 0) {
            const double dngb = desnumngb - num[0];
            const double newvolume = pow(hsml, 3) + dngb / dngbdv;
            hsml = pow(newvolume, 1. / 3);
        }
    }
    if(hsml < left)
        hsml = left;
    return hsml;
}

} // namespace mpg
