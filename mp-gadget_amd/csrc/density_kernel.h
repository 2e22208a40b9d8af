// density_kernel.h -- the SPH kernel functions of libgadget/densitykernel.c for device code: shared by the SPH loops (sph.hip) and the
// stellar density / metal return loops (metals.hip)
#pragma once
#include "mpg_common.h"
#include <cmath>

namespace mpg {

constexpr int NUMDIMS = 3;
constexpr double NORM_COEFF = 4.188790204786; // densitykernel.h:6


struct DKernel { // DensityKernel, densitykernel.h:23-33
    double H, HH, Hinv, Wknorm, dWknorm, support;
};

__device__ __forceinline__ double p2(double x) { return x * x; }
__device__ __forceinline__ double p3(double x) { return x * x * x; }
__device__ __forceinline__ double p4(double x) { return (x * x) * (x * x); }
__device__ __forceinline__ double p5(double x) { return (x * x) * (x * x) * x; }

__device__ __forceinline__ double ksupport(int type) { return type == 0 ? 2. : (type == 1 ? 3. : 2.5); }
__device__ __forceinline__ double ksigma3(int type) { return type == 0 ? 1 / M_PI : (type == 1 ? 1 / (120 * M_PI) : 1 / (20 * M_PI)); }

__device__ __forceinline__ DKernel kernel_init(double H, int type) // densitykernel.c:136-153
{
    DKernel k;
    k.H = H;
    k.HH = H * H;
    k.Hinv = 1. / H;
    k.support = ksupport(type);
    const double hinv = k.Hinv * k.support;
    k.Wknorm = ksigma3(type) * p3(hinv);
    k.dWknorm = k.Wknorm * hinv;
    return k;
}

// The kernel polynomials of densitykernel.c:24-90 without branches on q: every term (c - q)^n of the reference's piecewise form is taken
// of max(c - q, 0), which is the term where the reference has it and an exact zero (added or subtracted last, in the reference's order:
// the sums' bits do not change) where it has not.  The lanes of a wave hold neighbours at all distances: with three branches the wave ran
// all three bodies one after the other (round 4: the SPH kernels are issue-bound, profiles/r04a_experiments).
__device__ __forceinline__ double pos_part(double x) { return fmax(x, 0.0); }
template <int TYPE> __device__ __forceinline__ double wk_q(double q) // densitykernel.c:24-90
{
    if(TYPE == 0)
        return 0.25 * p3(pos_part(2 - q)) - p3(pos_part(1 - q));
    else if(TYPE == 1)
        return p5(pos_part(3 - q)) - 6 * p5(pos_part(2 - q)) + 15 * p5(pos_part(1 - q));
    else
        return p4(pos_part(2.5 - q)) - 5 * p4(pos_part(1.5 - q)) + 10 * p4(pos_part(0.5 - q));
}
template <int TYPE> __device__ __forceinline__ double dwk_q(double q)
{
    if(TYPE == 0)
        return -0.25 * 3 * p2(pos_part(2 - q)) + 3 * p2(pos_part(1 - q));
    else if(TYPE == 1)
        return -5 * p4(pos_part(3 - q)) + 30 * p4(pos_part(2 - q)) - 75 * p4(pos_part(1 - q));
    else
        return -4 * p3(pos_part(2.5 - q)) + 20 * p3(pos_part(1.5 - q)) - 40 * p3(pos_part(0.5 - q));
}
__device__ __forceinline__ double kernel_wk(const DKernel &k, int type, double u)
{
    const double q = u * k.support;
    return k.Wknorm * (type == 0 ? wk_q<0>(q) : (type == 1 ? wk_q<1>(q) : wk_q<2>(q)));
}
__device__ __forceinline__ double kernel_dwk(const DKernel &k, int type, double u)
{
    const double q = u * k.support;
    return k.dWknorm * (type == 0 ? dwk_q<0>(q) : (type == 1 ? dwk_q<1>(q) : dwk_q<2>(q)));
}

// 1 / x and 1 / sqrt(x) to within an ulp: v_rcp_f64 / v_rsq_f64 and Newton steps instead of the ~30-instruction IEEE division and
// square-root expansions (the reference itself is built with -ffast-math).  x > 0 and finite.  Round 4 took the quotients and the square
// root of the pair evaluations this way (k_hydro 10.1 -> 9.6 ms).
__device__ __forceinline__ double rcp_fast(const double x)
{
    double y = __builtin_amdgcn_rcp(x);
    y = fma(fma(-x, y, 1.0), y, y);
    return fma(fma(-x, y, 1.0), y, y);
}
__device__ __forceinline__ double rsqrt_fast(const double x)
{
    const double y = __builtin_amdgcn_rsq(x);
    const double e = fma(-(x * y), y, 1.0);
    return fma(y * e, fma(e, 0.375, 0.5), y);
}

} // namespace mpg
