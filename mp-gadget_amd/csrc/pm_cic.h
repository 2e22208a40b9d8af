// pm_cic.h -- the real-space rules of the particle mesh, each written once (device-inline): the base cell and CIC residual of a
// position, its fold into the mesh, the slab that owns it, the corner order with its weight and mesh index, and the 4-point
// difference stencil of the one-pass read-out.  pm.hip deposits and reads out by them, dist_gravity.hip routes particles by them: a rank
// receives a particle because of the same base cell that the slab kernels then find.
// Every order of operations here is deliberate (parity with the reference is bit-sensitive): see DESIGN.md 3.3.
#pragma once
#include <hip/hip_runtime.h>
#include <cstddef>

namespace mpg {

__device__ __forceinline__ int wrap(int i, int n)
{
    // periodic wrap of petapm.c:903-918 by one box: for a folded base cell plus the CIC corner or a stencil offset (-2 .. n + 2)
    i = (i >= n) ? i - n : i;
    i = (i < 0) ? i + n : i;
    return i;
}

__device__ __forceinline__ int fold(int i, int n)
{
    // the same wrap for a particle's BASE cell, by any number of boxes as the reference's while loops do (petapm.c:905-906, 917-918):
    // a position outside [0, BoxSize] must not become an index outside the mesh.  Once per axis and particle, and the division only
    // for a cell outside [0, n): particles inside the box pay a compare.  (The slab kernels use it axis by axis.)
    if((unsigned)i >= (unsigned)n) {
        i %= n;
        i = (i < 0) ? i + n : i;
    }
    return i;
}

__device__ __forceinline__ void fold3(int ic[3], int n)
{
    // fold() of the three axes behind ONE branch (the single-mesh kernels of every PM step: three branches cost the read-out 4 %)
    if(((unsigned)ic[0] >= (unsigned)n) | ((unsigned)ic[1] >= (unsigned)n) | ((unsigned)ic[2] >= (unsigned)n)) {
#pragma unroll
        for(int k = 0; k < 3; k++)
            ic[k] = fold(ic[k], n);
    }
}

// base cell (not folded yet) and CIC residual of one coordinate, petapm.c:965-972: the cell is the fp64 decision floor(x / cellsize)
__device__ __forceinline__ int cic_axis(double x, double cellsize, double &res)
{
    const double tmp = x / cellsize;
    const double fl = floor(tmp);
    res = tmp - fl;
    return (int)fl;
}

// ... folded, one axis at a time: the slab kernels, which test x first and leave before they look at y and z
__device__ __forceinline__ int cic_cell(double x, double cellsize, int nmesh, double &res) { return fold(cic_axis(x, cellsize, res), nmesh); }

// ... of a position, folded behind fold3's single branch: the whole-mesh kernels
__device__ __forceinline__ void cic_cell3(const double *__restrict__ p, double cellsize, int nmesh, int ic[3], double res[3])
{
#pragma unroll
    for(int k = 0; k < 3; k++)
        ic[k] = cic_axis(p[k], cellsize, res[k]);
    fold3(ic, nmesh);
}

// is x-plane ix one of the slab's [x0, x0 + P)?
__device__ __forceinline__ bool in_slab(int ix, int x0, int P) { return ix - x0 >= 0 && ix - x0 < P; }

// slab owner(s) of a particle's CIC cloud, P planes per rank: o0 owns the base cell's plane (and reads the particle out), o1 the
// plane above it (periodic)
__device__ __forceinline__ void pm_owners(double x, double cellsize, int nmesh, int P, int &o0, int &o1)
{
    double res;
    const int ix = cic_cell(x, cellsize, nmesh, res);
    o0 = ix / P;
    o1 = wrap(ix + 1, nmesh) / P;
}

// CIC weight of corner c (bit 0 -> x, bit 1 -> y, bit 2 -> z; the order of every corner loop): seed times the x, y and z factors in
// that order.  seed 1 gives ((wx wy) wz), which the plain deposits and the read-outs then multiply by the mass or the mesh value
// (1 wx is exact); seed m gives (((m wx) wy) wz), the order of the cell-sorted deposit, which sums weights that carry the mass.
__device__ __forceinline__ double cic_weight(int c, const double res[3], double seed)
{
    double w = seed;
#pragma unroll
    for(int k = 0; k < 3; k++)
        w *= ((c >> k) & 1) ? res[k] : (1 - res[k]);
    return w;
}

// mesh index of corner c of the folded base cell ic: x slowest, every axis wrapped
__device__ __forceinline__ size_t cic_index(int c, const int ic[3], int nmesh)
{
    size_t lin = 0;
#pragma unroll
    for(int k = 0; k < 3; k++)
        lin = lin * (size_t)nmesh + (size_t)wrap(ic[k] + ((c >> k) & 1), nmesh);
    return lin;
}

// ... in a slab that holds the x-planes [x0, x0 + P); false: the corner lies on another rank's plane
__device__ __forceinline__ bool cic_index_slab(int c, const int ic[3], int nmesh, int x0, int P, size_t &lin)
{
    const int ix = wrap(ic[0] + (c & 1), nmesh);
    if(!in_slab(ix, x0, P))
        return false;
    lin = (size_t)(ix - x0);
#pragma unroll
    for(int k = 1; k < 3; k++)
        lin = lin * (size_t)nmesh + (size_t)wrap(ic[k] + ((c >> k) & 1), nmesh);
    return true;
}

// the six rows ic - 2 .. ic + 3 of an axis that the stencil read-out of a base cell ic touches, wrapped, times the axis stride
__device__ __forceinline__ void stencil_rows(int ic, int nmesh, size_t stride, size_t wi[6])
{
#pragma unroll
    for(int j = 0; j < 6; j++)
        wi[j] = (size_t)wrap(ic - 2 + j, nmesh) * stride;
}

// ... along x in a slab stored with two ghost planes below its plane 0 and three above its last: px is relative to the slab and
// nothing wraps, the neighbours' planes are there ((px - 2 + j) + 2 ghost planes)
__device__ __forceinline__ void stencil_rows_ghost(int px, size_t stride, size_t wi[6])
{
#pragma unroll
    for(int j = 0; j < 6; j++)
        wi[j] = (size_t)(px + j) * stride;
}

// Potential and force at a particle from the potential mesh alone: per CIC corner the potential and, along each axis, its 4-point
// central difference
//     F = -[ 2/3 (phi[+1] - phi[-1]) - 1/12 (phi[+2] - phi[-2]) ] scale,    scale = N / Box
// a[0] = potential, a[1 .. 3] = force.  wi[k] = the six rows of axis k (above), res = the CIC residuals.  The expressions stay as
// they are written: corner order and weight product of cic_weight, c1 (..) - c2 (..) not regrouped.
__device__ __forceinline__ void cic_stencil_gather(const size_t wi[3][6], const double res[3], double scale, const double *__restrict__ phi,
                                                   double a[4])
{
    const double c1 = 2.0 / 3.0, c2 = 1.0 / 12.0;
    a[0] = a[1] = a[2] = a[3] = 0;
#pragma unroll
    for(int cc = 0; cc < 8; cc++) {
        const int ox = cc & 1, oy = (cc >> 1) & 1, oz = (cc >> 2) & 1;
        const double w = cic_weight(cc, res, 1.0);
        const size_t bx = wi[0][2 + ox], by = wi[1][2 + oy], bz = wi[2][2 + oz];
        a[0] += w * phi[bx + by + bz];
        a[1] += w * (-(c1 * (phi[wi[0][3 + ox] + by + bz] - phi[wi[0][1 + ox] + by + bz]) - c2 * (phi[wi[0][4 + ox] + by + bz] - phi[wi[0][0 + ox] + by + bz])) * scale);
        a[2] += w * (-(c1 * (phi[bx + wi[1][3 + oy] + bz] - phi[bx + wi[1][1 + oy] + bz]) - c2 * (phi[bx + wi[1][4 + oy] + bz] - phi[bx + wi[1][0 + oy] + bz])) * scale);
        a[3] += w * (-(c1 * (phi[bx + by + wi[2][3 + oz]] - phi[bx + by + wi[2][1 + oz]]) - c2 * (phi[bx + by + wi[2][4 + oz]] - phi[bx + by + wi[2][0 + oz]])) * scale);
    }
}

} // namespace mpg
