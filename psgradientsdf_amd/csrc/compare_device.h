// compare_device.h -- the device functions the nearest search (compare.hip) and the registration's row kernels (align.hip) share: the targets'
// corners and the closed pair function of include/psgsdf_compare.h, operation for operation.  Include it after `#pragma clang fp contract(off)`.
#pragma once
#include "device_common.h"
#include "compare.h"

namespace psg {
namespace {

__device__ __forceinline__ double cmp_dot(const double* u, const double* v) { return (u[0] * v[0] + u[1] * v[1]) + u[2] * v[2]; }

// the corners of target t, widened (a point target: three times the point)
__device__ __forceinline__ void cmp_target(const CompareArgs& a, int t, double* A, double* B, double* C) {
    int i0 = t, i1 = t, i2 = t;
    if (a.t_faces) { i0 = a.t_faces[3 * (long long)t]; i1 = a.t_faces[3 * (long long)t + 1]; i2 = a.t_faces[3 * (long long)t + 2]; }
#pragma unroll
    for (int k = 0; k < 3; ++k) { A[k] = (double)a.t_xyz[3 * (long long)i0 + k]; B[k] = (double)a.t_xyz[3 * (long long)i1 + k]; C[k] = (double)a.t_xyz[3 * (long long)i2 + k]; }
}

// Ericson 5.1.5 with the header's rules: the closest point q of triangle abc to p, and D2 = |p - q|^2
__device__ __forceinline__ double cmp_pair(const double* p, const double* a, const double* b, const double* c, double* q) {
#pragma clang fp contract(off)
    double ab[3], ac[3], ap[3], bp[3], cp[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) { ab[k] = b[k] - a[k]; ac[k] = c[k] - a[k]; ap[k] = p[k] - a[k]; bp[k] = p[k] - b[k]; cp[k] = p[k] - c[k]; }
    const double d1 = cmp_dot(ab, ap), d2 = cmp_dot(ac, ap), d3 = cmp_dot(ab, bp), d4 = cmp_dot(ac, bp), d5 = cmp_dot(ab, cp), d6 = cmp_dot(ac, cp);
    const double vc = d1 * d4 - d3 * d2, vb = d5 * d2 - d1 * d6, va = d3 * d6 - d5 * d4, e1 = d4 - d3, e2 = d5 - d6;
    if (d1 <= 0.0 && d2 <= 0.0) { q[0] = a[0]; q[1] = a[1]; q[2] = a[2]; }
    else if (d3 >= 0.0 && d4 <= d3) { q[0] = b[0]; q[1] = b[1]; q[2] = b[2]; }
    else if (vc <= 0.0 && d1 >= 0.0 && d3 <= 0.0) {
        const double v = d1 / (d1 - d3);
#pragma unroll
        for (int k = 0; k < 3; ++k) q[k] = a[k] + ab[k] * v;
    } else if (d6 >= 0.0 && d5 <= d6) { q[0] = c[0]; q[1] = c[1]; q[2] = c[2]; }
    else if (vb <= 0.0 && d2 >= 0.0 && d6 <= 0.0) {
        const double w = d2 / (d2 - d6);
#pragma unroll
        for (int k = 0; k < 3; ++k) q[k] = a[k] + ac[k] * w;
    } else if (va <= 0.0 && e1 >= 0.0 && e2 >= 0.0) {
        const double w = e1 / (e1 + e2);
#pragma unroll
        for (int k = 0; k < 3; ++k) q[k] = b[k] + (c[k] - b[k]) * w;
    } else {
        const double denom = 1.0 / ((va + vb) + vc), v = vb * denom, w = vc * denom;
#pragma unroll
        for (int k = 0; k < 3; ++k) q[k] = (a[k] + ab[k] * v) + ac[k] * w;
    }
    const double pq[3] = {p[0] - q[0], p[1] - q[1], p[2] - q[2]};
    return cmp_dot(pq, pq);
}

}  // namespace
}  // namespace psg
