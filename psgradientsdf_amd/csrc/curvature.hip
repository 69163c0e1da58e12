// curvature.hip -- curvature of the level sets of the distance field (include/psgsdf_curvature.h; DESIGN.md "Surface curvature"):
//   curv_voxel     the definition, for one voxel: range and border checks before any load, the 19 weights, the 19 distances widened to double, the
//                  gradient and the Hessian by central differences, the shape operator in the tangent frame of psgsdf_occlusion.h, its eigenvalues and
//                  the first eigenvector.  Double throughout, no contraction; seven floats and a flag come out.
//   k_curv_voxels  one thread per entry of the caller's list.  With the list ascending (the band's order) the x neighbours of adjacent lanes coalesce.
//   k_wmesh_curv   one thread per key slot of the welded mesh (engine.h WMeshGrid, next to mesh.hip k_wmesh_verts and fit.hip k_wmesh_fit): the float
//                  results of the vertex's end voxels, interpolated in double with the vertex's own float parameter.
//   k_bake_curv    one thread per atlas texel: the voxel of the bake's `voxel` plane, evaluated; 0 / 0 where there is none.
// No atomics, no LDS, plain stores: the same bytes on every call.
#pragma clang fp contract(off)
#include "curvature.h"
#include <algorithm>

namespace psg {
namespace {

struct Curv { float mean, gauss, k1, k2, d0, d1, d2; unsigned char valid; };

__device__ __forceinline__ Curv curv_voxel(const float* __restrict__ dist, const float* __restrict__ weight, int nx, int ny, int nz, double h, long long lin) {
    Curv r{};
    const long long sy = nx, sz = (long long)nx * ny;
    if (lin < 0 || lin >= sz * nz) return r;
    const int i = (int)(lin % nx), j = (int)((lin / nx) % ny), k = (int)(lin / sz);
    if (i < 1 || i > nx - 2 || j < 1 || j > ny - 2 || k < 1 || k > nz - 2) return r;
    const float* w = weight + lin;
    const bool seen = (w[0] > 0.f) & (w[1] > 0.f) & (w[-1] > 0.f) & (w[sy] > 0.f) & (w[-sy] > 0.f) & (w[sz] > 0.f) & (w[-sz] > 0.f)
        & (w[1 + sy] > 0.f) & (w[-1 - sy] > 0.f) & (w[1 - sy] > 0.f) & (w[-1 + sy] > 0.f)
        & (w[1 + sz] > 0.f) & (w[-1 - sz] > 0.f) & (w[1 - sz] > 0.f) & (w[-1 + sz] > 0.f)
        & (w[sy + sz] > 0.f) & (w[-sy - sz] > 0.f) & (w[sy - sz] > 0.f) & (w[-sy + sz] > 0.f);
    if (!seen) return r;
    const float* d = dist + lin;
    const double d0 = (double)d[0];
    const double xp = (double)d[1], xm = (double)d[-1], yp = (double)d[sy], ym = (double)d[-sy], zp = (double)d[sz], zm = (double)d[-sz];
    const double h2 = h * h, two_h = 2.0 * h, four_h2 = 4.0 * h * h;
    const double gx = (xp - xm) / two_h, gy = (yp - ym) / two_h, gz = (zp - zm) / two_h;
    const double G2 = (gx * gx + gy * gy) + gz * gz;
    if (!(G2 > 0.0)) return r;
    const double hxx = ((xp + xm) - 2.0 * d0) / h2, hyy = ((yp + ym) - 2.0 * d0) / h2, hzz = ((zp + zm) - 2.0 * d0) / h2;
    const double hxy = (((double)d[1 + sy] + (double)d[-1 - sy]) - ((double)d[1 - sy] + (double)d[-1 + sy])) / four_h2;
    const double hxz = (((double)d[1 + sz] + (double)d[-1 - sz]) - ((double)d[1 - sz] + (double)d[-1 + sz])) / four_h2;
    const double hyz = (((double)d[sy + sz] + (double)d[-sy - sz]) - ((double)d[sy - sz] + (double)d[-sy + sz])) / four_h2;
    const double G = sqrt(G2);
    const double m0 = gx / G, m1 = gy / G, m2 = gz / G;
    // the frame of m (psgsdf_occlusion.h); sg + m2 is never zero
    const double sg = copysign(1.0, m2), fa = -1.0 / (sg + m2), fb = m0 * m1 * fa;
    const double t10 = 1.0 + sg * m0 * m0 * fa, t11 = sg * fb, t12 = -sg * m0;
    const double t20 = fb, t21 = sg + m1 * m1 * fa, t22 = -m1;
    // the shape operator in (t1, t2)
    const double u10 = (hxx * t10 + hxy * t11) + hxz * t12, u11 = (hxy * t10 + hyy * t11) + hyz * t12, u12 = (hxz * t10 + hyz * t11) + hzz * t12;
    const double u20 = (hxx * t20 + hxy * t21) + hxz * t22, u21 = (hxy * t20 + hyy * t21) + hyz * t22, u22 = (hxz * t20 + hyz * t21) + hzz * t22;
    const double a = ((t10 * u10 + t11 * u11) + t12 * u12) / G;
    const double b = ((t10 * u20 + t11 * u21) + t12 * u22) / G;
    const double c = ((t20 * u20 + t21 * u21) + t22 * u22) / G;
    const double mean = (a + c) / 2.0, gauss = a * c - b * b, hd = (a - c) / 2.0;
    const double s = sqrt(hd * hd + b * b);
    double e0 = 1.0, e1 = 0.0;
    if (s == 0.0) { }
    else if (hd >= 0.0) { e0 = hd + s; e1 = b; }
    else { e0 = b; e1 = s - hd; }
    const double en = sqrt(e0 * e0 + e1 * e1);
    e0 = e0 / en; e1 = e1 / en;
    r.mean = (float)mean; r.gauss = (float)gauss; r.k1 = (float)(mean + s); r.k2 = (float)(mean - s);
    r.d0 = (float)(e0 * t10 + e1 * t20); r.d1 = (float)(e0 * t11 + e1 * t21); r.d2 = (float)(e0 * t12 + e1 * t22);
    r.valid = 1;
    return r;
}

__global__ void __launch_bounds__(kBlock) k_curv_voxels(CurvGrid c, const long long* __restrict__ lin, long long n, unsigned char* __restrict__ valid, float* __restrict__ mean,
                                                         float* __restrict__ gauss, float* __restrict__ k1, float* __restrict__ k2, float* __restrict__ dir1) {
    const long long q = blockIdx.x * (long long)blockDim.x + threadIdx.x;
    if (q >= n) return;
    const Curv r = curv_voxel(c.dist, c.weight, c.nx, c.ny, c.nz, (double)c.vs, lin[q]);
    valid[q] = r.valid; mean[q] = r.mean; gauss[q] = r.gauss; k1[q] = r.k1; k2[q] = r.k2;
    dir1[3 * q] = r.d0; dir1[3 * q + 1] = r.d1; dir1[3 * q + 2] = r.d2;
}

// Key slot s = 4 * ((kz * d1 + j) * d0 + i) + type of the crop voxel (i, j, kz + zc0), as in fit.hip k_wmesh_fit; num: the exclusive scan of the
// used-key flags.
__global__ void __launch_bounds__(kBlock) k_wmesh_curv(CurvGrid c, WMeshGrid g, const int* __restrict__ num, int n_verts, unsigned char* __restrict__ v_valid,
                                                        float* __restrict__ v_mean, float* __restrict__ v_gauss, float* __restrict__ v_k1, float* __restrict__ v_k2) {
    const long long s = blockIdx.x * (long long)blockDim.x + threadIdx.x;
    if (s >= g.nown) return;
    const int v = num[s];
    if ((s + 1 < g.nown ? num[s + 1] : n_verts) == v) return;      // an unused key
    const int type = (int)(s & 3), q = (int)(s >> 2);
    const int i = q % g.d[0], j = (q / g.d[0]) % g.d[1], k = q / (g.d[0] * g.d[1]) + g.zc0;
    const long long dl = (long long)(k + g.lo[2] - g.zlo) * g.nx * g.ny + (long long)(j + g.lo[1]) * g.nx + (i + g.lo[0]);
    const Curv lo = curv_voxel(c.dist, c.weight, c.nx, c.ny, c.nz, (double)c.vs, dl);
    Curv out = lo;
    unsigned char nvalid = lo.valid ? 2 : 0;
    if (type != 3) {
        const long long dh = dl + (type == 0 ? 1ll : type == 1 ? (long long)g.nx : (long long)g.nx * g.ny);
        const Curv hi = curv_voxel(c.dist, c.weight, c.nx, c.ny, c.nz, (double)c.vs, dh);
        nvalid = (unsigned char)(lo.valid + hi.valid);
        if (lo.valid && hi.valid) {
            const float tl = -g.dist[dl], th = -g.dist[dh];
            double mu = (double)((0.0f - tl) / (th - tl));      // k_wmesh_verts's interpolation parameter
            if (mu > 1.0) mu = 1.0; else if (mu < 0) mu = 0.0;
            const double m = (double)(float)mu;
            out.mean = (float)((double)lo.mean + m * ((double)hi.mean - (double)lo.mean));
            out.gauss = (float)((double)lo.gauss + m * ((double)hi.gauss - (double)lo.gauss));
            out.k1 = (float)((double)lo.k1 + m * ((double)hi.k1 - (double)lo.k1));
            out.k2 = (float)((double)lo.k2 + m * ((double)hi.k2 - (double)lo.k2));
        } else if (hi.valid) out = hi;
    }
    v_valid[v] = nvalid; v_mean[v] = out.mean; v_gauss[v] = out.gauss; v_k1[v] = out.k1; v_k2[v] = out.k2;      // (an invalid voxel holds zeros)
}

__global__ void __launch_bounds__(kBlock) k_bake_curv(CurvGrid c, const int* __restrict__ voxel, long long n, float* __restrict__ mean, unsigned char* __restrict__ valid) {
    const long long t = blockIdx.x * (long long)blockDim.x + threadIdx.x;
    if (t >= n) return;
    const int lin = voxel[t];
    Curv r{};
    if (lin >= 0) r = curv_voxel(c.dist, c.weight, c.nx, c.ny, c.nz, (double)c.vs, (long long)lin);
    mean[t] = r.mean; valid[t] = r.valid;
}

unsigned blocks(long long n) { return (unsigned)std::max<long long>(1, (n + kBlock - 1) / kBlock); }

}  // namespace

void launch_curv_voxels(const CurvGrid& c, const long long* lin, long long n, unsigned char* valid, float* mean, float* gauss, float* k1, float* k2, float* dir1, hipStream_t s) {
    hipLaunchKernelGGL(k_curv_voxels, dim3(blocks(n)), dim3(kBlock), 0, s, c, lin, n, valid, mean, gauss, k1, k2, dir1);
}
void launch_wmesh_curv(const CurvGrid& c, const WMeshGrid& g, const int* num, int n_verts, unsigned char* v_valid, float* v_mean, float* v_gauss, float* v_k1, float* v_k2, hipStream_t s) {
    hipLaunchKernelGGL(k_wmesh_curv, dim3(blocks(g.nown)), dim3(kBlock), 0, s, c, g, num, n_verts, v_valid, v_mean, v_gauss, v_k1, v_k2);
}
void launch_bake_curv(const CurvGrid& c, const int* voxel, long long n, float* mean, unsigned char* valid, hipStream_t s) {
    hipLaunchKernelGGL(k_bake_curv, dim3(blocks(n)), dim3(kBlock), 0, s, c, voxel, n, mean, valid);
}

}  // namespace psg
