// query.hip -- the field asked at the caller's points and along the caller's rays (include/psgsdf_query.h):
//   k_query_points<MODEL>    one lane per point: the model's distance, normal, colour and weight there
//   k_query_project<MODEL>   one lane per point: steps of phi along the model's normal until |phi| <= tol, the point leaves the observed grid or
//                            max_iters moves are made
//   k_query_rays             one lane per ray through the renderer's own cells (render_trace.h), cut at t_max - t_min, exactly as k_occlusion walks
//   One device function per model (query_eval) evaluates the field; the points kernel and the projection loop share it, so there is one copy of the
//   arithmetic: double, no contraction, in the order the header writes it.  The trilinear cell goes channel by channel (eight loads, seven lerps):
//   what is held across channels are the three fractions and the eight gradient lengths, never 8 x 8 values.
//   Queries arrive in the caller's order: a wavefront reads its 64 x 3 floats as one contiguous 768-byte run, the gathers behind it are uncoalesced
//   by nature and lean on L2 and the Infinity Cache.  Outputs are SoA, plain stores by the query's own lane; the counts are the wavefront's ballots,
//   added by one lane with integer atomics (integers: the same totals in whatever order).  No LDS, no barrier.
#include "device_common.h"
#include "render_trace.h"
#include "bake.h"
#include "query.h"

namespace psg {

// m(v): the stored gradient normalised in double, zero where its squared length is not > 0
__device__ __forceinline__ void query_unit(const float* const* g, long long v, double* m) {
#pragma clang fp contract(off)
    const double gx = (double)g[0][v], gy = (double)g[1][v], gz = (double)g[2][v];
    const double s = (gx * gx + gy * gy) + gz * gz;
    if (s > 0.0) { const double r = sqrt(s); m[0] = gx / r; m[1] = gy / r; m[2] = gz / r; }
    else { m[0] = 0.0; m[1] = 0.0; m[2] = 0.0; }
}

__device__ __forceinline__ double query_lerp(double A, double B, double t) {
#pragma clang fp contract(off)
    return A + t * (B - A);
}

// one channel of the trilinear cell whose lowest corner is `lin`: x first, then y, then z.  r (if given): the corners' gradient lengths, the
// channel is then a component of m(v) (zero where the length is)
__device__ __forceinline__ double query_tri(const float* plane, long long lin, int nx, long long nxy, const double* fr, const double* r = nullptr) {
#pragma clang fp contract(off)
    double X[4];
#pragma unroll
    for (int yz = 0; yz < 4; ++yz) {
        const long long at = lin + (long long)(yz & 1) * nx + (long long)(yz >> 1) * nxy;
        double A = (double)plane[at], B = (double)plane[at + 1];
        if (r) { A = r[2 * yz] > 0.0 ? A / r[2 * yz] : 0.0; B = r[2 * yz + 1] > 0.0 ? B / r[2 * yz + 1] : 0.0; }
        X[yz] = query_lerp(A, B, fr[0]);
    }
    return query_lerp(query_lerp(X[0], X[1], fr[1]), query_lerp(X[2], X[3], fr[1]), fr[2]);
}

// The model at p: the status byte (0 ok, 1 outside, 2 unobserved); phi and the normal for status 0; the voxel (-1 where the header says so);
// FULL: also the colour and the weight.  The grid test is written so that a coordinate that is not a number is outside: nothing is ever indexed
// with a cell that was not compared against both ends of its axis.
template <int MODEL, bool FULL>
__device__ __forceinline__ int query_eval(const QueryField& f, const double* p, double& phi, double* nrm, long long& vox, double* col, double& wgt) {
#pragma clang fp contract(off)
    const int nx = f.dim[0];
    const long long nxy = (long long)f.dim[0] * f.dim[1];
    double c[3], fr[3];
    bool inside = true;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const double u = MODEL == 0 ? p[a] / f.vs + 0.5 : p[a] / f.vs;
        c[a] = floor(u);
        fr[a] = u - c[a];
        inside = inside && c[a] >= 0.0 && c[a] < (double)(MODEL == 0 ? f.dim[a] : f.dim[a] - 1);
    }
    vox = -1;
    if (!inside) return 1;
    const long long lin = ((long long)c[2] * f.dim[1] + (long long)c[1]) * nx + (long long)c[0];
    if (MODEL == 0) {
        vox = lin;
        const float w = f.weight[lin];
        if (!(w > 0.f)) return 2;
        query_unit(f.g, lin, nrm);
        double e[3];
#pragma unroll
        for (int a = 0; a < 3; ++a) e[a] = p[a] - f.vs * c[a];
        phi = (double)f.dist[lin] + ((nrm[0] * e[0] + nrm[1] * e[1]) + nrm[2] * e[2]);
        if (FULL) { col[0] = (double)f.rho[0][lin]; col[1] = (double)f.rho[1][lin]; col[2] = (double)f.rho[2][lin]; wgt = (double)w; }
        return 0;
    }
    bool observed = true;
#pragma unroll
    for (int i = 0; i < 8; ++i) observed = observed && f.weight[lin + (i & 1) + (long long)((i >> 1) & 1) * nx + (long long)(i >> 2) * nxy] > 0.f;
    if (!observed) return 2;
    vox = lin;
    phi = query_tri(f.dist, lin, nx, nxy, fr);
    double r[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const long long at = lin + (i & 1) + (long long)((i >> 1) & 1) * nx + (long long)(i >> 2) * nxy;
        const double gx = (double)f.g[0][at], gy = (double)f.g[1][at], gz = (double)f.g[2][at];
        const double s = (gx * gx + gy * gy) + gz * gz;
        r[i] = s > 0.0 ? sqrt(s) : 0.0;
    }
    double S[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) S[a] = query_tri(f.g[a], lin, nx, nxy, fr, r);
    const double ss = (S[0] * S[0] + S[1] * S[1]) + S[2] * S[2];
    if (ss > 0.0) { const double l = sqrt(ss); nrm[0] = S[0] / l; nrm[1] = S[1] / l; nrm[2] = S[2] / l; }
    else { nrm[0] = 0.0; nrm[1] = 0.0; nrm[2] = 0.0; }
    if (FULL) {
#pragma unroll
        for (int a = 0; a < 3; ++a) col[a] = query_tri(f.rho[a], lin, nx, nxy, fr);
        wgt = query_tri(f.weight, lin, nx, nxy, fr);
    }
    return 0;
}

// the caller's point j widened; false if one of its three floats is not finite (raw: the floats as they came)
__device__ __forceinline__ bool query_point(const float* pts, long long j, float* raw, double* p) {
    bool finite = true;
#pragma unroll
    for (int a = 0; a < 3; ++a) { raw[a] = pts[3 * j + a]; finite = finite && isfinite(raw[a]); p[a] = (double)raw[a]; }
    return finite;
}

// the status counts of one wavefront (st < 0: no query on this lane)
__device__ __forceinline__ void query_count(unsigned long long* counts, int st, int n_status) {
    const int lane = threadIdx.x & 63;
    for (int k = 0; k < n_status; ++k) {
        const unsigned long long b = __ballot(st == k);
        if (lane == 0 && b) atomicAdd(counts + k, (unsigned long long)__popcll(b));
    }
}

template <int MODEL>
__global__ void __launch_bounds__(64) k_query_points(QueryArgs a) {
#pragma clang fp contract(off)
    const long long j = a.g0 + (long long)blockIdx.x * 64 + (threadIdx.x & 63);
    int st = -1;
    if (j < a.n) {
        float raw[3], o_dist = 0.f, o_n[3] = {0.f, 0.f, 0.f}, o_c[3] = {0.f, 0.f, 0.f}, o_w = 0.f;
        double p[3], phi = 0.0, nrm[3], col[3], wgt = 0.0;
        long long vox = -1;
        if (!query_point(a.pts, j, raw, p)) st = 3;
        else {
            st = query_eval<MODEL, true>(a.f, p, phi, nrm, vox, col, wgt);
            if (st == 0) {
                o_dist = (float)phi; o_w = (float)wgt;
#pragma unroll
                for (int k = 0; k < 3; ++k) { o_n[k] = (float)nrm[k]; o_c[k] = (float)col[k]; }
            }
        }
        a.status[j] = (unsigned char)st; a.dist[j] = o_dist; a.weight[j] = o_w; a.voxel[j] = vox;
#pragma unroll
        for (int k = 0; k < 3; ++k) { a.normal[3 * j + k] = o_n[k]; a.rgb[3 * j + k] = o_c[k]; }
    }
    query_count(a.counts, st, 4);
}

template <int MODEL>
__global__ void __launch_bounds__(64) k_query_project(QueryArgs a) {
#pragma clang fp contract(off)
    const long long j = a.g0 + (long long)blockIdx.x * 64 + (threadIdx.x & 63);
    int st = -1;
    if (j < a.n) {
        float raw[3], o_x[3], o_res = 0.f, o_n[3] = {0.f, 0.f, 0.f}, o_moved = 0.f;
        double p[3];
        long long vox = -1;
        int k = 0;
        if (!query_point(a.pts, j, raw, p)) { st = 3; o_x[0] = raw[0]; o_x[1] = raw[1]; o_x[2] = raw[2]; }
        else {
            const double p0[3] = {p[0], p[1], p[2]};
            double phi = 0.0, nrm[3], col[3], wgt, sg = 1.0;
            bool started = false;
            for (;;) {
                const int s = query_eval<MODEL, false>(a.f, p, phi, nrm, vox, col, wgt);
                if (k == 0 && s == 0) { started = true; sg = phi < 0.0 ? -1.0 : 1.0; }
                if (s != 0) { st = s; break; }
                if (fabs(phi) <= a.tol) { st = 0; break; }
                if (k == a.max_iters) { st = 4; break; }
#pragma unroll
                for (int q = 0; q < 3; ++q) p[q] = p[q] - phi * nrm[q];
                ++k;
            }
            if (st == 0 || st == 4) { o_res = (float)phi; o_n[0] = (float)nrm[0]; o_n[1] = (float)nrm[1]; o_n[2] = (float)nrm[2]; }
            if (started) {
                const double dx = p[0] - p0[0], dy = p[1] - p0[1], dz = p[2] - p0[2];
                o_moved = (float)(sg * sqrt((dx * dx + dy * dy) + dz * dz));
            }
            o_x[0] = (float)p[0]; o_x[1] = (float)p[1]; o_x[2] = (float)p[2];
        }
        a.status[j] = (unsigned char)st; a.dist[j] = o_res; a.voxel[j] = vox; a.iters[j] = (unsigned char)k; a.moved[j] = o_moved;
#pragma unroll
        for (int q = 0; q < 3; ++q) { a.xyz[3 * j + q] = o_x[q]; a.normal[3 * j + q] = o_n[q]; }
    }
    query_count(a.counts, st, kQueryCounts);
}

__global__ void __launch_bounds__(64) k_query_rays(QueryRayArgs a) {
#pragma clang fp contract(off)
    const int lane = threadIdx.x & 63;
    const long long j = a.g0 + (long long)blockIdx.x * 64 + lane;
    bool valid = false, hit = false, buried = false;
    if (j < a.n) {
        double o[3], w[3];
        bool finite = true;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const float x = a.org[3 * j + k], y = a.dir[3 * j + k];
            finite = finite && isfinite(x) && isfinite(y);
            o[k] = (double)x; w[k] = (double)y;
        }
        valid = finite && bake_unit(w);
        float o_t = 0.f, o_x[3] = {0.f, 0.f, 0.f}, o_n[3] = {0.f, 0.f, 0.f}, o_c[3] = {0.f, 0.f, 0.f};
        long long vox = -1;
        if (valid) {
            float uo[3], uw[3];
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const double os = o[k] + a.t_min * w[k];
                uo[k] = (float)(os / a.vs + 0.5); uw[k] = (float)(w[k] / a.vs);
            }
            float t = 0.f; long long lin = -1;
            const bool found = render_trace<false, true>(a.r, uo, uw, t, lin, a.t_cut);
            hit = found && (double)t <= a.span;
            if (hit) {
                buried = t == 0.f;
                const double T = (double)t + a.t_min;
                double m[3];
                query_unit(a.r.d.g, lin, m);
                o_t = (float)T; vox = lin;
#pragma unroll
                for (int k = 0; k < 3; ++k) { o_x[k] = (float)(o[k] + T * w[k]); o_n[k] = (float)m[k]; o_c[k] = a.r.d.rho[k][lin]; }
            }
        }
        a.status[j] = (unsigned char)(!valid ? 3 : !hit ? 1 : buried ? 2 : 0); a.t[j] = o_t; a.voxel[j] = vox;
#pragma unroll
        for (int k = 0; k < 3; ++k) { a.xyz[3 * j + k] = o_x[k]; a.normal[3 * j + k] = o_n[k]; a.rgb[3 * j + k] = o_c[k]; }
    }
    const unsigned long long b_valid = __ballot(valid), b_hit = __ballot(hit), b_bur = __ballot(buried);
    if (lane == 0) {
        if (b_valid) atomicAdd(a.counts + QR_VALID, (unsigned long long)__popcll(b_valid));
        if (b_hit) atomicAdd(a.counts + QR_HITS, (unsigned long long)__popcll(b_hit));
        if (b_bur) atomicAdd(a.counts + QR_BURIED, (unsigned long long)__popcll(b_bur));
    }
}

// A dispatch counts its work-items in 32 bits: the queries go out in launches of at most `chunk` (a multiple of 64: no wavefront straddles two
// launches), the kernel adding the launch's 64-bit base to its lane.
template <class Args, class Launch> static hipError_t query_chunks(Args& a, long long chunk, Launch&& launch) {
    for (a.g0 = 0; a.g0 < a.n; a.g0 += chunk) {
        launch((unsigned)((std::min(a.n - a.g0, chunk) + 63) / 64));
        if (hipError_t e = hipGetLastError()) return e;
    }
    return hipSuccess;
}

hipError_t launch_query_points(QueryArgs a, int model, long long chunk, hipStream_t s) {
    return query_chunks(a, chunk, [&](unsigned blocks) {
        if (model == 0) hipLaunchKernelGGL(k_query_points<0>, dim3(blocks), dim3(64), 0, s, a);
        else hipLaunchKernelGGL(k_query_points<1>, dim3(blocks), dim3(64), 0, s, a);
    });
}

hipError_t launch_query_project(QueryArgs a, int model, long long chunk, hipStream_t s) {
    return query_chunks(a, chunk, [&](unsigned blocks) {
        if (model == 0) hipLaunchKernelGGL(k_query_project<0>, dim3(blocks), dim3(64), 0, s, a);
        else hipLaunchKernelGGL(k_query_project<1>, dim3(blocks), dim3(64), 0, s, a);
    });
}

hipError_t launch_query_rays(QueryRayArgs a, long long chunk, hipStream_t s) {
    return query_chunks(a, chunk, [&](unsigned blocks) { hipLaunchKernelGGL(k_query_rays, dim3(blocks), dim3(64), 0, s, a); });
}

}  // namespace psg
