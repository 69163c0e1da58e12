// query.h -- the launchers of query.hip (psgsdf_query_points, psgsdf_project_points, psgsdf_cast_rays: include/psgsdf_query.h; DESIGN.md 22 "Field
// queries"), called from extract_query.hip.
#pragma once
#include "engine.h"

namespace psg {

enum { QC_OK = 0, QC_OUTSIDE, QC_UNOBSERVED, QC_INVALID, QC_NOT_CONVERGED, kQueryCounts };      // points and projections: one count per status byte
enum { QR_VALID = 0, QR_HITS, QR_BURIED, kQueryRayCounts };
constexpr long long kQueryChunk = 1ll << 30;      // queries per launch (a dispatch's work-items are a 32-bit count); PSGSDF_QUERY_CHUNK: a smaller multiple of 64

// the eight dense planes of a single-rank context, as psgsdf_download_volume returns them
struct QueryField { const float* dist; const float* g[3]; const float* weight; const float* rho[3]; int dim[3]; double vs; };

struct QueryArgs {
    QueryField f;
    long long n;                         // queries
    long long g0;                        // the first query of this launch (set by the launcher)
    const float* pts;                    // [n][3] the caller's points
    int max_iters; double tol;           // projection
    unsigned char* status;               // [n]
    float* dist;                         // [n] points: (float) phi; projection: the residual
    float* normal;                       // [n][3]
    float* rgb;                          // [n][3] points
    float* weight;                       // [n] points
    long long* voxel;                    // [n]
    float* xyz;                          // [n][3] projection: the point at the stop
    unsigned char* iters;                // [n] projection
    float* moved;                        // [n] projection: the signed distance moved
    unsigned long long* counts;          // [kQueryCounts], zeroed
};

struct QueryRayArgs {
    RenderArgs r;                        // the renderer's prepared state (occlusion.h): dense planes, grid, brick map and box
    long long n, g0;
    const float* org; const float* dir;  // [n][3]
    double t_min, span, vs;              // span = t_max - t_min
    float t_cut;                         // the walk's cut: (float) span (FLT_MAX: none)
    unsigned char* status;               // [n]
    float* t;                            // [n]
    float* xyz; float* normal; float* rgb;      // [n][3]
    long long* voxel;                    // [n]
    unsigned long long* counts;          // [kQueryRayCounts], zeroed
};

// chunk: queries per launch, a multiple of 64 (no wavefront straddles two launches).  Every launch is checked: the first error is returned
hipError_t launch_query_points(QueryArgs a, int model, long long chunk, hipStream_t s);
hipError_t launch_query_project(QueryArgs a, int model, long long chunk, hipStream_t s);
hipError_t launch_query_rays(QueryRayArgs a, long long chunk, hipStream_t s);

}  // namespace psg
