// compare.h -- the launchers of compare.hip (psgsdf_compare_reference: include/psgsdf_compare.h; DESIGN.md "Comparison with a reference"), called
// from extract_compare.hip.
#pragma once
#include "engine.h"

namespace psg {

// the integers of one direction, reduced on the device (k_cmp_stats)
enum { CS_VALID = 0, CS_MATCHED, CS_TAU, CS_SUM_D, CS_SUM_D2, CS_SIGNED, CS_MAX, CS_PAIRS, CS_HIST, kCmpStats = CS_HIST + 16 };
constexpr long long kCompareChunk = 1ll << 24;        // queries per launch (64 lanes each: a dispatch's work-items are a 32-bit count)
constexpr int kCompareStatBlocks = 128;               // workgroups of the statistics kernel (512 wavefronts: that many atomics per field at most)
constexpr long long kCompareMaxCells = 1ll << 25;     // cells of the search grid (two ints each); a finer grid_cell is coarsened to fit

// the uniform search grid over one direction's targets: cell (i, j, k) holds entries[start[l] .. start[l + 1]) with l = (k n[1] + j) n[0] + i, the
// targets whose bounding box overlaps it, in whatever order the atomics gave
struct CompareGrid {
    double lo[3], h;                     // the box's lower corner and the cells' edge
    int n[3];
    long long cells;                     // n[0] n[1] n[2]
    int* start;                          // [cells + 1]: counts, then their exclusive scan
    int* cursor;                         // [cells], zeroed: the fill's position inside each cell
    int* entries;                        // [start[cells]]
};

struct CompareArgs {
    CompareGrid g;
    // targets: triangles t_faces[nt][3] over t_xyz, or (t_faces == nullptr) the points t_xyz[nt][3]
    const float* t_xyz; const int* t_faces; int nt;
    // queries
    const float* q_xyz; long long nq;
    long long q0, q1;                    // this launch's queries [q0, q1) (set by the launcher)
    double max_dist, tau, vs;
    double* d;                           // [nq] the distance in double: NaN invalid, +inf unmatched (what the statistics are formed from)
    float* dist; int* nearest; signed char* side; int* pairs;      // [nq]; pairs: candidate pairs evaluated for the query
    unsigned long long* total;           // [1], zeroed: the entries the grid needs (k_cmp_total)
    unsigned long long* stats;           // [kCmpStats], zeroed
};

hipError_t launch_compare_total(const CompareArgs& a, hipStream_t s);      // a.total
hipError_t launch_compare_count(const CompareArgs& a, hipStream_t s);      // a.g.start = the counts
hipError_t launch_compare_fill(const CompareArgs& a, hipStream_t s);       // a.g.entries (start scanned, cursor zeroed)
// the queries in launches of at most `chunk`, every launch checked: the first error is returned
hipError_t launch_compare_query(CompareArgs a, long long chunk, hipStream_t s);
hipError_t launch_compare_stats(const CompareArgs& a, hipStream_t s);

}  // namespace psg
