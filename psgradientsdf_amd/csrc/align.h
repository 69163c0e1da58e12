// align.h -- the launchers of align.hip (psgsdf_align_reference: include/psgsdf_align.h; DESIGN.md "Alignment of a reference"), called from
// extract_compare.hip.  The search between a move and its rows is compare.hip's k_cmp_query (launch_compare_query), unchanged.
#pragma once
#include "compare.h"

namespace psg {

constexpr int kAlignRowBlocks = 128;      // workgroups of a row kernel at most: the order of the sums depends on the number of queries only
// one partial row: A's upper triangle row-major (21), g (6), e, the rows, the candidate pairs the search evaluated for the lane's queries
enum { AL_A = 0, AL_G = 21, AL_E = 27, AL_N = 28, AL_PAIRS = 29, kAlignRow = 30 };
// the folded system: A, g, e over both directions (28), then the rows and the candidate pairs per direction
enum { AS_N = 28, AS_PAIRS = 30, kAlignSys = 32 };

struct AlignMoveArgs {
    double M[12];                        // 3x4 row-major
    const float* src; float* dst; long long n;
};

struct AlignRowArgs {
    CompareArgs s;                       // the search these rows follow: its queries (the moved points), targets, nearest and pairs
    double T[12];                        // direction 2: the closest point, in the reference's units, goes through T (reference -> mesh units)
    const float* v_xyz; const float* v_nrm;      // direction 2: the mesh's vertices and their stored normals
    double c[3], vs;
    double* partial;                     // [workgroups][kAlignRow]
};

inline unsigned align_row_blocks(long long nq) { return (unsigned)std::min<long long>((nq + kBlock - 1) / kBlock, kAlignRowBlocks); }

hipError_t launch_align_move(const AlignMoveArgs& a, hipStream_t s);
hipError_t launch_align_rows(const AlignRowArgs& a, int dir, hipStream_t s);      // dir 1 or 2; align_row_blocks(a.s.nq) partial rows
// sys[kAlignSys] = the partial rows of direction 1 (nb1 of them), then those of direction 2, added in that order
hipError_t launch_align_fold(const double* p1, int nb1, const double* p2, int nb2, double* sys, hipStream_t s);

}  // namespace psg
