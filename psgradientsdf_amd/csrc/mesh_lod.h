// mesh_lod.h -- the launchers of mesh_lod.hip (psgsdf_extract_mesh_lod, include/psgsdf_mesh.h; DESIGN.md "Level of detail"), called from extract_mesh.hip.
#pragma once
#include <hip/hip_runtime.h>

namespace psg {

// per cluster slot kMlodAcc 64-bit integers, zeroed first: members, the fixed-point sums of the positions (2^20 units per voxel) and of the normals
// (2^20 units per unit length), the sums of the colour bytes
enum { ML_COUNT = 0, ML_POS = 1, ML_NRM = 4, ML_RGB = 7, kMlodAcc = 10 };
constexpr double kMlodFix = 1048576.0;
constexpr long long kMlodLimit = 1ll << 20;      // |cluster coordinate| < 2^20

struct MlodTables {
    unsigned long long* keys;   // [vcap] cluster keys, pre-filled with 0xff bytes
    long long* acc;             // [vcap][kMlodAcc], zeroed
    int* first;                 // [vcap] smallest member, pre-filled with 0x7f bytes
    int* used;                  // [vcap] 1 where a kept face uses the cluster, zeroed
    int* vslot;                 // [nv] slot of the vertex's cluster
    int* ftab;                  // [fcap] smallest face index of the slot's triple, pre-filled with 0xff bytes (-1)
    int* fslot;                 // [nf] slot of the face's triple, -1: two of its clusters are equal
    int* bad;                   // [1] set where a cluster coordinate is beyond the limit, zeroed
    unsigned long long vcap, fcap;
};
// one thread per vertex: cluster key -> slot, the slot's sums, members and smallest member
void launch_mlod_cluster(const float* xyz, const float* nrm, const unsigned char* rgb, int nv, double cell, double vs, const MlodTables& t, hipStream_t s);
// one thread per face: collapsed?  otherwise its unordered triple's slot, which ends up holding the smallest face index of that triple
void launch_mlod_ftable(const int* faces, int nf, const MlodTables& t, hipStream_t s);
// one thread per face: fflag = kept (the slot holds its own index); the clusters of kept faces flagged used
void launch_mlod_fkeep(const int* faces, int nf, const MlodTables& t, int* fflag, hipStream_t s);
// one thread per vertex: vflag = it is the smallest member of a used cluster
void launch_mlod_vflag(int nv, const MlodTables& t, int* vflag, hipStream_t s);
// vnum / fnum: the exclusive scans of the flags.  Output vertices (from the smallest members), faces and the map of every input vertex
void launch_mlod_emit(const float* xyz, const float* nrm, const unsigned char* rgb, int nv, const int* faces, int nf, double vs, const MlodTables& t, const int* vnum, const int* fnum,
                      float* oxyz, float* onrm, unsigned char* orgb, int* ofaces, int* vmap, hipStream_t s);

}  // namespace psg
