// extract_mesh.hip -- the C ABI of include/psgsdf_mesh.h: the welded, indexed mesh of the context's state (kernels: mesh.hip; DESIGN.md "Welded
// meshes"), its connected components and the mesh without its small pieces (mesh_cc.hip; "Mesh components") and a level-of-detail mesh by vertex
// clustering (mesh_lod.hip; "Level of detail"); and the C ABI of include/psgsdf_fit.h: the photometric fit per band row and per vertex of the welded
// mesh (fit.hip; "Photometric fit per voxel and vertex"); and the C ABI of include/psgsdf_bake.h: detail maps of the level-of-detail mesh (bake.hip;
// "Baked detail maps"); and the C ABI of include/psgsdf_occlusion.h: ambient occlusion at the caller's points and as a map of the bake
// (occlusion.hip; "Ambient occlusion"); and the C ABI of include/psgsdf_compare.h: distances to a reference mesh or cloud (compare.hip;
// "Comparison with a reference") and of include/psgsdf_align.h: its rigid alignment to the mesh (align.hip; "Alignment of a reference").  Each call is a chain of stages -- welded mesh -> components -> clusters, or band fit ->
// welded mesh -> vertex fit -- that hand each other device arrays whose kernels may still be in flight.  The CALL owns all device memory of its
// stages in one DevMem, which waits for the stream and frees when the call returns, whichever way it returns: a stage allocates from it and never frees.
// The frame arithmetic (extract_internal.h crop_frame) runs on the host and its results are compared bit for bit: no FMA contraction here either.
#pragma clang fp contract(off)
#include "extract_internal.h"
#include "../../include/psgsdf_mesh.h"
#include "../../include/psgsdf_fit.h"
#include "../../include/psgsdf_bake.h"
#include "../../include/psgsdf_occlusion.h"
#include "../../include/psgsdf_compare.h"
#include "../../include/psgsdf_align.h"
#include "mesh_lod.h"
#include "bake.h"
#include "occlusion.h"
#include "compare.h"
#include "align.h"

using namespace psge;

namespace {
// a mesh as device arrays, the kernels that write them launched on the stream and not waited for
struct MeshView { const float *xyz = nullptr, *nrm = nullptr; const unsigned char* rgb = nullptr; const int* faces = nullptr; int nv = 0, nf = 0; };

// ---- stage 1: the welded mesh of the context's state (this rank's share).  nv == 0 && nf == 0: nothing was launched for it
struct WMeshDev : MeshView { long long first = 0; psg::WMeshGrid grid{}; const int* num = nullptr; };      // grid, num: the key slots and their vertex numbers (the scan of the used-key flags)
int wmesh_device(psgsdf_ctx* c, DevMem& mem, WMeshDev* m) {
    const char* me = "extract_mesh_indexed";
    int lo[3], hi[3]; bool any = false;
    { int rc = crop_box_dev(c, lo, hi, &any); if (rc) return rc; }      // (collective: every rank takes the same early returns below)
    if (!any) return PSGSDF_OK;
    psg::WMeshGrid g{}; int zc1 = 0;
    if (!crop_frame(c, lo, hi, g, &zc1)) return PSGSDF_OK;      // psgsdf_extract_mesh's frame
    for (int a = 0; a < 3; ++a) g.g[a] = c->dense.g[a];
    g.zh = -1;
    const long long P = 4ll * g.d[0] * g.d[1];      // key slots per plane
    if (P * (g.d[2] + 1) >= (1ll << 31)) return fail(c, PSGSDF_ERR_UNSUPPORTED, "%s: %lld key slots", me, P * (g.d[2] + 1));
    // this context: the cells whose lower plane it owns, the key planes it owns [kp0, kp1) and the one above (the upper neighbour's first plane)
    const int kp1 = std::min(g.d[2], c->z1 - lo[2]);
    const long long ncell = (long long)(g.d[0] - 2) * (g.d[1] - 2) * std::max(0, zc1 - g.zc0);
    g.nown = P * std::max(0, kp1 - g.zc0);
    const bool up = c->rank + 1 < c->n_ranks, down = c->rank > 0;
    const size_t plane = (size_t)g.nx * g.ny;
    // temporaries: flags / vertex numbers (4 ints per voxel of the crop planes + one plane), face counts (1 int per cell), scan sums, the exchanged planes
    const long long nflag = g.nown + P, nscan = std::max(g.nown, ncell);
    int *flag = nullptr, *cnt = nullptr, *sums = nullptr, *xin = nullptr; float* halo = nullptr;
    bool ok = mem.get(&flag, (size_t)nflag) && mem.get(&cnt, (size_t)std::max(1ll, ncell)) && mem.get(&sums, (size_t)((nscan + psg::kTile - 1) / psg::kTile + 1));
    if (ok && c->n_ranks > 1) ok = mem.get(&xin, (size_t)(2 * P)) && (!up || mem.get(&halo, 6 * plane));
    if (c->n_ranks > 1) {      // every rank learns whether all of them have their temporaries before anyone enters an exchange
        std::vector<double> st(1, ok ? 0.0 : 1.0);
        if (int rc = host_allreduce(c, st, me)) return rc;
        if (st[0] != 0.0) return fail(c, PSGSDF_ERR_DEVICE, "%s: out of memory on %d rank(s)", me, (int)st[0]);
    } else if (!ok) return fail(c, PSGSDF_ERR_DEVICE, "%s: out of memory", me);
    int rc = 0;
    if (hipMemsetAsync(flag, 0, sizeof(int) * (size_t)nflag, c->stream) != hipSuccess) rc = fail(c, PSGSDF_ERR_DEVICE, "%s: memset", me);
    if (!rc && ncell > 0) timed(c, "wmesh_mark", [&] { psg::launch_wmesh_mark(g, ncell, cnt, flag, c->stream); });
    if (c->n_ranks > 1) {      // (entered even after a local failure: the neighbours wait for it)
        // the used flags of plane z1 go up and are OR-ed into the owner's first plane; the gradient and albedo of plane z0 go down (z-edges z1 - 1 -> z1)
        std::vector<psgsdf_comm_xfer> sends, recvs;
        if (up) {
            sends.push_back({(void*)(flag + g.nown), sizeof(int) * (size_t)P, c->rank + 1});
            for (int a = 0; a < 3; ++a) {
                recvs.push_back({(void*)(halo + plane * a), sizeof(float) * plane, c->rank + 1});
                recvs.push_back({(void*)(halo + plane * (3 + a)), sizeof(float) * plane, c->rank + 1});
                g.hg[a] = halo + plane * a; g.hrho[a] = halo + plane * (3 + a);
            }
            g.zh = c->z1;
        }
        if (down) {
            recvs.push_back({(void*)xin, sizeof(int) * (size_t)P, c->rank - 1});
            for (int a = 0; a < 3; ++a) {
                sends.push_back({(void*)(c->dense.g[a] + plane * (size_t)(c->z0 - c->zlo)), sizeof(float) * plane, c->rank - 1});
                sends.push_back({(void*)(c->dense.rho[a] + plane * (size_t)(c->z0 - c->zlo)), sizeof(float) * plane, c->rank - 1});
            }
        }
        if (int r2 = comm_xfer(c, sends, recvs)) rc = rc ? rc : r2;
        if (!rc && down && g.nown > 0) psg::launch_wmesh_or(flag, xin, P, c->stream);
    }
    int nv = 0, nf = 0;
    if (!rc && g.nown > 0) rc = scan_counts(c, flag, g.nown, sums, &nv);      // flags -> vertex numbers (key order)
    if (!rc && ncell > 0) rc = scan_counts(c, cnt, ncell, sums, &nf);         // face counts -> face offsets
    // the ranks' vertex counts: this share's first global vertex number, the upper neighbour's
    long long first = 0, first_up = 0, total_v = nv;
    if (c->n_ranks > 1) {
        std::vector<double> all((size_t)c->n_ranks + 1, 0.0);
        all[(size_t)c->rank] = rc ? 0.0 : (double)nv; all[(size_t)c->n_ranks] = rc ? 1.0 : 0.0;
        if (int r2 = host_allreduce(c, all, me)) return r2;
        if (all[(size_t)c->n_ranks] != 0.0 && !rc) rc = fail(c, PSGSDF_ERR_COMM, "%s: another rank failed", me);
        total_v = 0;
        for (int r = 0; r < c->n_ranks; ++r) { if (r < c->rank) first += (long long)all[(size_t)r]; if (r == c->rank + 1) first_up = first + nv; total_v += (long long)all[(size_t)r]; }
    }
    if (!rc && total_v > INT32_MAX) rc = fail(c, PSGSDF_ERR_UNSUPPORTED, "%s: %lld vertices", me, total_v);
    if (!rc && c->n_ranks > 1) {      // the vertex numbers of plane z1 come back down from its owner (as its local numbers; + first_up)
        std::vector<psgsdf_comm_xfer> sends, recvs;
        if (down) sends.push_back({(void*)flag, sizeof(int) * (size_t)P, c->rank - 1});
        if (up) recvs.push_back({(void*)(xin + P), sizeof(int) * (size_t)P, c->rank + 1});
        rc = comm_xfer(c, sends, recvs);
    }
    if (rc) return rc;
    m->nv = nv; m->nf = nf; m->first = first;
    if (nv == 0 && nf == 0) return PSGSDF_OK;
    float *xyz = nullptr, *nrm = nullptr; unsigned char* rgb = nullptr; int* faces = nullptr;
    if ((nv > 0 && !(mem.get(&xyz, 3 * (size_t)nv) && mem.get(&nrm, 3 * (size_t)nv) && mem.get(&rgb, 3 * (size_t)nv))) || (nf > 0 && !mem.get(&faces, 3 * (size_t)nf)))
        return fail(c, PSGSDF_ERR_DEVICE, "%s: out of memory (%d vertices, %d faces)", me, nv, nf);
    if (nf > 0) timed(c, "wmesh_faces", [&] { psg::launch_wmesh_faces(g, ncell, cnt, nf, flag, (int)first, xin ? xin + P : nullptr, (int)first_up, faces, c->stream); });
    if (nv > 0) timed(c, "wmesh_verts", [&] { psg::launch_wmesh_verts(g, flag, nv, xyz, nrm, rgb, c->stream); });
    m->xyz = xyz; m->nrm = nrm; m->rgb = rgb; m->faces = faces; m->grid = g; m->num = flag;
    return PSGSDF_OK;
}
}  // namespace

extern "C" int psgsdf_extract_mesh_indexed(psgsdf_ctx* c, const float** xyz, const float** normals, const uint8_t** rgb, int64_t* n_vertices,
                                           const int32_t** faces, int64_t* n_faces, int64_t* first_vertex) {
    const char* me = "extract_mesh_indexed";
    if (!xyz || !normals || !rgb || !n_vertices || !faces || !n_faces || !first_vertex) return fail(c, PSGSDF_ERR_ARG, "%s: null argument", me);
    { int rc = extract_ready(c, me); if (rc) return rc; }
    *xyz = nullptr; *normals = nullptr; *rgb = nullptr; *faces = nullptr; *n_vertices = 0; *n_faces = 0; *first_vertex = 0;
    DevMem mem(c);
    WMeshDev m;
    if (int rc = wmesh_device(c, mem, &m)) return rc;
    const size_t nv = (size_t)m.nv, nf = (size_t)m.nf;
    if (int rc = download(c, me, {{XO_IMESH_XYZ, m.xyz, sizeof(float) * 3 * nv, xyz}, {XO_IMESH_NORMALS, m.nrm, sizeof(float) * 3 * nv, normals}, {XO_IMESH_RGB, m.rgb, 3 * nv, rgb},
                                  {XO_IMESH_FACES, m.faces, sizeof(int) * 3 * nf, faces}})) return rc;
    *n_vertices = m.nv; *n_faces = m.nf; *first_vertex = m.first;
    return PSGSDF_OK;
}

namespace {
// ---- stage 2: the components of the welded mesh and the mesh without the ones the filter drops (the welded arrays themselves if all are kept); the
// component list is written to its pinned host slot.  nc == 0: an empty mesh, the stream has been waited for
struct MCompDev : MeshView { const int* vertex_component = nullptr; int nc = 0; psgsdf_mesh_component* list = nullptr; };
bool bad_filter(const psgsdf_mesh_filter& flt) { return flt.min_area != flt.min_area || flt.keep_largest < 0; }
int mcomp_device(psgsdf_ctx* c, DevMem& mem, const char* me, const psgsdf_mesh_filter& flt, MCompDev* d) {
    WMeshDev m;
    if (int rc = wmesh_device(c, mem, &m)) return rc;
    const int nv = m.nv, nf = m.nf;
    if (nv == 0 || nf == 0) return hipStreamSynchronize(c->stream) != hipSuccess ? fail(c, PSGSDF_ERR_DEVICE, "%s: kernels", me) : PSGSDF_OK;      // (every vertex belongs to a face: both or neither)
    // temporaries: 3 ints per vertex (parent, root flag / component number, component of the vertex), the edge table (6 slots of 12 B per face),
    // per component 8 x 8 B of counters and 6 x 4 B of box, the scan's sums; with a filter 1 int per vertex and face and the compacted arrays
    const size_t cap = std::max<size_t>(64, 6 * (size_t)nf);
    const long long nscan = std::max(nv, nf);
    int *parent = nullptr, *num = nullptr, *vcomp = nullptr, *uses = nullptr, *sums = nullptr; unsigned long long* keys = nullptr;
    auto oom = [&] { return fail(c, PSGSDF_ERR_DEVICE, "%s: out of memory (%d vertices, %d faces)", me, nv, nf); };
    if (!mem.get(&parent, (size_t)nv) || !mem.get(&num, (size_t)nv) || !mem.get(&vcomp, (size_t)nv) || !mem.get(&keys, cap) || !mem.get(&uses, cap)
        || !mem.get(&sums, (size_t)((nscan + psg::kTile - 1) / psg::kTile + 1))) return oom();
    if (hipMemsetAsync(keys, 0xff, sizeof(unsigned long long) * cap, c->stream) != hipSuccess || hipMemsetAsync(uses, 0, sizeof(int) * cap, c->stream) != hipSuccess)
        return fail(c, PSGSDF_ERR_DEVICE, "%s: memset", me);
    timed(c, "mcomp_init", [&] { psg::launch_mcomp_init(parent, nv, c->stream); });
    timed(c, "mcomp_hook", [&] { psg::launch_mcomp_hook(m.faces, nf, parent, c->stream); });
    timed(c, "mcomp_flatten", [&] { psg::launch_mcomp_flatten(parent, nv, num, c->stream); });
    timed(c, "mcomp_edges", [&] { psg::launch_mcomp_edges(m.faces, nf, keys, uses, cap, c->stream); });
    int nc = 0;
    if (int rc = scan_counts(c, num, nv, sums, &nc)) return rc;      // root flags -> component numbers in ascending first vertex
    long long* stat = nullptr; unsigned* box = nullptr;
    if (!mem.get(&stat, psg::kMcompStats * (size_t)nc) || !mem.get(&box, 6 * (size_t)nc)) return oom();
    unsigned *blo = box, *bhi = box + 3 * (size_t)nc;
    if (hipMemsetAsync(stat, 0, sizeof(long long) * psg::kMcompStats * (size_t)nc, c->stream) != hipSuccess || hipMemsetAsync(blo, 0xff, sizeof(unsigned) * 3 * (size_t)nc, c->stream) != hipSuccess
        || hipMemsetAsync(bhi, 0, sizeof(unsigned) * 3 * (size_t)nc, c->stream) != hipSuccess) return fail(c, PSGSDF_ERR_DEVICE, "%s: memset", me);
    const double vs = (double)c->grid.vs, unit = vs * vs / 16777216.0;      // one unit of the fixed-point area
    timed(c, "mcomp_vstats", [&] { psg::launch_mcomp_vstats(parent, num, nv, m.xyz, vcomp, stat, blo, bhi, c->stream); });
    timed(c, "mcomp_fstats", [&] { psg::launch_mcomp_fstats(m.faces, nf, vcomp, m.xyz, vs * vs, stat, c->stream); });
    timed(c, "mcomp_ecount", [&] { psg::launch_mcomp_ecount(keys, uses, cap, vcomp, stat, c->stream); });
    std::vector<long long> hstat((size_t)psg::kMcompStats * nc); std::vector<unsigned> hbox((size_t)6 * nc);
    if (hipMemcpyAsync(hstat.data(), stat, sizeof(long long) * hstat.size(), hipMemcpyDeviceToHost, c->stream) != hipSuccess
        || hipMemcpyAsync(hbox.data(), box, sizeof(unsigned) * hbox.size(), hipMemcpyDeviceToHost, c->stream) != hipSuccess || hipStreamSynchronize(c->stream) != hipSuccess)
        return fail(c, PSGSDF_ERR_DEVICE, "%s: download of the component table", me);
    void* hl = nullptr;
    if (int rc = host_out(c, XO_COMPONENTS, sizeof(psgsdf_mesh_component) * (size_t)nc, &hl)) return rc;
    psgsdf_mesh_component* list = (psgsdf_mesh_component*)hl;
    auto unordered = [](unsigned u) { u = (u & 0x80000000u) ? (u & 0x7fffffffu) : ~u; float f; memcpy(&f, &u, 4); return f; };
    for (int i = 0; i < nc; ++i) {
        const long long* s = hstat.data() + (size_t)psg::kMcompStats * i;
        psgsdf_mesh_component& k = list[i];
        k.first_vertex = s[psg::MC_FIRST]; k.n_vertices = s[psg::MC_VERTS]; k.n_faces = s[psg::MC_FACES]; k.n_edges = s[psg::MC_EDGES];
        k.n_boundary_edges = s[psg::MC_BOUNDARY]; k.n_nonmanifold_edges = s[psg::MC_NONMANIFOLD];
        k.area = unit * (double)s[psg::MC_AREA];
        for (int a = 0; a < 3; ++a) { k.lo[a] = unordered(hbox[(size_t)3 * i + a]); k.hi[a] = unordered(hbox[(size_t)3 * (nc + i) + a]); }
        k.kept = (k.n_faces >= flt.min_faces && k.area >= flt.min_area) ? 1 : 0; k.reserved = 0;
    }
    if (flt.keep_largest > 0) {      // of those that pass: the keep_largest with the most faces, ties to the smaller first vertex (= the smaller index)
        std::vector<int> pass;
        for (int i = 0; i < nc; ++i) if (list[i].kept) pass.push_back(i);
        std::stable_sort(pass.begin(), pass.end(), [&](int a, int b) { return list[a].n_faces > list[b].n_faces; });
        for (size_t q = (size_t)flt.keep_largest; q < pass.size(); ++q) list[pass[q]].kept = 0;
    }
    int n_kept = 0;
    for (int i = 0; i < nc; ++i) n_kept += list[i].kept;
    static_cast<MeshView&>(*d) = m; d->vertex_component = vcomp; d->nc = nc; d->list = list;
    if (n_kept == nc) return PSGSDF_OK;      // everything kept: the arrays as they are
    std::vector<int> hk((size_t)nc);
    for (int i = 0; i < nc; ++i) hk[(size_t)i] = list[i].kept;
    int *d_kept = nullptr, *vflag = nullptr, *fflag = nullptr, ov = 0, of = 0;
    if (!mem.get(&d_kept, (size_t)nc) || !mem.get(&vflag, (size_t)nv) || !mem.get(&fflag, (size_t)nf)) return oom();
    if (hipMemcpyAsync(d_kept, hk.data(), sizeof(int) * (size_t)nc, hipMemcpyHostToDevice, c->stream) != hipSuccess) return fail(c, PSGSDF_ERR_DEVICE, "%s: upload", me);
    timed(c, "mcomp_keep", [&] { psg::launch_mcomp_keep(d_kept, vcomp, nv, m.faces, nf, vflag, fflag, c->stream); });
    if (int rc = scan_counts(c, vflag, nv, sums, &ov)) return rc;      // (waits for the stream: hk stays alive until here)
    if (int rc = scan_counts(c, fflag, nf, sums, &of)) return rc;
    float *o_xyz = nullptr, *o_nrm = nullptr; unsigned char* o_rgb = nullptr; int *o_vcomp = nullptr, *o_faces = nullptr;
    if (ov > 0 && of > 0) {
        if (!mem.get(&o_xyz, 3 * (size_t)ov) || !mem.get(&o_nrm, 3 * (size_t)ov) || !mem.get(&o_rgb, 3 * (size_t)ov) || !mem.get(&o_vcomp, (size_t)ov) || !mem.get(&o_faces, 3 * (size_t)of)) return oom();
        timed(c, "mcomp_compact", [&] { psg::launch_mcomp_compact(d_kept, vcomp, nv, m.faces, nf, vflag, fflag, m.xyz, m.nrm, m.rgb, o_xyz, o_nrm, o_rgb, o_vcomp, o_faces, c->stream); });
    }
    d->xyz = o_xyz; d->nrm = o_nrm; d->rgb = o_rgb; d->faces = o_faces; d->vertex_component = o_vcomp; d->nv = ov; d->nf = of;
    return PSGSDF_OK;
}
}  // namespace

extern "C" int psgsdf_extract_mesh_components(psgsdf_ctx* c, const psgsdf_mesh_filter* filter, const float** xyz, const float** normals, const uint8_t** rgb, int64_t* n_vertices,
                                              const int32_t** faces, int64_t* n_faces, const int32_t** vertex_component, const psgsdf_mesh_component** components, int64_t* n_components) {
    const char* me = "extract_mesh_components";
    if (!xyz || !normals || !rgb || !n_vertices || !faces || !n_faces || !vertex_component || !components || !n_components) return fail(c, PSGSDF_ERR_ARG, "%s: null argument", me);
    // (before anything collective: no rank waits for another)
    if (c && c->n_ranks > 1) return fail(c, PSGSDF_ERR_UNSUPPORTED, "%s: not on a context attached to a rank (rank %d of %d): components are not merged across z-slabs yet", me, c->rank, c->n_ranks);
    psgsdf_mesh_filter flt{0, 0.0, 0};
    if (filter) flt = *filter;
    if (bad_filter(flt)) return fail(c, PSGSDF_ERR_ARG, "%s: min_area is NaN or keep_largest < 0", me);
    { int rc = extract_ready(c, me); if (rc) return rc; }
    *xyz = nullptr; *normals = nullptr; *rgb = nullptr; *faces = nullptr; *vertex_component = nullptr; *components = nullptr; *n_vertices = 0; *n_faces = 0; *n_components = 0;
    DevMem mem(c);
    MCompDev d;
    int rc = mcomp_device(c, mem, me, flt, &d);
    if (rc || d.nc == 0) return rc;      // (failed, or an empty mesh)
    const size_t nv = d.nv > 0 && d.nf > 0 ? (size_t)d.nv : 0, nf = nv ? (size_t)d.nf : 0;      // (a filter may drop everything)
    rc = download(c, me, {{XO_IMESH_XYZ, d.xyz, sizeof(float) * 3 * nv, xyz}, {XO_IMESH_NORMALS, d.nrm, sizeof(float) * 3 * nv, normals}, {XO_IMESH_RGB, d.rgb, 3 * nv, rgb},
                          {XO_IMESH_FACES, d.faces, sizeof(int) * 3 * nf, faces}, {XO_VERTEX_COMPONENT, d.vertex_component, sizeof(int) * nv, vertex_component}});
    if (rc) return rc;
    *n_vertices = (int64_t)nv; *n_faces = (int64_t)nf; *components = d.list; *n_components = d.nc;
    return PSGSDF_OK;
}

namespace {
// ---- stage 3: the input mesh `in` (nv > 0, nf > 0) clustered, and the result in its pinned host slots; dev (if asked for): the result's device arrays
struct LodOut {
    const float** xyz; const float** normals; const uint8_t** rgb; int64_t* n_vertices; const int32_t** faces; int64_t* n_faces; const int32_t** vertex_map;
    int64_t* n_vertices_in; int64_t* n_faces_in;
};
int lod_from_device(psgsdf_ctx* c, DevMem& mem, const MeshView& in, double cell, const LodOut& o, MeshView* dev = nullptr) {
    const char* me = "extract_mesh_lod";
    const int nv = in.nv, nf = in.nf;
    if (nv >= (1 << 30) || nf >= (1 << 30)) return fail(c, PSGSDF_ERR_UNSUPPORTED, "%s: %d vertices, %d faces", me, nv, nf);      // (slots are ints)
    // temporaries: the cluster table of 2 nv slots (8 B key, 10 x 8 B of sums, 4 B smallest member, 4 B used flag), the face table of 2 nf slots (4 B),
    // per vertex its slot, its flag / output number and its map entry, per face its slot and its flag / output number, the scan's sums
    psg::MlodTables t{};
    t.vcap = std::max<unsigned long long>(64, 2ull * (unsigned long long)nv); t.fcap = std::max<unsigned long long>(64, 2ull * (unsigned long long)nf);
    const size_t vcap = (size_t)t.vcap, fcap = (size_t)t.fcap;
    const long long nscan = std::max(nv, nf);
    int *vflag = nullptr, *fflag = nullptr, *sums = nullptr, *vmap = nullptr;
    auto give_up = [&](int code, const char* what) { return fail(c, code, "%s: %s (%d vertices, %d faces)", me, what, nv, nf); };
    if (!mem.get(&t.keys, vcap) || !mem.get(&t.acc, psg::kMlodAcc * vcap) || !mem.get(&t.first, vcap) || !mem.get(&t.used, vcap) || !mem.get(&t.vslot, (size_t)nv) || !mem.get(&t.ftab, fcap)
        || !mem.get(&t.fslot, (size_t)nf) || !mem.get(&t.bad, 1) || !mem.get(&vflag, (size_t)nv) || !mem.get(&fflag, (size_t)nf) || !mem.get(&vmap, (size_t)nv)
        || !mem.get(&sums, (size_t)((nscan + psg::kTile - 1) / psg::kTile + 1))) return give_up(PSGSDF_ERR_DEVICE, "out of memory");
    if (hipMemsetAsync(t.keys, 0xff, sizeof(unsigned long long) * vcap, c->stream) != hipSuccess || hipMemsetAsync(t.acc, 0, sizeof(long long) * psg::kMlodAcc * vcap, c->stream) != hipSuccess
        || hipMemsetAsync(t.first, 0x7f, sizeof(int) * vcap, c->stream) != hipSuccess || hipMemsetAsync(t.used, 0, sizeof(int) * vcap, c->stream) != hipSuccess
        || hipMemsetAsync(t.ftab, 0xff, sizeof(int) * fcap, c->stream) != hipSuccess || hipMemsetAsync(t.bad, 0, sizeof(int), c->stream) != hipSuccess) return give_up(PSGSDF_ERR_DEVICE, "memset");
    const double vs = (double)c->grid.vs;
    timed(c, "mlod_cluster", [&] { psg::launch_mlod_cluster(in.xyz, in.nrm, in.rgb, nv, cell, vs, t, c->stream); });
    int bad = 0;
    if (hipMemcpyAsync(&bad, t.bad, sizeof(int), hipMemcpyDeviceToHost, c->stream) != hipSuccess || hipStreamSynchronize(c->stream) != hipSuccess) return give_up(PSGSDF_ERR_DEVICE, "kernels");
    if (bad) return give_up(PSGSDF_ERR_UNSUPPORTED, "a cluster coordinate is beyond 2^20: the cell is too small for this mesh");
    timed(c, "mlod_ftable", [&] { psg::launch_mlod_ftable(in.faces, nf, t, c->stream); });
    timed(c, "mlod_fkeep", [&] { psg::launch_mlod_fkeep(in.faces, nf, t, fflag, c->stream); });
    timed(c, "mlod_vflag", [&] { psg::launch_mlod_vflag(nv, t, vflag, c->stream); });
    int ov = 0, of = 0;
    if (int rc = scan_counts(c, vflag, nv, sums, &ov)) return rc;      // smallest-member flags -> output vertex numbers
    if (int rc = scan_counts(c, fflag, nf, sums, &of)) return rc;      // kept-face flags -> output face numbers
    float *o_xyz = nullptr, *o_nrm = nullptr; unsigned char* o_rgb = nullptr; int* o_faces = nullptr;
    if (ov > 0 && (!mem.get(&o_xyz, 3 * (size_t)ov) || !mem.get(&o_nrm, 3 * (size_t)ov) || !mem.get(&o_rgb, 3 * (size_t)ov) || !mem.get(&o_faces, 3 * (size_t)of)))
        return give_up(PSGSDF_ERR_DEVICE, "out of memory");      // (a vertex exists only with a face: of > 0)
    timed(c, "mlod_emit", [&] { psg::launch_mlod_emit(in.xyz, in.nrm, in.rgb, nv, in.faces, nf, vs, t, vflag, fflag, o_xyz, o_nrm, o_rgb, o_faces, vmap, c->stream); });
    const size_t v = (size_t)ov, f = ov > 0 ? (size_t)of : 0;
    if (int rc = download(c, me, {{XO_LOD_VERTEX_MAP, vmap, sizeof(int) * (size_t)nv, o.vertex_map}, {XO_IMESH_XYZ, o_xyz, sizeof(float) * 3 * v, o.xyz}, {XO_IMESH_NORMALS, o_nrm, sizeof(float) * 3 * v, o.normals},
                                  {XO_IMESH_RGB, o_rgb, 3 * v, o.rgb}, {XO_IMESH_FACES, o_faces, sizeof(int) * 3 * f, o.faces}})) return rc;
    *o.n_vertices_in = nv; *o.n_faces_in = nf; *o.n_vertices = (int64_t)v; *o.n_faces = (int64_t)f;
    if (dev) { dev->xyz = o_xyz; dev->nrm = o_nrm; dev->rgb = o_rgb; dev->faces = o_faces; dev->nv = (int)v; dev->nf = (int)f; }
    return PSGSDF_OK;
}
// what psgsdf_extract_mesh_lod and psgsdf_bake_lod check first (before anything collective and before any device work: no rank waits for another) ...
int lod_ready(psgsdf_ctx* c, const char* me, const psgsdf_mesh_filter* filter, double cell) {
    if (c && c->n_ranks > 1) return fail(c, PSGSDF_ERR_UNSUPPORTED, "%s: not on a context attached to a rank (rank %d of %d): clusters are not merged across z-slabs", me, c->rank, c->n_ranks);
    if (!(cell > 0.0) || std::isinf(cell)) return fail(c, PSGSDF_ERR_ARG, "%s: the cell must be a finite size > 0", me);
    if (filter && bad_filter(*filter)) return fail(c, PSGSDF_ERR_ARG, "%s: min_area is NaN or keep_largest < 0", me);
    return PSGSDF_OK;
}
// ... and the stages both run: the welded mesh, its components if there is a filter, the clusters
int lod_stages(psgsdf_ctx* c, DevMem& mem, const char* me, const psgsdf_mesh_filter* filter, double cell, const LodOut& o, MeshView* dev = nullptr) {
    MeshView in;
    if (!filter) {      // the welded mesh as it is: no component pass
        WMeshDev m;
        if (int rc = wmesh_device(c, mem, &m)) return rc;
        in = m;
    } else {
        MCompDev d;
        int rc = mcomp_device(c, mem, me, *filter, &d);
        if (rc || d.nc == 0) return rc;      // (failed, or an empty mesh)
        in = d;
    }
    if (in.nv > 0 && in.nf > 0) return lod_from_device(c, mem, in, cell, o, dev);
    return hipStreamSynchronize(c->stream) != hipSuccess ? fail(c, PSGSDF_ERR_DEVICE, "%s: kernels", me) : PSGSDF_OK;
}
}  // namespace

extern "C" int psgsdf_extract_mesh_lod(psgsdf_ctx* c, const psgsdf_mesh_filter* filter, double cell, const float** xyz, const float** normals, const uint8_t** rgb, int64_t* n_vertices,
                                       const int32_t** faces, int64_t* n_faces, const int32_t** vertex_map, int64_t* n_vertices_in, int64_t* n_faces_in) {
    const char* me = "extract_mesh_lod";
    if (!xyz || !normals || !rgb || !n_vertices || !faces || !n_faces || !vertex_map || !n_vertices_in || !n_faces_in) return fail(c, PSGSDF_ERR_ARG, "%s: null argument", me);
    if (int rc = lod_ready(c, me, filter, cell)) return rc;
    { int rc = extract_ready(c, me); if (rc) return rc; }
    *xyz = nullptr; *normals = nullptr; *rgb = nullptr; *faces = nullptr; *vertex_map = nullptr; *n_vertices = 0; *n_faces = 0; *n_vertices_in = 0; *n_faces_in = 0;
    DevMem mem(c);
    return lod_stages(c, mem, me, filter, cell, LodOut{xyz, normals, rgb, n_vertices, faces, n_faces, vertex_map, n_vertices_in, n_faces_in});
}

namespace {
// ---- the photometric fit of this context's band rows [row0, row1) (fit.hip k_band_fit); n == 0: nothing was launched
struct BFitDev { const int* n_obs = nullptr; const double* loss = nullptr; const float* r2 = nullptr; int n = 0; };
int bfit_device(psgsdf_ctx* c, DevMem& mem, const char* me, BFitDev* d) {
    const int n = c->row1 - c->row0;
    if (n <= 0) return PSGSDF_OK;
    int* n_obs = nullptr; double* loss = nullptr; float* r2 = nullptr;      // temporaries: 24 B per band row
    if (!mem.get(&n_obs, (size_t)n) || !mem.get(&loss, (size_t)n) || !mem.get(&r2, 3 * (size_t)n)) return fail(c, PSGSDF_ERR_DEVICE, "%s: out of memory (%d band rows)", me, n);
    const SweepArgs a = make_args(c, 0);      // (fold.n = 0: the kernel takes no pending fold; it writes no partial slot either)
    timed(c, "band_fit", [&] { psg::launch_band_fit(a, n_obs, loss, r2, c->stream); });
    d->n_obs = n_obs; d->loss = loss; d->r2 = r2; d->n = n;
    return PSGSDF_OK;
}
// what both calls check first: no rank waits for another, nothing has touched the device
int fit_ready(psgsdf_ctx* c, const char* me) {
    if (c && c->n_ranks > 1) return fail(c, PSGSDF_ERR_UNSUPPORTED, "%s: not on a context attached to a rank (rank %d of %d): the fit is not gathered across z-slabs", me, c->rank, c->n_ranks);
    if (!c || !c->inited) return fail(c, PSGSDF_ERR_STATE, "%s: psgsdf_init first (no band)", me);
    return extract_ready(c, me);      // the quiescent point of the extraction calls: pending read-backs delivered
}
}  // namespace

extern "C" int psgsdf_band_fit(psgsdf_ctx* c, const int32_t** n_obs, const double** loss, const float** sum_r2, int64_t* n_band) {
    const char* me = "band_fit";
    if (!n_obs || !loss || !sum_r2 || !n_band) return fail(c, PSGSDF_ERR_ARG, "%s: null argument", me);
    { int rc = fit_ready(c, me); if (rc) return rc; }
    *n_obs = nullptr; *loss = nullptr; *sum_r2 = nullptr; *n_band = 0;
    DevMem mem(c);
    BFitDev d;
    if (int rc = bfit_device(c, mem, me, &d)) return rc;
    const size_t n = (size_t)d.n;
    if (int rc = download(c, me, {{XO_FIT_NOBS, d.n_obs, sizeof(int) * n, n_obs}, {XO_FIT_LOSS, d.loss, sizeof(double) * n, loss}, {XO_FIT_R2, d.r2, sizeof(float) * 3 * n, sum_r2}})) return rc;
    *n_band = d.n;
    return PSGSDF_OK;
}

extern "C" int psgsdf_extract_mesh_fit(psgsdf_ctx* c, const float** xyz, const float** normals, const uint8_t** rgb, int64_t* n_vertices, const int32_t** faces, int64_t* n_faces,
                                       const int32_t** vertex_n_obs, const float** vertex_rms, const float** vertex_loss) {
    const char* me = "extract_mesh_fit";
    if (!xyz || !normals || !rgb || !n_vertices || !faces || !n_faces || !vertex_n_obs || !vertex_rms || !vertex_loss) return fail(c, PSGSDF_ERR_ARG, "%s: null argument", me);
    { int rc = fit_ready(c, me); if (rc) return rc; }
    *xyz = nullptr; *normals = nullptr; *rgb = nullptr; *faces = nullptr; *vertex_n_obs = nullptr; *vertex_rms = nullptr; *vertex_loss = nullptr; *n_vertices = 0; *n_faces = 0;
    DevMem mem(c);
    BFitDev d;
    if (int rc = bfit_device(c, mem, me, &d)) return rc;
    WMeshDev m;
    if (int rc = wmesh_device(c, mem, &m)) return rc;
    const size_t nv = (size_t)m.nv, nf = (size_t)m.nf;
    int* v_n = nullptr; float *v_rms = nullptr, *v_loss = nullptr;      // temporaries: 12 B per vertex
    if (nv > 0) {
        if (!mem.get(&v_n, nv) || !mem.get(&v_rms, nv) || !mem.get(&v_loss, nv)) return fail(c, PSGSDF_ERR_DEVICE, "%s: out of memory (%d vertices)", me, m.nv);
        timed(c, "wmesh_fit", [&] { psg::launch_wmesh_fit(m.grid, m.num, m.nv, c->dense.row_of, c->row0, c->row1, d.n_obs, d.loss, d.r2, v_n, v_rms, v_loss, c->stream); });
    }
    if (int rc = download(c, me, {{XO_IMESH_XYZ, m.xyz, sizeof(float) * 3 * nv, xyz}, {XO_IMESH_NORMALS, m.nrm, sizeof(float) * 3 * nv, normals}, {XO_IMESH_RGB, m.rgb, 3 * nv, rgb},
                                  {XO_IMESH_FACES, m.faces, sizeof(int) * 3 * nf, faces}, {XO_VFIT_NOBS, v_n, sizeof(int) * nv, vertex_n_obs}, {XO_VFIT_RMS, v_rms, sizeof(float) * nv, vertex_rms},
                                  {XO_VFIT_LOSS, v_loss, sizeof(float) * nv, vertex_loss}})) return rc;
    *n_vertices = m.nv; *n_faces = m.nf;
    return PSGSDF_OK;
}

// ---- detail maps of the level-of-detail mesh (include/psgsdf_bake.h; kernel: bake.hip k_bake).  The clusters' device arrays are the kernel's mesh
// (lod_from_device hands them out: nothing is uploaded again), the brick map comes from the renderer's prepare path.
namespace {
// what psgsdf_bake_lod and psgsdf_bake_lod_ao check first
int bake_ready(psgsdf_ctx* c, const char* me, const psgsdf_mesh_filter* filter, double cell, int32_t res, double reach) {
    if (int rc = lod_ready(c, me, filter, cell)) return rc;
    if (res < 1) return fail(c, PSGSDF_ERR_ARG, "%s: res %d (at least 1)", me, res);
    if (!(reach > 0.0) || std::isinf(reach)) return fail(c, PSGSDF_ERR_ARG, "%s: the reach must be a finite length > 0", me);
    return PSGSDF_OK;
}
// the bake of both calls, its results in their pinned host slots (the stream has been waited for); dev (if asked for): the kernel's arguments, the
// atlas's device planes among them (dev->nf == 0: an empty level-of-detail mesh, nothing was baked)
int bake_device(psgsdf_ctx* c, DevMem& mem, const char* me, const psgsdf_mesh_filter* filter, double cell, int32_t res, double reach, psgsdf_bake* out, psg::BakeArgs* dev = nullptr) {
    *out = psgsdf_bake{};
    MeshView lod;
    if (int rc = lod_stages(c, mem, me, filter, cell, LodOut{&out->xyz, &out->normals, &out->rgb, &out->n_vertices, &out->faces, &out->n_faces, &out->vertex_map,
                                                            &out->n_vertices_in, &out->n_faces_in}, &lod)) { *out = psgsdf_bake{}; return rc; }
    if (lod.nf <= 0) return PSGSDF_OK;      // an empty level-of-detail mesh: all sizes 0
    auto give_up = [&](int code, const char* what) { *out = psgsdf_bake{}; return fail(c, code, "%s: %s (%d faces, res %d)", me, what, lod.nf, res); };
    // the atlas: two faces per block of (R + 1)^2 texels, the blocks in a near-square grid
    psg::BakeArgs a{};
    const long long B = (long long)res + 1, nblk = ((long long)lod.nf + 1) / 2;
    long long bpr = (long long)sqrt((double)nblk);
    while (bpr * bpr < nblk) ++bpr;
    while (bpr > 1 && (bpr - 1) * (bpr - 1) >= nblk) --bpr;
    const long long W = bpr * B, H = (nblk + bpr - 1) / bpr * B;
    if (W > psg::kBakeMaxSide || H > psg::kBakeMaxSide) return give_up(PSGSDF_ERR_UNSUPPORTED, "the atlas would be larger than 16384 texels along a side");
    { RenderArgs ra; int rc = render_prepare(c, mem, ra, me); if (rc) { *out = psgsdf_bake{}; return rc; } a.r = ra; }
    a.has_band = c->inited ? 1 : 0;
    a.xyz = lod.xyz; a.nrm = lod.nrm; a.rgb = lod.rgb; a.faces = lod.faces; a.nf = lod.nf;
    a.res = res; a.bpr = (int)bpr; a.nblk = (int)nblk; a.W = (int)W; a.H = (int)H;
    a.reach = reach; a.vs = (double)c->grid.vs;
    const size_t px = (size_t)W * (size_t)H;
    if (!mem.get(&a.albedo, 3 * px) || !mem.get(&a.normal, 3 * px) || !mem.get(&a.disp, px) || !mem.get(&a.voxel, px) || !mem.get(&a.face, px) || !mem.get(&a.counts, (size_t)psg::kBakeCounts))
        return give_up(PSGSDF_ERR_DEVICE, "out of memory");
    if (hipMemsetAsync(a.counts, 0, sizeof(unsigned long long) * psg::kBakeCounts, c->stream) != hipSuccess) return give_up(PSGSDF_ERR_DEVICE, "memset");
    timed(c, "bake", [&] { psg::launch_bake(a, c->stream); });
    // the texture coordinates: integers over 6 W / 6 H, one division each
    void* hu = nullptr;
    if (int rc = host_out(c, XO_BAKE_UV, sizeof(float) * 6 * (size_t)lod.nf, &hu)) { *out = psgsdf_bake{}; return rc; }
    float* uv = (float*)hu;
    const long long R6 = 6 * (long long)res;
    for (long long f = 0; f < lod.nf; ++f) {
        const long long q = f >> 1, x0 = 6 * (q % bpr) * B, y0 = 6 * (q / bpr) * B;
        const long long even[3][2] = {{1, 1}, {R6 + 7, 1}, {1, R6 + 7}}, odd[3][2] = {{R6 + 5, R6 + 5}, {-1, R6 + 5}, {R6 + 5, -1}};
        for (int k = 0; k < 3; ++k) {
            const long long* m = (f & 1) ? odd[k] : even[k];
            uv[6 * f + 2 * k] = (float)((double)(x0 + m[0]) / (double)(6 * W));
            uv[6 * f + 2 * k + 1] = (float)((double)(y0 + m[1]) / (double)(6 * H));
        }
    }
    unsigned long long cnt[psg::kBakeCounts] = {};
    if (hipMemcpyAsync(cnt, a.counts, sizeof(cnt), hipMemcpyDeviceToHost, c->stream) != hipSuccess) return give_up(PSGSDF_ERR_DEVICE, "download of the counts");
    if (int rc = download(c, me, {{XO_BAKE_ALBEDO, a.albedo, 3 * px, &out->albedo}, {XO_BAKE_NORMAL, a.normal, sizeof(float) * 3 * px, &out->normal},
                                  {XO_BAKE_DISPLACEMENT, a.disp, sizeof(float) * px, &out->displacement}, {XO_BAKE_VOXEL, a.voxel, sizeof(int) * px, &out->voxel},
                                  {XO_BAKE_FACE, a.face, sizeof(int) * px, &out->face}})) { *out = psgsdf_bake{}; return rc; }
    out->uv = uv; out->width = (int32_t)W; out->height = (int32_t)H;
    out->n_texels = (int64_t)cnt[psg::BK_OWNED]; out->n_hits = (int64_t)cnt[psg::BK_HITS]; out->n_hits_off_band = (int64_t)cnt[psg::BK_OFF_BAND]; out->n_buried = (int64_t)cnt[psg::BK_BURIED];
    out->n_misses = out->n_texels - out->n_hits - out->n_buried;
    if (dev) *dev = a;
    return PSGSDF_OK;
}
}  // namespace

extern "C" int psgsdf_bake_lod(psgsdf_ctx* c, const psgsdf_mesh_filter* filter, double cell, int32_t res, double reach, psgsdf_bake* out) {
    const char* me = "bake_lod";
    if (!out) return fail(c, PSGSDF_ERR_ARG, "%s: null argument", me);
    if (int rc = bake_ready(c, me, filter, cell, res, reach)) return rc;
    { int rc = extract_ready(c, me); if (rc) return rc; }
    DevMem mem(c);
    return bake_device(c, mem, me, filter, cell, res, reach, out);
}

// ---- ambient occlusion (include/psgsdf_occlusion.h; kernel: occlusion.hip k_occlusion): K short rays per sample through the renderer's walk, the
// samples either the caller's points or the texels of a bake, whose planes are still on the device when the rays start from them.
namespace {
int ao_bad_params(psgsdf_ctx* c, const char* me, const psgsdf_ao_params* p) {
    if (!p) return fail(c, PSGSDF_ERR_ARG, "%s: null argument", me);
    if ((p->n_dirs != 8 && p->n_dirs != 16 && p->n_dirs != 32 && p->n_dirs != 64) || p->reserved != 0)
        return fail(c, PSGSDF_ERR_ARG, "%s: n_dirs %d, reserved %d (8, 16, 32 or 64 directions; reserved 0)", me, p->n_dirs, p->reserved);
    if (!(p->radius > 0.0) || std::isinf(p->radius) || !(p->bias > 0.0) || std::isinf(p->bias)) return fail(c, PSGSDF_ERR_ARG, "%s: radius and bias must be finite lengths > 0", me);
    return PSGSDF_OK;
}
// the direction table into its pinned slot (the definition's arithmetic, in double)
int ao_dirs(psgsdf_ctx* c, int K, const double** dirs) {
    void* h = nullptr;
    if (int rc = host_out(c, XO_AO_DIRS, sizeof(double) * 3 * (size_t)K, &h)) return rc;
    double* D = (double*)h;
    const double g = 0.6180339887498949, pi = 3.141592653589793;
    for (int i = 0; i < K; ++i) {
        const double u = ((double)i + 0.5) / (double)K, r = sqrt(u), z = sqrt(1.0 - u), phi = 2.0 * pi * ((double)i * g - floor((double)i * g));
        D[3 * i] = r * cos(phi); D[3 * i + 1] = r * sin(phi); D[3 * i + 2] = z;
    }
    *dirs = D;
    return PSGSDF_OK;
}
// the arguments both providers share (a.n and the provider's own arrays are set by the caller before): brick map, table, results, counts; launch; download
int ao_run(psgsdf_ctx* c, DevMem& mem, const char* me, const psgsdf_ao_params& p, const double* dirs_host, psg::OcclusionArgs& a, bool bake, XoSlot s_mask, XoSlot s_occ,
           const uint64_t** mask, const uint8_t** occlusion, psgsdf_ao_counts* counts) {
    const int K = p.n_dirs;
    a.K = K; a.log2K = K == 8 ? 3 : K == 16 ? 4 : K == 32 ? 5 : 6;
    a.radius = p.radius; a.bias = p.bias; a.vs = (double)c->grid.vs;
    a.t_max = (float)p.radius;      // rounded up if the conversion rounded down: no hit within the radius is cut off
    if ((double)a.t_max < p.radius) a.t_max = nextafterf(a.t_max, INFINITY);
    if (!c->ao_cut) a.t_max = FLT_MAX;      // (PSGSDF_AO_CUT=0; tools/time_mesh.py: what the cut buys -- the same bits)
    double* d_dirs = nullptr;
    const size_t n = (size_t)a.n;
    if (!mem.get(&d_dirs, 3 * (size_t)K) || !mem.get(&a.mask, n) || !mem.get(&a.occ, n) || !mem.get(&a.counts, (size_t)psg::kAoCounts))
        return fail(c, PSGSDF_ERR_DEVICE, "%s: out of memory (%lld samples)", me, a.n);
    a.dirs = d_dirs;
    if (hipMemcpyAsync(d_dirs, dirs_host, sizeof(double) * 3 * (size_t)K, hipMemcpyHostToDevice, c->stream) != hipSuccess
        || hipMemsetAsync(a.counts, 0, sizeof(unsigned long long) * psg::kAoCounts, c->stream) != hipSuccess) return fail(c, PSGSDF_ERR_DEVICE, "%s: upload", me);
    hipError_t launched = hipSuccess;
    timed(c, "occlusion", [&] { launched = psg::launch_occlusion(a, bake, c->stream); });
    if (launched != hipSuccess) return fail(c, PSGSDF_ERR_DEVICE, "%s: launch of %lld rays: %s", me, a.n * K, hipGetErrorString(launched));
    unsigned long long cnt[psg::kAoCounts] = {};
    if (hipMemcpyAsync(cnt, a.counts, sizeof(cnt), hipMemcpyDeviceToHost, c->stream) != hipSuccess) return fail(c, PSGSDF_ERR_DEVICE, "%s: download of the counts", me);
    if (int rc = download(c, me, {{s_mask, a.mask, sizeof(uint64_t) * n, mask}, {s_occ, a.occ, n, occlusion}})) return rc;
    counts->n_samples = (int64_t)cnt[psg::AO_SAMPLES]; counts->n_valid = (int64_t)cnt[psg::AO_VALID]; counts->n_rays = (int64_t)K * counts->n_valid;
    counts->n_occluded = (int64_t)cnt[psg::AO_OCCLUDED]; counts->n_buried = (int64_t)cnt[psg::AO_BURIED];
    return PSGSDF_OK;
}
}  // namespace

extern "C" int psgsdf_occlusion_points(psgsdf_ctx* c, const float* xyz, const float* normals, int64_t n, const psgsdf_ao_params* params,
                                       const uint64_t** mask, const uint8_t** occlusion, const double** dirs, psgsdf_ao_counts* counts) {
    const char* me = "occlusion_points";
    if (!mask || !occlusion || !dirs || !counts || (n > 0 && (!xyz || !normals))) return fail(c, PSGSDF_ERR_ARG, "%s: null argument", me);
    // (before anything collective and before any device work: no rank waits for another)
    if (c && c->n_ranks > 1) return fail(c, PSGSDF_ERR_UNSUPPORTED, "%s: not on a context attached to a rank (rank %d of %d): a slab holds only its own planes of the volume", me, c->rank, c->n_ranks);
    if (int rc = ao_bad_params(c, me, params)) return rc;
    if (n < 0) return fail(c, PSGSDF_ERR_ARG, "%s: %lld points", me, (long long)n);
    { int rc = extract_ready(c, me); if (rc) return rc; }
    *mask = nullptr; *occlusion = nullptr; *dirs = nullptr; *counts = psgsdf_ao_counts{};
    const double* D = nullptr;
    if (int rc = ao_dirs(c, params->n_dirs, &D)) return rc;
    if (n > 0) {
        DevMem mem(c);
        psg::OcclusionArgs a{};
        { RenderArgs ra; int rc = render_prepare(c, mem, ra, me); if (rc) return rc; a.r = ra; }
        a.n = (long long)n;
        float *d_xyz = nullptr, *d_nrm = nullptr;
        if (!mem.get(&d_xyz, 3 * (size_t)n) || !mem.get(&d_nrm, 3 * (size_t)n)) return fail(c, PSGSDF_ERR_DEVICE, "%s: out of memory (%lld points)", me, (long long)n);
        if (hipMemcpyAsync(d_xyz, xyz, sizeof(float) * 3 * (size_t)n, hipMemcpyHostToDevice, c->stream) != hipSuccess
            || hipMemcpyAsync(d_nrm, normals, sizeof(float) * 3 * (size_t)n, hipMemcpyHostToDevice, c->stream) != hipSuccess) return fail(c, PSGSDF_ERR_DEVICE, "%s: upload", me);
        a.pts = d_xyz; a.pts_n = d_nrm;
        psgsdf_ao_counts cn{};
        if (int rc = ao_run(c, mem, me, *params, D, a, false, XO_AO_MASK, XO_AO_OCCLUSION, mask, occlusion, &cn)) { *mask = nullptr; *occlusion = nullptr; return rc; }
        *counts = cn;
    }
    *dirs = D;
    return PSGSDF_OK;
}

extern "C" int psgsdf_bake_lod_ao(psgsdf_ctx* c, const psgsdf_mesh_filter* filter, double cell, int32_t res, double reach, const psgsdf_ao_params* params, psgsdf_bake_ao* out) {
    const char* me = "bake_lod_ao";
    if (!out) return fail(c, PSGSDF_ERR_ARG, "%s: null argument", me);
    if (int rc = bake_ready(c, me, filter, cell, res, reach)) return rc;
    if (int rc = ao_bad_params(c, me, params)) return rc;
    { int rc = extract_ready(c, me); if (rc) return rc; }
    *out = psgsdf_bake_ao{};
    DevMem mem(c);
    psg::BakeArgs b{};
    if (int rc = bake_device(c, mem, me, filter, cell, res, reach, &out->bake, &b)) return rc;
    const double* D = nullptr;
    if (int rc = ao_dirs(c, params->n_dirs, &D)) { *out = psgsdf_bake_ao{}; return rc; }
    out->n_dirs = params->n_dirs;
    if (b.nf > 0) {
        psg::OcclusionArgs a{};
        a.r = b.r; a.n = (long long)b.W * b.H;
        a.xyz = b.xyz; a.nrm = b.nrm; a.faces = b.faces; a.res = b.res; a.W = b.W;
        a.normal = b.normal; a.disp = b.disp; a.voxel = b.voxel; a.face = b.face;
        if (int rc = ao_run(c, mem, me, *params, D, a, true, XO_BAKE_AO_MASK, XO_BAKE_AO_OCCLUSION, &out->mask, &out->occlusion, &out->counts)) { *out = psgsdf_bake_ao{}; return rc; }
    }
    out->dirs = D;
    return PSGSDF_OK;
}

// ---- comparison with a reference mesh or cloud (include/psgsdf_compare.h; kernels: compare.hip): the welded mesh (or its kept components) stays on
// the device, the reference is uploaded once, and each direction is a grid build over its targets, the search, and the integer reductions.
namespace {
struct CmpBox { double lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY}; bool any = false; };
// the bounding box of the finite points
CmpBox cmp_bbox(const float* xyz, size_t n) {
    CmpBox b;
    for (size_t i = 0; i < n; ++i) {
        const float* p = xyz + 3 * i;
        if (!std::isfinite(p[0]) || !std::isfinite(p[1]) || !std::isfinite(p[2])) continue;
        for (int k = 0; k < 3; ++k) { b.lo[k] = std::min(b.lo[k], (double)p[k]); b.hi[k] = std::max(b.hi[k], (double)p[k]); }
        b.any = true;
    }
    return b;
}
struct CmpOut { XoSlot s_dist, s_nearest, s_side; const float** dist; const int32_t** nearest; const int8_t** side; };
// the uniform grid over a.t_* (a.nt targets) and the box [lo, hi] into a.g (none if !box.any or without a target); waits for the stream once (the
// grid's size).  Shared by psgsdf_compare_reference and psgsdf_align_reference.
int compare_grid(psgsdf_ctx* c, DevMem& mem, const char* me, psg::CompareArgs& a, const CmpBox& box, double cell) {
    psg::CompareGrid& g = a.g;
    g = psg::CompareGrid{};
    if (!(a.nt > 0 && box.any)) return PSGSDF_OK;
    if (!mem.get(&a.total, 1)) return fail(c, PSGSDF_ERR_DEVICE, "%s: out of memory", me);
    if (hipMemsetAsync(a.total, 0, sizeof(unsigned long long), c->stream) != hipSuccess) return fail(c, PSGSDF_ERR_DEVICE, "%s: memset", me);
    // the cells: edge `cell`, doubled until the grid fits kCompareMaxCells (acceleration only: no result depends on it)
    // and the lower corner snapped down to a whole number of cells, so that the walls are the multiples of the edge
    double h = cell, nd[3], lo[3];
    for (;;) {
        double cells = 1.0;
        for (int k = 0; k < 3; ++k) { lo[k] = floor(box.lo[k] / h) * h; nd[k] = std::max(1.0, ceil((box.hi[k] - lo[k]) / h)); cells *= nd[k]; }
        if (cells <= (double)psg::kCompareMaxCells) break;
        h *= 2.0;
    }
    g.h = h; g.cells = 1;
    for (int k = 0; k < 3; ++k) { g.lo[k] = lo[k]; g.n[k] = (int)nd[k]; g.cells *= g.n[k]; }
    int* sums = nullptr;
    if (!mem.get(&g.start, (size_t)g.cells + 1) || !mem.get(&g.cursor, (size_t)g.cells) || !mem.get(&sums, (size_t)((g.cells + 1 + psg::kTile - 1) / psg::kTile + 1)))
        return fail(c, PSGSDF_ERR_DEVICE, "%s: out of memory (%lld grid cells)", me, g.cells);
    if (hipMemsetAsync(g.start, 0, sizeof(int) * ((size_t)g.cells + 1), c->stream) != hipSuccess || hipMemsetAsync(g.cursor, 0, sizeof(int) * (size_t)g.cells, c->stream) != hipSuccess)
        return fail(c, PSGSDF_ERR_DEVICE, "%s: memset", me);
    hipError_t e = hipSuccess;
    unsigned long long total = 0;
    timed(c, "compare_total", [&] { e = psg::launch_compare_total(a, c->stream); });
    if (e != hipSuccess || hipMemcpyAsync(&total, a.total, sizeof(total), hipMemcpyDeviceToHost, c->stream) != hipSuccess || hipStreamSynchronize(c->stream) != hipSuccess)
        return fail(c, PSGSDF_ERR_DEVICE, "%s: the grid's size", me);
    if (total > (unsigned long long)INT32_MAX)
        return fail(c, PSGSDF_ERR_UNSUPPORTED, "%s: the search grid would need %llu entries for %d targets (cells of %g): tessellate it", me, total, a.nt, h);
    timed(c, "compare_count", [&] { e = psg::launch_compare_count(a, c->stream); });
    if (e != hipSuccess) return fail(c, PSGSDF_ERR_DEVICE, "%s: launch: %s", me, hipGetErrorString(e));
    int tot = 0;
    if (int rc = scan_counts(c, g.start, g.cells + 1, sums, &tot)) return rc;      // counts -> the cells' first entries; start[cells] = the total
    if ((unsigned long long)tot != total) return fail(c, PSGSDF_ERR_DEVICE, "%s: the grid's counts (%d) and its total (%llu) differ", me, tot, total);
    if (!mem.get(&g.entries, (size_t)tot)) return fail(c, PSGSDF_ERR_DEVICE, "%s: out of memory (%d grid entries)", me, tot);
    timed(c, "compare_fill", [&] { e = psg::launch_compare_fill(a, c->stream); });
    if (e != hipSuccess) return fail(c, PSGSDF_ERR_DEVICE, "%s: launch: %s", me, hipGetErrorString(e));
    return PSGSDF_OK;
}
// the per-query arrays the search writes
bool compare_query_arrays(DevMem& mem, psg::CompareArgs& a) {
    const size_t nq = (size_t)a.nq;
    return mem.get(&a.d, nq) && mem.get(&a.dist, nq) && mem.get(&a.nearest, nq) && mem.get(&a.side, nq) && mem.get(&a.pairs, nq);
}
// one direction: a.t_*, a.nt, a.q_xyz, a.nq and the parameters are set; the grid over the box [lo, hi] (none if !box), the search, the
// statistics; the per-query arrays in their pinned slots (the stream has been waited for)
int compare_direction(psgsdf_ctx* c, DevMem& mem, const char* me, psg::CompareArgs a, const CmpBox& box, double cell, int dir, const CmpOut& o, psgsdf_compare_side* S) {
    *S = psgsdf_compare_side{};
    S->n = a.nq;
    c->cmp_queries[dir] = a.nq; c->cmp_pairs[dir] = 0;
    if (a.nq == 0) return PSGSDF_OK;
    const size_t nq = (size_t)a.nq;
    if (!compare_query_arrays(mem, a) || !mem.get(&a.stats, (size_t)psg::kCmpStats)) return fail(c, PSGSDF_ERR_DEVICE, "%s: out of memory (%lld queries)", me, a.nq);
    if (hipMemsetAsync(a.stats, 0, sizeof(unsigned long long) * psg::kCmpStats, c->stream) != hipSuccess) return fail(c, PSGSDF_ERR_DEVICE, "%s: memset", me);
    if (int rc = compare_grid(c, mem, me, a, box, cell)) return rc;
    hipError_t e = hipSuccess;
    timed(c, dir ? "compare_query_rec" : "compare_query_ref", [&] { e = psg::launch_compare_query(a, c->compare_chunk, c->stream); });
    if (e != hipSuccess) return fail(c, PSGSDF_ERR_DEVICE, "%s: launch of %lld queries: %s", me, a.nq, hipGetErrorString(e));
    timed(c, "compare_stats", [&] { e = psg::launch_compare_stats(a, c->stream); });
    if (e != hipSuccess) return fail(c, PSGSDF_ERR_DEVICE, "%s: launch: %s", me, hipGetErrorString(e));
    unsigned long long st[psg::kCmpStats] = {};
    if (hipMemcpyAsync(st, a.stats, sizeof(st), hipMemcpyDeviceToHost, c->stream) != hipSuccess) return fail(c, PSGSDF_ERR_DEVICE, "%s: download of the statistics", me);
    if (int rc = download(c, me, {{o.s_dist, a.dist, sizeof(float) * nq, o.dist}, {o.s_nearest, a.nearest, sizeof(int) * nq, o.nearest}, {o.s_side, a.side, nq, o.side}})) return rc;
    S->n_valid = (int64_t)st[psg::CS_VALID]; S->n_matched = (int64_t)st[psg::CS_MATCHED]; S->n_within_tau = (int64_t)st[psg::CS_TAU];
    S->sum_d = (int64_t)st[psg::CS_SUM_D]; S->sum_d2 = (int64_t)st[psg::CS_SUM_D2]; S->sum_signed = (int64_t)st[psg::CS_SIGNED];
    for (int b = 0; b < 16; ++b) S->hist[b] = (int64_t)st[psg::CS_HIST + b];
    memcpy(&S->max, &st[psg::CS_MAX], sizeof(double));
    if (S->n_matched > 0) {
        const double m = (double)S->n_matched, unit = 1048576.0;
        S->mean = a.vs * ((double)S->sum_d / unit) / m;
        S->rms = a.vs * sqrt(((double)S->sum_d2 / unit) / m);
        S->mean_signed = a.vs * ((double)S->sum_signed / unit) / m;
    }
    c->cmp_pairs[dir] = (long long)st[psg::CS_PAIRS];
    return PSGSDF_OK;
}
}  // namespace

extern "C" int psgsdf_compare_reference(psgsdf_ctx* c, const psgsdf_mesh_filter* filter, const float* ref_xyz, int64_t n_ref, const int32_t* ref_faces, int64_t n_ref_faces,
                                        const psgsdf_compare_params* params, psgsdf_compare* out) {
    const char* me = "compare_reference";
    if (!params || !out || (n_ref > 0 && !ref_xyz)) return fail(c, PSGSDF_ERR_ARG, "%s: null argument", me);
    // (before anything collective and before any device work: no rank waits for another)
    if (c && c->n_ranks > 1) return fail(c, PSGSDF_ERR_UNSUPPORTED, "%s: not on a context attached to a rank (rank %d of %d): a slab holds only its own share of the mesh", me, c->rank, c->n_ranks);
    if (n_ref < 0 || n_ref > (int64_t)INT32_MAX || n_ref_faces < 0 || (n_ref_faces > 0 && !ref_faces))
        return fail(c, PSGSDF_ERR_ARG, "%s: %lld reference points, %lld faces%s", me, (long long)n_ref, (long long)n_ref_faces, n_ref_faces > 0 && !ref_faces ? " (null)" : "");
    const psgsdf_compare_params& P = *params;
    if (!(P.max_dist > 0.0) || std::isinf(P.max_dist) || !(P.tau > 0.0) || !(P.tau <= P.max_dist) || !(P.grid_cell >= 0.0) || std::isinf(P.grid_cell) || P.reserved[0] != 0 || P.reserved[1] != 0)
        return fail(c, PSGSDF_ERR_ARG, "%s: max_dist %g, tau %g, grid_cell %g, reserved %d %d (finite, 0 < tau <= max_dist, grid_cell >= 0, reserved 0)", me, P.max_dist, P.tau, P.grid_cell, P.reserved[0], P.reserved[1]);
    if (c && c->have_volume && P.max_dist > 64.0 * (double)c->grid.vs) return fail(c, PSGSDF_ERR_ARG, "%s: max_dist %g is more than 64 voxels of %g", me, P.max_dist, (double)c->grid.vs);
    for (int64_t i = 0; i < 3 * n_ref_faces; ++i)
        if (ref_faces[i] < 0 || (int64_t)ref_faces[i] >= n_ref) return fail(c, PSGSDF_ERR_ARG, "%s: face %lld has the index %d (%lld reference points)", me, (long long)(i / 3), ref_faces[i], (long long)n_ref);
    if (filter && bad_filter(*filter)) return fail(c, PSGSDF_ERR_ARG, "%s: min_area is NaN or keep_largest < 0", me);
    if (n_ref_faces > (int64_t)INT32_MAX) return fail(c, PSGSDF_ERR_UNSUPPORTED, "%s: %lld reference faces", me, (long long)n_ref_faces);
    { int rc = extract_ready(c, me); if (rc) return rc; }
    *out = psgsdf_compare{};
    auto bail = [&](int rc) { *out = psgsdf_compare{}; return rc; };
    const double vs = (double)c->grid.vs;
    DevMem mem(c);
    // the compared mesh, on the device and in the slots of the call it mirrors
    MeshView mv;
    if (!filter) {
        WMeshDev m;
        if (int rc = wmesh_device(c, mem, &m)) return bail(rc);
        mv = m;
    } else {
        MCompDev d;
        if (int rc = mcomp_device(c, mem, me, *filter, &d)) return bail(rc);
        if (d.nc != 0 && d.nv > 0 && d.nf > 0) mv = d;      // (else: an empty mesh, or a filter that drops everything)
    }
    const size_t nv = (size_t)mv.nv, nf = (size_t)mv.nf;
    psgsdf_compare r{};
    if (int rc = download(c, me, {{XO_IMESH_XYZ, mv.xyz, sizeof(float) * 3 * nv, &r.xyz}, {XO_IMESH_NORMALS, mv.nrm, sizeof(float) * 3 * nv, &r.normals}, {XO_IMESH_RGB, mv.rgb, 3 * nv, &r.rgb},
                                  {XO_IMESH_FACES, mv.faces, sizeof(int) * 3 * nf, &r.faces}})) return bail(rc);
    r.n_vertices = (int64_t)nv; r.n_faces = (int64_t)nf;
    // the reference, uploaded once
    float* d_rxyz = nullptr; int* d_rfaces = nullptr;
    if ((n_ref > 0 && !mem.get(&d_rxyz, 3 * (size_t)n_ref)) || (n_ref_faces > 0 && !mem.get(&d_rfaces, 3 * (size_t)n_ref_faces)))
        return bail(fail(c, PSGSDF_ERR_DEVICE, "%s: out of memory (%lld reference points, %lld faces)", me, (long long)n_ref, (long long)n_ref_faces));
    if ((n_ref > 0 && hipMemcpyAsync(d_rxyz, ref_xyz, sizeof(float) * 3 * (size_t)n_ref, hipMemcpyHostToDevice, c->stream) != hipSuccess)
        || (n_ref_faces > 0 && hipMemcpyAsync(d_rfaces, ref_faces, sizeof(int) * 3 * (size_t)n_ref_faces, hipMemcpyHostToDevice, c->stream) != hipSuccess))
        return bail(fail(c, PSGSDF_ERR_DEVICE, "%s: upload", me));
    // one box for both grids: a matching pair has its query in the queries' box and its closest point within max_dist of it and in the targets'
    // box, so both lie in the intersection of the two boxes inflated by max_dist (taken a little larger: rounding never drops a pair at the rim)
    const double cell = P.grid_cell > 0.0 ? P.grid_cell : 2.0 * vs;
    const CmpBox bm = cmp_bbox(r.xyz, nv), br = cmp_bbox(ref_xyz, (size_t)n_ref);
    CmpBox box; box.any = bm.any && br.any;
    const double grow = P.max_dist * (1.0 + 1e-6) + 1e-6 * cell;
    for (int k = 0; k < 3 && box.any; ++k) {
        box.lo[k] = std::max(bm.lo[k], br.lo[k]) - grow; box.hi[k] = std::min(bm.hi[k], br.hi[k]) + grow;
        if (!(box.lo[k] <= box.hi[k])) box.any = false;      // the two are farther apart than 2 max_dist: nothing matches
    }
    psg::CompareArgs a{};
    a.max_dist = P.max_dist; a.tau = P.tau; a.vs = vs;
    // the mesh's vertices against the reference
    a.q_xyz = mv.xyz; a.nq = (long long)nv;
    a.t_xyz = d_rxyz; a.t_faces = d_rfaces; a.nt = (int)(n_ref_faces > 0 ? n_ref_faces : n_ref);
    if (int rc = compare_direction(c, mem, me, a, box, cell, 0, CmpOut{XO_CMP_VDIST, XO_CMP_VNEAREST, XO_CMP_VSIDE, &r.vertex_dist, &r.vertex_nearest, &r.vertex_side}, &r.to_reference)) return bail(rc);
    // the reference's points against the mesh's faces
    a.q_xyz = d_rxyz; a.nq = (long long)n_ref;
    a.t_xyz = mv.xyz; a.t_faces = mv.faces; a.nt = (int)nf;
    if (int rc = compare_direction(c, mem, me, a, box, cell, 1, CmpOut{XO_CMP_RDIST, XO_CMP_RNEAREST, XO_CMP_RSIDE, &r.ref_dist, &r.ref_nearest, &r.ref_side}, &r.to_reconstruction)) return bail(rc);
    if (r.to_reference.n_valid > 0) r.precision = (double)r.to_reference.n_within_tau / (double)r.to_reference.n_valid;
    if (r.to_reconstruction.n_valid > 0) r.recall = (double)r.to_reconstruction.n_within_tau / (double)r.to_reconstruction.n_valid;
    if (r.precision + r.recall > 0.0) r.fscore = 2.0 * r.precision * r.recall / (r.precision + r.recall);
    *out = r;
    return PSGSDF_OK;
}

// ---- alignment of a reference to the compared mesh (include/psgsdf_align.h; kernels: align.hip and compare.hip's search): the two grids are built
// once, every evaluation moves the points, searches, reduces the rows to one 6x6 system on the device and brings 32 doubles to the host, which
// solves and composes in double.
namespace {
// the step of the header: 0 and xi, or 1 (a pivot <= 1e-6: degenerate); *min_pivot the smallest pivot met
int align_solve(const double* sys, double* min_pivot, double* xi) {
    double A[6][6], S[6][6], L[6][6] = {}, s[6], b[6], z[6], w[6];
    for (int i = 0, k = 0; i < 6; ++i) for (int j = i; j < 6; ++j, ++k) A[i][j] = A[j][i] = sys[psg::AL_A + k];
    *min_pivot = 0.0;
    for (int i = 0; i < 6; ++i) { if (!(A[i][i] > 0.0)) return 1; s[i] = sqrt(A[i][i]); }
    for (int i = 0; i < 6; ++i) for (int j = 0; j < 6; ++j) S[i][j] = A[i][j] / (s[i] * s[j]);
    double mp = INFINITY;
    for (int j = 0; j < 6; ++j) {
        double d = S[j][j];
        for (int k = 0; k < j; ++k) d = d - L[j][k] * L[j][k];
        if (!(d >= mp)) mp = d;
        *min_pivot = mp;
        if (!(d > 1e-6)) return 1;
        L[j][j] = sqrt(d);
        for (int i = j + 1; i < 6; ++i) {
            double v = S[i][j];
            for (int k = 0; k < j; ++k) v = v - L[i][k] * L[j][k];
            L[i][j] = v / L[j][j];
        }
    }
    for (int i = 0; i < 6; ++i) b[i] = -(sys[psg::AL_G + i] / s[i]);
    for (int i = 0; i < 6; ++i) { double v = b[i]; for (int k = 0; k < i; ++k) v = v - L[i][k] * z[k]; z[i] = v / L[i][i]; }
    for (int i = 5; i >= 0; --i) { double v = z[i]; for (int k = i + 1; k < 6; ++k) v = v - L[k][i] * w[k]; w[i] = v / L[i][i]; }
    for (int i = 0; i < 6; ++i) xi[i] = w[i] / s[i];
    return 0;
}
inline double aln_dot(const double* u, const double* v) { return (u[0] * v[0] + u[1] * v[1]) + u[2] * v[2]; }
// T <- Delta o T with Delta(x) = c + Exp(omega)(x - c) + v; T is 3x4 row-major
void align_compose(double* T, const double* om, const double* v, const double* c) {
    const double th2 = aln_dot(om, om), th = sqrt(th2);
    double a, b;
    if (th < 1e-8) { a = 1.0 - th2 / 6.0; b = 0.5 - th2 / 24.0; } else { a = sin(th) / th; b = (1.0 - cos(th)) / th2; }
    const double K[3][3] = {{0.0, -om[2], om[1]}, {om[2], 0.0, -om[0]}, {-om[1], om[0], 0.0}};
    double E[3][3], N[12];
    for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) E[i][j] = ((i == j ? 1.0 : 0.0) + a * K[i][j]) + b * (om[i] * om[j] - (i == j ? th2 : 0.0));
    for (int i = 0; i < 3; ++i) {
        for (int j = 0; j < 3; ++j) N[4 * i + j] = (E[i][0] * T[j] + E[i][1] * T[4 + j]) + E[i][2] * T[8 + j];
        const double t[3] = {T[3], T[7], T[11]};
        N[4 * i + 3] = aln_dot(E[i], t) + ((c[i] - aln_dot(E[i], c)) + v[i]);
    }
    memcpy(T, N, sizeof(N));
}
}  // namespace

extern "C" int psgsdf_align_reference(psgsdf_ctx* c, const psgsdf_mesh_filter* filter, const float* ref_xyz, int64_t n_ref, const int32_t* ref_faces, int64_t n_ref_faces,
                                      const psgsdf_align_params* params, psgsdf_align* out) {
    const char* me = "align_reference";
    if (!params || !out || (n_ref > 0 && !ref_xyz)) return fail(c, PSGSDF_ERR_ARG, "%s: null argument", me);
    // (before anything collective and before any device work: no rank waits for another)
    if (c && c->n_ranks > 1) return fail(c, PSGSDF_ERR_UNSUPPORTED, "%s: not on a context attached to a rank (rank %d of %d): a slab holds only its own share of the mesh", me, c->rank, c->n_ranks);
    if (n_ref < 0 || n_ref > (int64_t)INT32_MAX || n_ref_faces < 0 || (n_ref_faces > 0 && !ref_faces))
        return fail(c, PSGSDF_ERR_ARG, "%s: %lld reference points, %lld faces%s", me, (long long)n_ref, (long long)n_ref_faces, n_ref_faces > 0 && !ref_faces ? " (null)" : "");
    const psgsdf_align_params& P = *params;
    {   // init: finite, last row 0 0 0 1, R^T R = I to 1e-6
        bool rigid = P.init[12] == 0.0 && P.init[13] == 0.0 && P.init[14] == 0.0 && P.init[15] == 1.0;
        for (int i = 0; i < 12; ++i) rigid = rigid && std::isfinite(P.init[i]);
        for (int i = 0; i < 3 && rigid; ++i)
            for (int j = 0; j < 3; ++j) {
                const double g = (P.init[i] * P.init[j] + P.init[4 + i] * P.init[4 + j]) + P.init[8 + i] * P.init[8 + j];
                rigid = rigid && fabs(g - (i == j ? 1.0 : 0.0)) <= 1e-6;
            }
        if (!rigid) return fail(c, PSGSDF_ERR_ARG, "%s: init is not a rigid transform (finite, last row 0 0 0 1, R^T R = I to 1e-6)", me);
    }
    if (!(P.max_dist > 0.0) || std::isinf(P.max_dist) || !(P.min_dist > 0.0) || !(P.min_dist <= P.max_dist) || !(P.shrink > 0.0) || !(P.shrink <= 1.0) || !(P.eps_rot >= 0.0) || std::isinf(P.eps_rot)
        || !(P.eps_trans >= 0.0) || std::isinf(P.eps_trans) || !(P.grid_cell >= 0.0) || std::isinf(P.grid_cell) || P.directions < 1 || P.directions > 3 || P.max_iters < 0 || P.max_iters > 64
        || P.reserved[0] != 0 || P.reserved[1] != 0)
        return fail(c, PSGSDF_ERR_ARG, "%s: max_dist %g, min_dist %g, shrink %g, eps_rot %g, eps_trans %g, grid_cell %g, directions %d, max_iters %d, reserved %d %d (finite, 0 < min_dist <= max_dist, 0 < shrink <= 1, "
                    "eps >= 0, grid_cell >= 0, directions 1 .. 3, max_iters 0 .. 64, reserved 0)", me, P.max_dist, P.min_dist, P.shrink, P.eps_rot, P.eps_trans, P.grid_cell, P.directions, P.max_iters, P.reserved[0], P.reserved[1]);
    if (c && c->have_volume && P.max_dist > 64.0 * (double)c->grid.vs) return fail(c, PSGSDF_ERR_ARG, "%s: max_dist %g is more than 64 voxels of %g", me, P.max_dist, (double)c->grid.vs);
    for (int64_t i = 0; i < 3 * n_ref_faces; ++i)
        if (ref_faces[i] < 0 || (int64_t)ref_faces[i] >= n_ref) return fail(c, PSGSDF_ERR_ARG, "%s: face %lld has the index %d (%lld reference points)", me, (long long)(i / 3), ref_faces[i], (long long)n_ref);
    if (filter && bad_filter(*filter)) return fail(c, PSGSDF_ERR_ARG, "%s: min_area is NaN or keep_largest < 0", me);
    if (n_ref_faces > (int64_t)INT32_MAX) return fail(c, PSGSDF_ERR_UNSUPPORTED, "%s: %lld reference faces", me, (long long)n_ref_faces);
    { int rc = extract_ready(c, me); if (rc) return rc; }
    *out = psgsdf_align{};
    auto bail = [&](int rc) { *out = psgsdf_align{}; return rc; };
    const double vs = (double)c->grid.vs;
    c->aln_evals = c->aln_iters = 0; c->aln_pairs[0] = c->aln_pairs[1] = c->aln_queries[0] = c->aln_queries[1] = 0;
    DevMem mem(c);
    // the compared mesh, on the device and in the slots of the call it mirrors
    MeshView mv;
    if (!filter) {
        WMeshDev m;
        if (int rc = wmesh_device(c, mem, &m)) return bail(rc);
        mv = m;
    } else {
        MCompDev d;
        if (int rc = mcomp_device(c, mem, me, *filter, &d)) return bail(rc);
        if (d.nc != 0 && d.nv > 0 && d.nf > 0) mv = d;      // (else: an empty mesh, or a filter that drops everything)
    }
    const size_t nv = (size_t)mv.nv, nf = (size_t)mv.nf;
    psgsdf_align r{};
    if (int rc = download(c, me, {{XO_IMESH_XYZ, mv.xyz, sizeof(float) * 3 * nv, &r.xyz}, {XO_IMESH_NORMALS, mv.nrm, sizeof(float) * 3 * nv, &r.normals}, {XO_IMESH_RGB, mv.rgb, 3 * nv, &r.rgb},
                                  {XO_IMESH_FACES, mv.faces, sizeof(int) * 3 * nf, &r.faces}})) return bail(rc);
    r.n_vertices = (int64_t)nv; r.n_faces = (int64_t)nf; r.n_ref = n_ref;
    memcpy(r.transform, P.init, sizeof(r.transform));
    // the reference, uploaded once; the moved points of both directions
    const bool dir1 = (P.directions & 1) != 0, dir2 = (P.directions & 2) != 0;
    float *d_rxyz = nullptr, *d_mref = nullptr, *d_mvert = nullptr; int* d_rfaces = nullptr;
    if ((n_ref > 0 && !(mem.get(&d_rxyz, 3 * (size_t)n_ref) && mem.get(&d_mref, 3 * (size_t)n_ref))) || (n_ref_faces > 0 && !mem.get(&d_rfaces, 3 * (size_t)n_ref_faces))
        || (dir2 && nv > 0 && !mem.get(&d_mvert, 3 * nv)))
        return bail(fail(c, PSGSDF_ERR_DEVICE, "%s: out of memory (%lld reference points, %lld faces)", me, (long long)n_ref, (long long)n_ref_faces));
    if ((n_ref > 0 && hipMemcpyAsync(d_rxyz, ref_xyz, sizeof(float) * 3 * (size_t)n_ref, hipMemcpyHostToDevice, c->stream) != hipSuccess)
        || (n_ref_faces > 0 && hipMemcpyAsync(d_rfaces, ref_faces, sizeof(int) * 3 * (size_t)n_ref_faces, hipMemcpyHostToDevice, c->stream) != hipSuccess))
        return bail(fail(c, PSGSDF_ERR_DEVICE, "%s: upload", me));
    // each grid covers its targets' box inflated by max_dist (a little more: rounding never drops a pair at the rim): the radius only shrinks, and
    // the search clamps or skips a query outside the box
    const double cell = P.grid_cell > 0.0 ? P.grid_cell : 2.0 * vs;
    const double grow = P.max_dist * (1.0 + 1e-6) + 1e-6 * cell;
    CmpBox bm = cmp_bbox(r.xyz, nv), br = cmp_bbox(ref_xyz, (size_t)n_ref);
    double ctr[3] = {0.0, 0.0, 0.0};
    for (int k = 0; k < 3 && bm.any; ++k) ctr[k] = (bm.lo[k] + bm.hi[k]) / 2.0;
    memcpy(r.centre, ctr, sizeof(ctr));
    for (int k = 0; k < 3; ++k) { bm.lo[k] -= grow; bm.hi[k] += grow; br.lo[k] -= grow; br.hi[k] += grow; }
    psg::AlignRowArgs R1{}, R2{};
    int nb1 = 0, nb2 = 0;
    double* d_sys = nullptr;
    if (!mem.get(&d_sys, (size_t)psg::kAlignSys)) return bail(fail(c, PSGSDF_ERR_DEVICE, "%s: out of memory", me));
    if (dir1 && n_ref > 0) {      // the moved reference points against the mesh's faces
        psg::CompareArgs& a = R1.s;
        a.vs = vs; a.tau = P.max_dist; a.max_dist = P.max_dist;
        a.q_xyz = d_mref; a.nq = (long long)n_ref; a.t_xyz = mv.xyz; a.t_faces = mv.faces; a.nt = (int)nf;
        nb1 = (int)psg::align_row_blocks(a.nq);
        if (!compare_query_arrays(mem, a) || !mem.get(&R1.partial, (size_t)nb1 * psg::kAlignRow)) return bail(fail(c, PSGSDF_ERR_DEVICE, "%s: out of memory (%lld queries)", me, a.nq));
        if (int rc = compare_grid(c, mem, me, a, bm, cell)) return bail(rc);
    }
    if (dir2 && nv > 0) {         // the mesh's vertices, moved into the reference's units, against the reference's targets
        psg::CompareArgs& a = R2.s;
        a.vs = vs; a.tau = P.max_dist; a.max_dist = P.max_dist;
        a.q_xyz = d_mvert; a.nq = (long long)nv; a.t_xyz = d_rxyz; a.t_faces = d_rfaces; a.nt = (int)(n_ref_faces > 0 ? n_ref_faces : n_ref);
        nb2 = (int)psg::align_row_blocks(a.nq);
        if (!compare_query_arrays(mem, a) || !mem.get(&R2.partial, (size_t)nb2 * psg::kAlignRow)) return bail(fail(c, PSGSDF_ERR_DEVICE, "%s: out of memory (%lld queries)", me, a.nq));
        if (int rc = compare_grid(c, mem, me, a, br, cell)) return bail(rc);
    }
    for (psg::AlignRowArgs* R : {&R1, &R2}) { memcpy(R->c, ctr, sizeof(ctr)); R->vs = vs; R->v_xyz = mv.xyz; R->v_nrm = mv.nrm; }
    double T[12];
    memcpy(T, P.init, sizeof(T));
    // one evaluation at T with the radius: 32 doubles and one wait
    auto evaluate = [&](double radius, double* sys) -> int {
        double Ti[12];
        for (int i = 0; i < 3; ++i) {
            for (int j = 0; j < 3; ++j) Ti[4 * i + j] = T[4 * j + i];
            Ti[4 * i + 3] = -((T[i] * T[3] + T[4 + i] * T[7]) + T[8 + i] * T[11]);
        }
        hipError_t e = hipSuccess;
        psg::AlignMoveArgs m{};
        memcpy(m.M, T, sizeof(T)); m.src = d_rxyz; m.dst = d_mref; m.n = (long long)n_ref;
        timed(c, "align_move", [&] { e = psg::launch_align_move(m, c->stream); });
        if (e == hipSuccess && nb2 > 0) {
            memcpy(m.M, Ti, sizeof(Ti)); m.src = mv.xyz; m.dst = d_mvert; m.n = (long long)nv;
            timed(c, "align_move", [&] { e = psg::launch_align_move(m, c->stream); });
        }
        if (e == hipSuccess && nb1 > 0) {
            R1.s.max_dist = radius;
            timed(c, "align_query_1", [&] { e = psg::launch_compare_query(R1.s, c->compare_chunk, c->stream); });
            if (e == hipSuccess) timed(c, "align_rows_1", [&] { e = psg::launch_align_rows(R1, 1, c->stream); });
        }
        if (e == hipSuccess && nb2 > 0) {
            R2.s.max_dist = radius; memcpy(R2.T, T, sizeof(T));
            timed(c, "align_query_2", [&] { e = psg::launch_compare_query(R2.s, c->compare_chunk, c->stream); });
            if (e == hipSuccess) timed(c, "align_rows_2", [&] { e = psg::launch_align_rows(R2, 2, c->stream); });
        }
        if (e == hipSuccess) timed(c, "align_fold", [&] { e = psg::launch_align_fold(R1.partial, nb1, R2.partial, nb2, d_sys, c->stream); });
        if (e != hipSuccess) return fail(c, PSGSDF_ERR_DEVICE, "%s: launch: %s", me, hipGetErrorString(e));
        if (hipMemcpyAsync(sys, d_sys, sizeof(double) * psg::kAlignSys, hipMemcpyDeviceToHost, c->stream) != hipSuccess || hipStreamSynchronize(c->stream) != hipSuccess)
            return fail(c, PSGSDF_ERR_DEVICE, "%s: download of the system", me);
        c->aln_evals += 1;
        c->aln_queries[0] += nb1 > 0 ? R1.s.nq : 0; c->aln_queries[1] += nb2 > 0 ? R2.s.nq : 0;
        c->aln_pairs[0] += (long long)sys[psg::AS_PAIRS]; c->aln_pairs[1] += (long long)sys[psg::AS_PAIRS + 1];
        return PSGSDF_OK;
    };
    r.status = PSGSDF_ALIGN_MAX_ITERS;
    bool last = P.max_iters == 0;
    double pw = 1.0;
    for (int k = 0;; ++k) {
        const double radius = std::max(P.min_dist, P.max_dist * pw);
        double sys[psg::kAlignSys];
        if (int rc = evaluate(radius, sys)) return bail(rc);
        if (k == 0) memcpy(r.system0, sys, sizeof(r.system0));
        psgsdf_align_iter it{};
        const double n = sys[psg::AS_N] + sys[psg::AS_N + 1];
        it.radius = radius; it.rms = n > 0.0 ? vs * sqrt(sys[psg::AL_E] / n) : 0.0;
        it.n_pairs[0] = (int64_t)sys[psg::AS_N]; it.n_pairs[1] = (int64_t)sys[psg::AS_N + 1];
        r.final = it;
        if (last) { if (r.n_iters == 0 && n < 6.0) r.status = PSGSDF_ALIGN_TOO_FEW; break; }
        if (n < 6.0) { r.status = PSGSDF_ALIGN_TOO_FEW; r.iters[k] = it; break; }
        double xi[6];
        const int deg = align_solve(sys, &it.min_pivot, xi);
        if (deg) { r.status = PSGSDF_ALIGN_DEGENERATE; r.iters[k] = it; break; }
        const double v[3] = {xi[3] * vs, xi[4] * vs, xi[5] * vs};
        for (int i = 0; i < 3; ++i) { it.step[i] = xi[i]; it.step[3 + i] = v[i]; }
        r.iters[k] = it; r.n_iters = k + 1;
        align_compose(T, xi, v, ctr);
        memcpy(r.transform, T, sizeof(T));
        const bool conv = sqrt(aln_dot(xi, xi)) <= P.eps_rot && sqrt(aln_dot(v, v)) <= P.eps_trans;
        if (conv) r.status = PSGSDF_ALIGN_CONVERGED;
        last = conv || k + 1 == P.max_iters;
        pw *= P.shrink;
    }
    c->aln_iters = r.n_iters;
    if (int rc = download(c, me, {{XO_ALN_XYZ, d_mref, sizeof(float) * 3 * (size_t)n_ref, &r.aligned_xyz}})) return bail(rc);
    *out = r;
    return PSGSDF_OK;
}
