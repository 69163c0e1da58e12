// extract_mesh.hip -- the C ABI of include/psgsdf_mesh.h: the welded, indexed mesh of the context's state (kernels: mesh.hip; DESIGN.md "Welded
// meshes"), its connected components and the mesh without its small pieces (mesh_cc.hip; "Mesh components") and a level-of-detail mesh by vertex
// clustering (mesh_lod.hip; "Level of detail"); and of include/psgsdf_fit.h: the photometric fit per band row and per vertex of the welded mesh
// (fit.hip; "Photometric fit per voxel and vertex").  It defines the stages of mesh_stages.h, which extract_bake.hip and extract_compare.hip go on from.
// The frame arithmetic (extract_internal.h crop_frame) runs on the host and its results are compared bit for bit: no FMA contraction here either.
#pragma clang fp contract(off)
#include "mesh_stages.h"
#include "../../include/psgsdf_fit.h"
#include "mesh_lod.h"

using namespace psge;

namespace psge {
// ---- stage 1 (mesh_stages.h)
int wmesh_device(psgsdf_ctx* c, DevMem& mem, WMeshDev* m, const PlaneView* pv) {
    const char* me = "extract_mesh_indexed";
    int lo[3], hi[3]; bool any = false;
    { int rc = crop_box_dev(c, lo, hi, &any, pv ? pv->dist : nullptr); if (rc) return rc; }      // (collective: every rank takes the same early returns below)
    if (!any) return PSGSDF_OK;
    psg::WMeshGrid g{}; int zc1 = 0;
    if (!crop_frame(c, lo, hi, g, &zc1, pv)) return PSGSDF_OK;      // psgsdf_extract_mesh's frame
    for (int a = 0; a < 3; ++a) g.g[a] = pv ? pv->g[a] : c->dense.g[a];
    if (pv && pv->framed) {      // another box's frame, crop_frame's arithmetic on that box: a voxel has the position it has in a mesh of that box
        const float vs = c->grid.vs;
        for (int a = 0; a < 3; ++a) {
            const float size = vs * pv->fd[a];
            g.voxel[a] = size / pv->fd[a]; g.origin[a] = -vs * pv->flo[a]; g.poff[a] = lo[a] - pv->flo[a];
        }
    }
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
// ---- stage 2 (mesh_stages.h)
bool bad_filter(const psgsdf_mesh_filter& flt) { return flt.min_area != flt.min_area || flt.keep_largest < 0; }
int mcomp_device(psgsdf_ctx* c, DevMem& mem, const char* me, const psgsdf_mesh_filter& flt, MCompDev* d, const PlaneView* pv) {
    WMeshDev m;
    if (int rc = wmesh_device(c, mem, &m, pv)) return rc;
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
    static_cast<MeshView&>(*d) = m; d->vertex_component = vcomp; d->nc = nc; d->list = list; d->welded = m;
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
    d->xyz = o_xyz; d->nrm = o_nrm; d->rgb = o_rgb; d->faces = o_faces; d->vertex_component = o_vcomp; d->nv = ov; d->nf = of; d->vkeep = vflag;
    return PSGSDF_OK;
}
int compared_mesh(psgsdf_ctx* c, DevMem& mem, const char* me, const psgsdf_mesh_filter* filter, MeshView* mv) {
    *mv = MeshView{};
    WMeshDev m; MCompDev d;
    if (int rc = filter ? mcomp_device(c, mem, me, *filter, &d) : wmesh_device(c, mem, &m)) return rc;
    if (!filter) *mv = m;
    else if (d.nc != 0 && d.nv > 0 && d.nf > 0) *mv = d;
    return PSGSDF_OK;
}
int download_mesh(psgsdf_ctx* c, const char* me, const MeshView& mv, const MeshOut& o, std::initializer_list<XoCopy> more) {
    const size_t nv = (size_t)mv.nv, nf = (size_t)mv.nf;
    std::vector<XoCopy> list{{XO_IMESH_XYZ, mv.xyz, sizeof(float) * 3 * nv, o.xyz}, {XO_IMESH_NORMALS, mv.nrm, sizeof(float) * 3 * nv, o.normals}, {XO_IMESH_RGB, mv.rgb, 3 * nv, o.rgb},
                             {XO_IMESH_FACES, mv.faces, sizeof(int) * 3 * nf, o.faces}};
    list.insert(list.end(), more.begin(), more.end());
    return download(c, me, list);
}
// ---- stage 3 (mesh_stages.h)
int lod_from_device(psgsdf_ctx* c, DevMem& mem, const MeshView& in, double cell, const LodOut& o, MeshView* dev) {
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
int lod_ready(psgsdf_ctx* c, const char* me, const psgsdf_mesh_filter* filter, double cell) {
    if (int rc = single_rank_only(c, me, "clusters are not merged across z-slabs")) return rc;
    if (!(cell > 0.0) || std::isinf(cell)) return fail(c, PSGSDF_ERR_ARG, "%s: the cell must be a finite size > 0", me);
    if (filter && bad_filter(*filter)) return fail(c, PSGSDF_ERR_ARG, "%s: min_area is NaN or keep_largest < 0", me);
    return PSGSDF_OK;
}
int lod_stages(psgsdf_ctx* c, DevMem& mem, const char* me, const psgsdf_mesh_filter* filter, double cell, const LodOut& o, MeshView* dev) {
    MeshView in;
    if (int rc = compared_mesh(c, mem, me, filter, &in)) return rc;
    if (in.nv > 0 && in.nf > 0) return lod_from_device(c, mem, in, cell, o, dev);
    return hipStreamSynchronize(c->stream) != hipSuccess ? fail(c, PSGSDF_ERR_DEVICE, "%s: kernels", me) : PSGSDF_OK;
}
}  // namespace psge

extern "C" int psgsdf_extract_mesh_indexed(psgsdf_ctx* c, const float** xyz, const float** normals, const uint8_t** rgb, int64_t* n_vertices,
                                           const int32_t** faces, int64_t* n_faces, int64_t* first_vertex) {
    const char* me = "extract_mesh_indexed";
    if (!xyz || !normals || !rgb || !n_vertices || !faces || !n_faces || !first_vertex) return fail(c, PSGSDF_ERR_ARG, "%s: null argument", me);
    { int rc = extract_ready(c, me); if (rc) return rc; }
    *xyz = nullptr; *normals = nullptr; *rgb = nullptr; *faces = nullptr; *n_vertices = 0; *n_faces = 0; *first_vertex = 0;
    DevMem mem(c);
    WMeshDev m;
    if (int rc = wmesh_device(c, mem, &m)) return rc;
    if (int rc = download_mesh(c, me, m, {xyz, normals, rgb, faces})) return rc;
    *n_vertices = m.nv; *n_faces = m.nf; *first_vertex = m.first;
    return PSGSDF_OK;
}

extern "C" int psgsdf_extract_mesh_components(psgsdf_ctx* c, const psgsdf_mesh_filter* filter, const float** xyz, const float** normals, const uint8_t** rgb, int64_t* n_vertices,
                                              const int32_t** faces, int64_t* n_faces, const int32_t** vertex_component, const psgsdf_mesh_component** components, int64_t* n_components) {
    const char* me = "extract_mesh_components";
    if (!xyz || !normals || !rgb || !n_vertices || !faces || !n_faces || !vertex_component || !components || !n_components) return fail(c, PSGSDF_ERR_ARG, "%s: null argument", me);
    if (int rc = single_rank_only(c, me, "components are not merged across z-slabs yet")) return rc;
    psgsdf_mesh_filter flt{0, 0.0, 0};
    if (filter) flt = *filter;
    if (bad_filter(flt)) return fail(c, PSGSDF_ERR_ARG, "%s: min_area is NaN or keep_largest < 0", me);
    { int rc = extract_ready(c, me); if (rc) return rc; }
    *xyz = nullptr; *normals = nullptr; *rgb = nullptr; *faces = nullptr; *vertex_component = nullptr; *components = nullptr; *n_vertices = 0; *n_faces = 0; *n_components = 0;
    DevMem mem(c);
    MCompDev d;
    int rc = mcomp_device(c, mem, me, flt, &d);
    if (rc || d.nc == 0) return rc;      // (failed, or an empty mesh)
    MeshView kept = d;
    if (!(d.nv > 0 && d.nf > 0)) kept.nv = kept.nf = 0;      // (a filter may drop everything)
    rc = download_mesh(c, me, kept, {xyz, normals, rgb, faces}, {{XO_VERTEX_COMPONENT, d.vertex_component, sizeof(int) * (size_t)kept.nv, vertex_component}});
    if (rc) return rc;
    *n_vertices = kept.nv; *n_faces = kept.nf; *components = d.list; *n_components = d.nc;
    return PSGSDF_OK;
}

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
// what both calls check first
int fit_ready(psgsdf_ctx* c, const char* me) {
    if (int rc = single_rank_only(c, me, "the fit is not gathered across z-slabs")) return rc;
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
    const size_t nv = (size_t)m.nv;
    int* v_n = nullptr; float *v_rms = nullptr, *v_loss = nullptr;      // temporaries: 12 B per vertex
    if (nv > 0) {
        if (!mem.get(&v_n, nv) || !mem.get(&v_rms, nv) || !mem.get(&v_loss, nv)) return fail(c, PSGSDF_ERR_DEVICE, "%s: out of memory (%d vertices)", me, m.nv);
        timed(c, "wmesh_fit", [&] { psg::launch_wmesh_fit(m.grid, m.num, m.nv, c->dense.row_of, c->row0, c->row1, d.n_obs, d.loss, d.r2, v_n, v_rms, v_loss, c->stream); });
    }
    if (int rc = download_mesh(c, me, m, {xyz, normals, rgb, faces}, {{XO_VFIT_NOBS, v_n, sizeof(int) * nv, vertex_n_obs}, {XO_VFIT_RMS, v_rms, sizeof(float) * nv, vertex_rms},
                                                                      {XO_VFIT_LOSS, v_loss, sizeof(float) * nv, vertex_loss}})) return rc;
    *n_vertices = m.nv; *n_faces = m.nf;
    return PSGSDF_OK;
}
