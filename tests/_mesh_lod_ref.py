"""Yardstick of the level-of-detail mesh by vertex clustering (include/psgsdf_mesh.h psgsdf_extract_mesh_lod, DESIGN.md "Level of detail"), in numpy,
written from the definition: np.floor of the float64 quotient for the cluster of a vertex, np.unique for the clusters and the faces' unordered
triples, np.rint for the fixed point, integer sums with np.add.at.

    lod(xyz, normals, rgb, faces, vs, cell) -> dict of xyz, normals, rgb, faces, vertex_map, n_vertices_in, n_faces_in (what Api.extract_mesh_lod
                                               returns) plus n_clusters, n_collapsed, n_duplicates
xyz, normals, rgb, faces: the input mesh (a welded mesh, or one filtered by its components); vs: the voxel size (rounded to float32 here);
cell: the cluster size in the mesh's units, a float64.  Raises ValueError where the call returns PSGSDF_ERR_ARG / PSGSDF_ERR_UNSUPPORTED."""
import numpy as np

LIMIT = 1 << 20      # |cluster coordinate| < 2^20: three biased coordinates pack into 63 bits
FIX = 1048576.0      # one voxel (one unit normal) = 2^20 fixed-point units


def clusters(xyz, cell):
    """integer cluster coordinates [V, 3] of the float32 positions: floor of the IEEE double quotient"""
    cell = float(cell)
    if not (np.isfinite(cell) and cell > 0):
        raise ValueError("cell")
    c = np.floor(np.asarray(xyz, np.float32).astype(np.float64) / cell)
    if len(c) and not (np.abs(c) < LIMIT).all():
        raise ValueError("cluster coordinate beyond 2^20")
    return c.astype(np.int64)


def lod(xyz, normals, rgb, faces, vs, cell):
    xyz = np.asarray(xyz, np.float32).reshape(-1, 3); normals = np.asarray(normals, np.float32).reshape(-1, 3)
    rgb = np.asarray(rgb, np.uint8).reshape(-1, 3); faces = np.asarray(faces, np.int64).reshape(-1, 3)
    vs = float(np.float32(vs))
    V, F = len(xyz), len(faces)
    c = clusters(xyz, cell) + LIMIT
    key = (c[:, 0] << 42) | (c[:, 1] << 21) | c[:, 2]
    _, cl = np.unique(key, return_inverse=True)      # cluster of every vertex (numbered by key: only equality matters)
    cl = cl.reshape(-1)
    K = int(cl.max()) + 1 if V else 0
    first = np.full(K, V, np.int64)
    np.minimum.at(first, cl, np.arange(V))
    n = np.bincount(cl, minlength=K).astype(np.int64)
    # faces: degenerate ones dropped, of equal unordered triples the smallest face index kept, input order
    fc = cl[faces]
    nondeg = (fc[:, 0] != fc[:, 1]) & (fc[:, 1] != fc[:, 2]) & (fc[:, 0] != fc[:, 2]) if F else np.zeros(0, bool)
    idx = np.nonzero(nondeg)[0]
    tri = np.sort(fc[idx], 1)
    _, where = np.unique(tri, return_index=True, axis=0)      # (return_index: the first occurrence = the smallest face index)
    kept = np.sort(idx[where]) if len(idx) else idx
    # vertices: the clusters of the kept faces, in ascending smallest member
    used = np.zeros(K, bool)
    used[fc[kept].reshape(-1)] = True
    order = np.nonzero(used)[0]
    order = order[np.argsort(first[order])]
    num = np.full(K, -1, np.int64); num[order] = np.arange(len(order))
    vertex_map = num[cl].astype(np.int32) if V else np.zeros(0, np.int32)
    out_faces = num[fc[kept]].astype(np.int32).reshape(-1, 3)
    # attributes: integer sums, so any order of addition gives the same bits
    x = xyz.astype(np.float64)
    S = np.zeros((K, 3), np.int64); np.add.at(S, cl, np.rint(x * FIX / vs).astype(np.int64))
    T = np.zeros((K, 3), np.int64); np.add.at(T, cl, np.rint(normals.astype(np.float64) * FIX).astype(np.int64))
    C = np.zeros((K, 3), np.int64); np.add.at(C, cl, rgb.astype(np.int64))
    S, T, C, nn = S[order], T[order], C[order], n[order]
    nd = nn.astype(np.float64)[:, None]
    pos = (S.astype(np.float64) / nd * (vs / FIX)).astype(np.float32)
    t = T.astype(np.float64)
    length = np.sqrt((t[:, 0] * t[:, 0] + t[:, 1] * t[:, 1]) + t[:, 2] * t[:, 2])
    nrm = np.where(length[:, None] > 0, t / np.where(length > 0, length, 1.0)[:, None], 0.0).astype(np.float32)
    col = ((2 * C + nn[:, None]) // (2 * nn[:, None])).astype(np.uint8)
    one = nn == 1      # a single-member cluster keeps its member bit for bit
    pos[one] = xyz[first[order][one]]; nrm[one] = normals[first[order][one]]; col[one] = rgb[first[order][one]]
    return dict(xyz=pos.reshape(-1, 3), normals=nrm.reshape(-1, 3), rgb=col.reshape(-1, 3), faces=out_faces, vertex_map=vertex_map, n_vertices_in=V, n_faces_in=F,
                n_clusters=K, n_single=int((n == 1).sum()), n_collapsed=int(F - len(idx)), n_duplicates=int(len(idx) - len(kept)))
