"""Yardstick of the welded mesh's connected components (include/psgsdf_mesh.h psgsdf_extract_mesh_components, DESIGN.md "Mesh components"), on the
host: scipy's connected_components for the labels, np.unique for the edges (as _mesh_ref.topology), float64 for the areas with the definition's
llrint quantisation.

    analyse(xyz, faces, vs)                                    -> (labels [V], table): component of every vertex, components in ascending first vertex
    keep(table, min_faces, min_area, keep_largest)             -> kept [K] (0 / 1)
    filtered(arrays, labels, kept)                             -> the arrays of the kept components, faces renumbered, labels of the kept vertices
    components(xyz, faces, vs, **filter)                       -> all of it as the dict Api.extract_mesh_components returns (arrays: those given)
xyz, faces: an UNFILTERED welded mesh (every vertex is used by a face)."""
import numpy as np
from scipy.sparse import coo_matrix
from scipy.sparse.csgraph import connected_components

DTYPE = np.dtype([("first_vertex", "<i8"), ("n_vertices", "<i8"), ("n_faces", "<i8"), ("n_edges", "<i8"), ("n_boundary_edges", "<i8"),
                  ("n_nonmanifold_edges", "<i8"), ("area", "<f8"), ("lo", "<f4", (3,)), ("hi", "<f4", (3,)), ("kept", "<i4"), ("reserved", "<i4")])
INT_FIELDS = ("first_vertex", "n_vertices", "n_faces", "n_edges", "n_boundary_edges", "n_nonmanifold_edges")


def labels_of(faces, nv):
    """component of every vertex, the components numbered by their smallest vertex"""
    faces = np.asarray(faces, np.int64)
    i = np.concatenate([faces[:, 0], faces[:, 1]]); j = np.concatenate([faces[:, 1], faces[:, 2]])
    g = coo_matrix((np.ones(len(i), np.int8), (i, j)), shape=(nv, nv))
    n, lab = connected_components(g, directed=False)
    first = np.full(n, nv, np.int64)
    np.minimum.at(first, lab, np.arange(nv))
    rank = np.empty(n, np.int64); rank[np.argsort(first)] = np.arange(n)
    return rank[lab].astype(np.int32), np.sort(first)


def face_units(xyz, faces, vs):
    """llrint(2^24 A_f / vs^2) per face: A_f in float64 from the float32 positions, vs the float32 voxel size widened"""
    vs = float(np.float32(vs))
    p = np.asarray(xyz, np.float32).astype(np.float64)[np.asarray(faces, np.int64)]
    a, b = p[:, 1] - p[:, 0], p[:, 2] - p[:, 0]
    cx = a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1]; cy = a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2]; cz = a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]
    area = 0.5 * np.sqrt((cx * cx + cy * cy) + cz * cz)
    return np.rint(16777216.0 * area / (vs * vs)).astype(np.int64)


def analyse(xyz, faces, vs):
    nv = len(xyz)
    faces = np.asarray(faces, np.int64)
    if nv == 0 or len(faces) == 0:
        return np.zeros(0, np.int32), np.zeros(0, DTYPE)
    lab, first = labels_of(faces, nv)
    K = len(first)
    t = np.zeros(K, DTYPE)
    t["first_vertex"] = first
    t["n_vertices"] = np.bincount(lab, minlength=K)
    flab = lab[faces[:, 0]]
    t["n_faces"] = np.bincount(flab, minlength=K)
    und = np.sort(np.concatenate([faces[:, [0, 1]], faces[:, [1, 2]], faces[:, [2, 0]]]), 1)
    u, cnt = np.unique(und[:, 0] * nv + und[:, 1], return_counts=True)
    elab = lab[u // nv]
    t["n_edges"] = np.bincount(elab, minlength=K)
    t["n_boundary_edges"] = np.bincount(elab[cnt == 1], minlength=K)
    t["n_nonmanifold_edges"] = np.bincount(elab[cnt > 2], minlength=K)
    units = np.zeros(K, np.int64)
    np.add.at(units, flab, face_units(xyz, faces, vs))
    vs = float(np.float32(vs))
    t["area"] = vs * vs / 16777216.0 * units.astype(np.float64)
    x = np.asarray(xyz, np.float32)
    lo = np.full((K, 3), np.inf, np.float32); hi = np.full((K, 3), -np.inf, np.float32)
    np.minimum.at(lo, lab, x); np.maximum.at(hi, lab, x)
    t["lo"] = lo; t["hi"] = hi
    t["kept"] = 1
    return lab, t


def keep(table, min_faces=0, min_area=0.0, keep_largest=0):
    ok = (table["n_faces"] >= min_faces) & (table["area"] >= min_area)
    if keep_largest > 0:
        idx = np.nonzero(ok)[0]
        idx = idx[np.lexsort((table["first_vertex"][idx], -table["n_faces"][idx]))]      # most faces first, ties to the smaller first vertex
        ok = np.zeros(len(table), bool); ok[idx[:keep_largest]] = True
    return ok.astype(np.int32)


def filtered(arrays, labels, kept):
    """arrays: (xyz, normals, rgb, faces) of the unfiltered mesh -> (xyz, normals, rgb, faces, vertex_component) of the kept components"""
    xyz, nrm, rgb, faces = arrays
    vk = kept[labels].astype(bool)
    new = np.cumsum(vk) - 1
    fk = vk[faces[:, 0]] if len(faces) else np.zeros(0, bool)
    assert (vk[faces[fk]].all() if fk.any() else True)
    return xyz[vk], nrm[vk], rgb[vk], new[faces[fk]].astype(np.int32).reshape(-1, 3), labels[vk].astype(np.int32)


def components(xyz, faces, vs, normals=None, rgb=None, min_faces=0, min_area=0.0, keep_largest=0):
    lab, t = analyse(xyz, faces, vs)
    if len(t) == 0:
        z = np.zeros((0, 3), np.float32)
        return dict(xyz=z, normals=z, rgb=np.zeros((0, 3), np.uint8), faces=np.zeros((0, 3), np.int32), vertex_component=np.zeros(0, np.int32), components=t, labels=lab)
    t["kept"] = keep(t, min_faces, min_area, keep_largest)
    normals = np.zeros_like(xyz) if normals is None else normals
    rgb = np.zeros((len(xyz), 3), np.uint8) if rgb is None else rgb
    x, n, c, f, vc = filtered((xyz, normals, rgb, np.asarray(faces)), lab, t["kept"])
    return dict(xyz=x, normals=n, rgb=c, faces=f, vertex_component=vc, components=t, labels=lab)
