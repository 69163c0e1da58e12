"""The binding's marshalling helpers (psgradientsdf_amd/capi.py), without a library and without a GPU: the one path from an engine pointer to a numpy
array the caller owns, the mesh filter argument and the counts dict."""
import ctypes as C

import numpy as np
import pytest

from psgradientsdf_amd import capi


@pytest.mark.parametrize("shape", [(7,), (5, 3), (4, 6, 3), (2, 4, 6)], ids=str)      # (n,), (n, 3), (H, W, 3), (F, H, W)
@pytest.mark.parametrize("ctype,dtype", [(C.c_float, np.float32), (C.c_uint8, np.uint8), (C.c_int32, np.int32), (C.c_uint64, np.uint64), (C.c_double, np.float64), (C.c_int8, np.int8)])
def test_a_result_is_an_owned_copy(shape, ctype, dtype):
    n = int(np.prod(shape))
    buf = (ctype * n)(*range(1, n + 1))
    got = capi._owned(C.cast(buf, C.POINTER(ctype)), shape, dtype)
    assert got.dtype == dtype and got.shape == shape and got.flags.owndata and got.flags.c_contiguous
    exp = np.arange(1, n + 1).astype(dtype).reshape(shape)
    assert np.array_equal(got, exp)
    C.memset(buf, 0x55, C.sizeof(buf))      # the engine's next extraction call reuses the memory
    assert np.array_equal(got, exp)


@pytest.mark.parametrize("shape", [(0,), (0, 3), (0, 6), (0, 3, 2), (0, 0, 3), (0, 0), (0, 5, 7)], ids=str)
@pytest.mark.parametrize("ctype,dtype", [(C.c_float, np.float32), (C.c_uint8, np.uint8), (C.c_int64, np.int64)])
def test_a_zero_size_result_never_touches_the_pointer(shape, ctype, dtype):
    got = capi._owned(C.POINTER(ctype)(), shape, dtype)      # NULL: what the engine leaves behind an empty result
    assert got.dtype == dtype and got.shape == shape and got.size == 0 and got.flags.owndata


def test_zero_size_shapes_with_a_free_extent_keep_it():
    assert capi._owned(C.POINTER(C.c_float)(), (0, 48, 64), np.float32).shape == (0, 48, 64)      # extract_sdf's (0, d1, d0)
    assert capi._owned(C.POINTER(C.c_uint8)(), (4, 0, 0), np.uint8).shape == (4, 0, 0)             # a status stack of an atlas without texels


def test_mesh_filter_argument():
    assert capi._mesh_filter(0, 0.0, 0) is None and capi._mesh_filter(False, 0, 0.0) is None
    assert capi._ref(None) is None
    for args in ((3, 0.0, 0), (0, 0.25, 0), (0, 0.0, 2), (np.int64(3), np.float32(0.5), True), (2.0, 1, 1.0)):
        f = capi._mesh_filter(*args)
        assert isinstance(f, capi.MeshFilter)
        got = (f.min_faces, f.min_area, f.keep_largest)
        assert got == (int(args[0]), float(args[1]), int(args[2])) and [type(x) for x in got] == [int, float, int]
        assert capi._ref(f)._obj is f
    f = capi._mesh_filter(0, 0.0, 0, always=True)      # extract_mesh_components passes a filter always
    assert isinstance(f, capi.MeshFilter) and (f.min_faces, f.min_area, f.keep_largest) == (0, 0.0, 0)


@pytest.mark.parametrize("cls", [capi.AoCounts, capi.PhotoCounts, capi.RelightCounts])
def test_counts_are_plain_ints(cls):
    c = cls(*range(1, len(cls._fields_) + 1))
    got = capi._counts(c)
    assert list(got) == [k for k, _ in cls._fields_]
    assert all(type(v) is int for v in got.values()) and list(got.values()) == list(range(1, len(cls._fields_) + 1))
    arr = (cls * 2)(); arr[1] = c      # relight reads them out of an array
    assert capi._counts(arr[1]) == got and capi._counts(arr[0]) == dict.fromkeys(got, 0)


def test_mesh_head_hands_out_its_parameters_in_abi_order():
    m = capi._MeshHead()
    refs = m.refs()
    assert [r._obj for r in refs] == [m.xyz, m.normals, m.rgb, m._nv, m.faces, m._nf]
    assert [type(r._obj) for r in refs] == [C.POINTER(C.c_float), C.POINTER(C.c_float), C.POINTER(C.c_uint8), C.c_int64, C.POINTER(C.c_int32), C.c_int64]
    got = m.arrays()      # untouched by a call: the empty mesh, pointers NULL
    assert list(got) == ["xyz", "normals", "rgb", "faces"] and all(a.shape == (0, 3) for a in got.values())
    assert [a.dtype for a in got.values()] == [np.float32, np.float32, np.uint8, np.int32]
    xyz = (C.c_float * 6)(1, 2, 3, 4, 5, 6); fc = (C.c_int32 * 3)(0, 1, 0); rgb = (C.c_uint8 * 6)(*range(6))
    for r, buf in zip(refs, (xyz, xyz, rgb, 2, fc, 1)):      # what the engine stores through the six references
        C.c_void_p.from_address(C.addressof(r._obj)).value = buf if isinstance(buf, int) else C.addressof(buf)
    got = m.arrays()
    assert got["xyz"].tolist() == [[1, 2, 3], [4, 5, 6]] and got["faces"].tolist() == [[0, 1, 0]] and got["rgb"].shape == (2, 3)
    b = capi.Bake(n_vertices=2, n_faces=1)      # the same four arrays from a result struct's fields
    b.xyz, b.normals, b.rgb, b.faces = m.xyz, m.normals, m.rgb, m.faces
    assert all(np.array_equal(a, got[k]) and a.dtype == got[k].dtype for k, a in capi._mesh_arrays(b).items())
