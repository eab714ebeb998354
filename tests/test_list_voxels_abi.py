"""svo_tree_list_voxels_gpu without a device: the library exports it, the header declares it with its documented
prototype and names it among the entry points detected by symbol, every argument error is SVO_EINVAL with the function's
name in svo_last_error() — reported before the first HIP call, never SVO_EDEVICE, although this machine may have no GPU
— and a tree that is not uploaded is SVO_ESTATE from C and SvoError from Tree.count_voxels / Tree.list_voxels."""
import ctypes as C
import os
import re

import pytest

EINVAL, ESTATE = -1, -4
NAME = "svo_tree_list_voxels_gpu"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROTOTYPE = """int svo_tree_list_voxels_gpu(const svo_tree* t, const int32_t origin[3], int32_t nx, int32_t ny, int32_t nz,
                             int32_t* xyz, uint16_t* ids, int64_t cap, int64_t* n, void* hip_stream);"""


def _header():
    with open(os.path.join(ROOT, "include", "svo_rt.h")) as f:
        return f.read()


def test_library_exports_the_symbol(rt):
    assert hasattr(C.CDLL(rt.LIB_PATH), NAME)
    assert NAME in rt.ABI_SYMBOLS
    assert rt.lib().svo_version() == 7  # new entry points are detected by symbol, not by version


def test_header_declares_it(rt):
    h = _header()
    assert PROTOTYPE in h
    version = re.search(r"#define SVO_RT_VERSION 7.*?\*/", h, re.S).group(0)
    assert "detected by symbol" in version and NAME in version
    assert "strictly increasing in the point builder's key" in h  # the order is stated


def _origin(*v):
    return (C.c_int32 * 3)(*v)


X, I = C.c_void_p(0x1000), C.c_void_p(0x2000)  # never dereferenced by a failing call
# (origin, nx, ny, nz, xyz, ids, cap) on a tree of 2 levels (16^3)
EINVAL_CASES = {
    "xyz alone": (None, 0, 0, 0, X, None, 4),
    "ids alone": (None, 0, 0, 0, None, I, 4),
    "xyz alone, cap 0": (None, 0, 0, 0, X, None, 0),
    "no buffers, cap > 0": (None, 0, 0, 0, None, None, 4),
    "cap negative": (None, 0, 0, 0, X, I, -1),
    "cap negative, no buffers": (None, 0, 0, 0, None, None, -1),
    "nx 0": ((0, 0, 0), 0, 4, 4, X, I, 4),
    "ny negative": ((0, 0, 0), 4, -4, 4, X, I, 4),
    "nz 0, count only": ((0, 0, 0), 4, 4, 0, None, None, 0),
    "origin negative": ((-1, 0, 0), 4, 4, 4, X, I, 4),
    "x leaves the extent": ((13, 0, 0), 4, 4, 4, X, I, 4),
    "y leaves the extent": ((0, 16, 0), 1, 1, 1, X, I, 4),
    "z leaves the extent": ((0, 0, 1), 16, 16, 16, None, None, 0),
    "no wrap past 2^31": ((2147483647, 0, 0), 2147483647, 1, 1, X, I, 4),
}


@pytest.mark.parametrize("case", sorted(EINVAL_CASES))
def test_einval(rt, case):
    t = rt.World(2).build()
    o, nx, ny, nz, xyz, ids, cap = EINVAL_CASES[case]
    n = C.c_int64(-7)
    rc = rt.lib().svo_tree_list_voxels_gpu(t._h, _origin(*o) if o else None, nx, ny, nz, xyz, ids, cap, C.byref(n), None)
    msg = (rt.lib().svo_last_error() or b"").decode()
    assert rc == EINVAL and NAME in msg, (rc, msg)
    assert n.value == -7


def test_null_tree_and_null_count(rt):
    t = rt.World(2).build()
    f = rt.lib().svo_tree_list_voxels_gpu
    n = C.c_int64()
    assert f(None, None, 0, 0, 0, None, None, 0, C.byref(n), None) == EINVAL and NAME in rt.lib().svo_last_error().decode()
    assert f(t._h, None, 0, 0, 0, None, None, 0, None, None) == EINVAL and NAME in rt.lib().svo_last_error().decode()


def test_a_tree_that_is_not_uploaded(rt):
    t = rt.World(2).build()
    n = C.c_int64(-7)
    for args in ((None, 0, 0, 0, None, None, 0), (_origin(1, 2, 3), 4, 5, 6, X, I, 100)):
        assert rt.lib().svo_tree_list_voxels_gpu(t._h, *args, C.byref(n), None) == ESTATE
        msg = rt.lib().svo_last_error().decode()
        assert NAME in msg and "not uploaded" in msg
    with pytest.raises(rt.SvoError, match=r"svo_tree_list_voxels_gpu failed \(-4\): tree not uploaded"):
        t.count_voxels()
    with pytest.raises(rt.SvoError, match=r"svo_tree_list_voxels_gpu failed \(-4\): tree not uploaded"):
        t.list_voxels((0, 0, 0), (4, 4, 4))
