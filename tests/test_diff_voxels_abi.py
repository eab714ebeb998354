"""svo_tree_diff_gpu without a device: the library exports it, the header declares it with its documented prototype and
names it among the entry points detected by symbol, every argument error is SVO_EINVAL with the function's name in
svo_last_error() — reported on trees that are not uploaded, so before their state is looked at and before the first HIP
call, never SVO_EDEVICE, although this machine may have no GPU — and a tree that is not uploaded, on either side, is
SVO_ESTATE from C and SvoError from Tree.count_diff / Tree.diff_voxels (an uploaded a against a b that is not needs a
device: tests/test_gpu_diff_voxels.py)."""
import ctypes as C
import os
import re

import pytest

from test_list_voxels_abi import EINVAL_CASES as BOX_AND_BUFFER_CASES  # the listing's table: buffers, cap, bad boxes (2 levels)

EINVAL, ESTATE = -1, -4
NAME = "svo_tree_diff_gpu"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROTOTYPE = """int svo_tree_diff_gpu(const svo_tree* a, const svo_tree* b,
                      const int32_t origin[3], int32_t nx, int32_t ny, int32_t nz,
                      int32_t* xyz, uint16_t* ids, int64_t cap, int64_t* n, void* hip_stream);"""
X, I = C.c_void_p(0x1000), C.c_void_p(0x2000)  # never dereferenced by a failing call


def _header():
    with open(os.path.join(ROOT, "include", "svo_rt.h")) as f:
        return f.read()


def _origin(*v):
    return (C.c_int32 * 3)(*v)


def _message(rt):
    return (rt.lib().svo_last_error() or b"").decode()


def test_library_exports_the_symbol(rt):
    assert hasattr(C.CDLL(rt.LIB_PATH), NAME)
    assert NAME in rt.ABI_SYMBOLS
    assert rt.lib().svo_version() == 7  # new entry points are detected by symbol, not by version
    assert hasattr(rt.Tree, "diff_voxels") and hasattr(rt.Tree, "count_diff")


def test_header_declares_it(rt):
    h = _header()
    assert PROTOTYPE in h
    version = re.search(r"#define SVO_RT_VERSION 7.*?\*/", h, re.S).group(0)
    assert "detected by symbol" in version and NAME in version
    comment = h[:h.index(PROTOTYPE)].rsplit("/*", 1)[1]
    assert "palettes are NOT" in comment and "compared as numbers" in comment  # ids are numbers; palettes are not compared
    assert "strictly increasing" in comment


@pytest.mark.parametrize("case", sorted(BOX_AND_BUFFER_CASES))
def test_einval(rt, case):
    a, b = rt.World(2).build(), rt.World(2).build()  # not uploaded: arguments are checked before state
    o, nx, ny, nz, xyz, ids, cap = BOX_AND_BUFFER_CASES[case]
    n = C.c_int64(-7)
    rc = rt.lib().svo_tree_diff_gpu(a._h, b._h, _origin(*o) if o else None, nx, ny, nz, xyz, ids, cap, C.byref(n), None)
    msg = _message(rt)
    assert rc == EINVAL and NAME in msg, (rc, msg)
    assert n.value == -7


def test_nulls(rt):
    t = rt.World(2).build()
    f = rt.lib().svo_tree_diff_gpu
    n = C.c_int64(-7)
    for args in ((None, t._h), (t._h, None), (None, None)):
        assert f(*args, None, 0, 0, 0, None, None, 0, C.byref(n), None) == EINVAL and NAME in _message(rt)
        assert n.value == -7
    assert f(t._h, t._h, None, 0, 0, 0, None, None, 0, None, None) == EINVAL and NAME in _message(rt)


def test_levels_must_match(rt):
    a, b = rt.World(2).build(), rt.World(3).build()
    n = C.c_int64(-7)
    for pair in ((a, b), (b, a)):
        rc = rt.lib().svo_tree_diff_gpu(pair[0]._h, pair[1]._h, None, 0, 0, 0, None, None, 0, C.byref(n), None)
        msg = _message(rt)
        assert rc == EINVAL and NAME in msg and "levels" in msg, (rc, msg)
        assert n.value == -7
    with pytest.raises(rt.SvoError):
        a.count_diff(b)


def test_trees_that_are_not_uploaded(rt):
    a, b = rt.World(2).build(), rt.World(2).build()
    n = C.c_int64(-7)
    for args in ((None, 0, 0, 0, None, None, 0), (_origin(1, 2, 3), 4, 5, 6, X, I, 100)):
        assert rt.lib().svo_tree_diff_gpu(a._h, b._h, *args, C.byref(n), None) == ESTATE
        msg = _message(rt)
        assert NAME in msg and "tree a not uploaded" in msg
        assert rt.lib().svo_tree_diff_gpu(a._h, a._h, *args, C.byref(n), None) == ESTATE
        assert n.value == -7
    for call in (lambda: a.count_diff(b), lambda: a.diff_voxels(b, (0, 0, 0), (4, 4, 4)), lambda: a.count_diff(a)):
        with pytest.raises(rt.SvoError, match=r"svo_tree_diff_gpu failed \(-4\): tree a not uploaded"):
            call()
    with pytest.raises(ValueError, match="other"):
        a.count_diff(None)

