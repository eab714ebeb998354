"""svo_tree_patch_points_gpu without a device: the library exports it and include/svo_rt.h declares it, and every argument
error is reported by its own code, with a message in svo_last_error that names the function, before the first HIP call —
never SVO_EDEVICE, although this machine may have no GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, EDEVICE, ESTATE, ERANGE = -1, -3, -4, -5
PTR = 0x1000  # a non-NULL buffer address: a failing call never dereferences it


def _patch(rt, tree, xyz, ids, n):
    assert hasattr(rt.lib(), "svo_tree_patch_points_gpu")
    rc = rt.lib().svo_tree_patch_points_gpu(tree, xyz, ids, n)
    return rc, (rt.lib().svo_last_error() or b"").decode()


@pytest.fixture(scope="module")
def host_tree(rt):
    w = rt.World(3)
    w.put_block(1, 2, 3, 0, 5)
    return w.build()


def test_library_exports_and_header_declares_it(rt):
    L = C.CDLL(rt.LIB_PATH)
    hdr = open(os.path.join(ROOT, "include", "svo_rt.h")).read()
    assert hasattr(L, "svo_tree_patch_points_gpu")
    assert "svo_tree_patch_points_gpu" in rt.ABI_SYMBOLS
    assert re.search(r"^int svo_tree_patch_points_gpu\(svo_tree\* t, const int32_t\* xyz, const uint16_t\* ids, int64_t n\);", hdr, re.M)
    assert rt.lib().svo_version() == 7  # detected by symbol, not by version
    listed = hdr[hdr.index("detected by symbol"):hdr.index("enum {")]
    assert "svo_tree_patch_points_gpu" in listed
    assert hasattr(rt.Tree, "patch_points")


def test_null_tree(rt):
    rc, msg = _patch(rt, None, PTR, PTR, 1)
    assert rc == EINVAL and "svo_tree_patch_points_gpu" in msg, (rc, msg)


def test_negative_n(rt, host_tree):
    rc, msg = _patch(rt, host_tree._h, PTR, PTR, -1)
    assert rc == EINVAL and "svo_tree_patch_points_gpu" in msg, (rc, msg)


@pytest.mark.parametrize("xyz,ids", [(None, PTR), (PTR, None), (None, None)])
def test_null_buffers_with_points(rt, host_tree, xyz, ids):
    rc, msg = _patch(rt, host_tree._h, xyz, ids, 3)
    assert rc == EINVAL and "svo_tree_patch_points_gpu" in msg, (rc, msg)


def test_two_to_the_31_points_is_erange(rt, host_tree):
    rc, msg = _patch(rt, host_tree._h, PTR, PTR, 1 << 31)
    assert rc == ERANGE and "svo_tree_patch_points_gpu" in msg and "2^31" in msg, (rc, msg)


def test_a_tree_never_uploaded_is_estate(rt, host_tree):
    """the state check comes before any HIP call, for a list and for an empty one"""
    for n in (1, (1 << 31) - 1, 0):
        rc, msg = _patch(rt, host_tree._h, PTR, PTR, n)
        assert rc == ESTATE and "svo_tree_patch_points_gpu" in msg and "not uploaded" in msg, (n, rc, msg)
    with pytest.raises(rt.SvoError, match=r"svo_tree_patch_points_gpu failed \(-4\).*not uploaded"):
        host_tree.patch_points(np.zeros((1, 3), np.int32), np.ones(1, np.uint16))
    assert host_tree.garbage() == (0, 0)
