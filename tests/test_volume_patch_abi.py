"""svo_tree_patch_volume_gpu / svo_tree_garbage without a device: the library exports them and include/svo_rt.h declares
them, and every argument error is reported by its own code, with a message in svo_last_error that names the function,
before the first HIP call — never SVO_EDEVICE, although this machine may have no GPU."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, EDEVICE, ESTATE = -1, -3, -4


def _box(rt, n=(8, 8, 8), origin=(4, 0, 50), voxels=0x1000):
    """a valid box of a 3-level world but for the arguments; the voxel pointer is never dereferenced by a failing call"""
    b = rt.VolumeBox()
    b.nx, b.ny, b.nz = n
    b.origin[:] = origin
    b.voxels = voxels
    return b


def _patch(rt, tree, box):
    assert hasattr(rt.lib(), "svo_tree_patch_volume_gpu")
    rc = rt.lib().svo_tree_patch_volume_gpu(tree, C.byref(box) if box is not None else None)
    return rc, (rt.lib().svo_last_error() or b"").decode()


@pytest.fixture(scope="module")
def host_tree(rt):
    w = rt.World(3)
    w.put_block(1, 2, 3, 0, 5)
    return w.build()


def test_library_exports_and_header_declares_both(rt):
    L = C.CDLL(rt.LIB_PATH)
    hdr = open(os.path.join(ROOT, "include", "svo_rt.h")).read()
    for s in ("svo_tree_patch_volume_gpu", "svo_tree_garbage"):
        assert hasattr(L, s), s
        assert s in rt.ABI_SYMBOLS
        assert re.search(r"^int %s\(" % s, hdr, re.M), s
    assert "svo_volume_box" in hdr
    assert rt.lib().svo_version() == 7  # detected by symbol, not by version
    assert "rebuilt from a new volume, not patched" not in hdr


EINVAL_CASES = {
    "null voxels": dict(voxels=None),
    "nx 0": dict(n=(0, 8, 8)),
    "ny negative": dict(n=(8, -2, 8)),
    "nz 0": dict(n=(8, 8, 0)),
    "negative origin": dict(origin=(-1, 0, 0)),
    "box past +x": dict(origin=(57, 0, 0)),
    "box past +y": dict(origin=(0, 57, 0)),
    "box past +z": dict(origin=(0, 0, 57)),
    "box far past (no int32 wrap)": dict(origin=(0x7FFFFFFF, 0, 0)),
}


@pytest.mark.parametrize("case", sorted(EINVAL_CASES))
def test_einval(rt, host_tree, case):
    rc, msg = _patch(rt, host_tree._h, _box(rt, **EINVAL_CASES[case]))
    assert rc == EINVAL and "svo_tree_patch_volume_gpu" in msg, (rc, msg)


def test_null_tree_and_null_box(rt, host_tree):
    rc, msg = _patch(rt, None, _box(rt))
    assert rc == EINVAL and "svo_tree_patch_volume_gpu" in msg
    rc, msg = _patch(rt, host_tree._h, None)
    assert rc == EINVAL and "svo_tree_patch_volume_gpu" in msg


def test_a_tree_never_uploaded_is_estate(rt, host_tree):
    """also the largest legal box: it passes the argument checks, and the state check comes before any HIP call"""
    for b in (_box(rt), _box(rt, n=(64, 64, 64), origin=(0, 0, 0))):
        rc, msg = _patch(rt, host_tree._h, b)
        assert rc == ESTATE and "svo_tree_patch_volume_gpu" in msg and "not uploaded" in msg, (rc, msg)
    with pytest.raises(rt.SvoError, match="not uploaded"):
        host_tree.patch_volume([[[0]]], (0, 0, 0))


def test_garbage_of_a_fresh_host_build(rt, host_tree):
    assert host_tree.garbage() == (0, 0)
    n = C.c_uint64(7)
    assert rt.lib().svo_tree_garbage(host_tree._h, C.byref(n), None) == 0 and n.value == 0  # either pointer may be NULL
    assert rt.lib().svo_tree_garbage(host_tree._h, None, None) == 0
    assert rt.lib().svo_tree_garbage(None, C.byref(n), None) == EINVAL
    assert b"svo_tree_garbage" in rt.lib().svo_last_error()


def test_garbage_counts_host_edits(rt):
    """svo_tree_update's superseded child blocks show in the same counter"""
    w = rt.World(3)
    w.put_block(1, 2, 3, 0, 5)
    w.put_block(40, 2, 3, 0, 5)
    t = w.build()
    w.put_block(2, 2, 3, 0, 6)
    t.update(w, [(2, 2, 3)])
    assert t.garbage()[0] > 0
