"""svo_tree_compact_gpu without a device: the library exports it and include/svo_rt.h declares it, and its argument and
state errors are reported by their own codes, with a message in svo_last_error that names the function, before the first
HIP call — never SVO_EDEVICE, although this machine may have no GPU."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, EDEVICE, ESTATE = -1, -3, -4


def _compact(rt, tree):
    assert hasattr(rt.lib(), "svo_tree_compact_gpu")
    rc = rt.lib().svo_tree_compact_gpu(tree)
    return rc, (rt.lib().svo_last_error() or b"").decode()


@pytest.fixture(scope="module")
def host_tree(rt):
    w = rt.World(3)
    w.put_block(1, 2, 3, 0, 5)
    return w.build()


def test_library_exports_and_header_declares_it(rt):
    assert hasattr(rt.lib(), "svo_tree_compact_gpu")
    L = C.CDLL(rt.LIB_PATH)
    hdr = open(os.path.join(ROOT, "include", "svo_rt.h")).read()
    for s in ("svo_tree_compact_gpu", "svo_tree_compact_times"):
        assert hasattr(L, s), s
        assert s in rt.ABI_SYMBOLS
        assert re.search(r"^int %s\(" % s, hdr, re.M), s
    assert rt.lib().svo_version() == 7  # detected by symbol, not by version
    assert "svo_tree_read_volume + svo_build_volume_gpu, pays" not in hdr  # the patch's note points at the new call
    assert hasattr(rt.Tree, "compact")


def test_null_tree_is_einval(rt):
    rc, msg = _compact(rt, None)
    assert rc == EINVAL and "svo_tree_compact_gpu" in msg, (rc, msg)


def test_a_tree_never_uploaded_is_estate(rt, host_tree):
    before = [a.tobytes() for a in host_tree.export()]
    rc, msg = _compact(rt, host_tree._h)
    assert rc == ESTATE and "svo_tree_compact_gpu" in msg and "not uploaded" in msg, (rc, msg)
    with pytest.raises(rt.SvoError, match=r"\(-4\).*not uploaded"):
        host_tree.compact()
    assert [a.tobytes() for a in host_tree.export()] == before


def test_a_host_edited_tree_never_uploaded_is_estate(rt):
    """the state check does not depend on what the tree holds: one that carries garbage from svo_tree_update is refused alike"""
    w = rt.World(3)
    w.put_block(1, 2, 3, 0, 5)
    w.put_block(40, 2, 3, 0, 5)
    t = w.build()
    w.put_block(2, 2, 3, 0, 6)
    t.update(w, [(2, 2, 3)])
    g = t.garbage()
    assert g[0] > 0
    rc, msg = _compact(rt, t._h)
    assert rc == ESTATE and "svo_tree_compact_gpu" in msg, (rc, msg)
    assert t.garbage() == g


def test_compact_times_arguments(rt, host_tree):
    ms = (C.c_double * 3)(7.0, 7.0, 7.0)
    assert rt.lib().svo_tree_compact_times(host_tree._h, ms) == 0 and tuple(ms) == (0.0, 0.0, 0.0)
    assert rt.lib().svo_tree_compact_times(None, ms) == EINVAL
    assert b"svo_tree_compact_times" in rt.lib().svo_last_error()
    assert rt.lib().svo_tree_compact_times(host_tree._h, None) == EINVAL
