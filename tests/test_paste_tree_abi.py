"""svo_tree_patch_tree_gpu without a device: the library exports it and include/svo_rt.h declares it with its two flag
values, and every argument and state error is reported by its own code, with a message in svo_last_error that names the
function, before the first HIP call — never SVO_EDEVICE, although this machine may have no GPU.  The trees are host-built
and never uploaded: the argument checks come before the state check, and both trees are unchanged afterwards."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, EDEVICE, ESTATE, ERANGE = -1, -3, -4, -5
WHOLE = object()


def _paste(rt, dst, src, src_origin, dims, dst_origin, flags=0):
    assert hasattr(rt.lib(), "svo_tree_patch_tree_gpu")
    so = None if src_origin is None else (C.c_int32 * 3)(*src_origin)
    do = None if dst_origin is None else (C.c_int32 * 3)(*dst_origin)
    rc = rt.lib().svo_tree_patch_tree_gpu(dst, src, so, dims[0], dims[1], dims[2], do, flags)
    return rc, (rt.lib().svo_last_error() or b"").decode()


def _world_tree(rt, levels, n_colours):
    w = rt.World(levels)
    for i in range(n_colours):
        w.put_block(1 + i % 2, 2, 3 - i % 3, 0, 5 + i)
    return w.build()


@pytest.fixture(scope="module")
def dst3(rt):
    return _world_tree(rt, 3, 2)


@pytest.fixture(scope="module")
def src2(rt):
    return _world_tree(rt, 2, 1)


def _image(t):
    n, m = t.export()
    return n.tobytes(), m.tobytes(), t.garbage(), t.info().n_nodes


def test_library_exports_and_header_declares_it(rt):
    L = C.CDLL(rt.LIB_PATH)
    hdr = open(os.path.join(ROOT, "include", "svo_rt.h")).read()
    assert hasattr(L, "svo_tree_patch_tree_gpu")
    assert "svo_tree_patch_tree_gpu" in rt.ABI_SYMBOLS
    assert re.search(r"^int svo_tree_patch_tree_gpu\(svo_tree\* dst, const svo_tree\* src,\s*const int32_t src_origin\[3\], int32_t nx, "
                     r"int32_t ny, int32_t nz,\s*const int32_t dst_origin\[3\], uint32_t flags\);", hdr, re.M)
    assert re.search(r"^#define SVO_PASTE_REPLACE 0\b", hdr, re.M) and re.search(r"^#define SVO_PASTE_KEEP_EMPTY 1\b", hdr, re.M)
    assert rt.lib().svo_version() == 7  # detected by symbol, not by version
    assert re.search(r"^#define SVO_RT_VERSION 7\b", hdr, re.M)
    listed = hdr[hdr.index("detected by symbol"):hdr.index("enum {")]
    assert "svo_tree_patch_tree_gpu" in listed
    assert hasattr(rt.Tree, "patch_tree") and (rt.PASTE_REPLACE, rt.PASTE_KEEP_EMPTY) == (0, 1)
    # the header comment: the content rule, the modes, self-paste, the conservative answer and the restart
    comment = hdr[hdr.index("/* Paste a box of one resident tree"):hdr.index("#define SVO_PASTE_REPLACE")]
    for word in ("KEEP_EMPTY", "src == dst", "conservative", "restarts the arrays", "SVO_ERANGE", "svo_tree_patch_times", "2 x 2 x 2"):
        assert word in comment, word


EINVAL_CASES = {
    "nx 0": ((0, 0, 0), (0, 4, 4), (0, 0, 0), 0),
    "ny negative": ((0, 0, 0), (4, -1, 4), (0, 0, 0), 0),
    "nz 0": ((0, 0, 0), (4, 4, 0), (0, 0, 0), 1),
    "src box negative origin": ((0, -1, 0), (4, 4, 4), (0, 0, 0), 0),
    "src box past +x": ((13, 0, 0), (4, 4, 4), (0, 0, 0), 0),
    "src box past +z": ((0, 0, 16), (1, 1, 1), (0, 0, 0), 0),
    "src box far past (no int32 wrap)": ((0x7FFFFFFF, 0, 0), (0x7FFFFFFF, 1, 1), (0, 0, 0), 0),
    "dst box negative origin": ((0, 0, 0), (4, 4, 4), (0, 0, -3), 0),
    "dst box past +y": ((0, 0, 0), (4, 4, 4), (0, 61, 0), 0),
    "dst box far past (no int32 wrap)": ((0, 0, 0), (4, 4, 4), (0x7FFFFFFF, 0, 0), 0),
    "the whole of src past dst's +x": (None, (0, 0, 0), (49, 0, 0), 0),
    "flag bit 1": ((0, 0, 0), (4, 4, 4), (0, 0, 0), 2),
    "flag bit 31": ((0, 0, 0), (4, 4, 4), (0, 0, 0), 0x80000001),
}


@pytest.mark.parametrize("case", sorted(EINVAL_CASES))
def test_einval(rt, dst3, src2, case):
    before = _image(dst3), _image(src2)
    so, dims, do, flags = EINVAL_CASES[case]
    rc, msg = _paste(rt, dst3._h, src2._h, so, dims, do, flags)
    assert rc == EINVAL and "svo_tree_patch_tree_gpu" in msg, (rc, msg)
    assert (_image(dst3), _image(src2)) == before


def test_null_arguments(rt, dst3, src2):
    for dst, src, do in ((None, src2._h, (0, 0, 0)), (dst3._h, None, (0, 0, 0)), (dst3._h, src2._h, None)):
        rc, msg = _paste(rt, dst, src, (0, 0, 0), (4, 4, 4), do)
        assert rc == EINVAL and "svo_tree_patch_tree_gpu" in msg and "NULL" in msg, (rc, msg)


def test_a_dst_of_one_level_is_erange(rt, src2):
    one = _world_tree(rt, 1, 1)
    assert one.info().levels == 1
    rc, msg = _paste(rt, one._h, one._h, None, (0, 0, 0), (0, 0, 0))
    assert rc == ERANGE and "svo_tree_patch_tree_gpu" in msg and "levels" in msg, (rc, msg)
    rc, msg = _paste(rt, one._h, src2._h, (0, 0, 0), (4, 4, 4), (0, 0, 0))
    assert rc == ERANGE, (rc, msg)


def test_a_src_palette_larger_than_dsts_is_erange(rt, dst3):
    """ids are numbers in dst's palette: with more entries in src's, one of them could be out of range on the device"""
    big = _world_tree(rt, 2, 3)
    assert big.info().n_materials == 4 and dst3.info().n_materials == 3
    before = _image(dst3), _image(big)
    rc, msg = _paste(rt, dst3._h, big._h, None, (0, 0, 0), (5, 6, 7))
    assert rc == ERANGE and "svo_tree_patch_tree_gpu" in msg and "palette" in msg, (rc, msg)
    assert (_image(dst3), _image(big)) == before
    rc, msg = _paste(rt, big._h, dst3._h, (0, 0, 0), (16, 16, 16), (0, 0, 0))   # the other way round it passes the argument checks
    assert rc == ESTATE, (rc, msg)


def test_trees_never_uploaded_are_estate(rt, dst3, src2):
    """the state check comes before any HIP call, for every valid combination of arguments"""
    before = _image(dst3), _image(src2)
    calls = ((None, (0, 0, 0), (0, 0, 0), 0), (None, (-1, -1, -1), (48, 48, 48), 1), ((3, 2, 1), (9, 10, 11), (30, 31, 29), 0),
             ((15, 15, 15), (1, 1, 1), (63, 63, 63), 1))
    for so, dims, do, flags in calls:
        rc, msg = _paste(rt, dst3._h, src2._h, so, dims, do, flags)
        assert rc == ESTATE and "svo_tree_patch_tree_gpu" in msg and "not uploaded" in msg, (rc, msg)
    rc, msg = _paste(rt, dst3._h, dst3._h, None, (0, 0, 0), (0, 0, 0))           # src == dst
    assert rc == ESTATE, (rc, msg)
    with pytest.raises(rt.SvoError, match=r"svo_tree_patch_tree_gpu failed \(-4\).*not uploaded"):
        dst3.patch_tree(src2, None, None, (1, 2, 3))
    with pytest.raises(ValueError):
        dst3.patch_tree("a tree", None, None, (1, 2, 3))
    assert (_image(dst3), _image(src2)) == before
