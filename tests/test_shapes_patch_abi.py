"""svo_tree_patch_shapes_gpu without a device: the library exports it and include/svo_rt.h declares it, svo_shape has the
layout of its ctypes mirror, and every argument error is reported by its own code, with a message in svo_last_error that
names the function, before the first HIP call — never SVO_EDEVICE, although this machine may have no GPU.  The trees are
host-built and never uploaded: the argument checks come before the state check."""
import ctypes as C
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, EDEVICE, ESTATE, ERANGE = -1, -3, -4, -5


def _patch(rt, tree, shapes, n=None):
    assert hasattr(rt.lib(), "svo_tree_patch_shapes_gpu")
    arr = (rt.Shape * max(1, len(shapes)))(*shapes) if shapes is not None else None
    rc = rt.lib().svo_tree_patch_shapes_gpu(tree, arr, len(shapes) if n is None else n)
    return rc, (rt.lib().svo_last_error() or b"").decode()


@pytest.fixture(scope="module")
def host_tree(rt):
    w = rt.World(3)
    w.put_block(1, 2, 3, 0, 5)
    return w.build()


def test_library_exports_and_header_declares_it(rt):
    L = C.CDLL(rt.LIB_PATH)
    hdr = open(os.path.join(ROOT, "include", "svo_rt.h")).read()
    assert hasattr(L, "svo_tree_patch_shapes_gpu")
    assert "svo_tree_patch_shapes_gpu" in rt.ABI_SYMBOLS
    assert re.search(r"^int svo_tree_patch_shapes_gpu\(svo_tree\* t, const svo_shape\* shapes /\* HOST \*/, int32_t n\);", hdr, re.M)
    assert re.search(r"^#define SVO_SHAPE_BOX 0\b", hdr, re.M) and re.search(r"^#define SVO_SHAPE_BALL 1\b", hdr, re.M)
    assert rt.lib().svo_version() == 7  # detected by symbol, not by version
    listed = hdr[hdr.index("detected by symbol"):hdr.index("enum {")]
    assert "svo_tree_patch_shapes_gpu" in listed
    assert hasattr(rt.Tree, "patch_shapes") and (rt.SHAPE_BOX, rt.SHAPE_BALL) == (0, 1)


def test_the_ctypes_mirror_has_the_documented_layout(rt):
    """kind, a[3], b[3]: seven int32; r2 aligned to 8; id behind it; the struct padded to a multiple of 8"""
    S = rt.Shape
    assert [(n, getattr(S, n).offset, getattr(S, n).size) for n, _ in S._fields_] == [
        ("kind", 0, 4), ("a", 4, 12), ("b", 16, 12), ("r2", 32, 8), ("id", 40, 2)]
    assert C.sizeof(S) == 48
    b = rt.box((1, 2, 3), (4, 5, 6), 7)
    assert (b.kind, list(b.a), list(b.b), b.id) == (0, [1, 2, 3], [4, 5, 6], 7)
    s = rt.ball((-1, 2, 3), 1 << 42, 65535)
    assert (s.kind, list(s.a), s.r2, s.id) == (1, [-1, 2, 3], 1 << 42, 65535)


@pytest.mark.skipif(shutil.which("gcc") is None, reason="no gcc")
def test_the_header_struct_has_the_mirrors_layout(rt, tmp_path):
    """svo_shape as a C compiler lays it out from include/svo_rt.h, against the ctypes mirror"""
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "svo_rt.h"\n'
                   'int main(void) { printf("%zu %zu %zu %zu %zu %zu\\n", sizeof(svo_shape), offsetof(svo_shape, kind), '
                   'offsetof(svo_shape, a), offsetof(svo_shape, b), offsetof(svo_shape, r2), offsetof(svo_shape, id)); return 0; }\n')
    exe = str(tmp_path / "layout")
    subprocess.run(["gcc", "-I" + os.path.join(ROOT, "include"), str(src), "-o", exe], check=True, timeout=120)
    got = [int(v) for v in subprocess.run([exe], capture_output=True, text=True, check=True, timeout=60).stdout.split()]
    S = rt.Shape
    assert got == [C.sizeof(S), S.kind.offset, S.a.offset, S.b.offset, S.r2.offset, S.id.offset]


def _kind(rt, k):
    s = rt.box((0, 0, 0), (4, 4, 4), 1)
    s.kind = k
    return s


EINVAL_CASES = {
    "unknown kind 2": lambda rt: [_kind(rt, 2)],
    "unknown kind -1": lambda rt: [_kind(rt, -1)],
    "box nx 0": lambda rt: [rt.box((0, 0, 0), (0, 4, 4), 1)],
    "box ny negative": lambda rt: [rt.box((0, 0, 0), (4, -2, 4), 1)],
    "box nz 0": lambda rt: [rt.box((0, 0, 0), (4, 4, 0), 1)],
    "box negative origin": lambda rt: [rt.box((-1, 0, 0), (4, 4, 4), 1)],
    "box past +x": lambda rt: [rt.box((61, 0, 0), (4, 4, 4), 1)],
    "box past +y": lambda rt: [rt.box((0, 1, 0), (4, 64, 4), 1)],
    "box past +z": lambda rt: [rt.box((0, 0, 64), (1, 1, 1), 1)],
    "box far past (no int32 wrap)": lambda rt: [rt.box((0x7FFFFFFF, 0, 0), (0x7FFFFFFF, 1, 1), 1)],
    "r2 negative": lambda rt: [rt.ball((5, 5, 5), -1, 1)],
    "a bad shape behind good ones": lambda rt: [rt.box((0, 0, 0), (64, 64, 64), 1), rt.ball((5, 5, 5), 9, 0), rt.ball((5, 5, 5), -9, 1)],
}

ERANGE_CASES = {
    "centre x past 2^20": lambda rt: [rt.ball(((1 << 20) + 1, 0, 0), 4, 1)],
    "centre z below -2^20": lambda rt: [rt.ball((0, 0, -(1 << 20) - 1), 4, 1)],
    "r2 past 2^42": lambda rt: [rt.ball((5, 5, 5), (1 << 42) + 1, 1)],
    "r2 the largest int64": lambda rt: [rt.ball((5, 5, 5), (1 << 63) - 1, 1)],
    "box id equal to the palette size": lambda rt: [rt.box((0, 0, 0), (4, 4, 4), 2)],
    "ball id 65535": lambda rt: [rt.ball((5, 5, 5), 4, 65535)],
    "a clipped-away ball's id is still checked": lambda rt: [rt.ball((-500, 5, 5), 4, 2)],
}


@pytest.mark.parametrize("case", sorted(EINVAL_CASES))
def test_einval(rt, host_tree, case):
    rc, msg = _patch(rt, host_tree._h, EINVAL_CASES[case](rt))
    assert rc == EINVAL and "svo_tree_patch_shapes_gpu" in msg, (rc, msg)
    if "behind" in case:
        assert "shape 2" in msg


@pytest.mark.parametrize("case", sorted(ERANGE_CASES))
def test_erange(rt, host_tree, case):
    assert host_tree.info().n_materials == 2
    rc, msg = _patch(rt, host_tree._h, ERANGE_CASES[case](rt))
    assert rc == ERANGE and "svo_tree_patch_shapes_gpu" in msg, (rc, msg)


def test_null_tree_null_shapes_and_negative_n(rt, host_tree):
    one = [rt.box((0, 0, 0), (4, 4, 4), 1)]
    rc, msg = _patch(rt, None, one)
    assert rc == EINVAL and "svo_tree_patch_shapes_gpu" in msg, (rc, msg)
    rc, msg = _patch(rt, host_tree._h, None, 3)
    assert rc == EINVAL and "svo_tree_patch_shapes_gpu" in msg, (rc, msg)
    rc, msg = _patch(rt, host_tree._h, one, -1)
    assert rc == EINVAL and "svo_tree_patch_shapes_gpu" in msg, (rc, msg)


def test_more_than_1024_shapes_is_erange(rt, host_tree):
    many = [rt.box((0, 0, 0), (4, 4, 4), 1)] * 1025
    rc, msg = _patch(rt, host_tree._h, many)
    assert rc == ERANGE and "svo_tree_patch_shapes_gpu" in msg and "1024" in msg, (rc, msg)
    rc, msg = _patch(rt, host_tree._h, many[:1024])   # 1024 pass the argument checks
    assert rc == ESTATE, (rc, msg)


def test_a_tree_of_one_level_is_erange(rt):
    w = rt.World(1)
    w.put_block(1, 2, 3, 0, 5)
    t = w.build()
    assert t.info().levels == 1
    rc, msg = _patch(rt, t._h, [rt.box((0, 0, 0), (4, 4, 4), 1)])
    assert rc == ERANGE and "svo_tree_patch_shapes_gpu" in msg and "levels" in msg, (rc, msg)


def test_a_tree_never_uploaded_is_estate(rt, host_tree):
    """the state check comes before any HIP call: for the limits of every argument, for an empty list, for a list clipped away"""
    lists = ([rt.box((0, 0, 0), (64, 64, 64), 1)], [rt.ball((1 << 20, -(1 << 20), 1 << 20), 1 << 42, 0)], [],
             [rt.ball((-500, 5, 5), 4, 1)])
    for shapes in lists:
        rc, msg = _patch(rt, host_tree._h, shapes)
        assert rc == ESTATE and "svo_tree_patch_shapes_gpu" in msg and "not uploaded" in msg, (rc, msg)
    rc, msg = _patch(rt, host_tree._h, None, 0)
    assert rc == ESTATE, (rc, msg)
    with pytest.raises(rt.SvoError, match=r"svo_tree_patch_shapes_gpu failed \(-4\).*not uploaded"):
        host_tree.patch_shapes([rt.box((0, 0, 0), (1, 1, 1), 1)])
    assert host_tree.garbage() == (0, 0)
