"""svo_tree_patch_tree_rule_gpu without a device: the library exports it, include/svo_rt.h declares it with its macros
(whose values are the package's constants), and every argument and state error is reported by its own code, with a message
in svo_last_error that names the function, before the first HIP call — never SVO_EDEVICE, although this machine may have
no GPU.  The trees are host-built and never uploaded: the argument checks come before the state check, and both trees are
unchanged afterwards."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, EDEVICE, ESTATE, ERANGE = -1, -3, -4, -5
NAME = "svo_tree_patch_tree_rule_gpu"


def _paste(rt, dst, src, rule=1, src_origin=(0, 0, 0), dims=(4, 4, 4), dst_origin=(0, 0, 0), flags=0, axis=(0, 1, 2), flip=(0, 0, 0), id_map=None,
           null=False):
    assert hasattr(rt.lib(), NAME)
    p = rt.Paste()
    p.src_origin[:], p.n[:], p.dst_origin[:], p.flags = src_origin, dims, dst_origin, flags
    p.axis[:], p.flip[:] = axis, flip
    table = None
    if id_map is not None:
        table = (C.c_uint16 * len(id_map))(*id_map)
        p.id_map = C.cast(table, C.POINTER(C.c_uint16))
    rc = getattr(rt.lib(), NAME)(dst, src, None if null else C.byref(p), rule)
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
    assert hasattr(L, NAME) and NAME in rt.ABI_SYMBOLS
    assert re.search(r"^int svo_tree_patch_tree_rule_gpu\(svo_tree\* dst, const svo_tree\* src, const svo_paste\* p, uint32_t rule\);", hdr, re.M)
    assert rt.lib().svo_version() == 7  # detected by symbol, not by version
    listed = hdr[hdr.index("detected by symbol"):hdr.index("enum {")]
    assert NAME in listed
    assert hasattr(rt.Tree, "patch_tree_rule")
    assert hdr.index("int svo_tree_patch_tree_oriented_gpu(") < hdr.index("int svo_tree_patch_tree_rule_gpu(") < hdr.index("int svo_tree_garbage(")
    # the macros are the package's constants
    macros = dict(re.findall(r"^#define (SVO_RULE_\w+) (\d+)u\b", hdr, re.M))
    assert {k: int(v) for k, v in macros.items()} == {
        "SVO_RULE_KEEP": rt.RULE_KEEP, "SVO_RULE_TAKE": rt.RULE_TAKE, "SVO_RULE_CLEAR": rt.RULE_CLEAR, "SVO_RULE_UNDER": rt.RULE_UNDER,
        "SVO_RULE_PAINT": rt.RULE_PAINT, "SVO_RULE_OVER": rt.RULE_OVER, "SVO_RULE_ERASE": rt.RULE_ERASE, "SVO_RULE_XOR": rt.RULE_XOR,
        "SVO_RULE_MASK": rt.RULE_MASK, "SVO_RULE_STENCIL": rt.RULE_STENCIL, "SVO_RULE_REPLACE": rt.RULE_REPLACE}
    assert (rt.RULE_KEEP, rt.RULE_TAKE, rt.RULE_CLEAR) == (0, 1, 2)
    assert [rt.RULE_UNDER, rt.RULE_PAINT, rt.RULE_OVER, rt.RULE_ERASE, rt.RULE_XOR, rt.RULE_MASK, rt.RULE_STENCIL, rt.RULE_REPLACE] == \
        [1, 4, 5, 8, 9, 32, 36, 37]
    assert re.search(r"^#define SVO_RULE\(a, b, c\) \(\(uint32_t\)\(a\) \| \(uint32_t\)\(b\) << 2 \| \(uint32_t\)\(c\) << 4\)", hdr, re.M)
    assert rt.paste_rule(rt.RULE_TAKE, rt.RULE_CLEAR, rt.RULE_KEEP) == rt.RULE_XOR and rt.paste_rule(1, 1, 2) == rt.RULE_REPLACE
    # the header comment: the table, d in dst's own view and what follows from it, no restart, what is still not done
    comment = " ".join(hdr[hdr.index("/* The oriented paste under a rule"):hdr.index("#define SVO_RULE_KEEP")].split())
    for word in ("IN DST'S OWN VIEW", "does NOT leave them the two views", "never restarts the arrays", "p->flags must be 0", "src == dst",
                 "svo_tree_patch_times", "Rule 0", "SVO_EINVAL", "lists of placements", "palette growth"):
        assert word in comment, word


EINVAL_CASES = {
    "flags 1": dict(flags=1),
    "flags 1 with rule 0": dict(flags=1, rule=0),
    "A is CLEAR": dict(rule=2),
    "A is 3": dict(rule=3),
    "B is 3": dict(rule=3 << 2),
    "C is TAKE": dict(rule=1 << 4),
    "C is 3": dict(rule=3 << 4),
    "bit 6": dict(rule=1 | 1 << 6),
    "bit 6 alone": dict(rule=1 << 6),
    "bit 31": dict(rule=5 | 1 << 31),
    "nx 0": dict(dims=(0, 4, 4)),
    "ny negative": dict(dims=(4, -1, 4), rule=0),
    "src box past +x": dict(src_origin=(13, 0, 0)),
    "src box far past (no int32 wrap)": dict(src_origin=(0x7FFFFFFF, 0, 0), dims=(0x7FFFFFFF, 1, 1)),
    "dst box past +y": dict(dst_origin=(0, 61, 0)),
    "dst box far past (no int32 wrap)": dict(dst_origin=(0x7FFFFFFF, 0, 0)),
    "dst box past +x only because the dimensions are permuted": dict(dims=(2, 16, 2), dst_origin=(50, 0, 0), axis=(1, 0, 2)),
    "axis repeats": dict(axis=(0, 0, 2)),
    "axis entry 3": dict(axis=(0, 1, 3)),
    "flip entry 2": dict(flip=(0, 2, 0)),
    "id_map[0] not 0": dict(id_map=(1, 1)),
}


@pytest.mark.parametrize("case", sorted(EINVAL_CASES))
def test_einval(rt, dst3, src2, case):
    before = _image(dst3), _image(src2)
    rc, msg = _paste(rt, dst3._h, src2._h, **EINVAL_CASES[case])
    assert rc == EINVAL and NAME in msg, (rc, msg)
    assert (_image(dst3), _image(src2)) == before


def test_null_arguments(rt, dst3, src2):
    for dst, src, null in ((None, src2._h, False), (dst3._h, None, False), (dst3._h, src2._h, True)):
        rc, msg = _paste(rt, dst, src, null=null)
        assert rc == EINVAL and NAME in msg and "NULL" in msg, (rc, msg)


def test_erange(rt, dst3, src2):
    one = _world_tree(rt, 1, 1)
    assert one.info().levels == 1
    rc, msg = _paste(rt, one._h, src2._h, rule=rt.RULE_ERASE)
    assert rc == ERANGE and NAME in msg and "levels" in msg, (rc, msg)
    big = _world_tree(rt, 2, 3)
    assert big.info().n_materials == 4 and dst3.info().n_materials == 3
    before = _image(dst3), _image(big)
    rc, msg = _paste(rt, dst3._h, big._h, rule=rt.RULE_UNDER, dst_origin=(5, 6, 7))       # no map and a larger src palette
    assert rc == ERANGE and NAME in msg and "palette" in msg, (rc, msg)
    rc, msg = _paste(rt, dst3._h, big._h, rule=rt.RULE_PAINT, id_map=(0, 2, 3, 65535))    # a map entry past dst's palette
    assert rc == ERANGE and NAME in msg and "id_map[2]" in msg, (rc, msg)
    rc, msg = _paste(rt, dst3._h, big._h, rule=2, id_map=(0, 2, 3, 65535))                # arguments first
    assert rc == EINVAL, (rc, msg)
    rc, msg = _paste(rt, dst3._h, big._h, rule=rt.RULE_MASK, dst_origin=(5, 6, 7), id_map=(0, 2, 1, 2))   # with a map it reaches the state check
    assert rc == ESTATE and NAME in msg and "not uploaded" in msg, (rc, msg)
    assert (_image(dst3), _image(big)) == before


def test_trees_never_uploaded_are_estate(rt, dst3, src2):
    """the state check comes after the arguments and before any HIP call, for every valid rule — rule 0 included"""
    before = _image(dst3), _image(src2)
    rules = [rt.paste_rule(a, b, c) for c in (0, 2) for b in (0, 1, 2) for a in (0, 1)]
    assert len(rules) == 12 and 0 in rules
    for rule in rules:
        rc, msg = _paste(rt, dst3._h, src2._h, rule=rule, src_origin=(3, 2, 1), dims=(9, 10, 11), dst_origin=(30, 31, 29), axis=(2, 1, 0), flip=(0, 0, 1),
                         id_map=(0, 2))
        assert rc == ESTATE and NAME in msg and "not uploaded" in msg, (rule, rc, msg)
    rc, msg = _paste(rt, dst3._h, dst3._h, rule=rt.RULE_XOR, dims=(64, 64, 64), axis=(1, 0, 2), flip=(1, 0, 0))           # src == dst
    assert rc == ESTATE, (rc, msg)
    with pytest.raises(rt.SvoError, match=r"svo_tree_patch_tree_rule_gpu failed \(-4\).*not uploaded"):
        dst3.patch_tree_rule(src2, None, None, (1, 2, 3), rt.RULE_UNDER, axis=(2, 1, 0), flip=(0, 0, 1))
    with pytest.raises(ValueError):
        dst3.patch_tree_rule("a tree", None, None, (1, 2, 3), rt.RULE_UNDER)
    assert (_image(dst3), _image(src2)) == before
