"""svo_tree_patch_tree_oriented_gpu without a device: the library exports it, include/svo_rt.h declares it with its struct
(whose layout the ctypes mirror matches), and every argument and state error is reported by its own code, with a message
in svo_last_error that names the function, before the first HIP call — never SVO_EDEVICE, although this machine may have
no GPU.  The trees are host-built and never uploaded: the argument checks come before the state check, and both trees are
unchanged afterwards."""
import ctypes as C
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, EDEVICE, ESTATE, ERANGE = -1, -3, -4, -5
NAME = "svo_tree_patch_tree_oriented_gpu"


def _paste(rt, dst, src, src_origin=(0, 0, 0), dims=(4, 4, 4), dst_origin=(0, 0, 0), flags=0, axis=(0, 1, 2), flip=(0, 0, 0), id_map=None,
           null=False):
    assert hasattr(rt.lib(), NAME)
    p = rt.Paste()
    p.src_origin[:], p.n[:], p.dst_origin[:], p.flags = src_origin, dims, dst_origin, flags
    p.axis[:], p.flip[:] = axis, flip
    table = None
    if id_map is not None:
        table = (C.c_uint16 * len(id_map))(*id_map)
        p.id_map = C.cast(table, C.POINTER(C.c_uint16))
    rc = getattr(rt.lib(), NAME)(dst, src, None if null else C.byref(p))
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
    assert re.search(r"^int svo_tree_patch_tree_oriented_gpu\(svo_tree\* dst, const svo_tree\* src, const svo_paste\* p\);", hdr, re.M)
    assert rt.lib().svo_version() == 7  # detected by symbol, not by version
    assert re.search(r"^#define SVO_RT_VERSION 7\b", hdr, re.M)
    listed = hdr[hdr.index("detected by symbol"):hdr.index("enum {")]
    assert NAME in listed
    assert hasattr(rt.Tree, "patch_tree_oriented")
    struct = hdr[hdr.index("typedef struct {\n    int32_t src_origin[3];"):hdr.index("} svo_paste;")]
    fields = re.findall(r"^\s+(?:const )?(\w+\*?) (\w+)(?:\[3\])?;", struct, re.M)
    assert fields == [("int32_t", "src_origin"), ("int32_t", "n"), ("int32_t", "dst_origin"), ("uint32_t", "flags"), ("uint8_t", "axis"),
                      ("uint8_t", "flip"), ("uint16_t*", "id_map")]
    assert [f[0] for f in rt.Paste._fields_] == [f[1] for f in fields]
    # the header comment: the content rule in full, the order of map, mode and view, and what is still not done
    comment = " ".join(hdr[hdr.index("/* The same paste turned"):hdr.index("typedef struct {\n    int32_t src_origin[3];")].split())
    for word in ("dn[a] = n[axis[a]]", "s[axis[a]] = src_origin[axis[a]] + (flip[a] ? n[axis[a]] - 1 - d[a] : d[a])", "48", "id_map[0] must be 0",
                 "KEEP_EMPTY", "src == dst", "restarts the arrays", "SVO_ERANGE", "svo_tree_patch_times", "2 x 2 x 2", "2 B per entry",
                 "lists of", "palette growth"):
        assert word in comment, word
    plain = " ".join(hdr[hdr.index("/* Paste a box of one resident tree"):hdr.index("#define SVO_PASTE_REPLACE")].split())
    assert NAME in plain and "lists of placements in one call" in plain and "rotation or mirroring" not in plain


@pytest.mark.skipif(shutil.which("gcc") is None, reason="no gcc")
def test_struct_layout_matches_the_ctypes_mirror(rt, tmp_path):
    """sizeof and every offsetof, as a C compiler lays svo_paste out"""
    src = tmp_path / "layout.c"
    names = [f[0] for f in rt.Paste._fields_]
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "svo_rt.h"\nint main(void) {\n    printf("%zu", sizeof(svo_paste));\n' +
                   "".join('    printf(" %%zu", offsetof(svo_paste, %s));\n' % n for n in names) + "    return 0;\n}\n")
    exe = str(tmp_path / "layout")
    subprocess.run(["gcc", "-I" + os.path.join(ROOT, "include"), str(src), "-o", exe], check=True, capture_output=True)
    got = [int(v) for v in subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split()]
    assert got == [C.sizeof(rt.Paste)] + [getattr(rt.Paste, n).offset for n in names]


EINVAL_CASES = {
    "nx 0": dict(dims=(0, 4, 4)),
    "ny negative": dict(dims=(4, -1, 4)),
    "nz 0": dict(dims=(4, 4, 0), flags=1),
    "src box negative origin": dict(src_origin=(0, -1, 0)),
    "src box past +x": dict(src_origin=(13, 0, 0)),
    "src box past +z": dict(src_origin=(0, 0, 16), dims=(1, 1, 1)),
    "src box far past (no int32 wrap)": dict(src_origin=(0x7FFFFFFF, 0, 0), dims=(0x7FFFFFFF, 1, 1)),
    "dst box negative origin": dict(dst_origin=(0, 0, -3)),
    "dst box past +y": dict(dst_origin=(0, 61, 0)),
    "dst box far past (no int32 wrap)": dict(dst_origin=(0x7FFFFFFF, 0, 0)),
    "the whole of src past dst's +x": dict(dims=(16, 16, 16), dst_origin=(49, 0, 0)),
    "dst box past +x only because the dimensions are permuted": dict(dims=(2, 16, 2), dst_origin=(50, 0, 0), axis=(1, 0, 2)),
    "flag bit 1": dict(flags=2),
    "flag bit 31": dict(flags=0x80000001),
    "axis repeats": dict(axis=(0, 0, 2)),
    "axis entry 3": dict(axis=(0, 1, 3)),
    "axis entry 255": dict(axis=(255, 1, 2)),
    "flip entry 2": dict(flip=(0, 2, 0)),
    "flip entry 255": dict(flip=(0, 0, 255)),
    "id_map[0] not 0": dict(id_map=(1, 1)),
}


@pytest.mark.parametrize("case", sorted(EINVAL_CASES))
def test_einval(rt, dst3, src2, case):
    before = _image(dst3), _image(src2)
    rc, msg = _paste(rt, dst3._h, src2._h, **EINVAL_CASES[case])
    assert rc == EINVAL and NAME in msg, (rc, msg)
    assert (_image(dst3), _image(src2)) == before


def test_the_permuted_dimensions_decide_the_destination_box(rt, dst3, src2):
    """(2, 16, 2) at x = 50: it fits as it is and with y and z exchanged, and leaves the extent with x and y exchanged"""
    for axis in ((0, 1, 2), (0, 2, 1)):
        rc, msg = _paste(rt, dst3._h, src2._h, dims=(2, 16, 2), dst_origin=(50, 0, 0), axis=axis)
        assert rc == ESTATE, (rc, msg)
    rc, msg = _paste(rt, dst3._h, src2._h, dims=(2, 16, 2), dst_origin=(50, 0, 0), axis=(1, 0, 2))
    assert rc == EINVAL and "destination box" in msg, (rc, msg)
    rc, msg = _paste(rt, dst3._h, src2._h, dims=(16, 2, 2), dst_origin=(50, 0, 0), axis=(1, 0, 2), flip=(1, 1, 0))   # dn = (2, 16, 2)
    assert rc == ESTATE, (rc, msg)


def test_null_arguments(rt, dst3, src2):
    for dst, src, null in ((None, src2._h, False), (dst3._h, None, False), (dst3._h, src2._h, True)):
        rc, msg = _paste(rt, dst, src, null=null)
        assert rc == EINVAL and NAME in msg and "NULL" in msg, (rc, msg)


def test_a_dst_of_one_level_is_erange(rt, src2):
    one = _world_tree(rt, 1, 1)
    assert one.info().levels == 1
    rc, msg = _paste(rt, one._h, one._h)
    assert rc == ERANGE and NAME in msg and "levels" in msg, (rc, msg)
    rc, msg = _paste(rt, one._h, src2._h, axis=(2, 0, 1), flip=(1, 0, 1))
    assert rc == ERANGE, (rc, msg)


def test_palettes_and_maps(rt, dst3):
    """without a map the plain paste's rule holds; a map lifts it, and is itself the range check"""
    big = _world_tree(rt, 2, 3)
    assert big.info().n_materials == 4 and dst3.info().n_materials == 3
    before = _image(dst3), _image(big)
    rc, msg = _paste(rt, dst3._h, big._h, dst_origin=(5, 6, 7))
    assert rc == ERANGE and NAME in msg and "palette" in msg, (rc, msg)
    rc, msg = _paste(rt, dst3._h, big._h, dst_origin=(5, 6, 7), id_map=(0, 2, 1, 2))       # with a map it reaches the state check
    assert rc == ESTATE and NAME in msg and "not uploaded" in msg, (rc, msg)
    rc, msg = _paste(rt, dst3._h, big._h, id_map=(0, 2, 3, 65535))                         # the first entry out of range is named
    assert rc == ERANGE and NAME in msg and "id_map[2]" in msg, (rc, msg)
    rc, msg = _paste(rt, dst3._h, big._h, id_map=(0, 0, 0, 3))
    assert rc == ERANGE and "id_map[3]" in msg, (rc, msg)
    rc, msg = _paste(rt, dst3._h, big._h, dims=(0, 4, 4), id_map=(0, 9, 9, 9))             # arguments first
    assert rc == EINVAL, (rc, msg)
    rc, msg = _paste(rt, dst3._h, big._h, id_map=(7, 9, 9, 9))
    assert rc == EINVAL and "id_map[0]" in msg, (rc, msg)
    rc, msg = _paste(rt, big._h, dst3._h, dims=(16, 16, 16))                                # the other way round no map is needed
    assert rc == ESTATE, (rc, msg)
    assert (_image(dst3), _image(big)) == before


def test_trees_never_uploaded_are_estate(rt, dst3, src2):
    """the state check comes before any HIP call, for every valid combination of arguments"""
    before = _image(dst3), _image(src2)
    calls = (dict(dims=(16, 16, 16)), dict(dims=(16, 16, 16), dst_origin=(48, 48, 48), flags=1, axis=(1, 2, 0), flip=(1, 1, 1)),
             dict(src_origin=(3, 2, 1), dims=(9, 10, 11), dst_origin=(30, 31, 29), axis=(2, 1, 0), flip=(0, 0, 1), id_map=(0, 2)),
             dict(src_origin=(15, 15, 15), dims=(1, 1, 1), dst_origin=(63, 63, 63), flags=1, flip=(1, 0, 0), id_map=(0, 0)))
    for kw in calls:
        rc, msg = _paste(rt, dst3._h, src2._h, **kw)
        assert rc == ESTATE and NAME in msg and "not uploaded" in msg, (rc, msg)
    rc, msg = _paste(rt, dst3._h, dst3._h, dims=(64, 64, 64), axis=(1, 0, 2), flip=(1, 0, 0))           # src == dst
    assert rc == ESTATE, (rc, msg)
    with pytest.raises(rt.SvoError, match=r"svo_tree_patch_tree_oriented_gpu failed \(-4\).*not uploaded"):
        dst3.patch_tree_oriented(src2, None, None, (1, 2, 3), axis=(2, 1, 0), flip=(0, 0, 1))
    with pytest.raises(ValueError):
        dst3.patch_tree_oriented("a tree", None, None, (1, 2, 3))
    assert (_image(dst3), _image(src2)) == before
