"""The numpy side of the rule paste's tests (tests/test_gpu_paste_rule.py, tests/test_paste_rule_model.py): the model of
svo_tree_patch_tree_rule_gpu's content rule over dense volumes.

The geometry, the orientation and the id map are the oriented paste's (tests/paste_oriented_cases.py).  For each voxel of
the destination box, s is src's id through the orientation and the map, d what dst stores there, in dst's own view, and R(s)
is s where dst's view holds it, else 0.  rule = a | b << 2 | c << 4 says what the voxel holds afterwards:
    a  where s != 0 and d == 0:  KEEP 0, TAKE R(s)
    b  where s != 0 and d != 0:  KEEP d, TAKE R(s), CLEAR 0
    c  where s == 0 and d != 0:  KEEP d, CLEAR 0
Coordinates, dimensions, axis and flip are (x, y, z); volumes are indexed [z, y, x]."""
import numpy as np

import paste_oriented_cases as poc

KEEP, TAKE, CLEAR = 0, 1, 2


def rule_of(a, b, c):
    return a | b << 2 | c << 4


# the 12 valid rules, (a, b, c) each, and the eight the header names
RULES = [rule_of(a, b, c) for c in (KEEP, CLEAR) for b in (KEEP, TAKE, CLEAR) for a in (KEEP, TAKE)]
UNDER, PAINT, OVER, ERASE, XOR, MASK, STENCIL, REPLACE = 1, 4, 5, 8, 9, 32, 36, 37
NAMED = {"UNDER": UNDER, "PAINT": PAINT, "OVER": OVER, "ERASE": ERASE, "XOR": XOR, "MASK": MASK, "STENCIL": STENCIL, "REPLACE": REPLACE}


def fields(rule):
    return rule & 3, (rule >> 2) & 3, (rule >> 4) & 3


def mapped_box(src_dense, src_origin, dims, axis, flip, id_map):
    """s over the destination box, [dnz, dny, dnx]: src's box oriented, then mapped"""
    src = np.asarray(src_dense, np.uint16)
    if src_origin is None:
        src_origin, dims = (0, 0, 0), src.shape[::-1]
    (sx, sy, sz), (nx, ny, nz) = src_origin, dims
    assert min(nx, ny, nz) > 0 and min(sx, sy, sz) >= 0
    assert sx + nx <= src.shape[2] and sy + ny <= src.shape[1] and sz + nz <= src.shape[0]
    s = poc.orient_box(src[sz:sz + nz, sy:sy + ny, sx:sx + nx], axis, flip)
    if id_map is not None:
        id_map = np.asarray(id_map, np.uint16)
        assert id_map[0] == 0
        s = id_map[s]
    return s


def apply_rule(dst_dense, src_dense, so, dims, do, axis, flip, id_map, rule, view_keep):
    """a copy of `dst_dense` (dst's stored content, in dst's view) with the box of `dims` at `so` of `src_dense` (src's stored
    content, in src's view) combined into it at `do` under `rule`.  view_keep: a bool per id of dst's palette."""
    a, b, c = fields(rule)
    assert a in (KEEP, TAKE) and b in (KEEP, TAKE, CLEAR) and c in (KEEP, CLEAR) and rule >> 6 == 0
    out = np.array(dst_dense, np.uint16)
    s = mapped_box(src_dense, so, dims, axis, flip, id_map)
    dn = s.shape[::-1]
    dx, dy, dz = do
    assert min(do) >= 0 and dx + dn[0] <= out.shape[2] and dy + dn[1] <= out.shape[1] and dz + dn[2] <= out.shape[0]
    box = out[dz:dz + dn[2], dy:dy + dn[1], dx:dx + dn[0]]
    d = box.copy()
    rs = np.where(np.asarray(view_keep, bool)[s], s, 0).astype(np.uint16)
    zero = np.zeros_like(d)
    res = d.copy()
    res = np.where((s != 0) & (d == 0), rs if a == TAKE else zero, res)
    res = np.where((s != 0) & (d != 0), d if b == KEEP else (rs if b == TAKE else zero), res)
    res = np.where((s == 0) & (d != 0), d if c == KEEP else zero, res)
    box[...] = res
    return out


def cases_in_box(dst_dense, src_dense, so, dims, do, axis, flip, id_map):
    """how many voxels of the destination box fall under A (src only), B (both) and C (dst only)"""
    s = mapped_box(src_dense, so, dims, axis, flip, id_map)
    dn = s.shape[::-1]
    d = np.asarray(dst_dense)[do[2]:do[2] + dn[2], do[1]:do[1] + dn[1], do[0]:do[0] + dn[0]]
    return int(((s != 0) & (d == 0)).sum()), int(((s != 0) & (d != 0)).sum()), int(((s == 0) & (d != 0)).sum())
