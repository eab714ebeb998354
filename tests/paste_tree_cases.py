"""The numpy side of the tree paste's tests (tests/test_gpu_paste_tree.py): the model of svo_tree_patch_tree_gpu's content
rule over dense volumes, and the tables of boxes the GPU cases run.  For every voxel p of the box, q = dst_origin + p takes
s = src(src_origin + p): src is taken in its own view first, then the mode is applied to s (REPLACE: q takes s; KEEP_EMPTY:
only where s != 0), and only then is the id resolved against dst's view (an id it does not hold writes 0).  Coordinates
are (x, y, z); volumes are indexed [z, y, x]."""
import numpy as np


def apply_paste(dst_dense, src_dense, src_origin, dims, dst_origin, keep_empty, in_view):
    """the composite: a copy of `dst_dense` (dst's stored content) with the box of `dims` = (nx, ny, nz) at `src_origin` of
    `src_dense` (src's stored content, in src's view) pasted at `dst_origin`; src_origin None: all of src_dense.
    in_view: a bool per id of dst's palette."""
    src = np.asarray(src_dense, np.uint16)
    out = np.array(dst_dense, np.uint16)
    if src_origin is None:
        src_origin, dims = (0, 0, 0), src.shape[::-1]
    (sx, sy, sz), (nx, ny, nz), (dx, dy, dz) = src_origin, dims, dst_origin
    assert min(nx, ny, nz) > 0 and min(sx, sy, sz, dx, dy, dz) >= 0
    assert sx + nx <= src.shape[2] and sy + ny <= src.shape[1] and sz + nz <= src.shape[0]
    assert dx + nx <= out.shape[2] and dy + ny <= out.shape[1] and dz + nz <= out.shape[0]
    s = src[sz:sz + nz, sy:sy + ny, sx:sx + nx]
    take = s != 0 if keep_empty else np.ones(s.shape, bool)          # the mode, decided on src's id
    stored = np.where(np.asarray(in_view, bool)[s], s, 0).astype(np.uint16)   # then dst's view
    box = out[dz:dz + nz, dy:dy + ny, dx:dx + nx]
    box[take] = stored[take]
    return out


# Boxes between two 64^3 worlds of tests/test_gpu_points_patch.py: old64, the planted world, whose first 16^3 is K_SOLID 4
# and which holds liquid (id 5); sparse64, mostly empty, whose last 16^3 is empty.
# name: (src world, dst world, src_origin, dims, dst_origin); src_origin None: the whole extent
BOXES64 = {
    "offset zero": ("old64", "sparse64", (8, 12, 16), (24, 20, 28), (8, 12, 16)),
    "offset a multiple of 16": ("old64", "old64", (0, 16, 0), (32, 32, 48), (32, 0, 16)),
    "offset a multiple of 4 only": ("old64", "old64", (4, 8, 12), (28, 24, 20), (16, 12, 24)),
    "offset (1, 2, 3)": ("old64", "old64", (10, 9, 8), (30, 29, 31), (11, 11, 11)),
    "negative offsets": ("old64", "sparse64", (33, 30, 21), (25, 30, 40), (2, 7, 18)),
    "a one-voxel box": ("old64", "old64", (21, 22, 20), (1, 1, 1), (38, 5, 19)),
    "one src brick off dst's grid": ("old64", "old64", (40, 24, 36), (4, 4, 4), (17, 30, 41)),
    "one src 16^3 off dst's grid": ("old64", "old64", (16, 16, 16), (16, 16, 16), (21, 6, 35)),
    "the whole extent": ("old64", "sparse64", None, None, (0, 0, 0)),
    "a K_SOLID 16^3 across dst's centre": ("old64", "old64", (0, 0, 0), (16, 16, 16), (25, 23, 26)),
    "src's empty 16^3": ("sparse64", "old64", (48, 48, 48), (16, 16, 16), (3, 9, 14)),
    "liquid in src": ("old64", "old64", (6, 6, 6), (30, 20, 25), (19, 22, 7)),
}
