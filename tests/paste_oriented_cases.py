"""The numpy side of the oriented paste's tests (tests/test_gpu_paste_oriented.py, tests/test_paste_oriented_model.py): the
model of svo_tree_patch_tree_oriented_gpu's content rule over dense volumes, written as plain index arithmetic.

The destination box is dst_origin + [0, dn) with dn[a] = n[axis[a]].  A voxel q of it has d = q - dst_origin and reads src
at s with s[axis[a]] = src_origin[axis[a]] + (n[axis[a]] - 1 - d[a] if flip[a] else d[a]).  The id goes through four steps:
src's id in src's own view; id_map[id] when a map is given; the mode, decided on the mapped id (REPLACE: q takes it;
KEEP_EMPTY: only where it is not 0); dst's view (an id it does not hold writes 0).
Coordinates, dimensions, axis and flip are (x, y, z); volumes are indexed [z, y, x]."""
import itertools

import numpy as np

# the 48 signed permutations: (axis, flip)
ORIENTATIONS = [(axis, flip) for axis in itertools.permutations(range(3)) for flip in itertools.product((0, 1), repeat=3)]
IDENTITY = ((0, 1, 2), (0, 0, 0))
QUARTER_Y = ((2, 1, 0), (0, 0, 1))     # a quarter turn about y: np.rot90(box, 1, axes=(0, 2)) of a [z, y, x] box
MIRROR_X = ((0, 1, 2), (1, 0, 0))
INVERSION = ((0, 1, 2), (1, 1, 1))


def determinant(axis, flip):
    """+1 for the 24 rotations, -1 for the mirrorings"""
    m = np.zeros((3, 3), np.int64)
    for a in range(3):
        m[a, axis[a]] = -1 if flip[a] else 1
    return int(round(np.linalg.det(m)))


def inverse(axis, flip):
    """the orientation that takes the turned box back: composing the two index maps gives the identity"""
    inv_axis, inv_flip = [0, 0, 0], [0, 0, 0]
    for a in range(3):
        inv_axis[axis[a]], inv_flip[axis[a]] = a, flip[a]
    return tuple(inv_axis), tuple(inv_flip)


def dst_dims(dims, axis):
    return tuple(dims[axis[a]] for a in range(3))


def source_index(dims, axis, flip):
    """index arrays (iz, iy, ix) into the src box [nz, ny, nx], each of the destination box's shape [dnz, dny, dnx]"""
    dn = dst_dims(dims, axis)
    d = np.meshgrid(np.arange(dn[0]), np.arange(dn[1]), np.arange(dn[2]), indexing="ij")   # d[a][x, y, z]: the offset along a
    s = [None, None, None]
    for a in range(3):
        s[axis[a]] = dims[axis[a]] - 1 - d[a] if flip[a] else d[a]
    # [x, y, z] order to [z, y, x]
    return tuple(np.transpose(s[j], (2, 1, 0)) for j in (2, 1, 0))


def orient_box(box, axis, flip):
    """the src box [nz, ny, nx] as the destination sees it, [dnz, dny, dnx]"""
    box = np.asarray(box)
    return box[source_index(box.shape[::-1], axis, flip)]


def apply_oriented(dst_dense, src_dense, src_origin, dims, dst_origin, axis, flip, id_map, keep_empty, in_view):
    """the composite: a copy of `dst_dense` (dst's stored content) with the box of `dims` = (nx, ny, nz) at `src_origin` of
    `src_dense` (src's stored content, in src's view) pasted at `dst_origin` under the orientation and the map; src_origin
    None: all of src_dense.  id_map: None or one id per id of src's palette; in_view: a bool per id of dst's palette."""
    src = np.asarray(src_dense, np.uint16)
    out = np.array(dst_dense, np.uint16)
    if src_origin is None:
        src_origin, dims = (0, 0, 0), src.shape[::-1]
    (sx, sy, sz), (nx, ny, nz), (dx, dy, dz) = src_origin, dims, dst_origin
    dn = dst_dims(dims, axis)
    assert sorted(axis) == [0, 1, 2] and all(f in (0, 1) for f in flip)
    assert min(nx, ny, nz) > 0 and min(sx, sy, sz, dx, dy, dz) >= 0
    assert sx + nx <= src.shape[2] and sy + ny <= src.shape[1] and sz + nz <= src.shape[0]
    assert dx + dn[0] <= out.shape[2] and dy + dn[1] <= out.shape[1] and dz + dn[2] <= out.shape[0]
    s = orient_box(src[sz:sz + nz, sy:sy + ny, sx:sx + nx], axis, flip)       # (1) src's id in src's view
    if id_map is not None:
        id_map = np.asarray(id_map, np.uint16)
        assert id_map[0] == 0
        s = id_map[s]                                                         # (2) the map
    take = s != 0 if keep_empty else np.ones(s.shape, bool)                   # (3) the mode, on the mapped id
    stored = np.where(np.asarray(in_view, bool)[s], s, 0).astype(np.uint16)   # (4) dst's view
    box = out[dz:dz + dn[2], dy:dy + dn[1], dx:dx + dn[0]]
    box[take] = stored[take]
    return out


def orient_point(p, src_origin, dims, dst_origin, axis, flip):
    """where the src voxel p of the box lands in dst"""
    q = [0, 0, 0]
    for a in range(3):
        j = axis[a]
        off = p[j] - src_origin[j]
        q[a] = dst_origin[a] + (dims[j] - 1 - off if flip[a] else off)
    return tuple(q)
