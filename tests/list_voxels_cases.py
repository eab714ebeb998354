"""The numpy side of the voxel listing's tests (tests/test_gpu_list_voxels.py): the point builder's key of a position,
and the model of svo_tree_list_voxels_gpu over a dense volume — the non-zero voxels a view stores inside a box, in key
order.  Volumes are numpy uint16 arrays indexed [z, y, x] that cover the whole extent from the world's origin; a list is
(xyz, ids) as in tests/points_cases.py."""
import numpy as np

import points_cases as pc
import volume_cases as vc  # noqa: F401  (the volumes the model is run over come from there)


def key_of(xyz, levels):
    """voxel_key (svo_points_source.h) of every row of xyz: 6 bits per level, the top level first, each level's slot
    z<<4 | y<<2 | x of that level's base-4 digits"""
    p = np.asarray(xyz, np.int64).reshape(-1, 3)
    key = np.zeros(len(p), np.int64)
    for d in range(levels):
        sh = 2 * (levels - 1 - d)
        key = (key << 6) | (((p[:, 2] >> sh) & 3) << 4) | (((p[:, 1] >> sh) & 3) << 2) | ((p[:, 0] >> sh) & 3)
    return key


def by_key(xyz, ids, levels):
    """a list of distinct voxels sorted by key"""
    xyz = np.asarray(xyz, np.int32).reshape(-1, 3)
    ids = np.asarray(ids, np.uint16).reshape(-1)
    order = np.argsort(key_of(xyz, levels), kind="stable")
    return np.ascontiguousarray(xyz[order]), np.ascontiguousarray(ids[order])


def levels_of(vol):
    E = vol.shape[0]
    assert vol.shape == (E, E, E)
    levels = int(round(np.log(E) / np.log(4)))
    assert 4 ** levels == E
    return levels


def model(vol, origin=None, shape=None, in_view=None):
    """(xyz, ids) of the non-zero voxels of `vol` inside the box of `shape` = (nz, ny, nx) at origin (x, y, z) — both None:
    the whole extent — sorted by key.  in_view: a boolean per id, False where the tree's view does not store the id
    (None: every id is stored)"""
    levels = levels_of(vol)
    if origin is None:
        origin, shape = (0, 0, 0), vol.shape
    (x0, y0, z0), (nz, ny, nx) = origin, shape
    sub = vol[z0:z0 + nz, y0:y0 + ny, x0:x0 + nx]
    if in_view is not None:
        sub = np.where(np.asarray(in_view, bool)[sub], sub, 0)
    z, y, x = np.nonzero(sub)
    return by_key(np.stack([x + x0, y + y0, z + z0], 1), sub[z, y, x], levels)


def in_box(xyz, ids, origin, shape):
    """the entries of a list inside the box of `shape` = (nz, ny, nx) at origin (x, y, z), in the list's order"""
    lo = np.asarray(origin, np.int64)
    hi = lo + np.asarray(shape[::-1], np.int64)
    keep = ((xyz >= lo) & (xyz < hi)).all(1)
    return np.ascontiguousarray(xyz[keep]), np.ascontiguousarray(ids[keep])


def survivors(xyz, ids, levels):
    """points_cases.last_wins of a list, sorted by key: what a points-built tree of every id's view lists"""
    return by_key(*pc.last_wins(xyz, ids), levels)
