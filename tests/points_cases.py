"""Sparse voxel lists for the point builder's tests (tests/test_gpu_points_build.py): lists made from the dense volumes of
tests/volume_cases.py, a numpy model of the list semantics (applied in order, the last entry of a voxel decides, id 0
erases) and the host-built twin of a list (an rt.World filled with put_blocks of the survivors).  A list is (xyz, ids):
xyz an int32 array (n, 3) of world positions (x, y, z), ids a uint16 array of n source ids into a table such as
volume_cases.TABLE."""
import numpy as np

import volume_cases as vc
from palette_cases import world_with_palette


def as_points(vol, origin, seed):
    """the non-zero voxels of a volume_cases volume ([z, y, x], element [0, 0, 0] at world `origin`) as a shuffled list"""
    z, y, x = np.nonzero(vol)
    ids = vol[z, y, x].astype(np.uint16)
    xyz = np.stack([x + origin[0], y + origin[1], z + origin[2]], 1).astype(np.int32)
    order = np.random.default_rng(seed).permutation(len(ids))
    return np.ascontiguousarray(xyz[order]), np.ascontiguousarray(ids[order])


def empty_list():
    return np.zeros((0, 3), np.int32), np.zeros(0, np.uint16)


def concat(*lists):
    """several lists applied one after the other"""
    return (np.ascontiguousarray(np.concatenate([np.asarray(l[0], np.int32).reshape(-1, 3) for l in lists])),
            np.ascontiguousarray(np.concatenate([np.asarray(l[1], np.uint16).reshape(-1) for l in lists])))


def last_wins(xyz, ids):
    """the model: (xyz, ids) of the voxels a list leaves — of every distinct position its last entry, those of id 0
    dropped — in the order of those last entries"""
    xyz = np.asarray(xyz, np.int64).reshape(-1, 3)
    ids = np.asarray(ids, np.uint16)
    if len(ids) == 0:
        return empty_list()
    key = (xyz[:, 2] << 42) | (xyz[:, 1] << 21) | xyz[:, 0]     # coordinates are below 2^14
    _, first_in_reverse = np.unique(key[::-1], return_index=True)
    last = np.sort(len(key) - 1 - first_in_reverse)
    last = last[ids[last] != 0]
    return np.ascontiguousarray(xyz[last].astype(np.int32)), np.ascontiguousarray(ids[last])


def host_twin(rt, levels, xyz, ids, view, table=vc.TABLE):
    """(host tree of `view`, its palette, the list's ids in that palette): volume_cases.host_twin's method for a list — an
    rt.World filled with put_blocks of the model's survivors at level levels + 1, built, the ids remapped to the host
    palette by (flags, colour).  The world interns the whole table first (palette_cases.world_with_palette), so that an
    id that survives nowhere — one overwritten wherever it was listed — still has its palette entry"""
    w = world_with_palette(rt, levels, [(f, c, 0.0) for f, c in table])
    sx, si = last_wins(xyz, ids)
    flags = np.array([t[0] for t in table], np.uint32)
    cols = np.array([t[1] for t in table], np.uint64)
    if len(si):
        w.put_blocks(sx, flags[si], cols[si])
    h = w.build(view)
    pal = h.palette()
    key = {(f, c): i for i, (f, c, _) in enumerate(pal)}
    remap = np.zeros(len(table), np.uint16)
    for i in range(1, len(table)):
        remap[i] = key[(1 | table[i][0], table[i][1])]
    return h, pal, remap[np.asarray(ids, np.uint16)]


def dense(levels, xyz, ids):
    """the whole extent as a volume [z, y, x] holding the model's survivors (small worlds only)"""
    E = 4 ** levels
    vol = np.zeros((E, E, E), np.uint16)
    sx, si = last_wins(xyz, ids)
    vol[sx[:, 2], sx[:, 1], sx[:, 0]] = si
    return vol
