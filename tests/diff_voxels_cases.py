"""The numpy side of the tree diff's tests (tests/test_gpu_diff_voxels.py): the model of svo_tree_diff_gpu over two dense
volumes — the positions of a box at which the two in-view volumes hold different ids, with the second volume's ids, in
the point builder's key order — and the same over two lists of stored voxels, for worlds whose dense volume does not
exist.  Volumes and lists are those of tests/list_voxels_cases.py."""
import numpy as np

import list_voxels_cases as lv


def model(vol_a, vol_b, origin=None, shape=None):
    """(xyz, ids) of the voxels of the box of `shape` = (nz, ny, nx) at origin (x, y, z) — both None: the whole extent —
    where vol_a and vol_b (each already reduced to what its tree's view stores) differ; ids are vol_b's, 0 where it is
    empty; sorted by key"""
    levels = lv.levels_of(vol_a)
    assert vol_a.shape == vol_b.shape
    if origin is None:
        origin, shape = (0, 0, 0), vol_a.shape
    (x0, y0, z0), (nz, ny, nx) = origin, shape
    sa = vol_a[z0:z0 + nz, y0:y0 + ny, x0:x0 + nx]
    sb = vol_b[z0:z0 + nz, y0:y0 + ny, x0:x0 + nx]
    z, y, x = np.nonzero(sa != sb)
    return lv.by_key(np.stack([x + x0, y + y0, z + z0], 1), sb[z, y, x], levels)


def of_lists(a, b, levels):
    """the symmetric difference by key of two lists of stored voxels (xyz, ids), each of distinct positions and non-zero
    ids: the positions either list holds and at which the two differ, with b's ids (0 where b does not hold the
    position), sorted by key"""
    (ax, ai), (bx, bi) = a, b
    ka, kb = lv.key_of(ax, levels), lv.key_of(bx, levels)
    assert len(np.unique(ka)) == len(ka) and len(np.unique(kb)) == len(kb)
    oa, ob = np.argsort(ka), np.argsort(kb)
    ka, ax, ai = ka[oa], np.asarray(ax, np.int32).reshape(-1, 3)[oa], np.asarray(ai, np.uint16)[oa]
    kb, bx, bi = kb[ob], np.asarray(bx, np.int32).reshape(-1, 3)[ob], np.asarray(bi, np.uint16)[ob]
    at = np.searchsorted(ka, kb)                       # b's entries looked up in a
    hit = np.zeros(len(kb), bool)
    inside = at < len(ka)
    hit[inside] = ka[at[inside]] == kb[inside]
    same = hit.copy()
    same[hit] = ai[at[hit]] == bi[hit]
    gone = np.ones(len(ka), bool)                      # a's entries that b does not hold
    gone[at[hit]] = False
    xyz = np.concatenate([bx[~same], ax[gone]])
    ids = np.concatenate([bi[~same], np.zeros(int(gone.sum()), np.uint16)])
    return lv.by_key(xyz, ids, levels)
