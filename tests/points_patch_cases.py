"""The numpy side of the points patch's tests (tests/test_gpu_points_patch.py): the model of svo_tree_patch_points_gpu's list
semantics — entries applied in order, the last entry of a voxel decides, an id of 0 or one the tree's view does not hold
writes 0 — and a walk of an exported tree that counts the records reachable from the root, against which svo_tree_garbage
is checked.  A list is (xyz, ids) as in tests/points_cases.py; volumes are indexed [z, y, x]."""
import numpy as np

K_INTERIOR, K_BRICK, K_SOLID, K_UNIFORM = 0, 1, 2, 4
NO_COLOUR = 0xFFFFFFFFFFFFFFFF


def view_keep(pal, view):
    """per palette id: the tree's view stores it (svo_internal.h material_in_view); id 0 never"""
    keep = np.array([c != NO_COLOUR and (view == 1 or not (f & 0x10)) for f, c, _ in pal], bool)
    keep[0] = False
    return keep


def resolve_edits(xyz, ids, in_view):
    """(xyz, ids) of the distinct positions of a list with what each ends up holding: its last entry, 0 where that entry
    is 0 or an id not in view (in_view: a bool per palette id)"""
    xyz = np.asarray(xyz, np.int64).reshape(-1, 3)
    ids = np.asarray(ids, np.uint16).reshape(-1)
    if len(ids) == 0:
        return np.zeros((0, 3), np.int32), np.zeros(0, np.uint16)
    key = (xyz[:, 2] << 42) | (xyz[:, 1] << 21) | xyz[:, 0]     # coordinates are below 2^14
    _, first_in_reverse = np.unique(key[::-1], return_index=True)
    last = np.sort(len(key) - 1 - first_in_reverse)
    out = ids[last].copy()
    out[~np.asarray(in_view, bool)[out]] = 0
    return np.ascontiguousarray(xyz[last].astype(np.int32)), out


def apply_edits(vol, xyz, ids, in_view):
    """the composite: a copy of `vol` (the tree's stored content) with the list applied"""
    p, i = resolve_edits(xyz, ids, in_view)
    out = np.array(vol, np.uint16)
    out[p[:, 2], p[:, 1], p[:, 0]] = i
    return out


def _popcount(m):
    return np.unpackbits(np.ascontiguousarray(m, np.uint64).view(np.uint8)).reshape(-1, 64).sum(1).astype(np.int64)


def reachable(nodes, levels):
    """(node records, material entries) reachable from the root of an exported node array, level by level"""
    mask, ref = nodes[:, 0], (nodes[:, 1] & np.uint64(0xFFFFFFFF)).astype(np.int64)
    info = nodes[:, 1] >> np.uint64(32)
    kind, uni = (info & np.uint64(3)).astype(np.int64), (info & np.uint64(4)).astype(np.int64)
    cur = np.zeros(1, np.int64)
    n_nodes, n_mats = 1, 0
    for _ in range(levels + 1):
        if not len(cur):
            break
        bricks = cur[kind[cur] == K_BRICK]
        n_mats += int(_popcount(mask[bricks[uni[bricks] == 0]]).sum())
        inner = cur[kind[cur] == K_INTERIOR]
        cnt = _popcount(mask[inner])
        total = int(cnt.sum())
        n_nodes += total
        cur = np.repeat(ref[inner], cnt) + (np.arange(total) - np.repeat(np.cumsum(cnt) - cnt, cnt))
    assert not len(cur), "records below the brick level"
    return n_nodes, n_mats


def expected_garbage(tree):
    """what svo_tree_garbage must report: the arrays' lengths minus what the root reaches"""
    nodes, mats = tree.export()
    n, m = reachable(nodes, tree.info().levels)
    return len(nodes) - n, len(mats) - m


def neighbours26(xyz, extent):
    """the 26 neighbours of every position, those outside [0, extent) dropped"""
    d = np.array([(a, b, c) for a in (-1, 0, 1) for b in (-1, 0, 1) for c in (-1, 0, 1) if (a, b, c) != (0, 0, 0)], np.int64)
    p = (np.asarray(xyz, np.int64)[:, None, :] + d[None, :, :]).reshape(-1, 3)
    ok = ((p >= 0) & (p < extent)).all(1)
    return np.ascontiguousarray(p[ok].astype(np.int32))
