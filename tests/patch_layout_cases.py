"""The patched trees whose raw layout tests/golden/patch_layout_digests.json pins, byte for byte: shared by
tests/test_gpu_patch_layout.py (which recomputes the digests with the tree's own library) and
tools/record_patch_layout_digests.py (which recorded them with the library of the commit named in the fixture).

A digest is the sha256 over a patched tree's exported node bytes, its material bytes, (n_nodes, n_mat_bytes, n_bricks,
nodes_per_level) of info() and garbage(), all taken before any compaction: the tail as the device-side patches append it,
record for record and in their order, which the content checks of the other GPU tests (made after compaction, or on voxels)
do not see.  Every patch entry point goes through one descent (csrc/svo_patch_cells.h); the cases take each of its paths.

The old world is test_gpu_volume_patch's old64 (3 levels, 64^3), in both views where a view matters; the cases that need an
empty 16^3, an empty brick position or a voxel alone in its brick take test_gpu_points_patch's sparse world."""
import hashlib

import numpy as np

import volume_cases as vc

EMPTY = (0, 0xFFFFFFFFFFFFFFFF, 0.0)
PAL = [EMPTY] + [(1 | f, c, 0.0) for f, c in vc.TABLE[1:]]  # ids = volume_cases' source ids (5: liquid)
VIEWS = (0, 1)


def old64():
    vol, has_big = vc.planted(64, 64, 64, (0, 0, 0), 7)
    assert has_big and (vol[0:16, 0:16, 0:16] == 4).all()  # the K_SOLID region
    vol[20:24, 20:24, 20:24] = 3            # BRICK | UNIFORM: one voxel missing
    vol[21, 22, 23] = 0
    vol[36:40, 24:28, 40:44] = 1            # a full brick of two materials
    vol[36:40, 24:26, 40:44] = 4
    return vol


def sparse64():
    """most bricks empty, one voxel alone in its brick and in its 16^3"""
    old = np.zeros((64, 64, 64), np.uint16)
    old[0:16, 0:12, 0:16] = vc.random_volume((16, 12, 16), 0.3, 5)
    old[35, 34, 33] = 1
    old[40:48, 40:44, 40:48] = 2
    return old


def digest(tree):
    nodes, mats = tree.export()
    i = tree.info()
    h = hashlib.sha256()
    h.update(nodes.tobytes())
    h.update(b"|" + mats.tobytes())
    h.update(b"|" + repr((int(i.n_nodes), int(i.n_mat_bytes), int(i.n_bricks), [int(x) for x in i.nodes_per_level])).encode())
    h.update(b"|" + repr(tuple(int(g) for g in tree.garbage())).encode())
    return h.hexdigest()


def _tree(rt, levels, vol, view=0):
    return rt.Tree.volume_gpu(levels, np.ascontiguousarray(vol, np.uint16), PAL, view=view)


def _points(entries):
    a = np.asarray(entries, np.int64).reshape(-1, 4)
    return np.ascontiguousarray(a[:, :3].astype(np.int32)), np.ascontiguousarray(a[:, 3].astype(np.uint16))


def _cube(x0, y0, z0, ids, s=4):
    z, y, x = np.meshgrid(np.arange(s), np.arange(s), np.arange(s), indexing="ij")
    xyz = np.stack([x.ravel() + x0, y.ravel() + y0, z.ravel() + z0], 1).astype(np.int32)
    return xyz, np.broadcast_to(np.asarray(ids, np.uint16), (s ** 3,)).copy()


def _rand(shape_zyx, seed):
    return vc.random_volume(shape_zyx, 0.5, seed)


def volume_cases(rt):
    """(name, digest): svo_tree_patch_volume_gpu"""
    old, full = old64(), np.full((16, 16, 16), 2, np.uint16)
    for view in VIEWS:
        def patched(vox, origin, base=old, levels=3):
            return digest(_tree(rt, levels, base, view).patch_volume(np.ascontiguousarray(vox, np.uint16), origin))

        v = "/view%d" % view
        yield "volume/off_grid_centre" + v, patched(_rand((11, 14, 13), 11), (29, 26, 31))  # residues 1, 2, 3; odd sizes
        yield "volume/one_voxel" + v, patched(np.full((1, 1, 1), 5, np.uint16), (23, 22, 21))
        yield "volume/one_brick" + v, patched(_rand((4, 4, 4), 12), (40, 24, 36))
        yield "volume/zeros_16" + v, patched(np.zeros((16, 16, 16), np.uint16), (32, 16, 48))
        yield "volume/cut_solid" + v, patched(_rand((9, 10, 11), 13), (10, 9, 8))            # cuts the K_SOLID 16^3
        yield "volume/mixed_over_solid" + v, patched(_rand((16, 16, 16), 14), (0, 0, 0))      # MIXED below a uniform cell
        yield "volume/whole_mixed" + v, patched(_rand((64, 64, 64), 15), (0, 0, 0))           # the restart
        yield "volume/whole_one_id" + v, patched(np.full((64, 64, 64), 3, np.uint16), (0, 0, 0))
        yield "volume/whole_zeros" + v, patched(np.zeros((64, 64, 64), np.uint16), (0, 0, 0))
        yield "volume/two_levels" + v, patched(_rand((5, 6, 7), 16), (3, 5, 6), base=old[16:32, 16:32, 16:32], levels=2)
        t = _tree(rt, 3, old, view).patch_volume(np.zeros((16, 16, 16), np.uint16), (32, 16, 48))
        yield "volume/one_id_into_empty_16" + v, digest(t.patch_volume(full, (32, 16, 48)))


def points_cases(rt):
    """(name, digest): svo_tree_patch_points_gpu"""
    old, sparse = old64(), sparse64()
    assert not sparse[20:24, 8:12, 48:52].any() and sparse[32:36, 32:36, 32:36].sum() == 1
    solid_voxel = tuple(int(c) for c in np.argwhere(old[24:28, 24:28, 24:28] != 0)[0][::-1] + 24)
    faces = [(0, 17, 30, 1), (63, 40, 9, 2), (22, 0, 41, 3), (50, 63, 33, 4), (13, 29, 0, 1), (44, 7, 63, 2)]
    erase = _cube(40, 24, 36, 0)
    dup = [(30, 31, 32, 1), solid_voxel + (0,), (30, 31, 32, 5), (5, 6, 7, 2), (30, 31, 32, 3), solid_voxel + (2,), (5, 6, 7, 0)]
    for view in VIEWS:
        def patched(xyz_ids, base=old, levels=3):
            return digest(_tree(rt, levels, base, view).patch_points(*xyz_ids))

        v = "/view%d" % view
        yield "points/one_voxel_empty" + v, patched(_points([(50, 9, 21, 3)]), base=sparse)
        yield "points/one_voxel_solid" + v, patched(_points([(5, 6, 7, 2)]))
        yield "points/one_voxel_brick_erased" + v, patched(_points([(33, 34, 35, 0)]), base=sparse)
        yield "points/one_voxel_brick_joined" + v, patched(_points([(34, 34, 35, 5)]), base=sparse)
        yield "points/whole_brick" + v, patched(_cube(20, 20, 20, 3))
        yield "points/whole_brick_mixed" + v, patched(_cube(40, 24, 36, np.arange(64) % 5 + 1))
        yield "points/erased_brick" + v, patched(erase)
        yield "points/duplicates" + v, patched(_points(dup))
        yield "points/faces" + v, patched(_points(faces))
        yield "points/solid_root" + v, patched(_points([(9, 40, 33, 0), (10, 40, 33, 2)]), base=np.full((64, 64, 64), 4, np.uint16))
        yield "points/two_levels" + v, patched(_points([(3, 5, 6, 2), (15, 0, 9, 0), (8, 8, 8, 5)]), base=old[16:32, 16:32, 16:32], levels=2)


def cell_cases(rt):
    """(name, digest): the shapes patch and the three pastes"""
    old = old64()
    src_vol = _rand((64, 64, 64), 21)
    src_vol[16:32, 0:16, 32:48] = 2   # a uniform 16^3, an empty one
    src_vol[32:48, 16:32, 0:16] = 0
    id_map = [0, 3, 0, 1, 5, 2]
    for view in VIEWS:
        v = "/view%d" % view
        src = _tree(rt, 3, src_vol, view)
        yield "shapes/off_grid_box" + v, digest(_tree(rt, 3, old, view).patch_shapes([rt.box((5, 6, 7), (21, 18, 23), 2)]))
        yield "shapes/ball_carve" + v, digest(_tree(rt, 3, old, view).patch_shapes([rt.ball((31, 32, 30), 13 * 13 + 2, 0)]))
        for keep in (False, True):
            t = _tree(rt, 3, old, view).patch_tree(src, (8, 4, 2), (37, 41, 39), (1, 2, 3), keep_empty=keep)
            yield "paste/offset_123_%s" % ("keep_empty" if keep else "replace") + v, digest(t)
        t = _tree(rt, 3, old, view).patch_tree_oriented(src, (8, 4, 2), (21, 34, 27), (6, 3, 9), axis=(2, 0, 1), flip=(1, 0, 1), id_map=id_map)
        yield "paste/oriented_map" + v, digest(t)
        t = _tree(rt, 3, old, view).patch_tree_rule(src, (8, 4, 2), (37, 41, 39), (1, 2, 3), rt.RULE_UNDER)
        yield "paste/rule_under" + v, digest(t)


def sequence_cases(rt):
    """(name, digest): a volume patch, a points patch, a shapes patch and a paste on one tree: tails behind tails.  This pins
    the layout of four of the 49 ordered pairs of kinds; tests/test_gpu_mixed_ops.py checks the content, the garbage counts,
    the host image and the ceilings of all of them, step by step, against a model (tests/mixed_ops_cases.py)."""
    old = old64()
    for view in VIEWS:
        src = _tree(rt, 3, _rand((64, 64, 64), 22), view)
        t = _tree(rt, 3, old, view)
        for step, patch in enumerate((
                lambda: t.patch_volume(_rand((11, 14, 13), 23), (29, 26, 31)),
                lambda: t.patch_points(*_points([(30, 30, 32, 0), (31, 30, 32, 4), (2, 3, 4, 1), (63, 63, 63, 5)])),
                lambda: t.patch_shapes([rt.ball((31, 32, 30), 90, 0), rt.box((27, 28, 29), (9, 5, 7), 3)]),
                lambda: t.patch_tree(src, (3, 2, 1), (25, 23, 21), (22, 27, 30), keep_empty=True))):
            patch()
            yield "sequence/step%d/view%d" % (step + 1, view), digest(t)


def all_cases(rt):
    for cases in (volume_cases, points_cases, cell_cases, sequence_cases):
        yield from cases(rt)
