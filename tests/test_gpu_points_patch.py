"""svo_tree_patch_points_gpu on the GPU: a resident tree patched from a sparse list of voxel edits holds the composite — every
listed voxel its resolved entry, every other voxel as before — and reads back, carries ceilings, casts and, once
compacted, is laid out exactly like a tree built afresh from that composite.  The reference for content is numpy
(points_patch_cases.apply_edits: the last entry per position, 0 or an id out of the view writing 0).

Checks of every content case, by the numbers used below: (1) read_volume of the whole extent equals the composite (at 7
levels: get_blocks_gpu at the edited positions, their 26 neighbours and 10,000 random positions equals the model); (2)
after compact(), export(), info() and the palette equal those of Tree.volume_gpu of the composite (at 7 levels: of
Tree.points_gpu of the merged list); (3) the ceilings, pairs and quads in HBM equal the fresh build's, before and after the
compaction; (4) casts give hit records identical to the fresh tree's; (5) garbage() equals the arrays' lengths minus what
a walk of export() reaches from the root.  No K_BRICK record has mask 0."""
import numpy as np
import pytest

import palette_cases as pcs
import points_cases as pc
import points_patch_cases as ppc
import volume_cases as vc
from test_gpu_volume_build import _same, _same_ceilings
from test_gpu_volume_patch import PAL, _kinds, _slot_is_clear, _tree, check_casts

pytestmark = pytest.mark.gpu

K_INTERIOR, K_BRICK, K_SOLID = 0, 1, 2


@pytest.fixture(scope="module")
def cuda(rt):
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    assert hasattr(rt.lib(), "svo_tree_patch_points_gpu")
    return torch


def _old64():
    """test_gpu_volume_patch's old64: planted(64^3) with a one-voxel-missing uniform brick and a full two-material brick"""
    vol, has_big = vc.planted(64, 64, 64, (0, 0, 0), 7)
    assert has_big
    vol[20:24, 20:24, 20:24] = 3
    vol[21, 22, 23] = 0
    vol[36:40, 24:28, 40:44] = 1
    vol[36:40, 24:26, 40:44] = 4
    return vol


@pytest.fixture(scope="module")
def old64():
    vol = _old64()
    vol.setflags(write=False)
    return vol


def _list(entries):
    """[(x, y, z, id)] as a list (xyz, ids)"""
    a = np.asarray(entries, np.int64).reshape(-1, 4)
    return np.ascontiguousarray(a[:, :3].astype(np.int32)), np.ascontiguousarray(a[:, 3].astype(np.uint16))


def _cube(x0, y0, z0, ids, s=4):
    """the s^3 voxels of the cube at (x0, y0, z0), x fastest, with `ids` (one id or s^3 of them)"""
    z, y, x = np.meshgrid(np.arange(s), np.arange(s), np.arange(s), indexing="ij")
    xyz = np.stack([x.ravel() + x0, y.ravel() + y0, z.ravel() + z0], 1).astype(np.int32)
    return xyz, np.broadcast_to(np.asarray(ids, np.uint16), (s ** 3,)).copy()


def _stored(t):
    E = 4 ** t.info().levels
    return t.read_volume((0, 0, 0), (E, E, E)).cpu().numpy().view(np.uint16).copy()


def check_patched(rt, cuda, t, comp, label, casts=True, compact=True, shift=(0.0, 0.0, 0.0)):
    """(1) .. (5) for a patched tree t whose content must be `comp` (already in the tree's view); returns the fresh tree"""
    i = t.info()
    levels, view, pal = i.levels, i.view, t.palette()
    got = _stored(t)
    assert np.array_equal(got, comp), "(1) %s: %d voxels differ" % (label, int((got != comp).sum()))
    assert t.garbage() == ppc.expected_garbage(t), "(5) %s" % label
    mask, kind, _ = _kinds(t)
    assert not ((kind == K_BRICK) & (mask == 0)).any(), "%s: a K_BRICK record with mask 0" % label
    fresh = rt.Tree.volume_gpu(levels, comp, pal, view=view)
    _same_ceilings(t, fresh, "(3) " + label)
    if casts:
        if view == 0:
            check_casts(rt, cuda, t, fresh, "(4) " + label, shift=shift)
        else:  # a full-view tree is walked as the scene of the shading pass
            solid = rt.Tree.volume_gpu(levels, vc.in_view(comp, pal, 0), pal, view=0)
            org, d = (1.0, 2.0, 3.0), rt.normalize((0.6, -0.45, 0.66))
            (ca, ha), (cb, hb) = (solid.shade_frame(org, d, 64, 32, 300, scene=s, time=0.25, with_hits=True) for s in (t, fresh))
            assert cuda.equal(ca, cb), "(4) %s colours" % label
            for k in ("pos_steps", "t", "info"):
                assert cuda.equal(ha[k], hb[k]), "(4) %s %s" % (label, k)
            assert t.guard_trips() == 0
    if compact:
        t.compact()
        _same(t, fresh, "(2) " + label)
        assert t.info().n_mat_bytes == fresh.info().n_mat_bytes and t.garbage() == (0, 0), "(2) " + label
        _same_ceilings(t, fresh, "(3) compacted, " + label)
    return fresh


def patch_and_check(rt, cuda, old, xyz, ids, label, view=0, levels=3, pal=PAL, **kw):
    """a volume-built tree of `old`, patched with the list, against the model"""
    t = rt.Tree.volume_gpu(levels, np.array(old, np.uint16), pal, view=view)
    keep = ppc.view_keep(pal, view)
    comp = ppc.apply_edits(vc.in_view(np.asarray(old), pal, view), xyz, ids, keep)
    assert t.patch_points(xyz, ids) is t
    check_patched(rt, cuda, t, comp, label, **kw)
    return t, comp


def _sparse64():
    """test_one_voxel_box's old world: most bricks empty, one voxel alone in its brick and in its 16^3"""
    old = np.zeros((64, 64, 64), np.uint16)
    old[0:16, 0:12, 0:16] = vc.random_volume((16, 12, 16), 0.3, 5)
    old[35, 34, 33] = 1
    old[40:48, 40:44, 40:48] = 2
    return old


# ----------------------------------------------------------------------------------------------- 1. single voxels --
def test_one_voxel_into_an_empty_brick_position(rt, cuda):
    old = _sparse64()
    assert not old[20:24, 8:12, 48:52].any()
    t, comp = patch_and_check(rt, cuda, old, *_list([(50, 9, 21, 3)]), "empty brick position", compact=False)
    assert comp[21, 9, 50] == 3 and t.get_block(50, 9, 21)[1] == 3
    check_patched(rt, cuda, t, comp, "empty brick position, compacted", casts=False)


def test_one_voxel_into_a_solid_16_cubed(rt, cuda, old64):
    assert (old64[0:16, 0:16, 0:16] == 4).all()
    t = _tree(rt, 3, old64)
    n0, root_children = t.info().n_nodes, bin(int(t.export()[0][0, 0])).count("1")
    t.patch_points(*_list([(5, 6, 7, 2)]))
    # the root's child block again, and the SOLID region expanded: 64 children of the 16^3, all K_SOLID siblings but the
    # one edited brick
    assert t.info().n_nodes - n0 == root_children + 64 and t.garbage() == (root_children, 0)
    mask, kind, mat = _kinds(t)
    ni, nj, nk = (int(i) for i in t.node_indices([(1, 1, 1), (9, 9, 9), (5, 6, 7)]))
    assert kind[ni] == K_SOLID and mat[ni] == 4 and kind[nj] == K_SOLID and ni != nj and kind[nk] == K_BRICK
    comp = ppc.apply_edits(old64, *_list([(5, 6, 7, 2)]), ppc.view_keep(PAL, 0))
    assert comp[7, 6, 5] == 2 and (comp != old64).sum() == 1
    check_patched(rt, cuda, t, vc.in_view(comp, PAL, 0), "into a SOLID 16^3")


def test_one_voxel_into_an_empty_tree(rt, cuda):
    old = np.zeros((64, 64, 64), np.uint16)
    t = _tree(rt, 3, old)
    assert len(t.export()[0]) == 1
    t.patch_points(*_list([(37, 5, 20, 1)]))
    assert t.info().n_nodes == 3            # the root, an interior, a brick, and no more
    comp = old.copy()
    comp[20, 5, 37] = 1
    check_patched(rt, cuda, t, comp, "empty tree")


def test_erasing_the_only_voxel_of_a_brick_clears_the_slot(rt, cuda):
    old = _sparse64()
    t, comp = patch_and_check(rt, cuda, old, *_list([(33, 34, 35, 0)]), "one-voxel brick erased", compact=False)
    assert comp[35, 34, 33] == 0 and _slot_is_clear(t, 33, 34, 35)
    t.patch_points(*_list([(50, 9, 21, 0)]))    # an erasure where nothing is stored: the slot stays clear
    assert _slot_is_clear(t, 50, 9, 21)
    check_patched(rt, cuda, t, comp, "one-voxel brick erased, then a void erased")


def test_erasing_one_voxel_of_an_all_solid_world(rt, cuda):
    old = np.full((64, 64, 64), 2, np.uint16)
    t = _tree(rt, 3, old)
    mask, kind, _ = _kinds(t)
    assert len(mask) == 1 and kind[0] == K_SOLID
    t.patch_points(*_list([(13, 22, 31, 0)]))
    mask, kind, _ = _kinds(t)
    assert kind[0] == K_INTERIOR and mask[0] == np.uint64(0xFFFFFFFFFFFFFFFF)   # the lone SOLID root became interior
    assert len(mask) == 1 + 64 + 64 and t.garbage() == (0, 0)
    comp = old.copy()
    comp[31, 22, 13] = 0
    check_patched(rt, cuda, t, comp, "hole in a solid world")


# -------------------------------------------------------------------------------------------------- 2. duplicates --
def _solid_voxel(vol):
    z, y, x = np.argwhere((vol >= 1) & (vol <= 4))[1234]
    return int(x), int(y), int(z)


def test_put_erase_put_of_one_voxel(rt, cuda, old64):
    p = (50, 9, 21)
    t, comp = patch_and_check(rt, cuda, old64, *_list([p + (1,), p + (0,), p + (3,)]), "put, erase, put")
    assert comp[21, 9, 50] == 3


def test_a_last_entry_of_0_erases_stored_content(rt, cuda, old64):
    p = _solid_voxel(old64)
    q = (p[0] ^ 1, p[1], p[2])
    t, comp = patch_and_check(rt, cuda, old64, *_list([p + (2,), q + (1,), p + (0,)]), "a last 0 erases")
    assert old64[p[2], p[1], p[0]] != 0 and comp[p[2], p[1], p[0]] == 0 and comp[q[2], q[1], q[0]] == 1


@pytest.mark.parametrize("view", [0, 1])
def test_a_liquid_last_entry_over_solid_content(rt, cuda, old64, view):
    p = _solid_voxel(old64)
    t, comp = patch_and_check(rt, cuda, old64, *_list([p + (2,), p + (5,)]), "liquid over solid, view %d" % view, view=view)
    assert comp[p[2], p[1], p[0]] == (5 if view else 0)
    assert t.get_block(*p)[1] == (5 if view else 0)


@pytest.mark.parametrize("view", [0, 1])
def test_shuffled_list_with_duplicates(rt, cuda, old64, view):
    rng = np.random.default_rng(81)
    pos = rng.integers(0, 64, (1500, 3)).astype(np.int32)
    xyz = np.ascontiguousarray(pos[rng.integers(0, 1500, 5000)])
    ids = rng.integers(0, 6, 5000).astype(np.uint16)
    assert len(np.unique(xyz, axis=0)) < 1501 and (ids == 0).any() and (ids == 5).any()
    patch_and_check(rt, cuda, old64, xyz, ids, "5000 entries over 1500 positions, view %d" % view, view=view)


def test_numpy_and_tensor_arguments_patch_alike(rt, cuda, old64):
    rng = np.random.default_rng(82)
    xyz = rng.integers(0, 64, (300, 3)).astype(np.int32)
    ids = rng.integers(0, 5, 300).astype(np.uint16)
    a, b = _tree(rt, 3, old64), _tree(rt, 3, old64)
    a.patch_points(xyz, ids)
    b.patch_points(cuda.from_numpy(xyz).cuda(), cuda.from_numpy(ids.view(np.int16)).cuda())
    _same(a, b, "numpy vs tensors")
    with pytest.raises(ValueError):
        a.patch_points(xyz, ids[:-1])
    with pytest.raises(ValueError):
        a.patch_points(xyz.astype(np.int64), ids)


# ------------------------------------------------------------------------------------------- 3. corners and bricks --
def test_two_edits_in_opposite_corners(rt, cuda, old64):
    t, comp = patch_and_check(rt, cuda, old64, *_list([(0, 0, 0, 1), (63, 63, 63, 2)]), "opposite corners")
    assert comp[0, 0, 0] == 1 and comp[63, 63, 63] == 2


BRICK = (40, 24, 36)  # old64's full two-material brick: x 40..43, y 24..27 (rows 24, 25: id 4; 26, 27: id 1), z 36..39


def test_a_whole_brick_rewritten_to_one_id(rt, cuda, old64):
    t, comp = patch_and_check(rt, cuda, old64, *_cube(*BRICK, 3), "brick to one id", compact=False)
    mask, kind, mat = _kinds(t)
    ni = int(t.node_indices([BRICK])[0])
    assert (kind[ni] in (K_BRICK, K_SOLID)) and mat[ni] == 3 and mask[ni] == np.uint64(0xFFFFFFFFFFFFFFFF)
    assert t.garbage()[1] == 64                                   # the old brick's run of 64 entries
    check_patched(rt, cuda, t, comp, "brick to one id, compacted", casts=False)
    ni = int(t.node_indices([BRICK])[0])
    assert _kinds(t)[1][ni] == K_SOLID                            # collapsing it is the compaction's job


def test_a_whole_brick_rewritten_to_mixed_ids(rt, cuda, old64):
    ids = np.random.default_rng(83).integers(0, 6, 64).astype(np.uint16)
    assert (ids == 0).any() and (ids == 5).any()
    patch_and_check(rt, cuda, old64, *_cube(*BRICK, ids), "brick to mixed ids")


def test_a_brick_edited_to_become_uniform(rt, cuda, old64):
    xyz, ids = _cube(*BRICK, 4)
    half = xyz[:, 1] >= 26                                        # only the voxels that held id 1
    t, comp = patch_and_check(rt, cuda, old64, np.ascontiguousarray(xyz[half]), np.ascontiguousarray(ids[half]), "brick made uniform",
                              compact=False)
    assert (comp[36:40, 24:28, 40:44] == 4).all()
    assert t.info().n_mat_bytes == _tree(rt, 3, old64).info().n_mat_bytes   # a one-material brick has no material run
    # the brick with a hole: filling the hole, and emptying all but one voxel
    t.patch_points(*_list([(23, 22, 21, 3)]))
    comp[21, 22, 23] = 3
    xyz, ids = _cube(20, 20, 20, 0)
    t.patch_points(np.ascontiguousarray(xyz[1:]), np.ascontiguousarray(ids[1:]))
    comp[20:24, 20:24, 20:24] = 0
    comp[20, 20, 20] = 3
    check_patched(rt, cuda, t, comp, "bricks made uniform")


def test_edits_on_the_faces_of_the_extent(rt, cuda, old64):
    rng = np.random.default_rng(84)
    ends = np.array([(x, y, z) for x in (0, 63) for y in (0, 63) for z in (0, 63)], np.int32)
    faces = rng.integers(0, 64, (120, 3)).astype(np.int32)
    faces[np.arange(120), np.arange(120) % 3] = np.where(np.arange(120) % 2, 63, 0)
    xyz = np.ascontiguousarray(np.concatenate([ends, faces]))
    ids = rng.integers(0, 5, len(xyz)).astype(np.uint16)
    patch_and_check(rt, cuda, old64, xyz, ids, "faces and corners")


def test_a_list_that_touches_every_brick_once(rt, cuda, old64):
    rng = np.random.default_rng(85)
    b = np.stack(np.meshgrid(np.arange(16), np.arange(16), np.arange(16), indexing="ij"), -1).reshape(-1, 3)
    xyz = np.ascontiguousarray((4 * b + rng.integers(0, 4, b.shape)).astype(np.int32)[rng.permutation(len(b))])
    ids = rng.integers(0, 6, len(xyz)).astype(np.uint16)
    assert len(np.unique(xyz // 4, axis=0)) == 4096
    patch_and_check(rt, cuda, old64, xyz, ids, "every brick once")


def test_two_levels(rt, cuda):
    """16^3: the anchor is the root and every touched child is a brick"""
    old = vc.random_volume((16, 16, 16), 0.3, 1)
    old[4:8, 8:12, 0:4] = 2                                       # a SOLID child of the root
    old[8:12, 0:4, 12:16] = 0                                     # an absent one
    rng = np.random.default_rng(86)
    xyz = rng.integers(0, 16, (200, 3)).astype(np.int32)
    ids = rng.integers(0, 6, 200).astype(np.uint16)
    for view in (0, 1):
        patch_and_check(rt, cuda, old, xyz, ids, "2 levels, view %d" % view, view=view, levels=2, casts=False)
    full = np.full((16, 16, 16), 3, np.uint16)
    t, comp = patch_and_check(rt, cuda, full, *_list([(0, 0, 0, 0), (15, 15, 15, 1)]), "2 levels, solid root", levels=2, casts=False)
    assert comp[0, 0, 0] == 0 and comp[15, 15, 15] == 1


# ------------------------------------------------------------------------------------------ 4. every builder's tree --
def _edits64(seed, n=400, top=5):
    rng = np.random.default_rng(seed)
    return rng.integers(0, 64, (n, 3)).astype(np.int32), rng.integers(0, top, n).astype(np.uint16)


def test_world_built_tree(rt, cuda):
    w = rt.World(3)
    rng = np.random.default_rng(71)
    pts = rng.integers(0, 64, (3000, 3))
    w.put_blocks(pts, np.zeros(len(pts), np.uint32), np.full(len(pts), int(vc.colour(3)), np.uint64))
    t = w.build().upload(0)
    assert t.info().n_materials == 2 and t.garbage() == (0, 0)
    before = _stored(t)
    xyz, ids = _edits64(91, top=2)
    t.patch_points(xyz, ids)
    comp = ppc.apply_edits(before, xyz, ids, ppc.view_keep(t.palette(), 0))
    check_patched(rt, cuda, t, comp, "world-built", compact=False)
    w.put_block(1, 1, 1, 0, int(vc.colour(3)))
    with pytest.raises(rt.SvoError, match=r"svo_tree_update failed \(-4\)"):
        t.update(w, [(1, 1, 1)])
    check_patched(rt, cuda, t, comp, "world-built, after the refused update", casts=False, compact=False)


def test_a_tree_with_unsynced_host_edits_is_refused(rt, cuda):
    w = rt.World(3)
    w.put_block(5, 6, 7, 0, int(vc.colour(3)))
    t = w.build().upload(0)
    w.put_block(9, 9, 9, 0, int(vc.colour(3)))
    t.update(w, [(9, 9, 9)])
    with pytest.raises(rt.SvoError, match=r"svo_tree_patch_points_gpu failed \(-4\).*not yet synced"):
        t.patch_points(*_list([(1, 1, 1, 1)]))
    t.sync()
    t.patch_points(*_list([(1, 1, 1, 1)]))
    assert t.get_block(1, 1, 1)[1] == 1 and t.get_block(9, 9, 9)[1] == 1


def test_terrain_built_tree(rt, cuda):
    x, z = np.meshgrid(np.arange(120), np.arange(120), indexing="ij")
    heights = (24 + 10 * np.sin(x / 9.0) + 8 * np.cos(z / 7.0)).astype(np.int32)
    t = rt.Tree.heightfield_gpu(4, heights)
    comp = _stored(t)
    keep = ppc.view_keep(t.palette(), t.info().view)
    solid = int(comp[comp != 0][0])
    rng = np.random.default_rng(92)
    xyz = np.ascontiguousarray(np.concatenate([rng.integers(0, 120, (600, 3)), rng.integers(0, 256, (200, 3))]).astype(np.int32))
    ids = np.where(rng.random(800) < 0.5, solid, 0).astype(np.uint16)
    t.patch_points(xyz, ids)
    comp = ppc.apply_edits(comp, xyz, ids, keep)
    check_patched(rt, cuda, t, comp, "terrain-built", shift=(30.0, 60.0, 30.0))


def test_points_built_tree(rt, cuda):
    vol, _ = vc.planted(37, 38, 41, (5, 2, 7), 4)
    pxyz, pids = pc.as_points(vol, (5, 2, 7), 93)
    t = rt.Tree.points_gpu(3, pxyz, pids, PAL)
    xyz, ids = _edits64(94)
    t.patch_points(xyz, ids)
    comp = ppc.apply_edits(vc.in_view(pc.dense(3, pxyz, pids), PAL, 0), xyz, ids, ppc.view_keep(PAL, 0))
    check_patched(rt, cuda, t, comp, "points-built")


def test_a_tree_already_patched_by_patch_volume(rt, cuda, old64):
    t = _tree(rt, 3, old64)
    t.patch_volume(np.zeros((20, 20, 20), np.uint16), (5, 6, 7))     # interiors with mask 0 may appear, and garbage
    t.patch_volume(vc.random_volume((9, 9, 9), 0.5, 61), (30, 2, 41))
    g0 = t.garbage()
    assert g0[0] > 0 and g0 == ppc.expected_garbage(t)
    before = _stored(t)
    xyz, ids = _edits64(95)
    xyz[:100] = np.random.default_rng(96).integers(5, 25, (100, 3))   # a hundred of them into the emptied box
    t.patch_points(xyz, ids)
    assert t.garbage()[0] > g0[0]
    check_patched(rt, cuda, t, ppc.apply_edits(before, xyz, ids, ppc.view_keep(PAL, 0)), "after patch_volume")


# ------------------------------------------------------------------------------------- 5. sequences and capacity --
def test_sequence_past_the_upload_slack(rt, cuda):
    E = 256
    comp = vc.random_volume((E, E, E), 0.02, 41, ids=(1, 2, 3, 4))
    t = _tree(rt, 4, comp)
    bytes_seen, garbage = [t.info().device_bytes], [t.garbage()]
    n0 = t.info().n_nodes
    keep = ppc.view_keep(PAL, 0)
    for i in range(12):
        rng = np.random.default_rng(100 + i)
        xyz = rng.integers(0, E, (400, 3)).astype(np.int32)
        ids = rng.integers(0, 5, 400).astype(np.uint16)
        t.patch_points(xyz, ids)
        comp = ppc.apply_edits(comp, xyz, ids, keep)
        bytes_seen.append(t.info().device_bytes)
        garbage.append(t.garbage())
        if i in (0, 5, 11):
            assert cuda.equal(t.read_volume((0, 0, 0), (E, E, E)), cuda.from_numpy(comp.view(np.int16)).cuda()), "(1) step %d" % i
    assert t.info().n_nodes > n0 + n0 // 8 + 65536                   # past the slack of the upload: the arrays were reallocated
    assert any(b > a for a, b in zip(bytes_seen, bytes_seen[1:]))
    assert all(b[0] > a[0] and b[1] >= a[1] for a, b in zip(garbage, garbage[1:])) and garbage[-1][1] > 0
    check_patched(rt, cuda, t, comp, "12 patches", casts=False)      # (compacts)
    xyz = np.random.default_rng(120).integers(0, E, (400, 3)).astype(np.int32)
    ids = np.random.default_rng(121).integers(0, 5, 400).astype(np.uint16)
    t.patch_points(xyz, ids)
    check_patched(rt, cuda, t, ppc.apply_edits(comp, xyz, ids, keep), "patched again after the compaction", casts=False)


# ---------------------------------------------------------------------------------------------------- 6. large ids --
WIDE = {
    # name: (the palette's table, volume_cases' ids 1..5 on its ids, further ids for the edits (the last without a colour))
    "65535 entries": (pcs.WIDE_TABLE, pcs.HIGH, (65533, 4096, pcs.WIDE_MIRROR, 0x8002)),
    "4097 entries": (pcs.WIDE_TABLE[:4097], (31, 32, 4095, 62, 4096), (64, 4094, 63)),
}


@pytest.mark.parametrize("view", [0, 1])
@pytest.mark.parametrize("case", sorted(WIDE))
def test_large_palettes(rt, cuda, case, view):
    table, lookup, more = WIDE[case]
    pal = pcs.stored_palette(table)
    assert len(pal) == (65535 if case == "65535 entries" else 4097) and max(lookup) == len(pal) - 1
    old = pcs.through(_old64(), lookup)
    rng = np.random.default_rng(87)
    xyz = rng.integers(0, 64, (600, 3)).astype(np.int32)
    ids = rng.choice(np.array((0,) + tuple(lookup) + tuple(more), np.uint16), 600)
    keep = ppc.view_keep(pal, view)
    assert not keep[more[-1]] and (ids == more[-1]).any() and (ids == len(pal) - 1).any()
    patch_and_check(rt, cuda, old, xyz, ids, "%s, view %d" % (case, view), view=view, pal=pal, casts=(view == 0))


# ----------------------------------------------------------------------------------------- 7. errors on the device --
BAD = {
    "an id equal to the palette size": ((7, 8, 9, len(PAL)), "palette"),
    "x equal to the extent": ((64, 8, 9, 1), "coordinate"),
    "a negative coordinate": ((7, -1, 9, 1), "coordinate"),
}


@pytest.mark.parametrize("case", sorted(BAD))
def test_bad_entries_change_nothing(rt, cuda, old64, case):
    t = _tree(rt, 3, old64)
    t.patch_points(*_edits64(97))                                    # (a tree that already carries garbage)
    nodes, mats = t.export()
    g, ceil, quads = t.garbage(), t.device_ceilings(), t.device_ceiling_quads()
    cam = rt.normalize((0.6, -0.45, 0.66))
    frame = {k: v.clone() for k, v in t.cast_frame((1.0, 2.0, 3.0), cam, 64, 32, 300).items() if k in ("pos_steps", "t", "info")}
    entry, names = BAD[case]
    xyz, ids = _edits64(98)
    xyz[211], ids[211] = entry[:3], entry[3]
    with pytest.raises(rt.SvoError, match=r"svo_tree_patch_points_gpu failed \(-5\).*" + names) as e:
        t.patch_points(xyz, ids)
    assert ("coordinate" if names == "palette" else "palette") not in str(e.value)
    n2, m2 = t.export()
    assert nodes.tobytes() == n2.tobytes() and mats.tobytes() == m2.tobytes() and t.garbage() == g
    c2 = t.device_ceilings()
    assert c2[0] == ceil[0] and np.array_equal(c2[1], ceil[1]) and np.array_equal(c2[2], ceil[2])
    assert np.array_equal(t.device_ceiling_quads(), quads)
    again = t.cast_frame((1.0, 2.0, 3.0), cam, 64, 32, 300)
    for k in frame:
        assert cuda.equal(frame[k], again[k]), k
    assert t.info().n_nodes == len(nodes)
    t.patch_points(*_edits64(98))                                    # the same list without the bad entry goes through


def test_an_empty_list_is_a_no_op(rt, cuda, old64):
    t = _tree(rt, 3, old64)
    t.patch_points(*_edits64(99))
    nodes, mats = t.export()
    g, times = t.garbage(), t.patch_times()
    assert t.patch_points(np.zeros((0, 3), np.int32), np.zeros(0, np.uint16)) is t
    assert rt.lib().svo_tree_patch_points_gpu(t._h, None, None, 0) == 0
    n2, m2 = t.export()
    assert nodes.tobytes() == n2.tobytes() and mats.tobytes() == m2.tobytes() and t.garbage() == g and t.patch_times() == times
    assert all(ms >= 0.0 for ms in times) and times[0] > 0.0


# ---------------------------------------------------------------------------------------------------- 8. 7 levels --
E7 = 4 ** 7
NEAR7 = (8200, 8200, 8200)


def _scatter7():
    """a few thousand points over the whole 16384^3 extent, a cluster of them around NEAR7 and a 64 x 64 plate below it for
    the casts to meet, a full one-material brick and a 16^3 of one material"""
    rng = np.random.default_rng(171)
    far = rng.integers(0, E7, (3000, 3))
    near = np.array(NEAR7) + rng.integers(-40, 40, (1500, 3))
    xyz = np.concatenate([far, near]).astype(np.int32)
    ids = rng.integers(1, 6, len(xyz)).astype(np.uint16)
    px, pz = np.meshgrid(np.arange(8160, 8224), np.arange(8160, 8224), indexing="ij")
    plate = np.stack([px.ravel(), np.full(px.size, 8150), pz.ravel()], 1)
    return pc.concat((xyz, ids), (plate, np.full(len(plate), 1, np.uint16)), _cube(8212, 8204, 8220, 2), _cube(8176, 8208, 8192, 4, 16))


@pytest.fixture(scope="module")
def scatter7():
    return _scatter7()


def _edits7(base, seed):
    """puts and erasures: scattered over the world, on stored voxels (half of them erased), and inside the planted cubes"""
    rng = np.random.default_rng(seed)
    stored = base[0][rng.integers(0, len(base[0]), 600)]
    far = rng.integers(0, E7, (500, 3))
    near = np.array(NEAR7) + rng.integers(-40, 40, (500, 3))
    cubes = np.array([(8213, 8205, 8221), (8180, 8210, 8199), (8191, 8223, 8207)])
    ends = np.array([(0, 0, 0), (E7 - 1, E7 - 1, E7 - 1), (E7 - 1, 0, 5)])
    xyz = np.concatenate([stored, far, near, cubes, ends, stored[:50]]).astype(np.int32)
    ids = rng.integers(0, 6, len(xyz)).astype(np.uint16)
    ids[:300] = 0
    return np.ascontiguousarray(xyz), ids


@pytest.mark.parametrize("view", [0, 1])
def test_seven_levels(rt, cuda, scatter7, view):
    t = rt.Tree.points_gpu(7, *scatter7, PAL, view=view)
    xyz, ids = _edits7(scatter7, 172)
    t.patch_points(xyz, ids)                 # succeeds where no dense box of the extent could exist
    keep = ppc.view_keep(PAL, view)
    # (1) the model: the merged list, last entry wins
    merged = pc.concat(scatter7, (xyz, ids))
    mx, mi = ppc.resolve_edits(*merged, keep)
    model = {tuple(p): int(i) for p, i in zip(mx.tolist(), mi.tolist())}
    rng = np.random.default_rng(173)
    where = np.ascontiguousarray(np.concatenate([xyz, ppc.neighbours26(xyz, E7), rng.integers(0, E7, (10000, 3)).astype(np.int32),
                                                 scatter7[0]]).astype(np.int32))
    got = t.get_blocks_gpu(where).cpu().numpy().view(np.uint16)
    want = np.array([model.get(tuple(p), 0) for p in where.tolist()], np.uint16)
    assert np.array_equal(got, want), "(1) %d positions differ" % int((got != want).sum())
    assert (want[:len(xyz)] == 0).any() and (want[:len(xyz)] != 0).any()
    assert t.garbage() == ppc.expected_garbage(t) and t.garbage()[0] > 0, "(5)"
    mask, kind, _ = _kinds(t)
    assert not ((kind == K_BRICK) & (mask == 0)).any()
    fresh = rt.Tree.points_gpu(7, *merged, PAL, view=view)
    _same_ceilings(t, fresh, "(3) 7 levels")
    if view == 0:
        assert check_casts(rt, cuda, t, fresh, "(4) 7 levels", shift=tuple(float(c - 30) for c in NEAR7)) > 0
    t.compact()
    _same(t, fresh, "(2) 7 levels")
    _same_ceilings(t, fresh, "(3) 7 levels, compacted")
    assert t.garbage() == (0, 0)


def test_work_bounds(rt, cuda, scatter7):
    """deterministic: the growth follows the edits, whatever the extent"""
    levels = 7
    t = rt.Tree.points_gpu(levels, *scatter7, PAL)
    i0 = t.info()
    t.patch_points(*_list([(12345, 6789, 4321, 1)]))
    i1 = t.info()
    assert 0 < i1.n_nodes - i0.n_nodes <= 64 * (levels - 1)
    assert i1.n_mat_bytes - i0.n_mat_bytes <= 2 * 64
    assert int(t.get_blocks_gpu(np.array([(12345, 6789, 4321)], np.int32)).cpu().numpy().view(np.uint16)[0]) == 1
    # one edit into a stored mixed brick: the whole brick is re-emitted, and no more
    p = scatter7[0][7]
    t.patch_points(*_list([(int(p[0]) ^ 1, int(p[1]), int(p[2]), 3)]))
    i2 = t.info()
    assert 0 < i2.n_nodes - i1.n_nodes <= 64 * (levels - 1) and i2.n_mat_bytes - i1.n_mat_bytes <= 2 * 64
    # k edits in k distinct bricks
    rng = np.random.default_rng(174)
    xyz = rng.integers(0, E7, (1000, 3)).astype(np.int32)
    k = len(np.unique(xyz // 4, axis=0))
    assert k == 1000
    t.patch_points(xyz, rng.integers(1, 5, 1000).astype(np.uint16))
    i3 = t.info()
    assert 0 < i3.n_nodes - i2.n_nodes <= k * 64 * (levels - 1)
    assert i3.n_mat_bytes - i2.n_mat_bytes <= k * 2 * 64
    assert t.garbage() == ppc.expected_garbage(t)
