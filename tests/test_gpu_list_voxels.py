"""svo_tree_list_voxels_gpu (Tree.list_voxels / Tree.count_voxels) against numpy models of the content: volume-built trees
of 2 and 3 levels in both views with every record shape planted, boxes on and off every grid of the tree, the layouts the
patches leave behind and their compaction, the round trip through svo_build_points_gpu, one-level and empty trees, a
7-level points-built tree whose dense read-back does not exist, a 7-level K_SOLID root counted in closed form and
unranked through seven levels, the capacity rules and a side stream.  Every comparison is exact."""
import ctypes as C

import numpy as np
import pytest

import list_voxels_cases as lv
import points_cases as pc
import volume_cases as vc

pytestmark = pytest.mark.gpu

EMPTY = (0, 0xFFFFFFFFFFFFFFFF, 0.0)
PAL = [EMPTY] + [(1 | f, c, 0.0) for f, c in vc.TABLE[1:]]
LIQUID = 5
K_INTERIOR, K_BRICK, K_SOLID, K_UNIFORM = 0, 1, 2, 4
ERANGE = -5
FULL = np.uint64(0xFFFFFFFFFFFFFFFF)


@pytest.fixture(scope="module")
def cuda(rt):
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    assert hasattr(rt.lib(), "svo_tree_list_voxels_gpu")
    return torch


def _np(pair):
    xyz, ids = pair
    return xyz.cpu().numpy(), ids.cpu().numpy().view(np.uint16)


def _same_list(got, want, levels, label):
    (gx, gi), (wx, wi) = got, want
    assert gx.shape == wx.shape and gi.shape == wi.shape, "%s: %d entries, the model has %d" % (label, len(gi), len(wi))
    assert gx.dtype == np.int32 and gi.dtype == np.uint16
    assert np.array_equal(gx, wx), "%s: %d positions differ" % (label, int((gx != wx).any(1).sum()))
    assert np.array_equal(gi, wi), "%s: %d ids differ" % (label, int((gi != wi).sum()))
    assert (np.diff(lv.key_of(gx, levels)) > 0).all(), "%s: the keys do not increase strictly" % label


def _kinds(tree):
    n, _ = tree.export()
    return n[:, 0], (n[:, 1] >> np.uint64(32)) & np.uint64(7), n[:, 1] >> np.uint64(48)


def _vol3():
    """64^3 at density 0.3 with an aligned 16^3 of one id (K_SOLID above brick depth), a full one-material brick, a
    partial one-material brick (K_UNIFORM), an empty 16^3 region and liquid voxels"""
    vol = vc.random_volume((64, 64, 64), 0.3, 301)
    vol[32:48, 16:32, 0:16] = 2      # x 0..15, y 16..31, z 32..47
    vol[4:8, 4:8, 20:24] = 3         # x 20..23, y 4..7, z 4..7
    vol[8:12, 4:8, 20:24] = 4        # x 20..23, y 4..7, z 8..11, with a voxel missing
    vol[9, 5, 22] = 0
    vol[48:64, 48:64, 48:64] = 0
    vol[1, 1, 1] = LIQUID
    return vol


@pytest.fixture(scope="module")
def vol3():
    v = _vol3()
    v.setflags(write=False)
    return v


def _state(t):
    nodes, mats = t.export()
    lvl, ceil, pairs = t.device_ceilings()
    return nodes.copy(), mats.copy(), t.garbage(), lvl, ceil.copy(), pairs.copy(), t.device_ceiling_quads().copy()


def _same_state(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


@pytest.fixture(scope="module")
def tree3(rt, cuda, vol3):
    """the 3-level tree of vol3 in the full view, its content, and its state before any listing"""
    t = rt.Tree.volume_gpu(3, np.array(vol3), PAL, view=1)
    mask, kind, mat = _kinds(t)
    at = [int(i) for i in t.node_indices([(5, 20, 40), (21, 5, 5), (21, 5, 9)])]
    assert kind[at[0]] == K_SOLID and kind[at[1]] == K_SOLID and at[0] != at[1]     # at depth 1 and at brick depth
    assert kind[at[2]] == (K_BRICK | K_UNIFORM) and mask[at[2]] != FULL
    return t, vc.in_view(np.asarray(vol3), PAL, 1), _state(t)


# ------------------------------------------------------------------------------------------------ 1. whole extent --
@pytest.mark.parametrize("view", [0, 1])
@pytest.mark.parametrize("levels", [2, 3])
def test_whole_extent(rt, cuda, vol3, levels, view):
    vol = np.array(vol3) if levels == 3 else vc.random_volume((16, 16, 16), 0.3, 300)
    t = rt.Tree.volume_gpu(levels, vol, PAL, view=view)
    got = _np(t.list_voxels())
    want = lv.model(vc.in_view(vol, PAL, view))
    _same_list(got, want, levels, "levels %d view %d" % (levels, view))
    assert t.count_voxels() == len(want[1]) > 0
    assert (vol == LIQUID).any() and bool((got[1] == LIQUID).any()) == (view == 1)


# -------------------------------------------------------------------------------------------------------- 2. boxes --
BOXES = {  # origin (x, y, z), shape (nz, ny, nx)
    "a stored voxel": ((5, 20, 40), (1, 1, 1)),
    "an empty voxel": ((50, 50, 50), (1, 1, 1)),
    "exactly one brick": ((20, 4, 8), (4, 4, 4)),
    "off the grid on every axis": ((9, 13, 6), (21, 18, 27)),
    "strictly inside the 16^3 solid": ((3, 18, 35), (9, 11, 10)),
    "cutting the solid and its neighbours": ((10, 10, 28), (25, 30, 20)),
    "the slab x = 63": ((63, 0, 0), (64, 64, 1)),
    "the slab z = 0": ((0, 0, 0), (1, 64, 64)),
    "the whole extent, given": ((0, 0, 0), (64, 64, 64)),
}


@pytest.mark.parametrize("box", sorted(BOXES))
def test_boxes(rt, cuda, tree3, box):
    t, content, _ = tree3
    origin, shape = BOXES[box]
    xyz, ids = t.list_voxels(origin, shape)
    assert xyz.dtype == cuda.int32 and ids.dtype == cuda.int16 and xyz.is_cuda and ids.is_cuda
    want = lv.model(content, origin, shape)
    _same_list(_np((xyz, ids)), want, 3, box)
    assert t.count_voxels(origin, shape) == len(want[1])
    if box == "a stored voxel":
        assert len(want[1]) == 1
    if box == "an empty voxel":
        assert tuple(xyz.shape) == (0, 3) and tuple(ids.shape) == (0,)
    if box == "exactly one brick":
        assert len(want[1]) == 63 and (want[1] == 4).all()
    if box == "strictly inside the 16^3 solid":
        assert len(want[1]) == 9 * 11 * 10 and (want[1] == 2).all()
    if box == "the whole extent, given":
        assert cuda.equal(xyz, t.list_voxels()[0])


# ----------------------------------------------------------------------------------- 3. layouts the patches leave --
BRICK_A, BRICK_B = (40, 40, 40), (44, 40, 40)   # outside the patch box and the solid


def _cube(x0, y0, z0, ids, s=4):
    z, y, x = np.meshgrid(np.arange(s), np.arange(s), np.arange(s), indexing="ij")
    xyz = np.stack([x.ravel() + x0, y.ravel() + y0, z.ravel() + z0], 1).astype(np.int32)
    return xyz, np.broadcast_to(np.asarray(ids, np.uint16), (s ** 3,)).copy()


def _patched(rt):
    """test_gpu_tree_lookup's patched volume tree (the same volume, box and origin), then a patch_points that completes
    BRICK_A to one material and leaves BRICK_B one voxel, and one that erases that voxel: (tree, composite content)"""
    vol = vc.random_volume((64, 64, 64), 0.3, 85)
    vol[16:32, 16:32, 16:32] = 2
    vol[0:16, 0:16, 0:16] = 0
    vol[8:14, 13:16, 10:15] = 1
    t = rt.Tree.volume_gpu(3, vol, PAL, view=1)
    box = vc.random_volume((21, 18, 27), 0.4, 86)
    box[0:10, 0:3, 0:7] = 0
    at = (9, 13, 6)
    t.patch_volume(box, at)
    comp = vol.copy()
    comp[at[2]:at[2] + 21, at[1]:at[1] + 18, at[0]:at[0] + 27] = box
    assert t.garbage()[0] > 0 and t.garbage()[1] > 0            # superseded records and material entries
    mask, kind, _ = _kinds(t)
    assert ((mask == 0) & (kind == K_INTERIOR)).any()           # an interior record with mask 0

    a = _cube(*BRICK_A, 3)
    bx, bi = _cube(*BRICK_B, 0)
    bi[0] = 1                                                   # BRICK_B keeps its first voxel alone
    t.patch_points(*pc.concat(a, (bx, bi)))
    comp[40:44, 40:44, 40:44] = 3
    comp[40:44, 40:44, 44:48] = 0
    comp[40, 40, 44] = 1
    mask, kind, mat = _kinds(t)
    na, nb = (int(i) for i in t.node_indices([BRICK_A, BRICK_B]))
    assert kind[na] == (K_BRICK | K_UNIFORM) and mask[na] == FULL and mat[na] == 3      # full, one material, still a brick
    assert (kind[nb] & np.uint64(3)) == K_BRICK and mask[nb] == np.uint64(1)
    t.patch_points(np.array([BRICK_B], np.int32), np.zeros(1, np.uint16))                # its last voxel goes
    comp[40, 40, 44] = 0
    assert t.get_block(*BRICK_B)[1] == 0
    return t, vc.in_view(comp, PAL, 1)


def test_patched_layouts_and_their_compaction(rt, cuda):
    t, comp = _patched(rt)
    before = _state(t)
    want = lv.model(comp)
    first = _np(t.list_voxels())
    _same_list(first, want, 3, "patched")
    assert t.count_voxels() == len(want[1])
    origin, shape = (9, 13, 6), (21, 18, 27)
    _same_list(_np(t.list_voxels(origin, shape)), lv.model(comp, origin, shape), 3, "patched, the patch's box")
    assert _same_state(before, _state(t))                       # the tree is only read
    t.compact()
    assert t.garbage() == (0, 0)
    second = _np(t.list_voxels())
    _same_list(second, want, 3, "compacted")
    assert np.array_equal(first[0], second[0]) and np.array_equal(first[1], second[1])


# --------------------------------------------------------------------------------------------------- 4. round trip --
def _same_tree(a, b, label):
    (na, ma), (nb, mb) = a.export(), b.export()
    assert np.array_equal(na, nb) and np.array_equal(ma, mb), label
    ia, ib = a.info(), b.info()
    assert list(ia.nodes_per_level) == list(ib.nodes_per_level) and ia.n_bricks == ib.n_bricks and ia.n_mat_bytes == ib.n_mat_bytes, label


def test_round_trip_of_the_patched_tree(rt, cuda):
    t, _ = _patched(rt)
    xyz, ids = t.list_voxels()
    back = rt.Tree.points_gpu(3, xyz, ids, t.palette(), 1)
    t.compact()
    _same_tree(back, t, "patched tree")


def test_round_trip_of_a_terrain_tree(rt, cuda):
    t = rt.Tree.terrain_gpu(4, 200, 200, 0)
    xyz, ids = t.list_voxels()
    dense = t.read_volume((0, 0, 0), (256, 256, 256)).cpu().numpy().view(np.uint16)
    want = lv.model(dense)
    _same_list(_np((xyz, ids)), want, 4, "terrain")
    assert len(want[1]) > 0
    back = rt.Tree.points_gpu(4, xyz, ids, t.palette(), t.info().view)
    t.compact()
    _same_tree(back, t, "terrain")


# ----------------------------------------------------------------------------------------- 5. one level, and empty --
def test_one_level(rt, cuda):
    w = rt.World(1)
    put = [(0, 0, 0, 1), (3, 1, 2, 2), (1, 3, 3, 1), (2, 2, 0, 3)]
    for x, y, z, i in put:
        w.put_block(x, y, z, *vc.TABLE[i])
    t = w.build().upload(0)
    z, y, x = np.meshgrid(np.arange(4), np.arange(4), np.arange(4), indexing="ij")
    every = np.stack([x.ravel(), y.ravel(), z.ravel()], 1).astype(np.int32)
    stored = t.get_blocks(every)
    assert (stored != 0).sum() == len(put)
    want = lv.by_key(every[stored != 0], stored[stored != 0], 1)
    _same_list(_np(t.list_voxels()), want, 1, "one level")
    assert t.count_voxels() == len(put) and t.count_voxels((3, 1, 2), (1, 1, 1)) == 1 and t.count_voxels((0, 1, 0), (1, 1, 4)) == 0


def test_empty_world(rt, cuda):
    t = rt.World(3).build().upload(0)
    assert t.count_voxels() == 0 and t.count_voxels((1, 2, 3), (4, 5, 6)) == 0
    xyz, ids = t.list_voxels()
    assert tuple(xyz.shape) == (0, 3) and tuple(ids.shape) == (0,)


# --------------------------------------------------------------------------------------- 6. seven levels, content --
CUBE7 = (4096, 8192, 12288)


@pytest.fixture(scope="module")
def scatter7(rt, cuda):
    """a 7-level points-built tree (full view): 50,000 seeded points over the whole 16384^3 extent, an aligned 64^3 cube
    of one id given as points, and a few duplicate and erased entries; with the list it was built from"""
    rng = np.random.default_rng(707)
    p = rng.integers(0, 16384, (50000, 3)).astype(np.int32)
    i = rng.integers(1, 6, 50000).astype(np.uint16)
    cube = _cube(*CUBE7, 4, s=64)
    again = (p[:200], ((i[:200] % 5) + 1).astype(np.uint16))            # duplicates: the last entry decides
    erased = (p[200:300], np.zeros(100, np.uint16))                      # erased scatter points
    hole = (np.array([(CUBE7[0] + 70, CUBE7[1] + 1, CUBE7[2] + 2)], np.int32), np.array([3], np.uint16))
    unhole = (hole[0], np.zeros(1, np.uint16))                           # put, then erased again
    xyz, ids = pc.concat((p, i), cube, again, erased, hole, unhole)
    t = rt.Tree.points_gpu(7, xyz, ids, PAL, 1)
    _, kind, mat = _kinds(t)
    n = int(t.node_indices([(CUBE7[0] + 9, CUBE7[1] + 9, CUBE7[2] + 9)])[0])
    assert kind[n] == K_SOLID and mat[n] == 4                            # the cube collapsed
    return t, lv.survivors(xyz, ids, 7)


def test_seven_levels_whole_extent(rt, cuda, scatter7):
    t, want = scatter7
    assert 64 ** 3 + 49000 < len(want[1]) <= 64 ** 3 + 50000
    _same_list(_np(t.list_voxels()), want, 7, "7 levels")
    assert t.count_voxels() == len(want[1])
    assert t.count_voxels((0, 0, 0), (16384, 16384, 16384)) == len(want[1])


def test_seven_levels_box_cutting_the_cube(rt, cuda, scatter7):
    t, want = scatter7
    origin, shape = (CUBE7[0] - 5, CUBE7[1] + 3, CUBE7[2] + 37), (50, 40, 30)
    inside = lv.in_box(*want, origin, shape)
    assert 25 * 40 * 27 <= len(inside[1]) <= 25 * 40 * 27 + 10           # the part of the cube, and whatever scatter fell in
    _same_list(_np(t.list_voxels(origin, shape)), inside, 7, "7 levels, a box cutting the cube")
    assert t.count_voxels(origin, shape) == len(inside[1])


# --------------------------------------------------------------------------------------- 7. seven levels, uniform --
def test_seven_levels_solid_root(rt, cuda):
    w = rt.World(7)
    w.put_block(0, 0, 0, *vc.TABLE[1], level=1)
    t = w.build().upload(0)
    nodes = t.export()[0]
    assert len(nodes) == 1 and ((int(nodes[0, 1]) >> 32) & 3) == K_SOLID
    assert t.count_voxels() == 2 ** 42
    assert t.count_voxels((5, 6, 7), (3000, 2000, 1000)) == 6 * 10 ** 9
    with pytest.raises(rt.SvoError, match=r"\(-5\).*2\^31"):
        t.list_voxels((5, 6, 7), (3000, 2000, 1000))
    origin, shape = (4093, 8190, 12287), (110, 90, 100)      # straddles region boundaries of several levels on each axis
    xyz, ids = _np(t.list_voxels(origin, shape))
    assert len(ids) == 990000
    z, y, x = np.meshgrid(np.arange(110), np.arange(90), np.arange(100), indexing="ij")
    grid = np.stack([x.ravel() + origin[0], y.ravel() + origin[1], z.ravel() + origin[2]], 1).astype(np.int32)
    the_id = int(t.get_blocks(np.array([origin], np.int32))[0])
    assert the_id != 0
    _same_list((xyz, ids), lv.by_key(grid, np.full(len(grid), the_id, np.uint16), 7), 7, "unranked through seven levels")


# ------------------------------------------------------------------------------------------------------ 8. capacity --
def _buffers(cuda, cap):
    return cuda.full((cap, 3), -1, dtype=cuda.int32, device="cuda:0"), cuda.full((cap,), -1, dtype=cuda.int16, device="cuda:0")


def test_capacity(rt, cuda, tree3):
    t, content, _ = tree3
    origin, shape = (9, 13, 6), (21, 18, 27)
    want = lv.model(content, origin, shape)
    need = len(want[1])
    assert need > 64
    xyz, ids = _buffers(cuda, need - 1)                          # one entry short
    n = C.c_int64(-7)
    o = (C.c_int32 * 3)(*origin)
    rc = rt.lib().svo_tree_list_voxels_gpu(t._h, o, shape[2], shape[1], shape[0], C.c_void_p(xyz.data_ptr()), C.c_void_p(ids.data_ptr()),
                                           need - 1, C.byref(n), None)
    cuda.cuda.synchronize()
    assert rc == ERANGE and n.value == need
    assert "svo_tree_list_voxels_gpu" in rt.lib().svo_last_error().decode()
    assert bool((xyz == -1).all()) and bool((ids == -1).all())  # nothing written
    with pytest.raises(rt.SvoError, match=r"\(-5\)"):
        t.list_voxels(origin, shape, out=(xyz, ids))
    for extra in (0, 5):
        xyz, ids = _buffers(cuda, need + extra)
        gx, gi = t.list_voxels(origin, shape, out=(xyz, ids))
        assert gx.data_ptr() == xyz.data_ptr() and gi.data_ptr() == ids.data_ptr() and len(gx) == len(gi) == need
        _same_list(_np((gx, gi)), want, 3, "capacity n + %d" % extra)
        assert bool((xyz[need:] == -1).all()) and bool((ids[need:] == -1).all())


def test_out_is_validated(rt, cuda, tree3):
    t, _, _ = tree3
    xyz, ids = _buffers(cuda, 100)
    bad = [
        (xyz.to(cuda.int64), ids),                                           # dtypes
        (xyz, ids.to(cuda.int32)),
        (xyz.reshape(3, 100), ids),                                          # shapes
        (xyz.reshape(-1), ids),
        (xyz, ids[:99]),
        (xyz, ids.reshape(100, 1)),
        (cuda.zeros((100, 6), dtype=cuda.int32, device="cuda:0")[:, ::2], ids),  # not contiguous
        (xyz.cpu(), ids),                                                    # devices
        (xyz, ids.cpu()),
    ]
    for pair in bad:
        with pytest.raises(ValueError, match="out"):
            t.list_voxels((0, 0, 0), (4, 4, 4), out=pair)
    for out in (xyz, (xyz,), (xyz, ids, ids), (xyz, None)):
        with pytest.raises(ValueError, match="out"):
            t.list_voxels((0, 0, 0), (4, 4, 4), out=out)


# -------------------------------------------------------------------------------------------------------- 9. stream --
def test_callers_buffers_on_another_stream(rt, cuda, tree3):
    t, content, before = tree3                                  # (before: ahead of every call of the tests above)
    want = lv.model(content)
    s = cuda.cuda.Stream()
    with cuda.cuda.stream(s):
        xyz, ids = _buffers(cuda, len(want[1]) + 3)
        gx, gi = t.list_voxels(out=(xyz, ids), stream=s)
        got = _np((gx, gi))                                      # (the call has waited for its stream: no synchronize)
    _same_list(got, want, 3, "side stream")
    assert t.count_voxels() == len(want[1])
    assert _same_state(before, _state(t))                       # host image, garbage and device ceilings as they were
