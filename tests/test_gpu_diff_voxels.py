"""svo_tree_diff_gpu (Tree.diff_voxels / Tree.count_diff) against numpy models of the two contents: a pair of 3-level
volume-built trees whose 16^3 cells cross six record shapes on the two sides, the listing's boxes on that pair, the
equalities with the listing (the diff of an empty tree against t is t's listing), the two views of one world, the layouts
the patches leave, the contract with svo_tree_patch_points_gpu (patching a with diff(a, b) and compacting gives b's bytes),
7-level trees whose dense volumes do not exist, a 7-level K_SOLID root counted in closed form, the capacity rules, a side
stream, and both trees unchanged by all of it.  Every comparison is exact and in order."""
import ctypes as C

import numpy as np
import pytest

import diff_voxels_cases as dm
import list_voxels_cases as lv
import points_cases as pc
import test_gpu_list_voxels as tl  # its helpers, boxes and patched tree (nothing of it is collected from here)
import volume_cases as vc

pytestmark = pytest.mark.gpu

PAL, LIQUID = tl.PAL, tl.LIQUID
K_BRICK, K_SOLID, K_UNIFORM = tl.K_BRICK, tl.K_SOLID, tl.K_UNIFORM
ERANGE, ESTATE = -5, -4
NAME = "svo_tree_diff_gpu"


@pytest.fixture(scope="module")
def cuda(rt):
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    assert hasattr(rt.lib(), NAME) and hasattr(rt.Tree, "diff_voxels")
    return torch


def _same(got, want, levels, label):
    """tl._same_list: shapes, dtypes, positions, ids, and the strict increase of the key"""
    tl._same_list(tl._np(got), want, levels, label)


def _diff_both_ways(a, b, va, vb, levels, label, origin=None, shape=None):
    for x, y, vx, vy, way in ((a, b, va, vb, "a -> b"), (b, a, vb, va, "b -> a")):
        want = dm.model(vx, vy, origin, shape)
        _same(x.diff_voxels(y, origin, shape), want, levels, "%s, %s" % (label, way))
        assert x.count_diff(y, origin, shape) == len(want[1])
    return len(want[1])


# ------------------------------------------------------------------------------------------ 1. record shapes crossed --
EMPTY, SOLID2, SOLID3, RANDOM, BRICKS, CHANGED = range(6)
FIRST_CELL = 28   # pair p = 6 * shape_a + shape_b lies in the 16^3 cell 28 + p (cell c at (c & 3, (c >> 2) & 3, c >> 4))


def _cell(shape, c):
    rnd = vc.random_volume((16, 16, 16), 0.3, 900 + c)
    if shape == EMPTY:
        return np.zeros((16, 16, 16), np.uint16)
    if shape in (SOLID2, SOLID3):
        return np.full((16, 16, 16), 2 if shape == SOLID2 else 3, np.uint16)
    if shape == RANDOM:
        return rnd
    if shape == BRICKS:                                 # one full one-material brick, one partial one
        v = np.zeros((16, 16, 16), np.uint16)
        v[0:4, 0:4, 0:4] = 3
        v[4:8, 0:4, 0:4] = 4
        v[5, 1, 2] = 0
        return v
    v = rnd.copy()                                      # CHANGED: five voxels of the random content
    stored = np.argwhere((rnd != 0) & (rnd != LIQUID))
    free = np.argwhere(rnd == 0)
    v[tuple(stored[0])] = 0                             # erased
    v[tuple(free[0])] = 1                               # added
    v[tuple(stored[1])] = LIQUID                        # a liquid id
    for at in (stored[2], stored[3]):                   # another solid id
        v[tuple(at)] = rnd[tuple(at)] % 4 + 1
    assert (v != rnd).sum() == 5
    return v


def _cell_origin(c):
    return 16 * (c & 3), 16 * ((c >> 2) & 3), 16 * (c >> 4)


def _pair_volumes():
    va, vb = np.zeros((64, 64, 64), np.uint16), np.zeros((64, 64, 64), np.uint16)
    for c in range(64):
        x, y, z = _cell_origin(c)
        p = c - FIRST_CELL
        if p >= 0:
            va[z:z + 16, y:y + 16, x:x + 16] = _cell(p // 6, c)
            vb[z:z + 16, y:y + 16, x:x + 16] = _cell(p % 6, c)
        elif c % 2:                                     # equal random content in both
            va[z:z + 16, y:y + 16, x:x + 16] = vb[z:z + 16, y:y + 16, x:x + 16] = _cell(RANDOM, c)
    return va, vb


def _cell_of(shape_a, shape_b):
    return FIRST_CELL + 6 * shape_a + shape_b


@pytest.fixture(scope="module")
def pair3(rt, cuda):
    """the two 3-level trees (full view), their volumes, and their states before any diff"""
    va, vb = _pair_volumes()
    a, b = rt.Tree.volume_gpu(3, va, PAL, view=1), rt.Tree.volume_gpu(3, vb, PAL, view=1)
    for t, side in ((a, 0), (b, 1)):                    # the shapes are really there, on either side
        mask, kind, mat = tl._kinds(t)
        cell = lambda s: _cell_origin(_cell_of(s, s) if s != SOLID3 else (_cell_of(s, EMPTY) if side == 0 else _cell_of(EMPTY, s)))
        x, y, z = cell(SOLID2)
        solid = int(t.node_indices([(x + 5, y + 5, z + 5)])[0])
        x, y, z = cell(SOLID3)
        solid3 = int(t.node_indices([(x + 5, y + 5, z + 5)])[0])
        x, y, z = cell(BRICKS)
        full, part = (int(i) for i in t.node_indices([(x + 1, y + 1, z + 1), (x + 1, y + 1, z + 5)]))
        assert kind[solid] == K_SOLID and mat[solid] == 2 and kind[solid3] == K_SOLID and mat[solid3] == 3
        assert kind[full] == K_SOLID and mat[full] == 3                               # a full brick: K_SOLID at brick depth
        assert kind[part] == (K_BRICK | K_UNIFORM) and mask[part] != tl.FULL and mat[part] == 4
        x, y, z = cell(RANDOM)
        mixed = int(t.node_indices([(x, y, z)])[0])
        assert kind[mixed] in (K_BRICK, K_BRICK | K_UNIFORM)
    va.setflags(write=False)
    vb.setflags(write=False)
    return a, b, va, vb, (tl._state(a), tl._state(b))


def test_record_shapes_crossed(rt, cuda, pair3):
    a, b, va, vb, _ = pair3
    n = _diff_both_ways(a, b, va, vb, 3, "whole extent")
    assert n > 10 * 16 ** 3                             # (18 of the pairs set a solid cell against something else)
    got = tl._np(a.diff_voxels(b))[1]
    assert (got == 0).any() and (got == LIQUID).any()


# -------------------------------------------------------------------------------------------------------- 2. boxes --
BOXES = dict(tl.BOXES)
BOXES["inside an equal random cell"] = (tuple(np.add(_cell_origin(_cell_of(RANDOM, RANDOM)), (2, 3, 1))), (9, 8, 10))
BOXES["cutting changed cells"] = ((9, 13, 38), (21, 18, 27))


@pytest.mark.parametrize("box", sorted(BOXES))
def test_boxes(rt, cuda, pair3, box):
    a, b, va, vb, _ = pair3
    origin, shape = BOXES[box]
    n = _diff_both_ways(a, b, va, vb, 3, box, origin, shape)
    if box == "strictly inside the 16^3 solid":           # cell 36: solid 2 against solid 3
        assert n == 9 * 11 * 10 and bool((a.diff_voxels(b, origin, shape)[1] == 3).all())
    if box in ("an empty voxel", "inside an equal random cell"):   # cells equal on both sides
        assert n == 0
        xyz, ids = a.diff_voxels(b, origin, shape)
        assert tuple(xyz.shape) == (0, 3) and tuple(ids.shape) == (0,)
    if box == "cutting changed cells":
        assert n > 64


# --------------------------------------------------------------------------------------------------- 3. equalities --
def _one_level(rt):
    w = rt.World(1)
    for x, y, z, i in [(0, 0, 0, 1), (3, 1, 2, 2), (1, 3, 3, 1), (2, 2, 0, 3)]:
        w.put_block(x, y, z, *vc.TABLE[i])
    return w.build().upload(0)


@pytest.mark.parametrize("levels", [1, 2, 3])
def test_equalities_with_the_listing(rt, cuda, pair3, levels):
    if levels == 1:
        t, box = _one_level(rt), ((0, 0, 0), (3, 2, 2))
    elif levels == 2:
        t, box = rt.Tree.volume_gpu(2, vc.random_volume((16, 16, 16), 0.3, 300), PAL, view=1), ((1, 0, 2), (9, 7, 5))
    else:
        t, box = pair3[0], BOXES["cutting changed cells"]
    empty = rt.World(levels).build().upload(0)
    for origin, shape in ((None, None), box):
        assert t.count_diff(t, origin, shape) == 0 and empty.count_diff(empty, origin, shape) == 0
        xyz, ids = t.diff_voxels(t, origin, shape)
        assert tuple(xyz.shape) == (0, 3) and tuple(ids.shape) == (0,)
        lx, li = t.list_voxels(origin, shape)
        dx, di = empty.diff_voxels(t, origin, shape)       # the listing is diff(empty, t), bit for bit
        assert len(li) > 0 and cuda.equal(dx, lx) and cuda.equal(di, li)
        ex, ei = t.diff_voxels(empty, origin, shape)       # the same positions erased
        assert cuda.equal(ex, lx) and ei.shape == li.shape and bool((ei == 0).all())
        assert t.count_diff(empty, origin, shape) == empty.count_diff(t, origin, shape) == t.count_voxels(origin, shape)


# -------------------------------------------------------------------------------------------------------- 4. views --
def test_views_differ_in_the_liquid(rt, cuda):
    vol = np.array(tl._vol3())
    vol[40:44, 40:44, 40:44] = LIQUID                    # a whole brick of liquid besides the scattered voxels
    solid, full = rt.Tree.volume_gpu(3, vol, PAL, view=0), rt.Tree.volume_gpu(3, vol, PAL, view=1)
    z, y, x = np.nonzero(vol == LIQUID)
    liquid = lv.by_key(np.stack([x, y, z], 1), np.full(len(x), LIQUID, np.uint16), 3)
    assert len(x) > 64
    _same(solid.diff_voxels(full), liquid, 3, "solid view -> full view")
    _same(full.diff_voxels(solid), (liquid[0], np.zeros(len(x), np.uint16)), 3, "full view -> solid view")
    assert solid.count_diff(full) == full.count_diff(solid) == len(x)
    want = dm.model(vc.in_view(vol, PAL, 0), vc.in_view(vol, PAL, 1))
    assert np.array_equal(want[0], liquid[0]) and np.array_equal(want[1], liquid[1])


# ------------------------------------------------------------------------------------ 5. layouts the patches leave --
def test_patched_layouts(rt, cuda):
    t, comp = tl._patched(rt)                            # records with mask 0, a full brick that stayed one, superseded records
    twin, _ = tl._patched(rt)
    twin.compact()
    assert t.garbage()[0] > 0 and twin.garbage() == (0, 0)
    before = tl._state(t), tl._state(twin)
    assert t.count_diff(twin) == 0 and twin.count_diff(t) == 0
    assert tuple(t.diff_voxels(twin)[0].shape) == (0, 3)
    vol = vc.random_volume((64, 64, 64), 0.3, 85)        # _patched's volume before its patches
    vol[16:32, 16:32, 16:32] = 2
    vol[0:16, 0:16, 0:16] = 0
    vol[8:14, 13:16, 10:15] = 1
    old = rt.Tree.volume_gpu(3, vol, PAL, view=1)
    n = _diff_both_ways(old, t, vc.in_view(vol, PAL, 1), comp, 3, "before the patches against after")
    assert n > 1000
    _diff_both_ways(old, t, vc.in_view(vol, PAL, 1), comp, 3, "the patch's box", (9, 13, 6), (21, 18, 27))
    assert tl._same_state(before[0], tl._state(t)) and tl._same_state(before[1], tl._state(twin))


# ------------------------------------------------------------------------------------- 6. the contract with the patch --
def _patch_makes_equal(a, b, label):
    xyz, ids = a.diff_voxels(b)
    assert len(ids) > 0, label
    a.patch_points(xyz, ids)
    assert a.count_diff(b) == 0 and b.count_diff(a) == 0, label
    a.compact()
    b.compact()
    (na, ma), (nb, mb) = a.export(), b.export()
    assert np.array_equal(na, nb) and np.array_equal(ma, mb), label     # byte for byte
    assert a.count_diff(b) == 0, label


def test_patching_with_the_diff_gives_the_other_tree(rt, cuda):
    va, vb = _pair_volumes()
    _patch_makes_equal(rt.Tree.volume_gpu(3, va, PAL, view=1), rt.Tree.volume_gpu(3, vb, PAL, view=1), "the crossed pair")


def test_patching_a_terrain_tree_with_the_diff(rt, cuda):
    a, b = rt.Tree.terrain_gpu(4, 200, 200, 0), rt.Tree.terrain_gpu(4, 200, 200, 0)
    _, stored = tl._np(b.list_voxels((0, 0, 0), (64, 256, 64)))
    choice = np.concatenate([[0], np.unique(stored)]).astype(np.uint16)
    rng = np.random.default_rng(606)
    top = int(b.list_voxels()[0][:, 1].max())
    p = np.stack([rng.integers(0, 256, 300), rng.integers(0, top + 3, 300), rng.integers(0, 256, 300)], 1).astype(np.int32)
    b.patch_points(p, rng.choice(choice, 300))
    assert 0 < a.count_diff(b) <= 300
    _patch_makes_equal(a, b, "terrain after 300 edits")


# --------------------------------------------------------------------------------------- 7. seven levels, content --
CUBE7 = tl.CUBE7
CUT = ((CUBE7[0] - 5, CUBE7[1] + 3, CUBE7[2] + 37), (50, 40, 30))   # the listing's box cutting the cube


@pytest.fixture(scope="module")
def scatter7(rt, cuda):
    """T: a 7-level points-built tree (full view) of 5,000 seeded points and an aligned 64^3 cube of id 4; T2: its copy
    patched with 200 seeded edits; the lists of what each stores; the positions overwritten with the id they had"""
    rng = np.random.default_rng(717)
    p = rng.integers(0, 16384, (5000, 3)).astype(np.int32)
    i = rng.integers(1, 6, 5000).astype(np.uint16)
    built = pc.concat((p, i), tl._cube(*CUBE7, 4, s=64))
    T, T2 = rt.Tree.points_gpu(7, *built, PAL, 1), rt.Tree.points_gpu(7, *built, PAL, 1)
    _, kind, mat = tl._kinds(T)
    n = int(T.node_indices([(CUBE7[0] + 9, CUBE7[1] + 9, CUBE7[2] + 9)])[0])
    assert kind[n] == K_SOLID and mat[n] == 4                            # the cube collapsed
    stored = lv.survivors(*built, 7)
    sx, si = pc.last_wins(p, i)                                          # the scatter points, each once
    puts = (rng.integers(0, 16384, (100, 3)).astype(np.int32), rng.integers(1, 6, 100).astype(np.uint16))
    erased = (sx[:40], np.zeros(40, np.uint16))
    recoloured = (sx[40:60], (si[40:60] % 5 + 1).astype(np.uint16))
    same_id = (sx[60:80], si[60:80])
    (ox, oy, oz), _ = CUT                                                # 20 distinct voxels of the cube inside the box CUT
    flat = rng.choice(24 * 39 * 27, 20, replace=False)
    inside = np.stack([CUBE7[0] + flat % 24, oy + (flat // 24) % 39, oz + flat // (24 * 39)], 1).astype(np.int32)
    in_cube = (inside, np.array([0, 2] * 10, np.uint16))                 # erased, or another id
    edits = pc.concat(puts, erased, recoloured, same_id, in_cube)
    assert len(edits[1]) == 200
    T2.patch_points(*edits)
    after = lv.survivors(*pc.concat(built, edits), 7)
    return T, T2, stored, after, same_id[0]


def test_seven_levels_after_edits(rt, cuda, scatter7):
    T, T2, stored, after, same_id = scatter7
    for a, b, la, lb, way in ((T, T2, stored, after, "before -> after"), (T2, T, after, stored, "after -> before")):
        want = dm.of_lists(la, lb, 7)
        assert 150 < len(want[1]) <= 180                                 # the same-id overwrites are no difference
        got = a.diff_voxels(b)
        _same(got, want, 7, "7 levels, " + way)
        assert a.count_diff(b) == len(want[1])
        keys = lv.key_of(tl._np(got)[0], 7)
        assert not np.isin(lv.key_of(same_id, 7), keys).any()
        origin, shape = CUT
        cut = lv.in_box(*want, origin, shape)
        assert len(cut[1]) >= 20
        _same(a.diff_voxels(b, origin, shape), cut, 7, "7 levels, a box cutting the cube, " + way)
        assert a.count_diff(b, origin, shape) == len(cut[1])


# --------------------------------------------------------------------------------------- 8. seven levels, uniform --
def _grid(origin, shape):
    nz, ny, nx = shape
    z, y, x = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    return np.stack([x.ravel() + origin[0], y.ravel() + origin[1], z.ravel() + origin[2]], 1).astype(np.int32)


def test_seven_levels_solid_root(rt, cuda, scatter7):
    T, _, stored, _, _ = scatter7
    w = rt.World(7)
    w.put_block(0, 0, 0, *vc.TABLE[1], level=1)
    R = w.build().upload(0)
    nodes = R.export()[0]
    assert len(nodes) == 1 and ((int(nodes[0, 1]) >> 32) & 3) == K_SOLID
    r = int(R.get_blocks(np.array([(7, 8, 9)], np.int32))[0])
    assert r != 0
    empty = rt.World(7).build().upload(0)
    assert R.count_diff(empty) == 2 ** 42 and empty.count_diff(R) == 2 ** 42
    assert R.count_diff(R) == 0 and empty.count_diff(empty) == 0
    k = int((stored[1] == r).sum())
    assert 0 < k
    assert R.count_diff(T) == 2 ** 42 - k and T.count_diff(R) == 2 ** 42 - k
    for a, b in ((R, empty), (R, T)):                                    # no list holds 2^42 entries
        with pytest.raises(rt.SvoError, match=r"\(-5\).*2\^31"):
            a.diff_voxels(b)
        xyz, ids = tl._buffers(cuda, 16)
        n = C.c_int64(-7)
        rc = rt.lib().svo_tree_diff_gpu(a._h, b._h, None, 0, 0, 0, C.c_void_p(xyz.data_ptr()), C.c_void_p(ids.data_ptr()), 16, C.byref(n), None)
        assert rc == ERANGE and n.value == (2 ** 42 if b is empty else 2 ** 42 - k)
        assert bool((xyz == -1).all()) and bool((ids == -1).all())

    origin, shape = (4093, 8190, 12287), (110, 90, 100)                  # straddles region boundaries of several levels
    grid = _grid(origin, shape)
    assert len(grid) == 990000
    _same(empty.diff_voxels(R, origin, shape), lv.by_key(grid, np.full(len(grid), r, np.uint16), 7), 7, "unranked through seven levels")
    _same(R.diff_voxels(empty, origin, shape), lv.by_key(grid, np.zeros(len(grid), np.uint16), 7), 7, "the solid root erased in a box")

    origin, shape = CUT                                                  # R against T where the box cuts T's cube
    grid = _grid(origin, shape)
    ids_t = np.zeros(len(grid), np.uint16)
    tx, ti = lv.in_box(*stored, origin, shape)
    (ox, oy, oz), (nz, ny, nx) = origin, shape
    ids_t[((tx[:, 2] - oz) * ny + (tx[:, 1] - oy)) * nx + (tx[:, 0] - ox)] = ti
    assert (ids_t == 4).sum() >= 25 * 40 * 27 and (ids_t == 0).sum() > 0
    differ = ids_t != r
    got = R.diff_voxels(T, origin, shape)
    _same(got, lv.by_key(grid[differ], ids_t[differ], 7), 7, "the solid root against the scatter, a box cutting the cube")
    gx, gi = tl._np(got)
    in_cube = ((gx >= np.array(CUBE7)) & (gx < np.array(CUBE7) + 64)).all(1)
    assert (gi[in_cube] == 4).all() and in_cube.sum() == 25 * 40 * 27 and np.isin(gi[~in_cube], [0, 1, 2, 3, 4, 5]).all()
    assert R.count_diff(T, origin, shape) == int(differ.sum())
    _same(T.diff_voxels(R, origin, shape), lv.by_key(grid[differ], np.full(int(differ.sum()), r, np.uint16), 7), 7, "the scatter against the solid root")


# ------------------------------------------------------------------------------------------------------ 9. capacity --
def test_capacity(rt, cuda, pair3):
    a, b, va, vb, _ = pair3
    origin, shape = BOXES["cutting changed cells"]
    want = dm.model(va, vb, origin, shape)
    need = len(want[1])
    assert need > 64
    xyz, ids = tl._buffers(cuda, need - 1)                       # one entry short
    n = C.c_int64(-7)
    o = (C.c_int32 * 3)(*origin)
    rc = rt.lib().svo_tree_diff_gpu(a._h, b._h, o, shape[2], shape[1], shape[0], C.c_void_p(xyz.data_ptr()), C.c_void_p(ids.data_ptr()),
                                    need - 1, C.byref(n), None)
    cuda.cuda.synchronize()
    assert rc == ERANGE and n.value == need
    assert NAME in rt.lib().svo_last_error().decode()
    assert bool((xyz == -1).all()) and bool((ids == -1).all())  # nothing written
    with pytest.raises(rt.SvoError, match=r"\(-5\)"):
        a.diff_voxels(b, origin, shape, out=(xyz, ids))
    for extra in (0, 5):
        xyz, ids = tl._buffers(cuda, need + extra)
        gx, gi = a.diff_voxels(b, origin, shape, out=(xyz, ids))
        assert gx.data_ptr() == xyz.data_ptr() and gi.data_ptr() == ids.data_ptr() and len(gx) == len(gi) == need
        _same((gx, gi), want, 3, "capacity n + %d" % extra)
        assert bool((xyz[need:] == -1).all()) and bool((ids[need:] == -1).all())
    with pytest.raises(ValueError, match="out"):
        a.diff_voxels(b, origin, shape, out=(xyz.to(cuda.int64), ids))


def test_the_second_tree_not_uploaded(rt, cuda):
    a, b = rt.World(2).build().upload(0), rt.World(2).build()
    n = C.c_int64(-7)
    f = rt.lib().svo_tree_diff_gpu
    assert f(a._h, b._h, None, 0, 0, 0, None, None, 0, C.byref(n), None) == ESTATE
    msg = rt.lib().svo_last_error().decode()
    assert NAME in msg and "tree b not uploaded" in msg and n.value == -7
    assert f(b._h, a._h, None, 0, 0, 0, None, None, 0, C.byref(n), None) == ESTATE
    assert "tree a not uploaded" in rt.lib().svo_last_error().decode() and n.value == -7
    with pytest.raises(rt.SvoError, match=r"svo_tree_diff_gpu failed \(-4\): tree b not uploaded"):
        a.count_diff(b)


# ------------------------------------------------------------------------------------- 10, 11. a side stream; nothing changes --
def test_callers_buffers_on_another_stream_and_nothing_changed(rt, cuda, pair3):
    a, b, va, vb, before = pair3                                # (before: ahead of every call of the tests above)
    want = dm.model(va, vb)
    s = cuda.cuda.Stream()
    with cuda.cuda.stream(s):
        xyz, ids = tl._buffers(cuda, len(want[1]) + 3)
        gx, gi = a.diff_voxels(b, out=(xyz, ids), stream=s)
        got = tl._np((gx, gi))                                   # (the call has waited for its stream: no synchronize)
    tl._same_list(got, want, 3, "side stream")
    assert a.count_diff(b) == len(want[1])
    assert tl._same_state(before[0], tl._state(a)) and tl._same_state(before[1], tl._state(b))   # nodes, mats, garbage, ceilings
