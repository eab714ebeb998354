"""svo_tree_patch_shapes_gpu on the GPU: a resident tree patched from a list of boxes and balls holds the composite — every
voxel the id of the last shape that contains it, a voxel inside no shape as before — and reads back, carries ceilings,
casts and, once compacted, is laid out exactly like a tree built afresh from that composite.  The reference for content
is numpy (shapes_patch_cases.apply_shapes: expected[mask(s)] = stored_id(s), in list order).

Every 64^3 content case runs test_gpu_points_patch's checks (1) .. (5) in both views: read_volume equals the model; after
compact(), export() equals a fresh volume_gpu of the model byte for byte; the ceilings equal the fresh tree's; hit records
are bit-equal to the fresh tree's; garbage() equals the arrays' lengths minus what a walk of export() reaches; no K_BRICK
record has mask 0.  At 7 levels, where neither a dense box nor an edit list of the patch could exist, the result is
checked through the closed-form counts of the listing and the diff, lookups and a listed slab."""
import numpy as np
import pytest

import list_voxels_cases as lvc
import points_cases as pc
import points_patch_cases as ppc
import shapes_patch_cases as spc
import volume_cases as vc
from test_gpu_points_patch import _old64, _scatter7, _sparse64, _stored, check_patched
from test_gpu_volume_build import _same
from test_gpu_volume_patch import PAL, _kinds, _tree

pytestmark = pytest.mark.gpu

K_INTERIOR, K_BRICK, K_SOLID = 0, 1, 2


@pytest.fixture(scope="module")
def cuda(rt):
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    assert hasattr(rt.lib(), "svo_tree_patch_shapes_gpu")
    return torch


@pytest.fixture(scope="module")
def old64():
    """the planted 64^3 world of test_gpu_volume_patch / test_gpu_points_patch: every record shape occurs"""
    vol = _old64()
    assert (vol[0:16, 0:16, 0:16] == 4).all()          # a K_SOLID 16^3
    vol.setflags(write=False)
    return vol


@pytest.fixture(scope="module")
def sparse64():
    vol = _sparse64()
    assert not vol[48:64, 48:64, 48:64].any()           # an empty 16^3
    vol.setflags(write=False)
    return vol


def patch_and_check(rt, cuda, old, shapes, label, view=0, levels=3, **kw):
    """a volume-built tree of `old`, patched with the shapes in one call, against the model"""
    t = rt.Tree.volume_gpu(levels, np.array(old, np.uint16), PAL, view=view)
    comp = spc.apply_shapes(vc.in_view(np.asarray(old), PAL, view), shapes, ppc.view_keep(PAL, view))
    assert t.patch_shapes(spc.to_abi(rt, shapes)) is t
    check_patched(rt, cuda, t, comp, label, **kw)
    return t, comp


A, ERASER, B = ("box", (8, 8, 8), (32, 32, 32), 1), ("ball", (24, 24, 24), 100, 0), ("box", (20, 20, 20), (32, 10, 32), 3)

# name: (world, shapes)
CASES = {
    "box of one voxel": ("old64", [("box", (37, 5, 20), (1, 1, 1), 2)]),
    "box off the grid": ("old64", [("box", (9, 10, 3), (13, 9, 22), 3)]),
    "box that is one brick": ("old64", [("box", (40, 24, 36), (4, 4, 4), 2)]),
    "box that is one 16^3": ("old64", [("box", (16, 32, 48), (16, 16, 16), 1)]),
    "box that is the extent": ("old64", [("box", (0, 0, 0), (64, 64, 64), 3)]),
    "box that is the extent, id 0": ("old64", [("box", (0, 0, 0), (64, 64, 64), 0)]),
    "ball of r2 0": ("old64", [("ball", (21, 22, 23), 0, 2)]),
    "ball of r2 2 on a brick corner": ("old64", [("ball", (16, 16, 16), 2, 1)]),
    "ball of r2 3 in an empty brick": ("sparse64", [("ball", (50, 9, 21), 3, 4)]),
    "ball across the centre": ("old64", [("ball", (32, 31, 33), 20 * 20 + 5, 2)]),
    "ball sticking out of a face": ("old64", [("ball", (-5, 30, 40), 30 * 30, 3)]),
    "ball centred past a corner": ("old64", [("ball", (70, 70, -6), 24 * 24, 1)]),
    "ball covering the extent": ("old64", [("ball", (32, 32, 32), 3 * 32 * 32, 2)]),
    "carve inside a K_SOLID region": ("old64", [("ball", (8, 8, 8), 25, 0)]),
    "fill in an empty region": ("sparse64", [("ball", (56, 56, 56), 36, 3)]),
    "carve in an empty region": ("sparse64", [("ball", (56, 56, 56), 36, 0)]),
    "liquid box": ("old64", [("box", (9, 10, 3), (13, 9, 22), 5)]),
    "liquid ball": ("old64", [("ball", (8, 8, 8), 25, 5)]),
    "A, eraser, B": ("old64", [A, ERASER, B]),
    "B, eraser, A": ("old64", [B, ERASER, A]),
    "a late box cuts what an early one covers": ("old64", [("box", (0, 0, 0), (64, 64, 64), 2), ("box", (30, 30, 30), (3, 3, 3), 4)]),
}


@pytest.mark.parametrize("view", [0, 1])
@pytest.mark.parametrize("case", sorted(CASES))
def test_content(rt, cuda, old64, sparse64, case, view):
    world, shapes = CASES[case]
    old = {"old64": old64, "sparse64": sparse64}[world]
    before = vc.in_view(np.asarray(old), PAL, view)
    compact = case not in ("box that is the extent", "box that is the extent, id 0", "ball covering the extent", "box that is one 16^3")
    t, comp = patch_and_check(rt, cuda, old, shapes, "%s, view %d" % (case, view), view=view, compact=compact)
    mask, kind, mat = _kinds(t)
    if case.startswith("liquid"):
        where, m = spc.mask(shapes[0], 64)
        assert (comp[where][m] == (5 if view else 0)).all() and (before[where][m] != 0).any()   # in the solid view it erases
    elif case in ("box that is the extent", "ball covering the extent"):
        assert len(mask) == 1 and kind[0] == K_SOLID and mat[0] == shapes[0][3] and t.garbage() == (0, 0)   # the arrays restarted
        assert len(t.export()[1]) == 0
    elif case == "box that is the extent, id 0":
        assert len(mask) == 1 and kind[0] == K_INTERIOR and mask[0] == 0 and t.garbage() == (0, 0)
    elif case == "box that is one 16^3":
        ni = int(t.node_indices([(20, 40, 50)])[0])
        assert kind[ni] == K_SOLID and mat[ni] == 1 and int(t.node_indices([(31, 47, 63)])[0]) == ni   # one record for the 16^3
    elif case == "box that is one brick":
        ni = int(t.node_indices([(41, 25, 37)])[0])
        assert kind[ni] == K_SOLID and mat[ni] == 2                                                  # and one for the brick
    elif case == "carve in an empty region":
        assert np.array_equal(comp, before)
    elif case == "B, eraser, A":
        other = spc.apply_shapes(before, [A, ERASER, B], ppc.view_keep(PAL, view))
        assert not np.array_equal(comp, other) and (comp[20:30, 20:30, 20:30] == 1).all() and (other[24, 24, 24] == 3)
    if not compact:   # the same checks once compacted, on a tree whose layout was looked at first
        check_patched(rt, cuda, t, comp, "%s, view %d, compacted" % (case, view), casts=False)


def test_one_call_equals_three(rt, cuda, old64):
    one, three = _tree(rt, 3, old64), _tree(rt, 3, old64)
    one.patch_shapes(spc.to_abi(rt, [A, ERASER, B]))
    for s in (A, ERASER, B):
        three.patch_shapes(spc.to_abi(rt, [s]))
    assert np.array_equal(_stored(one), _stored(three))
    assert three.garbage() == ppc.expected_garbage(three) and three.garbage()[0] > one.garbage()[0]
    one.compact()
    three.compact()
    _same(one, three, "one call against three")


def test_shape_objects_and_lists(rt, cuda, old64):
    t = _tree(rt, 3, old64)
    nodes = t.export()[0].tobytes()
    assert t.patch_shapes([]) is t and t.patch_shapes(iter([rt.ball((-500, 5, 5), 4, 1)])) is t    # nothing, and nothing left
    assert rt.lib().svo_tree_patch_shapes_gpu(t._h, None, 0) == 0
    assert t.export()[0].tobytes() == nodes and t.garbage() == (0, 0)
    with pytest.raises(ValueError):
        t.patch_shapes([("box", (0, 0, 0), (1, 1, 1), 1)])
    t.patch_shapes([rt.box((1, 2, 3), (1, 1, 1), 2)])
    assert t.get_block(1, 2, 3)[1] == 2 and all(ms >= 0.0 for ms in t.patch_times()) and t.patch_times()[0] > 0.0


# ------------------------------------------------------------------------------------------------------ refusals --
REFUSED = {
    "an id equal to the palette size": (lambda rt: rt.box((5, 5, 5), (9, 9, 9), len(PAL)), -5),
    "a box that leaves the extent": (lambda rt: rt.box((60, 5, 5), (5, 9, 9), 1), -1),
    "a box without volume": (lambda rt: rt.box((5, 5, 5), (9, 0, 9), 1), -1),
    "a negative r2": (lambda rt: rt.ball((5, 5, 5), -1, 1), -1),
    "a centre past 2^20": (lambda rt: rt.ball((5, -(1 << 20) - 1, 5), 9, 1), -5),
    "an r2 past 2^42": (lambda rt: rt.ball((5, 5, 5), (1 << 42) + 1, 1), -5),
}


@pytest.mark.parametrize("case", sorted(REFUSED))
def test_a_refused_call_changes_nothing(rt, cuda, old64, case):
    t = _tree(rt, 3, old64)
    t.patch_shapes(spc.to_abi(rt, [ERASER]))                       # (a tree that already carries garbage)
    nodes, mats = t.export()
    g, ceil, quads, times = t.garbage(), t.device_ceilings(), t.device_ceiling_quads(), t.patch_times()
    assert g[0] > 0
    make, code = REFUSED[case]
    with pytest.raises(rt.SvoError, match=r"svo_tree_patch_shapes_gpu failed \(%d\).*shape 2" % code):
        t.patch_shapes(spc.to_abi(rt, [A, B]) + [make(rt)])       # the good shapes before it are not applied either
    n2, m2 = t.export()
    assert nodes.tobytes() == n2.tobytes() and mats.tobytes() == m2.tobytes() and t.garbage() == g and t.patch_times() == times
    c2 = t.device_ceilings()
    assert c2[0] == ceil[0] and np.array_equal(c2[1], ceil[1]) and np.array_equal(c2[2], ceil[2])
    assert np.array_equal(t.device_ceiling_quads(), quads)
    assert t.info().n_nodes == len(nodes)
    t.patch_shapes(spc.to_abi(rt, [A, B]))                         # the same list without the bad shape goes through
    assert t.get_block(10, 10, 10)[1] == 1


def test_too_many_shapes_change_nothing(rt, cuda, old64):
    t = _tree(rt, 3, old64)
    nodes = t.export()[0].tobytes()
    with pytest.raises(rt.SvoError, match=r"svo_tree_patch_shapes_gpu failed \(-5\).*1024"):
        t.patch_shapes(spc.to_abi(rt, [A] * 1025))
    assert t.export()[0].tobytes() == nodes and t.garbage() == (0, 0)


# --------------------------------------------------------------------------------------- sequences and capacity --
def test_twenty_patches_past_the_upload_slack(rt, cuda):
    E = 256
    comp = vc.random_volume((E, E, E), 0.02, 41, ids=(1, 2, 3, 4))
    t = _tree(rt, 4, comp)
    keep = ppc.view_keep(PAL, 0)
    n0, bytes_seen, garbage = t.info().n_nodes, [t.info().device_bytes], [t.garbage()]
    rng = np.random.default_rng(131)
    for i in range(20):
        c = tuple(int(v) for v in rng.integers(20, E - 20, 3))
        if i % 3 == 2:
            d = tuple(int(v) for v in rng.integers(30, 90, 3))
            s = ("box", tuple(min(a, E - b) for a, b in zip(c, d)), d, int(rng.integers(0, 5)))
        else:
            s = ("ball", c, int(rng.integers(30, 70)) ** 2 + int(rng.integers(0, 50)), int(rng.integers(0, 5)))
        t.patch_shapes(spc.to_abi(rt, [s]))
        comp = spc.apply_shapes(comp, [s], keep)
        bytes_seen.append(t.info().device_bytes)
        garbage.append(t.garbage())
        assert cuda.equal(t.read_volume((0, 0, 0), (E, E, E)), cuda.from_numpy(comp.view(np.int16)).cuda()), "(1) step %d: %r" % (i, s)
    assert t.info().n_nodes > n0 + n0 // 8 + 65536                   # past the slack of the upload: the arrays were reallocated
    assert any(b > a for a, b in zip(bytes_seen, bytes_seen[1:]))
    assert all(b[0] > a[0] and b[1] >= a[1] for a, b in zip(garbage, garbage[1:])) and garbage[-1][1] > 0
    check_patched(rt, cuda, t, comp, "20 patches", casts=False)      # (compacts)
    t.patch_shapes(spc.to_abi(rt, [("ball", (100, 90, 80), 50 * 50, 0)]))
    check_patched(rt, cuda, t, spc.apply_shapes(comp, [("ball", (100, 90, 80), 50 * 50, 0)], keep), "patched again after the compaction",
                  casts=False)


# -------------------------------------------------------------------------------------------- other trees --
def test_two_levels(rt, cuda):
    """16^3: the anchor is the root and every cut child is a brick"""
    old = vc.random_volume((16, 16, 16), 0.3, 1)
    old[4:8, 8:12, 0:4] = 2                                       # a SOLID child of the root
    old[8:12, 0:4, 12:16] = 0                                     # an absent one
    shapes = [("ball", (7, 8, 5), 30, 3), ("box", (9, 1, 11), (5, 4, 5), 0), ("box", (0, 12, 0), (4, 4, 4), 5)]
    for view in (0, 1):
        patch_and_check(rt, cuda, old, shapes, "2 levels, view %d" % view, view=view, levels=2, casts=False)
    full = np.full((16, 16, 16), 3, np.uint16)
    t, comp = patch_and_check(rt, cuda, full, [("ball", (0, 0, 0), 9, 0)], "2 levels, solid root", levels=2, casts=False)
    assert comp[0, 0, 0] == 0 and comp[0, 0, 3] == 0 and comp[3, 3, 3] == 3
    t, comp = patch_and_check(rt, cuda, comp, [("ball", (8, 8, 8), 3 * 64, 2)], "2 levels, covered", levels=2, casts=False, compact=False)
    assert len(t.export()[0]) == 1 and t.garbage() == (0, 0)


def test_world_built_tree(rt, cuda):
    w = rt.World(3)
    rng = np.random.default_rng(71)
    pts = rng.integers(0, 64, (3000, 3))
    w.put_blocks(pts, np.zeros(len(pts), np.uint32), np.full(len(pts), int(vc.colour(3)), np.uint64))
    t = w.build().upload(0)
    assert t.info().n_materials == 2 and t.garbage() == (0, 0)
    before = _stored(t)
    shapes = [("ball", (30, 28, 33), 15 * 15, 1), ("box", (22, 20, 30), (20, 9, 3), 0)]
    t.patch_shapes(spc.to_abi(rt, shapes))
    comp = spc.apply_shapes(before, shapes, ppc.view_keep(t.palette(), 0))
    check_patched(rt, cuda, t, comp, "world-built", compact=False)
    w.put_block(1, 1, 1, 0, int(vc.colour(3)))
    with pytest.raises(rt.SvoError, match=r"svo_tree_update failed \(-4\)"):
        t.update(w, [(1, 1, 1)])
    check_patched(rt, cuda, t, comp, "world-built, after the refused update", casts=False)


def test_a_tree_with_unsynced_host_edits_is_refused(rt, cuda):
    w = rt.World(3)
    w.put_block(5, 6, 7, 0, int(vc.colour(3)))
    t = w.build().upload(0)
    w.put_block(9, 9, 9, 0, int(vc.colour(3)))
    t.update(w, [(9, 9, 9)])
    with pytest.raises(rt.SvoError, match=r"svo_tree_patch_shapes_gpu failed \(-4\).*not yet synced"):
        t.patch_shapes([rt.box((1, 1, 1), (1, 1, 1), 1)])
    t.sync()
    t.patch_shapes([rt.box((1, 1, 1), (1, 1, 1), 1)])
    assert t.get_block(1, 1, 1)[1] == 1 and t.get_block(9, 9, 9)[1] == 1


def test_a_tree_already_patched_by_the_other_patches(rt, cuda, old64):
    t = _tree(rt, 3, old64)
    t.patch_volume(np.zeros((20, 20, 20), np.uint16), (5, 6, 7))     # interiors with mask 0 may appear, and garbage
    rng = np.random.default_rng(95)
    t.patch_points(rng.integers(0, 64, (400, 3)).astype(np.int32), rng.integers(0, 5, 400).astype(np.uint16))
    g0 = t.garbage()
    before = _stored(t)
    shapes = [("ball", (14, 15, 16), 12 * 12, 2), ("box", (3, 3, 3), (40, 6, 7), 0)]
    t.patch_shapes(spc.to_abi(rt, shapes))
    assert t.garbage()[0] > g0[0]
    check_patched(rt, cuda, t, spc.apply_shapes(before, shapes, ppc.view_keep(PAL, 0)), "after patch_volume and patch_points")


# ---------------------------------------------------------------------------------------------------- 7 levels --
E7 = 4 ** 7
BOX7 = ("box", (5001, 3, 7001), (1300, 1300, 1300), 2)
BALL7 = ("ball", (5650, 700, 7500), 90000, 0)


def _faces_and_diameters():
    """positions one voxel either side of each face of BOX7, and along three diameters of BALL7 (past both ends)"""
    rng = np.random.default_rng(176)
    lo, n = np.array(BOX7[1]), np.array(BOX7[2])
    out = []
    for axis in range(3):
        for face in (lo[axis] - 1, lo[axis], lo[axis] + n[axis] - 1, lo[axis] + n[axis]):
            p = lo + rng.integers(0, 1300, (40, 3))
            p[:, axis] = face
            out.append(p[(p >= 0).all(1)])
        c = np.array(BALL7[1])
        d = np.tile(c, (640, 1))
        d[:, axis] += np.arange(-320, 320)
        out.append(d)
    return np.concatenate(out)


def _scatter_shapes7():
    """test_gpu_points_patch's 7-level scatter, and a few thousand more voxels in and around BOX7 and BALL7"""
    rng = np.random.default_rng(177)
    around = np.array(BOX7[1]) + rng.integers(-60, 1360, (2500, 3))
    around = around[(around >= 0).all(1)]
    near = np.array(BALL7[1]) + rng.integers(-320, 320, (1500, 3))
    xyz = np.concatenate([around, near]).astype(np.int32)
    return pc.concat(_scatter7(), (xyz, rng.integers(1, 6, len(xyz)).astype(np.uint16)))


def test_seven_levels(rt, cuda):
    """a 1300^3 fill (2,197,000,000 voxels: more than an edit list can hold, 4.4 GB as a dense box) and a ball carved out
    of it, in a 16384^3 world of scattered voxels"""
    scatter = _scatter_shapes7()
    keep = ppc.view_keep(PAL, 0)
    points = ppc.resolve_edits(*scatter, keep)                       # the distinct positions with what the tree stores
    points = (points[0][points[1] != 0], points[1][points[1] != 0])
    t = rt.Tree.points_gpu(7, *scatter, PAL)
    untouched = rt.Tree.points_gpu(7, *scatter, PAL)
    n_stored = t.count_voxels()
    assert n_stored == len(points[1])
    volume = 1300 ** 3
    assert volume > 2 ** 31 - 1
    lo, hi = np.array(BOX7[1]), np.array(BOX7[1]) + np.array(BOX7[2])
    c, r = np.array(BALL7[1]), 300
    assert (c - r > lo).all() and (c + r < hi).all()                 # the ball lies inside the box
    n_ball = spc.ball_count(BALL7[1], BALL7[2], lo, hi)
    assert n_ball == spc.ball_count(BALL7[1], BALL7[2], (0, 0, 0), (E7, E7, E7)) and 4.18 * r ** 3 < n_ball < 4.20 * r ** 3
    in_box, in_ball = spc.contains(BOX7, points[0]), spc.contains(BALL7, points[0])
    assert in_ball.sum() > 100 and (in_box & ~in_ball).sum() > 1000 and (~in_box).sum() > 3000
    assert (in_box & ~in_ball & (points[1] == BOX7[3])).sum() > 100

    # the box: growth follows the cells it cuts, not its volume
    i0 = t.info()
    t.patch_shapes(spc.to_abi(rt, [BOX7]))
    i1 = t.info()
    cut = {k: spc.box_cut_cells(BOX7[1], BOX7[2], 4 ** k) for k in range(1, 7)}
    assert 0 < i1.n_nodes - i0.n_nodes <= 64 * (1 + sum(cut[k] for k in range(2, 7)))   # every interior item appends one child block
    assert i1.n_mat_bytes - i0.n_mat_bytes <= 2 * 64 * cut[1]                           # and only cut bricks get material runs
    assert t.garbage() == ppc.expected_garbage(t)
    assert t.count_voxels(BOX7[1], BOX7[2][::-1]) == volume
    assert t.count_voxels() == volume + int((~in_box).sum())

    # the ball
    t.patch_shapes(spc.to_abi(rt, [BALL7]))
    shapes = [BOX7, BALL7]

    def counts(label):
        assert t.count_voxels(BOX7[1], BOX7[2][::-1]) == volume - n_ball, label
        assert t.count_voxels() == volume - n_ball + int((~in_box).sum()), label
        # against the untouched tree: the box's voxels outside the ball that did not hold its id, and what the ball emptied
        differ = volume - n_ball - int((in_box & ~in_ball & (points[1] == BOX7[3])).sum()) + int(in_ball.sum())
        assert t.count_diff(untouched) == differ and untouched.count_diff(t) == differ, label

    def lookups(label):
        rng = np.random.default_rng(175)
        where = np.concatenate([rng.integers(0, E7, (2048, 3)), lo + rng.integers(-100, 1400, (2048, 3)), _faces_and_diameters(),
                                points[0][:2000], points[0][in_box][:500]]).astype(np.int32)
        where = where[((where >= 0) & (where < E7)).all(1)]          # (the lookup wraps: only positions of the extent are asked)
        got = t.get_blocks_gpu(np.ascontiguousarray(where)).cpu().numpy().view(np.uint16)
        want = spc.lookup(points, shapes, keep, where)
        assert np.array_equal(got, want), "%s: %d lookups differ" % (label, int((got != want).sum()))
        assert (want == 0).any() and (want == BOX7[3]).any() and ((want != 0) & (want != BOX7[3])).any()

    counts("patched")
    lookups("patched")
    # a slab of the box one voxel thick, through the ball's centre, in key order
    origin, shape = (lo[0], lo[1], c[2]), (1, 1300, 1300)
    xyz, ids = (a.cpu().numpy() for a in t.list_voxels(origin, shape))
    yy, xx = np.meshgrid(np.arange(1300) + lo[1], np.arange(1300) + lo[0], indexing="ij")
    slab = np.stack([xx.ravel(), yy.ravel(), np.full(xx.size, c[2])], 1)
    sid = spc.lookup(points, shapes, keep, slab)
    wx, wi = lvc.by_key(slab[sid != 0], sid[sid != 0], 7)
    assert np.array_equal(xyz, wx) and np.array_equal(ids.view(np.uint16), wi)
    assert len(wi) == 1300 * 1300 - spc.ball_count(BALL7[1], BALL7[2], (lo[0], lo[1], c[2]), (hi[0], hi[1], c[2] + 1))
    assert t.garbage() == ppc.expected_garbage(t) and t.garbage()[0] > 0
    mask, kind, _ = _kinds(t)
    assert not ((kind == K_BRICK) & (mask == 0)).any()
    t.compact()
    assert t.garbage() == (0, 0)
    counts("compacted")
    lookups("compacted")
