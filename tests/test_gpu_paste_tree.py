"""svo_tree_patch_tree_gpu on the GPU: a box of one resident tree pasted into another leaves the destination holding the
composite — inside the box what the source stores at the matching position (REPLACE), or that only where the source stores
something (KEEP_EMPTY), resolved against the destination's view; outside the box what it held — and the source untouched.
The reference for content is numpy (paste_tree_cases.apply_paste).

Every 64^3 content case runs test_gpu_points_patch's checks (1) .. (5): read_volume equals the model; after compact(),
export() equals a fresh volume_gpu of the model byte for byte; the ceilings equal the fresh tree's; hit records are
bit-equal to the fresh tree's; garbage() equals the arrays' lengths minus what a walk of export() reaches; no K_BRICK
record has mask 0.  At 7 levels, where the pasted region could exist neither as a dense box nor as a list, the result is
checked against a third tree given the same shapes at the shifted position, through the diff, the listing's closed-form
counts, lookups and a listed slab, and the growth of the arrays against a bound derived from the cells the two boxes cut
and the records the source holds."""
import ctypes as C

import numpy as np
import pytest

import list_voxels_cases as lvc
import paste_tree_cases as ptc
import points_patch_cases as ppc
import shapes_patch_cases as spc
import volume_cases as vc
from test_gpu_points_patch import NEAR7, _cube, _old64, _scatter7, _sparse64, _stored, check_patched
from test_gpu_volume_build import _same
from test_gpu_volume_patch import PAL, _kinds, _tree

pytestmark = pytest.mark.gpu

K_INTERIOR, K_BRICK, K_SOLID = 0, 1, 2


@pytest.fixture(scope="module")
def cuda(rt):
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    assert hasattr(rt.lib(), "svo_tree_patch_tree_gpu")
    return torch


@pytest.fixture(scope="module")
def worlds():
    """the planted 64^3 worlds of test_gpu_points_patch: every record shape occurs in old64; sparse64 is mostly empty"""
    old, sparse = _old64(), _sparse64()
    assert (old[0:16, 0:16, 0:16] == 4).all() and (old == 5).any()   # a K_SOLID 16^3, and liquid
    assert not sparse[48:64, 48:64, 48:64].any()                       # an empty 16^3
    old.setflags(write=False)
    sparse.setflags(write=False)
    return {"old64": old, "sparse64": sparse}


def _export(t):
    n, m = t.export()
    return n.tobytes(), m.tobytes()


def paste_and_check(rt, cuda, dst_vol, src, src_dense, box, keep, label, view=0, levels=3, **kw):
    """a volume-built tree of `dst_vol`, given the box of the uploaded tree `src` (whose stored content is src_dense) in one
    call, against the model; src must come out byte-identical"""
    so, dims, do = box
    t = rt.Tree.volume_gpu(levels, np.array(dst_vol, np.uint16), PAL, view=view)
    comp = ptc.apply_paste(vc.in_view(np.asarray(dst_vol), PAL, view), src_dense, so, dims, do, keep, ppc.view_keep(PAL, view))
    before = _export(src), src.garbage(), src.info().n_nodes
    assert t.patch_tree(src, so, dims, do, keep_empty=keep) is t
    assert (_export(src), src.garbage(), src.info().n_nodes) == before, "%s: src changed" % label
    check_patched(rt, cuda, t, comp, label, **kw)
    return t, comp


# ------------------------------------------------------------------------------------------- 1. 3 levels into 3 --
@pytest.mark.parametrize("keep", [False, True], ids=["replace", "keep_empty"])
@pytest.mark.parametrize("view", [0, 1])
@pytest.mark.parametrize("case", sorted(ptc.BOXES64))
def test_content(rt, cuda, worlds, case, view, keep):
    src_world, dst_world, so, dims, do = ptc.BOXES64[case]
    src_view = 1 if case == "liquid in src" else view
    src_vol = vc.in_view(worlds[src_world], PAL, src_view)
    src = _tree(rt, 3, worlds[src_world], view=src_view)
    dst_vol = worlds[dst_world]
    before = vc.in_view(dst_vol, PAL, view)
    label = "%s, view %d, %s" % (case, view, "keep_empty" if keep else "replace")
    t = rt.Tree.volume_gpu(3, np.array(dst_vol, np.uint16), PAL, view=view)
    comp = ptc.apply_paste(before, src_vol, so, dims, do, keep, ppc.view_keep(PAL, view))
    image, n0 = _export(src), t.info().n_nodes
    assert t.patch_tree(src, so, dims, do, keep_empty=keep) is t
    assert _export(src) == image and src.garbage() == (0, 0), "%s: src changed" % label
    grown = t.info().n_nodes - n0
    mask, kind, mat = _kinds(t)
    if case == "the whole extent":
        if keep:
            assert t.garbage()[0] > 0                                      # KEEP_EMPTY never restarts
            assert np.array_equal(comp, np.where(src_vol != 0, src_vol, before))
        else:
            assert t.garbage() == (0, 0) and np.array_equal(comp, src_vol)  # the arrays restarted
    elif case == "src's empty 16^3":
        if keep:   # a no-op: nothing beyond the anchor's rewritten child block
            assert np.array_equal(comp, before) and 0 < grown <= 64 * 3
        else:
            assert not comp[14:30, 9:25, 3:19].any() and before[14:30, 9:25, 3:19].any()
    elif case == "a K_SOLID 16^3 across dst's centre":
        assert (comp[26:42, 23:39, 25:41] == 4).all()
        ni = int(t.node_indices([(32, 32, 32)])[0])
        assert kind[ni] == K_SOLID and mat[ni] == 4 and int(t.node_indices([(35, 35, 35)])[0]) == ni   # whole bricks inside: one record each
    elif case == "one src 16^3 off dst's grid":
        assert np.array_equal(comp[35:51, 6:22, 21:37] != 0, (src_vol[16:32, 16:32, 16:32] != 0) | (keep & (before[35:51, 6:22, 21:37] != 0)))
    elif case == "liquid in src":
        sx, sy, sz = so
        box = src_vol[sz:sz + dims[2], sy:sy + dims[1], sx:sx + dims[0]]
        got = comp[do[2]:do[2] + dims[2], do[1]:do[1] + dims[1], do[0]:do[0] + dims[0]]
        assert (box == 5).any()
        assert (got[box == 5] == (5 if view else 0)).all()                 # decided on src's id, then stored empty in the solid view
        if keep and not view:
            assert (before[do[2]:do[2] + dims[2], do[1]:do[1] + dims[1], do[0]:do[0] + dims[0]][box == 5] != 0).any()   # liquid erased solid content
    check_patched(rt, cuda, t, comp, label)


def test_the_two_views_of_one_world_stay_its_two_views(rt, cuda, worlds):
    """pasting the full-view src into the solid-view tree and into the full-view tree of one world"""
    src = _tree(rt, 3, worlds["old64"], view=1)
    a, b = _tree(rt, 3, worlds["sparse64"], view=0), _tree(rt, 3, worlds["sparse64"], view=1)
    for t in (a, b):
        t.patch_tree(src, (10, 9, 8), (30, 29, 31), (11, 11, 11))
        t.patch_tree(src, (33, 30, 21), (25, 30, 40), (2, 7, 18), keep_empty=True)
    full = _stored(b)
    assert (full == 5).any() and np.array_equal(_stored(a), vc.in_view(full, PAL, 0))


# ------------------------------------------------------------------------------------------------ 2. prefabs --
def _prefab1(rt, view):
    """a 4^3 prefab: a tree of one level, which only the host builder makes; (tree, its content in its own ids)"""
    vol = np.zeros((4, 4, 4), np.uint16)
    vol[0:2, :, :] = 1
    vol[2, 1:3, 0:3] = 2
    vol[3, 3, 3] = 5                                    # liquid: stored by the full view only
    h, pal, dense = vc.host_twin(rt, 1, vol, (0, 0, 0), view)
    assert h.info().levels == 1 and len(pal) <= len(PAL)
    t = h.upload(0)
    stored = _stored(t)
    assert np.array_equal(stored, vc.in_view(dense, pal, view)) and (stored != 0).sum() == (39 if view else 38)
    return t, stored


def _prefab2(rt, view):
    vol = vc.random_volume((16, 16, 16), 0.5, 23)
    vol[4:8, 8:12, 0:4] = 2                             # a SOLID child of the root
    vol[8:12, 0:4, 12:16] = 0                           # an absent one
    return _tree(rt, 2, vol, view=view), vc.in_view(vol, PAL, view)


PREFABS = {
    "4^3 off the grid": (_prefab1, None, None, (21, 34, 7)),
    "4^3 on a brick": (_prefab1, None, None, (40, 24, 36)),
    "4^3 in the far corner": (_prefab1, None, None, (60, 60, 60)),
    "part of a 4^3": (_prefab1, (1, 0, 2), (3, 4, 2), (9, 9, 9)),
    "16^3 off the grid": (_prefab2, None, None, (13, 22, 37)),
    "16^3 touching the -x face": (_prefab2, None, None, (0, 31, 5)),
    "16^3 touching the +z face": (_prefab2, None, None, (7, 2, 48)),
    "part of a 16^3": (_prefab2, (3, 2, 1), (9, 10, 11), (30, 31, 29)),
}


@pytest.mark.parametrize("views", [(0, 0), (1, 1), (0, 1), (1, 0)], ids=lambda v: "src%d-dst%d" % v)
@pytest.mark.parametrize("case", sorted(PREFABS))
def test_prefabs(rt, cuda, worlds, case, views):
    make, so, dims, do = PREFABS[case]
    src, dense = make(rt, views[0])
    assert src.info().levels < 3
    for keep in (False, True):
        label = "%s, src view %d into dst view %d, keep %d" % (case, views[0], views[1], keep)
        paste_and_check(rt, cuda, worlds["old64"], src, dense, (so, dims, do), keep, label, view=views[1], casts=keep)


# ------------------------------------------------------------------------------- 3. the layouts the patches leave --
def test_src_in_the_layouts_the_patches_leave(rt, cuda, worlds):
    src = _tree(rt, 3, worlds["sparse64"])
    src.patch_points(*_cube(20, 8, 48, 3))                               # a full one-material brick that stays a brick
    assert not worlds["sparse64"][48:64, 0:16, 0:16].any()
    src.patch_points(np.array([[5, 5, 60]], np.int32), np.ones(1, np.uint16))      # a voxel into an empty 16^3, and out again:
    src.patch_points(np.array([[5, 5, 60]], np.int32), np.zeros(1, np.uint16))     # an interior record with mask 0
    src.patch_shapes([rt.ball((44, 42, 44), 30, 0), rt.box((2, 50, 2), (20, 9, 30), 4)])          # and superseded records
    mask, kind, mat = _kinds(src)
    ni = int(src.node_indices([(21, 9, 49)])[0])
    assert kind[ni] == K_BRICK and mask[ni] == np.uint64(0xFFFFFFFFFFFFFFFF) and mat[ni] == 3
    assert ((kind == K_INTERIOR) & (mask == 0)).any() and src.garbage()[0] > 0
    dense = _stored(src)
    boxes = [((16, 4, 44), (24, 40, 16), (3, 18, 9)), ((30, 30, 30), (20, 20, 20), (30, 30, 30)), (None, None, (0, 0, 0)),
             ((0, 48, 0), (24, 12, 33), (37, 1, 30)), ((0, 0, 44), (16, 16, 20), (31, 17, 5))]
    image = _export(src)
    first = {}
    for keep in (False, True):
        for i, box in enumerate(boxes):
            t, comp = paste_and_check(rt, cuda, worlds["old64"], src, dense, box, keep, "patched src, box %d, keep %d" % (i, keep), casts=False)
            first[keep, i] = (t, comp)
    assert _export(src) == image
    src.compact()
    assert src.garbage() == (0, 0) and np.array_equal(_stored(src), dense)
    for keep in (False, True):
        for i, box in enumerate(boxes):
            t = _tree(rt, 3, worlds["old64"])
            t.patch_tree(src, *box, keep_empty=keep)
            assert np.array_equal(_stored(t), first[keep, i][1])
            t.compact()
            _same(t, first[keep, i][0], "compacted src, box %d, keep %d" % (i, keep))    # (check_patched compacted the first)


# ----------------------------------------------------------------------------------------------- 4. src == dst --
SELF = {
    "a clone to a disjoint place": ((0, 0, 0), (20, 30, 25), (40, 33, 37), False),
    "a clone that keeps what the target held": ((0, 0, 0), (20, 30, 25), (40, 33, 37), True),
    "a shift by (1, 0, 0) of an overlapping box": ((5, 6, 7), (40, 41, 42), (6, 6, 7), False),
    "a shift by (-3, 2, -1), keep_empty": ((8, 6, 7), (40, 41, 42), (5, 8, 6), True),
    "the whole extent onto itself": (None, None, (0, 0, 0), False),
    "the whole extent onto itself, keep_empty": (None, None, (0, 0, 0), True),
}


@pytest.mark.parametrize("view", [0, 1])
@pytest.mark.parametrize("case", sorted(SELF))
def test_self_paste(rt, cuda, worlds, case, view):
    so, dims, do, keep = SELF[case]
    old = vc.in_view(worlds["old64"], PAL, view)
    t = _tree(rt, 3, worlds["old64"], view=view)
    t.patch_points(np.array([[1, 1, 1]], np.int32), np.array([2], np.uint16))    # (a tree that already carries garbage)
    old[1, 1, 1] = 2
    assert t.garbage()[0] > 0
    comp = ptc.apply_paste(old, old, so, dims, do, keep, ppc.view_keep(PAL, view))   # the model reads the old content only
    assert t.patch_tree(t, so, dims, do, keep_empty=keep) is t
    if so is None:
        assert np.array_equal(comp, old)
        assert (t.garbage() == (0, 0)) == (not keep)                                # REPLACE over the extent restarts, KEEP_EMPTY never
    else:
        assert not np.array_equal(comp, old)
    check_patched(rt, cuda, t, comp, "%s, view %d" % (case, view), casts=so is not None and view == 0)


# --------------------------------------------------------------------------------------- 5. sequences and capacity --
def test_twenty_pastes_past_the_upload_slack(rt, cuda):
    E = 256
    comp = vc.random_volume((E, E, E), 0.02, 41, ids=(1, 2, 3, 4))
    src_vol = vc.random_volume((E, E, E), 0.03, 43, ids=(1, 2, 3, 4))
    src_vol[64:128, 64:128, 64:128] = 3                                  # a K_SOLID 64^3 and an empty one
    src_vol[128:192, 64:128, 64:128] = 0
    t, src = _tree(rt, 4, comp), _tree(rt, 4, src_vol)
    image = _export(src)
    keep_ids = ppc.view_keep(PAL, 0)
    n0, bytes_seen, garbage = t.info().n_nodes, [t.info().device_bytes], [t.garbage()]
    rng = np.random.default_rng(131)
    for i in range(20):
        dims = tuple(int(v) for v in rng.integers(70, 130, 3))
        so = tuple(int(rng.integers(0, E - d + 1)) for d in dims)
        do = tuple(int(rng.integers(0, E - d + 1)) for d in dims)
        keep = i % 3 == 1
        t.patch_tree(src, so, dims, do, keep_empty=keep)
        comp = ptc.apply_paste(comp, src_vol, so, dims, do, keep, keep_ids)
        bytes_seen.append(t.info().device_bytes)
        garbage.append(t.garbage())
        assert cuda.equal(t.read_volume((0, 0, 0), (E, E, E)), cuda.from_numpy(comp.view(np.int16)).cuda()), "(1) step %d: %r" % (i, (so, dims, do, keep))
    assert _export(src) == image
    assert t.info().n_nodes > n0 + n0 // 8 + 65536                   # past the slack of the upload: the arrays were reallocated
    assert any(b > a for a, b in zip(bytes_seen, bytes_seen[1:]))
    assert all(b[0] > a[0] and b[1] >= a[1] for a, b in zip(garbage, garbage[1:])) and garbage[-1][1] > 0
    check_patched(rt, cuda, t, comp, "20 pastes", casts=False)       # (compacts)
    t.patch_tree(t, (10, 20, 30), (100, 90, 80), (77, 66, 55))      # and once more after the compaction, from itself
    check_patched(rt, cuda, t, ptc.apply_paste(comp, comp, (10, 20, 30), (100, 90, 80), (77, 66, 55), False, keep_ids),
                  "pasted again after the compaction", casts=False)


# ---------------------------------------------------------------------------------------------------- 6. 7 levels --
E7 = 4 ** 7
BOX7 = ("box", (5001, 3, 7001), (1300, 1300, 1300), 2)
BALL7 = ("ball", (5650, 700, 7500), 90000, 0)
DST7 = (7000, 7500, 7800)                                             # BOX7's place in dst: an offset odd on every axis, over the cluster


def _mixed_per_level(t):
    """per depth, the records of an exported tree reachable from the root that are not K_SOLID: the cells of that level the
    tree does not hold as uniform (points_patch_cases.reachable's walk)"""
    nodes = t.export()[0]
    mask, ref = nodes[:, 0], (nodes[:, 1] & np.uint64(0xFFFFFFFF)).astype(np.int64)
    kind = ((nodes[:, 1] >> np.uint64(32)) & np.uint64(3)).astype(np.int64)
    cur, out = np.zeros(1, np.int64), []
    for _ in range(t.info().levels):
        out.append(int((kind[cur] != K_SOLID).sum()))
        inner = cur[kind[cur] == K_INTERIOR]
        cnt = ppc._popcount(mask[inner])
        total = int(cnt.sum())
        cur = np.repeat(ref[inner], cnt) + (np.arange(total) - np.repeat(np.cumsum(cnt) - cnt, cnt))
    return out


def _ball_cut_cells(centre, r2, cs):
    """the number of aligned cells of cs^3 voxels the ball cuts (svo_shape_cell.h's exact rule: the nearest voxel within r2,
    the farthest corner beyond it), counted over the cells of its bounding box"""
    r = int(np.sqrt(float(r2))) + 1
    near2, far2 = [], []
    for c in centre:
        o = np.arange((c - r) // cs, (c + r) // cs + 1, dtype=np.int64) * cs
        lo, hi = o - c, o - c + cs - 1
        near2.append(np.where(lo > 0, lo, np.where(hi < 0, -hi, 0)) ** 2)
        far2.append(np.maximum(np.abs(lo), np.abs(hi)) ** 2)
    near = near2[2][:, None, None] + near2[1][None, :, None] + near2[0][None, None, :]
    far = far2[2][:, None, None] + far2[1][None, :, None] + far2[0][None, None, :]
    return int(((near <= r2) & (far > r2)).sum())


def test_seven_levels(rt, cuda):
    """a 1300^3 region of one material with a ball carved out of it (2.2 * 10^9 voxels: more than a list can hold, 4.4 GB as
    a dense box), pasted from one 16384^3 world into another at an offset odd on every axis.

    The growth bound.  Every record the paste appends lies in the child block of a cut cell above the brick level (or of
    the anchor), at most 64 per block.  A destination cell of 4^k voxels is cut only where the destination box's surface
    cuts it — box_cut_cells(dst box, 4^k) cells — or where it meets a source cell of its level that src holds as a record
    of that level; a source cell meets at most 2 x 2 x 2 destination cells.  src was made from an empty tree by a box and
    a ball, so it holds such records only where the surface of one of them cuts a cell: at most
    box_cut_cells(src box, 4^k) + ball_cut_cells(4^k) of them, which is checked on its export before the bound is used."""
    scatter = _scatter7()
    keep = ppc.view_keep(PAL, 0)
    points = ppc.resolve_edits(*scatter, keep)
    points = (points[0][points[1] != 0], points[1][points[1] != 0])
    src = rt.Tree.points_gpu(7, np.zeros((0, 3), np.int32), np.zeros(0, np.uint16), PAL)
    assert src.count_voxels() == 0
    src.patch_shapes(spc.to_abi(rt, [BOX7, BALL7]))
    dst = rt.Tree.points_gpu(7, *scatter, PAL)
    want = rt.Tree.points_gpu(7, *scatter, PAL)
    shift = np.array(DST7) - np.array(BOX7[1])
    assert (shift % 2 == 1).all()
    box_d = ("box", DST7, BOX7[2], BOX7[3])
    ball_d = ("ball", tuple(int(v) for v in np.array(BALL7[1]) + shift), BALL7[2], 0)
    want.patch_shapes(spc.to_abi(rt, [box_d, ball_d]))
    lo, hi = np.array(DST7), np.array(DST7) + np.array(BOX7[2])
    assert (hi <= E7).all()
    volume = 1300 ** 3
    n_ball = spc.ball_count(ball_d[1], ball_d[2], lo, hi)
    assert n_ball == spc.ball_count(ball_d[1], ball_d[2], (0, 0, 0), (E7, E7, E7))         # the ball lies inside the box
    in_box = spc.contains(box_d, points[0])
    assert in_box.sum() > 1000 and (~in_box).sum() > 2000

    # src's records per level against the cells its two shapes cut
    mixed = _mixed_per_level(src)                                        # by depth: the cells of 4^(7 - depth) voxels
    cut_src = {k: spc.box_cut_cells(BOX7[1], BOX7[2], 4 ** k) + _ball_cut_cells(BALL7[1], BALL7[2], 4 ** k) for k in range(1, 7)}
    for k in range(1, 7):
        assert mixed[7 - k] <= cut_src[k], (k, mixed[7 - k], cut_src[k])
    bound = 64 * (1 + sum(spc.box_cut_cells(DST7, BOX7[2], 4 ** k) + 8 * cut_src[k] for k in range(2, 7)))
    print("7 levels: src records by depth %r, cut cells by k %r, bound %d" % (mixed, cut_src, bound))

    image, i0 = _export(src), dst.info()
    assert dst.patch_tree(src, BOX7[1], BOX7[2], DST7) is dst
    i1 = dst.info()
    print("7 levels: %d records appended, patch_times %r" % (i1.n_nodes - i0.n_nodes, dst.patch_times()))
    assert _export(src) == image
    assert 0 < i1.n_nodes - i0.n_nodes <= bound
    assert dst.garbage() == ppc.expected_garbage(dst)

    def checks(label):
        assert dst.count_diff(want) == 0 and want.count_diff(dst) == 0, label
        assert dst.count_voxels(DST7, BOX7[2][::-1]) == volume - n_ball, label
        assert dst.count_voxels() == volume - n_ball + int((~in_box).sum()), label
        rng = np.random.default_rng(175)
        c = np.array(ball_d[1])
        diam = np.tile(c, (640, 1))
        diam[:, 0] += np.arange(-320, 320)
        faces = lo + rng.integers(0, 1300, (400, 3))
        faces[:100, 0], faces[100:200, 0], faces[200:300, 2], faces[300:, 1] = lo[0] - 1, hi[0] - 1, hi[2], lo[1]
        where = np.concatenate([rng.integers(0, E7, (2048, 3)), lo + rng.integers(-100, 1400, (2048, 3)), diam, faces,
                                points[0][:2000], points[0][in_box][:500]]).astype(np.int32)
        where = where[((where >= 0) & (where < E7)).all(1)]
        got = dst.get_blocks_gpu(np.ascontiguousarray(where)).cpu().numpy().view(np.uint16)
        expect = spc.lookup(points, [box_d, ball_d], keep, where)
        assert np.array_equal(got, expect), "%s: %d lookups differ" % (label, int((got != expect).sum()))
        assert (expect == 0).any() and (expect == BOX7[3]).any() and ((expect != 0) & (expect != BOX7[3])).any()

    checks("pasted")
    # a slab of the box one voxel thick, through the ball's centre, in key order
    cz = ball_d[1][2]
    xyz, ids = (a.cpu().numpy() for a in dst.list_voxels((lo[0], lo[1], cz), (1, 1300, 1300)))
    yy, xx = np.meshgrid(np.arange(1300) + lo[1], np.arange(1300) + lo[0], indexing="ij")
    slab = np.stack([xx.ravel(), yy.ravel(), np.full(xx.size, cz)], 1)
    sid = spc.lookup(points, [box_d, ball_d], keep, slab)
    wx, wi = lvc.by_key(slab[sid != 0], sid[sid != 0], 7)
    assert np.array_equal(xyz, wx) and np.array_equal(ids.view(np.uint16), wi)
    mask, kind, _ = _kinds(dst)
    assert not ((kind == K_BRICK) & (mask == 0)).any()
    dst.compact()
    assert dst.garbage() == (0, 0)
    checks("compacted")
    # KEEP_EMPTY of the same region into the untouched world, the hole over the cluster: the carved ball is transparent
    dst = rt.Tree.points_gpu(7, *scatter, PAL)
    far = tuple(int(v) for v in np.array(NEAR7) - (np.array(BALL7[1]) - np.array(BOX7[1])))
    ball_f = ("ball", NEAR7, BALL7[2], 0)
    assert (np.array(far) >= 0).all() and (np.array(far) + 1300 <= E7).all()
    shown = int((spc.contains(ball_f, points[0])).sum())               # what dst holds inside the hole shows through
    assert shown > 1000
    dst.patch_tree(src, BOX7[1], BOX7[2], far, keep_empty=True)
    assert dst.count_voxels(far, BOX7[2][::-1]) == volume - n_ball + shown
    at = np.concatenate([points[0][spc.contains(ball_f, points[0])][:500], np.array([far])]).astype(np.int32)
    got = dst.get_blocks_gpu(np.ascontiguousarray(at)).cpu().numpy().view(np.uint16)
    assert np.array_equal(got[:-1], points[1][spc.contains(ball_f, points[0])][:500]) and got[-1] == BOX7[3]
    assert dst.garbage() == ppc.expected_garbage(dst)
    assert _export(src) == image


# ------------------------------------------------------------------------------------------------- 7. refusals --
def test_refusals_on_the_device_path_change_nothing(rt, cuda, worlds):
    t, src = _tree(rt, 3, worlds["old64"]), _tree(rt, 3, worlds["sparse64"])
    t.patch_tree(src, (0, 0, 0), (20, 20, 20), (5, 5, 5))                  # (a tree that already carries garbage)
    g, ceil, quads, times = t.garbage(), t.device_ceilings(), t.device_ceiling_quads(), t.patch_times()
    image, simage = _export(t), _export(src)
    assert g[0] > 0 and times[0] > 0.0

    def unchanged():
        assert _export(t) == image and _export(src) == simage and t.garbage() == g and t.patch_times() == times
        c2 = t.device_ceilings()
        assert c2[0] == ceil[0] and np.array_equal(c2[1], ceil[1]) and np.array_equal(c2[2], ceil[2])
        assert np.array_equal(t.device_ceiling_quads(), quads)

    for so, dims, do, code in (((0, 0, 0), (20, 20, 20), (50, 5, 5), -1), ((60, 0, 0), (5, 5, 5), (0, 0, 0), -1),
                               ((0, 0, 0), (4, 0, 4), (0, 0, 0), -1)):
        with pytest.raises(rt.SvoError, match=r"svo_tree_patch_tree_gpu failed \(%d\)" % code):
            t.patch_tree(src, so, dims, do)
        unchanged()
    assert rt.lib().svo_tree_patch_tree_gpu(t._h, src._h, None, 0, 0, 0, (C.c_int32 * 3)(0, 0, 0), 4) == -1
    unchanged()
    # a palette larger than dst's
    big = rt.Tree.volume_gpu(3, np.array(worlds["sparse64"], np.uint16), PAL + [(1, 12345, 0.0)])
    with pytest.raises(rt.SvoError, match=r"svo_tree_patch_tree_gpu failed \(-5\).*palette"):
        t.patch_tree(big, None, None, (0, 0, 0))
    unchanged()
    # unsynced trees on the same device, as src and as dst
    w = rt.World(3)
    w.put_block(5, 6, 7, 0, int(vc.colour(11)))
    u = w.build().upload(0)
    w.put_block(9, 9, 9, 0, int(vc.colour(11)))
    u.update(w, [(9, 9, 9)])
    uimage = _export(u)
    with pytest.raises(rt.SvoError, match=r"svo_tree_patch_tree_gpu failed \(-4\).*src.*not yet synced"):
        t.patch_tree(u, None, None, (0, 0, 0))
    unchanged()
    with pytest.raises(rt.SvoError, match=r"svo_tree_patch_tree_gpu failed \(-4\).*dst.*not yet synced"):
        u.patch_tree(u, (0, 0, 0), (8, 8, 8), (20, 20, 20))
    assert _export(u) == uimage
    u.sync()
    t.patch_tree(u, (4, 4, 4), (8, 8, 8), (30, 30, 30))                    # synced, it goes through
    assert t.get_block(31, 32, 33)[1] == 1 and t.get_block(35, 35, 35)[1] == 1 and t.patch_times() != times
