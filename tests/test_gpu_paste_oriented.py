"""svo_tree_patch_tree_oriented_gpu on the GPU: a box of one resident tree pasted into another turned or mirrored by any of
the 48 signed axis permutations, its ids through a map.  The reference for content is numpy
(paste_oriented_cases.apply_oriented, itself checked against numpy's transpose and flip in test_paste_oriented_model.py).

Every 64^3 content case runs test_gpu_points_patch's checks (1) .. (5), all exact: read_volume equals the model; after
compact(), export() equals a fresh volume_gpu of the model byte for byte; the ceilings equal the fresh tree's; hit records
are bit-equal to the fresh tree's; garbage() equals the arrays' lengths minus what a walk of export() reaches; no K_BRICK
record has mask 0; and src comes out byte-identical.  At 7 levels the result is checked through closed forms only: against
a third tree given the transformed shapes, through the diff, the listing's counts and lookups, and the growth of the
arrays against the plain paste's bound."""
import ctypes as C

import numpy as np
import pytest

import paste_oriented_cases as poc
import points_patch_cases as ppc
import shapes_patch_cases as spc
import volume_cases as vc
from test_gpu_paste_tree import _ball_cut_cells, _mixed_per_level
from test_gpu_points_patch import NEAR7, _cube, _old64, _scatter7, _sparse64, _stored, check_patched
from test_gpu_volume_build import _same
from test_gpu_volume_patch import PAL, _kinds, _tree

pytestmark = pytest.mark.gpu

K_INTERIOR, K_BRICK, K_SOLID = 0, 1, 2
TURNS = {"quarter turn about y": poc.QUARTER_Y, "mirror in x": poc.MIRROR_X, "inversion": poc.INVERSION}
OFF_GRID = ((10, 9, 8), (13, 22, 27), (11, 11, 11))      # three different dimensions, off every grid at both ends


@pytest.fixture(scope="module")
def cuda(rt):
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    assert hasattr(rt.lib(), "svo_tree_patch_tree_oriented_gpu")
    return torch


@pytest.fixture(scope="module")
def worlds():
    """the planted 64^3 worlds of test_gpu_paste_tree: every record shape occurs in old64; sparse64 is mostly empty"""
    old, sparse = _old64(), _sparse64()
    assert (old[0:16, 0:16, 0:16] == 4).all() and (old == 5).any()   # a K_SOLID 16^3, and liquid
    assert not sparse[48:64, 48:64, 48:64].any()                       # an empty 16^3
    old.setflags(write=False)
    sparse.setflags(write=False)
    return {"old64": old, "sparse64": sparse}


def _export(t):
    n, m = t.export()
    return n.tobytes(), m.tobytes()


def _name(orient):
    return "axis%d%d%d-flip%d%d%d" % (orient[0] + orient[1])


def paste_and_check(rt, cuda, dst_vol, src, src_dense, box, orient, keep, label, view=0, id_map=None, pal=PAL, **kw):
    """a volume-built tree of `dst_vol`, given the box of the uploaded tree `src` (whose stored content is src_dense) in one
    oriented call, against the model; src must come out byte-identical"""
    so, dims, do = box
    axis, flip = orient
    t = rt.Tree.volume_gpu(3, np.array(dst_vol, np.uint16), pal, view=view)
    comp = poc.apply_oriented(vc.in_view(np.asarray(dst_vol), pal, view), src_dense, so, dims, do, axis, flip, id_map, keep,
                              ppc.view_keep(pal, view))
    before = _export(src), src.garbage(), src.info().n_nodes
    assert t.patch_tree_oriented(src, so, dims, do, axis=axis, flip=flip, id_map=id_map, keep_empty=keep) is t
    assert (_export(src), src.garbage(), src.info().n_nodes) == before, "%s: src changed" % label
    check_patched(rt, cuda, t, comp, label, **kw)
    return t, comp


# --------------------------------------------------------------------------------------- 1. all 48 orientations --
@pytest.fixture(scope="module")
def old_src(rt, cuda, worlds):
    return _tree(rt, 3, worlds["old64"]), vc.in_view(worlds["old64"], PAL, 0)


@pytest.mark.parametrize("orient", poc.ORIENTATIONS, ids=_name)
def test_all_orientations(rt, cuda, worlds, old_src, orient):
    src, dense = old_src
    box = dense[8:35, 9:31, 10:23]
    mine = poc.orient_box(box, *orient)                                 # no other orientation gives this content
    assert len(set(OFF_GRID[1])) == 3 and mine.shape == poc.dst_dims(OFF_GRID[1], orient[0])[::-1]
    assert all(o == orient or poc.orient_box(box, *o).shape != mine.shape or not np.array_equal(poc.orient_box(box, *o), mine) for o in poc.ORIENTATIONS)
    for keep in (False, True):
        paste_and_check(rt, cuda, worlds["old64"], src, dense, OFF_GRID, orient, keep, "%s, keep %d" % (_name(orient), keep),
                        casts=poc.ORIENTATIONS.index(orient) % 8 == keep)


@pytest.mark.parametrize("views", [(0, 0), (1, 1), (0, 1), (1, 0)], ids=lambda v: "src%d-dst%d" % v)
@pytest.mark.parametrize("orient", [poc.IDENTITY, poc.QUARTER_Y, ((1, 2, 0), (1, 0, 1))], ids=_name)
def test_both_views(rt, cuda, worlds, orient, views):
    src = _tree(rt, 3, worlds["old64"], view=views[0])
    dense = vc.in_view(worlds["old64"], PAL, views[0])
    for keep in (False, True):
        paste_and_check(rt, cuda, worlds["sparse64"], src, dense, ((6, 6, 6), (30, 20, 25), (19, 22, 7)), orient, keep,
                        "%s, views %r, keep %d" % (_name(orient), views, keep), view=views[1], casts=keep)


# ----------------------------------------------------------------------------------------------- 2. directed boxes --
DIRECTED = {
    "a one-voxel box": ("old64", "old64", (21, 22, 20), (1, 1, 1), (38, 5, 19)),
    "one src brick off dst's grid": ("old64", "old64", (40, 24, 36), (4, 4, 4), (17, 30, 41)),
    "a K_SOLID 16^3 across dst's centre": ("old64", "old64", (0, 0, 0), (16, 16, 16), (25, 23, 26)),
    "src's empty 16^3": ("sparse64", "old64", (48, 48, 48), (16, 16, 16), (3, 9, 14)),
    "liquid in src": ("old64", "old64", (6, 6, 6), (30, 20, 25), (19, 22, 7)),
    "the whole extent": ("old64", "sparse64", None, None, (0, 0, 0)),
}


@pytest.mark.parametrize("turn", sorted(TURNS))
@pytest.mark.parametrize("case", sorted(DIRECTED))
def test_directed_boxes(rt, cuda, worlds, case, turn):
    src_world, dst_world, so, dims, do = DIRECTED[case]
    orient = TURNS[turn]
    liquid = case == "liquid in src"
    src_view = 1 if liquid else 0
    src_vol = vc.in_view(worlds[src_world], PAL, src_view)
    src = _tree(rt, 3, worlds[src_world], view=src_view)
    for view in ((0, 1) if liquid else (0,)):
        for keep in (False, True):
            label = "%s, %s, view %d, keep %d" % (case, turn, view, keep)
            before = vc.in_view(worlds[dst_world], PAL, view)
            t = rt.Tree.volume_gpu(3, np.array(worlds[dst_world], np.uint16), PAL, view=view)
            comp = poc.apply_oriented(before, src_vol, so, dims, do, orient[0], orient[1], None, keep, ppc.view_keep(PAL, view))
            image, n0 = _export(src), t.info().n_nodes
            assert t.patch_tree_oriented(src, so, dims, do, axis=orient[0], flip=orient[1], keep_empty=keep) is t
            assert _export(src) == image and src.garbage() == (0, 0), "%s: src changed" % label
            grown = t.info().n_nodes - n0
            mask, kind, mat = _kinds(t)
            if case == "the whole extent":
                if keep:
                    assert t.garbage()[0] > 0                                           # KEEP_EMPTY never restarts
                else:
                    assert t.garbage() == (0, 0)                                        # the arrays restarted
                    assert np.array_equal(comp, poc.orient_box(src_vol, *orient)) and not np.array_equal(comp, src_vol)
            elif case == "src's empty 16^3":
                if keep:   # a no-op: nothing beyond the anchor's rewritten child block
                    assert np.array_equal(comp, before) and 0 < grown <= 64 * 3
                else:
                    assert not comp[14:30, 9:25, 3:19].any() and before[14:30, 9:25, 3:19].any()
            elif case == "a K_SOLID 16^3 across dst's centre":
                assert (comp[26:42, 23:39, 25:41] == 4).all()
                ni = int(t.node_indices([(32, 32, 32)])[0])     # whole bricks inside stay one-record cells
                assert kind[ni] == K_SOLID and mat[ni] == 4 and int(t.node_indices([(35, 35, 35)])[0]) == ni
            elif case == "one src brick off dst's grid":
                got = comp[41:45, 30:34, 17:21]
                assert set(np.unique(got)) == {1, 4} and np.array_equal(got, poc.orient_box(src_vol[36:40, 24:28, 40:44], *orient))
                assert (got[:, 0, :] == (1 if orient[1][1] else 4)).all()               # the rows of 4 are the lower ones unless y is flipped
            elif case == "a one-voxel box":
                assert comp[19, 5, 38] == (src_vol[20, 22, 21] if src_vol[20, 22, 21] or not keep else before[19, 5, 38])
            elif liquid:
                dn = poc.dst_dims(dims, orient[0])
                box = poc.orient_box(src_vol[so[2]:so[2] + dims[2], so[1]:so[1] + dims[1], so[0]:so[0] + dims[0]], *orient)
                got = comp[do[2]:do[2] + dn[2], do[1]:do[1] + dn[1], do[0]:do[0] + dn[0]]
                assert (box == 5).any() and (got[box == 5] == (5 if view else 0)).all()   # decided on src's id, then stored empty
            check_patched(rt, cuda, t, comp, label, casts=not keep)


def test_faces_of_the_extent(rt, cuda, worlds, old_src):
    """a 40 x 10 x 10 box whose destination touches +x, +y and -z, and fits only with x and y exchanged"""
    src, dense = old_src
    box = ((5, 5, 5), (40, 10, 10), (54, 24, 0))
    t = _tree(rt, 3, worlds["sparse64"])
    image = _export(t)
    for orient in (poc.IDENTITY, ((0, 2, 1), (0, 0, 0)), ((0, 2, 1), (1, 1, 0))):       # dn[0] = 40: past +x
        with pytest.raises(rt.SvoError, match=r"svo_tree_patch_tree_oriented_gpu failed \(-1\).*destination box"):
            t.patch_tree_oriented(src, *box, axis=orient[0], flip=orient[1])
        assert _export(t) == image
    for orient in (((1, 0, 2), (0, 0, 0)), ((1, 0, 2), (1, 1, 1)), ((1, 2, 0), (0, 1, 0))):
        dn = poc.dst_dims(box[1], orient[0])
        assert box[2][0] + dn[0] == 64 and box[2][1] + dn[1] <= 64
        for keep in (False, True):
            paste_and_check(rt, cuda, worlds["sparse64"], src, dense, box, orient, keep, "faces, %s, keep %d" % (_name(orient), keep), casts=keep)
    corner = ((0, 0, 0), (3, 5, 7), (64 - 7, 64 - 3, 64 - 5))                            # into the far corner: dn = (7, 3, 5)
    paste_and_check(rt, cuda, worlds["sparse64"], src, dense, corner, ((2, 0, 1), (1, 0, 1)), False, "the far corner")


# ------------------------------------------------------------------------------------ 3. the identity and the maps --
BOXES = [((8, 12, 16), (24, 20, 28), (8, 12, 16)), OFF_GRID, ((0, 0, 0), (16, 16, 16), (25, 23, 26)), (None, None, (0, 0, 0)),
         ((33, 30, 21), (25, 30, 40), (2, 7, 18))]


def test_the_identity_is_the_plain_paste(rt, cuda, worlds, old_src):
    """without a map and with the identity map: the same arrays byte for byte as patch_tree on a copy of the same dst"""
    src, _ = old_src
    for so, dims, do in BOXES:
        for keep in (False, True):
            a, b, c = (_tree(rt, 3, worlds["sparse64"]) for _ in range(3))
            a.patch_points(*_cube(20, 8, 48, 3))
            b.patch_points(*_cube(20, 8, 48, 3))
            c.patch_points(*_cube(20, 8, 48, 3))
            a.patch_tree(src, so, dims, do, keep_empty=keep)
            b.patch_tree_oriented(src, so, dims, do, keep_empty=keep)
            c.patch_tree_oriented(src, so, dims, do, id_map=range(len(PAL)), keep_empty=keep)
            for t in (b, c):
                assert _export(t) == _export(a) and t.garbage() == a.garbage() and t.info().n_nodes == a.info().n_nodes, (so, dims, do, keep)
                ca, ct = a.device_ceilings(), t.device_ceilings()
                assert ca[0] == ct[0] and np.array_equal(ca[1], ct[1]) and np.array_equal(ca[2], ct[2])


MAPS = {
    "swap 1 and 2": [0, 2, 1, 3, 4, 5],
    "merge 1, 2 and 3 into 3": [0, 3, 3, 3, 4, 5],
    "drop 4": [0, 1, 2, 3, 0, 5],
    "drop everything but 4": [0, 0, 0, 0, 4, 0],
    "4 becomes the liquid": [0, 1, 2, 3, 5, 5],
}


@pytest.mark.parametrize("orient", [poc.IDENTITY, poc.QUARTER_Y, ((1, 2, 0), (1, 1, 0))], ids=_name)
@pytest.mark.parametrize("name", sorted(MAPS))
def test_maps(rt, cuda, worlds, old_src, name, orient):
    src, dense = old_src
    id_map = MAPS[name]
    box = ((0, 0, 0), (40, 30, 35), (19, 22, 7))          # holds the K_SOLID 16^3 of id 4
    for keep in (False, True):
        t, comp = paste_and_check(rt, cuda, worlds["sparse64"], src, dense, box, orient, keep, "%s, %s, keep %d" % (name, _name(orient), keep),
                                  id_map=id_map, casts=keep)
        dn = poc.dst_dims(box[1], orient[0])
        got = comp[7:7 + dn[2], 22:22 + dn[1], 19:19 + dn[0]]
        raw = poc.orient_box(dense[0:35, 0:30, 0:40], *orient)
        before = vc.in_view(worlds["sparse64"], PAL, 0)[7:7 + dn[2], 22:22 + dn[1], 19:19 + dn[0]]
        if name == "4 becomes the liquid":                # a solid id mapped to the liquid id into the solid-view tree: stored empty,
            assert not (got[raw == 4] != 0).any()         # and under KEEP_EMPTY it still erases: the mode saw id 5
        elif name == "drop 4":                            # transparent under KEEP_EMPTY, erasing under REPLACE
            assert np.array_equal(got[raw == 4], before[raw == 4] if keep else np.zeros((raw == 4).sum(), np.uint16))
        elif name == "swap 1 and 2":
            assert (got[raw == 1] == 2).all() and (got[raw == 2] == 1).all() and (raw == 1).any() and (raw == 2).any()


def test_a_merging_map_makes_a_two_material_region_uniform(rt, cuda, worlds):
    vol = np.zeros((64, 64, 64), np.uint16)
    vol[16:32, 16:24, 32:48] = 1                            # a 16^3 cell of src, its lower half 1 and its upper half 2
    vol[16:32, 24:32, 32:48] = 2
    vol[40:44, 8:12, 4:8] = vc.random_volume((4, 4, 4), 0.5, 3, ids=(1, 2))
    src = _tree(rt, 3, vol)
    for orient in (poc.IDENTITY, poc.QUARTER_Y, poc.INVERSION):
        for do in ((48, 0, 16), (21, 6, 35)):              # onto an aligned cell, and off every grid
            t, comp = paste_and_check(rt, cuda, worlds["old64"], src, vol, ((32, 16, 16), (16, 16, 16), do), orient, False,
                                      "merge, %s, to %r" % (_name(orient), do), id_map=[0, 3, 3, 3, 4, 5])
            assert (comp[do[2]:do[2] + 16, do[1]:do[1] + 16, do[0]:do[0] + 16] == 3).all()
            if do == (48, 0, 16):                           # (check_patched compacted t): one K_SOLID record
                mask, kind, mat = _kinds(t)
                ni = int(t.node_indices([(48, 0, 16)])[0])
                assert kind[ni] == K_SOLID and mat[ni] == 3 and int(t.node_indices([(63, 15, 31)])[0]) == ni


def test_a_prefab_with_a_larger_palette_goes_through_a_map(rt, cuda, worlds):
    """a 2-level prefab built as its own tree with 9 palette entries into the 6-entry world: the plain call refuses it"""
    pal9 = PAL + [(1, int(vc.colour(30 + i)), 0.0) for i in range(3)]
    vol = vc.random_volume((16, 16, 16), 0.6, 29, ids=(1, 3, 6, 7, 8))
    vol[4:8, 8:12, 0:4] = 8                                 # a SOLID child of the root
    vol[8:12, 0:4, 12:16] = 0                               # an absent one
    src = rt.Tree.volume_gpu(2, vol, pal9)
    assert src.info().n_materials == 9 and src.info().levels == 2
    t = _tree(rt, 3, worlds["old64"])
    image = _export(t)
    with pytest.raises(rt.SvoError, match=r"svo_tree_patch_tree_gpu failed \(-5\).*palette"):
        t.patch_tree(src, None, None, (13, 22, 37))
    with pytest.raises(rt.SvoError, match=r"svo_tree_patch_tree_oriented_gpu failed \(-5\).*palette"):
        t.patch_tree_oriented(src, None, None, (13, 22, 37))
    with pytest.raises(rt.SvoError, match=r"svo_tree_patch_tree_oriented_gpu failed \(-5\).*id_map\[7\]"):
        t.patch_tree_oriented(src, None, None, (13, 22, 37), id_map=[0, 1, 2, 3, 4, 5, 1, 6, 0])
    assert _export(t) == image
    id_map = [0, 1, 2, 3, 4, 5, 2, 4, 0]
    for orient in (poc.IDENTITY, poc.QUARTER_Y, ((0, 2, 1), (0, 1, 1))):
        for keep in (False, True):
            _, comp = paste_and_check(rt, cuda, worlds["old64"], src, vol, (None, None, (13, 22, 37)), orient, keep,
                                      "prefab, %s, keep %d" % (_name(orient), keep), id_map=id_map, casts=not keep)
            assert comp.max() <= 5


# --------------------------------------------------------------------------------------------------- 4. round trip --
@pytest.mark.parametrize("axis", sorted({o[0] for o in poc.ORIENTATIONS}), ids=lambda a: "axis%d%d%d" % a)
def test_round_trip(rt, cuda, worlds, axis):
    """orientation O into a scratch tree, then its inverse back into a copy of the original at the original place"""
    orig = _tree(rt, 3, worlds["old64"])
    image = _export(orig)
    so, dims, _ = OFF_GRID
    for flip in [o[1] for o in poc.ORIENTATIONS if o[0] == axis]:
        dn = poc.dst_dims(dims, axis)
        mid = _tree(rt, 3, worlds["sparse64"])
        mid.patch_tree_oriented(orig, so, dims, (31, 7, 19), axis=axis, flip=flip)
        inv = poc.inverse(axis, flip)
        assert poc.dst_dims(dn, inv[0]) == dims
        back = _tree(rt, 3, worlds["old64"])
        back.patch_points(*_cube(12, 12, 12, 0))                      # (damage inside the box, which the round trip repairs)
        back.patch_tree_oriented(mid, (31, 7, 19), dn, so, axis=inv[0], flip=inv[1])
        assert back.garbage()[0] > 0
        back.compact()
        assert _export(back) == image, (axis, flip)


# ---------------------------------------------------------------------------------------------------- 5. src == dst --
SELF = {
    "a quarter turn in place": ((20, 22, 18), (20, 20, 20), (20, 22, 18), poc.QUARTER_Y, False),
    "a quarter turn in place, keep_empty": ((20, 22, 18), (20, 20, 20), (20, 22, 18), poc.QUARTER_Y, True),
    "a quarter turn onto an overlapping box": ((20, 22, 18), (20, 20, 20), (27, 17, 25), poc.QUARTER_Y, False),
    "an inversion onto an overlapping box, keep_empty": ((20, 22, 18), (20, 20, 20), (13, 30, 11), poc.INVERSION, True),
    "the whole extent mirrored onto itself": (None, None, (0, 0, 0), poc.MIRROR_X, False),
}


@pytest.mark.parametrize("case", sorted(SELF))
def test_self_paste(rt, cuda, worlds, case):
    so, dims, do, orient, keep = SELF[case]
    old = vc.in_view(worlds["old64"], PAL, 0)
    t = _tree(rt, 3, worlds["old64"])
    t.patch_points(np.array([[1, 1, 1]], np.int32), np.array([2], np.uint16))    # (a tree that already carries garbage)
    old[1, 1, 1] = 2
    assert t.garbage()[0] > 0
    comp = poc.apply_oriented(old, old, so, dims, do, orient[0], orient[1], None, keep, ppc.view_keep(PAL, 0))   # the content on entry only
    assert t.patch_tree_oriented(t, so, dims, do, axis=orient[0], flip=orient[1], keep_empty=keep) is t
    assert not np.array_equal(comp, old)
    if so is None:
        assert t.garbage() == (0, 0) and np.array_equal(comp, old[:, :, ::-1])
    check_patched(rt, cuda, t, comp, case)


# ------------------------------------------------------------------------------- 6. the layouts the patches leave --
def test_src_in_the_layouts_the_patches_leave(rt, cuda, worlds):
    src = _tree(rt, 3, worlds["sparse64"])
    src.patch_points(*_cube(20, 8, 48, 3))                               # a full one-material brick that stays a brick
    src.patch_points(np.array([[5, 5, 60]], np.int32), np.ones(1, np.uint16))      # a voxel into an empty 16^3, and out again:
    src.patch_points(np.array([[5, 5, 60]], np.int32), np.zeros(1, np.uint16))     # an interior record with mask 0
    src.patch_shapes([rt.ball((44, 42, 44), 30, 0), rt.box((2, 50, 2), (20, 9, 30), 4)])          # and superseded records
    mask, kind, mat = _kinds(src)
    assert ((kind == K_INTERIOR) & (mask == 0)).any() and src.garbage()[0] > 0
    dense = _stored(src)
    cases = [(((16, 4, 44), (24, 40, 16), (3, 18, 9)), poc.QUARTER_Y), (((30, 30, 30), (20, 20, 20), (30, 30, 30)), poc.INVERSION),
             ((None, None, (0, 0, 0)), ((1, 2, 0), (0, 1, 0))), (((0, 48, 0), (24, 12, 33), (27, 1, 30)), ((0, 2, 1), (1, 0, 0)))]
    image = _export(src)
    first = {}
    for keep in (False, True):
        for i, (box, orient) in enumerate(cases):
            first[keep, i] = paste_and_check(rt, cuda, worlds["old64"], src, dense, box, orient, keep, "patched src, case %d, keep %d" % (i, keep),
                                             id_map=[0, 2, 1, 3, 4, 5], casts=False)
    assert _export(src) == image
    src.compact()
    assert src.garbage() == (0, 0) and np.array_equal(_stored(src), dense)
    for keep in (False, True):
        for i, (box, orient) in enumerate(cases):
            t = _tree(rt, 3, worlds["old64"])
            t.patch_tree_oriented(src, *box, axis=orient[0], flip=orient[1], id_map=[0, 2, 1, 3, 4, 5], keep_empty=keep)
            assert np.array_equal(_stored(t), first[keep, i][1])
            t.compact()
            _same(t, first[keep, i][0], "compacted src, case %d, keep %d" % (i, keep))    # (check_patched compacted the first)


# --------------------------------------------------------------------------------------- 7. sequences and capacity --
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
    rng = np.random.default_rng(137)
    for i in range(20):
        axis, flip = poc.ORIENTATIONS[int(rng.integers(0, 48))]
        dims = tuple(int(v) for v in rng.integers(70, 130, 3))
        dn = poc.dst_dims(dims, axis)
        so = tuple(int(rng.integers(0, E - d + 1)) for d in dims)
        do = tuple(int(rng.integers(0, E - d + 1)) for d in dn)
        keep, id_map = i % 3 == 1, ([0, 2, 3, 1, 0, 5] if i % 4 == 2 else None)
        t.patch_tree_oriented(src, so, dims, do, axis=axis, flip=flip, id_map=id_map, keep_empty=keep)
        comp = poc.apply_oriented(comp, src_vol, so, dims, do, axis, flip, id_map, keep, keep_ids)
        bytes_seen.append(t.info().device_bytes)
        garbage.append(t.garbage())
        assert cuda.equal(t.read_volume((0, 0, 0), (E, E, E)), cuda.from_numpy(comp.view(np.int16)).cuda()), "(1) step %d: %r" % (i, (so, dims, do, axis, flip, keep))
    assert _export(src) == image
    assert t.info().n_nodes > n0 + n0 // 8 + 65536                   # past the slack of the upload: the arrays were reallocated
    assert any(b > a for a, b in zip(bytes_seen, bytes_seen[1:]))
    assert all(b[0] > a[0] and b[1] >= a[1] for a, b in zip(garbage, garbage[1:])) and garbage[-1][1] > 0
    check_patched(rt, cuda, t, comp, "20 oriented pastes", casts=False)       # (compacts)


# ---------------------------------------------------------------------------------------------------- 8. 7 levels --
E7 = 4 ** 7
BOX7 = ("box", (5001, 3, 7001), (1300, 900, 1100), 2)
BALLS7 = [("ball", (5401, 423, 7501), 40000, 1), ("ball", (5901, 453, 7601), 40000, 3)]   # off the box's centre, apart, inside it
DST7 = (7401, 7501, 7603)                                             # odd on every axis, over the cluster
SWAP7 = [0, 3, 2, 1, 4, 5]


def test_seven_levels(rt, cuda):
    """a 1300 x 900 x 1100 region with two balls of other ids in it (1.3 * 10^9 voxels), pasted from one 16384^3 world into
    another under a quarter turn about y with the balls' ids exchanged, through closed forms only.

    The growth bound is the plain paste's (test_gpu_paste_tree.test_seven_levels), with the destination box in place of the
    shifted one: every appended record lies in the child block of a cut cell above the brick level (or of the anchor), at
    most 64 per block; a destination cell of 4^k voxels is cut only where the destination box's surface cuts it or where
    it meets a source cell of its level that src holds as a record of that level, and under an orientation a source cell
    still meets at most 2 x 2 x 2 destination cells; src holds such records only where the surface of one of its three
    shapes cuts a cell, which is checked on its export before the bound is used."""
    axis, flip = poc.QUARTER_Y
    scatter = _scatter7()
    keep = ppc.view_keep(PAL, 0)
    points = ppc.resolve_edits(*scatter, keep)
    points = (points[0][points[1] != 0], points[1][points[1] != 0])
    src = rt.Tree.points_gpu(7, np.zeros((0, 3), np.int32), np.zeros(0, np.uint16), PAL)
    src.patch_shapes(spc.to_abi(rt, [BOX7] + BALLS7))
    dst = rt.Tree.points_gpu(7, *scatter, PAL)
    want = rt.Tree.points_gpu(7, *scatter, PAL)
    dn = poc.dst_dims(BOX7[2], axis)
    assert dn == (1100, 900, 1300)
    box_d = ("box", DST7, dn, BOX7[3])
    balls_d = [("ball", poc.orient_point(b[1], BOX7[1], BOX7[2], DST7, axis, flip), b[2], SWAP7[b[3]]) for b in BALLS7]
    assert [b[3] for b in balls_d] == [3, 1]
    want.patch_shapes(spc.to_abi(rt, [box_d] + balls_d))
    lo, hi = np.array(DST7), np.array(DST7) + np.array(dn)
    assert (hi <= E7).all() and (lo % 2 == 1).all() and ((lo <= np.array(NEAR7)) & (np.array(NEAR7) < hi)).all()
    volume = dn[0] * dn[1] * dn[2]
    for b, bd in zip(BALLS7, balls_d):                                 # each ball lies inside its box, before and after
        n_ball = spc.ball_count(b[1], b[2], (0, 0, 0), (E7, E7, E7))
        assert n_ball == spc.ball_count(b[1], b[2], BOX7[1], np.array(BOX7[1]) + np.array(BOX7[2]))
        assert n_ball == spc.ball_count(bd[1], bd[2], lo, hi)
    in_box = spc.contains(box_d, points[0])
    assert in_box.sum() > 1000 and (~in_box).sum() > 2000

    mixed = _mixed_per_level(src)                                        # by depth: the cells of 4^(7 - depth) voxels
    cut_src = {k: spc.box_cut_cells(BOX7[1], BOX7[2], 4 ** k) + sum(_ball_cut_cells(b[1], b[2], 4 ** k) for b in BALLS7) for k in range(1, 7)}
    for k in range(1, 7):
        assert mixed[7 - k] <= cut_src[k], (k, mixed[7 - k], cut_src[k])
    bound = 64 * (1 + sum(spc.box_cut_cells(DST7, dn, 4 ** k) + 8 * cut_src[k] for k in range(2, 7)))

    image, i0 = _export(src), dst.info()
    assert dst.patch_tree_oriented(src, BOX7[1], BOX7[2], DST7, axis=axis, flip=flip, id_map=SWAP7) is dst
    i1 = dst.info()
    print("7 levels, oriented: %d records appended (bound %d), patch_times %r" % (i1.n_nodes - i0.n_nodes, bound, dst.patch_times()))
    assert _export(src) == image
    assert 0 < i1.n_nodes - i0.n_nodes <= bound
    assert dst.garbage() == ppc.expected_garbage(dst)

    def checks(label):
        assert dst.count_diff(want) == 0 and want.count_diff(dst) == 0, label
        assert dst.count_voxels(DST7, dn[::-1]) == volume, label
        assert dst.count_voxels() == volume + int((~in_box).sum()), label
        rng = np.random.default_rng(177)
        rows = []
        for b in BALLS7:                                               # landmarks of src, mapped: a diameter of each ball along src's x
            diam = np.tile(np.array(b[1]), (440, 1))
            diam[:, 0] += np.arange(-220, 220)
            rows.append(np.array([poc.orient_point(tuple(p), BOX7[1], BOX7[2], DST7, axis, flip) for p in diam]))
        corners = [poc.orient_point(tuple(np.array(BOX7[1]) + np.array(c) * (np.array(BOX7[2]) - 1)), BOX7[1], BOX7[2], DST7, axis, flip)
                   for c in np.ndindex(2, 2, 2)]
        faces = lo + rng.integers(0, 900, (400, 3))
        faces[:100, 0], faces[100:200, 0], faces[200:300, 2], faces[300:, 1] = lo[0] - 1, hi[0] - 1, hi[2], lo[1]
        where = np.concatenate([rng.integers(0, E7, (2048, 3)), lo + rng.integers(-100, 1400, (2048, 3))] + rows +
                               [np.array(corners), faces, points[0][:2000], points[0][in_box][:500]]).astype(np.int32)
        where = where[((where >= 0) & (where < E7)).all(1)]
        got = dst.get_blocks_gpu(np.ascontiguousarray(where)).cpu().numpy().view(np.uint16)
        expect = spc.lookup(points, [box_d] + balls_d, keep, where)
        assert np.array_equal(got, expect), "%s: %d lookups differ" % (label, int((got != expect).sum()))
        assert all((expect == v).any() for v in (0, 1, 2, 3))
        # the first ball of src, id 1, is id 3 at its mapped centre; src's first corner is a corner of the destination box
        at = np.array([balls_d[0][1], balls_d[1][1], corners[0]], np.int32)
        assert list(dst.get_blocks_gpu(np.ascontiguousarray(at)).cpu().numpy().view(np.uint16)) == [3, 1, 2]
        assert corners[0] == (DST7[0], DST7[1], DST7[2] + dn[2] - 1)   # src's x runs against dst's z

    checks("pasted")
    mask, kind, _ = _kinds(dst)
    assert not ((kind == K_BRICK) & (mask == 0)).any()
    dst.compact()
    assert dst.garbage() == (0, 0)
    checks("compacted")
    assert _export(src) == image


# ------------------------------------------------------------------------------------------------- 9. refusals --
def test_refusals_on_the_device_path_change_nothing(rt, cuda, worlds):
    t, src = _tree(rt, 3, worlds["old64"]), _tree(rt, 3, worlds["sparse64"])
    t.patch_tree_oriented(src, (0, 0, 0), (20, 20, 20), (5, 5, 5), axis=(2, 1, 0), flip=(0, 0, 1))     # (a tree that already carries garbage)
    g, ceil, quads, times = t.garbage(), t.device_ceilings(), t.device_ceiling_quads(), t.patch_times()
    image, simage = _export(t), _export(src)
    assert g[0] > 0 and times[0] > 0.0

    def unchanged():
        assert _export(t) == image and _export(src) == simage and t.garbage() == g and t.patch_times() == times
        c2 = t.device_ceilings()
        assert c2[0] == ceil[0] and np.array_equal(c2[1], ceil[1]) and np.array_equal(c2[2], ceil[2])
        assert np.array_equal(t.device_ceiling_quads(), quads)

    bad = (dict(src_origin=(0, 0, 0), dims=(20, 20, 20), dst_origin=(50, 5, 5)), dict(src_origin=(60, 0, 0), dims=(5, 5, 5), dst_origin=(0, 0, 0)),
           dict(src_origin=(0, 0, 0), dims=(4, 0, 4), dst_origin=(0, 0, 0)), dict(src_origin=(0, 0, 0), dims=(4, 4, 4), dst_origin=(0, 0, 0), axis=(0, 1, 1)),
           dict(src_origin=(0, 0, 0), dims=(4, 4, 4), dst_origin=(0, 0, 0), flip=(0, 3, 0)),
           dict(src_origin=(0, 0, 0), dims=(40, 4, 4), dst_origin=(0, 30, 0), axis=(1, 0, 2)),
           dict(src_origin=(0, 0, 0), dims=(4, 4, 4), dst_origin=(0, 0, 0), id_map=[1, 1, 2, 3, 4, 5]))
    for kw in bad:
        with pytest.raises(rt.SvoError, match=r"svo_tree_patch_tree_oriented_gpu failed \(-1\)"):
            t.patch_tree_oriented(src, **kw)
        unchanged()
    p = rt.Paste()
    p.n[:], p.axis[:], p.flags = (4, 4, 4), (0, 1, 2), 4
    assert rt.lib().svo_tree_patch_tree_oriented_gpu(t._h, src._h, C.byref(p)) == -1
    unchanged()
    with pytest.raises(rt.SvoError, match=r"svo_tree_patch_tree_oriented_gpu failed \(-5\).*id_map\[3\]"):
        t.patch_tree_oriented(src, (0, 0, 0), (4, 4, 4), (0, 0, 0), id_map=[0, 1, 2, 6, 4, 5])
    unchanged()
    big = rt.Tree.volume_gpu(3, np.array(worlds["sparse64"], np.uint16), PAL + [(1, 12345, 0.0)])
    with pytest.raises(rt.SvoError, match=r"svo_tree_patch_tree_oriented_gpu failed \(-5\).*palette"):
        t.patch_tree_oriented(big, None, None, (0, 0, 0), flip=(1, 0, 0))
    unchanged()
    with pytest.raises(ValueError):
        t.patch_tree_oriented(big, None, None, (0, 0, 0), id_map=[0, 1, 2])                       # one entry per entry of src's palette
    unchanged()
    # unsynced trees on the same device, as src and as dst
    w = rt.World(3)
    w.put_block(5, 6, 7, 0, int(vc.colour(11)))
    u = w.build().upload(0)
    w.put_block(9, 9, 9, 0, int(vc.colour(11)))
    u.update(w, [(9, 9, 9)])
    uimage = _export(u)
    with pytest.raises(rt.SvoError, match=r"svo_tree_patch_tree_oriented_gpu failed \(-4\).*src.*not yet synced"):
        t.patch_tree_oriented(u, None, None, (0, 0, 0), axis=(1, 0, 2))
    unchanged()
    with pytest.raises(rt.SvoError, match=r"svo_tree_patch_tree_oriented_gpu failed \(-4\).*dst.*not yet synced"):
        u.patch_tree_oriented(u, (0, 0, 0), (8, 8, 8), (20, 20, 20), flip=(1, 1, 1))
    assert _export(u) == uimage
    u.sync()
    t.patch_tree_oriented(u, (4, 4, 4), (8, 8, 8), (30, 30, 30), flip=(1, 1, 1))              # synced, it goes through
    assert t.get_block(36, 35, 34)[1] == 1 and t.get_block(32, 32, 32)[1] == 1 and t.patch_times() != times
