"""svo_tree_patch_tree_rule_gpu on the GPU: a box of one resident tree combined into another under a rule that asks both
sides — what src stores (through the orientation and the id map) and what dst stores on entry, in dst's own view.  The
reference for content is numpy (paste_rule_cases.apply_rule, itself checked against a triple loop and against the oriented
paste's model in test_paste_rule_model.py).

Every 64^3 content case runs test_gpu_points_patch's checks (1) .. (5), all exact: read_volume equals the model; after
compact(), export() equals a fresh volume_gpu of the model byte for byte; the ceilings equal the fresh tree's; hit records
are bit-equal to the fresh tree's; garbage() equals the arrays' lengths minus what a walk of export() reaches; no K_BRICK
record has mask 0; and src comes out byte-identical.  At 7 levels the result is checked through closed forms only: against
a third tree given the equivalent shapes, through the diff and the listing's counts, and the growth of the arrays against
a bound derived from the cells the boxes and the ball cut."""
import ctypes as C

import numpy as np
import pytest

import paste_oriented_cases as poc
import paste_rule_cases as prc
import points_patch_cases as ppc
import shapes_patch_cases as spc
import volume_cases as vc
from test_gpu_paste_tree import _ball_cut_cells, _mixed_per_level
from test_gpu_points_patch import NEAR7, _old64, _scatter7, _sparse64, _stored, check_patched
from test_gpu_volume_patch import PAL, _kinds, _tree

pytestmark = pytest.mark.gpu

K_INTERIOR, K_BRICK, K_SOLID = 0, 1, 2
OFF_GRID = ((10, 9, 8), (13, 22, 27), (11, 11, 11))      # three different dimensions, off every grid at both ends
BOTH_BOX = ((6, 6, 6), (30, 20, 25), (19, 22, 7))
NAMES = sorted(prc.NAMED)


@pytest.fixture(scope="module")
def cuda(rt):
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    assert hasattr(rt.lib(), "svo_tree_patch_tree_rule_gpu")
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


@pytest.fixture(scope="module")
def srcs(rt, cuda, worlds):
    """the uploaded source trees, by (world, view), with their stored content; never changed"""
    out = {}
    for w in ("old64", "sparse64"):
        for view in (0, 1):
            out[w, view] = (_tree(rt, 3, worlds[w], view=view), vc.in_view(worlds[w], PAL, view))
    images = {k: _export(t) for k, (t, _) in out.items()}
    yield out
    for k, (t, _) in out.items():
        assert _export(t) == images[k] and t.garbage() == (0, 0), "src %r changed" % (k,)


def _export(t):
    n, m = t.export()
    return n.tobytes(), m.tobytes()


def _name(orient):
    return "axis%d%d%d-flip%d%d%d" % (orient[0] + orient[1])


def rule_and_check(rt, cuda, dst_vol, src, src_dense, box, orient, rule, label, view=0, id_map=None, **kw):
    """a volume-built tree of `dst_vol`, given the box of the uploaded tree `src` (whose stored content is src_dense) in one
    rule call, against the model; src must come out byte-identical"""
    so, dims, do = box
    axis, flip = orient
    t = rt.Tree.volume_gpu(3, np.array(dst_vol, np.uint16), PAL, view=view)
    before = vc.in_view(np.asarray(dst_vol), PAL, view)
    comp = prc.apply_rule(before, src_dense, so, dims, do, axis, flip, id_map, rule, ppc.view_keep(PAL, view))
    image = _export(src), src.garbage(), src.info().n_nodes
    assert t.patch_tree_rule(src, so, dims, do, rule, axis=axis, flip=flip, id_map=id_map) is t
    assert (_export(src), src.garbage(), src.info().n_nodes) == image, "%s: src changed" % label
    check_patched(rt, cuda, t, comp, label, **kw)
    return t, comp, before


# ----------------------------------------------------------------------------------- 1. every rule, both views --
@pytest.mark.parametrize("rule", [r for r in prc.RULES if r], ids=lambda r: "rule%d" % r)
@pytest.mark.parametrize("views", [(0, 0), (1, 1), (0, 1), (1, 0)], ids=lambda v: "src%d-dst%d" % v)
@pytest.mark.parametrize("orient", [poc.IDENTITY, poc.QUARTER_Y], ids=_name)
def test_every_rule_in_both_views(rt, cuda, worlds, srcs, orient, views, rule):
    src, dense = srcs["old64", views[0]]
    so, dims, do = BOTH_BOX
    before = vc.in_view(worlds["old64"], PAL, views[1])
    na, nb, nc = prc.cases_in_box(before, dense, so, dims, do, orient[0], orient[1], None)
    assert na > 0 and nb > 0 and nc > 0                                   # all three cases occur in the box
    comp = prc.apply_rule(before, dense, so, dims, do, orient[0], orient[1], None, rule, ppc.view_keep(PAL, views[1]))
    assert not np.array_equal(comp, before)                               # no rule is tested vacuously
    rule_and_check(rt, cuda, worlds["old64"], src, dense, BOTH_BOX, orient, rule, "rule %d, %s, views %r" % (rule, _name(orient), views),
                   view=views[1], casts=orient == poc.IDENTITY and views[0] == views[1])


# ----------------------------------------------------------------------------------------------- 2. directed cells --
# (src world, dst world, src_origin, dims, dst_origin, src state, dst state): states 0 empty, 1 K_SOLID, None neither
DIRECTED = {
    "a K_SOLID 16^3 onto a K_SOLID 16^3": ("old64", "old64", (0, 0, 0), (16, 16, 16), (0, 0, 0), 1, 1),
    "a K_SOLID 16^3 onto an empty 16^3": ("old64", "sparse64", (0, 0, 0), (16, 16, 16), (48, 48, 48), 1, 0),
    "a K_SOLID 16^3 across dst's centre": ("old64", "old64", (0, 0, 0), (16, 16, 16), (25, 23, 26), 1, None),
    "src's empty 16^3 onto a K_SOLID 16^3": ("sparse64", "old64", (48, 48, 48), (16, 16, 16), (0, 0, 0), 0, 1),
    "src's empty 16^3 onto an empty 16^3": ("sparse64", "sparse64", (48, 48, 48), (16, 16, 16), (48, 48, 48), 0, 0),
    "src's empty 16^3 across dst's centre": ("sparse64", "old64", (48, 48, 48), (16, 16, 16), (25, 23, 26), 0, None),
    "a one-voxel box": ("old64", "old64", (21, 22, 20), (1, 1, 1), (38, 5, 19), None, None),
    "one src brick off dst's grid": ("old64", "old64", (40, 24, 36), (4, 4, 4), (17, 30, 41), None, None),
    "the whole extent": ("old64", "sparse64", None, None, (0, 0, 0), None, None),
}


def _table_says_out(rule, s_state, d_state):
    """the rows of the cell table that answer OUT for every cell the box meets: src empty and C keeps or dst empty too; src
    of one id over an empty dst and A keeps, over a K_SOLID dst and B keeps, over anything (d_state None) and A and B keep"""
    a, b, c = prc.fields(rule)
    if s_state == 0:
        return c == prc.KEEP or d_state == 0
    if s_state == 1:
        return (d_state == 0 and a == prc.KEEP) or (d_state == 1 and b == prc.KEEP) or (a == prc.KEEP and b == prc.KEEP)
    return False


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("case", sorted(DIRECTED))
def test_directed_cells(rt, cuda, worlds, srcs, case, name):
    src_world, dst_world, so, dims, do, s_state, d_state = DIRECTED[case]
    rule = prc.NAMED[name]
    src, dense = srcs[src_world, 0]
    label = "%s, %s" % (case, name)
    t = _tree(rt, 3, worlds[dst_world])
    before = vc.in_view(worlds[dst_world], PAL, 0)
    comp = prc.apply_rule(before, dense, so, dims, do, (0, 1, 2), (0, 0, 0), None, rule, ppc.view_keep(PAL, 0))
    n0, nodes0 = t.info().n_nodes, t.export()[0].copy()
    assert t.patch_tree_rule(src, so, dims, do, rule) is t
    grown = t.info().n_nodes - n0
    nodes1 = t.export()[0]
    assert grown >= 0 and int((nodes1[:n0] != nodes0).any(1).sum()) <= 1, label    # never a restart: one record rewritten in place
    if s_state is not None:
        # a 16^3 = (4^2)^3 box of a 3-level tree, aligned or across the centre.  The cells of 16^3 lie at depth levels - 2.
        # patch_anchor descends from the root only while the box lies inside one child region without filling it: an aligned
        # 16^3 box fills a child of the root and one across the centre lies in several, so the anchor is the root, depth 0.
        # The path from the anchor to a cell then holds cell_depth - anchor_depth child blocks, each re-emitted with at most
        # 64 records
        cell_depth, anchor_depth = t.info().levels - 2, 0
        assert dims == (16, 16, 16) and (all(v % 16 == 0 for v in do) or all(v < 32 < v + 16 for v in do))
        if _table_says_out(rule, s_state, d_state):
            assert np.array_equal(comp, before), label
            assert grown <= 64 * (cell_depth - anchor_depth), "%s: %d records appended over a cell that is OUT" % (label, grown)
            if d_state == 1:                                              # the K_SOLID record was copied, not re-made from voxels
                ni = int(t.node_indices([(do[0], do[1], do[2])])[0])
                _, kind, mat = _kinds(t)
                assert kind[ni] == K_SOLID and mat[ni] == 4
        elif d_state is not None:
            assert grown <= 64 * (cell_depth - anchor_depth)              # uniform against uniform is decided at the cell
    if case == "the whole extent":
        assert t.garbage()[0] > 0 or np.array_equal(comp, before), label
    if case == "a K_SOLID 16^3 across dst's centre" and name in ("OVER", "REPLACE"):
        ni = int(t.node_indices([(32, 32, 32)])[0])                       # whole bricks inside stay one-record cells
        _, kind, mat = _kinds(t)
        assert kind[ni] == K_SOLID and mat[ni] == 4 and int(t.node_indices([(35, 35, 35)])[0]) == ni
    check_patched(rt, cuda, t, comp, label, casts=name in ("UNDER", "ERASE"))


# ------------------------------------------------------------------------------------------------ 3. equivalences --
SIX = [poc.ORIENTATIONS[i] for i in (0, 5, 13, 22, 36, 47)]


@pytest.mark.parametrize("orient", SIX, ids=_name)
def test_replace_and_over_are_the_oriented_paste(rt, cuda, worlds, srcs, orient):
    src, _ = srcs["old64", 0]
    so, dims, do = OFF_GRID
    for id_map in (None, [0, 2, 2, 0, 4, 5]):
        for rule, keep in ((prc.REPLACE, False), (prc.OVER, True)):
            a, b = _tree(rt, 3, worlds["sparse64"]), _tree(rt, 3, worlds["sparse64"])
            a.patch_tree_oriented(src, so, dims, do, axis=orient[0], flip=orient[1], id_map=id_map, keep_empty=keep)
            b.patch_tree_rule(src, so, dims, do, rule, axis=orient[0], flip=orient[1], id_map=id_map)
            assert np.array_equal(_stored(a), _stored(b))
            a.compact()
            b.compact()
            assert _export(a) == _export(b) and a.info().n_nodes == b.info().n_nodes, (orient, id_map, rule)
            ca, cb = a.device_ceilings(), b.device_ceilings()
            assert ca[0] == cb[0] and np.array_equal(ca[1], cb[1]) and np.array_equal(ca[2], cb[2])


# ----------------------------------------------------------------------------------------------------- 4. algebra --
def test_algebra(rt, cuda, worlds, srcs):
    src, dense = srcs["old64", 0]
    so, dims, do = BOTH_BOX
    keep = ppc.view_keep(PAL, 0)
    old = vc.in_view(worlds["old64"], PAL, 0)
    ident = ((0, 1, 2), (0, 0, 0), None)
    s = prc.mapped_box(dense, so, dims, *ident)
    sl = (slice(do[2], do[2] + dims[2]), slice(do[1], do[1] + dims[1]), slice(do[0], do[0] + dims[0]))
    # ERASE then UNDER of the same box: d where it was kept, s elsewhere in the box
    t = _tree(rt, 3, worlds["old64"])
    t.patch_tree_rule(src, so, dims, do, rt.RULE_ERASE).patch_tree_rule(src, so, dims, do, rt.RULE_UNDER)
    want = prc.apply_rule(prc.apply_rule(old, dense, so, dims, do, *ident, prc.ERASE, keep), dense, so, dims, do, *ident, prc.UNDER, keep)
    got = _stored(t)
    assert np.array_equal(got, want)
    assert np.array_equal(got[sl], np.where(s != 0, np.where(keep[s], s, 0), old[sl])) and (s != 0).any() and ((s == 0) & (old[sl] != 0)).any()
    # XOR twice with a single-id src restores dst's occupancy in the box
    ones = [0, 1, 1, 1, 1, 1]
    t = _tree(rt, 3, worlds["old64"])
    t.patch_tree_rule(src, so, dims, do, rt.RULE_XOR, id_map=ones)
    once = _stored(t)
    assert np.array_equal(once[sl] != 0, (old[sl] != 0) ^ (s != 0))
    t.patch_tree_rule(src, so, dims, do, rt.RULE_XOR, id_map=ones)
    twice = _stored(t)
    assert np.array_equal(twice != 0, old != 0) and not np.array_equal(once != 0, old != 0)
    assert (twice[sl][(s != 0) & (old[sl] == 0)] == 0).all() and (twice[sl][(s != 0) & (old[sl] != 0)] == 1).all()
    # MASK followed by STENCIL equals STENCIL alone
    a, b = _tree(rt, 3, worlds["old64"]), _tree(rt, 3, worlds["old64"])
    a.patch_tree_rule(src, so, dims, do, rt.RULE_MASK).patch_tree_rule(src, so, dims, do, rt.RULE_STENCIL)
    b.patch_tree_rule(src, so, dims, do, rt.RULE_STENCIL)
    assert np.array_equal(_stored(a), _stored(b))
    assert np.array_equal(_stored(b), prc.apply_rule(old, dense, so, dims, do, *ident, prc.STENCIL, keep))
    a.compact()
    b.compact()
    assert _export(a) == _export(b)


# ---------------------------------------------------------------------------------------------------- 5. src == dst --
@pytest.mark.parametrize("name", ["UNDER", "ERASE"])
@pytest.mark.parametrize("orient", [poc.IDENTITY, poc.QUARTER_Y], ids=_name)
def test_self_paste(rt, cuda, worlds, orient, name):
    so, dims, do = (20, 22, 18), (20, 20, 20), (27, 17, 25)              # overlapping boxes
    old = vc.in_view(worlds["old64"], PAL, 0)
    t = _tree(rt, 3, worlds["old64"])
    t.patch_points(np.array([[1, 1, 1]], np.int32), np.array([2], np.uint16))    # (a tree that already carries garbage)
    old[1, 1, 1] = 2
    assert t.garbage()[0] > 0
    comp = prc.apply_rule(old, old, so, dims, do, orient[0], orient[1], None, prc.NAMED[name], ppc.view_keep(PAL, 0))   # the content on entry only
    assert t.patch_tree_rule(t, so, dims, do, prc.NAMED[name], axis=orient[0], flip=orient[1]) is t
    assert not np.array_equal(comp, old)
    check_patched(rt, cuda, t, comp, "self, %s, %s" % (name, _name(orient)))


# ------------------------------------------------------------------------------------------ 6. the views diverge --
def test_the_two_views_of_one_world_diverge_under_a_rule_that_reads_dst(rt, cuda, worlds):
    """UNDER of a solid material over a liquid voxel: d is read in dst's own view, so the solid-view tree (d == 0) stores the
    solid and the full-view tree (d == 5) keeps the liquid — the two trees are no longer the two views of one world"""
    world = worlds["old64"]
    z, y, x = (int(v[0]) for v in np.nonzero(world == 5))
    vol = np.zeros((64, 64, 64), np.uint16)
    vol[max(0, z - 3):z + 4, max(0, y - 3):y + 4, max(0, x - 3):x + 4] = 2
    src = _tree(rt, 3, vol)
    a, b = _tree(rt, 3, world, view=0), _tree(rt, 3, world, view=1)
    for t in (a, b):
        t.patch_tree_rule(src, None, None, (0, 0, 0), rt.RULE_UNDER)
    sa, sb = _stored(a), _stored(b)
    assert sa[z, y, x] == 2 and sb[z, y, x] == 5
    assert not np.array_equal(sa, vc.in_view(sb, PAL, 0))
    for t, got, view in ((a, sa, 0), (b, sb, 1)):
        comp = prc.apply_rule(vc.in_view(world, PAL, view), vol, None, None, (0, 0, 0), (0, 1, 2), (0, 0, 0), None, prc.UNDER, ppc.view_keep(PAL, view))
        assert np.array_equal(got, comp)
        check_patched(rt, cuda, t, comp, "views diverge, view %d" % view, casts=False)


# ------------------------------------------------------------------------------- 7. the layouts the patches leave --
def test_layouts_the_patches_leave(rt, cuda, worlds):
    src = _tree(rt, 3, worlds["sparse64"])
    src.patch_points(np.array([[5, 5, 60]], np.int32), np.ones(1, np.uint16))      # a voxel into an empty 16^3, and out again:
    src.patch_points(np.array([[5, 5, 60]], np.int32), np.zeros(1, np.uint16))     # an interior record with mask 0
    src.patch_shapes([rt.ball((30, 30, 30), 400, 3), rt.box((2, 20, 2), (40, 9, 30), 4)])          # and superseded records
    mask, kind, _ = _kinds(src)
    assert ((kind == K_INTERIOR) & (mask == 0)).any() and src.garbage()[0] > 0
    dense = _stored(src)
    box = ((3, 5, 2), (50, 41, 47), (9, 14, 11))
    keep = ppc.view_keep(PAL, 0)

    def patched_dst():
        t = _tree(rt, 3, worlds["old64"])
        t.patch_shapes([rt.ball((40, 30, 28), 150, 0), rt.box((20, 30, 40), (9, 9, 9), 2)])
        return t

    results = {}
    for layout in ("patched src", "compacted src"):
        if layout == "compacted src":
            src.compact()
            assert src.garbage() == (0, 0) and np.array_equal(_stored(src), dense)
        for kind_of_dst, make in (("fresh dst", lambda: _tree(rt, 3, worlds["old64"])), ("patched dst", patched_dst)):
            t = make()
            before = _stored(t)
            assert (t.garbage()[0] > 0) == (kind_of_dst == "patched dst")
            image = _export(src)
            t.patch_tree_rule(src, *box, rt.RULE_PAINT)
            assert _export(src) == image
            comp = prc.apply_rule(before, dense, *box, (0, 1, 2), (0, 0, 0), None, prc.PAINT, keep)
            assert not np.array_equal(comp, before)
            check_patched(rt, cuda, t, comp, "%s, %s" % (layout, kind_of_dst), casts=False)     # (compacts)
            results[layout, kind_of_dst] = _export(t)
    for kind_of_dst in ("fresh dst", "patched dst"):
        assert results["patched src", kind_of_dst] == results["compacted src", kind_of_dst]


# --------------------------------------------------------------------------------------- 8. sequences and capacity --
def test_twenty_rule_pastes_past_the_upload_slack(rt, cuda):
    E = 256
    comp = vc.random_volume((E, E, E), 0.02, 41, ids=(1, 2, 3, 4))
    comp[30:100, 40:120, 50:130] = 2                                   # solid regions for the rules that need d != 0
    src_vol = vc.random_volume((E, E, E), 0.03, 43, ids=(1, 2, 3, 4))
    src_vol[64:128, 64:128, 64:128] = 3                                  # a K_SOLID 64^3 and an empty one
    src_vol[128:192, 64:128, 64:128] = 0
    t, src = _tree(rt, 4, comp), _tree(rt, 4, src_vol)
    image = _export(src)
    keep_ids = ppc.view_keep(PAL, 0)
    n0, bytes_seen, garbage = t.info().n_nodes, [t.info().device_bytes], [t.garbage()]
    rng = np.random.default_rng(139)
    rules = [r for r in prc.RULES if r]
    for i in range(20):
        axis, flip = poc.ORIENTATIONS[int(rng.integers(0, 48))]
        dims = tuple(int(v) for v in rng.integers(70, 130, 3))
        dn = poc.dst_dims(dims, axis)
        so = tuple(int(rng.integers(0, E - d + 1)) for d in dims)
        do = tuple(int(rng.integers(0, E - d + 1)) for d in dn)
        rule, id_map = rules[i % len(rules)], ([0, 2, 3, 1, 0, 5] if i % 4 == 2 else None)
        t.patch_tree_rule(src, so, dims, do, rule, axis=axis, flip=flip, id_map=id_map)
        comp = prc.apply_rule(comp, src_vol, so, dims, do, axis, flip, id_map, rule, keep_ids)
        bytes_seen.append(t.info().device_bytes)
        garbage.append(t.garbage())
        assert cuda.equal(t.read_volume((0, 0, 0), (E, E, E)), cuda.from_numpy(comp.view(np.int16)).cuda()), "(1) step %d: %r" % (i, (so, dims, do, axis, flip, rule))
    assert _export(src) == image
    assert t.info().n_nodes > n0
    assert any(b > a for a, b in zip(bytes_seen, bytes_seen[1:]))      # past the slack of the upload: the arrays were reallocated
    assert all(b[0] > a[0] and b[1] >= a[1] for a, b in zip(garbage, garbage[1:]))   # never a restart
    check_patched(rt, cuda, t, comp, "20 rule pastes", casts=False)       # (compacts)


# ---------------------------------------------------------------------------------------------------- 9. 7 levels --
E7 = 4 ** 7
BOXD = ("box", (7001, 7003, 7005), (1300, 1300, 1300), 1)             # dst's region of id 1: 2.2 * 10^9 voxels, around NEAR7
R2 = 40000
# (the paste: src_origin, dims, dst_origin; the ball's centre in src).  "inside": the paste box is dst's region and the ball
# lies wholly in it; "across": a 440^3 paste box that holds the ball, whose centre lies 30 voxels inside the region's -x face
PLACE7 = {
    "inside": ((3002, 5001, 9003), (1300, 1300, 1300), BOXD[1], (3602, 5701, 9503)),
    "across": ((1001, 2002, 3002), (440, 440, 440), (6811, 7383, 7435), (1221, 2222, 3222)),
}
RULES7 = {"ERASE": ("across", 1), "UNDER": ("across", 5), "PAINT": ("inside", 2), "MASK": ("inside", 1)}   # (placement, the ball's id)


def _dst_cells_under_ball(centre, r2, region, xyz, cs):
    """the aligned cells of cs^3 voxels that meet the ball's bounding box and in which dst holds a record of their level: those
    the region's surface cuts (met by the region, not wholly inside it), plus one per point of the scatter whose cell meets
    the bounding box (a point in a cell the region cuts is counted twice: an upper bound)"""
    r = int(np.sqrt(float(r2)))
    r += (r + 1) ** 2 <= r2
    blo, bhi = np.array(centre) - r, np.array(centre) + r + 1
    lo, hi = np.array(region[1]), np.array(region[1]) + np.array(region[2])
    met, inside = [], []
    for a in range(3):
        o = np.arange(blo[a] // cs, (bhi[a] - 1) // cs + 1, dtype=np.int64) * cs
        met.append((o + cs > lo[a]) & (o < hi[a]))
        inside.append((o >= lo[a]) & (o + cs <= hi[a]))
    met3 = met[2][:, None, None] & met[1][None, :, None] & met[0][None, None, :]
    in3 = inside[2][:, None, None] & inside[1][None, :, None] & inside[0][None, None, :]
    o = np.asarray(xyz, np.int64) // cs * cs
    return int((met3 & ~in3).sum()) + int(((o + cs > blo) & (o < bhi)).all(1).sum())


@pytest.mark.parametrize("name", sorted(RULES7))
def test_seven_levels(rt, cuda, name):
    """dst: the 7-level scatter with a 1300^3 region of id 1; src: an empty 7-level tree with one ball.  Closed forms only.

    The growth bound.  Every appended record lies in the child block of a cut cell above the brick level (or of the anchor),
    at most 64 per block.  A destination cell of 4^k voxels is cut only where the paste box's surface cuts it —
    box_cut_cells(paste box, 4^k) cells —, where it meets a source cell of its level that src holds as a record of that
    level — src holds such records only where the ball's surface cuts a cell, and a source cell meets at most 2 x 2 x 2
    destination cells —, or where dst itself holds a record of that level under a non-empty src region.  dst holds such
    records only where the surface of its region cuts a cell or a point of the scatter lies in one (one cell per point and
    level), and src stores something only in the ball, so the third term counts those cells among the ones that meet the
    ball's bounding box (_dst_cells_under_ball), not all of dst's.  Both facts about the trees are checked on their
    exports before the bound is used."""
    place, ball_id = RULES7[name]
    so, dims, do, c_src = PLACE7[place]
    rule = prc.NAMED[name]
    view = 1 if name == "UNDER" else 0                                    # (id 5 is the liquid: only the full view stores it)
    keep = ppc.view_keep(PAL, view)
    shift = np.array(do) - np.array(so)
    assert (shift % 4 != 0).all()                                         # on no grid
    c_dst = tuple(int(v) for v in np.array(c_src) + shift)
    ball_d = ("ball", c_dst, R2, ball_id)
    lo, hi = np.array(BOXD[1]), np.array(BOXD[1]) + np.array(BOXD[2])
    plo, phi = np.array(do), np.array(do) + np.array(dims)
    assert (phi <= E7).all() and ((lo <= np.array(NEAR7)) & (np.array(NEAR7) < hi)).all()
    n_ball = spc.ball_count(c_dst, R2, (0, 0, 0), (E7, E7, E7))
    n_ball_in = spc.ball_count(c_dst, R2, lo, hi)
    assert n_ball == spc.ball_count(c_dst, R2, plo, phi)                  # the paste box holds the whole ball
    assert (n_ball_in == n_ball) if place == "inside" else (0 < n_ball_in < n_ball)

    xyz, ids = _scatter7()
    outside_in_ball = spc.contains(ball_d, xyz) & ~spc.contains(BOXD, xyz)
    xyz, ids = xyz[~outside_in_ball], ids[~outside_in_ball]               # no point of the scatter in the ball outside the region
    assert not (spc.contains(ball_d, xyz) & ~spc.contains(BOXD, xyz)).any() and len(xyz) > 4000
    points = ppc.resolve_edits(xyz, ids, keep)
    points = (points[0][points[1] != 0], points[1][points[1] != 0])
    in_box = spc.contains(BOXD, points[0])
    assert in_box.sum() > 1000 and (~in_box).sum() > 2000

    src = rt.Tree.points_gpu(7, np.zeros((0, 3), np.int32), np.zeros(0, np.uint16), PAL, view=view)
    src.patch_shapes(spc.to_abi(rt, [("ball", c_src, R2, ball_id)]))
    assert src.count_voxels() == n_ball
    dst, want, base = (rt.Tree.points_gpu(7, xyz, ids, PAL, view=view) for _ in range(3))
    dst.patch_shapes(spc.to_abi(rt, [BOXD]))
    base.patch_shapes(spc.to_abi(rt, [BOXD]))
    volume = 1300 ** 3
    assert dst.count_voxels(BOXD[1], BOXD[2]) == volume
    equivalent = {"ERASE": [BOXD, ("ball", c_dst, R2, 0)], "UNDER": [ball_d, BOXD], "PAINT": [BOXD, ball_d],
                  "MASK": [("box", BOXD[1], BOXD[2], 0), ball_d]}[name]
    want.patch_shapes(spc.to_abi(rt, equivalent))

    # the bound, from the cells the shapes cut
    cut_src = {k: _ball_cut_cells(c_src, R2, 4 ** k) for k in range(1, 7)}
    cut_dst = {k: spc.box_cut_cells(BOXD[1], BOXD[2], 4 ** k) + len(points[0]) for k in range(1, 7)}
    mixed_src, mixed_dst = _mixed_per_level(src), _mixed_per_level(dst)
    for k in range(1, 7):
        assert mixed_src[7 - k] <= cut_src[k] and mixed_dst[7 - k] <= cut_dst[k], (k, mixed_src[7 - k], cut_src[k], mixed_dst[7 - k], cut_dst[k])
    under_ball = {k: _dst_cells_under_ball(c_dst, R2, BOXD, points[0], 4 ** k) for k in range(2, 7)}
    assert all(under_ball[k] <= cut_dst[k] for k in range(2, 7)) and (under_ball[2] > 0) == (place == "across")   # the region's face in the ball
    bound = 64 * (1 + sum(spc.box_cut_cells(do, dims, 4 ** k) + 8 * cut_src[k] + under_ball[k] for k in range(2, 7)))
    assert bound < volume // 400

    image, i0 = _export(src), dst.info()
    assert dst.patch_tree_rule(src, so, dims, do, rule) is dst
    i1 = dst.info()
    print("7 levels, %s: %d records appended (bound %d), patch_times %r" % (name, i1.n_nodes - i0.n_nodes, bound, dst.patch_times()))
    assert _export(src) == image
    assert 0 < i1.n_nodes - i0.n_nodes <= bound
    assert dst.garbage() == ppc.expected_garbage(dst) and dst.garbage()[0] > 0

    def checks(label):
        if name == "MASK":
            assert dst.count_diff(want, BOXD[1], BOXD[2][::-1]) == 0 and want.count_diff(dst, BOXD[1], BOXD[2][::-1]) == 0, label
            assert dst.count_voxels(BOXD[1], BOXD[2][::-1]) == n_ball, label
            assert dst.count_voxels() == n_ball + int((~in_box).sum()), label
            assert dst.count_diff(base) == volume - n_ball, label
        else:
            assert dst.count_diff(want) == 0 and want.count_diff(dst) == 0, label
        if name == "ERASE":
            assert dst.count_voxels(BOXD[1], BOXD[2][::-1]) == volume - n_ball_in, label
            assert dst.count_voxels() == volume - n_ball_in + int((~in_box).sum()), label
            assert dst.count_diff(base) == n_ball_in, label
        elif name == "UNDER":
            assert dst.count_voxels(BOXD[1], BOXD[2][::-1]) == volume, label
            assert dst.count_voxels() == volume + (n_ball - n_ball_in) + int((~in_box).sum()), label
            assert dst.count_diff(base) == n_ball - n_ball_in, label
        elif name == "PAINT":
            assert dst.count_voxels() == volume + int((~in_box).sum()), label
            assert dst.count_diff(base) == n_ball, label
        at = np.array([c_dst, tuple(lo), tuple(hi - 1), (c_dst[0] - 150, c_dst[1], c_dst[2])], np.int32)
        got = list(dst.get_blocks_gpu(np.ascontiguousarray(at)).cpu().numpy().view(np.uint16))
        assert got == {"ERASE": [0, 1, 1, 0], "UNDER": [1, 1, 1, 5], "PAINT": [2, 1, 1, 2], "MASK": [1, 0, 0, 1]}[name], (label, got)

    checks("pasted")
    mask, kind, _ = _kinds(dst)
    assert not ((kind == K_BRICK) & (mask == 0)).any()
    dst.compact()
    assert dst.garbage() == (0, 0)
    checks("compacted")
    assert _export(src) == image


# ----------------------------------------------------------------------------------- 10. rule 0 and the refusals --
def test_rule_0_and_refusals_on_the_device_change_nothing(rt, cuda, worlds):
    t, src = _tree(rt, 3, worlds["old64"]), _tree(rt, 3, worlds["sparse64"])
    t.patch_tree_rule(src, (0, 0, 0), (20, 20, 20), (5, 5, 5), rt.RULE_XOR, axis=(2, 1, 0), flip=(0, 0, 1))     # (a tree that already carries garbage)
    g, ceil, quads, times, n_nodes = t.garbage(), t.device_ceilings(), t.device_ceiling_quads(), t.patch_times(), t.info().n_nodes
    image, simage, content, scontent = _export(t), _export(src), _stored(t), _stored(src)
    assert g[0] > 0 and times[0] > 0.0

    def unchanged():
        assert _export(t) == image and _export(src) == simage and t.garbage() == g and t.patch_times() == times and t.info().n_nodes == n_nodes
        c2 = t.device_ceilings()
        assert c2[0] == ceil[0] and np.array_equal(c2[1], ceil[1]) and np.array_equal(c2[2], ceil[2])
        assert np.array_equal(t.device_ceiling_quads(), quads)
        assert np.array_equal(_stored(t), content) and np.array_equal(_stored(src), scontent)           # on the device too

    # rule 0 keeps everything: SVO_OK, and nothing moves
    assert t.patch_tree_rule(src, (0, 0, 0), (40, 30, 20), (7, 9, 11), 0, axis=(1, 2, 0), flip=(1, 0, 1)) is t
    unchanged()
    assert t.patch_tree_rule(t, None, None, (0, 0, 0), rt.paste_rule(rt.RULE_KEEP, rt.RULE_KEEP, rt.RULE_KEEP)) is t
    unchanged()
    for rule in (2, 3, 3 << 2, 1 << 4, 3 << 4, 1 << 6, 5 | 1 << 31):
        with pytest.raises(rt.SvoError, match=r"svo_tree_patch_tree_rule_gpu failed \(-1\).*rule"):
            t.patch_tree_rule(src, (0, 0, 0), (20, 20, 20), (5, 5, 5), rule)
        unchanged()
    bad = (dict(src_origin=(0, 0, 0), dims=(20, 20, 20), dst_origin=(50, 5, 5)), dict(src_origin=(60, 0, 0), dims=(5, 5, 5), dst_origin=(0, 0, 0)),
           dict(src_origin=(0, 0, 0), dims=(4, 0, 4), dst_origin=(0, 0, 0)), dict(src_origin=(0, 0, 0), dims=(4, 4, 4), dst_origin=(0, 0, 0), axis=(0, 1, 1)),
           dict(src_origin=(0, 0, 0), dims=(4, 4, 4), dst_origin=(0, 0, 0), flip=(0, 3, 0)),
           dict(src_origin=(0, 0, 0), dims=(4, 4, 4), dst_origin=(0, 0, 0), id_map=[1, 1, 2, 3, 4, 5]))
    for kw in bad:
        for rule in (0, rt.RULE_UNDER):                                   # rule 0 is checked like any other
            with pytest.raises(rt.SvoError, match=r"svo_tree_patch_tree_rule_gpu failed \(-1\)"):
                t.patch_tree_rule(src, rule=rule, **kw)
            unchanged()
    p = rt.Paste()
    p.n[:], p.axis[:], p.flags = (4, 4, 4), (0, 1, 2), 1                   # svo_paste's flags must be 0
    assert rt.lib().svo_tree_patch_tree_rule_gpu(t._h, src._h, C.byref(p), rt.RULE_OVER) == -1
    unchanged()
    with pytest.raises(rt.SvoError, match=r"svo_tree_patch_tree_rule_gpu failed \(-5\).*id_map\[3\]"):
        t.patch_tree_rule(src, (0, 0, 0), (4, 4, 4), (0, 0, 0), rt.RULE_PAINT, id_map=[0, 1, 2, 6, 4, 5])
    unchanged()
    big = rt.Tree.volume_gpu(3, np.array(worlds["sparse64"], np.uint16), PAL + [(1, 12345, 0.0)])
    with pytest.raises(rt.SvoError, match=r"svo_tree_patch_tree_rule_gpu failed \(-5\).*palette"):
        t.patch_tree_rule(big, None, None, (0, 0, 0), rt.RULE_ERASE, flip=(1, 0, 0))
    unchanged()
    t.patch_tree_rule(src, (0, 0, 0), (20, 20, 20), (5, 5, 5), rt.RULE_XOR, axis=(2, 1, 0), flip=(0, 0, 1))     # and a valid one goes through
    assert not np.array_equal(_stored(t), content) and t.patch_times() != times
