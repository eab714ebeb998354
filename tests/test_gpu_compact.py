"""svo_tree_compact_gpu on the GPU: a resident tree that edits have grown — svo_tree_patch_volume_gpu's appended child
blocks, svo_tree_update's rewritten ones, regions that ended up uniform or empty without being collapsed — comes back as
the canonical linearisation of its own content, which every builder here emits byte for byte.  The expected arrays
therefore exist already: Tree.volume_gpu of the numpy composite (comp = old.copy(); comp[box] = new), and World.build()
for a tree that still follows a World.

"Equals fresh" (equals_fresh below), against Tree.volume_gpu(levels, comp, palette, view): export() of nodes and material
entries byte for byte; info() n_nodes, n_bricks, n_mat_bytes, nodes_per_level, device_bytes; garbage() == (0, 0); the
ceilings, pairs and quads in HBM; read_volume of the whole extent equals the in-view composite; frames from
test_gpu_degenerate_trees.CAMS with flags 0 and CAST_NO_CEILINGS equal in every field of the hit record (a VIEW_ALL tree
is no cast target: it is walked as the scene of the shading pass, colours and hit records equal); no guard trips.

Most cases are 3 levels (64^3) over test_gpu_volume_patch's old world; one is 4 levels (256^3).  Trees above 2^28 nodes
take the same kernels through 64-bit addressing and are not built here (tests/test_gpu_large.py's shapes are too slow to
repeat)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import edit_script as es  # noqa: E402
import palette_cases as pc  # noqa: E402
import volume_cases as vc  # noqa: E402
from test_gpu_degenerate_trees import CAMS  # noqa: E402
from test_gpu_parity import compare  # noqa: E402
from test_gpu_patched_trees import CAMS as EDIT_CAMS, cam_at  # noqa: E402
from test_gpu_volume_build import _same_ceilings  # noqa: E402
from test_gpu_volume_patch import (BOXES, K_BRICK, K_INTERIOR, K_SOLID, PAL, _case1, _kinds, _put, _tree, check_casts,  # noqa: E402
                                   check_content, old64)  # noqa: F401  (old64: the fixture, by import)
from test_patched_host import check_box  # noqa: E402

pytestmark = pytest.mark.gpu

K_UNIFORM = 4
PALW = pc.stored_palette(pc.WIDE_TABLE)


@pytest.fixture(scope="module")
def cuda(rt):
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    assert hasattr(rt.lib(), "svo_tree_compact_gpu")
    return torch


def _same_arrays(a, b, label):
    (na, ma), (nb, mb) = a, b
    assert na.shape == nb.shape and na.tobytes() == nb.tobytes(), "%s: node arrays differ (%d / %d records)" % (label, len(na), len(nb))
    assert ma.shape == mb.shape and ma.tobytes() == mb.tobytes(), "%s: material entries differ (%d / %d)" % (label, len(ma), len(mb))


def equals_fresh(rt, cuda, t, comp, view, label, levels=3, pal=PAL, shift=(0.0, 0.0, 0.0)):
    fresh = _tree(rt, levels, comp, view, pal)
    _same_arrays(t.export(), fresh.export(), label)
    a, b = t.info(), fresh.info()
    for f in ("n_nodes", "n_bricks", "n_mat_bytes", "device_bytes"):
        assert getattr(a, f) == getattr(b, f), "%s: %s %d, fresh %d" % (label, f, getattr(a, f), getattr(b, f))
    assert list(a.nodes_per_level) == list(b.nodes_per_level), label
    assert t.garbage() == (0, 0), label
    _same_ceilings(t, fresh, label + ": ceilings")
    E = comp.shape[0]
    got = t.read_volume((0, 0, 0), (E, E, E)).cpu().numpy().view(np.uint16)
    assert np.array_equal(got, vc.in_view(comp, pal, view)), label + ": content"
    if view == 0:
        check_casts(rt, cuda, t, fresh, label, shift=shift)
    else:
        solid = _tree(rt, levels, comp, 0, pal)
        for ci, (org, d) in enumerate(CAMS):
            dn = rt.normalize(d)
            (ca, ha), (cb, hb) = (solid.shade_frame(org, dn, 64, 32, 300, scene=s, time=0.25, with_hits=True) for s in (t, fresh))
            assert cuda.equal(ca, cb), "%s cam%d colours" % (label, ci)
            for k in ("pos_steps", "t", "info"):
                assert cuda.equal(ha[k], hb[k]), "%s cam%d %s" % (label, ci, k)
        assert t.guard_trips() == 0 and solid.guard_trips() == 0, label
    return fresh


def record_at(t, x, y, z, depth, levels=3):
    """(index, mask, kind, material) of the record of `depth` on the voxel's path; None where a slot bit above it is clear
    or the path ends in a leaf above it"""
    nodes = t.export()[0]
    n = 0
    for d in range(depth + 1):
        mask, ref, info = int(nodes[n, 0]), int(nodes[n, 1]) & 0xFFFFFFFF, int(nodes[n, 1]) >> 32
        if d == depth:
            return n, mask, info & 7, info >> 16
        if info & 3 != K_INTERIOR:
            return None
        sh = 2 * (levels - 1 - d)
        sl = (((z >> sh) & 3) << 4) | (((y >> sh) & 3) << 2) | ((x >> sh) & 3)
        if not (mask >> sl) & 1:
            return None
        n = ref + bin(mask & ((1 << sl) - 1)).count("1")


def patched(rt, vol, steps, view=0, pal=PAL, levels=3):
    """(tree of `vol` after the patches [(voxels, origin)], the composite)"""
    t = _tree(rt, levels, vol, view, pal)
    comp = vol
    for vox, at in steps:
        t.patch_volume(vox, at)
        comp = _put(comp, vox, at)
    return t, comp


def full(shape_zyx, ident):
    return np.full(shape_zyx, ident, np.uint16)


# ----------------------------------------------------------------------------------------- 1. a fixed point --
@pytest.mark.parametrize("view", [0, 1])
def test_a_canonical_tree_is_a_fixed_point(rt, cuda, old64, view):
    t = _tree(rt, 3, old64, view)
    before, bytes_before = t.export(), t.info().device_bytes
    assert t.compact() is t
    _same_arrays(t.export(), before, "fixed point, view %d" % view)
    assert t.info().device_bytes == bytes_before and t.garbage() == (0, 0)
    t.compact()  # (and again, over arrays the compaction itself allocated)
    _same_arrays(t.export(), before, "fixed point twice, view %d" % view)


# ---------------------------------------------------------------------- 2. patched, then compacted, equals fresh --
@pytest.mark.parametrize("view", [0, 1])
@pytest.mark.parametrize("which", sorted(BOXES))
def test_patched_then_compacted_equals_fresh(rt, cuda, old64, which, view):
    t, comp, origin, new = _case1(rt, old64, which, view)
    g, n = t.garbage(), t.info().n_nodes
    assert g[0] > 0
    t.compact()
    assert t.info().n_nodes < n
    equals_fresh(rt, cuda, t, comp, view, "%s view %d" % (which, view))
    check_content(t, comp, view, origin, new.shape)


# ------------------------------------------------------------------------------------------------ 3. re-collapse --
def test_an_emptied_region_clears_its_slot_bit(rt, cuda, old64):
    """the 16^3 at (16, 16, 16), which holds the uniform brick with a hole, emptied by two boxes meeting at x = 25"""
    assert old64[16:32, 16:32, 16:32].any()
    t, comp = patched(rt, old64, [(full((16, 16, 9), 0), (16, 16, 16)), (full((16, 16, 7), 0), (25, 16, 16))])
    assert not comp[16:32, 16:32, 16:32].any()
    i, mask, kind, _ = record_at(t, 16, 16, 16, 1)
    assert kind == K_INTERIOR and mask == 0 and i > 0      # the uncollapsed form: a mask-0 interior under a set bit
    t.compact()
    assert record_at(t, 16, 16, 16, 1) is None
    mask, kind, _ = _kinds(t)
    assert not ((kind == K_INTERIOR) & (mask == 0)).any()
    equals_fresh(rt, cuda, t, comp, 0, "emptied 16^3")


def test_a_completed_region_becomes_one_solid_child(rt, cuda, old64):
    """the 16^3 at (32, 32, 32) filled with one material by two boxes meeting at y = 39"""
    t, comp = patched(rt, old64, [(full((16, 7, 16), 2), (32, 32, 32)), (full((16, 9, 16), 2), (32, 39, 32))])
    assert (comp[32:48, 32:48, 32:48] == 2).all()
    _, mask, kind, _ = record_at(t, 32, 32, 32, 1)
    assert kind == K_INTERIOR and mask != 0                # the uncollapsed form: an interior over one material
    t.compact()
    _, mask, kind, mat = record_at(t, 40, 47, 33, 1)
    assert kind & 3 == K_SOLID and mat == 2 and mask == 0xFFFFFFFFFFFFFFFF
    equals_fresh(rt, cuda, t, comp, 0, "completed 16^3")


@pytest.mark.parametrize("ident", [3, 0])
def test_the_extent_in_halves_becomes_a_lone_root(rt, cuda, old64, ident):
    """filled with one material / emptied, by two boxes meeting at x = 30"""
    t, comp = patched(rt, old64, [(full((64, 64, 30), ident), (0, 0, 0)), (full((64, 64, 34), ident), (30, 0, 0))])
    assert (comp == ident).all()
    assert t.info().n_nodes > 1 and record_at(t, 0, 0, 0, 0)[2] == K_INTERIOR and t.garbage()[0] > 0
    t.compact()
    nodes, mats = t.export()
    assert len(nodes) == 1 and len(mats) == 0
    if ident:
        assert record_at(t, 0, 0, 0, 0) == (0, 0xFFFFFFFFFFFFFFFF, K_SOLID, ident)
    else:
        assert record_at(t, 0, 0, 0, 0) == (0, 0, K_INTERIOR, 0)
    equals_fresh(rt, cuda, t, comp, 0, "extent of %d" % ident)


def test_a_brick_overwritten_to_one_material_drops_its_run(rt, cuda, old64):
    """the full two-material brick at (40, 24, 36): its material-4 half becomes material 1 (x 40..41) and empty (x 42..43)"""
    assert set(np.unique(old64[36:40, 24:28, 40:44])) == {1, 4}
    t, comp = patched(rt, old64, [(full((4, 2, 2), 1), (40, 24, 36)), (full((4, 2, 2), 0), (42, 24, 36))])
    brick = comp[36:40, 24:28, 40:44]
    assert set(np.unique(brick)) == {0, 1} and (brick == 1).sum() == 48
    fresh_mats = len(_tree(rt, 3, comp).export()[1])
    before = len(t.export()[1])
    assert before >= fresh_mats + 64 and t.garbage()[1] >= 64   # the superseded runs of the brick are still in the array
    t.compact()
    _, mask, kind, mat = record_at(t, 40, 24, 36, 2)
    assert kind == K_BRICK | K_UNIFORM and mat == 1 and bin(mask).count("1") == 48
    assert len(t.export()[1]) == fresh_mats
    equals_fresh(rt, cuda, t, comp, 0, "brick to one material")


def test_a_completed_uniform_brick_becomes_a_solid_child(rt, cuda, old64):
    """the material-3 brick at (20, 20, 20) with a hole at (23, 22, 21): a second hole beside it, then both filled"""
    assert (old64[20:24, 20:24, 20:24] == 3).sum() == 63 and old64[21, 22, 23] == 0
    t, comp = patched(rt, old64, [(full((1, 1, 2), 0), (22, 22, 21)), (full((1, 1, 2), 3), (22, 22, 21))])
    assert (comp[20:24, 20:24, 20:24] == 3).all()
    _, mask, kind, mat = record_at(t, 20, 20, 20, 2)
    assert kind == K_BRICK | K_UNIFORM and mask == 0xFFFFFFFFFFFFFFFF and mat == 3   # the uncollapsed form
    t.compact()
    _, mask, kind, mat = record_at(t, 20, 20, 20, 2)
    assert kind == K_SOLID and mat == 3
    equals_fresh(rt, cuda, t, comp, 0, "completed brick")


# ------------------------------------------------------------------------------------------ 4. world-built trees --
STOP = 4  # the stage after which the tree is compacted: a 16^3 of 64 SOLID siblings, a mask-0 interior chain, rewritten blocks


def test_a_world_built_tree_still_follows_its_world(rt, cuda, oracle_mod):
    s = es.EditScript(rt, oracle_mod, 3)
    t = s.w.build().upload(0)
    s.trees.append(t)
    org, dn = cam_at(rt, s, EDIT_CAMS["fractional"])
    after = 0
    for stage in s.stages():
        t.sync()
        if stage == STOP:
            assert t.garbage()[0] > 0
            assert record_at(t, 16, 0, 0, 1)[2] == K_INTERIOR   # stage 4's 64 SOLID siblings, not collapsed
            t.compact()
            _same_arrays(t.export(), s.w.build().export(), "world tree at stage %d" % stage)
            assert record_at(t, 16, 0, 0, 1)[2] == K_SOLID and t.garbage() == (0, 0)   # ... and collapsed
            _same_ceilings(t, s.w.build().upload(0), "world tree: ceilings")
        if stage >= STOP:
            label = "world tree, stage %d" % stage
            check_box(rt, s, t, rt.VIEW_SOLID, label)                                       # the oracle
            assert np.array_equal(t.get_blocks(s.box_points()), s.w.build().get_blocks(s.box_points())), label   # the world
            ref = s.T.cast_frame(org, dn, 64, 32, 300)
            assert ref["rc"] == 0
            for flags in (0, rt.CAST_NO_CEILINGS):
                compare(rt, t, t.cast_frame(org, dn, 64, 32, 300, flags=flags), ref, "%s flags %d" % (label, flags))
            after += stage > STOP
    assert after == es.N_STAGES[3] - STOP and t.guard_trips() == 0


def test_a_volume_patched_world_tree_stays_refused_by_update(rt, cuda):
    w = rt.World(3)
    pts = np.random.default_rng(71).integers(0, 64, (3000, 3))
    w.put_blocks(pts, np.zeros(len(pts), np.uint32), np.full(len(pts), int(vc.colour(3)), np.uint64))
    t = w.build().upload(0)
    before = t.read_volume((0, 0, 0), (64, 64, 64)).cpu().numpy().view(np.uint16)
    new = vc.random_volume((11, 10, 9), 0.5, 72, ids=(1,))
    t.patch_volume(new, (30, 29, 27))
    assert t.garbage()[0] > 0
    t.compact()
    equals_fresh(rt, cuda, t, _put(before, new, (30, 29, 27)), 0, "patched world tree", pal=t.palette())
    w.put_block(1, 1, 1, 0, int(vc.colour(3)))
    with pytest.raises(rt.SvoError, match=r"\(-4\).*svo_tree_patch_volume_gpu"):
        t.update(w, [(1, 1, 1)])


# ------------------------------------------------------------------------------------- 5. a terrain tree, 4 levels --
def test_terrain_tree_at_4_levels(rt, cuda):
    t = rt.Tree.terrain_gpu(4, 256, 256)
    pal, view, E = t.palette(), t.info().view, 256
    comp = t.read_volume((0, 0, 0), (E, E, E)).cpu().numpy().view(np.uint16).copy()
    new = vc.random_volume((40, 20, 40), 0.5, 81, ids=(1, 2, 3))
    at = (101, 9, 83)
    assert comp[at[2]:at[2] + 40, at[1]:at[1] + 20, at[0]:at[0] + 40].any()   # the box cuts the ground
    t.patch_volume(new, at)
    comp = _put(comp, new, at)
    assert t.garbage()[0] > 0
    t.compact()
    equals_fresh(rt, cuda, t, comp, view, "terrain", levels=4, pal=pal, shift=(30.0, 60.0, 30.0))


# -------------------------------------------------------------------------------------------- 6. bounded growth --
def test_growth_is_bounded(rt, cuda, old64):
    rng = np.random.default_rng(91)
    steps = [(vc.random_volume((16, 16, 16), 0.5, 100 + i), tuple(int(v) for v in 4 * rng.integers(0, 12, 3) + rng.integers(1, 4, 3)))
             for i in range(12)]
    assert all(o % 4 for _, at in steps for o in at)
    a, b = _tree(rt, 3, old64), _tree(rt, 3, old64)
    comp, compactions, last = old64, 0, None
    for vox, at in steps:
        a.patch_volume(vox, at)
        b.patch_volume(vox, at)
        comp = _put(comp, vox, at)
        if a.garbage()[0] * 2 > a.info().n_nodes:
            a.compact()
            compactions += 1
            last = comp
            fresh = _tree(rt, 3, comp).info()
            assert (a.info().n_nodes, a.info().device_bytes) == (fresh.n_nodes, fresh.device_bytes)
    assert compactions >= 1
    got = a.read_volume((0, 0, 0), (64, 64, 64)).cpu().numpy().view(np.uint16)
    assert np.array_equal(got, vc.in_view(comp, PAL, 0))
    assert b.info().n_nodes > a.info().n_nodes             # without compaction: strictly more
    a.compact()
    equals_fresh(rt, cuda, a, comp, 0, "after 12 patches")
    assert last is not None


# ------------------------------------------------------------------------------------------------- 7. large ids --
def test_large_ids(rt, cuda):
    """a brick and a 16^3 of id 65534, one below the class words' MIXED marker, completed in halves"""
    top = pc.HIGH[2]
    assert top == 65534 == pc.CAP
    vol, _, has_big = pc.planted(64, 64, 64, (0, 0, 0), 7, "HIGH")
    assert has_big
    steps = [(full((16, 7, 16), top), (32, 32, 32)), (full((16, 9, 16), top), (32, 39, 32)),
             (full((4, 4, 1), top), (52, 4, 4)), (full((4, 4, 3), top), (53, 4, 4))]
    t, comp = patched(rt, vol, steps, pal=PALW)
    assert (comp[32:48, 32:48, 32:48] == top).all() and (comp[4:8, 4:8, 52:56] == top).all()
    assert record_at(t, 32, 32, 32, 1)[2] == K_INTERIOR and record_at(t, 52, 4, 4, 2)[2] == K_BRICK | K_UNIFORM
    t.compact()
    assert record_at(t, 32, 32, 32, 1)[2:] == (K_SOLID, top)
    assert record_at(t, 52, 4, 4, 2)[2:] == (K_SOLID, top)
    equals_fresh(rt, cuda, t, comp, 0, "ids up to 65534", pal=PALW)


# -------------------------------------------------------------------------------------------------- 8. refusals --
def test_refusals_change_nothing(rt, cuda):
    w = rt.World(3)
    pts = np.random.default_rng(71).integers(0, 64, (3000, 3))
    w.put_blocks(pts, np.zeros(len(pts), np.uint32), np.full(len(pts), int(vc.colour(3)), np.uint64))
    t = w.build().upload(0)
    w.put_block(5, 6, 7, 0, int(vc.colour(4)))
    t.update(w, [(5, 6, 7)])
    before, g = t.export(), t.garbage()
    assert g[0] > 0
    with pytest.raises(rt.SvoError, match=r"\(-4\).*svo_tree_compact_gpu.*not yet synced"):
        t.compact()
    _same_arrays(t.export(), before, "refused")
    assert t.garbage() == g
    t.sync().compact()
    _same_arrays(t.export(), w.build().export(), "synced, then compacted")
    assert t.garbage() == (0, 0)
    _same_ceilings(t, w.build().upload(0), "synced, then compacted: ceilings")


# ---------------------------------------------------------------------------------------- 9. save after compaction --
def test_save_after_compaction(rt, cuda, old64, tmp_path):
    t, comp, _, _ = _case1(rt, old64, sorted(BOXES)[0], 0)
    grown, small, ref = str(tmp_path / "grown.svo"), str(tmp_path / "compact.svo"), str(tmp_path / "fresh.svo")
    t.save(grown)
    t.compact().save(small)
    _tree(rt, 3, comp).save(ref)
    back = rt.Tree.load(small)
    _same_arrays(back.export(), t.export(), "loaded")
    assert os.path.getsize(small) == os.path.getsize(ref) < os.path.getsize(grown)


# -------------------------------------------------------------------------------------------- 10. shading scene --
def test_shaded_frame_with_a_compacted_scene(rt, cuda, old64):
    which = sorted(BOXES)[0]
    t0, comp, _, _ = _case1(rt, old64, which, 0)
    t1 = _case1(rt, old64, which, 1)[0]
    assert t1.garbage()[0] > 0
    t1.compact()
    f1 = _tree(rt, 3, comp, 1)
    cam = rt.normalize((0.6, -0.45, 0.66))
    (ca, ha), (cb, hb) = (t0.shade_frame((1.0, 40.0, 3.0), cam, 64, 32, 300, scene=s, time=0.25, with_hits=True) for s in (t1, f1))
    assert cuda.equal(ca, cb)
    for k in ("pos_steps", "t", "info"):
        assert cuda.equal(ha[k], hb[k]), k
    assert t0.guard_trips() == 0 and t1.guard_trips() == 0
