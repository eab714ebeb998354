"""svo_tree_patch_volume_gpu on the GPU: a resident tree patched from a dense box of voxels holds the composite — the box
inside, the old content outside — and reads back, answers host lookups, carries ceilings and casts exactly like a tree
built afresh from that composite (Tree.volume_gpu).  The reference for content is numpy:
comp = old.copy(); comp[box] = new, then the view filter (volume_cases.in_view).

Checks, by the letters used below: (a) read_volume of the whole extent equals comp; (b) svo_tree_get_blocks on the host
image equals comp at every voxel of the box's 16-aligned hull and at 4,096 seeded positions elsewhere; (c) the ceilings,
pairs and quads in HBM equal the fresh tree's; (d) frames from test_gpu_degenerate_trees.CAMS equal the fresh tree's in
every field of the hit record; (e) no K_BRICK record of the exported node array has mask 0; (f) no guard trips.

The old world of most cases is volume_cases.planted(64, 64, 64, (0, 0, 0), seed).  At that origin its aligned 16^3 of
one material lands on top of its three planted bricks, so the one-voxel-missing uniform brick and the full two-material
brick the boxes must cut are planted again here, at (20, 20, 20) and (40, 24, 36)."""
import numpy as np
import pytest

import volume_cases as vc
from test_gpu_degenerate_trees import CAMS
from test_gpu_parity import _explicit, compare
from test_gpu_volume_build import _same_ceilings

pytestmark = pytest.mark.gpu

EMPTY = (0, 0xFFFFFFFFFFFFFFFF, 0.0)
PAL = [EMPTY] + [(1 | f, c, 0.0) for f, c in vc.TABLE[1:]]  # ids = volume_cases' source ids (5: liquid), stored flags
K_INTERIOR, K_BRICK, K_SOLID = 0, 1, 2


@pytest.fixture(scope="module")
def cuda(rt):
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    assert hasattr(rt.lib(), "svo_tree_patch_volume_gpu")
    return torch


@pytest.fixture(scope="module")
def old64():
    vol, has_big = vc.planted(64, 64, 64, (0, 0, 0), 7)
    assert has_big
    vol[20:24, 20:24, 20:24] = 3            # BRICK | UNIFORM: one voxel missing
    vol[21, 22, 23] = 0
    vol[36:40, 24:28, 40:44] = 1            # a full brick of two materials
    vol[36:40, 24:26, 40:44] = 4
    vol.setflags(write=False)
    return vol


def _tree(rt, levels, vol, view=0, pal=PAL):
    return rt.Tree.volume_gpu(levels, np.array(vol, np.uint16), pal, view=view)


def _put(comp, new, origin):
    x, y, z = origin
    nz, ny, nx = new.shape
    comp = comp.copy()
    comp[z:z + nz, y:y + ny, x:x + nx] = new
    return comp


def _kinds(tree):
    n, _ = tree.export()
    return n[:, 0], (n[:, 1] >> np.uint64(32)) & np.uint64(3), n[:, 1] >> np.uint64(48)


def check_content(t, comp, view, origin, shape, seed=1, pal=PAL):
    """(a), (b), (e); pal: the tree's palette"""
    E = comp.shape[0]
    want = vc.in_view(comp, pal, view)
    got = t.read_volume((0, 0, 0), (E, E, E)).cpu().numpy().view(np.uint16)
    assert np.array_equal(got, want), "(a) %d voxels differ" % int((got != want).sum())
    lo = [(o // 16) * 16 for o in origin]
    hi = [min(E, -(-(o + n) // 16) * 16) for o, n in zip(origin, shape[::-1])]
    zz, yy, xx = np.meshgrid(np.arange(lo[2], hi[2]), np.arange(lo[1], hi[1]), np.arange(lo[0], hi[0]), indexing="ij")
    pts = np.stack([xx.ravel(), yy.ravel(), zz.ravel()], 1)
    pts = np.concatenate([pts, np.random.default_rng(seed).integers(0, E, (4096, 3))]).astype(np.int32)
    ids = t.get_blocks(pts)
    assert np.array_equal(ids, want[pts[:, 2], pts[:, 1], pts[:, 0]]), "(b)"
    mask, kind, _ = _kinds(t)
    assert not ((kind == K_BRICK) & (mask == 0)).any(), "(e) a K_BRICK record with mask 0"


def check_casts(rt, cuda, t, fresh, label, shift=(0.0, 0.0, 0.0), ao=False):
    """(d), (f)"""
    t.guard_trips(reset=True)
    hits = 0
    for ci, (org, d) in enumerate(CAMS):
        org = tuple(o + s for o, s in zip(org, shift))
        dn = rt.normalize(d)
        for flags in (0, rt.CAST_NO_CEILINGS):
            a = t.cast_frame(org, dn, 64, 32, 300, flags=flags, ao_samples=16 if ao else 0)
            b = fresh.cast_frame(org, dn, 64, 32, 300, flags=flags, ao_samples=16 if ao else 0)
            for k in ("pos_steps", "t", "info") + (("ao",) if ao else ()):
                assert cuda.equal(a[k], b[k]), "(d) %s cam%d flags=%d %s" % (label, ci, flags, k)
            hits += int((a["info"] < 0).sum())
    assert t.guard_trips() == 0, "(f)"
    return hits


def check_all(rt, cuda, t, comp, view, origin, shape, label, levels=3, casts=True, pal=PAL):
    check_content(t, comp, view, origin, shape, pal=pal)
    fresh = _tree(rt, levels, comp, view, pal)
    _same_ceilings(t, fresh, "(c) " + label)
    if casts and view == 0:
        check_casts(rt, cuda, t, fresh, label)
    elif casts:  # a full-view tree is walked as the scene of the shading pass: its primary, reflected and refracted rays
        solid = _tree(rt, levels, comp, 0, pal)
        for ci, (org, d) in enumerate(CAMS):
            dn = rt.normalize(d)
            (ca, ha), (cb, hb) = (solid.shade_frame(org, dn, 64, 32, 300, scene=s, time=0.25, with_hits=True) for s in (t, fresh))
            assert cuda.equal(ca, cb), "(d) %s cam%d colours" % (label, ci)
            for k in ("pos_steps", "t", "info"):
                assert cuda.equal(ha[k], hb[k]), "(d) %s cam%d %s" % (label, ci, k)
        assert t.guard_trips() == 0 and solid.guard_trips() == 0, "(f)"
    return fresh


# ------------------------------------------------------------------ 1. off-grid boxes over every kind of old content --
# 13 x 9 x 22 voxels; origins with residues mod 4 of (1, 2, 3), (3, 1, 2), (2, 3, 1)
BOXES = {
    "cuts the 16^3 SOLID": (9, 10, 3),              # x 9..21 over the planted (0..16)^3 and its neighbours
    "cuts the uniform brick with a hole": (23, 21, 18),
    "cuts the full two-material brick": (42, 23, 37),
}


def _case1(rt, old64, which, view):
    origin = BOXES[which]
    new = vc.random_volume((22, 9, 13), 0.5, 11 + sorted(BOXES).index(which))
    assert (new == 5).any()
    t = _tree(rt, 3, old64, view)
    t.patch_volume(new, origin)
    return t, _put(old64, new, origin), origin, new


@pytest.mark.parametrize("view", [0, 1])
@pytest.mark.parametrize("which", sorted(BOXES))
def test_off_grid_boxes(rt, cuda, old64, which, view):
    assert [o % 4 for o in BOXES[which]] in ([1, 2, 3], [3, 1, 2], [2, 3, 1])
    if which == "cuts the 16^3 SOLID":
        assert (old64[0:16, 0:16, 0:16] == 4).all()
    elif which == "cuts the uniform brick with a hole":
        assert (old64[20:24, 20:24, 20:24] == 3).sum() == 63
    else:
        assert set(np.unique(old64[36:40, 24:28, 40:44])) == {1, 4}
    t, comp, origin, new = _case1(rt, old64, which, view)
    assert t.garbage()[0] > 0
    check_all(rt, cuda, t, comp, view, origin, new.shape, "%s view %d" % (which, view))
    if which == "cuts the 16^3 SOLID":  # the SOLID region expanded: a voxel of it outside the box lies in a SOLID child now
        mask, kind, mat = _kinds(t)
        ni, nj = (int(i) for i in t.node_indices([(1, 1, 1), (5, 1, 1)]))
        assert kind[ni] == K_SOLID and mat[ni] == 4 and kind[nj] == K_SOLID and ni != nj


# --------------------------------------------------------------------------------------------- 2. a one-voxel box --
def _slot_is_clear(t, x, y, z, levels=3):
    """a lookup of the voxel ends at an interior node whose slot for it is clear"""
    nodes = t.export()[0]
    n = 0
    for depth in range(levels):
        mask, ref, kind = int(nodes[n, 0]), int(nodes[n, 1]) & 0xFFFFFFFF, (int(nodes[n, 1]) >> 32) & 3
        if kind != K_INTERIOR:
            return False
        sh = 2 * (levels - 1 - depth)
        sl = (((z >> sh) & 3) << 4) | (((y >> sh) & 3) << 2) | ((x >> sh) & 3)
        if not (mask >> sl) & 1:
            return True
        n = ref + bin(mask & ((1 << sl) - 1)).count("1")
    return False


def test_one_voxel_box(rt, cuda):
    old = np.zeros((64, 64, 64), np.uint16)
    old[0:16, 0:12, 0:16] = vc.random_volume((16, 12, 16), 0.3, 5)
    old[35, 34, 33] = 1                     # the only voxel of its brick (and of its 16^3)
    old[40:48, 40:44, 40:48] = 2
    t = _tree(rt, 3, old)
    one = np.array([[[3]]], np.uint16)
    comp = old
    for step, (vox, at) in enumerate([(one, (50, 9, 21)), (one * 0, (50, 9, 21)), (one * 0, (33, 34, 35))]):
        t.patch_volume(vox, at)
        comp = _put(comp, vox, at)
        check_all(rt, cuda, t, comp, 0, at, (1, 1, 1), "one voxel, step %d" % step, casts=False)
        if step == 0:
            assert t.get_block(*at)[1] == 3
        else:
            assert _slot_is_clear(t, *at)   # the emptied brick left no record: its parent's mask bit is clear
    assert np.array_equal(comp, _put(old, one * 0, (33, 34, 35)))


# ------------------------------------------------------------------------------- 3. a box across the world centre --
@pytest.mark.parametrize("view", [0, 1])
def test_box_across_the_world_centre(rt, cuda, old64, view):
    new = vc.random_volume((9, 9, 9), 0.5, 21)
    t = _tree(rt, 3, old64, view)
    t.patch_volume(new, (28, 28, 28))       # 28..36 on every axis: all eight depth-1 children around (32, 32, 32)
    check_all(rt, cuda, t, _put(old64, new, (28, 28, 28)), view, (28, 28, 28), new.shape, "centre view %d" % view)


# -------------------------------------------------------------------------------------- 4. emptying and filling --
def test_emptying_a_populated_region(rt, cuda, old64):
    """an all-zero 20^3 box, off the grid: interiors with mask 0 may appear; casts and AO through them equal the fresh
    tree's"""
    assert old64[7:27, 6:26, 5:25].any()
    t = _tree(rt, 3, old64)
    zero = np.zeros((20, 20, 20), np.uint16)
    t.patch_volume(zero, (5, 6, 7))
    comp = _put(old64, zero, (5, 6, 7))
    fresh = check_all(rt, cuda, t, comp, 0, (5, 6, 7), zero.shape, "emptied")
    assert check_casts(rt, cuda, t, fresh, "emptied, AO", ao=True) > 0


def test_filling_aligned_regions(rt, cuda, old64):
    t = _tree(rt, 3, old64)
    a = np.full((16, 16, 16), 2, np.uint16)
    t.patch_volume(a, (32, 16, 48))         # an aligned 16^3: one K_SOLID child of the root
    comp = _put(old64, a, (32, 16, 48))
    mask, kind, mat = _kinds(t)
    ni = t.node_indices([(32, 16, 48), (47, 31, 63), (40, 20, 50)])
    assert len(set(ni.tolist())) == 1 and kind[ni[0]] == K_SOLID and mat[ni[0]] == 2
    b = np.full((4, 4, 4), 2, np.uint16)
    t.patch_volume(b, (20, 24, 28))         # an aligned 4^3: a K_SOLID child of a cut 16^3 parent
    comp = _put(comp, b, (20, 24, 28))
    mask, kind, mat = _kinds(t)
    ni = t.node_indices([(20, 24, 28), (23, 27, 31)])
    assert ni[0] == ni[1] and kind[ni[0]] == K_SOLID and mat[ni[0]] == 2
    check_all(rt, cuda, t, comp, 0, (20, 24, 28), b.shape, "filled")


# --------------------------------------------------------------------- 5. whole-extent boxes and degenerate roots --
def test_one_voxel_into_an_empty_tree(rt, cuda):
    old = np.zeros((64, 64, 64), np.uint16)
    t = _tree(rt, 3, old)
    assert len(t.export()[0]) == 1
    one = np.array([[[1]]], np.uint16)
    t.patch_volume(one, (37, 5, 20))
    check_all(rt, cuda, t, _put(old, one, (37, 5, 20)), 0, (37, 5, 20), (1, 1, 1), "empty root")
    assert t.info().n_nodes == 3            # the root, an interior, a brick, and no more


def test_hole_carved_into_an_all_solid_world(rt, cuda):
    old = np.full((64, 64, 64), 2, np.uint16)
    t = _tree(rt, 3, old)
    mask, kind, _ = _kinds(t)
    assert len(mask) == 1 and kind[0] == K_SOLID
    hole = np.zeros((5, 5, 5), np.uint16)
    t.patch_volume(hole, (13, 22, 31))      # the SOLID expands at every level
    comp = _put(old, hole, (13, 22, 31))
    fresh = check_all(rt, cuda, t, comp, 0, (13, 22, 31), hole.shape, "solid root")
    # rays started inside the hole
    dirs = np.array([(1, 0.2, 0.1), (-1, 0.3, 0.2), (0.1, 1, 0.3), (0.2, -1, 0.1), (0.3, 0.1, 1), (0.1, 0.2, -1)], np.float32)
    org = cuda.from_numpy(np.tile(np.array([[15.5, 24.5, 33.5]], np.float32), (6, 1))).cuda()
    gd = cuda.from_numpy(dirs).cuda()
    a, b = t.cast_rays(gd, org, steps=50), fresh.cast_rays(gd, org, steps=50)
    for k in ("pos_steps", "t", "info"):
        assert cuda.equal(a[k], b[k]), k
    assert int((a["info"] < 0).sum()) == 6


@pytest.mark.parametrize("content", ["empty", "uniform", "random"])
def test_whole_extent_box(rt, cuda, old64, content):
    new = {"empty": lambda: np.zeros((64, 64, 64), np.uint16), "uniform": lambda: np.full((64, 64, 64), 3, np.uint16),
           "random": lambda: vc.random_volume((64, 64, 64), 0.3, 31)}[content]()
    t = _tree(rt, 3, old64)
    t.patch_volume(new, (0, 0, 0))
    fresh = check_all(rt, cuda, t, new, 0, (0, 0, 0), new.shape, "whole extent, " + content)
    mask, kind, mat = _kinds(t)
    if content == "empty":
        assert len(mask) == 1 and mask[0] == 0 and kind[0] == K_INTERIOR
    elif content == "uniform":
        assert len(mask) == 1 and kind[0] == K_SOLID and mat[0] == 3
    else:  # a full build: the canonical arrays
        (na, ma), (nb, mb) = t.export(), fresh.export()
        assert np.array_equal(na, nb) and np.array_equal(ma, mb)
    assert t.garbage() == (0, 0)


# ------------------------------------------------------------------------------------------ 6. against the oracle --
def test_patched_tree_against_the_oracle(rt, cuda, oracle_mod, old64):
    which = sorted(BOXES)[0]
    t, comp, origin, new = _case1(rt, old64, which, 0)
    T = vc.oracle_twin(oracle_mod, 3, vc.voxel_puts(comp, (0, 0, 0)))
    t.guard_trips(reset=True)
    org, d = CAMS[0]
    dn = rt.normalize(d)
    ref = T.cast_frame(org, dn, 64, 32, 300)
    assert ref["rc"] == 0
    for flags in (0, rt.CAST_NO_CEILINGS, rt.CAST_ITERATIVE):
        compare(rt, t, t.cast_frame(org, dn, 64, 32, 300, flags=flags), ref, "patched vs oracle flags=%d" % flags)
    # explicit rays aimed into the box from outside and out of it from inside
    rng = np.random.default_rng(3)
    centre = np.array(origin, np.float32) + np.array(new.shape[::-1], np.float32) / 2
    o1 = rng.uniform(0, 64, (64, 3)).astype(np.float32)
    d1 = (centre - o1) + rng.normal(size=(64, 3)).astype(np.float32)
    o2 = np.tile(centre + 0.25, (64, 1)).astype(np.float32)
    d2 = rng.normal(size=(64, 3)).astype(np.float32)
    out, ref = _explicit(rt, cuda, t, T, np.concatenate([o1, o2]), np.concatenate([d1, d2]), 200)
    compare(rt, t, out, ref, "patched vs oracle, explicit rays")
    assert ref["hit"].any()
    assert t.guard_trips() == 0


def test_shaded_frame_with_patched_full_view_scene(rt, cuda, old64):
    which = sorted(BOXES)[0]
    t0, comp, _, _ = _case1(rt, old64, which, 0)
    t1 = _case1(rt, old64, which, 1)[0]
    f0, f1 = _tree(rt, 3, comp, 0), _tree(rt, 3, comp, 1)
    cam = rt.normalize((0.6, -0.45, 0.66))
    a = t0.shade_frame((1.0, 40.0, 3.0), cam, 128, 64, 300, scene=t1, time=0.25)
    b = f0.shade_frame((1.0, 40.0, 3.0), cam, 128, 64, 300, scene=f1, time=0.25)
    assert cuda.equal(a, b)
    assert t0.guard_trips() == 0 and t1.guard_trips() == 0


# ------------------------------------------------------------------------------------- 7. sequences and capacity --
def test_sequence_and_capacity(rt, cuda, tmp_path):
    E = 256
    t = _tree(rt, 4, np.zeros((E, E, E), np.uint16))
    comp = vc.random_volume((E, E, E), 0.3, 41, ids=(1, 2, 3, 4))
    bytes_seen = [t.info().device_bytes]
    garbage = [t.garbage()]
    steps = [(comp, (0, 0, 0))] + [(vc.random_volume((40, 40, 40), 0.5, 50 + i, ids=(1, 2, 3, 4)), o)
                                   for i, o in enumerate([(101, 57, 83), (121, 77, 99), (90, 70, 110)])]
    for i, (vox, at) in enumerate(steps):
        t.patch_volume(vox, at)
        if i:
            comp = _put(comp, vox, at)
        else:
            assert t.info().n_nodes > 65536 + 1     # more than the slack of the empty tree: the arrays were reallocated
        got = t.read_volume((0, 0, 0), (E, E, E))
        want = cuda.from_numpy(comp.view(np.int16)).cuda()
        assert cuda.equal(got, want), "(a) step %d" % i
        del got, want
        _same_ceilings(t, _tree(rt, 4, comp), "(c) step %d" % i)
        bytes_seen.append(t.info().device_bytes)
        garbage.append(t.garbage())
    assert all(b[0] >= a[0] and b[1] >= a[1] for a, b in zip(garbage, garbage[1:]))
    assert garbage[1] == (0, 0) and garbage[2][0] > 0 and garbage[2][1] > 0
    assert sum(b != a for a, b in zip(bytes_seen, bytes_seen[1:])) == 1 and bytes_seen[1] > bytes_seen[0]
    mask, kind, _ = _kinds(t)
    assert not ((kind == K_BRICK) & (mask == 0)).any()
    path = str(tmp_path / "patched.svo")
    t.save(path)
    u = rt.Tree.load(path).upload(0)
    assert cuda.equal(u.read_volume((0, 0, 0), (E, E, E)), cuda.from_numpy(comp.view(np.int16)).cuda())


# --------------------------------------------------------------------------------------- 8. errors on the device --
def test_an_id_equal_to_the_palette_size_changes_nothing(rt, cuda, old64):
    t = _tree(rt, 3, old64)
    t.patch_volume(vc.random_volume((9, 9, 9), 0.5, 61), (3, 2, 1))   # (a tree that already carries garbage)
    before = t.read_volume((0, 0, 0), (64, 64, 64)).clone()
    nodes, mats = t.export()
    g = t.garbage()
    bad = vc.random_volume((22, 9, 13), 0.5, 62)
    bad[21, 8, 12] = len(PAL)
    with pytest.raises(rt.SvoError, match=r"\(-5\).*palette"):
        t.patch_volume(bad, (9, 10, 3))
    assert cuda.equal(t.read_volume((0, 0, 0), (64, 64, 64)), before)
    n2, m2 = t.export()
    assert nodes.tobytes() == n2.tobytes() and mats.tobytes() == m2.tobytes()
    assert t.garbage() == g


def test_world_built_trees(rt, cuda):
    w = rt.World(3)
    rng = np.random.default_rng(71)
    pts = rng.integers(0, 64, (3000, 3))
    w.put_blocks(pts, np.zeros(len(pts), np.uint32), np.full(len(pts), int(vc.colour(3)), np.uint64))
    t = w.build().upload(0)
    assert t.info().n_materials == 2
    w.put_block(5, 6, 7, 0, int(vc.colour(3)))
    t.update(w, [(5, 6, 7)])
    one = np.array([[[1]]], np.uint16)
    with pytest.raises(rt.SvoError, match=r"\(-4\).*not yet synced"):
        t.patch_volume(one, (9, 9, 9))
    t.sync()
    before = t.read_volume((0, 0, 0), (64, 64, 64)).cpu().numpy().view(np.uint16)
    new = vc.random_volume((11, 10, 9), 0.5, 72, ids=(1,))
    t.patch_volume(new, (30, 29, 27))
    got = t.read_volume((0, 0, 0), (64, 64, 64)).cpu().numpy().view(np.uint16)
    assert np.array_equal(got, _put(before, new, (30, 29, 27)))
    w.put_block(1, 1, 1, 0, int(vc.colour(3)))
    with pytest.raises(rt.SvoError, match=r"\(-4\).*svo_tree_patch_volume_gpu"):
        t.update(w, [(1, 1, 1)])


# ------------------------------------------------------------------------------------------ 9. other tree sources --
def test_terrain_tree(rt, cuda):
    x, z = np.meshgrid(np.arange(120), np.arange(120), indexing="ij")
    heights = (24 + 10 * np.sin(x / 9.0) + 8 * np.cos(z / 7.0)).astype(np.int32)
    t = rt.Tree.heightfield_gpu(4, heights)
    pal, view, E = t.palette(), t.info().view, 256
    comp = t.read_volume((0, 0, 0), (E, E, E)).cpu().numpy().view(np.uint16).copy()
    solid = int(comp[comp != 0][0])
    block = np.full((10, 10, 10), solid, np.uint16)
    cave = np.zeros((11, 7, 9), np.uint16)
    assert not comp[41:51, 70:80, 33:43].any() and comp[50:61, 2:9, 50:59].any()
    for vox, at in ((block, (33, 70, 41)), (cave, (50, 2, 50))):   # floating above the surface; carved below it
        t.patch_volume(vox, at)
        comp = _put(comp, vox, at)
        lo = [(o // 16) * 16 for o in at]
        n = [-(-(o + s) // 16) * 16 - l for o, s, l in zip(at, vox.shape[::-1], lo)]
        got = t.read_volume(lo, n[::-1]).cpu().numpy().view(np.uint16)
        assert np.array_equal(got, comp[lo[2]:lo[2] + n[2], lo[1]:lo[1] + n[1], lo[0]:lo[0] + n[0]]), "(a)"
    fresh = rt.Tree.volume_gpu(4, comp, pal, view=view)
    assert np.array_equal(t.read_volume((0, 0, 0), (E, E, E)).cpu().numpy().view(np.uint16), comp)
    _same_ceilings(t, fresh, "(c) terrain")
    assert check_casts(rt, cuda, t, fresh, "terrain", shift=(30.0, 60.0, 30.0)) > 0
    mask, kind, _ = _kinds(t)
    assert not ((kind == K_BRICK) & (mask == 0)).any()
