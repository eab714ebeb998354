"""svo_build_points_gpu on the GPU: a tree built from a sparse list of voxels in HBM is, byte for byte, the canonical
linearisation svo_build_view emits for a host world holding what the list leaves (tests/points_cases.py: the numpy
last-wins model, its survivors put into an rt.World, the ids remapped to its palette) and what svo_build_volume_gpu
emits for a dense volume of it; lists are applied in order; 7-level worlds, where no dense route exists, build from a
few tens of thousands of points; bad points are found on the device; the result is an ordinary resident tree."""
import numpy as np
import pytest

import points_cases as pc
import volume_cases as vc
from test_gpu_parity import compare
from test_gpu_volume_build import _same, _same_ceilings

pytestmark = pytest.mark.gpu

EMPTY = (0, 0xFFFFFFFFFFFFFFFF, 0.0)
K_INTERIOR, K_BRICK, K_SOLID, K_UNIFORM = 0, 1, 2, 4


@pytest.fixture(scope="module")
def cuda():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


def _records(t):
    """(mask, kind, uniform bit, material) per node record of the host image"""
    n, _ = t.export()
    info = n[:, 1] >> np.uint64(32)
    return n[:, 0], (info & np.uint64(3)).astype(int), (info & np.uint64(4)).astype(int), (info >> np.uint64(16)).astype(int)


def _record_at(t, x, y, z):
    i = int(t.node_indices([(x, y, z)])[0])
    mask, kind, uni, mat = _records(t)
    return int(mask[i]), int(kind[i]), int(uni[i]), int(mat[i])


def _pair(rt, levels, xyz, ids, view):
    """(points-built tree, host-built twin, palette, the list's ids in that palette)"""
    h, pal, pid = pc.host_twin(rt, levels, xyz, ids, view)
    g = rt.Tree.points_gpu(levels, xyz, pid, pal, view=view)
    return g, h, pal, pid


def _check_equal(rt, levels, xyz, ids, view, label):
    g, h, pal, pid = _pair(rt, levels, xyz, ids, view)
    _same(g, h, label)
    assert g.info().device == 0
    h.upload(0)
    _same_ceilings(g, h, label)
    return g, h, pal, pid


def _brick(x0, y0, z0, ident, s=4):
    """the s^3 points of the aligned cube at (x0, y0, z0), one id, x fastest"""
    z, y, x = np.meshgrid(np.arange(s), np.arange(s), np.arange(s), indexing="ij")
    xyz = np.stack([x.ravel() + x0, y.ravel() + y0, z.ravel() + z0], 1).astype(np.int32)
    return xyz, np.full(len(xyz), ident, np.uint16)


def _shuffled(lst, seed):
    order = np.random.default_rng(seed).permutation(len(lst[1]))
    return np.ascontiguousarray(lst[0][order]), np.ascontiguousarray(lst[1][order])


# ------------------------------------------------------------------------------------- 1. levels 2, both views --
def _random16():
    return pc.as_points(vc.random_volume((16, 16, 16), 0.3, 1), (0, 0, 0), 11)


SMALL = {
    "empty": pc.empty_list,
    "one point": lambda: (np.array([[5, 9, 14]], np.int32), np.array([3], np.uint16)),
    "full brick": lambda: _shuffled(_brick(8, 4, 12, 2), 12),
    "brick less one": lambda: tuple(a[:63] for a in _shuffled(_brick(8, 4, 12, 2), 13)),
    "one material": lambda: _shuffled(_brick(0, 0, 0, 2, 16), 14),
    "all liquid": lambda: _shuffled(_brick(0, 0, 0, 5, 16), 15),
    "random": _random16,
    "63 points": lambda: tuple(a[:63] for a in _random16()),
    "64 points": lambda: tuple(a[:64] for a in _random16()),
    "65 points": lambda: tuple(a[:65] for a in _random16()),
    "257 points": lambda: tuple(a[:257] for a in _random16()),
}


@pytest.mark.parametrize("view", [0, 1])
@pytest.mark.parametrize("case", sorted(SMALL))
def test_levels2_equals_host(rt, cuda, case, view):
    xyz, ids = SMALL[case]()
    g, h, pal, pid = _check_equal(rt, 2, xyz, ids, view, "L2 %s view %d" % (case, view))
    mask, kind, uni, mat = _records(g)
    i = g.info()
    if case == "empty" or (case == "all liquid" and view == 0):
        assert len(mask) == 1 and mask[0] == 0 and kind[0] == K_INTERIOR and i.n_bricks == 0   # the lone record {0, 0, K_INTERIOR}
    elif case in ("one material", "all liquid"):
        assert len(mask) == 1 and kind[0] == K_SOLID and mat[0] == int(pid[0])                 # a lone K_SOLID root
    elif case == "full brick":
        assert len(mask) == 2 and kind[1] == K_SOLID and mat[1] == int(pid[0]) and i.n_bricks == 0
    elif case == "brick less one":
        assert len(mask) == 2 and kind[1] == K_BRICK and uni[1] == K_UNIFORM and bin(int(mask[1])).count("1") == 63
        assert i.n_mat_bytes == 0
    elif case == "one point":
        assert len(mask) == 2 and kind[1] == K_BRICK and bin(int(mask[1])).count("1") == 1
    else:
        assert i.n_bricks > 1 and i.n_mat_bytes > 0
    if len(ids):
        got = g.get_blocks_gpu(xyz).cpu().numpy().view(np.uint16)
        assert np.array_equal(got, g.get_blocks(xyz))


def test_numpy_and_tensor_arguments_build_the_same_tree(rt, cuda):
    xyz, ids = _random16()
    h, pal, pid = pc.host_twin(rt, 2, xyz, ids, 1)
    a = rt.Tree.points_gpu(2, xyz, pid, pal, view=1)
    b = rt.Tree.points_gpu(2, cuda.from_numpy(xyz).cuda(), cuda.from_numpy(pid.view(np.int16)).cuda(), pal, view=1)
    _same(a, b, "numpy vs tensors")
    _same(b, h, "tensors vs host")


# ------------------------------------------------------------------------------------ 2. order and duplicates --
def test_order_of_distinct_points_does_not_matter(rt, cuda):
    xyz, ids = _random16()
    h, pal, pid = pc.host_twin(rt, 2, xyz, ids, 0)
    a = rt.Tree.points_gpu(2, xyz, pid, pal)
    order = np.random.default_rng(21).permutation(len(pid))
    b = rt.Tree.points_gpu(2, np.ascontiguousarray(xyz[order]), np.ascontiguousarray(pid[order]), pal)
    c = rt.Tree.points_gpu(2, np.ascontiguousarray(xyz[::-1]), np.ascontiguousarray(pid[::-1]), pal)
    _same(a, b, "shuffled")
    _same(a, c, "reversed")
    _same(a, h, "host")


def _background():
    """a sparse random list that keeps clear of the brick column x = 8..11, y = 4..7 the cases below write to"""
    vol = vc.random_volume((16, 16, 16), 0.2, 5)
    vol[:, 4:8, 8:12] = 0
    return pc.as_points(vol, (0, 0, 0), 22)


P = (9, 5, 2)  # a voxel of the brick (8, 4, 0)


def _one(p, ident):
    return np.array([p], np.int32), np.array([ident], np.uint16)


DUPLICATES = {
    # name: (the list, the voxel to look at, the source id it stores per view (solid, all))
    "three ids, last wins": (lambda: pc.concat(_one(P, 1), _background(), _one(P, 2), _one(P, 3)), P, (3, 3)),
    "three in a row": (lambda: pc.concat(_background(), _one(P, 4), _one(P, 1), _one(P, 2)), P, (2, 2)),
    "a later 0 erases": (lambda: pc.concat(_one(P, 1), _background(), _one(P, 0)), P, (0, 0)),
    "0 then an id": (lambda: pc.concat(_one(P, 0), _background(), _one(P, 4)), P, (4, 4)),
    "liquid over solid": (lambda: pc.concat(_one(P, 2), _background(), _one(P, 5)), P, (0, 5)),
    "solid over liquid": (lambda: pc.concat(_one(P, 5), _background(), _one(P, 2)), P, (2, 2)),
    "brick listed twice": (lambda: pc.concat(_brick(8, 4, 0, 3), _background(), _shuffled(_brick(8, 4, 0, 3), 23)), P, (3, 3)),
    "brick overwritten": (lambda: pc.concat(_brick(8, 4, 0, 1), _background(), _brick(8, 4, 0, 4)), P, (4, 4)),
    "full brick, one voxel ends 0": (lambda: pc.concat(_brick(8, 4, 0, 3), _background(), _one(P, 0)), (8, 4, 0), (3, 3)),
    "full brick, one voxel ends liquid": (lambda: pc.concat(_brick(8, 4, 0, 3), _one(P, 5), _background()), (8, 4, 0), (3, 3)),
}


@pytest.mark.parametrize("view", [0, 1])
@pytest.mark.parametrize("case", sorted(DUPLICATES))
def test_duplicates_resolve_in_list_order(rt, cuda, case, view):
    make, at, want = DUPLICATES[case]
    xyz, ids = make()
    sx, si = pc.last_wins(xyz, ids)
    assert len(si) < len(ids)  # the list does hold duplicates or erasures
    g, h, pal, pid = _check_equal(rt, 2, xyz, ids, view, "%s view %d" % (case, view))
    # what the voxel stores, as a source id: through the palette's (flags, colour)
    block, mat = g.get_block(*at)
    src = {(1 | f, c): i for i, (f, c) in enumerate(vc.TABLE) if i}
    assert (src[(pal[mat][0], pal[mat][1])] if mat else 0) == want[view], case
    assert int(g.get_blocks_gpu(np.array([at], np.int32)).cpu().numpy().view(np.uint16)[0]) == mat
    mask, kind, uni, m = _record_at(g, *at)
    if case in ("brick listed twice", "brick overwritten"):
        assert kind == K_SOLID and m == mat                                    # 128 points, still one K_SOLID child
    elif case == "full brick, one voxel ends 0" or (case == "full brick, one voxel ends liquid" and view == 0):
        assert kind == K_BRICK and uni == K_UNIFORM and bin(mask).count("1") == 63
    elif case == "full brick, one voxel ends liquid":
        assert kind == K_BRICK and uni == 0 and bin(mask).count("1") == 64      # two materials: a run of 64 entries


def test_liquid_over_solid_differs_between_the_views(rt, cuda):
    xyz, ids = DUPLICATES["liquid over solid"][0]()
    a, b = (_pair(rt, 2, xyz, ids, view)[0] for view in (0, 1))
    assert a.get_block(*P)[1] == 0 and b.get_block(*P)[1] != 0
    assert b.get_block(*P)[0][0] & 0x10  # LIQUID


# ------------------------------------------------------------------------------------------------ 3. levels 3 --
@pytest.fixture(scope="module")
def planted38():
    vol, has_big = vc.planted(37, 38, 41, (5, 2, 7), 4)
    assert has_big
    return vol


@pytest.mark.parametrize("view", [0, 1])
def test_levels3_equals_host_and_volume_builder(rt, cuda, planted38, view):
    xyz, ids = pc.as_points(planted38, (5, 2, 7), 31)
    g, h, pal, pid = _check_equal(rt, 3, xyz, ids, view, "L3 view %d" % view)
    vol = np.zeros_like(planted38)
    vol[xyz[:, 2] - 7, xyz[:, 1] - 2, xyz[:, 0] - 5] = pid
    v = rt.Tree.volume_gpu(3, vol, pal, origin=(5, 2, 7), view=view)
    _same(g, v, "L3 view %d vs volume_gpu" % view)
    _same_ceilings(g, v, "L3 view %d vs volume_gpu" % view)
    assert g.info().n_bricks > 0 and g.info().n_mat_bytes > 0
    assert _record_at(g, 16, 16, 16)[1] == K_SOLID   # the aligned 16^3 of one material: SOLID at depth 1


# ------------------------------------------------------------------------------------------------ 4. levels 4 --
def test_levels4_cavern_equals_volume_builder_and_casts_alike(rt, cuda):
    """the only million-point case: one view, one build"""
    vol, _ = vc.mini_cavern()
    pal = [EMPTY] + [(1 | f, c, 0.0) for f, c in vc.TABLE[1:]]
    xyz, ids = pc.as_points(vol, (0, 0, 0), 41)
    assert len(ids) > 1000000
    g = rt.Tree.points_gpu(4, cuda.from_numpy(xyz).cuda(), cuda.from_numpy(ids.view(np.int16)).cuda(), pal)
    v = rt.Tree.volume_gpu(4, vol, pal)
    _same(g, v, "L4 cavern")
    _same_ceilings(g, v, "L4 cavern")
    npl = list(g.info().nodes_per_level)
    assert npl[0] == 1 and npl[1] > 0 and npl[2] > 0 and npl[3] > 0
    cam = rt.normalize((0.6, -0.45, 0.66))
    g.guard_trips(reset=True)
    a = g.cast_frame((101.0, 50.0, 123.0), cam, 64, 32, 400)
    b = v.cast_frame((101.0, 50.0, 123.0), cam, 64, 32, 400)
    for k in ("pos_steps", "t", "info"):
        assert cuda.equal(a[k], b[k]), k
    d = rt.decode_hits(b)
    pf, pcol = np.array([p[0] for p in pal], np.uint32), np.array([p[1] for p in pal], np.uint64)
    mid = np.where(d["hit"], d["material"], 0)
    ref = dict(hit=d["hit"].astype(np.int32), pos=d["pos"], steps=d["steps"], last=d["last_pos"], flags=pf[mid], color=pcol[mid], t=d["t"])
    compare(rt, g, a, ref, "L4 cavern cast")
    assert int(d["hit"].sum()) > 0 and g.guard_trips() == 0


# ------------------------------------------------------------------------------------------------ 5. levels 7 --
E7 = 4 ** 7
BRICK7, CUBE7 = (9000, 12000, 16380), (8272, 16368, 10000)   # an aligned 4^3 and an aligned 16^3, coordinates >= 8192
TWINS7 = ((100, 200, 300), (100 + 8192, 200, 300))            # differ only in the top bit of x


def _scatter7():
    rng = np.random.default_rng(71)
    n = 30000
    xyz = rng.integers(0, E7, (n, 3)).astype(np.int32)
    ids = rng.integers(1, 6, n).astype(np.uint16)
    assert (xyz.max(0) >= E7 - 8).all() and (xyz.min(0) < 8).all()   # all 14 bits in use
    corners = (np.array([(0, 0, 0), (E7 - 1, E7 - 1, E7 - 1)], np.int32), np.array([1, 2], np.uint16))
    twins = (np.array(TWINS7, np.int32), np.array([3, 4], np.uint16))
    # the planted structures last: they win over any scattered point that fell into them
    return pc.concat((xyz, ids), corners, _brick(*BRICK7, 2), _brick(*CUBE7, 4, 16), twins)


def test_levels7_equals_host_and_looks_up_on_the_device(rt, cuda):
    xyz, ids = _scatter7()
    g, h, pal, pid = _check_equal(rt, 7, xyz, ids, 0, "L7 scatter")
    i = g.info()
    npl = list(i.nodes_per_level)
    assert i.levels == 7 and all(n > 0 for n in npl[:7]) and i.n_bricks > 20000
    assert _record_at(g, *BRICK7)[1] == K_SOLID and _record_at(g, *CUBE7)[1] == K_SOLID
    assert g.node_indices([BRICK7])[0] != g.node_indices([CUBE7])[0]
    cube_record = int(g.node_indices([CUBE7])[0])
    assert int(g.node_indices([tuple(c + 15 for c in CUBE7)])[0]) == cube_record   # one record for the whole 16^3
    a, b = (g.get_block(*p)[1] for p in TWINS7)
    assert a and b and a != b
    assert g.get_block(0, 0, 0)[1] and g.get_block(E7 - 1, E7 - 1, E7 - 1)[1]
    # lookups: every point, the six neighbours of a sample (those of the corners wrap), seeded random positions
    rng = np.random.default_rng(72)
    sample = np.concatenate([xyz[rng.integers(0, len(xyz), 2000)], xyz[30000:30002]])
    steps = np.array([(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)], np.int32)
    near = (sample[:, None, :] + steps[None, :, :]).reshape(-1, 3)
    anywhere = rng.integers(0, E7, (20000, 3)).astype(np.int32)
    where = np.ascontiguousarray(np.concatenate([xyz, near, anywhere]).astype(np.int32))
    got = g.get_blocks_gpu(where).cpu().numpy().view(np.uint16)
    want = g.get_blocks(where)
    assert np.array_equal(got, want)
    # the survivors read back their own ids (the solid view drops the liquid ones)
    sx, si = pc.last_wins(xyz, pid)
    keep = np.array([not (p[0] & 0x10) for p in pal])
    assert np.array_equal(g.get_blocks_gpu(sx).cpu().numpy().view(np.uint16), np.where(keep[si], si, 0))
    assert (want[len(xyz):] != 0).any() and (want == 0).any()


def test_levels7_full_view(rt, cuda):
    xyz, ids = _scatter7()
    g, h, pal, pid = _check_equal(rt, 7, xyz, ids, 1, "L7 scatter, full view")
    sx, si = pc.last_wins(xyz, pid)
    assert np.array_equal(g.get_blocks_gpu(sx).cpu().numpy().view(np.uint16), si)


# ------------------------------------------------------------------------------------ 6. errors on the device --
BAD = {
    "an id equal to n_palette": (lambda xyz, pid, n_pal: (xyz, np.concatenate([pid[:100], [n_pal], pid[101:]]).astype(np.uint16)), "n_palette"),
    "a coordinate equal to the extent": (lambda xyz, pid, n_pal: (np.concatenate([xyz[:70], [[3, 64, 5]], xyz[71:]]).astype(np.int32), pid),
                                         "coordinate"),
    "a coordinate of -1": (lambda xyz, pid, n_pal: (np.concatenate([xyz[:333], [[7, 9, -1]], xyz[334:]]).astype(np.int32), pid), "coordinate"),
}


@pytest.mark.parametrize("case", sorted(BAD))
def test_bad_points_are_reported_and_nothing_is_built(rt, cuda, planted38, case):
    xyz, ids = pc.as_points(planted38, (5, 2, 7), 61)
    h, pal, pid = pc.host_twin(rt, 3, xyz, ids, 0)
    spoil, names = BAD[case]
    bx, bi = spoil(xyz, pid, len(pal))
    assert len(bi) == len(pid) and len(bx) == len(xyz)
    with pytest.raises(rt.SvoError, match=r"svo_build_points_gpu failed \(-5\).*" + names) as e:
        rt.Tree.points_gpu(3, np.ascontiguousarray(bx), np.ascontiguousarray(bi), pal)
    other = "coordinate" if names == "n_palette" else "n_palette"
    assert other not in str(e.value)
    g = rt.Tree.points_gpu(3, xyz, pid, pal)  # a good build right after
    _same(g, h, "after " + case)


# ---------------------------------------------------------------------------- 7. an ordinary resident tree --
def test_patch_then_compact_equals_the_volume_builder(rt, cuda, planted38):
    xyz, ids = pc.as_points(planted38, (5, 2, 7), 71)
    g, h, pal, pid = _pair(rt, 3, xyz, ids, 0)
    comp = pc.dense(3, xyz, pid)
    box = vc.random_volume((9, 11, 13), 0.5, 73, ids=tuple(range(1, len(pal))))
    at = (14, 15, 30)
    g.patch_volume(box, at)
    comp[at[2]:at[2] + 9, at[1]:at[1] + 11, at[0]:at[0] + 13] = box
    assert g.garbage() != (0, 0)
    g.compact()
    fresh = rt.Tree.volume_gpu(3, comp, pal)
    _same(g, fresh, "patched and compacted")
    _same_ceilings(g, fresh, "patched and compacted")
    assert g.garbage() == (0, 0)
    where = np.random.default_rng(74).integers(-64, 128, (5000, 3)).astype(np.int32)
    assert np.array_equal(g.get_blocks_gpu(where).cpu().numpy().view(np.uint16), fresh.get_blocks(where))


def test_compact_of_a_fresh_points_tree_changes_nothing(rt, cuda, planted38):
    xyz, ids = pc.as_points(planted38, (5, 2, 7), 75)
    g, h, pal, pid = _pair(rt, 3, xyz, ids, 1)
    g.compact()
    _same(g, h, "compacted")


def test_update_refuses_a_points_built_tree(rt, cuda):
    xyz, ids = _random16()
    g, h, pal, pid = _pair(rt, 2, xyz, ids, 0)
    w = rt.World(2)
    w.put_block(1, 1, 1, 0, int(vc.colour(3)))
    with pytest.raises(rt.SvoError, match=r"svo_tree_update failed \(-4\)"):
        g.update(w, [(1, 1, 1)])
    g.patch_volume(np.array([[[1]]], np.uint16), (2, 2, 2))
    with pytest.raises(rt.SvoError, match=r"svo_tree_update failed \(-4\)"):
        g.update(w, [(1, 1, 1)])
    _same(rt.Tree.points_gpu(2, xyz, pid, pal), h, "untouched by the refused updates")
