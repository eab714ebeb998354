"""svo_build_volume_gpu / svo_tree_read_volume on the GPU: a tree built from a dense voxel volume in HBM is, byte for byte,
the canonical linearisation svo_build_view emits for a host world holding the same blocks (tests/volume_cases.py
host_twin: the world is filled voxel by voxel and the volume remapped to its palette, so both number the materials
alike); it casts, shades and reads back like it; volumes of more than 2^31 voxels are indexed correctly.

The issue's 3-level case, a 37 x 22 x 41 volume at (5, 2, 7), is 22 rows tall from row 2: it holds no aligned 16^3
region, so its two 16^3 structures cannot be planted in it.  It runs with every structure that fits, and a sibling of 37 x
38 x 41 at the same origin (rows 2..39 hold the aligned rows 16..31) carries all of them."""
import numpy as np
import pytest

import volume_cases as vc
from test_gpu_parity import compare
from test_gpu_degenerate_trees import CAMS

pytestmark = pytest.mark.gpu

EMPTY = (0, 0xFFFFFFFFFFFFFFFF, 0.0)


@pytest.fixture(scope="module")
def cuda():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


def _same(a, b, label):
    """tests/test_gpu_build.py _same restated, plus equal palettes"""
    na, ma = a.export()
    nb, mb = b.export()
    assert na.shape == nb.shape, "%s: %d vs %d nodes" % (label, len(na), len(nb))
    assert np.array_equal(na, nb), "%s: node arrays differ at %d records" % (label, int((na != nb).any(1).sum()))
    assert np.array_equal(ma, mb), label
    ia, ib = a.info(), b.info()
    assert list(ia.nodes_per_level) == list(ib.nodes_per_level) and ia.n_bricks == ib.n_bricks, label
    assert a.palette() == b.palette() and ia.view == ib.view and ia.levels == ib.levels, label


def _same_ceilings(g, h, label):
    lg, cg, pg = g.device_ceilings()
    lh, ch, ph = h.device_ceilings()
    assert lg == lh and np.array_equal(cg, ch) and np.array_equal(pg, ph), label
    assert np.array_equal(g.device_ceiling_quads(), h.device_ceiling_quads()), label


def _to_dev(torch, vol):
    return torch.from_numpy(np.ascontiguousarray(vol).view(np.int16)).cuda()


def _pair(rt, torch, levels, vol, origin, view):
    """(volume-built tree, uploaded host-built tree, palette, volume in palette ids)"""
    h, pal, ids = vc.host_twin(rt, levels, vol, origin, view)
    g = rt.Tree.volume_gpu(levels, _to_dev(torch, ids), pal, origin=origin, view=view)
    return g, h, pal, ids


def _check_equal(rt, torch, levels, vol, origin, view, label):
    g, h, pal, ids = _pair(rt, torch, levels, vol, origin, view)
    _same(g, h, label)
    assert g.info().device == 0
    h.upload(0)
    _same_ceilings(g, h, label)
    return g, h, pal, ids


# ------------------------------------------------------------------------------------- 1. byte equality, both views --
SMALL = {
    "random": lambda: vc.random_volume((16, 16, 16), 0.3, 1),
    "one material": lambda: np.full((16, 16, 16), 2, np.uint16),     # a SOLID root
    "zeros": lambda: np.zeros((16, 16, 16), np.uint16),              # an empty root
    "all liquid": lambda: np.full((16, 16, 16), 5, np.uint16),       # empty in the solid view, a SOLID root in the full view
}


@pytest.mark.parametrize("view", [0, 1])
@pytest.mark.parametrize("case", sorted(SMALL))
def test_levels2_equals_host(rt, cuda, case, view):
    g, h, pal, ids = _check_equal(rt, cuda, 2, SMALL[case](), (0, 0, 0), view, "L2 %s view %d" % (case, view))
    n, _ = g.export()
    if case == "zeros" or (case == "all liquid" and view == 0):
        assert len(n) == 1 and n[0, 0] == 0 and g.info().n_bricks == 0   # the lone record {0, 0, K_INTERIOR}
    elif case != "random":
        assert len(n) == 1 and ((int(n[0, 1]) >> 32) & 3) == 2            # a lone K_SOLID root


@pytest.fixture(scope="module")
def planted22():
    return vc.planted(37, 22, 41, (5, 2, 7), 3)[0]


@pytest.fixture(scope="module")
def planted38():
    vol, has_big = vc.planted(37, 38, 41, (5, 2, 7), 4)
    assert has_big
    return vol


@pytest.fixture(scope="module")
def cavern4():
    return vc.mini_cavern()


@pytest.mark.parametrize("view", [0, 1])
@pytest.mark.parametrize("which", ["planted22", "planted38"])
def test_levels3_equals_host(rt, cuda, request, which, view):
    vol = request.getfixturevalue(which)
    g, h, pal, ids = _check_equal(rt, cuda, 3, vol, (5, 2, 7), view, "L3 %s view %d" % (which, view))
    assert g.info().n_bricks > 0 and g.info().n_mat_bytes > 0


def test_levels3_views_differ_where_the_liquid_voxel_sits(rt, cuda, planted38):
    """the 16^3 full of one solid material except one liquid voxel collapses in neither view: a brick there in both, with
    one voxel fewer in the solid view's mask"""
    trees = [_pair(rt, cuda, 3, planted38, (5, 2, 7), view)[0] for view in (0, 1)]
    x, y, z = 16 + 2, 16 + 9, 32 + 5
    a, b = (t.get_block(x, y, z)[1] for t in trees)
    assert a == 0 and b != 0
    ia, ib = (t.node_indices([(x, y, z)])[0] for t in trees)
    na, nb = trees[0].export()[0][ia], trees[1].export()[0][ib]
    assert bin(int(na[0])).count("1") == 63 and bin(int(nb[0])).count("1") == 64


@pytest.mark.parametrize("view", [0, 1])
def test_levels4_cavern_equals_host(rt, cuda, cavern4, view):
    g, h, pal, ids = _check_equal(rt, cuda, 4, cavern4[0], (0, 0, 0), view, "L4 cavern view %d" % view)
    npl = list(g.info().nodes_per_level)
    assert npl[0] == 1 and npl[1] > 0 and npl[2] > 0 and npl[3] > 0


# ------------------------------------------------------------------------------------------------------- 2. casts --
def _cast_case(rt, cuda, oracle_mod, levels, vol, origin, puts, shift, label):
    g, h, pal, ids = _pair(rt, cuda, levels, vol, origin, 0)
    T = vc.oracle_twin(oracle_mod, levels, puts)
    g.guard_trips(reset=True)
    for ci, (org, d) in enumerate(CAMS):
        org = tuple(o + s for o, s in zip(org, shift))
        dn = rt.normalize(d)
        ref = T.cast_frame(org, dn, 64, 32, 300)
        assert ref["rc"] == 0
        for flags in (0, rt.CAST_NO_CEILINGS, rt.CAST_ITERATIVE):
            out = g.cast_frame(org, dn, 64, 32, 300, flags=flags)
            compare(rt, g, out, ref, "%s cam%d flags=%d" % (label, ci, flags))
    assert g.guard_trips() == 0


def test_casts_levels3_against_oracle(rt, cuda, oracle_mod, planted38):
    """the cameras of tests/test_gpu_degenerate_trees.py, as they are (inside the 64^3 world, next to the volume's low
    corner) — about 23 thousand voxel puts on the oracle side"""
    puts = vc.voxel_puts(planted38, (5, 2, 7))
    assert len(puts) < 40000
    _cast_case(rt, cuda, oracle_mod, 3, planted38, (5, 2, 7), puts, (0.0, 0.0, 0.0), "L3")


def test_casts_levels4_against_oracle(rt, cuda, oracle_mod, cavern4):
    """the same cameras moved above the cavern's floor, between the staircase, the floating block and the plate"""
    vol, puts = cavern4
    assert len(puts) < 40000
    _cast_case(rt, cuda, oracle_mod, 4, vol, (0, 0, 0), puts, (100.0, 36.0, 120.0), "L4")


def test_ao_frame_equals_host_tree(rt, cuda, cavern4):
    g, h, pal, ids = _pair(rt, cuda, 4, cavern4[0], (0, 0, 0), 0)
    h.upload(0)
    cam = rt.normalize((0.6, -0.45, 0.66))
    a = g.cast_frame((101.0, 50.0, 123.0), cam, 128, 64, 400, ao_samples=16)
    b = h.cast_frame((101.0, 50.0, 123.0), cam, 128, 64, 400, ao_samples=16)
    for k in ("pos_steps", "t", "info", "ao"):
        assert cuda.equal(a[k], b[k]), k
    assert int((a["info"] < 0).sum()) > 0 and int(a["ao"].sum()) > 0   # hits (bit 31), occluded samples
    assert g.guard_trips() == 0


def test_shaded_frame_with_full_view_scene_equals_host_trees(rt, cuda, cavern4):
    g0, h0, _, _ = _pair(rt, cuda, 4, cavern4[0], (0, 0, 0), 0)
    g1, h1, _, _ = _pair(rt, cuda, 4, cavern4[0], (0, 0, 0), 1)
    h0.upload(0)
    h1.upload(0)
    cam = rt.normalize((0.6, -0.45, 0.66))
    a = g0.shade_frame((101.0, 50.0, 123.0), cam, 128, 64, 400, scene=g1, time=0.25)
    b = h0.shade_frame((101.0, 50.0, 123.0), cam, 128, 64, 400, scene=h1, time=0.25)
    assert cuda.equal(a, b)
    assert g0.guard_trips() == 0 and g1.guard_trips() == 0


# --------------------------------------------------------------------------------------------------- 3. read-back --
@pytest.mark.parametrize("view", [0, 1])
def test_read_volume_over_the_source_box(rt, cuda, planted38, view):
    g, h, pal, ids = _pair(rt, cuda, 3, planted38, (5, 2, 7), view)
    got = g.read_volume((5, 2, 7), ids.shape).cpu().numpy().view(np.uint16)
    assert np.array_equal(got, vc.in_view(ids, pal, view))
    if view == 0:
        assert (got != ids).any()  # (the liquid voxels: the check above is not vacuous)
    else:
        assert np.array_equal(got, ids)


def test_read_volume_past_the_box_and_wrapping(rt, cuda, planted38):
    g, h, pal, ids = _pair(rt, cuda, 3, planted38, (5, 2, 7), 1)
    nz, ny, nx = ids.shape
    want = np.zeros((64, 64, 64), np.uint16)           # the whole world [z, y, x]
    want[7:7 + nz, 2:2 + ny, 5:5 + nx] = ids
    got = g.read_volume((0, 0, 0), (64, 64, 64)).cpu().numpy().view(np.uint16)
    assert np.array_equal(got, want)
    # a box that wraps the extent on every axis: origin (-9, 60, 40), 30 x 20 x 50 voxels
    ox, oy, oz, bx, by, bz = -9, 60, 40, 30, 20, 50
    got = g.read_volume((ox, oy, oz), (bz, by, bx)).cpu().numpy().view(np.uint16)
    zi, yi, xi = (np.arange(o, o + n) % 64 for o, n in ((oz, bz), (oy, by), (ox, bx)))
    assert np.array_equal(got, want[np.ix_(zi, yi, xi)])
    assert got.any() and not got.all()


def test_read_volume_of_a_terrain_tree_equals_get_blocks(rt, cuda):
    t = rt.Tree.terrain_gpu(4, 200, 200, 0)
    ox, oy, oz, nx, ny, nz = 150, 3, 170, 70, 60, 45      # reaches past the terrain's columns
    got = t.read_volume((ox, oy, oz), (nz, ny, nx)).cpu().numpy().view(np.uint16)
    zz, yy, xx = np.meshgrid(np.arange(oz, oz + nz), np.arange(oy, oy + ny), np.arange(ox, ox + nx), indexing="ij")
    want = t.get_blocks(np.stack([xx.ravel(), yy.ravel(), zz.ravel()], 1)).reshape(nz, ny, nx)
    assert np.array_equal(got, want)
    assert len(np.unique(got)) >= 3


# ----------------------------------------------------------------------------- 4. scale and 64-bit indexing --
PAL4 = [EMPTY, (1, int(vc.colour(1)), 0.0), (1, int(vc.colour(2)), 0.0), (1, int(vc.colour(3)), 0.0)]


def _patterns(torch, nx, ny, nz, dev):
    """three 1-D int16 patterns; vol[z, y, x] = 1 where py is 1 (rows below 32: uniform aligned 16^3 regions),
    (px[x] + pz[z]) % 4 where py is 2 (four rows at every 200th row from 200 on: mixed bricks of three materials and
    holes), 0 elsewhere (empty space).  px and pz have no short period, so a voxel read from a wrong (wrapped) index
    differs"""
    x, y, z = (torch.arange(n, device=dev, dtype=torch.int64) for n in (nx, ny, nz))
    px = ((x * 7) // 13 + x // 97).to(torch.int16)
    pz = ((z * 5) // 11 + z // 61).to(torch.int16)
    py = torch.where(y < 32, 1, torch.where((y >= 200) & (y % 200 < 4), 2, 0)).to(torch.int16)
    if ny <= 200:
        py = torch.where(y < 32, 1, torch.where((y >= 64) & (y < 68), 2, 0)).to(torch.int16)
    return px, py, pz


def _slab(torch, px, py, pz, z0, z1):
    m = (px[None, None, :] + pz[z0:z1, None, None]) % 4
    k = py[None, :, None]
    return torch.where(k == 1, torch.ones_like(m), torch.where(k == 2, m, torch.zeros_like(m)))


def test_levels5_generated_volume_reads_back(rt, cuda):
    """1024 x 128 x 1024, no host world.  Checked once on an MI355X: nodes_per_level [1, 16, 512, 12288, 65536], 65536
    bricks, 3145620 material entries — the tree holds empty space (rows 68..127 and the holes: root children and slots
    without a record), uniform aligned regions (SOLID records for the 16^3 regions of rows 0..31) and mixed bricks (rows
    64..67, all 65536 of them with material runs)."""
    dev = cuda.device("cuda", 0)
    px, py, pz = _patterns(cuda, 1024, 128, 1024, dev)
    vol = _slab(cuda, px, py, pz, 0, 1024).contiguous()
    t = rt.Tree.volume_gpu(5, vol, PAL4)
    i = t.info()
    print("levels-5 nodes_per_level", list(i.nodes_per_level), "bricks", i.n_bricks, "mats", i.n_mat_bytes // 2)
    assert i.n_bricks > 0 and i.n_mat_bytes > 0 and i.n_nodes > i.n_bricks + 1
    assert cuda.equal(t.read_volume((0, 0, 0), vol.shape), vol)


def test_levels6_volume_beyond_2_31_voxels(rt, cuda):
    """2048 x 1100 x 1000 = 2.25e9 voxels (4.5 GB), filled and checked in z-slabs of 100 so that no temporary is larger
    than a slab: a 32-bit voxel index or a grid above 2^32 work-items would read or classify the wrong voxels.  Checked
    once on an MI355X: nodes_per_level [1, 2, 128, 3072, 56448, 648192], 640000 bricks (five bands of four rows),
    30719000 material entries; SOLID 16^3 records for rows 0..31, empty space between the bands."""
    dev = cuda.device("cuda", 0)
    nx, ny, nz, step = 2048, 1100, 1000, 100
    assert nx * ny * nz > 2 ** 31
    px, py, pz = _patterns(cuda, nx, ny, nz, dev)
    vol = cuda.empty((nz, ny, nx), dtype=cuda.int16, device=dev)
    for z0 in range(0, nz, step):
        vol[z0:z0 + step] = _slab(cuda, px, py, pz, z0, z0 + step)
    t = rt.Tree.volume_gpu(6, vol, PAL4, origin=(1024, 0, 2048))
    i = t.info()
    print("levels-6 nodes_per_level", list(i.nodes_per_level), "bricks", i.n_bricks, "mats", i.n_mat_bytes // 2)
    assert i.n_bricks > 0 and i.n_mat_bytes > 0
    out = cuda.empty((step, ny, nx), dtype=cuda.int16, device=dev)
    for z0 in range(0, nz, step):
        t.read_volume((1024, 0, 2048 + z0), (step, ny, nx), out=out)
        assert cuda.equal(out, vol[z0:z0 + step]), "slab at z = %d" % z0
    # one read of more than 2^31 voxels in a single call, compared in place
    del out
    whole = t.read_volume((1024, 0, 2048), (nz, ny, nx))
    assert cuda.equal(whole, vol)


# ------------------------------------------------------------------------------------------ 5. errors on the device --
def test_an_id_equal_to_n_palette_is_reported(rt, cuda):
    vol = cuda.zeros((9, 10, 21), dtype=cuda.int16, device="cuda:0")
    vol[8, 9, 20] = len(PAL4)
    with pytest.raises(rt.SvoError, match="n_palette"):
        rt.Tree.volume_gpu(3, vol, PAL4, origin=(3, 1, 2))
    vol[8, 9, 20] = len(PAL4) - 1
    t = rt.Tree.volume_gpu(3, vol, PAL4, origin=(3, 1, 2))
    assert t.get_block(23, 10, 10)[1] == len(PAL4) - 1
    vol[0, 0, 0] = -1  # 0xFFFF
    with pytest.raises(rt.SvoError, match="n_palette"):
        rt.Tree.volume_gpu(3, vol, PAL4, origin=(3, 1, 2))
