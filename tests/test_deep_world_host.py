"""The deep-world fixture (tests/deep_world.py) itself, on the CPU, at 6 and 7 levels: the product's World and its
linearised tree (both views) hold the blocks the oracle's tree holds; the column ceilings (svo_tree_ceilings) have four
levels there — 16, 64, 256 and 1024 columns — and each equals the model computed from the put list; and the
preconditions the GPU module (tests/test_gpu_deep_world.py) relies on hold on the oracle's results, so that a broken
fixture shows up here."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import deep_world as dw  # noqa: E402
import deep_cases as dc  # noqa: E402


@pytest.fixture(scope="module", params=dw.LEVELS, ids=lambda v: "levels%d" % v)
def trio(request, rt, oracle_mod):
    levels = request.param
    w, T = dw.deep(rt, oracle_mod, levels)
    return levels, w, T


def _oracle_blocks(T, pts):
    ref = [T.get_block(int(x), int(y), int(z)) for x, y, z in pts]
    return np.array([r[0] for r in ref], np.uint32), np.array([r[1] for r in ref], np.uint64)


def test_the_list_holds_what_the_issue_asks_for():
    for levels in (6, 7):
        g = dw.layout(levels)
        dust = dw.dust_points(levels)
        assert dw.inside(dust, g.big256, 256).sum() >= 1
        if levels == 7:
            assert dw.inside(dust, g.big1024, 1024).sum() >= 1
            assert (np.asarray(g.big1024) // g.q).tolist() != [2, 0, 2]           # another root child than the cavern's
        assert (np.asarray(g.root_solid) // g.q).tolist() not in ([2, 0, 2], [3, 0, 2])
        for pts, _, _, level in dw.puts(levels):
            s = 1 << (2 * (levels + 1 - level))
            assert (pts % s == 0).all() and (pts >= 0).all() and (pts + s <= g.E).all()
            far = (pts[:, 0] < g.H) | (pts[:, 2] < g.H)
            assert not far.any() or s == 1 or level == 2                          # everything else at x, z >= H
        assert tuple(g.far[0]) == (g.H - 1, 777, g.H - 1)
        assert g.roof[0] % 4 and g.roof[2] % 4                                    # the roof's corner is off every block boundary
        xyz, _, _ = dw.light_points(levels)
        assert 400000 < len(xyz) <= 1200000
    edits, ids = dc.patch_edits(7)   # (put-only, at coordinates >= H, no voxel twice: asserted there)
    g = dw.layout(7)
    assert 250 <= len(edits) == len(ids) and dw.inside(edits, g.big64, 64).sum() >= 1 and dw.inside(edits, g.brick63, 4).sum() == 1


def test_block_parity(rt, trio):
    """6000 seeded voxels in and around every structure: World.get_blocks and the built tree's palette entry in both
    views equal the oracle's getBlock (the solid view stores no liquid)"""
    levels, w, T = trio
    pts = dw.probe_points(6000, levels)
    rf, rc = _oracle_blocks(T, pts)
    wf, wc, _ = w.get_blocks(pts)
    assert np.array_equal(wc, rc) and np.array_equal(wf, rf)
    for view in (rt.VIEW_SOLID, rt.VIEW_ALL):
        tree = w.build(view)
        ids = tree.get_blocks(pts)
        pal = tree.palette()
        pf = np.array([p[0] for p in pal], np.uint32)
        pc = np.array([p[1] for p in pal], np.uint64)
        gone = (rf & dw.F_LIQUID) != 0 if view == rt.VIEW_SOLID else np.zeros(len(pts), bool)
        assert np.array_equal(ids == 0, (rc == dw.EMPTY) | gone)
        keep = ids != 0
        assert np.array_equal(pc[ids][keep], rc[keep]) and np.array_equal(pf[ids][keep], rf[keep])
    stored = rc != dw.EMPTY
    assert 0.2 < stored.mean() < 0.8  # the probe sees both
    kinds = set(dw.ident(rc[stored]).tolist())
    for colour in (100, 201, 202, 203, 204, 300, 320, 330, 400, 500, 600, 700, 750, 800, 900, 950) + ((310,) if levels == 7 else ()):
        assert colour in kinds, colour
    assert sum(1000 <= k < 1037 for k in kinds) > 20  # dust
    # the solids with one voxel of another id inside them
    g = dw.layout(levels)
    dust = dw.dust_points(levels)
    for corner, size, own in ((g.big256, 256, 300), (g.big1024, 1024, 310)):
        if corner:
            odd = dust[dw.inside(dust, corner, size)][0]
            here = int(dw.ident(T.get_block(*[int(v) for v in odd])[1]))
            beside = int(dw.ident(T.get_block(int(odd[0]) + 1, int(odd[1]), int(odd[2]))[1]))
            assert 1000 <= here < 1037 and beside == own


def test_ceilings(rt, trio):
    """Tree.ceilings() has exactly four levels and each equals the model; the 1024-column level is not constant, and adjacent
    blocks along every staircase are one block apart"""
    levels, w, T = trio
    tree = w.build()
    cs = tree.ceilings()
    model = dw.ceiling_model(levels)
    assert len(cs) == 4 and tree.ceil_k0 == 2
    for j, (c, m) in enumerate(zip(cs, model)):
        assert c.shape == m.shape and np.array_equal(c.astype(np.int64), m), "ceiling level %d (%d columns)" % (j, 16 << (2 * j))
        assert c.min() == -1 and c.max() == dw.layout(levels).E - 1, j
    assert len(np.unique(cs[3])) >= 4
    g = dw.layout(levels)
    for j, wd in enumerate((16, 64, 256, 1024)):
        x0, z0, depth, n, y0 = g.stairs[wd]
        got = cs[j][z0 // wd, x0 // wd:x0 // wd + n]
        assert np.array_equal(got, [dw.stair_top(g, wd, i) for i in range(n)]), wd
        assert n < 2 or (np.diff(got) == wd).all()
    # overhangs: empty space under the floating solids
    x, y, z = g.big256
    assert model[0][(z + 5) >> 4, (x + 5) >> 4] >= y + 255 and T.get_block(x + 5, y - 1, z + 5)[1] == int(dw.EMPTY)


def test_gpu_module_preconditions(rt, oracle_mod, trio):
    """the conditions tests/test_gpu_deep_world.py asserts on the oracle's results, computed here as well"""
    levels, w, T = trio
    dc.check_preconditions(rt, oracle_mod, T, levels)
