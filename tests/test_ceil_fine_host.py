"""The fine column ceilings (svo_tree_ceilings_fine: per aligned block of 4 x 4 columns the highest stored voxel row, -1
for none — the table the march before the traversal loop descends onto) against a brute-force column scan of the tree
by its own voxel lookup (svo_tree_get_blocks), at 3 and 4 levels: terrain, the overhang world of tests/cavern.py, a
SOLID region above the brick level, an empty tree, a tree too shallow to have the level, and every stage of
tests/edit_script.py's edit sequence through svo_tree_update.  No GPU."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cavern  # noqa: E402
import edit_script  # noqa: E402


def column_tops(tree, y_rows=None):
    """[z][x] the highest row of each column holding a voxel of the tree's view (-1: none), by lookups of every voxel"""
    E = 1 << (2 * tree.info().levels)
    top = np.full((E, E), -1, np.int64)
    ys = np.arange(E if y_rows is None else y_rows)
    slab = max(1, (1 << 21) // (E * len(ys)))  # z-rows per batch of lookups
    for z0 in range(0, E, slab):
        z, y, x = np.meshgrid(np.arange(z0, min(E, z0 + slab)), ys, np.arange(E), indexing="ij")
        ids = tree.get_blocks(np.stack([x, y, z], -1).reshape(-1, 3).astype(np.int32)).reshape(z.shape)
        top[z0:z0 + slab] = np.where(ids != 0, y, -1).max(axis=1)
    return top


def fine_want(top, shift):
    B, n = 1 << shift, top.shape[0] >> shift
    return top.reshape(n, B, n, B).max(axis=(1, 3))


def check(rt, tree, y_rows=None):
    """the fine table against the scan, and against the level above it (a 16-column block's ceiling is its 16 sub-blocks')"""
    f = tree.ceilings_fine()
    cs = tree.ceilings()
    assert (f is None) == (len(cs) == 0)
    if f is None:
        return None
    assert f.dtype == np.int16
    want = fine_want(column_tops(tree, y_rows), 2 * (rt.ceiling_layout()[0] - 1))
    assert f.shape == want.shape and np.array_equal(f.astype(np.int64), want)
    n = cs[0].shape[0]
    assert np.array_equal(f.reshape(n, 4, n, 4).max(axis=(1, 3)), cs[0])
    return f


@pytest.mark.parametrize("levels", [3, 4])
@pytest.mark.parametrize("view", [0, 1])
def test_terrain(rt, levels, view):
    E = 1 << (2 * levels)
    W, L = (64, 64) if levels == 3 else (200, 256)  # (4 levels: columns beyond x = 200 hold nothing)
    f = check(rt, rt.Tree.terrain(levels, W, L, view=view))
    assert f.shape == (E // 4, E // 4) and f.max() > 0
    assert levels == 3 or (f[:, W // 4:] == -1).all()
    assert len(np.unique(f)) > 4  # neighbouring sub-blocks differ: the table says more than the level above it


@pytest.mark.parametrize("tall", [False, True], ids=["low", "tall"])
def test_cavern_overhangs(rt, oracle_mod, tall):
    """ceilings above empty space: the highest stored row, whatever lies under it"""
    w, _ = cavern.cavern(rt, oracle_mod, tall)
    tree = w.build()
    # (a 1024^3 world: every row of the columns its structures occupy is scanned; every other column must hold nothing)
    top = np.full((cavern.E, cavern.E), -1, np.int64)
    for x0, z0, nx, nz, _ in cavern.occupied_boxes(tall):
        for zz in range(z0, z0 + nz, 8):
            z, y, x = np.meshgrid(np.arange(zz, min(z0 + nz, zz + 8)), np.arange(cavern.E), np.arange(x0, x0 + nx), indexing="ij")
            ids = tree.get_blocks(np.stack([x, y, z], -1).reshape(-1, 3).astype(np.int32)).reshape(z.shape)
            top[zz:zz + z.shape[0], x0:x0 + nx] = np.maximum(top[zz:zz + z.shape[0], x0:x0 + nx], np.where(ids != 0, y, -1).max(axis=1))
    f = tree.ceilings_fine()
    assert np.array_equal(f.astype(np.int64), fine_want(top, 2))
    n = cavern.E // 16
    assert np.array_equal(f.reshape(n, 4, n, 4).max(axis=(1, 3)), tree.ceilings()[0])  # (which test_cavern_host.py scans)
    x, y, z = cavern.BIG
    assert f[(z + 5) // 4, (x + 5) // 4] >= y + 63 and tree.get_blocks([(x + 5, y - 1, z + 5)])[0] == 0


@pytest.mark.parametrize("levels", [3, 4])
def test_solid_region_above_bricks(rt, levels):
    """a 16^3 (and at 4 levels a 64^3) block of one material is a SOLID record above the brick level: its top row over
    every sub-block under it; a lone voxel beside it is a brick"""
    w = rt.World(levels)
    w.put_blocks([(16, 32, 16)], [0], [77], level=levels - 1)  # 16^3 at (16..31, 32..47, 16..31)
    if levels == 4:
        w.put_blocks([(64, 128, 128)], [0], [78], level=levels - 2)  # 64^3
    w.put_blocks([(2, 9, 41)], [0], [79])
    f = check(rt, w.build())
    assert (f[4:8, 4:8] == 47).all() and f[10, 0] == 9 and (f[0:4, 0:4] == -1).all()
    if levels == 4:
        assert (f[32:48, 16:32] == 191).all()


@pytest.mark.parametrize("levels", [3, 4])
def test_empty_tree(rt, levels):
    f = check(rt, rt.World(levels).build())
    assert f is None or (f == -1).all()


def test_tree_too_shallow(rt):
    """two levels (16^3): no ceiling table, so no fine one either"""
    w = rt.World(2)
    w.put_blocks([(3, 4, 5)], [0], [5])
    t = w.build()
    assert t.ceilings() == [] and t.ceilings_fine() is None
    check(rt, t)


@pytest.mark.parametrize("levels", [3, 4])
def test_edit_sequence(rt, oracle_mod, levels):
    """after each stage of the scripted edits (svo_tree_update): ceilings that rise and fall, a world emptied, uniform
    and mixed again"""
    es = edit_script.EditScript(rt, oracle_mod, levels)
    tree = es.w.build()
    es.trees.append(tree)
    check(rt, tree)
    seen = set()
    for s in es.stages():
        f = check(rt, tree)
        seen.add(None if f is None else int(f.max()))
    assert len(seen) >= 2  # the top moved
