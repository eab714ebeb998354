"""The edit script (tests/edit_script.py) on the CPU, at 3, 4 and 6 levels: after every stage the patched linear trees of
both views (SVO_VIEW_SOLID, SVO_VIEW_ALL) hold, voxel by voxel over the working box, what the oracle's tree holds after
the same putBlock / deleteBlock calls; their column ceilings are a fresh build's; and the script really leaves the
shapes it is there for (more nodes than a fresh build until the forced rebuild).  The device copies of the same trees:
tests/test_gpu_patched_trees.py."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import edit_script as es  # noqa: E402


def check_box(rt, s, tree, view, label):
    """tree.get_blocks over every voxel of the box against orc_dump_box: presence, palette colour and flags"""
    ny = es.BOX_TOP[s.L]
    ids = tree.get_blocks(s.box_points(ny))
    pf, pc = es.palette_arrays(tree)
    rf, rc = s.oracle_box(view, ny)
    rf, rc = rf.reshape(-1), rc.reshape(-1)
    assert np.array_equal(ids == 0, rc == es.EMPTY), "%s: presence differs at %d voxels" % (label, int(((ids == 0) != (rc == es.EMPTY)).sum()))
    assert np.array_equal(pc[ids], rc) and np.array_equal(pf[ids], rf), label
    if s.L == 3:  # the world is the box: its images one and two extents away read the same (the wrap corners among them)
        for shift in ((-64, -64, -64), (64, 64, 64), (-64, 64, 128)):
            assert np.array_equal(tree.get_blocks(s.box_points(ny, shift)), ids), (label, shift)
    return rc


def top_row(tree):
    return int(tree.ceilings()[-1].max())


@pytest.mark.parametrize("levels", [3, 4, 6])
def test_patched_trees_match_oracle(rt, oracle_mod, levels, tmp_path):
    s = es.EditScript(rt, oracle_mod, levels)
    views = (rt.VIEW_SOLID, rt.VIEW_ALL)
    s.trees += [s.w.build(v) for v in views]
    assert [t.info().view for t in s.trees] == list(views)
    n_base = s.trees[0].info().n_nodes
    assert 1500 <= n_base <= 1700 + 3 * (levels - 3), n_base  # (about 1600 nodes: room below the rebuild threshold)
    last = [t.info().n_nodes for t in s.trees]
    tops, stored = {0: top_row(s.trees[0])}, {}
    for stage in s.stages():
        for k, (tree, view) in enumerate(zip(s.trees, views)):
            label = "levels %d stage %d view %d" % (levels, stage, view)
            rc = check_box(rt, s, tree, view, label)
            stored[stage, view] = int((rc != es.EMPTY).sum())
            fresh = s.w.build(view)
            cs, fs = tree.ceilings(), fresh.ceilings()
            assert len(cs) == len(fs) == min(levels - rt.ceiling_layout()[0], 4)
            for j, (a, b) in enumerate(zip(cs, fs)):
                assert np.array_equal(a, b), "%s: ceilings of level %d" % (label, j)
            n, nf = tree.info().n_nodes, fresh.info().n_nodes
            if stage <= 13:  # superseded blocks and uncollapsed regions are really there, and nothing was rebuilt yet
                assert n > nf, (label, n, nf)
                assert n >= last[k], (label, n, last[k])
            if stage == 14 and k == 0:
                assert n < last[k], (label, n, last[k])  # the rebuild
            last[k] = n
        tops[stage] = top_row(s.trees[0])
        if stage == 2:  # the lone voxel's chain is still there: nodes an empty region does not need
            assert s.trees[0].info().n_nodes > n_base
        if stage == 13:
            for tree, view in zip(s.trees, views):
                path = str(tmp_path / ("patched_%d_%d.svo" % (levels, view)))
                tree.save(path)
                back = rt.Tree.load(path)
                pts = s.box_points(es.BOX_TOP[levels])
                assert np.array_equal(back.get_blocks(pts), tree.get_blocks(pts))
                assert back.palette() == tree.palette() and back.info().n_nodes == tree.info().n_nodes and back.info().view == view
                for a, b in zip(back.export(), tree.export()):
                    assert np.array_equal(a, b)
                for a, b in zip(back.ceilings(), tree.ceilings()):
                    assert np.array_equal(a, b)
    print("levels %d: nodes %d -> %s, churned %d pairs, top rows %s" % (levels, n_base, last, s.churned, tops))
    # what the stages are there for
    assert stored[9, rt.VIEW_ALL] - stored[9, rt.VIEW_SOLID] == 16 * 64  # the water is stored in the scene only
    assert stored[4, rt.VIEW_SOLID] - stored[3, rt.VIEW_SOLID] == 4096 and stored[6, rt.VIEW_SOLID] == stored[4, rt.VIEW_SOLID] - 65
    assert stored[8, rt.VIEW_SOLID] == stored[6, rt.VIEW_SOLID]
    if levels > 3:  # the tree's top row rises and falls (svo_tree_sync recomputes dev_top_y from it)
        assert tops[12] == es.ABOVE_Y and tops[11] == tops[13] == 63
    else:
        assert stored[16, rt.VIEW_ALL] == 0 and stored[17, rt.VIEW_ALL] == 1
        assert stored[18, rt.VIEW_SOLID] == 64 ** 3 and stored[19, rt.VIEW_SOLID] == 64 ** 3 - 1
