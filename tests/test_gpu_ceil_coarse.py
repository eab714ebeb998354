"""The march's coarse levels (svo_ceil_march.h: 256- and 64-column blocks before the 16- and 4-column ones, one loop per
level, for launches whose budget spans 8 blocks of a level) against the oracle's castRayFromCam, every field bit-exact
(test_gpu_parity.compare).  Worlds: 5-level trees (1024^3: the 256-column level has 4 x 4 blocks) and 4-level trees (256^3:
no 256-column level, the 64-column one has 4 x 4), from a heightfield whose coarse ceilings say much in some blocks and
nothing in others (ceil_coarse_cases.heights) and from tests/cavern.py's world.

Chosen rays (frames with a projection plane of size 0: every pixel casts the camera direction) reach every way a coarse
phase ends — entry at or below a ceiling, the ceiling event first, an x / z corner tie, a tie between a boundary and the
ceiling event, a next boundary beyond the budget — cross the world's edge at each coarse level, and descend after an x
entry, after a z entry and from the block they start in, at each level: ceil_coarse_cases.march restates the march on the
CPU and says which, the test asserts the set on its inputs, and the diagnostics instance's counters (Tree.cast_stats'
buffer) must equal the restatement's block counts ray for ray.  Cameras above and below the tree's top row, budgets that
end in each phase, all eight octants, patched trees, and launches with the ceilings off."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cavern  # noqa: E402
import ceil_coarse_cases as cc  # noqa: E402
from test_gpu_directed_rays import check_frames  # noqa: E402
from test_gpu_parity import compare  # noqa: E402

pytestmark = pytest.mark.gpu

# directions: x / z / y crossings in ratios of small integers (exact ties) and general ones; all descend
DIRS = [(1, -1, 1), (1, -0.5, 1), (1, -0.25, 0.5), (0.5, -0.5, 1), (1, -0.125, 1), (1, -0.25, 0.25), (1, -0.45, 1), (-0.3, -0.6, 1),
        (0.8, -0.7, -1), (-1, -0.25, -1), (1, -0.0625, 0.5), (-1, -0.5, 1), (1, -0.03125, 1), (0.25, -0.03125, -1), (1, -2, 1), (-1, -1, -0.5)]
# a coarse level is walked when the budget spans 8 of its blocks (kMarchCoarseSpan): 2500 steps walk the 256- and the
# 64-column level, 700 the 64-column one, 60 neither (the march as it was)
BUDGETS = (2500, 700, 60)


@pytest.fixture(scope="module")
def cuda():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


@pytest.fixture(scope="module")
def worlds(rt, oracle_mod, cuda):
    """{levels: (uploaded Tree, oracle Tree, {width: ceilings}, top row)}, built once and left unchanged"""
    res = {}
    for levels in (4, 5):
        h = cc.heights(levels)
        t = rt.Tree.heightfield(levels, h)
        res[levels] = (t.upload(0), oracle_mod.Tree.heightfield(levels, h), cc.tables(t), int(h.max()))
    return res


def origins(levels):
    """16 per launch, integral and half-integral: above the tree's top row and below it (above the hills, under the spikes'
    tops), near the world's edge and inside it"""
    E = 1 << (2 * levels)
    top = cc.SPIKE[levels]
    o = [(3 + 61 * i, top + 9 + 5 * (i % 3), 2 + 67 * i) for i in range(4)] + [(5 + 29 * i, 70 + 4 * i, 5 + 29 * i) for i in range(4)]
    o += [(E - 2 - 3 * i + 0.5, 60.5 + 20 * i, 1 + 9 * i + 0.5) for i in range(4)] + [(130 + 17 * i, 52 + 6 * i, E - 3 - 40 * i) for i in range(2)]
    o[3] = (7, (top + E) // 2, 9)  # high above the top row: along the shallow directions its budget ends first, so it marches from here, until the next boundary lies beyond the budget
    o += [(0, 75, 3) if levels == 5 else (14, 48, 3), (0, 146, 50)]  # (5 levels, along (1, -0.5, 1): a boundary event equal to the ceiling event of a 64- and a 256-column block)
    return [(float(x) % E, float(y), float(z) % E) for x, y, z in o]


def raw_stats(rt, cuda, tree, orgs, dn, W, H, steps):
    """the diagnostics instance's counters of one launch over the camera positions orgs, summed over its rays: {name: int}"""
    d = rt.Tree.frame_desc(orgs[0], dn, W, H, steps, ppx=0.0, ppy=0.0, flags=rt.CAST_STATS, frame_origins=orgs)
    n = rt.Tree.count(d)
    st = cuda.zeros(rt.STATS_HEADER + 2 * tree.blocks(d) + n, dtype=cuda.int64, device="cuda:0")
    d.stats = st.data_ptr()
    tree.cast(d, rt.Tree.alloc_hits(n, 0))
    cuda.cuda.synchronize()
    names = rt.STAT_NAMES + rt.MARCH_STAT_NAMES
    return dict(zip(names, st[:len(names)].cpu().tolist()))


@pytest.mark.parametrize("levels", [4, 5])
def test_every_end_of_the_coarse_phases(rt, oracle_mod, cuda, worlds, levels):
    tree, T, tabs, top = worlds[levels]
    E = 1 << (2 * levels)
    coarse = [w for w in cc.march_widths(tabs) if w > 16]
    assert coarse == ([256, 64] if levels == 5 else [64])
    org = origins(levels)
    seen = set()
    for S in BUDGETS:
        launches = []
        for d in DIRS:
            dn = rt.normalize(d)
            ray = oracle_mod.pixel_dir(dn, 0.0, 0.0, 16, 4, 0, 0)
            want = {"march_256": 0, "march_64": 0, "march_fine": 0, "march_descents": 0}
            for o in org:
                m = cc.march(o, ray, S, tabs, E, pre_top=top)
                assert m is not None and (S >= 256 or m["widths"] == [16, 4])
                for w, rec in m["levels"].items():
                    if w > 16:
                        seen |= {(w, rec["end"])} | ({(w, "wrap")} if rec["wrap"] else set())
                        want["march_%d" % w] += rec["blocks"]
                    if w < m["widths"][0]:  # the descent onto this level came from the block the level above ended in
                        seen.add((4 * w, "descent_" + rec["entry"]))
                if 4 in m["levels"]:
                    want["march_fine"] += m["levels"][4]["blocks"]
                    want["march_descents"] += 1
            # the kernel's own counters say the same, ray for ray (64 equal rays per camera position)
            got = raw_stats(rt, cuda, tree, org, dn, 16, 4, S)
            assert got["no_progress"] == 0
            for k, v in want.items():
                assert got[k] == 64 * v, (levels, S, d, k, got[k] / 64.0, v)
            launches.append((org, dn))
        check_frames(rt, cuda, tree, T, launches, 16, 4, S, "coarse ends L%d" % levels)
    # a condition on the inputs: the rays reach every end, at every coarse level
    need = {(w, e) for w in coarse for e in ("enter_below", "ceiling_event", "corner_tie", "boundary_ceiling_tie", "beyond_budget", "wrap",
                                             "descent_x", "descent_z", "descent_start")}
    assert seen >= need, sorted(need - seen)


@pytest.mark.parametrize("levels", [4, 5])
def test_budget_sweep_above_and_below_the_top_row(rt, worlds, levels):
    """64 x 32 frames from above the tree's top row and from below it, every budget 1 .. 96 and 26 more up to 325: the budget
    ends above the top row, in the 16- and 4-column phases in turn, and in the loop; then budgets round 512 and 2048 steps,
    where the 64- and the 256-column level come in, and up to 2600, which end in the coarse phases' reach"""
    tree, T, _, top = worlds[levels]
    dn = rt.normalize((1.0, -0.45, 1.0))
    for org in ((4.0, float(top + 30), 4.0), (4.0, 70.0, 4.0)):
        for S in list(range(1, 97)) + list(range(200, 330, 5)) + list(range(505, 600, 6)) + list(range(2040, 2100, 7)) + [700, 900, 1500, 2600]:
            ref = T.cast_frame(org, dn, 64, 32, S)
            assert ref["rc"] == 0
            for flags in (0, rt.CAST_SEGMENTS):
                out = tree.cast_frame(org, dn, 64, 32, S, flags=flags)
                compare(rt, tree, out, ref, "L%d %s S=%d flags=%d" % (levels, org, S, flags))
                assert (out["pos_steps"][:, 3] >= 0).all()
    assert tree.guard_trips() == 0


@pytest.mark.parametrize("levels", [4, 5])
def test_octants_and_switches(rt, cuda, worlds, levels):
    """64 x 32 frames in all eight octants from a corner of the world (the rays wrap in x and z), from an integral and a
    fractional origin (the segment instance: its lanes that are not linear do not march); the four ascending octants count
    no march block at any level; the ceilings off and the iterative cast give the same frames"""
    tree, T, _, top = worlds[levels]
    E = 1 << (2 * levels)
    for sx in (1.0, -1.0):
        for sy in (1.0, -1.0):
            for sz in (1.0, -1.0):
                dn = rt.normalize((sx, 0.4 * sy, 0.8 * sz))
                for org in ((E - 3.0, float(top + 12), 2.0), (E - 2.7, 80.3, 1.9)):
                    ref = T.cast_frame(org, dn, 64, 32, 2400)
                    assert ref["rc"] == 0
                    for flags in (0, rt.CAST_NO_OCTANT, rt.CAST_NO_CEILINGS, rt.CAST_ITERATIVE):
                        out = tree.cast_frame(org, dn, 64, 32, 2400, flags=flags)
                        compare(rt, tree, out, ref, "L%d %s %s flags=%d" % (levels, org, (sx, sy, sz), flags))
                s = tree.cast_stats((E - 3.0, float(top + 12), 2.0), dn, 64, 32, 2400)
                marched = s["march_64"] + s["march_256"] + s["march_fine"] + s["march_descents"]
                assert s["no_progress"] == 0 and ((marched == 0) if sy > 0 else (s["march_64"] > 0)), (sx, sy, sz, s)
    off = tree.cast_stats((E - 3.0, float(top + 12), 2.0), rt.normalize((1.0, -0.4, 0.8)), 64, 32, 2400, flags=rt.CAST_NO_CEILINGS)
    assert off["march_64"] == 0 and off["march_256"] == 0 and off["march_fine"] == 0 and off["ceil_moves"] == 0
    assert tree.guard_trips() == 0


def test_cavern(rt, oracle_mod, cuda):
    """tests/cavern.py's world (5 levels, not a heightfield): from high above it, from beside the floating block and from
    under the roof, where no ceiling proves anything; the coarse levels pass blocks over the empty root children"""
    w, T = cavern.cavern(rt, oracle_mod, False)
    tree = w.build().upload(0)
    x, y, z = cavern.BIG
    for d in ((1.0, -0.3, 0.7), (-1.0, -0.6, -0.4)):
        dn = rt.normalize(d)
        for org in ((40.0, 900.0, 60.0), (x - 20.5, y + 80.5, z - 20.5), (x + 8.0, y - 6.0, z + 8.0), (cavern.ROOF_X + 4.0, cavern.ROOF_Y - 5.0, cavern.ROOF_Z + 4.0)):
            ref = T.cast_frame(org, dn, 64, 32, 3000)
            assert ref["rc"] == 0
            for flags in (0, rt.CAST_NO_CEILINGS):
                compare(rt, tree, tree.cast_frame(org, dn, 64, 32, 3000, flags=flags), ref, "cavern %s %s flags=%d" % (org, d, flags))
    s = tree.cast_stats((40.0, 900.0, 60.0), rt.normalize((1.0, -0.3, 0.7)), 64, 32, 3000)
    assert s["march_256"] > 0 and s["march_64"] > 0 and s["no_progress"] == 0
    assert tree.guard_trips() == 0


@pytest.mark.parametrize("levels", [4, 5])
def test_patched_tree(rt, oracle_mod, cuda, levels):
    """a tower raised inside a coarse block whose ceiling was low, by svo_tree_update + svo_tree_sync, and a second one by a
    device-side patch: the coarse tables in HBM are the host tree's, and frames over the blocks stay bit-exact"""
    E = 1 << (2 * levels)
    w = rt.World(levels)
    T = oracle_mod.Tree(levels)
    oracle_mod.lib().orc_init_clean_root(T.h)
    pts = [(x, y, z) for x in range(64, 128, 3) for z in range(64, 128, 5) for y in range(3 + (x + z) % 4)]
    pts += [(200, y, 201) for y in range(131)]  # a pillar elsewhere: the tree's top row stays 130 throughout
    w.put_blocks(pts, np.zeros(len(pts), np.uint32), np.full(len(pts), 5, np.uint64))
    for x, y, z in pts:
        assert T.put_block(x, y, z, 0, 5, 0.0, levels + 1) == 0
    tree = w.build().upload(0)
    org, dn = (20.0, 150.0, 24.0), rt.normalize((1.0, -0.9, 1.0))
    S = 2000  # (spans 8 blocks of the 64-column level)

    def frames(label):
        lv, c, _ = tree.device_ceilings()
        host = np.concatenate([np.asarray(a).reshape(-1) for a in tree.ceilings()])
        assert lv == levels - 2 and np.array_equal(c[:len(host)], host), label
        ref = T.cast_frame(org, dn, 64, 32, S)
        assert ref["rc"] == 0
        compare(rt, tree, tree.cast_frame(org, dn, 64, 32, S), ref, label)
        return tree.cast_stats(org, dn, 64, 32, S)

    s0 = frames("built")
    tower = np.array([[100, y, 101] for y in range(0, 120)], np.int32)
    for x, y, z in tower.tolist():
        w.put_blocks(np.array([[x, y, z]], np.int32), [0], [6])
        assert T.put_block(x, y, z, 0, 6, 0.0, levels + 1) == 0
    tree.update(w, tower)
    tree.sync()
    s1 = frames("tower raised")
    assert 0 < s1["march_64"] < s0["march_64"]  # the tower's 64-column block stops the coarse phase earlier
    # a second tower, two 64-column blocks on, raised on the device (the oracle's tree takes it voxel by voxel)
    pid = int(tree.get_blocks([(200, 0, 201)])[0])
    second = np.array([[150, y, 170] for y in range(0, 100)], np.int32)
    tree.patch_points(second, np.full(len(second), pid, np.uint16))
    for x, y, z in second.tolist():
        assert T.put_block(x, y, z, 0, 5, 0.0, levels + 1) == 0
    s2 = frames("second tower raised on the device")
    assert 0 < s2["march_64"] <= s1["march_64"] and s2["no_progress"] == 0
    assert tree.guard_trips() == 0
