"""The march's fine descent (svo_ceil_march.h: from 16-column blocks onto the 4-column ceilings, svo_tree.d_ceilf) against
the oracle's castRayFromCam, every field bit-exact (test_gpu_parity.compare), on 3- and 4-level heightfields built so
that the 16-column ceilings say little: one spike per 16 x 16 columns stands far above terraces of 4 x 4 columns.

Chosen rays (frames with a projection plane of size 0: every pixel casts the camera direction) from integral and
half-integral origins reach every way the fine phase ends — a fine ceiling event first, entry at or below a fine
ceiling, a tie at a 4-column corner, a tie between a boundary and a fine ceiling event, the walk through several
16-column blocks and its bound — which classify() below asserts on the inputs by stepping the reference DDA through the
fine table.  Budgets 1 .. 96 end inside each phase; rays wrap in x / z, start under an overhang, climb (the ascending
octants do not march), start from fractional origins (the segment instance: only linear lanes march); a patched tree is
cast after its sync; the diagnostics instance counts the fine blocks.  The table as it is kept in HBM is read back after
every stage of tests/edit_script.py's sequence and after a device-side patch."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cavern  # noqa: E402
from test_gpu_directed_rays import cast_frames, check_frames, ref_frames  # noqa: E402
from test_gpu_parity import compare  # noqa: E402

pytestmark = pytest.mark.gpu

FINE_MAX = 24  # kMarchFineMax of csrc/svo_ceil_march.h
SPIKE = {3: 44, 4: 120}
CAM_Y = 34.0  # above every terrace (at most row 22), below the spikes' tops: the 16-column phase proves nothing from here
# directions: x / z / y crossings in ratios of small integers (exact ties) and general ones; all descend
DIRS = [(1, -1, 1), (1, -0.5, 1), (1, -0.25, 0.5), (0.5, -0.5, 1), (1, -0.125, 1), (1, -0.25, 0.25), (0.25, -0.5, 1), (1, -0.45, 1), (-0.3, -0.6, 1), (0.8, -0.7, -1),
        (-1, -0.25, -1), (1, -0.0625, 0.5), (-1, -0.5, 1), (1, -0.03125, 1), (1, -0.03125, 2.0 ** -10)]


def heights(levels):
    """terraces of 4 x 4 columns, 3 rows apart, and one spike per 16 x 16 columns"""
    E = 1 << (2 * levels)
    x, z = np.meshgrid(np.arange(E), np.arange(E), indexing="ij")
    h = 6 + 3 * (((x >> 2) + 2 * (z >> 2)) % 5) + ((x >> 4) % 2) * 4
    h[(x & 15) == 5 + ((z >> 4) % 3) * 4] = np.where((z & 15) == 9, SPIKE[levels], h)[(x & 15) == 5 + ((z >> 4) % 3) * 4]
    return h.astype(np.int32)


@pytest.fixture(scope="module")
def cuda():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


@pytest.fixture(scope="module")
def worlds(rt, oracle_mod, cuda):
    """{levels: (uploaded Tree, oracle Tree, fine table, 16-column table)}, built once and left unchanged"""
    res = {}
    for levels in (3, 4):
        h = heights(levels)
        t = rt.Tree.heightfield(levels, h)
        res[levels] = (t.upload(0), oracle_mod.Tree.heightfield(levels, h), t.ceilings_fine(), t.ceilings()[0])
    return res


def origins(levels):
    """16 per launch: integral and half-integral, above the terraces and below the spikes' tops"""
    E = 1 << (2 * levels)
    y0 = 26
    o = [(3 + 5 * i, y0 + (i % 3) * 4, 2 + 7 * i) for i in range(8)] + [(E - 2 - 3 * i + 0.5, y0 - 3 + 0.5, 1 + 9 * i + 0.5) for i in range(8)]
    return [(float(x) % E, float(y), float(z) % E) for x, y, z in o]


def classify(org, d, steps, cf, c16):
    """how the march's fine phase ends for the linear ray (org, d), by the reference DDA (ray_caster.cpp:58-80: f64
    accumulation of |f32(1 / d)|) stepped voxel by voxel through the fine table cf [z][x]: a set of the names below"""
    E = cf.shape[0] * 4
    o, dd = np.asarray(org, np.float32), np.asarray(d, np.float32)
    dl = (np.float32(1.0) / dd).astype(np.float64)
    a = np.abs(dl)
    T = a - ((o.astype(np.float64) - (dd < 0)) - np.trunc(o).astype(np.float64)) * dl
    s = np.where(dd < 0, -1, 1)
    p = np.trunc(o).astype(np.int64)
    out, fine_blocks, blocks16 = set(), set(), set()

    def fine(q):
        return int(cf[(q[2] % E) >> 2, (q[0] % E) >> 2])

    for i in range(steps):
        ax = 0 if (T[0] < T[1] and T[0] < T[2]) else (1 if T[1] < T[2] else 2)
        q = p.copy()
        q[ax] += s[ax]
        if i > 0:  # (the first step is taken before the march)
            y = int(p[1]) % E
            if y <= fine(p):
                break
            if y <= int(c16[(p[2] % E) >> 4, (p[0] % E) >> 4]):
                fine_blocks.add(((p[0] % E) >> 2, (p[2] % E) >> 2))
                blocks16.add(((p[0] % E) >> 4, (p[2] % E) >> 4))
            edge = ax != 1 and (q[ax] >> 2) != (p[ax] >> 2)
            x_edge_next = ((p[0] + s[0]) >> 2) != (p[0] >> 2)
            if ax == 2 and edge and T[0] == T[2] and x_edge_next:
                out.add("corner_tie")
                break
            if ax == 1 and int(q[1]) % E <= fine(p):
                out.add("ceiling_event")
                break
            if edge and T[1] == T[ax] and (y - 1) <= fine(p):
                out.add("boundary_ceiling_tie")
                break
            if edge and y <= fine(q):
                out.add("enter_below")
                break
        T[ax] += a[ax]
        p = q
    if len(blocks16) >= 2:
        out.add("across_blocks")
    if len(fine_blocks) > FINE_MAX + 4:
        out.add("bound")
    return out


@pytest.mark.parametrize("levels", [3, 4])
def test_every_end_of_the_fine_phase(rt, oracle_mod, cuda, worlds, levels):
    tree, T, cf, c16 = worlds[levels]
    org = origins(levels)
    seen = set()
    launches = []
    for d in DIRS:
        dn = rt.normalize(d)
        ray = oracle_mod.pixel_dir(dn, 0.0, 0.0, 16, 4, 0, 0)
        for o in org:
            seen |= classify(o, ray, 300, cf, c16)
        launches.append((org, dn))
    # a condition on the inputs: the rays reach every end
    assert seen >= {"ceiling_event", "enter_below", "corner_tie", "boundary_ceiling_tie", "across_blocks", "bound"}, seen
    check_frames(rt, cuda, tree, T, launches, 16, 4, 300, "fine ends L%d" % levels)


@pytest.mark.parametrize("levels", [3, 4])
def test_budget_sweep(rt, worlds, levels):
    """64 x 32 frames, every budget 1 .. 96 and 26 more up to 325: the budget ends in the 16-column phase, in the loop, and
    where the fine phase runs (kMarchFineSpan steps to spare) within its reach, so that its end is given up for the first
    phase's"""
    tree, T, _, _ = worlds[levels]
    org, dn = (4.0, CAM_Y, 4.0), rt.normalize((1.0, -0.45, 1.0))
    for S in list(range(1, 97)) + list(range(200, 330, 5)):  # (from 200 on the fine phase runs, and the budget ends inside it)
        ref = T.cast_frame(org, dn, 64, 32, S)
        assert ref["rc"] == 0
        for flags in (0, rt.CAST_SEGMENTS):
            out = tree.cast_frame(org, dn, 64, 32, S, flags=flags)
            compare(rt, tree, out, ref, "L%d S=%d flags=%d" % (levels, S, flags))
            assert (out["pos_steps"][:, 3] >= 0).all()
    assert tree.guard_trips() == 0


@pytest.mark.parametrize("levels", [3, 4])
def test_octants_wrap_and_fractional_origins(rt, cuda, worlds, levels):
    """64 x 64 frames in all eight octants (the ascending ones do not march) from a corner of the world, so that the rays
    wrap in x and z; from an integral, a half-integral and a fractional origin (the segment instance: its lanes that are
    not linear do not march)"""
    tree, T, _, _ = worlds[levels]
    E = 1 << (2 * levels)
    y = CAM_Y
    for sx in (1.0, -1.0):
        for sy in (1.0, -1.0):
            for sz in (1.0, -1.0):
                dn = rt.normalize((sx, 0.4 * sy, 0.8 * sz))
                for org in ((E - 3.0, y, 2.0), (1.5, y + 0.5, E - 2.5), (E - 2.7, y + 0.3, 1.9)):
                    ref = T.cast_frame(org, dn, 64, 64, 400)
                    assert ref["rc"] == 0
                    for flags in (0, rt.CAST_NO_OCTANT):
                        out = tree.cast_frame(org, dn, 64, 64, 400, flags=flags)
                        compare(rt, tree, out, ref, "L%d %s %s flags=%d" % (levels, org, (sx, sy, sz), flags))
    assert tree.guard_trips() == 0


def test_under_an_overhang(rt, oracle_mod, cuda):
    """the cavern: rays that start under the floating 64^3 block and the roof, where no ceiling proves anything"""
    w, T = cavern.cavern(rt, oracle_mod, False)
    tree = w.build().upload(0)
    x, y, z = cavern.BIG
    dn = rt.normalize((1.0, -0.3, 0.7))
    for org in ((x + 8.0, y - 6.0, z + 8.0), (cavern.ROOF_X + 4.0, cavern.ROOF_Y - 5.0, cavern.ROOF_Z + 4.0), (x - 20.5, y + 80.5, z - 20.5)):
        ref = T.cast_frame(org, dn, 64, 64, 300)
        assert ref["rc"] == 0
        compare(rt, tree, tree.cast_frame(org, dn, 64, 64, 300), ref, "overhang %s" % (org,))
    assert tree.guard_trips() == 0


@pytest.mark.parametrize("levels", [3, 4])
def test_patched_tree_after_sync(rt, oracle_mod, cuda, levels):
    """a column raised and a column lowered inside one 4-column block, by svo_tree_update + svo_tree_sync and by a
    device-side patch: the fine table in HBM is the host tree's, and frames over the block stay bit-exact"""
    h = heights(levels)
    w = rt.World(levels)
    T = oracle_mod.Tree(levels)
    oracle_mod.lib().orc_init_clean_root(T.h)
    pts = [(x, y, z) for x in range(16, 32) for z in range(16, 32) for y in range(int(h[x, z]) + 1)]
    w.put_blocks(pts, np.zeros(len(pts), np.uint32), np.full(len(pts), 5, np.uint64))
    for x, y, z in pts:
        assert T.put_block(x, y, z, 0, 5, 0.0, levels + 1) == 0
    tree = w.build().upload(0)
    assert np.array_equal(tree.device_ceilings_fine(), tree.ceilings_fine())
    org, dn = (12.0, float(h[16:32, 16:32].max() + 6), 12.0), rt.normalize((1.0, -0.6, 1.0))

    def frames(label):
        f = tree.device_ceilings_fine()
        assert np.array_equal(f, tree.ceilings_fine()), label
        ref = T.cast_frame(org, dn, 64, 64, 400)
        assert ref["rc"] == 0
        compare(rt, tree, tree.cast_frame(org, dn, 64, 64, 400), ref, label)
        return f

    f0 = frames("built")
    up, down = (21, int(h[21, 22]) + 5, 22), (22, int(h[22, 23]), 23)  # both in the 4-column block (5, 5), which holds no spike
    for y in range(int(h[21, 22]) + 1, up[1] + 1):
        p = np.array([[up[0], y, up[2]]], np.int32)
        w.put_blocks(p, [0], [6])
        tree.update(w, p)
        assert T.put_block(up[0], y, up[2], 0, 6, 0.0, levels + 1) == 0
    w.delete_block(*down, level=levels + 1)
    tree.update(w, [down])
    assert T.delete_block(*down, level=levels + 1)[0] in (0, 1)
    tree.sync()
    f1 = frames("raised and lowered")
    assert f1[5, 5] == up[1] and (f1 != f0).sum() == 1
    # the raised column lowered again, on the device (the oracle's voxel deletes are not edited a second time: edit_script.py)
    xyz = np.array([[up[0], y, up[2]] for y in range(int(h[21, 22]) + 1, up[1] + 1)], np.int32)
    tree.patch_points(xyz, np.zeros(len(xyz), np.uint16))
    for x, y, z in xyz.tolist():
        assert T.delete_block(x, y, z, level=levels + 1)[0] in (0, 1)
    f2 = frames("lowered on the device")
    assert np.array_equal(f2, f0)
    assert tree.guard_trips() == 0


@pytest.mark.parametrize("levels", [3, 4])
def test_counters(rt, worlds, levels):
    """the diagnostics instance: fine blocks are marched, every descending ray of the frame descends once, nothing trips
    the progress guard; without ceilings nothing marches"""
    tree, _, _, _ = worlds[levels]
    org, dn = (4.0, CAM_Y, 4.0), rt.normalize((1.0, -0.45, 1.0))
    s = tree.cast_stats(org, dn, 64, 64, 300)
    assert s["march_fine"] > 1.0 and 0.5 < s["march_descents"] <= 1.0 and s["no_progress"] == 0
    up = tree.cast_stats(org, rt.normalize((1.0, 0.9, 1.0)), 64, 64, 300)
    assert up["march_fine"] == 0 and up["march_descents"] == 0
    off = tree.cast_stats(org, dn, 64, 64, 300, flags=rt.CAST_NO_CEILINGS)
    assert off["march_fine"] == 0 and off["march_descents"] == 0 and off["no_progress"] == 0


@pytest.mark.parametrize("levels", [3, 4, 6])
def test_kept_table_over_the_edit_sequence(rt, oracle_mod, cuda, levels):
    """The table that is maintained, not a rebuild of it: after each stage of tests/edit_script.py's sequence
    (svo_tree_update, then svo_tree_sync: rectangle re-walks of the host copy, the spans copied to HBM, the whole-tree
    upload of the forced rebuild, the emptied world, the SOLID root, the wrap corners) the fine ceilings read back from
    HBM equal the table rebuilt from the host tree and, at 3 and 4 levels, the column scan by the tree's own lookup; so do
    the 16-column ceilings next to them, which are kept as its 4 x 4 maxima.  Then the same through a device-side patch
    (svo_tree_patch_points_gpu: a column raised, a column erased), which reaches the table by the same sync."""
    import edit_script
    from test_ceil_fine_host import column_tops, fine_want

    s = edit_script.EditScript(rt, oracle_mod, levels)
    tree = s.w.build().upload(0)
    s.trees.append(tree)

    def check(label):
        dev = tree.device_ceilings_fine()
        host = tree.ceilings_fine()
        assert (dev is None) == (host is None), label
        if dev is None:
            return None
        assert np.array_equal(dev, host), label
        if levels < 6:
            assert np.array_equal(dev.astype(np.int64), fine_want(column_tops(tree), 2)), label
        lv, c, _ = tree.device_ceilings()
        n = dev.shape[0] // 4
        assert lv >= 1 and np.array_equal(c[:n * n].reshape(n, n), dev.reshape(n, 4, n, 4).max(axis=(1, 3))), label
        return dev

    check("built")
    tops = set()
    for stage in s.stages():
        tree.sync()
        f = check("stage %d" % stage)
        tops.add(-2 if f is None else int(f.max()))
    assert len(tops) >= 2  # the top moved
    ids = tree.get_blocks(s.box_points())
    pid = int(ids[ids != 0][0])
    ox = s.ox
    # (3 levels: the script leaves a solid world, so a whole 4-column block is erased; else a column rises above the box)
    raised = [] if levels == 3 else [[ox + 40, y, 41] for y in range(64, 76)]
    erased = [[ox + x, y, z] for x in range(32, 36) for z in range(8, 12) for y in range(edit_script.BOX)]
    before = check("before the patch")
    tree.patch_points(np.array(raised + erased, np.int32), np.array([pid] * len(raised) + [0] * len(erased), np.uint16))
    after = check("patched on the device")
    assert after[2, (ox + 32) // 4] == -1 and before[2, (ox + 32) // 4] >= 0
    assert levels == 3 or after[10, (ox + 40) // 4] == 75
    assert tree.guard_trips() == 0
