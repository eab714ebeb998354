"""The device copy of a patched tree: svo_tree_update + svo_tree_sync after every stage of the edit script
(tests/edit_script.py; host side: tests/test_patched_host.py) against the oracle's tree after the same edits.

A patched tree holds shapes no builder emits (a mask-0 interior node under a set bit, 64 SOLID siblings of one material,
child blocks rewritten at the tail, one record rewritten in place) and svo_tree_sync moves only what changed: the
appended tail, runs of rewritten records, rows of the ceiling tables, dev_top_y.  After every stage's sync:

  readback  every voxel of the working box is read back from HBM by a one-step ray from the centre of the voxel before
            it (262,144 explicit rays, direction (+-1, +-2^-20, +-2^-20) with the large component cycling through the six
            axis directions): the ray ends in the neighbouring voxel, so pos, hit, material, stepsLeft = 0, lastPos and
            t = 0.5 follow from orc_dump_box moved by one voxel (wrapped at 3 levels, where the box is the world; at 4
            and 6 levels the origins are the box moved back by one voxel).  A seeded sample of the same rays (6,000 over
            the stages) goes through the oracle's castRayFromCam to pin that rule.  Casts with flags 0, CAST_ITERATIVE
            and CAST_NO_CEILINGS, every field through test_gpu_parity.compare, no ray left out, no guard trip.
  frames    96 x 64 frames from an integral (linear octant instance), a half-integral and a fractional (segment instance)
            origin looking across the edits, and from above the box down on the voxel that raises the tree's top row
            (stages 12 / 13: rays that start above dev_top_y), S = 7 and 300, under every flag of
            test_gpu_directed_rays.frame_flags, against orc_cast_frame; one AO frame (16 samples, 5 steps) per stage
            against the oracle's counts.
  ceilings  device_ceilings() / device_ceiling_quads() equal those of a fresh build freshly uploaded, and the pair and
            quad tables derived from the host ceilings() (6 levels: all four ceiling levels).
  shade     both trees updated and synced; shade_frame(scene=) from three cameras (mirror, glass and water; dust behind
            them; the raised top from above) against the oracle's liquid shading, lit pixels bit-exact, sky within
            SKY_ATOL; the image without hit records (early escape above dev_top_y, which stages 12 / 13 raise and lower)
            equals the one with them.
  idle      a second sync() with nothing changed leaves the records, frames and tables as they were.

A VIEW_ALL scene tree is refused by the casts (test_gpu_shade.py::test_full_view_tree_is_not_castable): its device copy
is checked through `shade` only, its host image voxel by voxel in tests/test_patched_host.py."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import edit_script as es  # noqa: E402
from test_gpu_directed_rays import check_frames, no_guard, ref_rays, take  # noqa: E402
from test_gpu_edits import _pairs_of, _quads_of  # noqa: E402
from test_gpu_parity import compare  # noqa: E402

pytestmark = pytest.mark.gpu

LEVELS = [3, 4, 6]
AXES = [(0, 1), (0, -1), (1, 1), (1, -1), (2, 1), (2, -1)]  # (axis, sign) of the read-back rays' large component
EPS = 2.0 ** -20
N_SAMPLE = 6000
W, H = 96, 64
# (origin relative to OX, direction): in the emptied half of the box, looking across the edits at the dust
CAMS = {"integral": ((14.0, 16.0, 17.0), (1.0, -0.2, -0.3)), "half": ((2.5, 12.5, 30.5), (1.0, -0.1, -0.6)),
        "fractional": ((10.3, 40.7, 2.45), (0.8, -0.7, 0.5)),
        # above the box, looking down on the voxel stages 12 / 13 put and delete in row ABOVE_Y: its rays start above the tree's top
        # row (trace: pre_top, from dev_top_y), which that voxel raises and lowers
        "above": ((2.5, 84.5, 1.5), (0.3, -1.0, 0.35))}
ABOVE = CAMS["above"]
SHADE_CAMS = [((30.5, 38.5, 10.5), (-0.7, -0.1, 0.7)),   # the mirror, the glass wall and the water from the dust's side
              ((-4.5, 40.5, 50.5), (1.0, -0.25, -0.45)),  # glass and mirror with the dust behind them
              ABOVE]


@pytest.fixture(scope="module")
def cuda():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


def start(rt, oracle_mod, levels, scene=False):
    """the script with its base world built and the solid tree (and the scene tree) uploaded"""
    s = es.EditScript(rt, oracle_mod, levels)
    s.trees.append(s.w.build().upload(0))
    if scene:
        s.trees.append(s.w.build(rt.VIEW_ALL).upload(0))
    return s


def synced(s):
    """the script's stages, every tree synced once after each"""
    for stage in s.stages():
        for t in s.trees:
            t.sync()
        yield stage


def cam_at(rt, s, cam):
    """the camera in the script's box.  At 3 levels the box is the world and every long ray wraps; the camera then stands 16
    extents up in x, y and z (the same place to the product, which wraps coordinates), so that no ray reaches negative
    coordinates: there the oracle's getBlock misreads the voxels deleted on their own (edit_script: voxel_deletes) and
    castRayFromCam reports an error for the ray."""
    (x, y, z), d = cam
    up = 16 * es.BOX if s.L == 3 else 0
    return (x + s.ox + up, y + up, z + up), rt.normalize(d)


# ------------------------------------------------------------------------------------------------------------ readback --
def readback_rays(s, stage):
    """(origins f32, direction f32, reference): one ray per voxel of the box, ending in it (3 levels: in its wrapped
    neighbour), and what compare() must find there according to orc_dump_box"""
    axis, sign = AXES[stage % 6]
    d = np.empty(3, np.float32)
    d[axis] = sign
    d[(axis + 1) % 3] = EPS * (1 if (stage // 6) % 2 == 0 else -1)
    d[(axis + 2) % 3] = EPS * (1 if (stage // 3) % 2 == 0 else -1)
    step = np.zeros(3, np.int32)
    step[axis] = sign
    vox = s.box_points() if s.L == 3 else s.box_points(shift=-step)
    if s.L > 3:  # (row -1 by its image at the top of the world: castRayFromCam truncates, so -0.5 would lie in voxel 0)
        vox = np.where(vox < 0, vox + (1 << (2 * s.L)), vox)
    end = vox + step
    rel = (end - np.array([s.ox, 0, 0], np.int32)) & (es.BOX - 1)
    assert s.L == 3 or np.array_equal(end & ((1 << (2 * s.L)) - 1), s.box_points())  # the voxels read are exactly the box
    f, c = s.oracle_box(s.rt.VIEW_SOLID)
    f, c = f[rel[:, 2], rel[:, 1], rel[:, 0]], c[rel[:, 2], rel[:, 1], rel[:, 0]]
    n = len(vox)
    ref = dict(pos=end.astype(np.int64), last=vox.astype(np.int64), steps=np.zeros(n, np.int64), hit=(c != es.EMPTY).astype(np.int64),
               flags=f, color=c, t=np.full(n, 0.5))
    return (vox + np.float32(0.5)).astype(np.float32), d, ref


def rule_sample(s, stage, org, d, ref, k):
    """k seeded rays of the battery through the oracle's castRayFromCam: the rule readback_rays states is the oracle's.
    Left out: rays ending at a negative coordinate in a voxel deleted on its own (edit_script: voxel_deletes)."""
    ok = np.ones(len(org), bool)
    if s.voxel_deletes:
        gone = np.array(s.voxel_deletes, np.int64)
        neg = (ref["pos"] < 0).any(1)
        wrapped = ref["pos"][neg] & (es.BOX - 1)
        ok[np.nonzero(neg)[0][(wrapped[:, None, :] == gone[None, :, :]).all(2).any(1)]] = False
    idx = np.sort(np.random.default_rng(100 + stage).choice(np.nonzero(ok)[0], k, replace=False))
    got = ref_rays(s.T, org[idx], np.tile(d, (k, 1)), 1)
    want = take(ref, idx)
    for key in got:
        assert np.array_equal(got[key], want[key]), "stage %d: the oracle's %s differs from the one-step rule at %d of %d rays" % (
            stage, key, int((got[key] != want[key]).reshape(k, -1).any(1).sum()), k)
    return k


@pytest.mark.parametrize("levels", LEVELS)
def test_readback(rt, oracle_mod, cuda, levels):
    s = start(rt, oracle_mod, levels)
    tree = s.trees[0]
    per_stage = -(-N_SAMPLE // es.N_STAGES[levels])
    sampled, stored = 0, []
    for stage in synced(s):
        org, d, ref = readback_rays(s, stage)
        assert len(org) == es.BOX ** 3
        sampled += rule_sample(s, stage, org, d, ref, per_stage)
        go, gd = cuda.from_numpy(org).cuda(), cuda.from_numpy(np.tile(d, (len(org), 1))).cuda()
        for flags in (0, rt.CAST_ITERATIVE, rt.CAST_NO_CEILINGS):
            out = tree.cast_rays(gd, go, steps=1, flags=flags)
            compare(rt, tree, out, ref, "readback levels %d stage %d flags %d" % (levels, stage, flags))
            no_guard(rt, tree, out)
        stored.append(int(ref["hit"].sum()))
    assert sampled >= N_SAMPLE
    print("readback levels %d: stored voxels per stage %s, %d rays through the oracle" % (levels, stored, sampled))
    assert stored[3] - stored[2] == 4096 and len(set(stored)) >= 7  # the box changes from stage to stage


# -------------------------------------------------------------------------------------------------------------- frames --
@pytest.mark.parametrize("kind", sorted(CAMS))
@pytest.mark.parametrize("levels", LEVELS)
def test_frames(rt, oracle_mod, cuda, levels, kind):
    s = start(rt, oracle_mod, levels)
    tree = s.trees[0]
    org, dn = cam_at(rt, s, CAMS[kind])
    desc = rt.Tree.frame_desc(org, dn, W, H, 300, frame_origins=[org])
    assert tree.wire_bytes(desc) == (12 if kind == "fractional" else 8)  # (the launch's instance follows the same test: need_seg)
    fr, on_top = [], {}
    for stage in synced(s):
        for S in (7, 300):
            ref = check_frames(rt, cuda, tree, s.T, [([org], dn)], W, H, S, "frames levels %d %s stage %d" % (levels, kind, stage),
                               ppx=None, ppy=None)
        fr.append((ref["hit"] != 0).mean())
        on_top[stage] = int(((ref["pos"] == (s.ox + 5, es.ABOVE_Y, 5)).all(1) & (ref["hit"] != 0)).sum())
        ao, hit = s.T.cast_frame_ao(org, dn, W, H, 300, 16, 5)
        g = rt.decode_hits(tree.cast_frame(org, dn, W, H, 300, ao_samples=16, ao_steps=5))
        assert np.array_equal(g["hit"], hit != 0) and np.array_equal(g["ao"], ao), (levels, kind, stage)
        no_guard(rt, tree)
    print("frames levels %d %s: oracle hit fraction per stage (S = 300) %s" % (levels, kind, " ".join("%.2f" % f for f in fr)))
    assert fr[3] > fr[2]  # the 16^3 of stage 4 is in view
    if levels > 3:  # hits and misses (at 3 levels the box is the world: every ray comes round to the dust)
        assert all(0.1 < f < 0.995 for f in fr)
        if kind == "above":  # the raised top is hit from above it, and gone again
            assert on_top[12] > 100 and on_top[11] == on_top[13] == 0, on_top


# ------------------------------------------------------------------------------------------------------------ ceilings --
def device_tables(tree):
    lv, c, p = tree.device_ceilings()
    return lv, c, p, tree.device_ceiling_quads()


@pytest.mark.parametrize("levels", LEVELS)
def test_ceiling_tables(rt, oracle_mod, cuda, levels):
    s = start(rt, oracle_mod, levels)
    tree = s.trees[0]
    E = 1 << (2 * levels)
    k0, pair_step = rt.ceiling_layout()
    changed, last = 0, None
    for stage in synced(s):
        label = "levels %d stage %d" % (levels, stage)
        lv, c, p, q = device_tables(tree)
        flv, fc, fp, fq = device_tables(s.w.build().upload(0))
        assert lv == flv and np.array_equal(c, fc), label + ": ceilings differ from a fresh upload's"
        assert np.array_equal(p, fp), label + ": pairs differ from a fresh upload's"
        assert np.array_equal(q, fq), label + ": quads differ from a fresh upload's"
        host = tree.ceilings()
        assert lv == len(host)
        if lv:
            assert lv == min(levels - k0, 4)
            full = np.concatenate([x.reshape(-1) for x in host])
            assert np.array_equal(c, full), label
            assert np.array_equal(p, _pairs_of(full, E, k0, lv, pair_step)), label + ": pair table"
            assert np.array_equal(q, _quads_of(full, E, k0, lv)), label + ": quads"
        changed += last is not None and not np.array_equal(c, last)
        last = c
    assert changed >= 4  # (the ceilings moved: lone voxel, the top rising and falling, the root edits)


# --------------------------------------------------------------------------------------------------------------- shade --
@pytest.mark.parametrize("levels", LEVELS)
def test_shading_with_edited_scene(rt, oracle_mod, cuda, levels):
    from test_gpu_shade import _check

    s = start(rt, oracle_mod, levels, scene=True)
    tree, scene = s.trees
    sun = rt.sun_dir()
    seen = {"mirror": 0, "glass": 0, "water": 0, "top": 0}
    for stage in synced(s):
        for ci, cam in enumerate(SHADE_CAMS):
            org, dn = cam_at(rt, s, cam)
            label = "shade levels %d stage %d cam %d" % (levels, stage, ci)
            ref = s.T.shade_frame(org, dn, W, H, 300, sun, liquid=True)
            rgba, hits = tree.shade_frame(org, dn, W, H, 300, sun=sun, with_hits=True, scene=scene)
            g = rt.decode_hits(hits)
            _check(rgba, ref, g["hit"], label)
            bare = tree.shade_frame(org, dn, W, H, 300, sun=sun, scene=scene)
            _check(bare, ref, g["hit"], label + ", no records")
            assert cuda.equal(bare, rgba), label + ": the image without hit records differs"
            if stage in (7, 10):  # what the cameras are there for (the mirror is deleted at stage 8): primary hits, by the oracle
                prim = s.T.cast_frame(org, dn, W, H, 300)
                assert prim["rc"] == 0
                fl = prim["flags"][prim["hit"] != 0]
                seen["mirror"] += int((fl == (es.F_MIRROR | 1)).sum())
                seen["glass"] += int((fl == (es.F_GLASS | 1)).sum())
                seen["water"] += int((ref != s.T.shade_frame(org, dn, W, H, 300, sun)).any(1).sum())
            if stage == 12 and cam is ABOVE:
                prim = s.T.cast_frame(org, dn, W, H, 300)
                seen["top"] = int(((prim["pos"] == (s.ox + 5, es.ABOVE_Y, 5)).all(1) & (prim["hit"] != 0)).sum())
        no_guard(rt, tree)
    print("shade levels %d: primary hits on the mirror %d, on glass %d, pixels the water changes %d" % (levels, seen["mirror"], seen["glass"], seen["water"]))
    assert seen["mirror"] > 500 and seen["glass"] > 100 and seen["water"] > 20
    assert levels == 3 or seen["top"] > 100  # the voxel that raises the top row, seen from above it


# ---------------------------------------------------------------------------------------------------------------- idle --
@pytest.mark.parametrize("levels", LEVELS)
def test_idle_sync_changes_nothing(rt, oracle_mod, cuda, levels):
    s = start(rt, oracle_mod, levels)
    tree = s.trees[0]

    def state(stage):
        org, d, _ = readback_rays(s, stage)
        out = tree.cast_rays(cuda.from_numpy(np.tile(d, (len(org), 1))).cuda(), cuda.from_numpy(org).cuda(), steps=1)
        res = [out[k].view(cuda.int32).cpu().numpy() for k in ("pos_steps", "t", "info")]
        for kind in sorted(CAMS):
            org_, dn = cam_at(rt, s, CAMS[kind])
            fr = tree.cast_frame(org_, dn, W, H, 300)
            res += [fr[k].view(cuda.int32).cpu().numpy() for k in ("pos_steps", "t", "info")]
        return res + [np.asarray(x) for x in device_tables(tree)]

    for stage in synced(s):
        before = state(stage)
        nodes = tree.info().n_nodes
        tree.sync()
        after = state(stage)
        assert tree.info().n_nodes == nodes
        assert len(before) == len(after) and all(np.array_equal(a, b) for a, b in zip(before, after)), (levels, stage)
        no_guard(rt, tree)
