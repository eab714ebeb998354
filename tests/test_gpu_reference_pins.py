"""The GPU casts and device lookups against the reference's own recorded answers, with no oracle in between.

tests/golden/pins_R.npz and pins_P.npz (tests/pin_cases.py, oracle/REFERENCE_PINS.md) hold ray batteries, pixel fans and
lookups on the reference application's world (R) and the pin world (P, tests/pin_world.py), answered by the reference's
compiled tetrahexa_tree.cpp / world_gen.cpp / ray_caster.cpp.  Here both worlds are built as device trees and every
recorded ray goes through the cast kernel's instances: pos, lastPos (pos minus the step `info` names), stepsLeft, hit,
and the hit material's palette flags and colour must equal the record, every ray, bit for bit.  castRayFromCam leaves
lastPos without a value at a budget of 0, so it is not compared there.  Nothing here reads the oracle."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pin_cases as pc  # noqa: E402
from test_gpu_directed_rays import frame_flags  # noqa: E402

pytestmark = pytest.mark.gpu

WORLDS = ("R", "P")
N = pc.FRAME_W * pc.FRAME_H


@pytest.fixture(scope="module")
def cuda():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


@pytest.fixture(scope="module")
def pinned(rt, cuda):
    """{world: (uploaded Tree, inputs, records)}, built once and left unchanged"""
    res = {}
    for w in WORLDS:
        inp, rec, _, _ = pc.load(w)
        res[w] = (pc.product_world(rt, w).build().upload(0), inp, rec)
    return res


def cast_flags(rt):
    return tuple(frame_flags(rt)) + (rt.CAST_WIDE_ADDR,)


def palette(tree):
    pal = tree.palette()
    return np.array([p[0] for p in pal], np.uint32), np.array([p[1] for p in pal], np.uint64)


def take(rec, name, idx):
    return {k: rec[name + "_" + k][idx] for k in ("pos", "last", "steps", "flags", "color")}


def compare(rt, tree, out, ref, budget, label):
    """device hit records against the reference's records `ref` (pos, last, steps, and flags / color of the block at pos)"""
    g = rt.decode_hits(out)
    pf, pcol = palette(tree)
    budget = np.broadcast_to(np.asarray(budget), (len(ref["steps"]),))
    assert len(g["hit"]) == len(ref["steps"]), label
    bad = np.nonzero((g["pos"] != ref["pos"]).any(1))[0]
    assert len(bad) == 0, "%s: pos differs at %d rays, first %s gpu=%s reference=%s" % (label, len(bad), bad[:5], g["pos"][bad[:3]], ref["pos"][bad[:3]])
    assert np.array_equal(g["steps"], ref["steps"]), label
    hit = pc.hit_of(ref["flags"], ref["color"], budget)
    assert np.array_equal(g["hit"], hit), label
    stepped = budget > 0
    assert np.array_equal(g["last_pos"][stepped], ref["last"][stepped]), label
    mat = g["material"][hit]
    assert (mat > 0).all() and np.array_equal(pf[mat], ref["flags"][hit]) and np.array_equal(pcol[mat], ref["color"][hit]), label
    return hit


@pytest.mark.parametrize("world", WORLDS)
def test_explicit_batteries(rt, cuda, pinned, world):
    """the recorded ray battery in explicit mode, one launch per budget and instance"""
    tree, inp, rec = pinned[world]
    tree.guard_trips(reset=True)
    hits = 0
    for b in np.unique(inp["ray_budget"]):
        idx = np.nonzero(inp["ray_budget"] == b)[0]
        go = cuda.from_numpy(np.ascontiguousarray(inp["ray_org"][idx])).cuda()
        gd = cuda.from_numpy(np.ascontiguousarray(inp["ray_dir"][idx])).cuda()
        ref = take(rec, "ray", idx)
        for flags in cast_flags(rt):
            out = tree.cast_rays(gd, go, steps=int(b), flags=flags)
            hit = compare(rt, tree, out, ref, int(b), "%s explicit S=%d flags=%d" % (world, b, flags))
            assert (out["pos_steps"][:, 3] >= 0).all()
        hits += int(hit.sum())
    print("%s: %d rays, %d reference hits" % (world, len(inp["ray_budget"]), hits))
    assert hits > 200 and tree.guard_trips() == 0


@pytest.mark.parametrize("world", WORLDS)
def test_fans_in_frame_mode(rt, cuda, pinned, world):
    """the recorded 64 x 48 fans in frame mode: the integral and half-integral cameras take the linear instances (8-byte
    wire records), the fractional one the segment instance; the product's pixel directions are the recorded ones"""
    tree, inp, rec = pinned[world]
    tree.guard_trips(reset=True)
    ppx, ppy = (float(v) for v in inp["frame_pp"])
    assert (ppx, ppy) == rt.proj_plane(pc.FRAME_W, pc.FRAME_H)
    kinds, hits = [], 0
    for k, (cam, d, S) in enumerate(zip(inp["frame_cam"], inp["frame_dir"], inp["frame_budget"])):
        assert np.array_equal(rt.normalize(pc.CAMERAS[world][k // len(pc.FRAME_STEPS)][1]).view(np.uint32), d.view(np.uint32))
        assert pc.dir_checksum(rt.pixel_dirs(d, pc.FRAME_W, pc.FRAME_H, ppx, ppy).reshape(-1, 3)) == rec["frame_dirsum"][k]
        ref = take(rec, "frame", np.arange(k * N, (k + 1) * N))
        desc = rt.Tree.frame_desc(cam, d, pc.FRAME_W, pc.FRAME_H, int(S), ppx=ppx, ppy=ppy)
        kinds.append(tree.wire_bytes(desc))
        for flags in cast_flags(rt):
            out = tree.cast_frame(cam, d, pc.FRAME_W, pc.FRAME_H, int(S), ppx=ppx, ppy=ppy, flags=flags)
            hit = compare(rt, tree, out, ref, int(S), "%s fan %d S=%d flags=%d" % (world, k, S, flags))
            assert (out["pos_steps"][:, 3] >= 0).all()
        hits += int(hit.sum())
    assert 0.1 < hits / len(rec["frame_steps"]) < 0.9
    assert kinds == [8, 8, 8, 8, 12, 12]  # integral, half-integral, fractional camera, two budgets each
    assert tree.guard_trips() == 0


@pytest.mark.parametrize("world", WORLDS)
def test_cast_ray_from_cam(rt, cuda, pinned, world):
    """svo_cast_ray_from_cam on 48 recorded rays spread over the battery (every budget among them)"""
    tree, inp, rec = pinned[world]
    order = np.argsort(inp["ray_budget"], kind="stable")
    pick = order[np.linspace(0, len(order) - 1, 48).astype(int)]
    assert len(set(inp["ray_budget"][pick].tolist())) >= len(pc.BUDGETS)
    hits = 0
    for i in pick:
        b = int(inp["ray_budget"][i])
        (pos, last, steps), blk = tree.cast_ray_from_cam(inp["ray_org"][i], inp["ray_dir"][i], b)
        assert pos == tuple(rec["ray_pos"][i]) and steps == rec["ray_steps"][i], (world, i)
        assert b == 0 or last == tuple(rec["ray_last"][i]), (world, i)
        if pc.hit_of(rec["ray_flags"][i], rec["ray_color"][i], b):
            assert (blk[0], blk[1]) == (rec["ray_flags"][i], rec["ray_color"][i]), (world, i)
            hits += 1
    assert hits >= 5 and tree.guard_trips() == 0


READ_BOXES = {"R": [((-4, 0, -4), (208, 76, 208))],                           # (origin x y z, shape nz ny nx): the terrain and a margin
              "P": [((256, 0, 256), (256, 330, 256)), ((-8, -8, -8), (16, 16, 16)), ((496, 700, 496), (8, 324, 8))]}  # cavern; wrap corners; tower top


@pytest.mark.parametrize("world", WORLDS)
def test_device_lookups(rt, cuda, pinned, world):
    """svo_tree_get_blocks at every recorded probe and svo_tree_read_volume over boxes that hold most of them: the stored
    palette entry is the reference's getBlock; LIQUID and empty read as id 0 in the cast tree"""
    tree, inp, rec = pinned[world]
    pf, pcol = palette(tree)
    empty = (rec["probe_color"] == pc.EMPTY) | ((rec["probe_flags"] & 0x10) != 0)

    def check(ids, sel, label):
        assert np.array_equal(ids == 0, empty[sel]), label
        st = ids != 0
        assert np.array_equal(pf[ids[st]], rec["probe_flags"][sel][st]) and np.array_equal(pcol[ids[st]], rec["probe_color"][sel][st]), label

    check(tree.get_blocks(inp["probes"]), np.arange(len(empty)), world + " get_blocks")
    seen = np.zeros(len(empty), bool)
    for lo, shape in READ_BOXES[world]:
        vol = tree.read_volume(lo, shape).cpu().numpy().view(np.uint16)
        rel = (inp["probes"].astype(np.int64) - np.array(lo)) & (pc.E - 1)
        sel = np.nonzero((rel < np.array(shape)[::-1]).all(1))[0]
        check(vol[rel[sel, 2], rel[sel, 1], rel[sel, 0]].astype(np.int64), sel, "%s read_volume %s" % (world, lo))
        seen[sel] = True
    print("%s: %d of %d probes inside the boxes read, %d of them stored" % (world, seen.sum(), len(seen), (seen & ~empty).sum()))
    assert seen.sum() > 1500 and (seen & ~empty).sum() > 300
