"""Directed shading: the bounces of svo_shade_rays, aimed at instead of hoped for.

The shading pass runs a straight trace on the camera's sign octant and hands its state to a bouncing trace at the first
mirror or refractive block (svo_cast_kernel.h, k_cast SHADE); the bouncing trace undoes a crossing and flips an axis at a
mirror, rebuilds deltaPos from the shader's origin-based exact position at the first refractive block, walks uniform
refractive regions and bricks without lookups (svo_trace.h, REFLECT).  One voxel off anywhere moves where a reflected or
bent ray ends.  Every battery here casts chosen rays on the hall (tests/hall.py: mirrors, glass and water as voxels, 4^3 and
16^3 regions, inside one another and across the wrap) and compares with the oracle's shading of the same explicit rays
(oracle.c orc_shade_rays: low_res.frag:170-240, 319-391 restated):

  records   every field bit-exact, t included, no ray left out (test_gpu_parity.compare);
  colours   lit pixels bit-exact, sky pixels within test_gpu_shade.SKY_ATOL, split by the ORACLE's hit (test_gpu_shade._check);
  guard     no ray ends on the progress guard.

What the batteries exercise is decided from the oracle alone, in tests/test_hall_host.py (which runs without a GPU); each
test here prints the oracle's event counts of what it cast."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hall  # noqa: E402
from test_gpu_parity import compare  # noqa: E402
from test_gpu_shade import _check  # noqa: E402

pytestmark = pytest.mark.gpu

TIME = 1.25
BUDGETS = (1, 2, 3, 40, 300)


@pytest.fixture(scope="module")
def cuda():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


@pytest.fixture(scope="module")
def world(rt, oracle_mod, cuda):
    """(solid Tree, VIEW_ALL scene Tree, oracle Tree) of the hall, built and uploaded once and left unchanged"""
    w, T = hall.hall(rt, oracle_mod)
    return w.build().upload(0), w.build(rt.VIEW_ALL).upload(0), T


@pytest.fixture(scope="module")
def frames(oracle_mod):
    """{pose name: (pose, origins, dirs, cam, ppx, ppy)}: the oracle's pixel directions of every pose's 96 x 64 frame"""
    return {p[0]: (p,) + hall.frame_rays(oracle_mod, p) for p in hall.FRAME_POSES}


def counts(label, r):
    c = hall.event_counts(r)
    keys = ("refl1", "refl2", "refl3+", "refl10+", "bent", "liq_bend", "bend_then_refl", "refl_then_bend", "tints8+", "hit_after_event",
            "miss_after_event", "last_step_mirror", "last_step_refractive")
    print("%-28s %5d rays | %s | bend faces %s" % (label, len(r["hit"]), " ".join("%s=%d" % (k, c[k]) for k in keys),
                                                  "/".join(str(c["bend" + f]) for f in ("+x", "-x", "+y", "-y", "+z", "-z"))))


def no_guard(solid, scene):
    assert solid.guard_trips() == 0 and scene.guard_trips() == 0


def check(rt, pal_tree, rgba, out, ref, label, palette=None):
    """one launch against the oracle: the records (when the launch wrote them) and the colours (palette: compare's)"""
    if out is not None:
        compare(rt, pal_tree, out, ref, label, palette)
        assert (out["pos_steps"][:, 3] >= 0).all(), label
    _check(rgba, ref["rgba"], ref["hit"], label)


def shade_desc(rt, torch, solid, desc, n, records, scene=None, time=0.0, **kw):
    """the shading pass over desc's n rays: (rgba, hit records or None)"""
    rgba = torch.empty((n, 4), dtype=torch.float32, device="cuda")
    out = rt.Tree.alloc_hits(n, 0) if records else None
    solid.shade(desc, rgba, out=out, scene=scene, time=time, **kw)
    torch.cuda.synchronize()
    return rgba, out


def explicit_desc(rt, go, gd, steps, flags):
    d = rt.CastDesc()
    d.ray_dirs, d.ray_origins, d.n_rays, d.steps, d.flags = gd.data_ptr(), go.data_ptr(), gd.shape[0], steps, flags
    return d


# -------------------------------------------------------------------------------------------------- A: explicit rays --
@pytest.mark.parametrize("name", ["room", "mirrors", "glass", "water", "wrap", "budget", "singles"])
def test_explicit_rays(rt, cuda, world, name):
    """A: the shading pass in explicit mode (ray_dirs / ray_origins: the generic-sign instances) over one set of
    hall.batteries() at every budget: with the scene at two times, without it (water passes unseen), under every flag that
    must change nothing, and without hit records"""
    torch = cuda
    solid, scene, T = world
    org, dirs = hall.batteries()[name]
    n = len(org)
    go, gd = torch.from_numpy(org).cuda(), torch.from_numpy(dirs).cuda()
    sun = rt.sun_dir()
    for S in BUDGETS:
        wet = {tm: T.shade_rays(org, dirs, S, sun, liquid=True, time=tm) for tm in (0.0, TIME)}
        dry = T.shade_rays(org, dirs, S, sun, liquid=False)
        counts("A %s S=%d wet" % (name, S), wet[TIME])
        for tm in (0.0, TIME):
            rgba, out = shade_desc(rt, torch, solid, explicit_desc(rt, go, gd, S, 0), n, True, scene=scene, time=tm)
            check(rt, scene, rgba, out, wet[tm], "A %s S=%d t=%g" % (name, S, tm))
        for flags in (rt.CAST_ITERATIVE, rt.CAST_NO_CEILINGS, rt.CAST_SEGMENTS, rt.CAST_WIDE_ADDR):
            rgba, out = shade_desc(rt, torch, solid, explicit_desc(rt, go, gd, S, flags), n, True, scene=scene, time=TIME)
            check(rt, scene, rgba, out, wet[TIME], "A %s S=%d flags=%d" % (name, S, flags))
            rgba, out = shade_desc(rt, torch, solid, explicit_desc(rt, go, gd, S, flags), n, True)
            check(rt, solid, rgba, out, dry, "A %s S=%d dry flags=%d" % (name, S, flags))
        rgba, out = shade_desc(rt, torch, solid, explicit_desc(rt, go, gd, S, 0), n, True)
        check(rt, solid, rgba, out, dry, "A %s S=%d dry" % (name, S))
        rgba, _ = shade_desc(rt, torch, solid, explicit_desc(rt, go, gd, S, 0), n, False, scene=scene, time=TIME)
        check(rt, scene, rgba, None, wet[TIME], "A %s S=%d colours only" % (name, S))
        rgba, _ = shade_desc(rt, torch, solid, explicit_desc(rt, go, gd, S, 0), n, False)
        check(rt, solid, rgba, None, dry, "A %s S=%d dry colours only" % (name, S))
    no_guard(solid, scene)


# --------------------------------------------------------------------------------------------------------- B: frames --
def frame_flags(rt):
    return (0, rt.CAST_ITERATIVE, rt.CAST_NO_CEILINGS, rt.CAST_NO_OCTANT, rt.CAST_SEGMENTS, rt.CAST_WIDE_ADDR)


def frame_desc(rt, frame, steps, flags=0):
    pose, _, _, cam, ppx, ppy = frame
    return rt.Tree.frame_desc(pose[1], cam, hall.FRAME_W, hall.FRAME_H, steps, ppx=ppx, ppy=ppy, flags=flags)


@pytest.mark.parametrize("name", [p[0] for p in hall.FRAME_POSES])
def test_frames(rt, cuda, world, frames, name):
    """B: 96 x 64 frames from inside the mirror room, in front of the uniform mirrors, under the water cube, beside the pool
    and through the wrap, at S = 300 and 40: the reference is the oracle's shading of the frame's pixel directions; every
    flag that must change nothing, with records (the instances that walk every ray's whole budget) and without (the
    no-record instances, whose rays may escape), with the scene and without it"""
    torch = cuda
    solid, scene, T = world
    f = frames[name]
    _, org, dirs = f[0], f[1], f[2]
    n = len(org)
    sun = rt.sun_dir()
    for S in (300, 40):
        wet = T.shade_rays(org, dirs, S, sun, liquid=True, time=TIME)
        dry = T.shade_rays(org, dirs, S, sun, liquid=False)
        counts("B %s S=%d wet" % (name, S), wet)
        counts("B %s S=%d dry" % (name, S), dry)
        for flags in frame_flags(rt):
            d = frame_desc(rt, f, S, flags)
            assert rt.Tree.count(d) == n
            for records in (True, False):
                rgba, out = shade_desc(rt, torch, solid, d, n, records, scene=scene, time=TIME)
                check(rt, scene, rgba, out, wet, "B %s S=%d flags=%d records=%d" % (name, S, flags, records))
                rgba, out = shade_desc(rt, torch, solid, d, n, records)
                check(rt, solid, rgba, out, dry, "B %s S=%d dry flags=%d records=%d" % (name, S, flags, records))
    no_guard(solid, scene)


# -------------------------------------------------------------------------------------------- C: diagnostic instances --
@pytest.mark.parametrize("name", ["room_fractional", "pool_wide"])
def test_stats_instances(rt, cuda, world, frames, name):
    """C: the STATS and TIMELINE instances run one bouncing trace from the origin where the plain launch runs two traces
    with a handoff: the same image, and the frame's bend and tint counters are the oracle's sums of reflections + bends and
    of refractive blocks passed"""
    torch = cuda
    solid, scene, T = world
    f = frames[name]
    org, dirs = f[1], f[2]
    n = len(org)
    for S in (300, 40):
        ref = T.shade_rays(org, dirs, S, rt.sun_dir(), liquid=True, time=TIME)
        plain, _ = shade_desc(rt, torch, solid, frame_desc(rt, f, S), n, False, scene=scene, time=TIME)
        for flag in (rt.CAST_STATS, rt.CAST_TIMELINE):
            d = frame_desc(rt, f, S, flag)
            st = torch.zeros(rt.STATS_HEADER + 2 * rt.Tree.blocks(d) + n, dtype=torch.int64, device="cuda")
            d.stats = st.data_ptr()
            for records in (False, True):
                st.zero_()
                rgba, out = shade_desc(rt, torch, solid, d, n, records, scene=scene, time=TIME)
                check(rt, scene, rgba, out, ref, "C %s S=%d flag=%d records=%d" % (name, S, flag, records))
                assert torch.equal(rgba, plain), (name, S, flag, records)
                if flag == rt.CAST_STATS:
                    v = dict(zip(rt.STAT_NAMES, st[:len(rt.STAT_NAMES)].cpu().tolist()))
                    print("C %s S=%d: bends %d tints %d" % (name, S, v["bends"], v["tints"]))
                    assert v["rays"] == n and v["no_progress"] == 0
                    assert v["bends"] == int((ref["nrefl"] + ref["bent"]).sum()) > 0
                    assert v["tints"] == int(ref["tints"].sum()) > 0
        if f[0][3] is None:  # Tree.shade_stats itself (the reference's plane, time 0): its per-pixel means
            r0 = T.shade_rays(org, dirs, S, rt.sun_dir(), liquid=True, time=0.0)
            v = solid.shade_stats(f[0][1], f[3], hall.FRAME_W, hall.FRAME_H, S, scene=scene)
            assert round(v["bends"] * n) == int((r0["nrefl"] + r0["bent"]).sum()) and round(v["tints"] * n) == int(r0["tints"].sum())
            assert v["no_progress"] == 0
    no_guard(solid, scene)


# --------------------------------------------------------------------------------------------------------- D: layout --
def shard_pixels(W, H, start, step):
    """record order of a shard: the pixels of tile rows start, start + step, ... (8 pixel rows each)"""
    py = np.concatenate([np.arange(t * 8, min(H, t * 8 + 8)) for t in range(start, (H + 7) // 8, step)])
    return (py[:, None] * W + np.arange(W)[None, :]).ravel()


def test_multi_frame_and_shards(rt, oracle_mod, cuda, world):
    """D: one launch of three frame origins (integral, half-integral, fractional, inside the mirror room) is the three single
    frames, whole and as the shard of tile rows 1, 4, ...: records and colours, each against the oracle per frame"""
    torch = cuda
    solid, scene, T = world
    W, H, S = 72, 44, 300
    origins = [(538.0, 58.0, 550.0), (538.5, 58.5, 550.5), (538.3, 58.7, 550.9)]
    pose = ("layout", origins[0], (0.9, -0.7, -0.8), None)
    _, dirs, cam, ppx, ppy = hall.frame_rays(oracle_mod, pose, W, H)
    refs = [T.shade_rays(np.tile(np.array(o, np.float32), (W * H, 1)), dirs, S, rt.sun_dir(), liquid=True, time=TIME) for o in origins]
    for start, step in ((0, 1), (1, 3)):
        pix = shard_pixels(W, H, start, step)
        part = [{k: v[pix] for k, v in r.items()} for r in refs]
        cat = {k: np.concatenate([p[k] for p in part]) for k in part[0]}
        counts("D shard %d/%d" % (start, step), cat)
        d = rt.Tree.frame_desc(origins[0], cam, W, H, S, tile_row_start=start, tile_row_step=step, frame_origins=origins)
        n = rt.Tree.count(d)
        assert n == 3 * len(pix)
        for records in (True, False):
            rgba, out = shade_desc(rt, torch, solid, d, n, records, scene=scene, time=TIME)
            check(rt, scene, rgba, out, cat, "D multi shard %d/%d records=%d" % (start, step, records))
            for i, o in enumerate(origins):
                d1 = rt.Tree.frame_desc(o, cam, W, H, S, tile_row_start=start, tile_row_step=step)
                r1, o1 = shade_desc(rt, torch, solid, d1, len(pix), records, scene=scene, time=TIME)
                check(rt, scene, r1, o1, part[i], "D single %d shard %d/%d records=%d" % (i, start, step, records))
                sl = slice(i * len(pix), (i + 1) * len(pix))
                assert torch.equal(rgba[sl], r1), (i, start, step, records)
                if records:
                    for k in out:
                        assert torch.equal(out[k][sl], o1[k]), (i, start, step, k)
    no_guard(solid, scene)


# -------------------------------------------------------------------------------------------------------- E: look-at --
def test_look_at_after_bounces(rt, cuda, world, frames):
    """E: lookingAtBlock (low_res.frag:340-347 compares every ray's END voxel) on the end voxel of a reflected hit, of a bent
    miss, and on a mirror voxel that rays hit on their last step: the image is the oracle's with the same look-at, with and
    without records, and the oracle highlights pixels"""
    torch = cuda
    solid, scene, T = world
    sun = rt.sun_dir()
    inside = lambda r: ((r["pos"] >= 0) & (r["pos"] < hall.E)).all(1)  # noqa: E731
    cases = [("reflected hit", "room_wide", 300, lambda r: (r["nrefl"] > 0) & (r["hit"] != 0)),
             ("bent miss", "wrap", 40, lambda r: (r["bent"] != 0) & (r["hit"] == 0) & inside(r)),
             ("bent miss in the room", "room_fractional", 40, lambda r: (r["bent"] != 0) & (r["hit"] == 0)),
             ("mirror on the last step", "room_wide", 40, lambda r: (r["hit"] != 0) & (r["steps"] == 0) & ((r["flags"] & 7) == 3))]
    for label, name, S, pick in cases:
        f = frames[name]
        org, dirs = f[1], f[2]
        n = len(org)
        base = T.shade_rays(org, dirs, S, sun, liquid=True, time=TIME)
        idx = np.nonzero(pick(base))[0]
        assert len(idx) > 0, label
        look = tuple(int(v) for v in base["pos"][idx[len(idx) // 2]])
        ref = T.shade_rays(org, dirs, S, sun, look_at=look, liquid=True, time=TIME)
        lit = (ref["pos"] == np.array(look)).all(1)
        print("E %s: look-at %s, %d pixels highlighted, %d change colour" % (label, look, lit.sum(), (ref["rgba"] != base["rgba"]).any(1).sum()))
        assert lit.sum() > 0 and (ref["rgba"] != base["rgba"]).any(1).sum() > 0
        for flags in (0, rt.CAST_NO_OCTANT):
            for records in (True, False):
                rgba, out = shade_desc(rt, torch, solid, frame_desc(rt, f, S, flags), n, records, scene=scene, time=TIME, look_at=look)
                check(rt, scene, rgba, out, ref, "E %s flags=%d records=%d" % (label, flags, records))
    no_guard(solid, scene)


# ------------------------------------------------------------------------------------------------------------ F: sun --
@pytest.mark.parametrize("name", ["room_pillar", "pool_wide"])
def test_suns_and_shadows(rt, cuda, world, frames, name):
    """F: shadow rays that start next to mirrors, glass and water (they walk the solid tree: water passes unseen): the
    reference sun, a sun in another octant, one from below, and no shadow budget"""
    torch = cuda
    solid, scene, T = world
    f = frames[name]
    org, dirs = f[1], f[2]
    n = len(org)
    for sun, shadow in ((rt.sun_dir(), 75), (tuple(rt.normalize((-1.0, 0.5, -0.2))), 75), (tuple(rt.normalize((0.3, -0.8, 0.5))), 75),
                        (rt.sun_dir(), 0), (rt.sun_dir(), 3)):
        ref = T.shade_rays(org, dirs, 300, sun, shadow_steps=shadow, liquid=True, time=TIME)
        shadowless = T.shade_rays(org, dirs, 300, sun, shadow_steps=0, liquid=True, time=TIME)
        print("F %s sun %s shadow %d: %d pixels darkened by shadow rays" % (name, np.round(sun, 2).tolist(), shadow,
                                                                          (ref["rgba"] != shadowless["rgba"]).any(1).sum()))
        for flags in (0, rt.CAST_NO_OCTANT):
            for records in (True, False):
                rgba, out = shade_desc(rt, torch, solid, frame_desc(rt, f, 300, flags), n, records, scene=scene, time=TIME, sun=sun,
                                       shadow_steps=shadow)
                check(rt, scene, rgba, out, ref, "F %s sun=%s shadow=%d flags=%d records=%d" % (name, sun, shadow, flags, records))
    no_guard(solid, scene)
