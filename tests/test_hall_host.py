"""The hall fixture (tests/hall.py) itself, on the CPU: the product's World and linearised trees hold the blocks the oracle's
tree holds; the oracle's explicit-ray shading entry (shade_rays) is its frame entry (shade_frame) ray by ray; and the
batteries tests/test_gpu_directed_shading.py casts produce, by the oracle's records alone, every event class of the
shading pass — so the GPU tests cannot pass by seeing nothing."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hall  # noqa: E402

EMPTY = np.uint64(0xFFFFFFFFFFFFFFFF)
FACES = ("+x", "-x", "+y", "-y", "+z", "-z")


@pytest.fixture(scope="module")
def pair(rt, oracle_mod):
    return hall.hall(rt, oracle_mod)


@pytest.fixture(scope="module")
def results(rt, pair):
    """the oracle's shade_rays over every battery at S = 300, liquid on: computed once, left unchanged"""
    _, T = pair
    return {k: T.shade_rays(o, d, 300, rt.sun_dir(), liquid=True, time=1.25) for k, (o, d) in hall.batteries().items()}


def test_block_parity(rt, pair):
    """12,000 seeded voxels in and next to every structure: World.get_block is the oracle's getBlock; the solid tree's palette
    entry is the oracle's block with liquid taken as empty (castRayFromCam's view), the VIEW_ALL tree's is the block itself"""
    w, T = pair
    pts = hall.probe_points(12000)
    ref = [T.get_block(int(x), int(y), int(z)) for x, y, z in pts]
    rf = np.array([r[0] for r in ref], np.uint32)
    rc = np.array([r[1] for r in ref], np.uint64)
    wf, wc, _ = w.get_blocks(pts)
    assert np.array_equal(wc, rc)
    assert np.array_equal(wf[rc != EMPTY], rf[rc != EMPTY])
    for i in range(0, len(pts), 97):  # (the unbatched call as well)
        f, c, _ = w.get_block(*[int(v) for v in pts[i]])
        assert c == rc[i] and (c == EMPTY or f == rf[i])
    liquid = (rc != EMPTY) & ((rf & 0x10) != 0)
    for view, gone in ((rt.VIEW_SOLID, liquid), (rt.VIEW_ALL, np.zeros(len(pts), bool))):
        tree = w.build(view)
        ids = tree.get_blocks(pts)
        pal = tree.palette()
        pf = np.array([p[0] for p in pal], np.uint32)
        pc = np.array([p[1] for p in pal], np.uint64)
        stored = (rc != EMPTY) & ~gone
        assert np.array_equal(ids != 0, stored), view
        assert np.array_equal(pc[ids][stored], rc[stored]) and np.array_equal(pf[ids][stored], rf[stored]), view
    stored = rc != EMPTY
    assert 0.2 < stored.mean() < 0.8  # the probe sees both
    kinds = set(hall.ident(rc[stored]).tolist())
    assert kinds == set(hall.ALL_IDS), set(hall.ALL_IDS) ^ kinds  # every put is seen, under its own colour
    want = {hall.C_WALL: 3, hall.C_MIRROR16: 3, hall.C_MIRROR4: 3, hall.C_G16_MIRROR: 3, hall.C_POOL_MIRROR: 3, hall.C_GLASS16: 5,
            hall.C_GLASS4: 5, hall.C_PANE_X: 5, hall.C_PANE_Y: 5, hall.C_PANE_Z: 5, hall.C_POOL_GLASS: 5, hall.C_WRAP_GLASS: 5,
            hall.C_CUBE: 0x15, hall.C_POOL: 0x15, hall.C_ROOM_WATER: 0x15, hall.C_WRAP_WATER: 0x15, hall.C_FLOOR: 1, hall.C_PILLAR: 1}
    for cid, flags in want.items():
        assert set(rf[rc == hall.colour(cid)].tolist()) == {flags}, cid


POSES = [((543.5, 50.5, 541.5), (0.7, -0.2, 0.5)),      # inside the mirror room
         ((640.5, 52.5, 618.5), (0.1, -0.6, 1.0))]      # beside the pool, looking down into it


@pytest.mark.parametrize("pose", range(len(POSES)))
def test_shade_rays_is_shade_frame(rt, oracle_mod, pair, pose):
    """the new entry cannot drift from the old one: on the pixel directions of a 48 x 32 frame shade_rays returns exactly
    shade_frame's rgba, liquid on and off, with and without a look-at voxel (the end voxel of a ray that had an event)"""
    _, T = pair
    org, cd = POSES[pose]
    cam = oracle_mod.normalize(cd)
    W, H, S = 48, 32, 300
    ppx, ppy = oracle_mod.proj_plane(W, H)
    dirs = np.array([oracle_mod.pixel_dir(cam, ppx, ppy, W, H, i % W, i // W) for i in range(W * H)], np.float32)
    orgs = np.tile(np.array(org, np.float32), (W * H, 1))
    sun = rt.sun_dir()
    for liquid in (False, True):
        base = T.shade_rays(orgs, dirs, S, sun, liquid=liquid, time=0.75)
        ev = np.nonzero((base["nrefl"] > 0) | (base["bent"] != 0))[0]
        assert len(ev) >= 20  # (the same floor as the coverage classes below)
        looks = [None, tuple(int(v) for v in base["pos"][ev[len(ev) // 2]])]
        for look in looks:
            a = T.shade_rays(orgs, dirs, S, sun, look_at=look, liquid=liquid, time=0.75)
            b = T.shade_frame(org, cam, W, H, S, sun, look_at=look, liquid=liquid, time=0.75)
            assert np.array_equal(a["rgba"].view(np.uint32), b.view(np.uint32)), (pose, liquid, look)
            if look is not None:
                assert (a["rgba"] != base["rgba"]).any(1).sum() > 0  # the highlight shows
        # one thread or many, the same records
        c = T.shade_rays(orgs, dirs, S, sun, liquid=liquid, time=0.75, nthreads=1)
        for k in base:
            assert np.array_equal(base[k], c[k], equal_nan=base[k].dtype.kind == "f"), k


def test_battery_coverage(results):
    """by the oracle's records at S = 300, at least 20 rays of every event class over hall.batteries()"""
    total = {}
    for name, r in results.items():
        c = hall.event_counts(r)
        print("%-8s %5d rays: %s" % (name, len(r["hit"]), " ".join("%s=%d" % kv for kv in c.items())))
        for k, v in c.items():
            total[k] = total.get(k, 0) + v
    n = sum(len(r["hit"]) for r in results.values())
    assert n < 10000
    classes = ["refl1", "refl2", "refl3+", "refl10+", "bend_then_refl", "refl_then_bend", "tints8+", "hit_after_event",
               "miss_after_event", "last_step_mirror", "last_step_refractive"]
    classes += ["bend" + f for f in FACES] + ["liq_bend" + f for f in FACES]
    for k in classes:
        assert total[k] >= 20, (k, total[k])


def test_origin_and_direction_classes():
    """origins: integral, half-integral, generic fractional and one extent down (negative, trunc != floor) in every sampled
    set; directions: the tie set of test_gpu_directed_rays among seeded normals"""
    from test_gpu_directed_rays import tie_directions

    ties = {d.tobytes() for d in tie_directions()}
    B = hall.batteries()
    for name in ("room", "mirrors", "glass", "water", "wrap"):
        o, d = B[name]
        integral = (o == np.floor(o)).all(1)
        half = (o - np.floor(o) == 0.5).all(1)
        down = o[:, 1] < 0  # (every y lies below the extent; the wrap set's x may stay positive one extent down)
        assert (o[down][:, 1:] < 0).all() and (o[~down] >= 0).all(), name
        generic = ~integral & ~half & ~down & (o != np.floor(o)).all(1)
        for cls in (integral & ~down, half, generic, down, down & ~integral):
            assert cls.sum() >= len(o) // 10, name
    tied = sum(x.tobytes() in ties for name in ("room", "glass", "water") for x in B[name][1])
    assert tied >= 700


def test_directed_singles(rt, pair):
    """the built rays do what they were built for, by the oracle"""
    _, T = pair
    sun = rt.sun_dir()
    sg = hall.singles()
    run = lambda name, S: T.shade_rays(sg[name][0], sg[name][1], S, sun, liquid=True, time=1.25)  # noqa: E731
    # inside the uniform mirror: a reflection at every step but the last, which is the hit with no budget left
    r = run("inside_mirror", 300)
    assert r["nrefl"].tolist() == [299, 299, 299] and (r["hit"] == 1).all() and (r["steps"] == 0).all()
    assert (hall.ident(r["color"]) == hall.C_MIRROR16).all()
    # one voxel in front of each face: S = 1 ends on the block (no budget left: no event), S = 2 and 3 reflect / bend
    o, d = sg["faces"]
    assert len(o) == 24
    face = np.array([2 * a + (s < 0) for _ in range(2) for a in range(3) for s in (1, -1) for _ in range(2)])
    mirror = np.arange(24) < 12
    r = run("faces", 1)
    assert (r["hit"] == 1).all() and (r["steps"] == 0).all() and (r["nrefl"] == 0).all() and (r["bent"] == 0).all()
    assert (hall.ident(r["color"]) == np.where(mirror, hall.C_MIRROR16, hall.C_GLASS16)).all()
    for S in (2, 3):
        r = run("faces", S)
        assert (r["nrefl"][mirror] == 1).all() and (r["bent"][mirror] == 0).all()
        assert (r["bent"][~mirror] == 1).all() and (r["tints"][~mirror] == 1 if S == 2 else r["tints"][~mirror] >= 1).all()
        assert np.array_equal(r["bend_face"][~mirror], face[~mirror])
        assert (r["hit"][mirror] == 0).all()  # reflected into the open
    # tied diagonals into the room's corners and edges: all of them keep bouncing
    r = run("room_ties", 300)
    assert len(r["hit"]) == 40 and (r["nrefl"] >= 3).all()
    # +x through the water across the wrap: a liquid bend through the +x face (the wobble lands on the normal's own axis)
    r = run("wrap_x", 300)
    k = slice(0, 3)  # (the fourth is exactly axial: it never leaves x = 1010)
    assert (r["bent"][k] == 1).all() and (r["liq_bend"][k] == 1).all() and (r["bend_face"][k] == 0).all() and (r["tints"][k] >= 4).all()
    assert r["bent"][3] == 0 and r["pos"][3][0] == 1010
    print("wrap_x: tints %s, end %s" % (r["tints"].tolist(), r["pos"].tolist()))


def test_frame_poses(rt, oracle_mod, pair):
    """the frames of test_gpu_directed_shading: the narrow poses keep one sign octant over the whole frame (the compiled-octant
    instances of the straight trace, which hands over to the bouncing trace), all eight between them; at least two wide
    poses mix signs (per-wave sign flags); and every pose's frame has events, by the oracle, at both budgets"""
    _, T = pair
    seen, mixed = set(), 0
    for pose in hall.FRAME_POSES:
        org, dirs, cam, ppx, ppy = hall.frame_rays(oracle_mod, pose)
        sg = np.sign(dirs)
        one = bool((sg == sg[0]).all() and (np.abs(dirs) > 1e-3).all())
        if pose[3] is not None:
            assert one, pose[0]
            seen.add(tuple(sg[0].tolist()))
        else:
            mixed += not (sg == sg[0]).all()
        for S in (300, 40):
            r = T.shade_rays(org, dirs, S, rt.sun_dir(), liquid=True, time=1.25)
            ev = (r["nrefl"] > 0) | (r["bent"] != 0)
            assert ev.sum() >= 20 or (S == 40 and pose[0] == "pool"), (pose[0], S)  # (the pool lies more than 40 steps off that pose)
    assert len(seen) == 8 and mixed >= 2
