"""Directed rays: the equalities of svo_skip.h's closed-form crossings, aimed at instead of hoped for.

skip_box (lexicographic minimum of three exit events, ties z < y < x), count_est (f32 estimate + fix-up), seg_cap
(exact segments by binade), ceil_march and the in-loop ceiling boxes (tc > Ein, Ex == Ez, Ez <= tc && Ez <= Ex), the
post-loop dda_step tail and the 2^20 budget threshold are exact-arithmetic code: one ulp or one tie moves a hit by a
voxel.  Every battery here casts chosen rays on the cavern (tests/cavern.py: overhangs, a staircase of 16-column
blocks, dust, a tower to the top row) and compares with the oracle's castRayFromCam (ray_caster.cpp:54-87) on the same
inputs, every field bit-exact (test_gpu_parity.compare), no ray left out; the result must be the same with voxel
stepping (CAST_ITERATIVE), without ceilings (CAST_NO_CEILINGS) and, for frames, with per-wave sign flags
(CAST_NO_OCTANT) and in the segment instance (CAST_SEGMENTS); no ray may end on the progress guard.

Frames with a projection plane of size 0 give every pixel the camera direction itself (asserted below), and
frame_origins gives one launch several origins: that drives the frame-only instances (linear, the eight compiled sign
octants, their cached segment bounds, AO, wire records) with chosen rays."""
import os
import sys
import time

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cavern  # noqa: E402
from test_gpu_parity import compare  # noqa: E402

pytestmark = pytest.mark.gpu

SIGNS = [(sx, sy, sz) for sx in (1.0, -1.0) for sy in (1.0, -1.0) for sz in (1.0, -1.0)]
VALS = [1.0, 0.5, 0.25, 2.0 ** -6, 0.75, 0.375, 1.5, 1.0 / 3.0, 0.1, 0.0, -0.0]
# directions whose crossings tie exactly: |1 / d| in ratios of small integers
CORE = [(1, 1, 1), (1, 0.5, 0.25), (0.25, 1, 0.5), (1, 1, 0.5), (0.5, 1, 1), (0.75, 0.375, 1.5), (1, 1, 0.0), (0.0, 1, 1), (1, 0.0, 1),
        (1, 0.5, 0.0), (0.0, 1, 0.0), (1, 0.25, 2.0 ** -6)]
BUDGETS = (0, 1, 2, 3, 7, 300, 5000)
BASE = np.array([330.0, 60.0, 400.0])  # air inside the cavern: stairs, arch, roof, the 64^3 block and dust around it


@pytest.fixture(scope="module")
def cuda():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


@pytest.fixture(scope="module")
def worlds(rt, oracle_mod, cuda):
    """{tall: (uploaded Tree, oracle Tree)}, built once and left unchanged"""
    res = {}
    for tall in (False, True):
        w, T = cavern.cavern(rt, oracle_mod, tall)
        res[tall] = (w.build().upload(0), T)
    return res


# ---------------------------------------------------------------------------------------------------------- references --
def ref_rays(T, org, dirs, steps):
    """the oracle's castRayFromCam per explicit ray, as compare()'s reference"""
    ref = {k: [] for k in ("pos", "last", "steps", "hit", "flags", "color", "t")}
    for o, d in zip(np.ascontiguousarray(org, np.float32), np.ascontiguousarray(dirs, np.float32)):
        r = T.cast_ray(o, d, steps)
        assert r.err == 0
        for k, v in (("pos", list(r.pos)), ("last", list(r.last)), ("steps", r.steps), ("hit", r.hit), ("flags", r.flags),
                     ("color", r.color), ("t", r.t)):
            ref[k].append(v)
    dt = {"flags": np.uint32, "color": np.uint64, "t": np.float64}
    return {k: np.array(v, dtype=dt.get(k, np.int64)) for k, v in ref.items()}


def ref_frames(T, origins, dn, W, H, steps, ppx=0.0, ppy=0.0):
    """the oracle's frame per origin, concatenated in launch order"""
    parts = [T.cast_frame(o, dn, W, H, steps, ppx=ppx, ppy=ppy, nthreads=8 if W * H > 64 else 1) for o in origins]
    assert all(p["rc"] == 0 for p in parts)
    return {k: np.concatenate([p[k] for p in parts]) for k in ("pos", "last", "steps", "hit", "t", "color", "flags")}


def take(ref, idx):
    return {k: v[idx] for k, v in ref.items()}


def cat_refs(refs):
    return {k: np.concatenate([r[k] for r in refs]) for k in refs[0]}


def cat_outs(torch, outs):
    return {k: torch.cat([o[k] for o in outs]) for k in outs[0]}


def frame_flags(rt):
    return (0, rt.CAST_ITERATIVE, rt.CAST_NO_CEILINGS, rt.CAST_NO_OCTANT, rt.CAST_SEGMENTS)


def cast_frames(rt, tree, origins, dn, W, H, steps, flags=0, ppx=0.0, ppy=0.0, ao=False):
    """one launch over a list of camera positions (at most rt.MAX_FRAMES)"""
    assert 0 < len(origins) <= rt.MAX_FRAMES
    d = rt.Tree.frame_desc(origins[0], dn, W, H, steps, ppx=ppx, ppy=ppy, flags=flags, frame_origins=origins,
                           ao_samples=16 if ao else 0, ao_steps=5)
    n = rt.Tree.count(d)
    assert n == len(origins) * W * H
    out = rt.Tree.alloc_hits(n, 0, ao=ao)
    tree.cast(d, out)
    return d, out


def no_guard(rt, tree, out=None):
    assert tree.guard_trips() == 0
    if out is not None:
        assert (out["pos_steps"][:, 3] >= 0).all()


def ref_zero_plane(oracle_mod, T, origins, dn, W, H, steps):
    """ref_frames for a projection plane of size 0 from one castRayFromCam per origin: every pixel's ray is the oracle's
    pixel direction at that plane (test_zero_plane_gives_the_camera_direction), so its record is repeated W * H times"""
    d = oracle_mod.pixel_dir(dn, 0.0, 0.0, W, H, 0, 0)
    r = ref_rays(T, origins, np.tile(d, (len(origins), 1)), steps)
    return {k: np.repeat(v, W * H, axis=0) for k, v in r.items()}


def check_frames(rt, torch, tree, T, launches, W, H, steps, label, ppx=0.0, ppy=0.0, ref=None):
    """launches: [(origins, dn)]; all of them per flag variant, one comparison of the concatenated records"""
    if ref is None:
        ref = cat_refs([ref_frames(T, o, dn, W, H, steps, ppx, ppy) for o, dn in launches])
    for flags in frame_flags(rt):
        out = cat_outs(torch, [cast_frames(rt, tree, o, dn, W, H, steps, flags, ppx, ppy)[1] for o, dn in launches])
        torch.cuda.synchronize()
        compare(rt, tree, out, ref, "%s S=%d flags=%d" % (label, steps, flags))
        no_guard(rt, tree, out)
    return ref


# -------------------------------------------------------------------------------------------------------- A: explicit --
def tie_counts(org, dirs, nsteps=300):
    """exact ties per ray within nsteps DDA steps: castRayFromCam's f64 accumulation (deltaPos += absDelta, absDelta =
    |f32(1 / d)| widened; ray_caster.cpp:58-80) restated; a step counts when the stepping axis' value equals another's"""
    o, d = np.asarray(org, np.float32), np.asarray(dirs, np.float32)
    with np.errstate(all="ignore"):
        dl = (np.float32(1.0) / d).astype(np.float64)
        a = np.abs(dl)
        ex = o.astype(np.float64) - (d < 0)
        T = a - (ex - np.trunc(o).astype(np.float64)) * dl
        ties = np.zeros(len(o), np.int64)
        rows = np.arange(len(o))
        for _ in range(nsteps):
            ax = np.where((T[:, 0] < T[:, 1]) & (T[:, 0] < T[:, 2]), 0, np.where(T[:, 1] < T[:, 2], 1, 2))
            v = T[rows, ax]
            ties += np.isfinite(v) & ((T == v[:, None]).sum(1) >= 2)
            T[rows, ax] += a[rows, ax]
    return ties


def tie_directions():
    """unnormalised f32 directions from VALS under all sign patterns: the tied core, each core direction with one
    component moved by +-1 ulp, and a seeded sample of the other triples"""
    rng = np.random.default_rng(31)
    out = []
    for c in CORE:
        for s in SIGNS:
            d = np.array(c, np.float32) * np.array(s, np.float32)
            out.append(d)
            for k in range(3):
                for to in (np.float32(np.inf), np.float32(-np.inf)):
                    e = d.copy()
                    e[k] = np.nextafter(d[k], to)  # (a zero component becomes the smallest subnormal: an infinite absDelta)
                    out.append(e)
    for _ in range(28):
        c = rng.choice(VALS, 3)
        for s in SIGNS:
            out.append(np.array(c, np.float32) * np.array(s, np.float32))
    return np.array(out, np.float32)


def origin_classes(rng, n):
    """n origins of each class, (class id, (n, 3) f32): integral, half-integral, mixed, dyadic k + 2^-j (j = 1..14: short and
    long first segments), generic fractions, negative (trunc != floor; the same places, one extent down), in or at solids"""
    jit = lambda: rng.integers(-12, 13, (n, 3)).astype(np.float64)  # noqa: E731
    cls = [BASE + jit(), BASE + jit() + 0.5, BASE + jit() + rng.integers(0, 2, (n, 3)) * 0.5,
           BASE + jit() + 2.0 ** -rng.integers(1, 15, (n, 3)), BASE + jit() + rng.uniform(0.01, 0.99, (n, 3)),
           BASE + jit() - cavern.E + np.where(rng.integers(0, 2, (n, 1)) == 1, rng.uniform(0.01, 0.99, (n, 3)), 0.0),
           np.array([300.5, 15.5, 300.5]) + rng.integers(0, 3, (n, 3)) * np.array([1.0, 1.0, 1.0])]
    return [(i, c.astype(np.float32)) for i, c in enumerate(cls)]


def explicit_battery():
    """(origins, dirs, group key) of battery A, in grouped order: sign octant, then origin class"""
    rng = np.random.default_rng(32)
    dirs = tie_directions()
    per = 3
    o, d, key = [], [], []
    for i, dv in enumerate(dirs):
        octant = int(dv[0] < 0) + 2 * int(dv[1] < 0) + 4 * int(dv[2] < 0)
        classes = origin_classes(rng, 1)
        pick = [0, 1 + i % 2] + list(rng.choice(np.arange(3, 7), per - 2, replace=False)) if i % 3 else [0, 3, 4]
        for c in pick:
            o.append(classes[c][1][0])
            d.append(dv)
            key.append(octant * 16 + c)
    o, d, key = np.array(o, np.float32), np.array(d, np.float32), np.array(key)
    order = np.argsort(key, kind="stable")
    return o[order], d[order], key[order]


def test_explicit_tied_rays(rt, cuda, worlds):
    """A: tied and nearly tied explicit rays (the segment instance with per-wave sign flags), grouped and shuffled"""
    tree, T = worlds[False]
    org, dirs, _ = explicit_battery()
    n = len(org)
    assert n * len(BUDGETS) <= 21000
    ties = tie_counts(org, dirs)
    print("A: %d rays x %d budgets, %d rays with >= 20 exact ties in 300 steps (max %d)" % (n, len(BUDGETS), (ties >= 20).sum(), ties.max()))
    assert (ties >= 20).sum() >= 200
    perm = np.random.default_rng(33).permutation(n)
    gd = {False: cuda.from_numpy(dirs).cuda(), True: cuda.from_numpy(np.ascontiguousarray(dirs[perm])).cuda()}
    go = {False: cuda.from_numpy(org).cuda(), True: cuda.from_numpy(np.ascontiguousarray(org[perm])).cuda()}
    for steps in BUDGETS:
        ref = ref_rays(T, org, dirs, steps)
        print("A: S=%d oracle hit fraction %.3f" % (steps, (ref["hit"] != 0).mean()))
        for shuffled in (False, True):
            r = take(ref, perm) if shuffled else ref
            for flags in (0, rt.CAST_ITERATIVE, rt.CAST_NO_CEILINGS):
                out = tree.cast_rays(gd[shuffled], go[shuffled], steps=steps, flags=flags)
                compare(rt, tree, out, r, "A S=%d shuffled=%d flags=%d" % (steps, shuffled, flags))
                no_guard(rt, tree, out)


# ---------------------------------------------------------------------------------------------- B: the frame instances --
def frame_directions(rt):
    """the tie set, normalised: all components nonzero in all eight octants (the compiled-octant instances), and with a zero
    component (no octant: frame_dirs returns 0)"""
    full = [np.array(c, np.float32) * np.array(s, np.float32) for c in ((1, 0.5, 0.25), (1, 1, 1), (0.5, 1, 1)) for s in SIGNS]
    zero = [(1, -1, 0), (0, -1, 1), (1, 0, 1), (-1, 0, -1), (0, -1, 0), (1, 0, 0), (-1, 0.5, 0), (0, 1, -0.25)]
    return [rt.normalize(d) for d in full], [rt.normalize(d) for d in zero]


def origin_lists():
    """16 camera positions each: integral; half-integral and mixed; one holding fractional origins (dyadic and generic)"""
    rng = np.random.default_rng(34)
    jit = lambda: rng.integers(-12, 13, (16, 3)).astype(np.float64)  # noqa: E731
    li = BASE + jit()
    li[3] -= cavern.E  # (negative coordinates: the same place one extent down)
    lh = BASE + jit() + rng.integers(0, 2, (16, 3)) * 0.5
    lh[0] = BASE + 0.5
    lh[5] -= cavern.E
    lf = BASE + jit()
    lf[1::2] += 2.0 ** -rng.integers(1, 15, (8, 3))
    lf[2::4] += rng.uniform(0.01, 0.99, (4, 3))
    lf[7] -= cavern.E
    return {"integral": li.astype(np.float32), "half": lh.astype(np.float32), "fractional": lf.astype(np.float32)}


def test_zero_plane_gives_the_camera_direction(rt, oracle_mod):
    """the premise of the frame batteries: with ppx = ppy = 0 every pixel's direction is the camera direction, and normalising
    keeps power-of-two ratios (so exact ties survive)"""
    full, zero = frame_directions(rt)
    for dn in full + zero:
        px = rt.pixel_dirs(dn, 32, 8, 0.0, 0.0).reshape(-1, 3)
        assert (px.view(np.uint32) == px[0].view(np.uint32)).all()
        assert np.array_equal(px[0], oracle_mod.pixel_dir(dn, 0.0, 0.0, 32, 8, 5, 3))
    d = rt.normalize((1, -0.5, 0.25))
    assert d[0] == -2 * d[1] == 4 * d[2]
    org = np.tile(BASE.astype(np.float32), (len(full), 1))
    assert tie_counts(org, np.array(full, np.float32)).min() >= 100  # (from an integral origin, of 300 steps)


@pytest.mark.parametrize("kind", ["integral", "half", "fractional"])
@pytest.mark.parametrize("steps", [300, 3000])
def test_frame_instances_tied_rays(rt, cuda, worlds, kind, steps):
    """B: the tie set through the frame instances, 32 x 8 pixels of one direction per camera position: the linear instances
    (origins all integral / half-integral: 8-byte wire records) and the segment ones with cached bounds (a fractional origin)"""
    tree, T = worlds[False]
    origins = origin_lists()[kind]
    full, zero = frame_directions(rt)
    d = rt.Tree.frame_desc(origins[0], full[0], 32, 8, steps, ppx=0.0, ppy=0.0, frame_origins=origins)
    assert tree.wire_bytes(d) == (12 if kind == "fractional" else 8)  # (the launch's instance follows the same test: need_seg)
    ref = check_frames(rt, cuda, tree, T, [(origins, dn) for dn in full + zero], 32, 8, steps, "B " + kind)
    print("B %s S=%d: %d rays, oracle hit fraction %.3f" % (kind, steps, len(ref["hit"]), (ref["hit"] != 0).mean()))
    assert 0.05 < (ref["hit"] != 0).mean() < 0.95


@pytest.mark.parametrize("kind", ["integral", "half", "fractional"])
def test_frame_instances_ao_and_wire(rt, cuda, worlds, kind):
    """B: the AO instance (16 samples, 5 steps) against the oracle's counts, and cast_wire -> wire_scatter equal to the plain
    cast, on the same directed frames"""
    tree, T = worlds[False]
    origins = origin_lists()[kind]
    full, zero = frame_directions(rt)
    W, H, S = 32, 8, 300
    n_hit = 0
    for dn in full + zero[:4]:
        aos, hits = zip(*[T.cast_frame_ao(o, dn, W, H, S, 16, 5, ppx=0.0, ppy=0.0) for o in origins])
        ao, hit = np.concatenate(aos), np.concatenate(hits)
        for flags in (0, rt.CAST_NO_OCTANT, rt.CAST_SEGMENTS):
            d, out = cast_frames(rt, tree, origins, dn, W, H, S, flags, ao=True)
            cuda.cuda.synchronize()
            g = rt.decode_hits(out)
            assert np.array_equal(g["hit"], hit != 0), (kind, dn, flags)
            assert np.array_equal(g["ao"], ao), (kind, dn, flags)
        n_hit += int((hit != 0).sum())
        # the wire round trip of the same launch
        d, plain = cast_frames(rt, tree, origins, dn, W, H, S, 0, ao=True)
        n = rt.Tree.count(d)
        wire = cuda.zeros((n, tree.wire_bytes(d)), dtype=cuda.uint8, device="cuda")
        wao = cuda.zeros(n, dtype=cuda.uint8, device="cuda")
        tree.cast_wire(d, wire, wao)
        back = rt.Tree.alloc_hits(n, 0, ao=True)
        for k in back:
            back[k].fill_(-1 if back[k].dtype != cuda.uint8 else 255)
        tree.wire_scatter(d, wire, back, ao=wao)
        cuda.cuda.synchronize()
        for k in ("pos_steps", "t", "info", "ao"):  # (t by its bits: NaN on rays that step along a NaN axis)
            a, b = (back[k].view(cuda.int32), plain[k].view(cuda.int32)) if k == "t" else (back[k], plain[k])
            assert cuda.equal(a, b), (kind, dn, k)
    assert n_hit > 1000  # AO counts were compared on hits
    no_guard(rt, tree)


@pytest.mark.parametrize("pp", [2.0 ** -14, 2.0 ** -10])
def test_narrow_fans_around_ties(rt, cuda, worlds, pp):
    """B: 64 x 32 fans of near-ties around each tie direction (count_est's one-step fix-up)"""
    tree, T = worlds[False]
    L = origin_lists()
    lin = np.concatenate([L["integral"][:2], L["half"][:2]])
    seg = L["fractional"][1:4]
    full, zero = frame_directions(rt)
    launches = [(o, dn) for dn in full + zero[:4] for o in (lin, seg)]
    ref = check_frames(rt, cuda, tree, T, launches, 64, 32, 300, "fan %g" % pp, ppx=pp, ppy=pp)
    print("fans pp=%g: %d rays, oracle hit fraction %.3f" % (pp, len(ref["hit"]), (ref["hit"] != 0).mean()))


# ------------------------------------------------------------------------------ C: ceiling events at block boundaries --
STAIR_DIRS = {"boundary": [(1, -1, 0), (1, -1, 1), (-1, -1, 1), (1, -0.5, 0.25), (1, -0.25, 0.5), (1, -2.0 ** -3, 2.0 ** -1), (1, -2, 1)],
              # block corners: the x and the z boundary event coincide (Ex == Ez) k and m columns away, before, at and after the ceiling event
              "corner": [(1, -0.5, 1), (1, -0.25, 1), (1, -3, 1), (1, -1, 0.5), (0.5, -1, 1), (1, -0.5, 0.5), (0.25, -1, 1), (1, -2.0 ** -4, 1),
                         (0.5, -0.25, 1)]}


def stair_directions(rt, group):
    """STAIR_DIRS[group] and their mirror images in x (up / down the stairs) and z, normalised"""
    seen, out = set(), []
    for d in STAIR_DIRS[group]:
        for mx in (1, -1):
            for mz in (1, -1):
                e = (d[0] * mx, d[1], d[2] * mz)
                if (e[0], e[1], abs(e[2]) if e[2] == 0 else e[2]) not in seen:
                    seen.add((e[0], e[1], abs(e[2]) if e[2] == 0 else e[2]))
                    out.append(rt.normalize(e))
    return out


def stair_origins(ceil16, offs=(-1, 0, 1)):
    """integral origins around 16-column block boundaries of the staircase: x (z) one column before, at and after a boundary,
    y = c + 1, c + 2, c + 16, c + 17, c + 18 above the ceiling c of the origin's own block: from there the y event entering the
    ceiling row coincides with an x (z, or both) boundary event for the directions of STAIR_DIRS"""
    bx = [cavern.STAIR_X0, cavern.STAIR_X0 + 16, cavern.STAIR_X0 + 80, cavern.STAIR_X0 + 176, cavern.STAIR_X0 + 192]
    xs = [b + k for b in bx for k in offs]
    zs = [b + k for b in (cavern.STAIR_Z0, cavern.STAIR_Z0 + 32) for k in offs] + [cavern.STAIR_Z0 + 15, cavern.STAIR_Z0 + 16]
    out = []
    for x in xs:
        for z in zs:
            c = int(ceil16[z >> 4, x >> 4])
            out += [(x, c + k, z) for k in (1, 2, 16, 17, 18)]
    return np.array(out, np.float32)


@pytest.mark.parametrize("group", sorted(STAIR_DIRS))
@pytest.mark.parametrize("shift", [0.0, 0.5, 2.0 ** -3, 2.0 ** -11])
def test_ceiling_events_at_block_boundaries(rt, oracle_mod, cuda, worlds, shift, group):
    """C: descents over the staircase whose ceiling event ties with a block-boundary event (ceil_march at the start of the ray
    and the in-loop ceiling boxes): integral and half-integral grids reach the linear instances, the same grid shifted by a
    dyadic fraction the segment ones.  The "corner" group aims at Ex == Ez.  (A build without that term of ceil_march gives the
    same results on all of these: the term ends the march early at a block corner, and without it the march still takes the z
    boundary before the x one, as the DDA does, re-testing tc > Ein in the block between.)"""
    tree, T = worlds[False]
    ceil16 = tree.ceilings()[0]
    assert tree.ceil_k0 == 2
    org = stair_origins(ceil16, (-1, 0, 1) if group == "boundary" else (-4, -2, -1, 0))
    stairs = ceil16[cavern.STAIR_Z0 >> 4, (cavern.STAIR_X0 >> 4):(cavern.STAIR_X0 >> 4) + cavern.STAIR_N]
    assert np.array_equal(stairs, [cavern.stair_top(i) for i in range(cavern.STAIR_N)])  # ceilings 16 rows apart
    org = org + np.float32(shift)
    dirs = stair_directions(rt, group)
    launches = [(org[i:i + rt.MAX_FRAMES], dn) for dn in dirs for i in range(0, len(org), rt.MAX_FRAMES)]
    ref = cat_refs([ref_zero_plane(oracle_mod, T, o, dn, 8, 8, 300) for o, dn in launches])
    some = launches[:: max(1, len(launches) // 40)]  # (and whole oracle frames for a sample of the launches)
    whole = cat_refs([ref_frames(T, o, dn, 8, 8, 300) for o, dn in some])
    part = cat_refs([ref_zero_plane(oracle_mod, T, o, dn, 8, 8, 300) for o, dn in some])
    assert all(np.array_equal(whole[k], part[k], equal_nan=k == "t") for k in part)
    check_frames(rt, cuda, tree, T, launches, 8, 8, 300, "C %s shift %g" % (group, shift), ref=ref)
    print("C %s shift=%g: %d origins x %d directions, oracle hit fraction %.3f" % (group, shift, len(org), len(dirs), (ref["hit"] != 0).mean()))
    assert (ref["hit"] != 0).mean() > 0.5


def test_ceiling_march_runs(rt, cuda, worlds):
    """C: on a representative pose over the stairs the march crosses blocks (ceil_moves > 0)"""
    tree, _ = worlds[False]
    st = tree.cast_stats((cavern.STAIR_X0 - 1.0, 240.0, cavern.STAIR_Z0 + 8.0), rt.normalize((1, -1, 0)), 96, 64, 300)
    print("C: ceil_moves per ray %.3f" % st["ceil_moves"])
    assert st["ceil_moves"] > 0 and st["no_progress"] == 0


# --------------------------------------------------------------------------------------------------- D: overhang frames --
CAMS = {"integral": (330.0, 60.0, 400.0), "half": (350.5, 70.5, 380.5), "fractional": (412.3, 50.7, 371.45)}


@pytest.mark.parametrize("cam", sorted(CAMS))
def test_overhang_frames(rt, cuda, worlds, cam):
    """D: 96 x 64 frames from inside the cavern in all eight sign octants, S = 300 and 3000: every field, the AO counts and the
    flag variants against the oracle"""
    tree, T = worlds[False]
    org = CAMS[cam]
    fr = []
    for s in SIGNS:
        dn = rt.normalize((s[0] * 1.0, s[1] * 0.45, s[2] * 0.8))
        for S in (300, 3000):
            ref = check_frames(rt, cuda, tree, T, [([org], dn)], 96, 64, S, "D %s %s" % (cam, s), ppx=None, ppy=None)
            fr.append((ref["hit"] != 0).mean())
        ao, hit = T.cast_frame_ao(org, dn, 96, 64, 300, 16, 5)
        for flags in (0, rt.CAST_NO_OCTANT):
            g = rt.decode_hits(tree.cast_frame(org, dn, 96, 64, 300, ao_samples=16, ao_steps=5, flags=flags))
            assert np.array_equal(g["hit"], hit != 0) and np.array_equal(g["ao"], ao), (cam, s, flags)
    print("D %s: oracle hit fractions per pose / budget: %s" % (cam, " ".join("%.2f" % f for f in fr)))
    assert 0.2 <= np.mean(fr) <= 0.8 and sum(0 < f < 1 for f in fr[::2]) >= 2
    no_guard(rt, tree)


SHADE_POSES = [((394.5, 22.5, 288.5), (0.6, -0.1, 0.5)),        # the mirror patch and the glass wall on the floor, some sky
               ((296.5, 44.5, 452.5), (-0.55, -0.6, -0.6)),     # the arch and the shadow its floating pillar casts on the floor
               ((404.0, 300.0, 330.25), (0.1, 0.35, 1.0))]      # the 64^3 block from below, dust, sky


@pytest.mark.parametrize("pose", [0, 1, 2])
def test_overhang_shading(rt, cuda, worlds, pose):
    """D: the shading pass where overhangs cast shadows and mirror / glass voxels bend rays, with and without hit records
    (without them the straight trace may leave early: ESCAPE)"""
    from test_gpu_shade import _check

    tree, T = worlds[False]
    org, d = SHADE_POSES[pose]
    dn = rt.normalize(d)
    sun = rt.sun_dir()
    ref = T.shade_frame(org, dn, 96, 64, 300, sun)
    rgba, hits = tree.shade_frame(org, dn, 96, 64, 300, sun=sun, with_hits=True)
    hit = rt.decode_hits(hits)["hit"]
    _check(rgba, ref, hit, "D shade %d" % pose)
    _check(tree.shade_frame(org, dn, 96, 64, 300, sun=sun), ref, hit, "D shade %d, no records" % pose)
    assert 0.1 < hit.mean() < 1.0
    no_guard(rt, tree)


# ------------------------------------------------------------------------------- E: top of the world, wrap, outside it --
def edge_rays(rt):
    """[(direction, origins)]: climbing along and past the tower, wrapping in y from below and above, through the wrap corners,
    starting outside the extent"""
    tx, tz = cavern.TOWER
    n = rt.normalize
    return [
        ((0.0, 1.0, 0.0), [(tx - 1, 20, tz), (tx + 1.5, 900.5, tz + 0.5), (tx + 0.5, 1000.25, tz - 0.5), (tx, 1100, tz + 1), (tx - 1, -30, tz)]),
        (n((0.001, 1, 0.0005)), [(tx - 1, 20, tz), (tx - 0.75, 600.5, tz - 0.25), (tx - 1.5, 1030.5, tz + 0.5), (tx - 2, -700, tz)]),
        (n((0.05, 1, 0.02)), [(tx - 40, 200, tz - 16), (tx - 50.5, 30.5, tz - 20.5), (330, 60, 400), (330.25, 1500.5, 400.125)]),
        (n((0.05, -1, 0.02)), [(tx - 5, 1023, tz - 2), (tx - 5.5, 100.5, tz - 2.5), (330, 2060, 400), (10, 3, 10), (10.5, -0.5, 10.5)]),
        (n((1, 1, 1)), [(1000, 1000, 1000), (1020.5, 1020.5, 1020.5), (1022.25, 1021.5, 1022), (-30, -30, -30), (990, 1000, 1010)]),
        (n((-1, -1, -1)), [(20, 20, 20), (3.5, 3.5, 3.5), (1.25, 2.5, 1), (1040, 1050, 1045), (2.0, 1.0, 2.0)]),
        (n((1, 0.5, 0.25)), [(1023 - 40, 1023 - 20, 1023 - 10), (-1064.5, -1.5, -1034.5), (2030, 1010, 2040), (1500.5, 900.25, -1500.75)]),
        (n((-1, 0.5, -1)), [(330, 60, 400), (-1700, 1000, 2400), (1100.5, 1023.5, 1100.5), (4, 1019, 4)]),
    ]


@pytest.mark.parametrize("tall", [True, False], ids=["tall", "low"])
def test_top_wrap_and_outside(rt, cuda, worlds, tall):
    """E: ceiling = the top row, wrap in every axis, origins outside [0, 1024)^3 (coordinates wrap), on the tall world; the
    same rays on the low world, where upward rays start above the tree's highest row (the pre_top move)"""
    tree, T = worlds[tall]
    rays = edge_rays(rt)
    org = np.array([o for _, os_ in rays for o in os_], np.float32)
    dirs = np.array([d for d, os_ in rays for _ in os_], np.float32)
    go, gd = cuda.from_numpy(org).cuda(), cuda.from_numpy(dirs).cuda()
    hits = 0
    for steps in (300, 1100, 5000):
        ref = ref_rays(T, org, dirs, steps)
        hits += int((ref["hit"] != 0).sum())
        for flags in (0, rt.CAST_ITERATIVE, rt.CAST_NO_CEILINGS):
            out = tree.cast_rays(gd, go, steps=steps, flags=flags)
            compare(rt, tree, out, ref, "E explicit tall=%d S=%d flags=%d" % (tall, steps, flags))
            no_guard(rt, tree, out)
        for d, os_ in rays:  # the same rays through the frame instances
            check_frames(rt, cuda, tree, T, [(np.array(os_, np.float32), np.asarray(d, np.float32))], 8, 8, steps, "E frames tall=%d" % tall)
    print("E tall=%d: %d rays x 3 budgets, %d oracle hits" % (tall, len(org), hits))
    assert hits >= (12 if tall else 3)


# ------------------------------------------------------------------------------------------- F: the 2^20 budget boundary --
def long_rays():
    """64 explicit rays on the low world: rows 600..900 are empty, so axis-aligned rays there spend any budget, and slowly
    descending ones reach the cavern after hundreds of thousands of steps"""
    rng = np.random.default_rng(36)
    org, dirs = [], []
    for i, d in enumerate([(1, 0, 0), (0, 0, 1), (-1, 0, 0), (0, 0, -1), (1, 0, 1), (-1, 0, 1), (1, -0.0, -1), (0, 0, 0), (1, 0, 0), (0, 0, 1),
                           (1, 1e-30, 0), (1, 0, 0.5)]):
        org.append((10.5 + 3 * i, 700.0 + 7 * i + (0.5 if i % 2 else 0.0), 10.5 + 5 * i) if i < 8 else (300.25 + i, 640.5, 280.75))
        dirs.append(d)
    while len(org) < 64:
        org.append((rng.uniform(0, 1024), rng.uniform(455, 600), rng.uniform(0, 1024)) if len(org) % 2 else
                   (float(rng.integers(0, 1024)) + 0.5, float(rng.integers(455, 600)) + 0.5, float(rng.integers(0, 1024)) + 0.5))
        dirs.append((1.0, -rng.uniform(0.0002, 0.002), rng.uniform(-1, 1)) if len(org) % 3 else (rng.uniform(-1, 1), -rng.uniform(0.0002, 0.002), 1.0))
    return np.array(org, np.float32), np.array(dirs, np.float32)


def path_counters(rt, torch, tree, org, dn, steps, stream, limit):
    """traversal counters (CAST_STATS) of an 8 x 8 zero-plane frame, summed over its 64 rays; the launch under a time limit"""
    d = rt.Tree.frame_desc(org, dn, 8, 8, steps, ppx=0.0, ppy=0.0, flags=rt.CAST_STATS)
    n = rt.Tree.count(d)
    st = torch.zeros(rt.STATS_HEADER + 2 * rt.Tree.blocks(d) + n, dtype=torch.int64, device="cuda")
    d.stats = st.data_ptr()
    out = rt.Tree.alloc_hits(n, 0)
    torch.cuda.synchronize()
    wait_launch(torch, stream, lambda: tree.cast(d, out, stream), limit, "stats S=%d" % steps)
    return dict(zip(rt.STAT_NAMES, st[:len(rt.STAT_NAMES)].cpu().numpy().tolist())), out


def wait_launch(torch, stream, launch, limit, label):
    """launch() on `stream`, then poll for its end: fails when it takes longer than `limit` seconds"""
    t0 = time.perf_counter()
    res = launch()
    done = torch.cuda.Event()
    done.record(stream)
    while not done.query():
        assert time.perf_counter() - t0 < limit, "%s: the launch did not end within %.1f s" % (label, limit)
        time.sleep(0.001)
    print("F %s: launch %.3f s" % (label, time.perf_counter() - t0))
    return res


# one lane's 2^20 dda_step iterations (a voxel lookup through at most 5 levels each), at a generous 10 us per iteration
LONG_LIMIT_S = (1 << 20) * 10e-6


def test_budget_threshold_2_20(rt, oracle_mod, cuda, worlds):
    """F: budget < 2^20 selects the closed-form crossings, 2^20 voxel stepping: both against the oracle, and the two budgets'
    results differ only as the oracle's do.  Each launch gets its own time limit (LONG_LIMIT_S)."""
    tree, T = worlds[False]
    org, dirs = long_rays()
    go, gd = cuda.from_numpy(org).cuda(), cuda.from_numpy(dirs).cuda()
    stream = cuda.cuda.Stream()
    res, refs = {}, {}
    for steps in ((1 << 20) - 1, 1 << 20):
        ref = refs[steps] = ref_rays(T, org, dirs, steps)
        used = steps - ref["steps"]
        spent, far = (ref["hit"] == 0).sum(), ((ref["hit"] != 0) & (used > 100000)).sum()
        print("F S=%d: %d rays spend the budget, %d hit after > 100,000 steps (longest %d)" % (steps, spent, far, used[ref["hit"] != 0].max()))
        assert spent >= 8 and far >= 8
        for flags in (0, rt.CAST_ITERATIVE, rt.CAST_NO_CEILINGS):
            out = wait_launch(cuda, stream, lambda: tree.cast_rays(gd, go, steps=steps, flags=flags, stream=stream, sync=False), LONG_LIMIT_S,
                              "S=%d flags=%d" % (steps, flags))
            compare(rt, tree, out, ref, "F S=%d flags=%d" % (steps, flags))
            no_guard(rt, tree, out)
            if flags == 0:
                res[steps] = rt.decode_hits(out)
    a, b = res[(1 << 20) - 1], res[1 << 20]
    ra, rb = refs[(1 << 20) - 1], refs[1 << 20]
    assert np.array_equal(b["steps"] - a["steps"], rb["steps"] - ra["steps"])
    assert np.array_equal((a["pos"] != b["pos"]).any(1), (ra["pos"] != rb["pos"]).any(1))
    assert np.array_equal(a["hit"] != b["hit"], (ra["hit"] != 0) != (rb["hit"] != 0))
    # which path ran: closed-form crossings below 2^20 (their count estimates are proven for budgets < 2^20 only), voxel stepping from
    # 2^20 on; a ray along an empty row, from a linear and from a fractional origin
    dn = rt.normalize((1.0, 2.0 ** -21, 0.5))  # (rises one row in 2^21 x steps: the rows it crosses hold nothing)
    for o in ((300.0, 640.5, 280.0), (300.25, 640.5, 280.75)):
        fastc, fo = path_counters(rt, cuda, tree, o, dn, (1 << 20) - 1, stream, LONG_LIMIT_S)
        slowc, so = path_counters(rt, cuda, tree, o, dn, 1 << 20, stream, LONG_LIMIT_S)
        print("F path counters %s: S=2^20-1 skips %d lookups %d; S=2^20 skips %d lookups %d" % (o, fastc["skips"], fastc["lookups"], slowc["skips"], slowc["lookups"]))
        assert fastc["rays"] == slowc["rays"] == 64 and fastc["no_progress"] == slowc["no_progress"] == 0
        assert fastc["skips"] >= 64 * 1000 and slowc["skips"] == 0
        for steps, o_ in (((1 << 20) - 1, fo), (1 << 20, so)):
            compare(rt, tree, o_, ref_zero_plane(oracle_mod, T, [o], dn, 8, 8, steps), "F frame %s S=%d" % (o, steps))
    no_guard(rt, tree)
