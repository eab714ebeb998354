"""Inputs, recording and comparison for the reference pins (oracle/REFERENCE_PINS.md): lookups, ray batteries and pixel
fans on two worlds, recorded from the reference's own compiled code (oracle.ref_core_run) into tests/golden/pins_R.npz
and pins_P.npz by tests/golden/make_golden.py, and generated again with other seeds by the live tests.

  R: initTetraHexaTree() + genWorld(), the reference application's world.  getBlock inside root child 63 (all three
     wrapped coordinates >= 768) ends the reference process (the aliased root child array), so
     no probe lies there and no ray's free DDA path (the walk with no tree, the whole budget) passes through it:
     budgets are lowered at construction until that holds, and child63_on_path() is asserted before the reference runs.
  P: tests/pin_world.py, put-only over a clean root.

A record set (`records`) is a dict of arrays: probe_flags, probe_color; ray_pos, ray_last, ray_steps, ray_flags,
ray_color; frame_pos, frame_last, frame_steps, frame_flags, frame_color (frames concatenated).  castRayFromCam gives
pos, lastPos and the steps left; flags and colour are getBlock(pos)'s, which tells a hit on the last step from a miss
(hit_of).  lastPos has no value in the reference when the budget is 0 (ray_caster.cpp:68): it is 0 in the records and
left out of comparisons there (same_records)."""
import hashlib
import io
import os
import sys
import zipfile

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cavern  # noqa: E402
import pin_world  # noqa: E402
import test_gpu_directed_rays as directed  # noqa: E402  (the tie directions, VALS, SIGNS and edge rays of the directed batteries)

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
E = cavern.E
EMPTY = np.uint64(0xFFFFFFFFFFFFFFFF)
BUDGETS = (0, 1, 2, 3, 7, 30, 300, 3000)
BUDGET_CYCLE = (300, 3000, 30, 7, 300, 3, 2, 1, 0, 3000, 300, 30)  # every budget of BUDGETS, the long ones more often
FRAME_W, FRAME_H, FRAME_STEPS = 64, 48, (30, 300)
DEBUG_BLOCKS = [(10, 100, 10), (100, 10, 100), (20, 10, 200), (1, 10, 10), (2, 10, 10), (3, 10, 10), (4, 10, 10)]  # (not the one in root child 63)
BASES = {"R": [(100.0, 45.0, 100.0), (60.0, 30.0, 140.0)], "P": [tuple(directed.BASE)]}
# (camera position, camera direction before normalising): an integral, a half-integral and a fractional position
CAMERAS = {"R": [((35.0, 50.0, 35.0), (1.0, 0.0, 1.0)), ((60.5, 70.5, 40.5), (1.0, -0.5, 0.6)), ((150.3, 44.7, 20.9), (-0.6, -0.2, 1.0))],
           "P": [((330.0, 60.0, 400.0), (1.0, -0.45, 0.8)), ((350.5, 70.5, 380.5), (-1.0, -0.45, 0.8)), ((412.3, 50.7, 371.45), (1.0, -0.45, -0.8))]}
SPECIAL = [0.0, -0.0, 1e-40, -1e-40, 1e-45, 1.0, -0.5, 37.5]  # zero, -0.0, denormals (1e-45: the smallest), un-normalised


# ------------------------------------------------------------------------------------------------------------ worlds --
def world_commands(world):
    return [("init",), ("gen",)] if world == "R" else pin_world.ref_commands()


def oracle_world(O, world):
    return O.Tree.reference_world() if world == "R" else pin_world.oracle_tree(O)


def product_world(rt, world):
    return rt.World.reference() if world == "R" else pin_world.product_world(rt)


def in_child63(p):
    return ((np.asarray(p, np.int64) & (E - 1)) >= 768).all(axis=-1)


# ------------------------------------------------------------------------------------------------------------ inputs --
def lookups(world, n, seed):
    """(n, 3) int32 probes: P — pin_world.probe_points; R — random points of [-50, 1100)^3, as many in and around the
    terrain's box (a quarter of those whole extents away), and the debug blocks; none in root child 63"""
    if world == "P":
        return pin_world.probe_points(n, seed)
    rng = np.random.default_rng(seed)
    k = (n - len(DEBUG_BLOCKS)) // 2
    near = np.stack([rng.integers(-6, 206, 4 * k), rng.integers(-3, 76, 4 * k), rng.integers(-6, 206, 4 * k)], 1)
    move = rng.integers(0, 4, len(near)) == 0
    near[move] += rng.integers(-1, 2, (int(move.sum()), 3)) * E
    wide = rng.integers(-50, 1100, (4 * (n - k), 3))
    near, wide = near[~in_child63(near)][:k], wide[~in_child63(wide)][:n - k - len(DEBUG_BLOCKS)]
    p = np.concatenate([np.array(DEBUG_BLOCKS), near, wide]).astype(np.int32)
    assert len(p) == n and not in_child63(p).any()
    return p


def _origins(rng, base, n):
    """n origins of each class around base: integral, half-integral, dyadic fraction, generic fraction, negative (trunc is
    not floor) and beyond the extent (the last two integral, half-integral or fractional in turn)"""
    jit = lambda: rng.integers(-12, 13, (n, 3)).astype(np.float64)  # noqa: E731
    frac = lambda: np.choose(np.arange(n)[:, None] % 3, [np.zeros((n, 3)), np.full((n, 3), 0.5), rng.uniform(0.01, 0.99, (n, 3))])  # noqa: E731
    b = np.asarray(base, np.float64)
    return [b + jit(), b + jit() + 0.5, b + jit() + 2.0 ** -rng.integers(1, 15, (n, 3)), b + jit() + rng.uniform(0.01, 0.99, (n, 3)),
            b + jit() + frac() - E * rng.integers(1, 3, (n, 3)), b + jit() + frac() + E * rng.integers(0, 3, (n, 3))]


def ray_battery(world, O, seed, n_random):
    """(origins f32 (n, 3), directions f32 (n, 3), budgets int32 (n,)): random rays (normalised and not) from every origin
    class, n_random per class; every tie direction of the directed batteries and every triple of SPECIAL, the origin
    class and the budget changing from ray to ray; on P the edge rays (wrap, tower, outside the extent) at 300, 1100, 3000
    and rays into the liquid, some ending inside it"""
    rng = np.random.default_rng(seed)
    bases = BASES[world]
    org, dirs = [], []
    for b in bases:
        for cls in _origins(rng, b, n_random // len(bases)):
            d = rng.normal(size=(len(cls), 3))
            d /= np.linalg.norm(d, axis=1)[:, None]
            d[::3] *= 10.0 ** rng.uniform(-3, 3, (len(d[::3]), 1))
            org.append(cls)
            dirs.append(d)
    sp = np.array([(a, b, c) for a in SPECIAL for b in SPECIAL for c in SPECIAL], np.float32)
    for fixed in (directed.tie_directions(), sp):
        cls = np.stack(_origins(rng, bases[0], len(fixed)))  # (class, ray, 3)
        pick = rng.integers(0, len(cls), len(fixed))
        pick[:len(cls) * 8] = np.arange(len(cls) * 8) % len(cls)
        org.append(cls[pick, np.arange(len(fixed))])
        dirs.append(fixed)
    org, dirs = np.concatenate(org).astype(np.float32), np.concatenate(dirs).astype(np.float32)
    budgets = np.array(BUDGET_CYCLE, np.int32)[(np.arange(len(org)) + rng.integers(0, 12)) % len(BUDGET_CYCLE)]
    if world == "P":
        eo, ed, eb = [], [], []
        for d, os_ in directed.edge_rays(O):  # (it asks its argument for normalize() only)
            for o in os_:
                for s in (300, 1100, 3000):
                    eo.append(o), ed.append(d), eb.append(s)
        cx, cy, cz = pin_world.CURTAIN  # through the liquid wall at the block behind it, and down through the pool to the floor
        px, py, pz = pin_world.POOL
        for i in range(48):
            eo.append((cx - 2 - i % 7 + (0.5, 0.0, 0.3)[i % 3], cy + 1 + i % 11 + 0.5, cz + 2 + i % 13 + 0.25))
            ed.append((1.0, (0.0, 0.05, -0.02)[i % 3], (0.01, 0.0, -0.03)[i % 3]))
            eo.append((px + 1 + i % 28 + 0.5, py + 6 + i % 5, pz + 1 + i % 27 + (0.0, 0.5)[i % 2]))
            ed.append(((0.1, 0.0, -0.2)[i % 3], -1.0, (0.2, 0.0, 0.1)[i % 3]))
            eb += [(300, 1, 2, 3, 7, 30)[i % 6]] * 2
        for i in range(24):  # straight down onto the floor from k rows above it: budget k + 1 hits on the last step, budget k misses
            k = i % 7
            eo += [(270.5 + 3 * i, cavern.FLOOR_TOP + 1 + k + 0.5, 260.5)] * 2
            ed += [(0.001, -1.0, -0.002)] * 2  # (not (0, -1, 0): with two zero components castRayFromCam compares NaNs and walks z)
            eb += [k + 1, k]
        org, dirs = np.concatenate([org, np.array(eo, np.float32)]), np.concatenate([dirs, np.array(ed, np.float32)])
        budgets = np.concatenate([budgets, np.array(eb, np.int32)])
    else:
        ladder = sorted(BUDGETS)
        bad = child63_on_path(org, dirs, budgets)
        while bad.any():  # lower the budget of a ray whose free path enters root child 63 (budget 0 takes no step)
            budgets[bad] = [ladder[ladder.index(int(b)) - 1] for b in budgets[bad]]
            bad[bad] = child63_on_path(org[bad], dirs[bad], budgets[bad])
    return np.ascontiguousarray(org), np.ascontiguousarray(dirs), budgets


def child63_on_path(org, dirs, budgets):
    """per ray: does castRayFromCam's walk with no tree (ray_caster.cpp:54-80 restated in numpy: f32 1 / d widened,
    f64 accumulation, ties z before y before x), over the whole budget, visit a voxel whose three wrapped coordinates
    are >= 768?  (the origin's voxel is not looked up and does not count)"""
    o, d, bud = np.asarray(org, np.float32), np.asarray(dirs, np.float32), np.asarray(budgets, np.int64)
    seen = np.zeros(len(o), bool)
    with np.errstate(all="ignore"):
        for b in np.unique(bud[bud > 0]):  # rays of one budget walk together
            idx = np.nonzero(bud == b)[0]
            oo, dd, rows = o[idx], d[idx], np.arange(len(idx))
            dl = (np.float32(1.0) / dd).astype(np.float64)
            a = np.where(dl >= 0, dl, -dl)
            st = np.where(dd < 0, -1, 1).astype(np.int64)
            r = np.trunc(oo).astype(np.int64)
            T = a - ((oo.astype(np.float64) - (dd < 0)) - r.astype(np.float64)) * dl
            hit = np.zeros(len(idx), bool)
            for _ in range(int(b)):
                ax = np.where((T[:, 0] < T[:, 1]) & (T[:, 0] < T[:, 2]), 0, np.where(T[:, 1] < T[:, 2], 1, 2))
                r[rows, ax] += st[rows, ax]
                T[rows, ax] += a[rows, ax]
                hit |= ((r & 768) == 768).all(1)
            seen[idx] = hit
    return seen


def frame_list(world, O):
    """[(camera position f32, normalised direction f32, steps)]: the three cameras at each budget of FRAME_STEPS"""
    return [(np.asarray(c, np.float32), O.normalize(d), s) for c, d in CAMERAS[world] for s in FRAME_STEPS]


def frame_dirs(O, cam_dir, ppx, ppy):
    """the oracle's pixel directions of a FRAME_W x FRAME_H fan, pixel order (py * W + px)"""
    return np.array([O.pixel_dir(cam_dir, ppx, ppy, FRAME_W, FRAME_H, k % FRAME_W, k // FRAME_W) for k in range(FRAME_W * FRAME_H)], np.float32)


def dir_checksum(dirs):
    return hashlib.sha256(np.ascontiguousarray(dirs, np.float32).tobytes()).hexdigest()[:16]


def make_inputs(world, O, seed, n_probes, n_random, fans=True):
    org, dirs, budgets = ray_battery(world, O, seed + 1, n_random)
    ppx, ppy = O.proj_plane(FRAME_W, FRAME_H)
    fl = frame_list(world, O) if fans else []
    inp = dict(probes=lookups(world, n_probes, seed), ray_org=org, ray_dir=dirs, ray_budget=budgets,
               frame_cam=np.array([f[0] for f in fl], np.float32).reshape(-1, 3), frame_dir=np.array([f[1] for f in fl], np.float32).reshape(-1, 3),
               frame_budget=np.array([f[2] for f in fl], np.int32), frame_pp=np.array([ppx, ppy], np.float32))
    if world == "R":  # nothing may reach root child 63: no probe or ray is left out afterwards
        assert not in_child63(inp["probes"]).any()
        assert not child63_on_path(org, dirs, budgets).any()
        for cam, d, s in fl:
            fd = frame_dirs(O, d, ppx, ppy)
            assert not child63_on_path(np.tile(cam, (len(fd), 1)), fd, np.full(len(fd), s)).any()
    return inp


# ----------------------------------------------------------------------------------------------------------- records --
def _frame_rays(O, inp):
    ppx, ppy = (float(v) for v in inp["frame_pp"])
    org, dirs, steps, sums = [], [], [], []
    for cam, d, s in zip(inp["frame_cam"], inp["frame_dir"], inp["frame_budget"]):
        fd = frame_dirs(O, d, ppx, ppy)
        sums.append(dir_checksum(fd))
        org.append(np.tile(cam, (len(fd), 1))), dirs.append(fd), steps.append(np.full(len(fd), s, np.int32))
    if not sums:
        return np.zeros((0, 3), np.float32), np.zeros((0, 3), np.float32), np.zeros(0, np.int32), sums
    return np.concatenate(org), np.concatenate(dirs), np.concatenate(steps), sums


def reference_records(O, world, inp, extra=()):
    """the records from the reference's own code: one process builds the world and answers everything.  None when
    oracle/_ref/ref_core has not been built; the process must exit 0 with an empty array free list.  Returns
    (records, pools, root[, results of the `extra` commands])"""
    fo, fd, fs, sums = _frame_rays(O, inp)
    cmds = world_commands(world)
    k = len(cmds)
    res = O.ref_core_run(cmds + [("pools",), ("root",), ("get", inp["probes"]), ("cast", inp["ray_org"], inp["ray_dir"], inp["ray_budget"]),
                                 ("cast", fo, fd, fs)] + list(extra) + [("pools",)])
    if res is None:
        return None
    pools, root, g, rays, fr = res[k:k + 5]
    assert pools["array_free"] == 0 and res[-1] == pools, "outside the reference's defined behaviour"
    rec = dict(probe_flags=g["flags"], probe_color=g["color"])
    for name, r in (("ray", rays), ("frame", fr)):
        rec.update({name + "_pos": r["pos"], name + "_last": r["last"], name + "_steps": r["steps"], name + "_flags": r["flags"],
                    name + "_color": r["color"]})
    rec["frame_dirsum"] = np.array(sums)
    return (rec, pools, root) + ((res[k + 5:-1],) if extra else ())


def oracle_records(O, T, inp):
    """the same records from the oracle (oracle/oracle.c): orc_get_block, orc_cast_ray and orc_get_block at its pos"""
    fo, fd, fs, sums = _frame_rays(O, inp)
    g = [T.get_block(int(x), int(y), int(z)) for x, y, z in inp["probes"]]
    rec = dict(probe_flags=np.array([b[0] for b in g], np.uint32), probe_color=np.array([b[1] for b in g], np.uint64))
    for name, (o, d, s) in (("ray", (inp["ray_org"], inp["ray_dir"], inp["ray_budget"])), ("frame", (fo, fd, fs))):
        pos, last, steps, fl, col = (np.zeros((len(o), 3), np.int32), np.zeros((len(o), 3), np.int32), np.zeros(len(o), np.int32),
                                     np.zeros(len(o), np.uint32), np.zeros(len(o), np.uint64))
        for i in range(len(o)):
            r = T.cast_ray(o[i], d[i], int(s[i]))
            assert r.err == 0
            pos[i], steps[i] = r.pos, r.steps
            if s[i] > 0:
                last[i] = r.last
            b = T.get_block(*[int(v) for v in r.pos])
            fl[i], col[i] = b[0], b[1]
            assert bool(r.hit) == bool(hit_of(fl[i], col[i], s[i]))  # (the oracle's own hit flag says the same as the block at pos)
            assert not r.hit or (r.flags, r.color) == (b[0], b[1])
        rec.update({name + "_pos": pos, name + "_last": last, name + "_steps": steps, name + "_flags": fl, name + "_color": col})
    rec["frame_dirsum"] = np.array(sums)
    return rec


def hit_of(flags, color, budget):
    """castRayFromCam's hit test (ray_caster.cpp:82) on the block at the returned pos: a stored block that is not LIQUID;
    with a budget of 0 no voxel is looked at"""
    return (np.asarray(color, np.uint64) != EMPTY) & ((np.asarray(flags, np.uint32) & 0x10) == 0) & (np.asarray(budget) > 0)


def same_records(a, b, label):
    """every field of two record sets equal, bit for bit, no entry left out"""
    for k in sorted(a):
        assert k in b and len(a[k]) == len(b[k]), (label, k)
        if len(a[k]) == 0:
            continue
        bad = np.nonzero(np.asarray(a[k] != b[k]).reshape(len(a[k]), -1).any(1))[0]
        assert len(bad) == 0, "%s: %s differs at %d of %d entries, first %s: %s / %s" % (label, k, len(bad), len(a[k]), bad[:5], a[k][bad[:3]], b[k][bad[:3]])
    assert sorted(a) == sorted(b), label


# ---------------------------------------------------------------------------------------------------------- fixtures --
def _last_code(pos, last, budget):
    """lastPos as one byte: pos - lastPos is one step along one axis; 2 * axis + (step < 0), 255 where the budget is 0"""
    d = pos.astype(np.int64) - last
    ax = np.abs(d).argmax(1)
    code = np.where(budget > 0, 2 * ax + (d[np.arange(len(d)), ax] < 0), 255).astype(np.uint8)
    assert np.array_equal(_last_decode(pos, code), last)
    return code


def _last_decode(pos, code):
    last = pos.astype(np.int32).copy()
    m = code != 255
    last[m, code[m] // 2] -= np.where(code[m] % 2 == 1, -1, 1)
    last[~m] = 0
    return last


def pack(inp, rec, pools, root):
    """a fixture's arrays: inputs as they are (f32 as bit patterns), records compact — positions int16, lastPos one byte,
    colours as indices into a table"""
    table = np.unique(np.concatenate([rec["probe_color"], rec["ray_color"], rec["frame_color"]]))
    assert len(table) < 65536
    fs = np.repeat(inp["frame_budget"], FRAME_W * FRAME_H)
    out = dict(probes=inp["probes"].astype(np.int32), ray_org=inp["ray_org"].view(np.uint32), ray_dir=inp["ray_dir"].view(np.uint32),
               ray_budget=inp["ray_budget"].astype(np.int16), frame_cam=inp["frame_cam"].view(np.uint32), frame_dir=inp["frame_dir"].view(np.uint32),
               frame_budget=inp["frame_budget"].astype(np.int16), frame_pp=inp["frame_pp"].view(np.uint32), frame_dirsum=rec["frame_dirsum"],
               colors=table, pools=np.array([pools[k] for k in ("node_next", "array_next", "node_free", "array_free")], np.int64),
               root=np.array([root["flags"], root["bitmap"], root["children"]], np.uint64))
    for name, budget in (("probe", None), ("ray", inp["ray_budget"]), ("frame", fs)):
        assert rec[name + "_flags"].max() < 256
        out[name + "_flags"] = rec[name + "_flags"].astype(np.uint8)
        out[name + "_color"] = np.searchsorted(table, rec[name + "_color"]).astype(np.uint16)
        if budget is not None:
            assert np.abs(rec[name + "_pos"]).max() < 32768 and 0 <= rec[name + "_steps"].min() and rec[name + "_steps"].max() < 32768
            out[name + "_pos"] = rec[name + "_pos"].astype(np.int16)
            out[name + "_steps"] = rec[name + "_steps"].astype(np.int16)
            out[name + "_last"] = _last_code(rec[name + "_pos"], rec[name + "_last"], budget)
    return out


def unpack(z):
    """(inputs, records, pools, root) of a fixture, as make_inputs / reference_records give them"""
    f32 = lambda k: np.ascontiguousarray(z[k]).view(np.float32)  # noqa: E731
    inp = dict(probes=z["probes"], ray_org=f32("ray_org"), ray_dir=f32("ray_dir"), ray_budget=z["ray_budget"].astype(np.int32),
               frame_cam=f32("frame_cam"), frame_dir=f32("frame_dir"), frame_budget=z["frame_budget"].astype(np.int32), frame_pp=f32("frame_pp"))
    rec = dict(frame_dirsum=z["frame_dirsum"])
    for name in ("probe", "ray", "frame"):
        rec[name + "_flags"] = z[name + "_flags"].astype(np.uint32)
        rec[name + "_color"] = z["colors"][z[name + "_color"]]
        if name != "probe":
            rec[name + "_pos"] = z[name + "_pos"].astype(np.int32)
            rec[name + "_steps"] = z[name + "_steps"].astype(np.int32)
            rec[name + "_last"] = _last_decode(rec[name + "_pos"], z[name + "_last"])
    pools = dict(zip(("node_next", "array_next", "node_free", "array_free"), (int(v) for v in z["pools"])))
    pools.update(nodes=pools["node_next"] >> 4, arrays=pools["array_next"] >> 8)
    root = dict(flags=int(z["root"][0]), bitmap=int(z["root"][1]), children=int(z["root"][2]))
    return inp, rec, pools, root


def load(world):
    with np.load(os.path.join(GOLD, "pins_%s.npz" % world)) as z:
        return unpack({k: z[k] for k in z.files})


def save_npz(path, arrays):
    """np.savez_compressed with fixed member order and dates: the same arrays give the same bytes"""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED, compresslevel=9) as zf:
        for k in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.ascontiguousarray(arrays[k]), allow_pickle=False)
            info = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            zf.writestr(info, buf.getvalue(), compresslevel=9)


FIXTURE_SEED = {"R": 20261, "P": 20262}
FIXTURE_PROBES, FIXTURE_RANDOM = 4000, 100  # probes per world; random rays per origin class (600 in all, of ~2,000 rays per world)
