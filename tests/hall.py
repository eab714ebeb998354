"""A hall of mirrors, glass and water, put block by block into the product's World and the oracle's tree alike (as
tests/cavern.py does): the fixture of tests/test_hall_host.py and tests/test_gpu_directed_shading.py.  The shading pass
(svo_shade_rays) reflects on flags & 7 == 3 and tints / bends on flags & 7 == 5; this world holds each kind as single
voxels (brick walks), as 4^3 and 16^3 uniform regions (closed-form crossings, the region walk), inside one another, next
to one another and across the world's wrap, with every face exposed.  5 levels (1024^3); levels as putBlock numbers
them: 6 = a voxel, 5 = 4^3, 4 = 16^3.  The oracle side starts from a clean root.  Everything lies in x, z in
[512, 672) except the blocks at the wrap in x.

batteries() returns the rays every test of the two files casts; which events they produce is decided from the oracle
alone, in test_hall_host.py."""
import numpy as np

from cavern import colour, ident  # noqa: F401  (the same Block colours: ids in the low 13 bits)

LEVELS = 5
E = 1 << (2 * LEVELS)
F_MIRROR, F_GLASS, F_WATER = 0x2, 0x4, 0x14
X0, X1 = 512, 672
ROOM_LO, ROOM_HI = (530, 40, 530), (555, 65, 555)  # the mirror room's one-voxel walls lie on these planes
ROOM_IN = ((531, 41, 531), (555, 65, 555))         # its interior [lo, hi): aligned to no brick
PILLAR = (540, 41, 545)                            # plain 2 x 6 x 2
PANE_X = 548                                       # glass pane x = 548, y 41..52, z 535..545
ROOM_WATER = (544, 44, 536)                        # 4 x 4 x 4 water voxels, put as voxels
MIRROR16, MIRROR4 = (576, 48, 528), (600, 52, 540)
GLASS16, GLASS4 = (576, 48, 560), (600, 52, 572)
GLASS16_MIRROR, GLASS16_PLAIN = (583, 55, 567), (580, 50, 570)
PANE_Y, PANE_Z = 70, 590                           # y = 70 over x, z in [560, 576); z = 590 over x in [560, 576), y in [48, 60)
CUBE = (608, 48, 592)                              # a standing 16^3 water cube: sides and bottom exposed
POOL = (624, 656)                                  # bed y = 40 and water y 41..46 over [624, 656)^2
POOL_GLASS = (640, 43, 640)
WRAP_WATER = [(1020, 60, 600), (0, 60, 600)]       # two 4^3 water blocks: one region of water across x = 1023 -> 1024
WRAP_PLAIN, WRAP_GLASS = (6, 61, 601), (1016, 56, 596)
# colour ids
C_FLOOR, C_WALL, C_PILLAR, C_PANE_X, C_ROOM_WATER, C_MIRROR16, C_MIRROR4, C_GLASS16, C_G16_MIRROR, C_G16_PLAIN = range(100, 110)
C_GLASS4, C_PANE_Y, C_PANE_Z, C_CUBE, C_BED, C_POOL, C_POOL_MIRROR, C_POOL_PLAIN, C_POOL_GLASS, C_WRAP_WATER = range(110, 120)
C_WRAP_PLAIN, C_WRAP_GLASS = 120, 121
ALL_IDS = tuple(range(100, 122))


def pool_mirrors():
    return [(630 + 3 * i, 41, 630 + 2 * i) for i in range(8)]


def pool_plains():
    return [(631 + 3 * i, 41, 640) for i in range(8)]


def _box(lo, n):
    return [(lo[0] + i, lo[1] + j, lo[2] + k) for i in range(n[0]) for j in range(n[1]) for k in range(n[2])]


def _puts():
    """the world as a list of (points (n, 3), flags (n,), colours (n,), level); later entries overwrite earlier ones"""
    out = []

    def add(pts, cid, level, flags=0):
        p = np.asarray(pts, np.int32).reshape(-1, 3)
        out.append((p, np.full(len(p), flags, np.uint32), np.full(len(p), colour(cid), np.uint64), level))

    g = np.arange(X0, X1, 16)
    add([(x, 16, z) for x in g for z in g], C_FLOOR, 4)
    lo, hi = ROOM_LO, ROOM_HI
    walls = set()
    for a in range(3):
        for v in (lo[a], hi[a]):
            n = [hi[k] - lo[k] + 1 for k in range(3)]
            n[a] = 1
            s = list(lo)
            s[a] = v
            walls.update(_box(s, n))
    add(sorted(walls), C_WALL, 6, F_MIRROR)
    add(_box(PILLAR, (2, 6, 2)), C_PILLAR, 6)
    add(_box((PANE_X, 41, 535), (1, 12, 11)), C_PANE_X, 6, F_GLASS)
    add(_box(ROOM_WATER, (4, 4, 4)), C_ROOM_WATER, 6, F_WATER)
    add([MIRROR16], C_MIRROR16, 4, F_MIRROR)
    add([MIRROR4], C_MIRROR4, 5, F_MIRROR)
    add([GLASS16], C_GLASS16, 4, F_GLASS)
    add([GLASS16_MIRROR], C_G16_MIRROR, 6, F_MIRROR)
    add([GLASS16_PLAIN], C_G16_PLAIN, 6)
    add([GLASS4], C_GLASS4, 5, F_GLASS)
    add(_box((560, PANE_Y, 560), (16, 1, 16)), C_PANE_Y, 6, F_GLASS)
    add(_box((560, 48, PANE_Z), (16, 12, 1)), C_PANE_Z, 6, F_GLASS)
    add([CUBE], C_CUBE, 4, F_WATER)
    n = POOL[1] - POOL[0]
    add(_box((POOL[0], 40, POOL[0]), (n, 1, n)), C_BED, 6)
    add(_box((POOL[0], 41, POOL[0]), (n, 6, n)), C_POOL, 6, F_WATER)
    add(pool_mirrors(), C_POOL_MIRROR, 6, F_MIRROR)
    add(pool_plains(), C_POOL_PLAIN, 6)
    add([POOL_GLASS], C_POOL_GLASS, 6, F_GLASS)
    add(WRAP_WATER, C_WRAP_WATER, 5, F_WATER)
    add([WRAP_PLAIN], C_WRAP_PLAIN, 6)
    add([WRAP_GLASS], C_WRAP_GLASS, 5, F_GLASS)
    return out


FILLER_AT = (700, 700, 700)                        # a voxel the hall leaves empty: palette_cases.preload's scratch voxel


def hall(rt, oracle_mod, preload=0, T=None):
    """(rt.World, oracle Tree) holding the same blocks.  preload: that many throw-away materials interned first
    (palette_cases.preload), so the hall's palette ids start at preload + 1; the oracle stores blocks per voxel and has no
    palette, so its tree is the same for any preload: pass a tree built earlier as T to share it (it is returned as is)"""
    w = rt.World(LEVELS)
    if preload:
        import palette_cases

        palette_cases.preload(w, preload, FILLER_AT)
    build_oracle = T is None
    if build_oracle:
        T = oracle_mod.Tree(LEVELS)
        oracle_mod.lib().orc_init_clean_root(T.h)
    for pts, flags, colours, level in _puts():
        w.put_blocks(pts, flags, colours, level=level)
        if build_oracle:
            for (x, y, z), f, c in zip(pts.tolist(), flags.tolist(), colours.tolist()):
                assert T.put_block(x, y, z, f, c, 0.0, level) == 0
    return w, T


# the structures' boxes (lo, hi) with hi exclusive: probe points and ray targets are drawn from them
BOXES = {
    "room": (ROOM_LO, tuple(v + 1 for v in ROOM_HI)),
    "room_water": (ROOM_WATER, tuple(v + 4 for v in ROOM_WATER)),
    "pillar": (PILLAR, (PILLAR[0] + 2, PILLAR[1] + 6, PILLAR[2] + 2)),
    "mirror16": (MIRROR16, tuple(v + 16 for v in MIRROR16)),
    "mirror4": (MIRROR4, tuple(v + 4 for v in MIRROR4)),
    "glass16": (GLASS16, tuple(v + 16 for v in GLASS16)),
    "glass4": (GLASS4, tuple(v + 4 for v in GLASS4)),
    "pane_y": ((560, PANE_Y, 560), (576, PANE_Y + 1, 576)),
    "pane_z": ((560, 48, PANE_Z), (576, 60, PANE_Z + 1)),
    "cube": (CUBE, tuple(v + 16 for v in CUBE)),
    "pool": ((POOL[0], 40, POOL[0]), (POOL[1], 47, POOL[1])),
    "wrap": ((1016, 56, 596), (1032, 64, 604)),
}


def probe_points(n, seed=11):
    """n seeded voxels in and next to every structure, the floor, and empty space"""
    rng = np.random.default_rng(seed)
    parts = []
    k = n // (len(BOXES) + 3)
    for lo, hi in BOXES.values():
        parts.append(np.stack([rng.integers(lo[a] - 3, hi[a] + 3, k) for a in range(3)], 1))
    parts.append(np.stack([rng.integers(X0 - 8, X1 + 8, k), rng.integers(12, 36, k), rng.integers(X0 - 8, X1 + 8, k)], 1))
    small = np.asarray(pool_mirrors() + pool_plains() + [POOL_GLASS, GLASS16_MIRROR, GLASS16_PLAIN, WRAP_PLAIN])
    parts.append(small[rng.integers(0, len(small), k)] + rng.integers(-1, 2, (k, 3)))
    parts.append(small)
    rest = n - sum(len(p) for p in parts)
    parts.append(rng.integers(0, E, (rest, 3)))
    return np.concatenate(parts).astype(np.int32) & (E - 1)


# ---------------------------------------------------------------------------------------------------------------- rays --
def _classes(rng, pts):
    """origins of four classes in turn from the points `pts` (n, 3): integral, half-integral, generic fractional, and one
    extent down on every axis (negative coordinates: trunc != floor), integral and fractional alternating"""
    p = np.asarray(pts, np.float64).copy()
    k = np.arange(len(p)) % 4
    fl = np.floor(p)
    p[k == 0] = fl[k == 0]
    p[k == 1] = fl[k == 1] + 0.5
    down = k == 3
    p[down] = np.where((np.arange(len(p)) % 8 == 3)[down, None], fl[down], p[down]) - E
    return p.astype(np.float32)


def _down(o):
    """the rows of _classes' result that lie one extent down"""
    return (np.arange(len(o)) % 4 == 3)[:, None]


def _normals(rng, n):
    d = rng.normal(size=(n, 3))
    return (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)


def _aimed(rng, n, box, near, far):
    """n rays at seeded points of box (lo, hi) from seeded points between `near` and `far` voxels off its faces, all round"""
    lo, hi = np.asarray(box[0], np.float64), np.asarray(box[1], np.float64)
    tgt = rng.uniform(lo, hi, (n, 3))
    c, h = (lo + hi) / 2, (hi - lo) / 2
    u = rng.normal(size=(n, 3))
    u /= np.abs(u).max(axis=1, keepdims=True)  # on the unit cube's surface: every face gets its share
    org = c + u * (h + rng.uniform(near, far, (n, 1)))
    return org, tgt


def _dirs_to(org32, tgt):
    # (an origin one extent down sees the same world: aim at the target's image there)
    d = tgt - (org32.astype(np.float64) + E * _down(org32))
    return (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)


def _tie_dirs():
    from test_gpu_directed_rays import tie_directions

    return tie_directions()


def singles():
    """the directed rays, built and not sampled: {name: (origins, dirs)}"""
    S = {}
    # inside the 16^3 mirror: every step lands in the mirror and is reflected
    S["inside_mirror"] = (np.array([[584.5, 56.5, 536.5], [584.0, 56.0, 536.0], [577.25, 49.75, 542.5]], np.float32),
                          np.array([[0.6, 0.3, -0.7], [1.0, 1.0, 1.0], [-0.2, 0.9, 0.4]], np.float32))
    # one voxel in front of every face of the uniform mirror and of the 16^3 glass, nearly straight and slanted
    o, d = [], []
    for lo in (MIRROR16, GLASS16):
        c = np.array(lo, np.float64) + 8.5
        for a in range(3):
            for s in (1.0, -1.0):
                p = c.copy()
                p[a] = lo[a] - 0.5 if s > 0 else lo[a] + 16.5
                for slant in (2.0 ** -10, 0.3):  # (an exactly axial ray's other crossings are NaN: castRayFromCam then steps in z)
                    v = np.full(3, slant)
                    v[(a + 1) % 3] *= -0.5
                    v[a] = s
                    o.append(p)
                    d.append(v)
    S["faces"] = (np.array(o, np.float32), np.array(d, np.float32))
    # tied diagonals into the mirror room's corners and edges, from integral and half-integral origins
    o, d = [], []
    c = np.array([543.0, 53.0, 543.0])
    tri = [(sx, sy, sz) for sx in (1, -1) for sy in (1, -1) for sz in (1, -1)]
    duo = [tuple(np.roll((sx, sy, 0), r)) for sx in (1, -1) for sy in (1, -1) for r in range(3)]
    for v in tri + duo:
        for half in (0.0, 0.5):
            o.append(c + 9.0 * np.array(v) + half)
            d.append(v)
    S["room_ties"] = (np.array(o, np.float32), np.array(d, np.float32))
    # along +x through the water that spans x = 1023 -> 1024
    # (the last one exactly axial: its y and z crossings are NaN, and castRayFromCam steps in z for ever)
    S["wrap_x"] = (np.array([[1010.5, 61.5, 601.5], [1010.5, 61.5, 601.5], [-13.5, 61.5, 601.5], [1010.5, 61.5, 601.5]], np.float32),
                   np.array([[1.0, 2.0 ** -12, 2.0 ** -13], [1.0, 0.02, -0.01], [1.0, -(2.0 ** -12), 2.0 ** -13], [1.0, 0.0, 0.0]], np.float32))
    return S


def _budget_rays(S):
    """rays whose S-th step lands in a refractive region (the water cube, the 16^3 glass) or on a mirror (the 16^3 one): the
    `steps > 0` boundary; along each axis' negative and positive direction, barely slanted"""
    o, d = [], []
    for lo in (CUBE, GLASS16, MIRROR16):
        for j in range(0, 16, 3):
            for a, s in ((0, 1.0), (2, -1.0), (1, -1.0)):
                for slant in (2.0 ** -20, 2.0 ** -12):
                    p = np.array(lo, np.float64) + np.array([5.5, 9.5, 3.5])
                    # the first voxel of the block along the ray is step S - j: the ray ends j voxels inside
                    p[a] = lo[a] - (S - j) + 0.5 if s > 0 else lo[a] + 15 + (S - j) + 0.5
                    v = np.full(3, slant)
                    v[a] = s
                    o.append(p)
                    d.append(v)
    return np.array(o, np.float32), np.array(d, np.float32)


_BATTERIES = None


def batteries():
    """{name: (origins (n, 3) f32, dirs (n, 3) f32)}: the sampled sets room / mirrors / glass / water / wrap, the rays that
    end on the budget's boundary, and the directed singles; the same arrays on every call"""
    global _BATTERIES
    if _BATTERIES is not None:
        return _BATTERIES
    rng = np.random.default_rng(41)
    ties = _tie_dirs()
    B = {}

    # room: from inside the closed mirror room, seeded normals and the tie set
    n = 1500
    lo, hi = np.array(ROOM_IN[0]) + 1, np.array(ROOM_IN[1]) - 1
    org = _classes(rng, rng.uniform(lo, hi, (n, 3)))
    d = _normals(rng, n)
    d[::4] = ties[rng.integers(0, len(ties), len(d[::4]))]
    B["room"] = (org, d)

    # mirrors: the uniform 16^3 and 4^3 mirrors from all round, and from the gaps between the 16^3 mirror and its
    # neighbours (the 4^3 mirror at +x, the 16^3 glass at +z): reflections that end on the other block
    parts_o, parts_d = [], []
    for name, k in (("mirror16", 450), ("mirror4", 250)):
        o, t = _aimed(rng, k, BOXES[name], 1.0, 24.0)
        o = _classes(rng, o)
        parts_o.append(o)
        parts_d.append(_dirs_to(o, t))
    k = 300
    o = _classes(rng, np.stack([rng.uniform(592.5, 599.5, k), rng.uniform(50, 58, k), rng.uniform(538, 546, k)], 1))
    t = np.stack([np.full(k, 592.0), rng.uniform(50, 58, k), rng.uniform(538, 546, k)], 1)
    parts_o.append(o)
    parts_d.append(_dirs_to(o, t))
    o = _classes(rng, np.stack([rng.uniform(576, 592, k), rng.uniform(48, 64, k), rng.uniform(544.5, 559.5, k)], 1))
    t = np.stack([rng.uniform(576, 592, k), rng.uniform(48, 64, k), np.full(k, 544.0)], 1)
    parts_o.append(o)
    parts_d.append(_dirs_to(o, t))
    B["mirrors"] = (np.concatenate(parts_o), np.concatenate(parts_d))

    # glass: every glass structure from all round; some rays at the mirror and the plain voxel inside the 16^3 block
    parts_o, parts_d = [], []
    for name, k in (("glass16", 800), ("glass4", 300), ("pane_y", 300), ("pane_z", 300)):
        o, t = _aimed(rng, k, BOXES[name], 1.0, 20.0)
        o = _classes(rng, o)
        parts_o.append(o)
        parts_d.append(_dirs_to(o, t))
    for vox in (GLASS16_MIRROR, GLASS16_PLAIN):
        o, _ = _aimed(rng, 150, BOXES["glass16"], 1.0, 12.0)
        o = _classes(rng, o)
        parts_o.append(o)
        parts_d.append(_dirs_to(o, np.array(vox) + rng.uniform(0.2, 0.8, (150, 3))))
    B["glass"] = (np.concatenate(parts_o), np.concatenate(parts_d))
    B["glass"][1][::10] = ties[rng.integers(0, len(ties), len(B["glass"][1][::10]))]

    # water: the standing cube from all round (its sides and bottom), the pool from above, from its sides and from inside
    parts_o, parts_d = [], []
    o, t = _aimed(rng, 1000, BOXES["cube"], 1.0, 20.0)
    o = _classes(rng, o)
    parts_o.append(o)
    parts_d.append(_dirs_to(o, t))
    o, t = _aimed(rng, 900, ((POOL[0], 41, POOL[0]), (POOL[1], 47, POOL[1])), 1.0, 16.0)
    o[:, 1] = np.maximum(o[:, 1], 41.2)  # (not from under the bed)
    o = _classes(rng, o)
    parts_o.append(o)
    parts_d.append(_dirs_to(o, t))
    k = 600  # from inside the pool's water, half of them at the bed's mirrors
    o = _classes(rng, np.stack([rng.uniform(625, 655, k), rng.uniform(42, 47, k), rng.uniform(625, 655, k)], 1))
    dd = _normals(rng, k)
    pm = np.array(pool_mirrors(), np.float64)
    dd[::2] = _dirs_to(o, pm[rng.integers(0, len(pm), k)] + rng.uniform(0.2, 0.8, (k, 3)))[::2]
    parts_o.append(o)
    parts_d.append(dd)
    B["water"] = (np.concatenate(parts_o), np.concatenate(parts_d))
    B["water"][1][::10] = ties[rng.integers(0, len(ties), len(B["water"][1][::10]))]

    # wrap: the water that spans x = 1023 -> 1024, the plain voxel behind it and the glass block before it, from both sides
    k = 600
    o, t = _aimed(rng, k, BOXES["wrap"], 1.0, 16.0)  # (coordinates beyond 1023: the same world, wrapped)
    o = _classes(rng, o)
    B["wrap"] = (o, _dirs_to(o, t))

    # budget: ends on the `steps > 0` boundary at S = 300 and at S = 40
    o3, d3 = _budget_rays(300)
    o4, d4 = _budget_rays(40)
    B["budget"] = (np.concatenate([o3, o4]), np.concatenate([d3, d4]))

    sg = singles()
    B["singles"] = (np.concatenate([v[0] for v in sg.values()]), np.concatenate([v[1] for v in sg.values()]))
    B = {k: (np.ascontiguousarray(o, np.float32), np.ascontiguousarray(d, np.float32)) for k, (o, d) in B.items()}
    for o, d in B.values():
        assert o.shape == d.shape and np.isfinite(o).all() and not np.isnan(d).any()
        o.setflags(write=False)
        d.setflags(write=False)
    assert sum(len(o) for o, _ in B.values()) < 10000
    _BATTERIES = B
    return B


def event_counts(r):
    """the event classes of an oracle shade_rays result, as {name: rays}"""
    nrefl, bent, tints, hit = r["nrefl"], r["bent"] != 0, r["tints"], r["hit"] != 0
    ev = (nrefl > 0) | bent | (tints > 0)
    c = {"refl1": nrefl == 1, "refl2": nrefl == 2, "refl3+": nrefl >= 3, "refl10+": nrefl >= 10, "bent": bent,
         "liq_bend": bent & (r["liq_bend"] != 0),
         "bend_then_refl": bent & (nrefl > r["refl_at_bend"]), "refl_then_bend": bent & (r["refl_at_bend"] > 0),
         "tints8+": tints >= 8, "hit_after_event": ev & hit, "miss_after_event": ev & ~hit,
         "last_step_mirror": hit & (r["steps"] == 0) & ((r["flags"] & 7) == 3),
         "last_step_refractive": hit & (r["steps"] == 0) & ((r["flags"] & 7) == 5)}
    for f, name in enumerate(("+x", "-x", "+y", "-y", "+z", "-z")):
        c["bend" + name] = r["bend_face"] == f
        c["liq_bend" + name] = (r["bend_face"] == f) & (r["liq_bend"] != 0)
    return {k: int(v.sum()) for k, v in c.items()}


# -------------------------------------------------------------------------------------------------------------- frames --
FRAME_W, FRAME_H = 96, 64
NARROW = 0.3  # projection plane width of the one-octant poses: every pixel's direction keeps the camera's signs
# (name, camera position, camera direction, ppx or None for the reference's plane).  The narrow poses cover the eight sign
# octants (the straight trace's compiled-octant instances); the wide ones mix signs within the frame (per-wave flags).
FRAME_POSES = [
    ("room_integral", (543.0, 53.0, 543.0), (1.0, 0.8, 0.9), NARROW),            # + + +
    ("room_half", (543.5, 50.5, 541.5), (-1.0, -0.6, -0.8), NARROW),             # - - -
    ("room_fractional", (538.3, 58.7, 550.9), (0.9, -0.7, -0.8), NARROW),        # + - -  at the pane and the water
    ("room_wide", (542.3, 52.7, 543.9), (0.8, -0.1, 0.2), None),
    ("room_pillar", (546.5, 52.5, 552.5), (-0.55, -0.55, -0.65), None),          # the plain pillar's sunward faces, unreflected
    ("mirrors", (612.5, 44.5, 556.5), (-1.0, 0.45, -0.75), NARROW),              # - + -  the 4^3 mirror before the 16^3 one
    ("mirrors_wide", (610.25, 58.5, 551.75), (-1.0, -0.1, -0.45), None),
    ("under_cube", (629.5, 36.5, 589.25), (-0.6, 1.0, 0.5), NARROW),             # - + +  up through the cube's bottom face
    ("pool", (620.3, 60.2, 618.6), (1.0, -0.8, 1.0), NARROW),                    # + - +  down into the pool
    ("pool_wide", (640.5, 52.5, 618.5), (0.1, -0.6, 1.0), None),
    ("wrap", (1006.5, 57.5, 608.5), (1.0, 0.15 * 2.5, -0.45), NARROW),           # + + -  through the water across x = 1023 -> 1024
    ("wrap_down", (12.25 - E, 66.5 - E, 592.5 - E), (-1.0, -0.5, 0.7), NARROW),  # - - +  from the other side, one extent down
]


def frame_rays(oracle_mod, pose, W=FRAME_W, H=FRAME_H):
    """(origins, dirs, normalised camera direction, ppx, ppy) of a pose's frame, the oracle's pixel directions in record order"""
    _, org, cd, ppx = pose
    cam = oracle_mod.normalize(cd)
    px, py = oracle_mod.proj_plane(W, H)
    if ppx is not None:
        px, py = ppx, ppx * H / W
    dirs = np.array([oracle_mod.pixel_dir(cam, px, py, W, H, i % W, i // W) for i in range(W * H)], np.float32)
    return np.tile(np.array(org, np.float32), (W * H, 1)), dirs, cam, px, py
