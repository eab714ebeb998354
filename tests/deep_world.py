"""Deep worlds that are not heightfields: the 6- and 7-level (4096^3, 16384^3) counterpart of tests/cavern.py, put block
by block into the product's World and the oracle's tree alike; the fixture of tests/test_deep_world_host.py and
tests/test_gpu_deep_world.py.  Levels as putBlock numbers them: levels + 1 = a voxel, each step down 4 x wider, 2 = a root
child.  With E = 4^levels and H = E / 2 the cavern area is x, z in [H, H + 1024): the top coordinate bit is in use.

Contents (layout(levels) holds the coordinates): a floor of 64^3 blocks (rows 0..63); four staircases whose steps are 16,
64, 256 and 1024 columns wide and one block higher each, so that adjacent blocks of every column-ceiling level have
ceilings one block apart (no dust over them); floating solids of 64^3, 256^3, at 7 levels 1024^3 (in another root child)
and one whole root child; seeded dust, some of it inside the floating solids (those leaves split: a solid with one voxel
of another id in it); a one-voxel roof plate with holes, its corner off every block boundary; a one-voxel tower up to row
E - 1; the wrap corners; far voxels in otherwise empty root children, one of them at (H - 1, y, H - 1); mirror, glass and
liquid voxels on the floor.  Nothing is ever erased: later puts only overwrite or split."""
from types import SimpleNamespace

import numpy as np

from cavern import colour, ident  # noqa: F401  (the same colour coding: a small id in the low 13 bits)

EMPTY = np.uint64(0xFFFFFFFFFFFFFFFF)
LEVELS = (6, 7)
AREA = 1024
FLOOR_TOP = 63
DUST_N, DUST_LO, DUST_TOP = 3000, 64, 1500
DUST_Z = (192, 768)          # dust lies over z in [H + 192, H + 768): the staircases' columns hold none
ROOF_Y, ROOF_N = 300, 70
F_MIRROR, F_GLASS, F_LIQUID = 0x2, 0x4, 0x10
STAIR_STEPS = {16: 12, 64: 6, 256: 3}   # steps per staircase (the 1024-column one: 3 at 7 levels; one at 6, where its
# blocks are root children and the next column of them holds the wrap corner)


def layout(levels):
    """the coordinates of everything, for levels 6 or 7"""
    assert levels in (6, 7)
    E = 1 << (2 * levels)
    H, q = E // 2, E // 4
    g = SimpleNamespace(levels=levels, E=E, H=H, q=q)
    # staircases: width -> (x0, z0, depth in z, number of steps, first block row); step i covers x in [x0 + w i, + w) and is
    # solid from the floor (rows 0..) up to row stair_top(g, w, i)
    g.stairs = {16: (H + 16, H + 64, 32, STAIR_STEPS[16], 64), 64: (H + 256, H + 128, 64, STAIR_STEPS[64], 64),
                256: (H, H + 768, 256, STAIR_STEPS[256], 0), 1024: (H, H + 1024, 1024, 3 if levels == 7 else 1, 0)}
    # an apron of floor (64^3 blocks, rows 0..63) beside and behind the widest staircase, in 1024 x 1024 tiles (x, z): what
    # descends from its steps away from the area lands on something
    g.apron = ([(H + 3072, H + 1024)] + [(H + 1024 * i, H + 2048) for i in range(4)]) if levels == 7 else [(H + 1024, H + 1024)]
    g.big64 = (H + 384, 320, H + 448)
    g.big256 = (H + 512, 512, H + 256)
    g.big1024 = (H + 4096, 1024, H) if levels == 7 else None   # root child (3, 0, 2): not the cavern's
    g.root_solid = (q, 2 * q, 3 * q)                            # root child (1, 2, 3), put as one block
    g.roof = (H + 322, ROOF_Y, H + 361)
    g.mirror = (H + 400, 64, H + 296)      # 8 x 8 mirror voxels on the floor, low corner
    g.glass = (H + 420, 64, H + 296)       # a glass wall: x fixed, 12 rows, 12 voxels in z
    g.liquid = (H + 430, 64, H + 296)      # a 6 x 6 pool lying on the floor
    g.brick63 = (H + 600, 200, H + 300)    # a 4^3 brick with its last voxel (+3, +3, +3) missing
    g.tower = (H + 900, H + 600)
    g.corners = [(0, 0, 0), (E - 1, E - 1, E - 1)]
    g.far = [(H - 1, 777, H - 1), (40, q + 440, 3 * q + 900), (3 * q + 900, 50, 40), (100, 3 * q + 5, q + 600),
             (3 * q + 1000, 2 * q + 200, 1000)]
    return g


def stair_top(g, w, i):
    """the top row of step i of the staircase whose steps are w columns wide"""
    return g.stairs[w][4] + w * (i + 1) - 1


def dust_points(levels):
    """seeded dust over the area's middle strip, then a few voxels inside each floating solid of 256^3 and more"""
    g = layout(levels)
    rng = np.random.default_rng(2026)
    p = np.stack([rng.integers(g.H, g.H + AREA, DUST_N), rng.integers(DUST_LO, DUST_TOP + 1, DUST_N),
                  rng.integers(g.H + DUST_Z[0], g.H + DUST_Z[1], DUST_N)], 1)
    extra = [np.asarray(g.big256) + rng.integers(1, 255, (2, 3))]
    if g.big1024:
        extra.append(np.asarray(g.big1024) + rng.integers(1, 1023, (3, 3)))
    return np.concatenate([p] + extra).astype(np.int32)


def inside(points, corner, size):
    p, c = np.asarray(points), np.asarray(corner)
    return ((p >= c) & (p < c + size)).all(1)


def _roof(g):
    x0, y, z0 = g.roof
    xs, zs = np.meshgrid(np.arange(x0, x0 + ROOF_N), np.arange(z0, z0 + ROOF_N), indexing="ij")
    keep = ~((xs % 4 == 1) & (zs % 4 == 2))
    return np.stack([xs[keep], np.full(keep.sum(), y), zs[keep]], 1)


def _stair_blocks(g, w):
    x0, z0, depth, n, y0 = g.stairs[w]
    return [(x0 + w * i, y0 + w * j, z0 + w * k) for i in range(n) for j in range(i + 1) for k in range(depth // w)]


def puts(levels, light=False):
    """the world as a list of (points (n, 3), flags (n,), colours (n,), level); later entries overwrite earlier ones.
    light: the subset whose blocks are at most 64^3 (the 16-column staircase, the 64^3 block, the brick less one, roof,
    dust, tower, corners, far voxels), which the point builder can take as a voxel list.
    Colour ids: 100 floor, 110 apron, 201..204 stairs, 300 / 310 / 320 / 330 the 256^3, 1024^3, root-child and 64^3 solids, 400 the
    brick less one, 500.. roof, 600 mirror, 700 glass, 750 liquid, 800.. far voxels, 900 tower, 950 corners, 1000.. dust"""
    g = layout(levels)
    H = g.H
    out = []

    def add(pts, ids, k, flags=0):  # k: the blocks are 4^k wide
        p = np.asarray(pts, np.int32).reshape(-1, 3)
        c = np.broadcast_to(colour(ids), (len(p),)).copy()
        out.append((p, np.full(len(p), flags, np.uint32), c, levels + 1 - k))

    if not light:
        # (no floor under the 256-column staircase: its steps are 256^3 blocks from row 0)
        add([(H + 64 * i, 0, H + 64 * j) for i in range(16) for j in range(16) if not (j >= 12 and i < 12)], 100, 3)
        add([(x + 64 * i, 0, z + 64 * j) for x, z in g.apron for i in range(16) for j in range(16)], 110, 3)
    add(_stair_blocks(g, 16), 201, 2)
    if not light:
        add(_stair_blocks(g, 64), 202, 3)
        add(_stair_blocks(g, 256), 203, 4)
        add(_stair_blocks(g, 1024), 204, 5)
        add([g.big256], 300, 4)
        if g.big1024:
            add([g.big1024], 310, 5)
        add([g.root_solid], 320, levels - 1)
    add([g.big64], 330, 3)
    bx, by, bz = g.brick63
    add([(bx + i, by + j, bz + k) for k in range(4) for j in range(4) for i in range(4)][:63], 400, 0)
    roof = _roof(g)
    add(roof, 500 + (roof[:, 0] + roof[:, 2]) % 7, 0)
    dust = dust_points(levels)
    if light:
        dust = dust[:DUST_N]
    add(dust, 1000 + np.arange(len(dust)) % 37, 0)   # (those inside the solids split their leaves)
    if not light:
        mx, my, mz = g.mirror
        add([(mx + i, my, mz + k) for i in range(8) for k in range(8)], 600, 0, F_MIRROR)
        gx, gy, gz = g.glass
        add([(gx, gy + j, gz + k) for j in range(12) for k in range(12)], 700, 0, F_GLASS)
        lx, ly, lz = g.liquid
        add([(lx + i, ly, lz + k) for i in range(6) for k in range(6)], 750, 0, F_LIQUID)
    add(g.far, 800 + np.arange(len(g.far)), 0)
    add([(g.tower[0], y, g.tower[1]) for y in range(FLOOR_TOP + 1, g.E)], 900, 0)
    add(g.corners, 950, 0)
    return out


def oracle_tree(oracle_mod, levels, put_list):
    """the oracle's tree of a put list, from a clean root (orc_init_clean_root: no region has to be left out of a comparison)"""
    T = oracle_mod.Tree(levels)
    oracle_mod.lib().orc_init_clean_root(T.h)
    put = T.put_block
    for pts, flags, colours, level in put_list:
        for (x, y, z), f, c in zip(pts.tolist(), flags.tolist(), colours.tolist()):
            assert put(x, y, z, f, c, 0.0, level) == 0
    return T


def fill(rt, oracle_mod, levels, put_list):
    """(rt.World, oracle Tree) filled from one put list"""
    w = rt.World(levels)
    for pts, flags, colours, level in put_list:
        w.put_blocks(pts, flags, colours, level=level)
    return w, oracle_tree(oracle_mod, levels, put_list)


def deep(rt, oracle_mod, levels):
    """(rt.World, oracle Tree) holding the same blocks"""
    return fill(rt, oracle_mod, levels, puts(levels))


def ceiling_model(levels, light=False, extra=None):
    """the column ceilings of the solid view from the put list alone: per 16-column block the highest occupied row (the
    maximum over the puts of y + size - 1: nothing is erased; liquid is not stored in that view), and that coarsened by
    maximum to 64, 256 and 1024 columns: four int64 arrays [z][x], -1 where nothing is stored.  extra: further voxels"""
    E = 1 << (2 * levels)
    n = E >> 4
    top = np.full((n, n), -1, np.int64)
    for pts, flags, _, level in puts(levels, light):
        s = 1 << (2 * (levels + 1 - level))
        pts = pts[(flags & F_LIQUID) == 0]
        if s >= 16:
            for x, y, z in pts.tolist():
                blk = top[z >> 4:(z + s) >> 4, x >> 4:(x + s) >> 4]
                np.maximum(blk, y + s - 1, out=blk)
        elif len(pts):
            np.maximum.at(top, (pts[:, 2] >> 4, pts[:, 0] >> 4), pts[:, 1] + s - 1)
    if extra is not None and len(extra):
        e = np.asarray(extra, np.int64)
        np.maximum.at(top, (e[:, 2] >> 4, e[:, 0] >> 4), e[:, 1])
    res = [top]
    for _ in range(3):
        m = len(res[-1]) // 4
        res.append(res[-1].reshape(m, 4, m, 4).max(axis=(1, 3)))
    return res


def probe_points(n, levels, seed=7):
    """n seeded voxels in and next to every structure, across the H boundary, and anywhere"""
    g = layout(levels)
    H, E = g.H, g.E
    rng = np.random.default_rng(seed)
    parts = []

    def box(lo, hi, k):
        parts.append(np.stack([rng.integers(lo[a], hi[a], k) for a in range(3)], 1))

    def around(pts, k):
        pts = np.asarray(pts)
        parts.append(pts[rng.integers(0, len(pts), k)] + rng.integers(-1, 2, (k, 3)) * rng.integers(0, 2, (k, 1)))  # (half of them the voxels themselves)

    k = n // 20
    box((H - 8, 0, H - 8), (H + AREA + 8, 72, H + AREA + 8), 2 * k)               # floor, its rim, the H boundary
    for w in (16, 64, 256, 1024):
        x0, z0, depth, steps, y0 = g.stairs[w]
        box((x0 - 4, 0, z0 - 4), (x0 + w * steps + 4, stair_top(g, w, steps - 1) + 6, z0 + depth + 4), k)
    for c, s in ((g.big64, 64), (g.big256, 256), (g.big1024, 1024), (g.root_solid, g.q)):
        if c:
            box([v - 6 for v in c], [v + s + 6 for v in c], k)
    box((g.roof[0] - 3, ROOF_Y - 2, g.roof[2] - 3), (g.roof[0] + ROOF_N + 3, ROOF_Y + 3, g.roof[2] + ROOF_N + 3), k)
    box((g.mirror[0] - 4, 62, g.mirror[2] - 4), (g.liquid[0] + 10, 80, g.mirror[2] + 16), k // 2)
    for pts, flags, _, _ in puts(levels):
        if flags[0]:
            around(pts, k // 4)                                                   # mirror, glass, liquid
    box((g.brick63[0] - 2, g.brick63[1] - 2, g.brick63[2] - 2), (g.brick63[0] + 6, g.brick63[1] + 6, g.brick63[2] + 6), k // 2)
    box((g.tower[0] - 2, 0, g.tower[1] - 2), (g.tower[0] + 3, E, g.tower[1] + 3), k)
    box((H - 3, 0, H - 3), (H + 3, 1000, H + 3), k)                               # both sides of the top-bit boundary
    around(dust_points(levels), 2 * k)
    around(g.far + g.corners, k)
    box((0, 0, 0), (E, E, E), n - sum(len(p) for p in parts))
    return np.concatenate(parts).astype(np.int32) & (E - 1)


def light_puts(levels):
    return puts(levels, light=True)


def light_points(levels):
    """the light world as a voxel list for the point builder: (xyz int32 (n, 3), flags, colours), in put order (a later
    entry of a voxel wins)"""
    xyz, fl, col = [], [], []
    for pts, flags, colours, level in light_puts(levels):
        s = 1 << (2 * (levels + 1 - level))
        assert s <= 64
        if s == 1:
            xyz.append(pts)
        else:
            z, y, x = np.meshgrid(np.arange(s), np.arange(s), np.arange(s), indexing="ij")
            cube = np.stack([x.ravel(), y.ravel(), z.ravel()], 1).astype(np.int32)
            xyz.append((pts[:, None, :] + cube[None, :, :]).reshape(-1, 3))
        fl.append(np.repeat(flags, s ** 3))
        col.append(np.repeat(colours, s ** 3))
    xyz = np.ascontiguousarray(np.concatenate(xyz).astype(np.int32))
    assert len(xyz) <= 1200000
    return xyz, np.concatenate(fl), np.concatenate(col)
