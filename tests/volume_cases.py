"""Dense voxel volumes for the volume builder's tests (tests/test_gpu_volume_build.py): id volumes with planted structures,
their host-built twins (an rt.World filled voxel by voxel, the only route to arbitrary content besides
svo_build_volume_gpu) and the same content in the oracle's tree.  Volumes are numpy uint16 arrays indexed [z, y, x];
`origin` is the world position (x, y, z) of element [0, 0, 0]."""
import numpy as np

from cavern import colour

LIQUID_FLAGS = 0x14  # LIQUID | REFRACTIVE, as genWorld's water
# source ids 1..5: (flags, colour); id 5 is liquid (empty in the solid view)
TABLE = [(0, 0)] + [(0, int(colour(10 + i))) for i in range(1, 5)] + [(LIQUID_FLAGS, int(colour(20)))]


def random_volume(shape_zyx, fill, seed, ids=(1, 2, 3, 4, 5)):
    rng = np.random.default_rng(seed)
    v = rng.choice(np.asarray(ids, np.uint16), size=shape_zyx)
    v[rng.random(shape_zyx) >= fill] = 0
    return v.astype(np.uint16)


def _box(vol, origin, lo, size, value):
    """vol[world box lo .. lo + size) = value (the part inside the volume)"""
    ox, oy, oz = origin
    x0, y0, z0 = lo[0] - ox, lo[1] - oy, lo[2] - oz
    vol[max(z0, 0):max(z0 + size, 0), max(y0, 0):max(y0 + size, 0), max(x0, 0):max(x0 + size, 0)] = value


def planted(nx, ny, nz, origin, seed):
    """a random volume (about 30 % filled, five materials, one liquid) with, where the box holds them:
    an aligned 4^3 of one material (a SOLID child), one with a voxel removed (BRICK | UNIFORM), one full of two
    materials (a mixed brick of 64 material entries), a 4^3 straddling the volume's +x face (its outer part reads as
    outside), and — in boxes that hold an aligned 16^3 on every axis — a 16^3 of one material (SOLID at depth 1 of a
    3-level tree) and one full of a solid material except one liquid voxel (collapses in neither view; different masks)"""
    ox, oy, oz = origin
    vol = random_volume((nz, ny, nx), 0.3, seed)

    def first_aligned(o, n, s, skip=0):
        a = -(-o // s) * s + skip * s
        return a if a + s <= o + n else None

    bx, by, bz = (first_aligned(o, n, 4) for o, n in ((ox, nx), (oy, ny), (oz, nz)))
    _box(vol, origin, (bx, by, bz), 4, 2)                      # SOLID child
    _box(vol, origin, (bx + 4, by, bz), 4, 3)                  # BRICK | UNIFORM
    vol[bz - oz + 1, by - oy + 2, bx + 4 - ox + 3] = 0
    _box(vol, origin, (bx + 8, by, bz), 4, 1)                  # mixed, full
    vol[bz - oz:bz - oz + 4, by - oy:by - oy + 2, bx + 8 - ox:bx + 12 - ox] = 4
    sx = ((ox + nx - 1) // 4) * 4                              # the last brick column: cut by the +x face unless aligned
    _box(vol, origin, (sx, by + 4, bz), 4, 2)
    big = [first_aligned(o, n, 16) for o, n in ((ox, nx), (oy, ny), (oz, nz))]
    has_big = all(b is not None for b in big)
    if has_big:
        bz2 = first_aligned(oz, nz, 16, 1)
        _box(vol, origin, big, 16, 4)
        if bz2 is not None:
            _box(vol, origin, (big[0], big[1], bz2), 16, 3)
            vol[bz2 - oz + 5, big[1] - oy + 9, big[0] - ox + 2] = 5
    return vol, has_big


def mini_cavern():
    """tests/cavern.py in miniature, 4 levels (256^3), a 256 x 64 x 256 volume at the origin: a floor of 16^3 blocks, a
    64^3 block standing in it (the box is 64 rows tall: a 64^3 block fills its height), a staircase of 16^3 blocks, a
    floating 32^3 made of eight 16^3 blocks, a one-voxel plate with holes and liquid stripes, seeded dust.  Returns
    (vol, puts): puts = [(x, y, z, source id, level)] for the oracle, levels as putBlock numbers them (5 = a voxel,
    3 = 16^3, 2 = 64^3), later entries overwriting earlier ones."""
    nx, ny, nz = 256, 64, 256
    vol = np.zeros((nz, ny, nx), np.uint16)
    puts = []

    def block(x, y, z, s, ident, level):
        vol[z:z + s, y:y + s, x:x + s] = ident
        puts.append((x, y, z, ident, level))

    for x in range(0, 256, 16):                        # floor: rows 0..15, but for the 64^3 block's footprint
        for z in range(0, 256, 16):
            if not (128 <= x < 192 and 64 <= z < 128):
                block(x, 0, z, 16, 1, 3)
    block(128, 0, 64, 64, 2, 2)                        # a 64^3 block (SOLID at depth 1)
    for i in range(3):                                 # staircase: step i is i + 1 blocks above the floor
        for j in range(i + 1):
            block(32 + 16 * i, 16 * (j + 1), 48, 16, 3, 3)
    for dx in (0, 16):                                 # floating: eight 16^3 blocks, rows 32..63
        for dy in (0, 16):
            for dz in (0, 16):
                block(64 + dx, 32 + dy, 160 + dz, 16, 4, 3)
    py, px0, pz0, pn = 41, 133, 150, 60                # plate: corner not on a block boundary, holes, liquid stripes
    for x in range(px0, px0 + pn):
        for z in range(pz0, pz0 + pn):
            if not (x % 4 == 1 and z % 4 == 2):
                ident = 5 if x % 16 == 7 else 1 + (x + z) % 3
                vol[z, py, x] = ident
                puts.append((x, py, z, ident, 5))
    rng = np.random.default_rng(2025)                  # dust above the floor (some inside the blocks: splits them)
    for x, y, z, i in zip(rng.integers(0, 256, 1200), rng.integers(16, 64, 1200), rng.integers(0, 256, 1200), rng.integers(1, 5, 1200)):
        vol[z, y, x] = i
        puts.append((int(x), int(y), int(z), int(i), 5))
    return vol, puts


def voxel_puts(vol, origin):
    """[(x, y, z, id, None)] over the non-zero voxels: the oracle's puts of a small volume"""
    z, y, x = np.nonzero(vol)
    return [(int(a) + origin[0], int(b) + origin[1], int(c) + origin[2], int(i), None) for a, b, c, i in zip(x, y, z, vol[z, y, x])]


def host_twin(rt, levels, vol, origin, view, table=TABLE, world=None):
    """(host tree of `view`, its palette, the volume in that palette's ids): an rt.World filled with put_blocks over the
    non-zero voxels at level levels + 1, built; the volume remapped to the host palette by (flags, colour), so that both
    builders number the materials alike by construction.  world: an empty World to fill instead of a new one — one whose
    palette already holds `table` entry for entry (palette_cases.world_with_palette) numbers the materials as the table
    does, and the remap is the identity"""
    w = rt.World(levels) if world is None else world
    z, y, x = np.nonzero(vol)
    ids = vol[z, y, x]
    flags = np.array([t[0] for t in table], np.uint32)
    cols = np.array([t[1] for t in table], np.uint64)
    if len(ids):
        w.put_blocks(np.stack([x + origin[0], y + origin[1], z + origin[2]], 1), flags[ids], cols[ids])
    h = w.build(view)
    pal = h.palette()
    key = {(f, c): i for i, (f, c, _) in enumerate(pal)}
    remap = np.zeros(len(table), np.uint16)
    for i in range(1, len(table)):
        remap[i] = key.get((1 | table[i][0], table[i][1]), 0)
    if world is not None:
        assert len(pal) == len(table) and np.array_equal(remap[1:], np.arange(1, len(table))), "the world's palette is not the table"
    return h, pal, remap[vol]


def oracle_twin(oracle_mod, levels, puts, table=TABLE):
    T = oracle_mod.Tree(levels)
    oracle_mod.lib().orc_init_clean_root(T.h)
    for x, y, z, i, level in puts:
        assert T.put_block(x, y, z, table[i][0], table[i][1], 0.0, levels + 1 if level is None else level) == 0
    return T


def in_view(vol, pal, view):
    """the volume with the ids a tree of `view` does not store zeroed (svo_internal.h material_in_view)"""
    keep = np.array([c != 0xFFFFFFFFFFFFFFFF and (view == 1 or not (f & 0x10)) for f, c, _ in pal], bool)
    return np.where(keep[vol], vol, 0).astype(np.uint16)
