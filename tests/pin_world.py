"""The pin world P: a put-only world that the reference's own compiled tree (oracle/_ref/ref_core) can build, so that
its lookups and casts are recorded from the reference itself (tests/golden/pins_P.npz) and compared with the oracle,
the product's host side and the GPU casts (tests/test_reference_pins.py, tests/test_gpu_reference_pins.py).

It is tests/cavern.py's tall world without the dust (16^3 / 64^3 / 4^3 leaves and single voxels, an overhang, the
one-voxel tower to row 1023, both wrap corners, far voxels in otherwise empty root children, mirror and glass voxels),
plus LIQUID voxels and a LIQUID 4^3 block (flags 0x14: castRayFromCam passes through them) and a reflective and a
refractive 4^3 block.

Reference-safe by construction (oracle/REFERENCE_PINS.md): the reference's putBlock faults when the voxel lies inside a
coarser leaf, and replacing a branch by a leaf frees child arrays that its allocator hands back wrongly.  So every put
of a safe list targets a region that is empty or already a leaf of exactly that level; check_reference_safe() decides
that from the list alone, with a plain occupancy record and no tree."""
import numpy as np

import cavern

LEVELS = cavern.LEVELS
E = cavern.E
F_LIQUID = 0x14             # REFRACTIVE | LIQUID, as genWorld's water (world_gen.cpp:26)
POOL = (440, 16, 270)       # liquid voxels on the floor: 30 x 4 x 30 from this corner
CURTAIN = (360, 16, 380)    # a liquid wall one voxel thick: x = 360, 24 rows, z in [380, 400)
LIQUID_BLOCK = (300, 100, 300)  # a liquid 4^3 leaf in mid air
BEHIND = (364, 20, 384)     # a solid 4^3 block behind the curtain (seen through it)
MIRROR_BLOCK = (460, 40, 460)   # reflective 4^3 leaf (flags 2, metadata 0.94 as the reference's hotbar)
GLASS_BLOCK = (300, 40, 280)    # refractive 4^3 leaf (flags 4, metadata 1.5)


def puts():
    """the world as cavern._puts gives it: [(points (n, 3), flags (n,), colours (n,), level, metadata)].  Colour ids
    above cavern's: 1100 pool, 1110 curtain, 1120 liquid block, 1130 the block behind the curtain, 1140 mirror block,
    1150 glass block"""
    out = [(p, f, c, lv, 0.0) for p, f, c, lv in cavern._puts(True) if cavern.ident(c).min() < 1000]  # (without the dust)
    assert len(out) == len(cavern._puts(True)) - 1

    def add(pts, ids, level, flags, meta=0.0):
        p = np.asarray(pts, np.int32).reshape(-1, 3)
        out.append((p, np.full(len(p), flags, np.uint32), np.broadcast_to(cavern.colour(ids), (len(p),)).copy(), level, meta))

    x, y, z = POOL
    add([(x + i, y + j, z + k) for i in range(30) for j in range(4) for k in range(30)], 1100, 6, F_LIQUID)
    x, y, z = CURTAIN
    add([(x, y + j, z + k) for j in range(24) for k in range(20)], 1110, 6, F_LIQUID)
    add([LIQUID_BLOCK], 1120, 5, F_LIQUID)
    add([BEHIND], 1130, 5, 0)
    add([MIRROR_BLOCK], 1140, 5, cavern.F_MIRROR, 0.94)
    add([GLASS_BLOCK], 1150, 5, cavern.F_GLASS, 1.5)
    return out


def check_reference_safe(put_list, levels=LEVELS):
    """ValueError unless every put of [(points, flags, colours, level, ...)] targets a region that is empty or already
    a leaf of exactly that level (coordinates wrap as the tree's do).  Returns the number of puts."""
    leaves = {lv: set() for lv in range(1, levels + 2)}    # level -> cells stored as leaves of that level
    branches = {lv: set() for lv in range(1, levels + 2)}  # level -> cells that hold finer leaves
    n = 0
    for entry in put_list:
        pts, level = np.asarray(entry[0], np.int64).reshape(-1, 3), int(entry[3])
        if not 2 <= level <= levels + 1:
            raise ValueError("level %d: a put replaces the root or lies below the voxels" % level)
        for x, y, z in (pts & ((1 << (2 * levels)) - 1)).tolist():
            cell = lambda lv: (x >> (2 * (levels + 1 - lv)), y >> (2 * (levels + 1 - lv)), z >> (2 * (levels + 1 - lv)))  # noqa: E731
            for lv in range(1, level):
                if cell(lv) in leaves[lv]:
                    raise ValueError("put %d at (%d, %d, %d) level %d lies inside a level-%d leaf: the reference's putBlock "
                                     "faults there" % (n, x, y, z, level, lv))
            if cell(level) in branches[level]:
                raise ValueError("put %d at (%d, %d, %d) level %d replaces a branch: the reference frees its child arrays"
                                 % (n, x, y, z, level))
            leaves[level].add(cell(level))
            for lv in range(1, level):
                branches[lv].add(cell(lv))
            n += 1
    return n


def ref_commands():
    """the world as a command list for oracle.ref_core_run (a clean root, then the puts in order), checked first"""
    pl = puts()
    check_reference_safe(pl)
    return [("clean",)] + [("put", p, f, c, lv, m) for p, f, c, lv, m in pl]


def oracle_tree(oracle_mod):
    T = oracle_mod.Tree(LEVELS)
    oracle_mod.lib().orc_init_clean_root(T.h)
    for pts, flags, colours, level, meta in puts():
        for (x, y, z), f, c in zip(pts.tolist(), flags.tolist(), colours.tolist()):
            assert T.put_block(x, y, z, f, c, meta, level) == 0
    return T


def product_world(rt):
    w = rt.World(LEVELS)
    for pts, flags, colours, level, meta in puts():
        w.put_blocks(pts, flags, colours, metadata=meta, level=level)
    return w


def probe_points(n, seed=11):
    """cavern.probe_points plus voxels in and next to the liquid and the new blocks, some of all of them moved whole
    extents away (negative and beyond-extent coordinates: lookups wrap)"""
    rng = np.random.default_rng(seed)
    k = n // 16
    parts = [cavern.probe_points(n - 6 * k)]
    for (x, y, z), (nx, ny, nz) in ((POOL, (30, 4, 30)), (CURTAIN, (1, 24, 20)), (LIQUID_BLOCK, (4, 4, 4)), (BEHIND, (4, 4, 4)),
                                    (MIRROR_BLOCK, (4, 4, 4)), (GLASS_BLOCK, (4, 4, 4))):
        parts.append(np.stack([rng.integers(x - 2, x + nx + 2, k), rng.integers(y - 2, y + ny + 2, k), rng.integers(z - 2, z + nz + 2, k)], 1))
    p = np.concatenate(parts).astype(np.int64)
    move = rng.integers(0, 4, len(p)) == 0
    p[move] += rng.integers(-2, 3, (int(move.sum()), 3)) * E
    return p.astype(np.int32)
