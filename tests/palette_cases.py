"""Large palettes: the cases tests/test_palette_host.py and tests/test_gpu_palette.py share.  Material ids are 16 bits wide
everywhere (a palette holds up to 65535 entries, ids up to 65534 = 0xFFFE) and the other fixtures use ids up to 22; the
cases here put the same scenes on the ids where a width goes wrong: the first word boundary of a bit table (31 / 32), the
wire formats' 12-bit limit (4095 / 4096), the sign bit of a 16-bit id (0x7FFF / 0x8000) and the cap (65534, next to the
volume builder's C_MIXED = 0xFFFF).

Two routes to a high id:
  preload()             interns k throw-away materials into a World before a scene is put: the scene's ids shift up by k.
                        The oracle stores flags and colour per voxel and has no palette, so its tree of the unshifted scene
                        is the reference for every shift.
  WIDE_TABLE, HIGH/WORD a 65535-entry palette for the volume builder, and lookups that carry volume_cases' source ids 1..5
                        onto its boundary ids, keeping every structure volume_cases plants."""
import numpy as np

import cavern
import hall
import volume_cases as vc

EMPTY = (0, 0xFFFFFFFFFFFFFFFF, 0.0)
NO_COLOUR = 0xFFFFFFFFFFFFFFFF
CAP = 65534                     # the highest id: svo_put_block interns up to 65534 distinct blocks
REFLECTIVE, REFRACTIVE, LUMINESCENT, LIQUID = 0x2, 0x4, 0x8, 0x10

# ---------------------------------------------------------------------------------------------------------- preload --
FILLER_IDENT = 0x1FFF           # the fillers' low 13 bits (cavern.ident): an id no scene uses
assert FILLER_IDENT not in hall.ALL_IDS and FILLER_IDENT > 1000 + 37 and FILLER_IDENT > 950  # (cavern's ids end at 1036)


def filler_colours(k):
    """k distinct colours, none of them ~0 and none a cavern.colour() / hall.colour() of a scene (those carry their id in
    the low 13 bits; these carry FILLER_IDENT there and the filler's number above)"""
    j = np.arange(1, k + 1, dtype=np.uint64)
    return (j << np.uint64(13)) | np.uint64(FILLER_IDENT)


def preload(world, k, where):
    """intern k filler blocks (flags 0, distinct colours) at the voxel `where`, which the scene leaves empty, then delete
    the voxel: the palette holds 1 + k entries and the world's content is unchanged"""
    if k:
        world.put_blocks(np.tile(np.asarray(where, np.int32), (k, 1)), np.zeros(k, np.uint32), filler_colours(k))
        world.delete_block(*[int(v) for v in where])


def scene_materials(world):
    """M: the materials of an (unshifted) scene"""
    return len(world.build().palette()) - 1


SHIFT_NAMES = ("word", "wire_last", "wire_over", "sign", "cap")


def SHIFTS(M):
    """{name: K}: the preloads that put a scene of M materials (ids K + 1 .. K + M) on each boundary"""
    return {
        "word": 31 - 3,          # ids straddle 31 / 32: the first word boundary of a bit table (k_vol_classes' in-view bits)
        "wire_last": 4095 - M,   # last id 4095, palette size exactly 4096: the most the 12-bit wire fields carry
        "wire_over": 4096 - M,   # palette size 4097, last id 4096: one past the wire limit (SVO_ERANGE)
        "sign": 32768 - 5,       # ids straddle 0x7FFF / 0x8000: a sign-extended or 15-bit id shows
        "cap": CAP - M,          # last id 65534 = 0xFFFE: the cap, one below the builders' MIXED marker
    }


# ----------------------------------------------------------------------------------------------------------- growth --
# the voxels of the palette-growth tests (svo_tree_update on the CPU, svo_tree_sync on the GPU): on the axis of
# hall.FRAME_POSES' room_fractional, inside the mirror room; (flags, colour id) in the order put: the mirror takes the
# highest id
GROWTH = [((546, 52, 544), 0, 200), ((544, 53, 545), hall.F_GLASS, 201), ((543, 54, 546), hall.F_MIRROR, 202)]


def grow(world):
    """put the three voxels of new materials; returns the points"""
    for at, flags, cid in GROWTH:
        world.put_block(*at, flags, int(hall.colour(cid)))
    return np.array([g[0] for g in GROWTH], np.int32)


# ------------------------------------------------------------------------------------------------------- WIDE_TABLE --
N_WIDE = 65535
# flagged entries at high and boundary ids.  The three entries without a colour are stored in no view; a palette interns
# blocks by (flags, colour, metadata), so they differ in flag bits the casts do not read (no bit of flags & 0x17)
WIDE_LIQUID = (64, 4096, 0x8001, 65533)
WIDE_NO_COLOUR = {63: 0, 0x8002: LUMINESCENT, 65532: 0x40}
WIDE_MIRROR, WIDE_GLASS = 0x8003, 65531


def _wide_table():
    i = np.arange(N_WIDE, dtype=np.uint64)
    r, g = (i * np.uint64(37) + np.uint64(60)) % np.uint64(256), (i * np.uint64(91) + np.uint64(30)) % np.uint64(256)
    col = (r << np.uint64(55)) | (g << np.uint64(34)) | (i << np.uint64(13)) | np.uint64(0x1FFE)  # unique: the id in bits 13..28
    flags = np.zeros(N_WIDE, np.uint32)
    flags[list(WIDE_LIQUID)] = LIQUID | REFRACTIVE
    for k, f in WIDE_NO_COLOUR.items():
        flags[k], col[k] = f, NO_COLOUR
    flags[WIDE_MIRROR], flags[WIDE_GLASS] = REFLECTIVE, REFRACTIVE
    return [(0, 0)] + list(zip(flags[1:].tolist(), col[1:].tolist()))


WIDE_TABLE = _wide_table()
assert len(WIDE_TABLE) == N_WIDE and len(set(WIDE_TABLE[1:])) == N_WIDE - 1

# volume_cases' source ids 1..5 -> WIDE_TABLE ids (the fifth is the liquid)
HIGH = (0x7FFF, 0x8000, 65534, 4095, 0x8001)
WORD = (31, 32, 33, 62, 64)     # (62, not 63: 63 has no colour and would be stored in no view)
LOOKUPS = {"HIGH": HIGH, "WORD": WORD}
WORD_TABLE = WIDE_TABLE[:65]    # WORD's palette: 65 entries, a bit table with a partial last word
for _L in LOOKUPS.values():
    assert WIDE_TABLE[_L[4]][0] & LIQUID and vc.TABLE[5][0] & LIQUID
    assert all(WIDE_TABLE[m][0] == 0 and WIDE_TABLE[m][1] != NO_COLOUR for m in _L[:4])


def table_of(lookup_name):
    return WIDE_TABLE if lookup_name == "HIGH" else WORD_TABLE


def extras_of(lookup_name):
    """the flagged ids besides the lookup's own that a volume of this lookup is sprinkled with: (ids, of them without colour)"""
    if lookup_name == "HIGH":
        return (0x8002, 65532, WIDE_MIRROR, WIDE_GLASS, 65533, 4096), (0x8002, 65532)
    return (63,), (63,)


def stored_palette(table):
    """the palette a tree of `table` carries: entry 0 the empty block, flags stored as 1 | flags"""
    return [EMPTY] + [(1 | f, c, 0.0) for f, c in table[1:]]


def through(vol, lookup):
    """a volume of source ids 0..5 carried onto the lookup's ids"""
    assert int(vol.max()) <= 5
    return np.array((0,) + tuple(lookup), np.uint16)[vol]


def puts_through(puts, lookup):
    """volume_cases' oracle puts [(x, y, z, source id, level)] carried onto the lookup's ids"""
    return [(x, y, z, lookup[i - 1], level) for x, y, z, i, level in puts]


def planted(nx, ny, nz, origin, seed, lookup_name):
    """volume_cases.planted() through a lookup, sprinkled with the lookup's extra ids where no structure is planted.  The
    structures lie where the volume is the same for every seed; a sprinkle falls only on voxels that differ between two
    seeds, so every planted structure survives"""
    src, has_big = vc.planted(nx, ny, nz, origin, seed)
    other, _ = vc.planted(nx, ny, nz, origin, seed + 1000)
    vol = through(src, LOOKUPS[lookup_name])
    free = np.argwhere(src != other)
    rng = np.random.default_rng(seed)
    ids, _ = extras_of(lookup_name)
    pick = free[rng.choice(len(free), 40 * len(ids), replace=False)]
    for n, m in enumerate(ids):
        z, y, x = pick[40 * n:40 * (n + 1)].T
        vol[z, y, x] = m
    return vol, src, has_big


def voxel_puts(vol, origin, table):
    """volume_cases.voxel_puts without the voxels whose id has no colour (the oracle holds no such block)"""
    return [p for p in vc.voxel_puts(vol, origin) if table[p[3]][1] != NO_COLOUR]


def world_with_palette(rt, levels, table):
    """an empty World whose palette equals `table` entry for entry (flags stored as 1 | flags): the entries are interned in
    order at a scratch voxel, which is then deleted"""
    w = rt.World(levels)
    n = len(table) - 1
    w.put_blocks(np.zeros((n, 3), np.int32), np.array([t[0] for t in table[1:]], np.uint32), np.array([t[1] for t in table[1:]], np.uint64))
    w.delete_block(0, 0, 0)
    return w


def decoded(tree):
    """(flags, colours) of a tree's palette as arrays: test_gpu_parity.compare's optional argument, decoded once per tree"""
    pal = tree.palette()
    return np.array([p[0] for p in pal], np.uint32), np.array([p[1] for p in pal], np.uint64)


def cavern_is_clear_of_fillers():
    """no filler colour is a colour of tests/cavern.py's world either"""
    used = set(np.concatenate([c for _, _, c, _ in cavern._puts(True)]).tolist())
    return not (used & set(filler_colours(64).tolist())) and all(int(cavern.ident(c)) != FILLER_IDENT for c in used)
