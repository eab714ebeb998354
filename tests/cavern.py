"""A world that is not a heightfield, put block by block into the product's World and the oracle's tree alike (the way
tests/test_gpu_degenerate_trees.py::_pair does): the fixture of tests/test_cavern_host.py and
tests/test_gpu_directed_rays.py.  5 levels (1024^3); levels as putBlock numbers them: 6 = a voxel, 5 = 4^3, 4 = 16^3,
3 = 64^3.  The oracle side starts from a clean root (orc_init_clean_root), so no region has to be left out of a
comparison.  Everything lies in x, z in [256, 512) except the far voxels (and, with `tall`, the wrap corners)."""
import numpy as np

LEVELS = 5
E = 1 << (2 * LEVELS)
X0, X1 = 256, 512           # the cavern's extent in x and z
FLOOR_TOP = 15              # 16^3 blocks at rows 0..15 over the whole extent
# staircase: step i (0..STAIR_N-1) covers x in [STAIR_X0 + 16 i, +16), z in [STAIR_Z0, STAIR_Z0 + 32), solid from the
# floor up to row stair_top(i): adjacent 16-column blocks have ceilings 16 rows apart
STAIR_X0, STAIR_Z0, STAIR_N = 272, 320, 12
BIG = (384, 320, 384)       # the floating 64^3 block's low corner
ARCH_Z = 448                # the arch of 4^3 blocks: x in [288, 352), rows 24..63, z in [448, 452)
ROOF_Y, ROOF_X, ROOF_Z, ROOF_N = 300, 322, 361, 70  # a one-voxel plate (corner not on a block boundary) with holes
MIRROR = (400, 16, 296)     # 8 x 8 mirror voxels (flags 2) on the floor, low corner
GLASS = (420, 16, 296)      # a glass wall (flags 4): x = 420, 12 rows, z in [296, 308)
DUST_N, DUST_TOP = 1500, 450
FAR = [(40, 440, 900), (900, 50, 40), (700, 300, 128), (100, 5, 600), (1000, 200, 1000)]  # in otherwise empty root children
TOWER = (500, 500)          # tall: a one-voxel tower from the floor to row 1023 at this (x, z)
CORNERS = [(1023, 1023, 1023), (0, 0, 0)]  # tall: the wrap corners
F_MIRROR, F_GLASS = 0x2, 0x4


def colour(ident):
    """a Block colour (three 21-bit channels, as the shading pass reads them) for a small id, which stays in its low 13 bits"""
    i = np.asarray(ident, np.uint64)
    r, g, b = (i * 37 + 60) % 256, (i * 91 + 30) % 256, (i * 53 + 120) % 256
    return (r << np.uint64(55)) | (g << np.uint64(34)) | (b << np.uint64(13)) | i


def ident(colours):
    return np.asarray(colours, np.uint64) & np.uint64(0x1FFF)


def stair_top(i):
    return FLOOR_TOP + 16 * (i + 1)


def occupied_boxes(tall):
    """(x0, z0, nx, nz, ny) column boxes (rows 0..ny-1) that hold every stored voxel; all other columns are empty"""
    top = E if tall else 512
    boxes = [(X0, X0, X1 - X0, X1 - X0, top)]
    for x, y, z in FAR + (CORNERS if tall else []):
        boxes.append((x & ~15, z & ~15, 16, 16, E))
    return boxes


def dust_points():
    """seeded dust, none over the staircase and the floor strip around it (x < 480, z in [304, 368)): there the 16-column
    ceilings are the stair tops and the floor, 16 rows apart from block to block"""
    rng = np.random.default_rng(2024)
    p = np.stack([rng.integers(X0, X1, 2 * DUST_N), rng.integers(FLOOR_TOP + 1, DUST_TOP + 1, 2 * DUST_N), rng.integers(X0, X1, 2 * DUST_N)], 1)
    return p[~((p[:, 0] < 480) & (p[:, 2] >= 304) & (p[:, 2] < 368))][:DUST_N]


def _puts(tall):
    """the world as a list of (points (n, 3), flags (n,), colours (n,), level); later entries overwrite earlier ones.
    Colour ids: 100 floor, 200 stairs, 300 the 64^3 block, 400 arch, 500.. roof, 600 mirror, 700 glass, 800.. far voxels,
    900 tower, 950 wrap corners, 1000.. dust"""
    out = []

    def add(pts, ids, level, flags=0):
        p = np.asarray(pts, np.int32).reshape(-1, 3)
        c = np.broadcast_to(colour(ids), (len(p),)).copy()
        out.append((p, np.full(len(p), flags, np.uint32), c, level))

    g = np.arange(X0, X1, 16)
    add([(x, 0, z) for x in g for z in g], 100, 4)
    add([(STAIR_X0 + 16 * i, 16 * (j + 1), STAIR_Z0 + 16 * k) for i in range(STAIR_N) for j in range(i + 1) for k in (0, 1)], 200, 4)
    add([BIG], 300, 3)
    arch = [(x, y, ARCH_Z) for x in (288, 348) for y in range(24, 60, 4)] + [(x, 60, ARCH_Z) for x in range(288, 352, 4)]
    add(arch, 400, 5)
    xs, zs = np.meshgrid(np.arange(ROOF_X, ROOF_X + ROOF_N), np.arange(ROOF_Z, ROOF_Z + ROOF_N), indexing="ij")
    keep = ~((xs % 4 == 1) & (zs % 4 == 2))
    roof = np.stack([xs[keep], np.full(keep.sum(), ROOF_Y), zs[keep]], 1)
    add(roof, 500 + (roof[:, 0] + roof[:, 2]) % 7, 6)
    add(dust_points(), 1000 + np.arange(DUST_N) % 37, 6)  # (some fall inside the 16^3 / 64^3 blocks: putBlock splits those leaves)
    mx, my, mz = MIRROR
    add([(mx + i, my, mz + k) for i in range(8) for k in range(8)], 600, 6, F_MIRROR)
    gx, gy, gz = GLASS
    add([(gx, gy + j, gz + k) for j in range(12) for k in range(12)], 700, 6, F_GLASS)
    add(FAR, 800 + np.arange(len(FAR)), 6)
    if tall:
        add([(TOWER[0], y, TOWER[1]) for y in range(FLOOR_TOP + 1, E)], 900, 6)
        add(CORNERS, 950, 6)
    return out


def cavern(rt, oracle_mod, tall):
    """(rt.World, oracle Tree) holding the same blocks"""
    w = rt.World(LEVELS)
    T = oracle_mod.Tree(LEVELS)
    oracle_mod.lib().orc_init_clean_root(T.h)
    for pts, flags, colours, level in _puts(tall):
        w.put_blocks(pts, flags, colours, level=level)
        for (x, y, z), f, c in zip(pts.tolist(), flags.tolist(), colours.tolist()):
            assert T.put_block(x, y, z, f, c, 0.0, level) == 0
    return w, T


def probe_points(n, seed=7):
    """n seeded voxels around the structures: in and next to every kind of block, dust and far voxels, and empty space"""
    rng = np.random.default_rng(seed)
    parts = []

    def box(lo, hi, k):
        parts.append(np.stack([rng.integers(lo[a], hi[a], k) for a in range(3)], 1))

    k = n // 10
    box((X0 - 8, 0, X0 - 8), (X1 + 8, 24, X1 + 8), k)                                   # floor and its rim
    box((STAIR_X0 - 4, 0, STAIR_Z0 - 4), (STAIR_X0 + 16 * STAIR_N + 4, 230, STAIR_Z0 + 36), 2 * k)  # staircase
    box((BIG[0] - 6, BIG[1] - 6, BIG[2] - 6), (BIG[0] + 70, BIG[1] + 70, BIG[2] + 70), k)
    box((284, 20, ARCH_Z - 3), (356, 68, ARCH_Z + 7), k)
    box((ROOF_X - 3, ROOF_Y - 2, ROOF_Z - 3), (ROOF_X + ROOF_N + 3, ROOF_Y + 3, ROOF_Z + ROOF_N + 3), k)
    box((396, 14, 292), (432, 32, 312), k)                                              # mirror and glass
    box((TOWER[0] - 2, 0, TOWER[1] - 2), (TOWER[0] + 3, E, TOWER[1] + 3), k)
    for dst in (dust_points(), np.asarray(FAR + CORNERS)):  # dust, far voxels: they and their neighbours
        parts.append(dst[rng.integers(0, len(dst), k // 2)] + rng.integers(-1, 2, (k // 2, 3)))
    rest = n - sum(len(p) for p in parts)
    box((0, 0, 0), (E, E, E), rest)
    return np.concatenate(parts).astype(np.int32) & (E - 1)
