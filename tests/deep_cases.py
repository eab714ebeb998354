"""The rays and poses of tests/test_gpu_deep_world.py on the deep worlds of tests/deep_world.py, and the conditions that
keep them honest, computed from the oracle's results or the put list alone (check_preconditions: run by
tests/test_deep_world_host.py on the CPU and, battery by battery, by the GPU module).  Direction sets, tie counting and the
oracle references come from tests/test_gpu_directed_rays.py, whose batteries these are the deep counterparts of."""
import numpy as np

import deep_world as dw
from test_gpu_directed_rays import SIGNS, STAIR_DIRS, ref_frames, ref_rays, ref_zero_plane, stair_directions, tie_counts, tie_directions  # noqa: F401


def frac_bits(levels):
    """fraction bits f32 keeps at coordinates in [H, E): 23 - (2 levels - 1)"""
    return 24 - 2 * levels


def base(levels):
    """air in the deep cavern: under the roof, stairs, the floating solids and dust around it"""
    g = dw.layout(levels)
    return np.array([g.H + 330.0, 110.0, g.H + 400.0])


def base_low(levels):
    """a second centre just below H in x: first segments cross the top-bit boundary"""
    g = dw.layout(levels)
    return np.array([g.H - 5.0, 100.0, g.H + 210.0])


# ------------------------------------------------------------------------------------------------------------------ A --
def budgets_A(levels):
    return (0, 1, 3, 300, 5000, 3 * dw.layout(levels).E)


def origin_classes(rng, levels, centre, n):
    """n origins of each class around `centre`: integral, half-integral, dyadic k + 2^-j (only j that f32 holds at that
    magnitude), generic fractions, negative (the same places one extent down), in or at solids"""
    g = dw.layout(levels)
    jit = lambda: rng.integers(-12, 13, (n, 3)).astype(np.float64)  # noqa: E731
    jmax = frac_bits(levels)
    cls = [centre + jit(), centre + jit() + 0.5, centre + jit() + 2.0 ** -rng.integers(1, jmax + 1, (n, 3)),
           centre + jit() + rng.uniform(0.01, 0.99, (n, 3)),
           centre + jit() - g.E + np.where(rng.integers(0, 2, (n, 1)) == 1, rng.uniform(0.01, 0.99, (n, 3)), 0.0),
           np.array([g.H + 300.5, dw.FLOOR_TOP + 0.5, g.H + 300.5]) + rng.integers(0, 3, (n, 3)) * np.array([1.0, 1.0, 1.0])]
    return [c.astype(np.float32) for c in cls]


def centres_light(levels):
    """the light world has no floor: over the 16-column staircase, and beside the 64^3 block"""
    g = dw.layout(levels)
    return np.array([g.H + 100.0, 190.0, g.H + 80.0]), np.array([g.big64[0] - 14.0, g.big64[1] + 30.0, g.big64[2] + 32.0])


def battery_A(levels, light=False):
    """(origins, dirs) in grouped order (sign octant, then origin class): every tie direction from two origins, one
    around each centre (base and base_low; on the light world centres_light)"""
    rng = np.random.default_rng(320 + levels)
    c0, c1 = centres_light(levels) if light else (base(levels), base_low(levels))
    dirs = tie_directions()
    o, d, key = [], [], []
    for i, dv in enumerate(dirs):
        octant = int(dv[0] < 0) + 2 * int(dv[1] < 0) + 4 * int(dv[2] < 0)
        for centre, c in ((c0, (0, 1, 2, 3, 4, 5)[i % 6]), (c1, (0, 1, 2, 3, 0, 1)[(i // 2) % 6])):
            o.append(origin_classes(rng, levels, centre, 1)[c][0])
            d.append(dv)
            key.append(octant * 16 + c)
    o, d, key = np.array(o, np.float32), np.array(d, np.float32), np.array(key)
    order = np.argsort(key, kind="stable")
    return o[order], d[order]


def check_A(org, dirs):
    ties = tie_counts(org, dirs)
    print("A: %d rays, %d with >= 20 exact ties in 300 steps (max %d)" % (len(org), (ties >= 20).sum(), ties.max()))
    assert len(org) <= 2000 and (ties >= 20).sum() >= 200


# ------------------------------------------------------------------------------------------------------------------ B --
def origin_lists_B(levels):
    """16 camera positions each: integral; half-integral and mixed; fractional (dyadic and generic)"""
    g = dw.layout(levels)
    rng = np.random.default_rng(340 + levels)
    b, lo = base(levels), base_low(levels)
    jit = lambda: rng.integers(-12, 13, (16, 3)).astype(np.float64)  # noqa: E731
    li = b + jit()
    li[3] -= g.E  # (negative coordinates: the same place one extent down)
    li[8:12] = lo + jit()[:4]
    lh = b + jit() + rng.integers(0, 2, (16, 3)) * 0.5
    lh[0] = b + 0.5
    lh[5] -= g.E
    lh[8:12] = lo + jit()[:4] + 0.5
    lf = b + jit()
    lf[1::2] += 2.0 ** -rng.integers(1, frac_bits(levels) + 1, (8, 3))
    lf[2::4] += rng.uniform(0.01, 0.99, (4, 3))
    lf[7] -= g.E
    lf[12:16] = lo + jit()[:4] + rng.uniform(0.01, 0.99, (4, 3))
    return {"integral": li.astype(np.float32), "half": lh.astype(np.float32), "fractional": lf.astype(np.float32)}


# ------------------------------------------------------------------------------------------------------------------ C --
def stair_budget(levels, w):
    """a shallow descent from row c + w + 1 takes 8 w steps and more: the widest staircase gets what crosses the world"""
    return {16: 300, 64: 600, 256: 1500, 1024: 3 * dw.layout(levels).E}[w]


def stair_origins(levels, w, model, offs):
    """integral origins around the step boundaries of the staircase of w-column steps: x one column before, at and after
    a boundary (offs), z likewise around the staircase's two sides and its middle, rows c + 1, c + 2, c + w, c + w + 1
    above the ceiling c of the origin's own w-column block (model: dw.ceiling_model)"""
    g = dw.layout(levels)
    x0, z0, depth, n, _ = g.stairs[w]
    j = {16: 0, 64: 1, 256: 2, 1024: 3}[w]
    # (the widest staircase stands in empty space except towards the area: its foot and far side are left out, since rays
    # that start over nothing and head away from it never end)
    wide = w == 1024 and n > 1
    xs = [x0 + w * i + k for i in sorted({1, n} if wide else {0, 1, n}) for k in offs]
    zs = [b + k for b in ((z0,) if w == 1024 else (z0, z0 + depth)) for k in offs] + [z0 + depth // 2 - 1, z0 + depth // 2]
    out = []
    for x in xs:
        for z in zs:
            c = int(model[j][(z & (g.E - 1)) // w, (x & (g.E - 1)) // w])  # (the widest staircase ends at the extent: beyond it is column 0)
            out += [(x, c + k, z) for k in (1, 2, w, w + 1)]
    return np.array(out, np.float32)


def stair_poses(levels):
    """one cast_stats pose per staircase: above its foot, looking down the steps' risers"""
    g = dw.layout(levels)
    res = {}
    for w, (x0, z0, depth, n, _) in g.stairs.items():
        if n > 1:
            res[w] = ((x0 - 1.0, dw.stair_top(g, w, n - 1) + w + 8.0, z0 + depth / 2.0), (1.0, -1.0, 0.0), min(4 * w + 300, 3000))
        else:  # (a single step, the solid root child's column before it: from over the step, down across its far edge)
            res[w] = ((x0 + w / 2.0, dw.stair_top(g, w, 0) + 200.0, z0 + depth / 2.0), (1.0, -0.25, 0.0), 3000)
    return res


# ------------------------------------------------------------------------------------------------------------------ D --
def cams_D(levels):
    """ten rows under the roof near its corner; beside and just under the 256^3 block at its corner; beside the 64^3 block"""
    H = dw.layout(levels).H
    return {"integral": (H + 330.0, 290.0, H + 370.0), "half": (H + 505.5, 505.5, H + 250.5), "fractional": (H + 460.3, 340.7, H + 470.45)}


def dirs_D(rt):
    return [(s, rt.normalize((s[0] * 1.0, s[1] * 0.45, s[2] * 0.8))) for s in SIGNS]


def shade_pose(levels):
    """the mirror patch, the glass wall and the pool on the floor, some sky"""
    H = dw.layout(levels).H
    return (H + 394.5, 72.5, H + 288.5), (0.6, -0.2, 0.5)


def check_mixed(fr, label):
    """fr: the oracle's hit fraction per octant pose (budget 300 and 3000 alternating)"""
    print("%s: oracle hit fractions per pose / budget: %s" % (label, " ".join("%.2f" % f for f in fr)))
    assert 0.05 < np.mean(fr) < 0.95 and sum(0 < fr[i] < 1 or 0 < fr[i + 1] < 1 for i in range(0, len(fr), 2)) >= 2


# ------------------------------------------------------------------------------------------------------------------ E --
def budgets_E(levels):
    E = dw.layout(levels).E
    return (300, E + 100, 3 * E)


def edge_rays(rt, levels):
    """[(direction, origins)]: from far root children into the cavern area; along and past the tower to row E - 1 and
    through the y wrap; through both wrap corners; from outside [0, E)^3 on each side; grazing the solid root child and
    the 1024^3 block along faces and edges (tie directions, integral origins); into and out of the split 256^3 block
    next to its odd voxel"""
    g = dw.layout(levels)
    E, H, q = g.E, g.H, g.q
    tx, tz = g.tower
    n = rt.normalize
    rays = [
        ((0.0, 1.0, 0.0), [(tx - 1, 80, tz), (tx + 1.5, E - 100.5, tz + 0.5), (tx + 0.5, E - 23.75, tz - 0.5), (tx, E + 76, tz + 1), (tx - 1, -30, tz),
                           (tx, E - 200, tz), (tx, -E + 70, tz)]),
        (n((0.001, 1, 0.0005)), [(tx - 1, 80, tz), (tx - 0.75, E - 400.5, tz - 0.25), (tx - 1.5, E + 6.5, tz + 0.5), (tx - 2, -700, tz)]),
        (n((0.05, 1, 0.02)), [(tx - 40, 800, tz - 16), (tx - 50.5, 30.5, tz - 20.5), (H + 330, 110, H + 400), (H + 330.25, E + 500.5, H + 400.125)]),
        (n((0.05, -1, 0.02)), [(tx - 5, E - 1, tz - 2), (tx - 5.5, 1000.5, tz - 2.5), (H + 330, 2 * E + 60, H + 400), (10, 3, 10), (10.5, -0.5, 10.5)]),
        (n((1, 1, 1)), [(E - 24, E - 24, E - 24), (E - 3.5, E - 3.5, E - 3.5), (E - 1.75, E - 2.5, E - 2), (-30, -30, -30), (E - 34, E - 24, E - 14),
                        (-E - 5, -E - 5, -E - 5)]),
        (n((-1, -1, -1)), [(20, 20, 20), (3.5, 3.5, 3.5), (1.25, 2.5, 1), (E + 16, E + 26, E + 21), (2.0, 1.0, 2.0), (2 * E + 9, 2 * E + 9, 2 * E + 9)]),
        (n((1, 0.5, 0.25)), [(E - 41, E - 21, E - 11), (-E - 40.5, -1.5, -E - 10.5), (2 * E - 18, E - 14, 2 * E - 8), (E + 476.5, E - 124.75, -E - 476.25)]),
        (n((-1, 0.5, -1)), [(H + 330, 110, H + 400), (-E - 700, E - 24, 2 * E + 400), (E + 76.5, E - 0.5, E + 76.5), (4, E - 5, 4)]),
    ]
    # from far root children into the area: more than E steps before the floor, the stairs or a solid is reached
    for k, (a, b, sx, sz, dy) in enumerate([(500, 500, 1, 1, 0.02), (80, 80, 1, 1, 0.02), (300, 150, 1, 1, 0.03), (700, 300, 1, -1, 0.02),
                                            (450, 420, -1, 1, 0.025), (900, 610, -1, -1, 0.02), (520, 300, 1, 1, 0.05), (200, 700, -1, 1, 0.015),
                                            (640, 260, 1, -1, 0.04), (400, 340, -1, -1, 0.03), (333, 333, 1, 1, 0.01), (150, 500, 1, -1, 0.0125)]):
        run = 0.55 * E + 64 * k
        o = np.array([H + a - sx * run, 64.0 + dy * run, H + b - sz * run]) + (0.0 if k % 2 else 0.375)
        rays.append((n((sx, -dy, sz)), [tuple(o), tuple(o + (0.0, 8.0, 0.0))]))
    # the solid root child [q, 2q) x [2q, 3q) x [3q, 4q): faces, edges and corners
    rays += [
        ((0.0, 0.0, 1.0), [(q - 1, 2 * q + 5, 3 * q - 10), (q, 2 * q + 5, 3 * q - 10), (q + 7, 2 * q - 1, 3 * q - 3), (q + 7, 2 * q, 3 * q - 3)]),
        ((1.0, 0.0, 0.0), [(q - 9, 2 * q, 3 * q), (q - 9, 2 * q - 1, 3 * q), (q - 9, 3 * q, E - 1), (q - 9, 3 * q - 1, E - 1)]),
        ((1.0, 1.0, 0.0), [(q - 5, 2 * q - 5, 3 * q + 7), (q - 5, 2 * q - 6, 3 * q + 7), (q - 5, 2 * q - 4, 3 * q), (2 * q - 3, 2 * q - 9, E - 1)]),
        ((1.0, 1.0, 1.0), [(q - 9, 2 * q - 9, 3 * q - 9), (q - 9, 2 * q - 8, 3 * q - 9), (2 * q - 1, 3 * q - 2, 3 * q - 9)]),
        ((-1.0, -1.0, -1.0), [(2 * q + 3, 3 * q + 3, E + 3), (2 * q + 3, 3 * q + 3, E + 4), (2 * q + 300, 3 * q + 300, E + 300)]),
        ((-1.0, 0.5, -0.25), [(2 * q + 8, 2 * q + 4, E + 2), (2 * q + 8, 3 * q - 4, E + 2), (2 * q + 64, 2 * q + 100, E + 16)]),
    ]
    if g.big1024:
        bx, by, bz = g.big1024
        rays += [
            ((0.0, 1.0, 0.0), [(bx - 1, by - 20, bz + 3), (bx, by - 20, bz + 3), (bx + 1023, by - 20, bz + 1023), (bx + 1024, by - 20, bz + 1023)]),
            ((1.0, 0.0, 1.0), [(bx - 7, by, bz - 7), (bx - 7, by - 1, bz - 7), (bx - 7, by + 1023, bz - 7), (bx - 7, by + 1024, bz - 7), (bx - 8, by + 5, bz - 7)]),
            ((-1.0, -1.0, 0.0), [(bx + 1030, by + 1030, bz), (bx + 1030, by + 1031, bz), (bx + 1030, by + 1030, bz - 1)]),
            ((1.0, 0.5, 0.25), [(bx - 64, by - 32, bz - 16), (bx - 64, by + 991, bz + 1007), (bx - 64, by + 992, bz + 1008)]),
        ]
    # the split 256^3 block: towards its odd voxel from outside on every axis, and from the voxels next to it inside
    dust = dw.dust_points(levels)
    ox, oy, oz = (int(v) for v in dust[dw.inside(dust, g.big256, 256)][0])
    bx, by, bz = g.big256
    rays += [
        ((1.0, 0.0, 0.0), [(bx - 9, oy, oz), (bx - 9.5, oy + 0.5, oz + 0.5), (ox - 1, oy, oz), (ox, oy, oz), (ox + 1, oy, oz)]),
        ((0.0, -1.0, 0.0), [(ox, by + 300, oz), (ox + 0.5, by + 260.25, oz + 0.5), (ox, oy + 1, oz), (ox, oy - 1, oz)]),
        ((0.0, 0.0, -1.0), [(ox, oy, bz + 270), (ox, oy, oz + 1), (ox, oy, oz - 1), (ox + 0.25, oy + 0.75, bz + 300.5)]),
        ((1.0, 1.0, 1.0), [(ox - 1, oy - 1, oz - 1), (ox + 1, oy + 1, oz + 1), (bx - 4, by - 4, bz - 4), (bx + 250, by + 250, bz + 250)]),
    ]
    return [(n(d), np.array(os_, np.float32)) for d, os_ in rays]  # (normalised: equal components stay equal)


def flat_rays(rays):
    org = np.concatenate([os_ for _, os_ in rays]).astype(np.float32)
    dirs = np.concatenate([np.tile(d, (len(os_), 1)) for d, os_ in rays]).astype(np.float32)
    return org, dirs


def check_E(levels, org, ref):
    """on the oracle's results at the budget 3 E"""
    g = dw.layout(levels)
    hit = ref["hit"] != 0
    used = 3 * g.E - ref["steps"]
    start = (np.floor(org.astype(np.float64)).astype(np.int64) & (g.E - 1)) // g.q
    end = (ref["pos"].astype(np.int64) & (g.E - 1)) // g.q
    crossed = (start != end).any(1)
    print("E levels %d: %d rays, %d oracle hits, %d end in another root child than they start in, %d hit after more than E steps" % (
        levels, len(org), hit.sum(), crossed.sum(), (hit & (used > g.E)).sum()))
    assert hit.sum() >= 12 and crossed.sum() >= 8 and (hit & (used > g.E)).sum() >= 8


# ------------------------------------------------------------------------------------------------------------------ F --
def pose_F(levels):
    """from the middle of the area towards -x and slightly down: the rays leave the area sideways, across the top-bit boundary
    and the 1024- and 4096-wide regions beyond it"""
    H = dw.layout(levels).H
    return (H + 200.0, 150.0, H + 500.0), (-1.0, -0.05, -0.3)


# ------------------------------------------------------------------------------------------------------------------ G --
WIRE_STEPS = 32767


def wire_rays(rt, levels=7):
    """rays along empty rows of the 7-level world at the wire formats' budget cap.  Per axis a and sign: the ray runs N >
    16384 voxels along a, drifting m = 3 voxels on the next axis b (d_b = (m + 1/4) / N: the drift is over well before the
    end from any origin fraction below 0.7, and the target's column is passed E voxels early one voxel to the side), and
    ends on a far voxel of an otherwise empty root child; a twin displaced on the third axis spends the budget.
    Returns [(axis, direction, {"integral" | "half" | "fractional": origins})]"""
    g = dw.layout(levels)
    targets = {0: g.far[1], 1: g.far[2], 2: g.far[3]}
    m = 3
    out = []
    for a in range(3):
        b, c = (a + 1) % 3, (a + 2) % 3
        F = np.array(targets[a], np.float64)
        for s in (1.0, -1.0):
            for N in (20000, 17000, 26000):
                d = np.zeros(3)
                d[a], d[b], d[c] = s, (m + 0.25) / N, 2.0 ** -30  # (not 0: from an integral coordinate a zero component makes deltaPos NaN)
                kinds = {"integral": [], "half": [], "fractional": []}
                for miss in (0, 7):
                    o = F.copy()
                    o[a] -= s * N
                    o[b] -= m
                    o[c] += miss
                    kinds["integral"].append(o.copy())
                    kinds["half"].append(o + 0.5)
                    f = o + (0.25, 0.625, 0.375)
                    kinds["fractional"].append(f)
                out.append((a, rt.normalize(d), {k: np.array(v, np.float32) for k, v in kinds.items()}))
    return out


def check_G(org, ref, axis):
    """per axis, on the oracle's records of the rays that run along it: step counts on the axis (from pos and the origin's
    voxel) of 16384 and more, displacements of -16384 and less, and hits among those long rays"""
    cell = np.trunc(org.astype(np.float64)).astype(np.int64)
    disp = ref["pos"].astype(np.int64)[:, axis] - cell[:, axis]
    long_ = np.abs(disp) >= 16384
    hits = long_ & (ref["hit"] != 0)
    print("G axis %d: %d records, %d with >= 16384 steps on the axis, %d with a displacement <= -16384, %d of the long ones hit" % (
        axis, len(org), long_.sum(), (disp <= -16384).sum(), hits.sum()))
    assert long_.sum() >= 32 and (disp <= -16384).sum() >= 8 and hits.sum() >= 8
    assert np.abs(disp).max() <= 32767


# ------------------------------------------------------------------------------------------------------------------ H --
def patch_edits(levels):
    """put-only edits at coordinates >= H for the light world: (xyz int32 (n, 3), colour ids (n,)): seeded voxels over the
    light battery's two centres, some high above every ceiling of the area, the voxel that completes the 4^3 brick, and one inside the 64^3 block"""
    g = dw.layout(levels)
    rng = np.random.default_rng(380)
    n = 300
    c0, c1 = centres_light(levels)
    near = [np.round(c).astype(np.int64) + rng.integers(-20, 21, (140, 3)) for c in (c0, c1)]   # in view of battery A's origins
    high = np.stack([rng.integers(g.H, g.H + dw.AREA, 20), rng.integers(1500, 1800, 20), rng.integers(g.H, g.H + dw.AREA, 20)], 1)
    p = np.unique(np.concatenate(near + [high]), axis=0)
    p = p[rng.permutation(len(p))]
    assert 250 <= len(p) <= n
    ids = 1000 + rng.integers(0, 37, len(p))
    bx, by, bz = g.brick63
    x, y, z = g.big64
    p = np.concatenate([p, [(bx + 3, by + 3, bz + 3), (x + 31, y + 17, z + 40)]]).astype(np.int32)
    ids = np.concatenate([ids, [400, 1005]])
    assert (p[:, [0, 2]] >= g.H).all() and len(np.unique(p, axis=0)) == len(p)
    return np.ascontiguousarray(p), ids


# ------------------------------------------------------------------------------------------------------ all of them --
def check_preconditions(rt, oracle_mod, T, levels):
    """every condition the GPU module asserts on the oracle's results, for the World-built tree of `levels`"""
    g = dw.layout(levels)
    org, dirs = battery_A(levels)
    check_A(org, dirs)
    # C: hit fraction above 0.5 per staircase
    model = dw.ceiling_model(levels)
    for group in sorted(STAIR_DIRS):
        for w in (16, 64, 256, 1024):
            o = stair_origins(levels, w, model, (-1, 0, 1) if group == "boundary" else (-2, -1, 0))
            for shift in (0.0, 0.5, 2.0 ** -3):
                fr = np.mean([(ref_zero_plane(oracle_mod, T, o + np.float32(shift), dn, 1, 1, stair_budget(levels, w))["hit"] != 0).mean()
                              for dn in stair_directions(rt, group)])
                print("C levels %d %s w=%d shift=%g: oracle hit fraction %.3f" % (levels, group, w, shift, fr))
                assert fr > 0.5
    # E
    eo, ed = flat_rays(edge_rays(rt, levels))
    check_E(levels, eo, ref_rays(T, eo, ed, 3 * g.E))
    if levels != 7:
        return
    # B: zero-plane frames of the tied directions
    from test_gpu_directed_rays import frame_directions

    full, zero = frame_directions(rt)
    for kind, origins in origin_lists_B(levels).items():
        for steps in (300, 3000):
            fr = np.mean([(ref_zero_plane(oracle_mod, T, origins, dn, 1, 1, steps)["hit"] != 0).mean() for dn in full + zero])
            print("B %s S=%d: oracle hit fraction %.3f" % (kind, steps, fr))
            assert 0.05 < fr < 0.95
    # D
    for cam, o in cams_D(levels).items():
        fr = [(ref_frames(T, [o], dn, 96, 64, S, None, None)["hit"] != 0).mean() for _, dn in dirs_D(rt) for S in (300, 3000)]
        check_mixed(fr, "D " + cam)
    # G
    for a in range(3):
        os_, ds = [], []
        for axis, dn, kinds in wire_rays(rt):
            if axis == a:
                for o in kinds.values():
                    os_.append(o)
                    ds.append(np.tile(dn, (len(o), 1)))
        o, d = np.concatenate(os_), np.concatenate(ds)
        ref = ref_rays(T, o, d, WIRE_STEPS)
        # (each frame origin gives 64 records of its ray; a third of the origins are cast as explicit rays as well)
        check_G(np.repeat(o, 64, 0), {k: np.repeat(v, 64, 0) for k, v in ref.items()}, a)
        assert ((ref["hit"] != 0) & (np.abs(ref["pos"][:, a] - np.trunc(o[:, a])) >= 16384)).sum() >= 8
