"""The worlds of tests/test_gpu_ceil_coarse.py and a restatement of the march before the loop (csrc/svo_ceil_march.h) on the
CPU: one loop per level, coarse to fine, on the exact event values of castRayFromCam's DDA (ray_caster.cpp:58-80: f64
accumulation of |f32(1 / d)|; for the linear rays the march takes, T + j * a is exact in f64, so Python's product and sum
are the kernel's fma).  march() says how each level ends for a ray, how many blocks it passed there, how the ray had
entered the block it descended from and whether it crossed the world's edge; the GPU test asserts those on its inputs and
holds the diagnostics counters of the kernel against the counts."""
import math

import numpy as np

FINE_MAX = 24  # kMarchFineMax, kMarchFineSpan of csrc/svo_ceil_march.h
FINE_SPAN = 8 * FINE_MAX
COARSE_SPAN = 8  # kMarchCoarseSpan: a coarse level is walked when the budget spans this many of its blocks
SPIKE = {4: 120, 5: 200}


def heights(levels):
    """(E, E) column tops [x][z]: terraces of 4 x 4 columns 3 rows apart, hills of 64 x 64 columns 10 rows apart, and in
    every other coarsest block (256 columns at 5 levels, 64 at 4) one spike far above them: the coarse ceilings say much in
    the blocks without one and nothing in those with"""
    E = 1 << (2 * levels)
    x, z = np.meshgrid(np.arange(E), np.arange(E), indexing="ij")
    h = 6 + 3 * (((x >> 2) + 2 * (z >> 2)) % 5) + ((x >> 4) % 2) * 4 + 10 * (((x >> 6) + 2 * (z >> 6)) % 3)
    csh = 2 * (levels - 1)
    cm = (1 << csh) - 1
    spike = (((x >> csh) + (z >> csh)) % 2 == 1) & ((x & cm) == 37) & ((z & cm) == 41)
    h[spike] = SPIKE[levels]
    return h.astype(np.int32)


def tables(tree):
    """{block width: ceilings [z][x]} of a host tree: 4 columns (the fine table), then 16, 64, ... as the tree has them"""
    out = {4: np.asarray(tree.ceilings_fine(), np.int64)}
    for j, c in enumerate(tree.ceilings()):
        out[16 << (2 * j)] = np.asarray(c, np.int64)
    return out


def march_widths(tabs, steps=None, coarse_max=2):
    """the block widths the march of a launch walks, coarsest first (svo_plan.cpp march_levels restated: at most coarse_max
    levels above 16 columns, each with at least 2 x 2 blocks), ending on 16 and 4; with `steps`, the budget the march starts
    with, only the coarse levels it spans COARSE_SPAN blocks of"""
    ws = sorted([w for w in (64, 256)[:coarse_max] if w in tabs and tabs[w].shape[0] >= 2], reverse=True)
    while steps is not None and ws and steps // ws[0] < COARSE_SPAN:
        ws = ws[1:]
    return ws + [16, 4]


def setup(org, d):
    o, dd = np.asarray(org, np.float32), np.asarray(d, np.float32)
    with np.errstate(all="ignore"):
        dl = (np.float32(1.0) / dd).astype(np.float64)
    a = np.abs(dl)
    T = a - ((o.astype(np.float64) - (dd < 0)) - np.trunc(o).astype(np.float64)) * dl
    return [float(v) for v in T], [float(v) for v in a], [int(v) for v in np.where(dd < 0, -1, 1)], [int(v) for v in np.trunc(o)]


def first_step(T, a, s, p):
    ax = 0 if (T[0] < T[1] and T[0] < T[2]) else (1 if T[1] < T[2] else 2)
    p[ax] += s[ax]
    T[ax] += a[ax]
    return ax


def _count(T, a, V, strict):
    """#{j >= 0: T + j a < V} (strict) or <= V"""
    if V == -math.inf or a == math.inf:
        return 0 if (V == -math.inf or not ((T < V) if strict else (T <= V))) else 1
    n = max(0, int((V - T) / a) - 2)
    while (T + n * a < V) if strict else (T + n * a <= V):
        n += 1
    return n


def march(org, d, steps, tabs, E, widths=None, pre_top=-1):
    """The march of the linear descending ray (org, d) with budget `steps` over the levels `widths` (coarsest first, ending
    ..., 16, 4; None: the levels the kernel takes for the budget the march starts with).  A ray above the tree's top row
    pre_top first takes the crossing down to it, when its budget reaches that far, and marches from there.  Returns {"levels": {width: {"blocks", "end", "entry", "wrap"}}, "stop": (axis, index) or None, "dda": the
    DDA steps from the state after the first step up to and including the stop event, "widths": the levels walked}; end is one of enter_below,
    ceiling_event, corner_tie, boundary_ceiling_tie, beyond_budget, bound; entry (of the block the level ended in) x, z or
    start.  None when the ray does not march (it ascends, or its budget ends with the first step)."""
    T, a, s, p = setup(org, d)
    if steps <= 0 or s[1] >= 0:
        return None
    first_step(T, a, s, p)
    steps -= 1
    if steps <= 0:
        return None
    wm = E - 1
    pre = 0
    if pre_top >= 0 and (p[1] & wm) > pre_top:  # the crossing down to the top row: up to and including the y step that enters it
        T2, p2, n = list(T), list(p), 0
        while (p2[1] & wm) > pre_top and n <= steps:
            first_step(T2, a, s, p2)
            n += 1
        if n <= steps:
            T, p, steps, pre = T2, p2, steps - n, n
    if steps <= 0:
        return None
    if widths is None:
        widths = march_widths(tabs, steps)
    wx, wy, wz = p[0] & wm, p[1] & wm, p[2] & wm
    w0 = widths[0]
    jx = (w0 - 1 - (wx & (w0 - 1))) if s[0] > 0 else (wx & (w0 - 1))
    jz = (w0 - 1 - (wz & (w0 - 1))) if s[2] > 0 else (wz & (w0 - 1))
    bx, bz = wx // w0, wz // w0
    Ein, ein_axis, ein_j = -math.inf, -1, 0
    res = {}
    stop16 = None
    stop = None
    jy = 0
    for li, w in enumerate(widths):
        if w == 4:
            reach = jx + jz + 2 + (jy if jy >= 0 else wy) + 1
            if steps - reach < FINE_SPAN:
                break
        if li > 0:  # the descent: the sub-block the entering event left the ray in
            ez = ein_axis == 2
            n = _count(T[0], a[0], Ein, True) if ez else (_count(T[2], a[2], Ein, False) if ein_axis == 0 else 0)
            kx = ein_j + 1 if ein_axis == 0 else (n if ez else 0)
            kz = ein_j + 1 if ez else (n if ein_axis == 0 else 0)
            lx, lz = ((jx - kx) // w) & 3, ((jz - kz) // w) & 3
            jx -= lx * w
            jz -= lz * w
            bx = bx * 4 + (3 - lx if s[0] > 0 else lx)
            bz = bz * 4 + (3 - lz if s[2] > 0 else lz)
        tab, rows = tabs[w], E // w
        bound = FINE_MAX if w == 4 else 1024
        rec = {"blocks": 0, "wrap": False, "entry": {-1: "start", 0: "x", 2: "z"}[ein_axis]}
        while True:
            Ex, Ez = T[0] + jx * a[0], T[2] + jz * a[2]
            xn = Ex < Ez
            jy = wy - 1 - int(tab[bz, bx])
            tc = T[1] + jy * a[1] if jy >= 0 else -math.inf
            if not (tc > Ein) or rec["blocks"] == bound:
                rec["end"] = "bound" if tc > Ein else "enter_below"
                stop = (ein_axis, ein_j) if ein_axis >= 0 else None
                break
            Eexit = Ex if xn else Ez
            far = (jx if xn else jz) > steps
            if not (Eexit < tc) or Ex == Ez or far:
                rec["end"] = "beyond_budget" if far else ("corner_tie" if Ex == Ez and Eexit < tc else
                                                         ("boundary_ceiling_tie" if Eexit == tc else "ceiling_event"))
                zfirst = Ez <= tc and Ez <= Ex
                stop = (1, jy) if (far or (not zfirst and tc <= Ex)) else ((2, jz) if zfirst else (0, jx))
                break
            rec["blocks"] += 1
            Ein = Eexit
            if xn:
                ein_axis, ein_j = 0, jx
                jx += w
                nb = bx + s[0]
                rec["wrap"] |= nb < 0 or nb >= rows
                bx = nb % rows
            else:
                ein_axis, ein_j = 2, jz
                jz += w
                nb = bz + s[2]
                rec["wrap"] |= nb < 0 or nb >= rows
                bz = nb % rows
        res[w] = rec
        if w == 16:
            stop16 = stop
        if w == 4 and jx + jz + 2 + (jy if jy >= 0 else wy) + 1 > steps:
            stop = stop16
    out = {"levels": res, "stop": stop, "dda": None, "widths": list(widths)}
    if stop is not None:
        # the DDA steps up to and including the stop event: the events of each axis that precede it in the DDA's order (z, y, x at ties)
        V = T[stop[0]] + stop[1] * a[stop[0]]
        n = 0
        for k in range(3):
            if k == stop[0]:
                n += stop[1] + 1
            else:
                n += _count(T[k], a[k], V, strict=not (k > stop[0]))  # (a lower-ranked axis — z before y before x — wins ties)
        out["dda"] = pre + n
    return out
