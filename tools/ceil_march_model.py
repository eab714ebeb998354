"""A CPU model of the C3 frame's traversal iterations under three marches before the loop: none below 16-column blocks
(the march as it was), the fine descent onto 4-column ceilings with its bound (svo_ceil_march.h), and the same without a
bound.  No GPU: the oracle's heights(4096, 4096) and pixel_dir, the reference DDA stepped voxel by voxel from (4, 90, 4).

What it counts.  A voxel is solid when y <= h(x, z).  The march walks 16-column blocks while the ray's row is above the
block's ceiling, then (fine) 4-column blocks the same way for at most FINE_MAX of them; the loop starts at the first
voxel the march could not pass.  One loop iteration is counted per ceiling box (the 64-column block's when the row is
above its ceiling, else the 16-column block's), per empty aligned cell (the largest of 4 .. 1024 voxels wide that holds
the voxel and nothing solid) and per brick visited; the iteration that meets a solid voxel ends the ray.  Forward-box
growth is ignored, so absolute counts run high (the model's old mean per wave against the measured wave_iters calibrates
that); the claim is the ratio between the marches.  A wave is a 16 x 4 footprint, its iterations the maximum over the
lanes sampled.

usage: python tools/ceil_march_model.py [--out profiles/fine_march/model_c3.txt]

--levels 256,64,16,4 (block widths, coarsest first) models the march as one loop per level instead, each level handing over
to the next finer one where it fails, from the ray's own voxel and with the move down to the terrain's top row taken first
(the blocks above that row are then not walked), next to today's 16,4: the march trips per wave (the maximum over a
footprint's lanes, summed over the levels), the blocks per ray at each level, and the DDA step the march ends at, which
must not depend on the levels.
usage: python tools/ceil_march_model.py --levels 256,64,16,4 --levels 64,16,4 [--out profiles/coarse_march/model_c3.txt]"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import oracle as O  # noqa: E402

E, W, H, STEPS = 4096, 1920, 1080, 16384
ORG, CAM = (4.0, 90.0, 4.0), (1.0, -0.45, 1.0)
FINE_MAX = 24  # kMarchFineMax of csrc/svo_ceil_march.h
ROWS, COLS, LANES = 13, 5, 24
CELLS = (4, 16, 64, 256, 1024)


def mip(h, s):
    n = h.shape[0] // s
    return h.reshape(n, s, n, s).max(axis=(1, 3))


def rays():
    """(tile row, footprint, direction) of the sampled lanes: ROWS rows of 4 pixels over the frame's height, COLS footprints
    of 16 x 4 pixels each, LANES of their 64 pixels"""
    cam = O.normalize(CAM)
    ppx, ppy = O.proj_plane(W, H)
    rng = np.random.default_rng(3)
    out = []
    for r in range(ROWS):
        py0 = int(round(r * (H - 4) / (ROWS - 1))) // 4 * 4
        for c in range(COLS):
            px0 = int(round(c * (W - 16) / (COLS - 1))) // 16 * 16
            for k in rng.choice(64, LANES, replace=False):
                out.append((r, r * COLS + c, O.pixel_dir(cam, ppx, ppy, W, H, px0 + int(k) % 16, py0 + int(k) // 16)))
    return out


def run(h, mips, dirs, fine, bound, sizes=None, top_first=False, org=ORG, steps=STEPS):
    """per ray: loop iterations, 16-column march blocks, fine march blocks; with sizes (the levels' block widths, coarsest
    first): loop iterations, {width: march blocks}, the DDA step the march ended at.  top_first: the blocks above the
    terrain's top row are not walked (one move takes the ray down to it)"""
    E = h.shape[0]
    cells = [c for c in CELLS if c <= E]
    phases = tuple(sizes) if sizes else ((16, 4) if fine else (16,))
    top = int(h.max())
    n = len(dirs)
    d = np.asarray(dirs, np.float32)
    dl = (np.float32(1.0) / d).astype(np.float64)
    a = np.abs(dl)
    o = np.asarray(org, np.float32)
    T = a - ((o.astype(np.float64) - (d < 0)) - np.trunc(o).astype(np.float64)) * dl
    s = np.where(d < 0, -1, 1).astype(np.int64)
    p = np.tile(np.trunc(o).astype(np.int64), (n, 1))
    live = np.ones(n, bool)
    phase = np.zeros(n, np.int64)  # the march's level (0: 16-column march, 1: fine march without sizes); len(phases): the loop
    iters, mb = np.zeros(n, np.int64), {sz: np.zeros(n, np.int64) for sz in phases}
    end = np.full(n, -1, np.int64)
    # the region the ray is crossing: a column block (size rs, rows above rb) or a cell (rb: its low row, rt: its top)
    rs = np.zeros(n, np.int64)
    rx, rz = np.full(n, -1, np.int64), np.full(n, -1, np.int64)
    rb, rtop = np.zeros(n, np.int64), np.zeros(n, np.int64)
    for step in range(steps):
        if not live.any():
            break
        # one DDA step (ray_caster.cpp:70-80)
        cx = (T[:, 0] < T[:, 1]) & (T[:, 0] < T[:, 2])
        cy = ~cx & (T[:, 1] < T[:, 2])
        ax = np.where(cx, 0, np.where(cy, 1, 2))
        idx = np.nonzero(live)[0]
        p[idx, ax[idx]] += s[idx, ax[idx]]
        T[idx, ax[idx]] += a[idx, ax[idx]]
        x, y, z = p[:, 0] % E, p[:, 1] % E, p[:, 2] % E
        # still inside the region being crossed?
        inside = (rs > 0) & ((x // np.maximum(rs, 1)) == rx) & ((z // np.maximum(rs, 1)) == rz) & (y >= rb) & (y <= rtop)
        todo = live & ~inside
        for ph, size in enumerate(phases):
            mp = mips[size]
            k = np.nonzero(todo & (phase == ph))[0]
            if not len(k):
                continue
            c = mp[x[k] // size, z[k] // size]
            ok = y[k] > c
            if size == 4:
                ok &= mb[4][k] < bound
            go = k[ok]
            mb[size][go] += 1 if not top_first else (y[go] <= top + 1).astype(np.int64)
            rs[go], rx[go], rz[go], rb[go], rtop[go] = size, x[go] // size, z[go] // size, c[ok] + 1, E - 1
            stop = k[~ok]
            phase[stop] = ph + 1
            todo[go] = False
        k = np.nonzero(todo & (phase == len(phases)))[0]
        if len(k):
            end[k] = np.where(end[k] < 0, step, end[k])
            iters[k] += 1
            xs, ys, zs = x[k], y[k], z[k]
            hit = ys <= h[xs, zs]
            live[k[hit]] = False
            c64, c16 = mips[64][xs // 64, zs // 64], mips[16][xs // 16, zs // 16]
            size = np.zeros(len(k), np.int64)
            lo = np.zeros(len(k), np.int64)
            hi = np.full(len(k), E - 1, np.int64)
            box64, box16 = ys > c64, (ys > c16) & ~(ys > c64)
            size[box64], lo[box64] = 64, c64[box64] + 1
            size[box16], lo[box16] = 16, c16[box16] + 1
            cell = ~box64 & ~box16
            for cs in cells:  # the largest empty aligned cell; none: the brick
                y0 = ys // cs * cs
                e = cell & (y0 > mips[cs][xs // cs, zs // cs])
                size[e], lo[e], hi[e] = cs, y0[e], y0[e] + cs - 1
            brick = cell & (size == 0)
            y0 = ys // 4 * 4
            size[brick], lo[brick], hi[brick] = 4, y0[brick], y0[brick] + 3
            rs[k], rx[k], rz[k], rb[k], rtop[k] = size, xs // size, zs // size, lo, hi
    if sizes:
        return iters, mb, end
    return iters, mb[16], mb.get(4, np.zeros(n, np.int64))


def levels_table(h, mips, rr, level_lists):
    """the --levels table: per level list and start (the top-row move first, or the ray's own voxel) the march trips per wave
    and the blocks per ray at each level; every variant's march must end at the same DDA step"""
    fp = np.array([r[1] for r in rr])
    dirs = [r[2] for r in rr]
    lines = ["C3 model, one march loop per level: %d tile rows x %d footprints x %d lanes" % (ROWS, COLS, LANES),
             "trips per wave: the maximum over a footprint's lanes at each level, summed over the levels (mean over the waves)", ""]
    ends = None
    for sizes in level_lists:
        for top_first in (True, False):
            it, mb, end = run(h, mips, dirs, True, FINE_MAX, sizes=sizes, top_first=top_first)
            if ends is None:
                ends = end
            assert np.array_equal(end, ends), "the march's end depends on the levels"
            waves = sorted(set(fp.tolist()))
            trips = {sz: np.mean([mb[sz][fp == w].max() for w in waves]) for sz in sizes}
            lines.append("levels %-14s %-22s trips per wave %s = %.2f; blocks per ray %s; wave iterations %.2f" % (
                ",".join(map(str, sizes)), "top-row move first" if top_first else "from the ray's voxel",
                " + ".join("%.2f" % trips[sz] for sz in sizes), sum(trips.values()),
                " + ".join("%.2f" % mb[sz].mean() for sz in sizes), np.mean([it[fp == w].max() for w in waves])))
    lines.append("")
    lines.append("every variant ends its march at the same DDA step: mean %.1f" % ends.mean())
    return "\n".join(lines) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fine_march", "model_c3.txt"))
    ap.add_argument("--levels", action="append", default=[], help="block widths of a march with one loop per level, coarsest first (e.g. 256,64,16,4); repeatable")
    args = ap.parse_args()
    h = O.heights(E, E).astype(np.int64)
    mips = {cs: mip(h, cs) for cs in CELLS}
    rr = rays()
    if args.levels:
        text = levels_table(h, mips, rr, [(16, 4)] + [tuple(int(v) for v in l.split(",")) for l in args.levels])
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)
        sys.stdout.write(text)
        return
    row = np.array([r[0] for r in rr])
    fp = np.array([r[1] for r in rr])
    dirs = [r[2] for r in rr]
    lines = ["C3 model: %d tile rows x %d footprints x %d lanes; wave iterations = max over a footprint's lanes" % (ROWS, COLS, LANES), ""]
    res = {}
    for name, fine, bound in (("march16", False, 0), ("fine%d" % FINE_MAX, True, FINE_MAX), ("fine_unbounded", True, 1 << 30)):
        res[name] = run(h, mips, dirs, fine, bound)
    lines.append("%-5s %s" % ("row", "  ".join("%-34s" % n for n in res)))
    lines.append("%-5s %s" % ("", "  ".join("%-34s" % "wave iters (5 footprints)  blocks/ray" for _ in res)))
    tot = {n: 0 for n in res}
    for r in range(ROWS):
        cols = []
        for n, (it, m16, m4) in res.items():
            w = [int(it[fp == r * COLS + c].max()) for c in range(COLS)]
            tot[n] += sum(w)
            sel = row == r
            cols.append("%-18s %5.1f + %5.1f" % ("/".join(map(str, w)), m16[sel].mean(), m4[sel].mean()))
        lines.append("%-5d %s" % (r, "  ".join("%-34s" % c for c in cols)))
    lines.append("")
    for n, (it, m16, m4) in res.items():
        lines.append("%-16s wave iterations summed %4d, mean per wave %.2f; march blocks per ray %.1f of 16 columns + %.1f of 4" %
                     (n, tot[n], tot[n] / (ROWS * COLS), m16.mean(), m4.mean()))
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    sys.stdout.write(text)


if __name__ == "__main__":
    main()
