"""Time of a patch of a resident tree from solid shapes (svo_tree_patch_shapes_gpu), against the dense route where one exists:
  terrain  the 5-level terrain tree (1024^3): an off-grid 400^3 box fill and an r = 200 ball carve, each through
           patch_shapes and, the same composite, through svo_tree_patch_volume_gpu — the box as a dense tensor filled on the
           device, the ball as its clipped bounding box read from the tree and masked on the device; the time to make
           the tensor is part of that route and is timed with it
  scatter  the 7-level world (16384^3) of tests/test_gpu_shapes_patch.py: its 1300^3 box fill and the ball carved from it,
           for which no other route exists
Every run patches a tree built afresh (the build is not timed).  Host clock around each call, which ends synchronised;
WARM warm-ups, then the median of RUNS runs with their range.  The three svo_tree_patch_times slots of every patch are
reported as medians too (device passes, commit with the copy back to the host image, the host's ceiling update), and
the node records each route appends.  After the last run the two routes' trees are compared voxel by voxel.
The claim under test: patch_shapes' device time follows the cells the shapes cut, not their volume.  The cut cells of
the boxes are printed beside the times (closed form, tests/shapes_patch_cases.py).
Writes profiles/shapes_patch.txt (or the path given) with the library's svo_build_id().
usage: python tools/shapes_patch_timing.py [out.txt]"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

WARM, RUNS = 2, 7
BOX5 = ("box", (301, 3, 299), (400, 400, 400))
BALL5 = ("ball", (512, 60, 512), 200 * 200)


def clock(f):
    t0 = time.perf_counter()
    r = f()
    return (time.perf_counter() - t0) * 1e3, r


def med(a, warm=WARM):
    a = np.asarray(a[warm:])
    return "%.3f ms (%.3f .. %.3f)" % (np.median(a), a.min(), a.max())


def slots(s, warm=WARM):
    return "device passes %.3f ms, commit + host image %.3f ms, ceilings + top row %.3f ms (medians of svo_tree_patch_times)" % tuple(
        np.median(np.array(s[warm:]), 0))


def main():
    import torch

    import raytracing_test_amd as rt
    import shapes_patch_cases as spc

    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    out_path = args[0] if args else os.path.join(ROOT, "profiles", "shapes_patch.txt")
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    dev = torch.device("cuda", 0)
    lines = ["svo_build_id %s" % rt.build_id(), "device %s" % torch.cuda.get_device_name(0),
             "host clock around each call, %d warm-ups, median of %d (min .. max); every run patches a freshly built tree" % (WARM, RUNS)]

    # ------------------------------------------------------------------------------------------------ terrain --
    E = 1024
    probe = rt.Tree.terrain_gpu(5, E, E, 0)
    fill = int(probe.read_volume((0, 0, 0), (64, 64, 64)).max().item())   # an id the terrain stores
    lines += ["terrain, 5 levels (1024^3), %d node records; the fill stores id %d" % (probe.info().n_nodes, fill)]
    del probe

    def dense_box():
        return torch.full(BOX5[2][::-1], fill, dtype=torch.int16, device=dev), BOX5[1]

    def dense_ball(t):
        c, r = np.array(BALL5[1]), 200
        lo, hi = np.maximum(c - r, 0), np.minimum(c + r + 1, E)
        box = t.read_volume(tuple(int(v) for v in lo), tuple(int(v) for v in (hi - lo)[::-1])).contiguous()
        ax = [torch.arange(int(a), int(b), device=dev, dtype=torch.int64) - int(m) for a, b, m in zip(lo, hi, c)]
        box[(ax[2] ** 2)[:, None, None] + (ax[1] ** 2)[None, :, None] + (ax[0] ** 2)[None, None, :] <= BALL5[2]] = 0
        return box, tuple(int(v) for v in lo)

    for label, shape, dense in (("off-grid 400^3 box fill at %r" % (BOX5[1],), rt.box(BOX5[1], BOX5[2], fill), lambda t: dense_box()),
                                ("r = 200 ball carve at %r" % (BALL5[1],), rt.ball(BALL5[1], BALL5[2], 0), dense_ball)):
        ts, tv, ss, sv, gs, gv = [], [], [], [], [], []
        for _ in range(WARM + RUNS):
            a, b = rt.Tree.terrain_gpu(5, E, E, 0), rt.Tree.terrain_gpu(5, E, E, 0)
            n0 = a.info().n_nodes
            torch.cuda.synchronize()
            ms, _ = clock(lambda: a.patch_shapes([shape]))
            ts.append(ms)
            ss.append(a.patch_times())
            gs.append(a.info().n_nodes - n0)

            def route():
                vox, at = dense(b)
                b.patch_volume(vox, at)
            ms, _ = clock(route)
            tv.append(ms)
            sv.append(b.patch_times())
            gv.append(b.info().n_nodes - n0)
            same = a.count_diff(b) == 0
            del a, b
        lines += ["  %s: the two routes' trees %s" % (label, "hold the same voxels" if same else "DIFFER"),
                  "    svo_tree_patch_shapes_gpu                      %s, +%d node records" % (med(ts), gs[-1]),
                  "      " + slots(ss),
                  "    dense tensor + svo_tree_patch_volume_gpu       %s, +%d node records" % (med(tv), gv[-1]),
                  "      " + slots(sv) + "; the rest is the tensor"]
    lines += ["  cells the 400^3 box cuts, by cell size: %s" % ", ".join("%d^3: %d" % (4 ** k, spc.box_cut_cells(BOX5[1], BOX5[2], 4 ** k))
                                                                        for k in range(1, 5))]

    # ------------------------------------------------------------------------------------------------ scatter --
    import test_gpu_shapes_patch as tg

    xyz, ids = tg._scatter_shapes7()
    dx, di = torch.from_numpy(xyz).to(dev), torch.from_numpy(ids.view(np.int16)).to(dev)
    lines += ["scatter, 7 levels (16384^3), %d points" % len(ids)]
    box7, ball7 = rt.box(*tg.BOX7[1:]), rt.ball(*tg.BALL7[1:])
    warm, runs = 1, 4
    tb, tc, sb, sc, gb, gc = [], [], [], [], [], []
    for _ in range(warm + runs):
        t = rt.Tree.points_gpu(7, dx, di, tg.PAL)
        n0 = t.info().n_nodes
        torch.cuda.synchronize()
        ms, _ = clock(lambda: t.patch_shapes([box7]))
        tb.append(ms)
        sb.append(t.patch_times())
        n1 = t.info().n_nodes
        gb.append(n1 - n0)
        ms, _ = clock(lambda: t.patch_shapes([ball7]))
        tc.append(ms)
        sc.append(t.patch_times())
        gc.append(t.info().n_nodes - n1)
        stored = t.count_voxels(tg.BOX7[1], tg.BOX7[2][::-1])
        del t
    n_ball = spc.ball_count(tg.BALL7[1], tg.BALL7[2], (0, 0, 0), (4 ** 7,) * 3)
    lines += ["  %d warm-up, median of %d; no other route exists: the box holds %d voxels (an edit list ends at 2^31 - 1; a dense box is 4.4 GB)"
              % (warm, runs, 1300 ** 3),
              "  1300^3 box fill at %r                          %s, +%d node records" % (tg.BOX7[1], med(tb, warm), gb[-1]),
              "      " + slots(sb, warm),
              "  r2 = %d ball carve at %r inside it        %s, +%d node records" % (tg.BALL7[2], tg.BALL7[1], med(tc, warm), gc[-1]),
              "      " + slots(sc, warm),
              "  voxels counted in the box afterwards: %d (1300^3 - %d lattice points of the ball: %s)"
              % (stored, n_ball, "equal" if stored == 1300 ** 3 - n_ball else "DIFFERENT"),
              "  cells the 1300^3 box cuts, by cell size: %s" % ", ".join("%d^3: %d" % (4 ** k, spc.box_cut_cells(tg.BOX7[1], tg.BOX7[2], 4 ** k))
                                                                         for k in range(1, 7))]
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write(text)
    print(text, flush=True)


if __name__ == "__main__":
    main()
