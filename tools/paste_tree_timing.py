"""Time of a paste of a box of one resident tree into another (svo_tree_patch_tree_gpu), against the routes that move the
same content through its voxels:
  terrain  the 5-level terrain tree (1024^3) as src, an empty 5-level tree as dst: an off-grid 64^3 box and an off-grid
           256^3 box, each through patch_tree and, the same composite, through (a) read_volume of src's box + patch_volume,
           and (b) list_voxels of src's box, the positions shifted on the device, + patch_points (dst is empty there, so
           the list of src's stored voxels is the whole difference; the time to read and shift is part of each route)
  scatter  the 7-level world (16384^3) of tests/test_gpu_paste_tree.py: the 1300^3 region with a ball carved out of it,
           made in an empty tree by patch_shapes and pasted into the scattered world at an offset odd on every axis — on
           its own, since the other routes cannot hold it (4.4 GB as a dense box, 2.2 * 10^9 list entries)
Every run pastes into a tree built afresh (the builds are not timed).  Host clock around each call, which ends
synchronised; WARM warm-ups, then the median of RUNS runs with their range.  The three svo_tree_patch_times slots of every
patch are reported as medians too (device passes, commit with the copy back to the host image, the host's ceiling
update), and the node records each route appends.  After the last run the routes' trees are compared voxel by voxel.
The claim under test: the paste's time follows the cells cut — the box's surface and src's records in it — not the
volume.  The cells the boxes cut are printed beside the times (closed form, tests/shapes_patch_cases.py).
Writes profiles/paste_tree.txt (or the path given) with the library's svo_build_id().
usage: python tools/paste_tree_timing.py [out.txt]"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

WARM, RUNS = 2, 7
E5 = 1024
# (src_origin, edge, dst_origin): off every grid, low enough to hold the terrain's surface
BOXES5 = (((301, 3, 299), 64, (410, 40, 388)), ((301, 3, 299), 256, (410, 40, 388)))


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
    out_path = args[0] if args else os.path.join(ROOT, "profiles", "paste_tree.txt")
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    dev = torch.device("cuda", 0)
    lines = ["svo_build_id %s" % rt.build_id(), "device %s" % torch.cuda.get_device_name(0),
             "host clock around each call, %d warm-ups, median of %d (min .. max); every run pastes into a freshly built tree" % (WARM, RUNS)]

    # ------------------------------------------------------------------------------------------------ terrain --
    src = rt.Tree.terrain_gpu(5, E5, E5, 0)
    pal = src.palette()
    none = (np.zeros((0, 3), np.int32), np.zeros(0, np.uint16))
    lines += ["terrain, 5 levels (1024^3), %d node records, into an empty 5-level tree" % src.info().n_nodes]
    for so, n, do in BOXES5:
        dims = (n, n, n)
        shift = torch.tensor([d - s for s, d in zip(so, do)], dtype=torch.int32, device=dev)
        tp, tv, tl, sp, sv, sl, gp, gv, gl = [], [], [], [], [], [], [], [], []
        for _ in range(WARM + RUNS):
            a, b, c = (rt.Tree.points_gpu(5, *none, pal) for _ in range(3))
            n0 = a.info().n_nodes
            torch.cuda.synchronize()
            ms, _ = clock(lambda: a.patch_tree(src, so, dims, do))
            tp.append(ms)
            sp.append(a.patch_times())
            gp.append(a.info().n_nodes - n0)

            def dense():
                b.patch_volume(src.read_volume(so, dims).contiguous(), do)
            ms, _ = clock(dense)
            tv.append(ms)
            sv.append(b.patch_times())
            gv.append(b.info().n_nodes - n0)

            def listed():
                xyz, ids = src.list_voxels(so, dims)
                c.patch_points((xyz + shift).contiguous(), ids)
            ms, _ = clock(listed)
            tl.append(ms)
            sl.append(c.patch_times())
            gl.append(c.info().n_nodes - n0)
            same = a.count_diff(b) == 0 and a.count_diff(c) == 0
            stored = a.count_voxels()
            del a, b, c
        lines += ["  %d^3 box of src at %r to %r (%d voxels stored): the three routes' trees %s"
                  % (n, so, do, stored, "hold the same voxels" if same else "DIFFER"),
                  "    svo_tree_patch_tree_gpu                        %s, +%d node records" % (med(tp), gp[-1]),
                  "      " + slots(sp),
                  "    read_volume + svo_tree_patch_volume_gpu        %s, +%d node records" % (med(tv), gv[-1]),
                  "      " + slots(sv) + "; the rest is the read",
                  "    list_voxels + shift + svo_tree_patch_points_gpu %s, +%d node records" % (med(tl), gl[-1]),
                  "      " + slots(sl) + "; the rest is the listing",
                  "    cells the destination box cuts, by cell size: %s" % ", ".join(
                      "%d^3: %d" % (4 ** k, spc.box_cut_cells(do, dims, 4 ** k)) for k in range(1, 5))]
    del src

    # ------------------------------------------------------------------------------------------------ scatter --
    import test_gpu_paste_tree as tg

    xyz, ids = tg._scatter7()
    dx, di = torch.from_numpy(xyz).to(dev), torch.from_numpy(ids.view(np.int16)).to(dev)
    src = rt.Tree.points_gpu(7, *none, tg.PAL)
    src.patch_shapes(spc.to_abi(rt, [tg.BOX7, tg.BALL7]))
    lines += ["scatter, 7 levels (16384^3), %d points; src: an empty tree given the 1300^3 box and the carved ball, %d node records"
              % (len(ids), src.info().n_nodes)]
    warm, runs = 1, 4
    tb, sb, gb = [], [], []
    for _ in range(warm + runs):
        t = rt.Tree.points_gpu(7, dx, di, tg.PAL)
        n0 = t.info().n_nodes
        torch.cuda.synchronize()
        ms, _ = clock(lambda: t.patch_tree(src, tg.BOX7[1], tg.BOX7[2], tg.DST7))
        tb.append(ms)
        sb.append(t.patch_times())
        gb.append(t.info().n_nodes - n0)
        stored = t.count_voxels(tg.DST7, tg.BOX7[2][::-1])
        del t
    n_ball = spc.ball_count(tg.BALL7[1], tg.BALL7[2], (0, 0, 0), (4 ** 7,) * 3)
    lines += ["  %d warm-up, median of %d; no other route exists: the box holds %d voxels (a list ends at 2^31 - 1; a dense box is 4.4 GB)"
              % (warm, runs, 1300 ** 3),
              "  1300^3 box of src at %r to %r             %s, +%d node records" % (tg.BOX7[1], tg.DST7, med(tb, warm), gb[-1]),
              "      " + slots(sb, warm),
              "  voxels counted in the destination box afterwards: %d (1300^3 - %d lattice points of the ball: %s)"
              % (stored, n_ball, "equal" if stored == 1300 ** 3 - n_ball else "DIFFERENT"),
              "  cells the destination box cuts, by cell size: %s" % ", ".join(
                  "%d^3: %d" % (4 ** k, spc.box_cut_cells(tg.DST7, tg.BOX7[2], 4 ** k)) for k in range(1, 7)),
              "  cells the source box cuts, by cell size:      %s" % ", ".join(
                  "%d^3: %d" % (4 ** k, spc.box_cut_cells(tg.BOX7[1], tg.BOX7[2], 4 ** k)) for k in range(1, 7))]
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write(text)
    print(text, flush=True)


if __name__ == "__main__":
    main()
