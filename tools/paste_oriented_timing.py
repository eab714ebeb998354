"""Time of the oriented paste (svo_tree_patch_tree_oriented_gpu) beside the plain one (svo_tree_patch_tree_gpu), on one
run, over the boxes of tools/paste_tree_timing.py:
  terrain  the 5-level terrain tree (1024^3) as src, an empty 5-level tree as dst: the off-grid 64^3 and 256^3 boxes
  scatter  the 7-level world (16384^3) of tests/test_gpu_paste_tree.py: the 1300^3 region with a ball carved out of it,
           pasted into the scattered world at an offset odd on every axis
Four routes per box, interleaved run by run, their order rotated from run to run (the slot "commit + host image" is
reported by position in that order too: it is the same function with the same arguments for every route, and what differs
is which tree of a run is committed first): patch_tree; patch_tree_oriented with the identity orientation and no map
(the same content: the trees are compared); patch_tree_oriented under a quarter turn about y (axis (2, 1, 0), flip
(0, 0, 1)) without a map, and the same with a map that exchanges two ids (the difference between the last two is the
map: its upload, one allocation and one synchronous copy per call, and one table load after each walk).
Every run pastes into a tree built afresh (the builds are not timed).  Host clock around each call, which ends
synchronised; WARM warm-ups, then the median of RUNS runs with their range, and the medians of svo_tree_patch_times' three
slots (device passes, commit with the copy back to the host image, the host's ceiling update).
The expectation: per cell the oriented paste makes the plain paste's eight walks of the same trip counts — the affine map
costs a few integer instructions per cell, the id map one 2-byte load per walk — so its time should lie within the plain
paste's own min-to-max range of the same run.  The last line of each box says whether it did.
Writes profiles/paste_oriented.txt (or the path given) with the library's svo_build_id().
usage: python tools/paste_oriented_timing.py [out.txt]"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

from paste_tree_timing import BOXES5, E5, RUNS, WARM, clock, med, slots  # noqa: E402

QUARTER_Y = ((2, 1, 0), (0, 0, 1))


def verdict(plain, other, warm):
    p, o = np.asarray(plain[warm:]), float(np.median(other[warm:]))
    return "within the plain paste's range" if p.min() <= o <= p.max() else ("below the plain paste's range" if o < p.min() else "ABOVE the plain paste's range")


def routes(rt, torch, fresh, src, so, dims, do, swap, warm, runs):
    """the four routes, interleaved; returns the report lines"""
    names = ("svo_tree_patch_tree_gpu", "oriented, identity, no map", "oriented, quarter turn about y, no map",
             "oriented, quarter turn about y, ids swapped")
    t, s, g = ([], [], [], []), ([], [], [], []), ([], [], [], [])
    by_pos = ([], [], [], [])  # the commit slot by position in the run's order, after the warm-ups
    same = True
    for run in range(warm + runs):
        trees = [fresh() for _ in range(4)]
        n0 = trees[0].info().n_nodes
        torch.cuda.synchronize()
        calls = (lambda: trees[0].patch_tree(src, so, dims, do), lambda: trees[1].patch_tree_oriented(src, so, dims, do),
                 lambda: trees[2].patch_tree_oriented(src, so, dims, do, axis=QUARTER_Y[0], flip=QUARTER_Y[1]),
                 lambda: trees[3].patch_tree_oriented(src, so, dims, do, axis=QUARTER_Y[0], flip=QUARTER_Y[1], id_map=swap))
        for pos in range(4):
            i = (pos + run) % 4
            ms, _ = clock(calls[i])
            t[i].append(ms)
            s[i].append(trees[i].patch_times())
            g[i].append(trees[i].info().n_nodes - n0)
            if run >= warm:
                by_pos[pos].append(s[i][-1][1])
        same = same and trees[0].count_diff(trees[1]) == 0
        del trees
    lines = []
    for i, name in enumerate(names):
        lines += ["    %-46s %s, +%d node records" % (name, med(t[i], warm), g[i][-1]), "      " + slots(s[i], warm)]
    lines += ["    commit + host image by position in a run's order, whatever the route: %s ms (medians)" % ", ".join("%.3f" % np.median(b) for b in by_pos),
              "    the identity route's tree %s the plain paste's" % ("holds the same voxels as" if same else "DIFFERS from"),
              "    identity: %s; quarter turn: %s; quarter turn with map: %s"
              % (verdict(t[0], t[1], warm), verdict(t[0], t[2], warm), verdict(t[0], t[3], warm))]
    return lines


def main():
    import torch

    import raytracing_test_amd as rt
    import shapes_patch_cases as spc
    import test_gpu_paste_tree as tg

    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    out_path = args[0] if args else os.path.join(ROOT, "profiles", "paste_oriented.txt")
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    dev = torch.device("cuda", 0)
    lines = ["svo_build_id %s" % rt.build_id(), "device %s" % torch.cuda.get_device_name(0),
             "host clock around each call, %d warm-ups, median of %d (min .. max); every run pastes into a freshly built tree; the four routes"
             " are interleaved run by run, their order rotated from run to run" % (WARM, RUNS),
             "expectation: the per-cell work is the same eight walks, so the oriented routes lie within the plain paste's own range"]

    src = rt.Tree.terrain_gpu(5, E5, E5, 0)
    pal = src.palette()
    none = (np.zeros((0, 3), np.int32), np.zeros(0, np.uint16))
    swap = list(range(len(pal)))
    if len(swap) > 2:
        swap[1], swap[2] = 2, 1
    lines += ["terrain, 5 levels (1024^3), %d node records, %d palette entries, into an empty 5-level tree" % (src.info().n_nodes, len(pal))]
    for so, n, do in BOXES5:
        lines += ["  %d^3 box of src at %r to %r" % (n, so, do)]
        lines += routes(rt, torch, lambda: rt.Tree.points_gpu(5, *none, pal), src, so, (n, n, n), do, swap, WARM, RUNS)
    del src

    xyz, ids = tg._scatter7()
    dx, di = torch.from_numpy(xyz).to(dev), torch.from_numpy(ids.view(np.int16)).to(dev)
    src = rt.Tree.points_gpu(7, *none, tg.PAL)
    src.patch_shapes(spc.to_abi(rt, [tg.BOX7, tg.BALL7]))
    swap7 = list(range(len(tg.PAL)))
    swap7[2], swap7[3] = 3, 2
    lines += ["scatter, 7 levels (16384^3), %d points; src: an empty tree given the 1300^3 box and the carved ball, %d node records"
              % (len(ids), src.info().n_nodes),
              "  1300^3 box of src at %r to %r, 1 warm-up, median of 4" % (tg.BOX7[1], tg.DST7)]
    lines += routes(rt, torch, lambda: rt.Tree.points_gpu(7, dx, di, tg.PAL), src, tg.BOX7[1], tg.BOX7[2], tg.DST7, swap7, 1, 4)
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write(text)
    print(text, flush=True)


if __name__ == "__main__":
    main()
