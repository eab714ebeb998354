"""Time of the rule paste (svo_tree_patch_tree_rule_gpu) beside the oriented one (svo_tree_patch_tree_oriented_gpu), on one
run, over the boxes of tools/paste_tree_timing.py and tools/paste_oriented_timing.py:
  terrain  the 5-level terrain tree (1024^3) as src, an empty 5-level tree as dst: the off-grid 64^3 and 256^3 boxes
  scatter  the 7-level world (16384^3) of tests/test_gpu_paste_tree.py: the 1300^3 region with a ball carved out of it,
           pasted into the scattered world at an offset odd on every axis
Seven routes per box, interleaved run by run, their order rotated from run to run: the oriented paste under REPLACE and
under KEEP_EMPTY (the yardstick), the rule paste under RULE_REPLACE and RULE_OVER with the same arguments (the same content:
the trees are compared), and RULE_UNDER, RULE_PAINT and RULE_ERASE on the same boxes, with the records each route appends.
All under the identity orientation, without a map.
Every run pastes into a tree built afresh (the builds are not timed).  Host clock around each call, which ends
synchronised; WARM warm-ups, then the median of RUNS runs with their range, and the medians of svo_tree_patch_times' three
slots (device passes, commit with the copy back to the host image, the host's ceiling update).
The expectation: per cell the rule paste makes nine walks where the oriented paste makes eight (the ninth over dst), so its
device-passes slot should exceed the oriented paste's by about one eighth of what the walks cost, and the commit and the
ceilings, which depend on the appended records and the box alone, should be equal.  The lines "rule / oriented" give the
ratios of the slots' medians for the two pairs of equal content.
Writes profiles/paste_rule.txt (or the path given) with the library's svo_build_id().
usage: python tools/paste_rule_timing.py [out.txt]"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

from paste_tree_timing import BOXES5, E5, RUNS, WARM, clock, med, slots  # noqa: E402


def routes(rt, torch, fresh, src, so, dims, do, warm, runs):
    """the seven routes, interleaved; returns the report lines"""
    names = ("oriented, REPLACE", "rule, RULE_REPLACE", "oriented, KEEP_EMPTY", "rule, RULE_OVER", "rule, RULE_UNDER", "rule, RULE_PAINT",
             "rule, RULE_ERASE")
    n = len(names)
    t, s, g = [[] for _ in range(n)], [[] for _ in range(n)], [[] for _ in range(n)]
    same = True
    for run in range(warm + runs):
        trees = [fresh() for _ in range(n)]
        n0 = trees[0].info().n_nodes
        torch.cuda.synchronize()
        calls = (lambda: trees[0].patch_tree_oriented(src, so, dims, do), lambda: trees[1].patch_tree_rule(src, so, dims, do, rt.RULE_REPLACE),
                 lambda: trees[2].patch_tree_oriented(src, so, dims, do, keep_empty=True), lambda: trees[3].patch_tree_rule(src, so, dims, do, rt.RULE_OVER),
                 lambda: trees[4].patch_tree_rule(src, so, dims, do, rt.RULE_UNDER), lambda: trees[5].patch_tree_rule(src, so, dims, do, rt.RULE_PAINT),
                 lambda: trees[6].patch_tree_rule(src, so, dims, do, rt.RULE_ERASE))
        for pos in range(n):
            i = (pos + run) % n
            ms, _ = clock(calls[i])
            t[i].append(ms)
            s[i].append(trees[i].patch_times())
            g[i].append(trees[i].info().n_nodes - n0)
        same = same and trees[0].count_diff(trees[1]) == 0 and trees[2].count_diff(trees[3]) == 0
        del trees
    lines = []
    for i, name in enumerate(names):
        lines += ["    %-24s %s, +%d node records" % (name, med(t[i], warm), g[i][-1]), "      " + slots(s[i], warm)]
    lines += ["    the rule routes' trees %s the oriented paste's" % ("hold the same voxels as" if same else "DIFFER from")]
    for a, b, what in ((0, 1, "RULE_REPLACE / REPLACE"), (2, 3, "RULE_OVER / KEEP_EMPTY")):
        ma, mb = np.median(np.asarray(s[a][warm:]), 0), np.median(np.asarray(s[b][warm:]), 0)
        lines += ["    rule / oriented, %s: device passes %.3f (+%.3f ms), commit + host image %.3f, ceilings + top row %.3f; records +%d / +%d"
                  % (what, mb[0] / ma[0], mb[0] - ma[0], mb[1] / ma[1], mb[2] / ma[2], g[b][-1], g[a][-1])]
    return lines


def main():
    import torch

    import raytracing_test_amd as rt
    import shapes_patch_cases as spc
    import test_gpu_paste_tree as tg

    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    out_path = args[0] if args else os.path.join(ROOT, "profiles", "paste_rule.txt")
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    dev = torch.device("cuda", 0)
    lines = ["svo_build_id %s" % rt.build_id(), "device %s" % torch.cuda.get_device_name(0),
             "host clock around each call, %d warm-ups, median of %d (min .. max); every run pastes into a freshly built tree; the seven routes"
             " are interleaved run by run, their order rotated from run to run" % (WARM, RUNS),
             "expectation: nine walks per cell where the oriented paste makes eight, so the device-passes slot exceeds the oriented paste's by"
             " about the ninth walk, and commit and ceilings are equal"]

    src = rt.Tree.terrain_gpu(5, E5, E5, 0)
    pal = src.palette()
    none = (np.zeros((0, 3), np.int32), np.zeros(0, np.uint16))
    lines += ["terrain, 5 levels (1024^3), %d node records, %d palette entries, into an empty 5-level tree" % (src.info().n_nodes, len(pal))]
    for so, n, do in BOXES5:
        lines += ["  %d^3 box of src at %r to %r" % (n, so, do)]
        lines += routes(rt, torch, lambda: rt.Tree.points_gpu(5, *none, pal), src, so, (n, n, n), do, WARM, RUNS)
    del src

    xyz, ids = tg._scatter7()
    dx, di = torch.from_numpy(xyz).to(dev), torch.from_numpy(ids.view(np.int16)).to(dev)
    src = rt.Tree.points_gpu(7, *none, tg.PAL)
    src.patch_shapes(spc.to_abi(rt, [tg.BOX7, tg.BALL7]))
    lines += ["scatter, 7 levels (16384^3), %d points; src: an empty tree given the 1300^3 box and the carved ball, %d node records"
              % (len(ids), src.info().n_nodes),
              "  1300^3 box of src at %r to %r, 1 warm-up, median of 4" % (tg.BOX7[1], tg.DST7)]
    lines += routes(rt, torch, lambda: rt.Tree.points_gpu(7, dx, di, tg.PAL), src, tg.BOX7[1], tg.BOX7[2], tg.DST7, 1, 4)
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write(text)
    print(text, flush=True)


if __name__ == "__main__":
    main()
