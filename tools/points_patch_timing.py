"""Time of a patch of a resident tree from a sparse list of voxel edits in HBM (svo_tree_patch_points_gpu), on the two
contents of tools/points_build_timing.py:
  scatter  the 7-level world (16384^3) of 1.5 million points
  cavern   the 4-level mini cavern (about 1.3 million stored voxels) as a list
Patches of 1, 1,000 and 15,000 edits scattered over the whole extent, half of them puts at seeded random positions and
half erasures of voxels the list holds.  Every run patches a tree built afresh from the list (the build is not timed), and
is set against svo_build_points_gpu rebuilding the full merged list (the list followed by the edits) in the same process,
interleaved run by run.  Host clock around each call, which ends synchronised; 3 warm-ups, then the median of 10 runs.
The three svo_tree_patch_times slots of every patch are reported as medians too: the device passes, the commit with the
copy back to the host image, the host's ceiling update.  Where the edits' bounding box fits in memory (at most 2^28 voxels)
the same edits are also applied as a dense box through svo_tree_patch_volume_gpu (the box read from the tree, the edits
written into it; only the patch is timed).  After the last run the patched tree and the rebuilt one are looked up at
every edited position and at as many random ones, and the line says whether they agree.
Writes profiles/points_patch.txt (or the path given) with the library's svo_build_id().
usage: python tools/points_patch_timing.py [out.txt]"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

WARM, RUNS = 3, 10
SIZES = (1, 1000, 15000)
BOX_LIMIT = 1 << 28


def edits(levels, xyz, n_ids, k, seed):
    """k edits: (k + 1) // 2 puts at random positions of the extent, k // 2 erasures of listed voxels, shuffled"""
    rng = np.random.default_rng(seed)
    E = 4 ** levels
    n_put = (k + 1) // 2
    put = rng.integers(0, E, (n_put, 3))
    gone = xyz[rng.choice(len(xyz), k - n_put, replace=False)]
    p = np.concatenate([put, gone]).astype(np.int32)
    i = np.concatenate([rng.integers(1, n_ids, n_put), np.zeros(k - n_put, np.int64)]).astype(np.uint16)
    order = rng.permutation(k)
    return np.ascontiguousarray(p[order]), np.ascontiguousarray(i[order])


def clock(f):
    t0 = time.perf_counter()
    r = f()
    return (time.perf_counter() - t0) * 1e3, r


def med(a):
    a = np.asarray(a[WARM:])
    return "%.3f ms (%.3f .. %.3f)" % (np.median(a), a.min(), a.max())


def main():
    import torch

    import points_build_timing as pbt
    import raytracing_test_amd as rt

    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    out_path = args[0] if args else os.path.join(ROOT, "profiles", "points_patch.txt")
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    dev = torch.device("cuda", 0)
    lines = ["svo_build_id %s" % rt.build_id(), "device %s" % torch.cuda.get_device_name(0),
             "host clock around each call, %d warm-ups, median of %d (min .. max); every run patches a freshly built tree" % (WARM, RUNS)]
    for name, (levels, xyz, ids, pal, _) in (("scatter", pbt.scatter()), ("cavern", pbt.cavern())):
        dx, di = torch.from_numpy(xyz).to(dev), torch.from_numpy(ids.view(np.int16)).to(dev)
        E = 4 ** levels
        lines += ["%s, %d levels, %d points" % (name, levels, len(ids))]
        for k in SIZES:
            ex, ei = edits(levels, xyz, len(pal), k, 100 + k)
            dex, dei = torch.from_numpy(ex).to(dev), torch.from_numpy(ei.view(np.int16)).to(dev)
            mx, mi = torch.cat([dx, dex]).contiguous(), torch.cat([di, dei]).contiguous()
            lo, hi = ex.min(0), ex.max(0) + 1
            shape = tuple(int(v) for v in (hi - lo)[::-1])
            fits = int(np.prod([float(s) for s in shape])) <= BOX_LIMIT
            t_patch, t_build, t_box, slots, grow = [], [], [], [], []
            for _ in range(WARM + RUNS):
                t = rt.Tree.points_gpu(levels, dx, di, pal)
                n0 = t.info().n_nodes
                torch.cuda.synchronize()
                ms, _ = clock(lambda: t.patch_points(dex, dei))
                t_patch.append(ms)
                slots.append(t.patch_times())
                grow.append(t.info().n_nodes - n0)
                ms, fresh = clock(lambda: rt.Tree.points_gpu(levels, mx, mi, pal))
                t_build.append(ms)
                if fits:
                    b = rt.Tree.points_gpu(levels, dx, di, pal)
                    box = b.read_volume(tuple(int(v) for v in lo), shape).contiguous()
                    rel = (dex - torch.from_numpy(lo.astype(np.int32)).to(dev)).long()
                    # (the edits of one size hold no voxel twice but by chance: the last entry is written last)
                    for j in range(0, k, 1 << 20):
                        box[rel[j:j + (1 << 20), 2], rel[j:j + (1 << 20), 1], rel[j:j + (1 << 20), 0]] = dei[j:j + (1 << 20)]
                    torch.cuda.synchronize()
                    ms, _ = clock(lambda: b.patch_volume(box, tuple(int(v) for v in lo)))
                    t_box.append(ms)
                    del b, box
            where = torch.cat([dex, torch.from_numpy(np.random.default_rng(9).integers(0, E, ex.shape).astype(np.int32)).to(dev)]).contiguous()
            agree = bool(torch.equal(t.get_blocks_gpu(where), fresh.get_blocks_gpu(where)))
            slots = np.array(slots[WARM:])
            lines += ["  %d edits (%d puts, %d erasures): +%d node records, garbage %s; lookups at the edits and elsewhere %s the rebuilt tree's"
                      % (k, (k + 1) // 2, k // 2, grow[-1], t.garbage(), "equal" if agree else "DIFFER FROM"),
                      "    svo_tree_patch_points_gpu end to end      %s" % med(t_patch),
                      "      device passes %.3f ms, commit + host image %.3f ms, ceilings + top row %.3f ms (medians of svo_tree_patch_times)"
                      % tuple(np.median(slots, 0)),
                      "    svo_build_points_gpu of the merged list    %s" % med(t_build)]
            if fits:
                lines += ["    svo_tree_patch_volume_gpu, the %d x %d x %d bounding box  %s" % (shape[2], shape[1], shape[0], med(t_box))]
            else:
                lines += ["    svo_tree_patch_volume_gpu: not possible (the bounding box of %d x %d x %d voxels does not fit in memory)"
                          % (shape[2], shape[1], shape[0])]
            del t, fresh, dex, dei, mx, mi, where
        del dx, di
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write(text)
    print(text, flush=True)


if __name__ == "__main__":
    main()
