"""Time of the diff of two resident trees (svo_tree_diff_gpu), count-only calls and full diffs, on three worlds, each against
a copy of itself changed by 1, 1,000 and 15,000 edits through svo_tree_patch_points_gpu:
  cavern   the 4-level mini cavern of tests/volume_cases.py (256 x 64 x 256, about 1.4 million stored voxels), volume-built
  terrain  svo_build_terrain_gpu over 1024 x 1024 columns at 5 levels (1024^3)
  scatter  the 7-level world of tools/points_build_timing.py (16384^3): a million seeded points plus aligned full 4^3 and
           16^3 blocks, points-built
The edits are seeded: stored voxels of the world drawn without replacement, every other one (the first included) erased, the
rest given the id of another stored voxel (an edit that draws the id the voxel already has changes nothing and is no
difference).
The route the diff replaces is timed in the same run, on the same build: svo_tree_list_voxels_gpu of both trees into
buffers allocated once, and a torch merge of the two lists by key (keys, a searchsorted, a compare, a final sort) — "not
possible" where that does not fit in memory.  Host clock around each call — the diff ends with its stream waited for, the
list route with a synchronize — 3 warm-ups, then the median of 10 runs with min .. max.  No threshold is set for these times.
Writes profiles/diff_voxels.txt (or the path given) with the library's svo_build_id() on the first line.
usage: python tools/diff_voxels_timing.py [out.txt]"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

WARM, RUNS = 3, 10
EDITS = (1, 1000, 15000)


def times(f):
    ts = []
    for _ in range(WARM + RUNS):
        t0 = time.perf_counter()
        r = f()
        ts.append(time.perf_counter() - t0)
    return np.array(ts[WARM:]) * 1e3, r


def fmt(ts):
    return "%.3f ms (%.3f .. %.3f)" % (np.median(ts), ts.min(), ts.max())


def key_of(torch, xyz, levels):
    """the point builder's key of every row (tests/list_voxels_cases.py key_of, in torch)"""
    p = xyz.to(torch.int64)
    key = torch.zeros(len(p), dtype=torch.int64, device=p.device)
    for d in range(levels):
        sh = 2 * (levels - 1 - d)
        key = (key << 6) | (((p[:, 2] >> sh) & 3) << 4) | (((p[:, 1] >> sh) & 3) << 2) | ((p[:, 0] >> sh) & 3)
    return key


def merge(torch, a, b, levels):
    """the diff from two key-ordered lists: b's entries that a lacks or holds with another id, a's entries that b lacks
    with id 0, in key order"""
    (ax, ai), (bx, bi) = a, b
    ka, kb = key_of(torch, ax, levels), key_of(torch, bx, levels)
    at = torch.searchsorted(ka, kb)
    hit = torch.zeros(len(kb), dtype=torch.bool, device=kb.device)
    inside = at < len(ka)
    hit[inside] = ka[at[inside]] == kb[inside]
    same = hit.clone()
    same[hit] = ai[at[hit]] == bi[hit]
    gone = torch.ones(len(ka), dtype=torch.bool, device=ka.device)
    gone[at[hit]] = False
    xyz = torch.cat([bx[~same], ax[gone]])
    ids = torch.cat([bi[~same], torch.zeros(int(gone.sum()), dtype=bi.dtype, device=bi.device)])
    order = torch.argsort(torch.cat([kb[~same], ka[gone]]))
    return xyz[order], ids[order]


def main():
    import torch

    import points_build_timing as pbt
    import raytracing_test_amd as rt

    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    out_path = args[0] if args else os.path.join(ROOT, "profiles", "diff_voxels.txt")
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    dev = torch.device("cuda", 0)
    lines = ["svo_build_id %s" % rt.build_id(), "device %s" % torch.cuda.get_device_name(0),
             "host clock around each call, %d warm-ups, median of %d (min .. max)" % (WARM, RUNS)]

    def cavern():
        levels, _, _, pal, vol = pbt.cavern()
        return rt.Tree.volume_gpu(levels, vol, pal)

    def terrain():
        return rt.Tree.terrain_gpu(5, 1024, 1024, 0)

    def scatter():
        levels, xyz, ids, pal, _ = pbt.scatter()
        return rt.Tree.points_gpu(levels, xyz, ids, pal)

    for name, make in (("cavern", cavern), ("terrain", terrain), ("scatter", scatter)):
        a = make()
        info = a.info()
        levels, E = info.levels, 4 ** info.levels
        ax, ai = a.list_voxels()
        n_a = len(ai)
        lines += ["%s, %d levels (%d^3), %d nodes, %d bricks: %d stored voxels" % (name, levels, E, info.n_nodes, info.n_bricks, n_a)]
        g = torch.Generator(device="cpu").manual_seed(4242)
        for n_edits in EDITS:
            b = make()
            pick = torch.randperm(n_a, generator=g)[:2 * n_edits].to(dev)
            exyz = ax[pick[:n_edits]].contiguous()
            eids = ai[pick[n_edits:]].clone()
            eids[0::2] = 0
            b.patch_points(exyz, eids)
            torch.cuda.synchronize()
            tc, n = times(lambda: a.count_diff(b))
            xyz = torch.empty((max(n, 1), 3), dtype=torch.int32, device=dev)
            ids = torch.empty((max(n, 1),), dtype=torch.int16, device=dev)
            td, got = times(lambda: a.diff_voxels(b, out=(xyz, ids)))
            assert len(got[1]) == n
            lines += ["  %d edits: %d voxels differ" % (n_edits, n),
                      "    count only                          %s" % fmt(tc),
                      "    full diff                           %s" % fmt(td)]
            try:
                n_b = b.count_voxels()
                la = (torch.empty((n_a, 3), dtype=torch.int32, device=dev), torch.empty((n_a,), dtype=torch.int16, device=dev))
                lb = (torch.empty((n_b, 3), dtype=torch.int32, device=dev), torch.empty((n_b,), dtype=torch.int16, device=dev))

                def lists():
                    r = merge(torch, a.list_voxels(out=la), b.list_voxels(out=lb), levels)
                    torch.cuda.synchronize()
                    return r

                tl, (mx, mi) = times(lists)
                same = len(mi) == n and bool(torch.equal(mx, got[0])) and bool(torch.equal(mi, got[1]))
                ratio = np.median(tl) / np.median(td)
                lines += ["    list_voxels of both + torch merge   %s; the diff is %.1f x %s; %s"
                          % (fmt(tl), max(ratio, 1.0 / ratio), "faster" if ratio > 1.0 else "SLOWER", "same list" if same else "DIFFERENT list")]
                del la, lb, mx, mi
            except torch.OutOfMemoryError:
                lines += ["    list_voxels of both + torch merge   not possible (the lists and the merge do not fit in memory)"]
            del b, xyz, ids, got
            torch.cuda.empty_cache()
        del a, ax, ai
        torch.cuda.empty_cache()
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write(text)
    print(text, flush=True)


if __name__ == "__main__":
    main()
