"""Time of the voxel listing of a resident tree (svo_tree_list_voxels_gpu), count-only calls and full lists, on three trees:
  cavern   the 4-level mini cavern of tests/volume_cases.py (256 x 64 x 256, about 1.4 million stored voxels), volume-built
  scatter  the 7-level world of tools/points_build_timing.py (16384^3): a million seeded points plus aligned full 4^3 and
           16^3 blocks, points-built
  terrain  svo_build_terrain_gpu over 1024 x 1024 columns at 5 levels (1024^3)
Where the dense box fits (cavern, terrain) the route the listing replaces is timed in the same run: svo_tree_read_volume of
the whole extent, torch.nonzero, and a gather of the ids (its positions come out in z, y, x order, not in key order).
Host clock around each call — the listing ends with its stream waited for, the dense route with a synchronize — 3 warm-ups,
then the median of 10 runs with min .. max.  Full lists go into buffers allocated once (out=), so a run is one call.
Writes profiles/list_voxels.txt (or the path given) with the library's svo_build_id() on the first line.
usage: python tools/list_voxels_timing.py [out.txt]"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

WARM, RUNS = 3, 10


def times(f):
    ts = []
    for _ in range(WARM + RUNS):
        t0 = time.perf_counter()
        r = f()
        ts.append(time.perf_counter() - t0)
    return np.array(ts[WARM:]) * 1e3, r


def fmt(ts):
    return "%.3f ms (%.3f .. %.3f)" % (np.median(ts), ts.min(), ts.max())


def main():
    import torch

    import points_build_timing as pbt
    import raytracing_test_amd as rt

    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    out_path = args[0] if args else os.path.join(ROOT, "profiles", "list_voxels.txt")
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    dev = torch.device("cuda", 0)
    lines = ["svo_build_id %s" % rt.build_id(), "device %s" % torch.cuda.get_device_name(0),
             "host clock around each call, %d warm-ups, median of %d (min .. max)" % (WARM, RUNS)]

    def cavern():
        levels, _, _, pal, vol = pbt.cavern()
        return rt.Tree.volume_gpu(levels, vol, pal), True

    def scatter():
        levels, xyz, ids, pal, _ = pbt.scatter()
        return rt.Tree.points_gpu(levels, xyz, ids, pal), False

    def terrain():
        return rt.Tree.terrain_gpu(5, 1024, 1024, 0), True

    for name, make in (("cavern", cavern), ("scatter", scatter), ("terrain", terrain)):
        t, dense_fits = make()
        info = t.info()
        E = 4 ** info.levels
        torch.cuda.synchronize()
        tc, n = times(t.count_voxels)
        xyz = torch.empty((n, 3), dtype=torch.int32, device=dev)
        ids = torch.empty((n,), dtype=torch.int16, device=dev)
        tl, got = times(lambda: t.list_voxels(out=(xyz, ids)))
        assert len(got[1]) == n
        lines += ["%s, %d levels (%d^3), %d nodes, %d bricks: %d stored voxels" % (name, info.levels, E, info.n_nodes, info.n_bricks, n),
                  "  count only, whole extent          %s" % fmt(tc),
                  "  full list, whole extent           %s = %.4f ms per million voxels" % (fmt(tl), np.median(tl) / (n / 1e6))]
        lo = E // 2 - 50                                     # a box off every grid: 100^3 on the ground, mid-extent in x and z
        tb, nb = times(lambda: t.count_voxels((lo, 0, lo), (100, 100, 100)))
        bx, bi = torch.empty((nb, 3), dtype=torch.int32, device=dev), torch.empty((nb,), dtype=torch.int16, device=dev)
        tbl, _ = times(lambda: t.list_voxels((lo, 0, lo), (100, 100, 100), out=(bx, bi)))
        lines += ["  100^3 box at (%d, 0, %d): %d voxels; count only %s; full list %s" % (lo, lo, nb, fmt(tb), fmt(tbl))]
        if dense_fits:
            vol = torch.empty((E, E, E), dtype=torch.int16, device=dev)

            def dense():
                t.read_volume((0, 0, 0), (E, E, E), out=vol)
                at = torch.nonzero(vol)
                what = vol[at[:, 0], at[:, 1], at[:, 2]]
                torch.cuda.synchronize()
                return at, what

            td, (at, what) = times(dense)
            same = len(what) == n and bool(torch.equal(torch.sort(what.to(torch.int32))[0], torch.sort(ids.to(torch.int32))[0]))
            lines += ["  read_volume of %d^3 (%.2f GB) + torch.nonzero + gather  %s; the listing is %.1f x %s; %s"
                      % (E, 2.0 * E ** 3 / 1e9, fmt(td), max(np.median(td) / np.median(tl), np.median(tl) / np.median(td)),
                         "faster" if np.median(tl) < np.median(td) else "SLOWER", "same voxels" if same else "DIFFERENT voxels")]
            del vol, at, what
        else:
            lines += ["  read_volume: not possible (the dense volume of this extent would be 8.8 TB)"]
        del t, xyz, ids, got, bx, bi
        torch.cuda.empty_cache()
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write(text)
    print(text, flush=True)


if __name__ == "__main__":
    main()
