"""Time of a tree build from a sparse list of voxels in HBM (svo_build_points_gpu) and of the device-side lookup
(svo_tree_get_blocks_gpu), on two contents:
  cavern   the 4-level mini cavern of tests/volume_cases.py (256 x 64 x 256, about 1.4 million stored voxels) as a
           shuffled list; the same content built by svo_build_volume_gpu from the dense volume for comparison
  scatter  a 7-level world (16384^3): seeded random points over the whole extent plus aligned full 4^3 and 16^3 blocks —
           a content svo_build_volume_gpu cannot build at all (its pyramid spans the bounding box: the whole extent)
Builds: host clock around the call, which ends synchronised (its host image is copied back); 3 warm-ups, then the median
of 10 runs.  Lookups: HIP events around svo_tree_get_blocks_gpu over the list's own positions followed by as many seeded
random positions, per million lookups; 3 warm-ups, median of 10.
Writes profiles/points_build.txt (or the path given) with the library's svo_build_id().
usage: python tools/points_build_timing.py [out.txt]"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

EMPTY = (0, 0xFFFFFFFFFFFFFFFF, 0.0)
WARM, RUNS = 3, 10


def cavern():
    import volume_cases as vc

    vol, _ = vc.mini_cavern()
    pal = [EMPTY] + [(1 | f, c, 0.0) for f, c in vc.TABLE[1:]]
    z, y, x = np.nonzero(vol)
    order = np.random.default_rng(1).permutation(len(z))
    xyz = np.stack([x, y, z], 1).astype(np.int32)[order]
    return 4, np.ascontiguousarray(xyz), np.ascontiguousarray(vol[z, y, x][order]), pal, vol


def scatter(n=1000000):
    E = 4 ** 7
    rng = np.random.default_rng(7)
    parts = [rng.integers(0, E, (n, 3))]
    ids = [rng.integers(1, 4, n)]
    g = np.stack(np.meshgrid(np.arange(16), np.arange(16), np.arange(16), indexing="ij"), -1).reshape(-1, 3)
    for c in rng.integers(0, E // 16, (64, 3)) * 16:    # 64 aligned 16^3 blocks of one material
        parts.append(c + g)
        ids.append(np.full(len(g), 2))
    for c in rng.integers(0, E // 4, (4096, 3)) * 4:     # 4096 aligned full bricks
        parts.append(c + g[(g < 4).all(1)])
        ids.append(np.full(64, 3))
    pal = [EMPTY, (1, 0x111, 0.0), (1, 0x222, 0.0), (1, 0x333, 0.0)]
    return 7, np.ascontiguousarray(np.concatenate(parts).astype(np.int32)), np.ascontiguousarray(np.concatenate(ids).astype(np.uint16)), pal, None


def times(f):
    ts = []
    for _ in range(WARM + RUNS):
        t0 = time.perf_counter()
        r = f()
        ts.append(time.perf_counter() - t0)
    return np.array(ts[WARM:]) * 1e3, r


def main():
    import torch

    import raytracing_test_amd as rt

    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    out_path = args[0] if args else os.path.join(ROOT, "profiles", "points_build.txt")
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    dev = torch.device("cuda", 0)
    lines = ["svo_build_id %s" % rt.build_id(), "device %s" % torch.cuda.get_device_name(0),
             "builds: host clock, %d warm-ups, median of %d (min .. max); lookups: HIP events, the same" % (WARM, RUNS)]
    for name, (levels, xyz, ids, pal, vol) in (("cavern", cavern()), ("scatter", scatter())):
        dx, di = torch.from_numpy(xyz).to(dev), torch.from_numpy(ids.view(np.int16)).to(dev)
        torch.cuda.synchronize()
        ts, t = times(lambda: rt.Tree.points_gpu(levels, dx, di, pal))
        info = t.info()
        lines += ["%s, %d levels, %d points: nodes %d (per level %s), bricks %d, material entries %d"
                  % (name, levels, len(ids), info.n_nodes, list(info.nodes_per_level)[:levels], info.n_bricks, info.n_mat_bytes // 2),
                  "  svo_build_points_gpu end to end   %.3f ms (%.3f .. %.3f)" % (np.median(ts), ts.min(), ts.max())]
        if vol is not None:
            dv = torch.from_numpy(vol.view(np.int16)).to(dev)
            torch.cuda.synchronize()
            tv, v = times(lambda: rt.Tree.volume_gpu(levels, dv, pal))
            same = all(np.array_equal(a, b) for a, b in zip(t.export(), v.export()))
            lines += ["  svo_build_volume_gpu of the dense %d x %d x %d volume  %.3f ms (%.3f .. %.3f); the two trees are %s"
                      % (vol.shape[2], vol.shape[1], vol.shape[0], np.median(tv), tv.min(), tv.max(), "byte-equal" if same else "DIFFERENT")]
            del v, dv
        else:
            lines += ["  svo_build_volume_gpu: not possible (the dense volume of this extent would be 8.8 TB)"]
        E = 4 ** levels
        where = torch.cat([dx, torch.from_numpy(np.random.default_rng(9).integers(0, E, xyz.shape).astype(np.int32)).to(dev)]).contiguous()
        out = torch.empty(len(where), dtype=torch.int16, device=dev)
        ms = []
        for _ in range(WARM + RUNS):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            t.get_blocks_gpu(where, out=out, stream=torch.cuda.current_stream())
            e1.record()
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
        ms = np.array(ms[WARM:])
        per_m = ms / (len(where) / 1e6)
        lines += ["  svo_tree_get_blocks_gpu, %d lookups  %.4f ms (%.4f .. %.4f) = %.4f ms per million; %d of them found a voxel"
                  % (len(where), np.median(ms), ms.min(), ms.max(), np.median(per_m), int((out != 0).sum()))]
        del t, dx, di, where, out
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write(text)
    print(text, flush=True)


if __name__ == "__main__":
    main()
