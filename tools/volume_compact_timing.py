"""Time of the compaction of a resident tree on its device (svo_tree_compact_gpu), against the route it replaces: the tree
read back into a dense volume of the whole extent (svo_tree_read_volume) and built again from it (svo_build_volume_gpu).
  worlds    profiles/volume_patch.txt's two volume trees: the generated 1024 x 128 x 1024 and 1024 x 1024 x 1024 volumes
            (tools/volume_build_timing.py generate), 5 levels
  garbage   each tree is patched with that file's two boxes (64^3, then 256 x 64 x 256 over it, at the same origin off the
            brick grid), after which svo_tree_garbage is non-zero
  compact   host clock around the call (it synchronises the device on entry and is complete on return); 3 warm-ups, then
            the median of 10 (min .. max).  Every repetition compacts a freshly built and patched tree (built and patched
            outside the clock).  The call's own phase clocks (svo_tree_compact_times) split it into the device passes
            (reach, classes, emission into the new arrays), the copy back to the host image with the swap, and the
            release of the scratch and the old host image.
  replaced  svo_tree_read_volume of the whole extent (1024^3 voxels, whatever the world holds) and svo_build_volume_gpu of
            that volume, the same run, device and patched content: 3 warm-ups, median of 10.  (The dense volume is
            allocated outside the clock.)
The compacted tree is checked against the rebuilt one, record for record, before anything is written.
Writes profiles/volume_compact.txt (or the path given) with the library's svo_build_id().
usage: python tools/volume_compact_timing.py [out.txt]"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from volume_build_timing import PAL, generate  # noqa: E402
from volume_patch_timing import BOXES, ORIGIN, RUNS, WARM, med  # noqa: E402

LEVELS, E = 5, 1024


def main():
    import torch

    import raytracing_test_amd as rt

    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    out_path = args[0] if args else os.path.join(ROOT, "profiles", "volume_compact.txt")
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    dev = torch.device("cuda", 0)
    lines = ["svo_build_id %s" % rt.build_id(), "device %s" % torch.cuda.get_device_name(0),
             "trees patched with boxes %s at origin %s (off the brick grid on every axis), random content, half filled; "
             "%d warm-ups, median of %d (min .. max)" % (" then ".join("%d x %d x %d" % b for b in BOXES), ORIGIN, WARM, RUNS)]
    g = torch.Generator(device=dev)
    g.manual_seed(7)
    boxes = []
    for nx, ny, nz in BOXES:
        ids = torch.randint(1, 4, (nz, ny, nx), device=dev, generator=g, dtype=torch.int16)
        keep = torch.rand((nz, ny, nx), device=dev, generator=g) < 0.5
        boxes.append(torch.where(keep, ids, torch.zeros_like(ids)).contiguous())

    def patched(vol):
        t = rt.Tree.volume_gpu(LEVELS, vol, PAL)
        for box in boxes:
            t.patch_volume(box, ORIGIN)
        assert t.garbage()[0] > 0
        return t

    verdict = None
    for wx, wy, wz in ((1024, 128, 1024), (1024, 1024, 1024)):
        vol = generate(torch, wx, wy, wz, dev)
        dense = torch.empty((E, E, E), dtype=torch.int16, device=dev)
        torch.cuda.synchronize()
        ts, ph, before = [], [], None
        for i in range(WARM + RUNS):
            t = patched(vol)
            if before is None:
                before = (t.info().n_nodes, t.info().n_mat_bytes // 2, t.garbage(), t.info().device_bytes)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            t.compact()
            ts.append((time.perf_counter() - t0) * 1e3)
            ph.append(t.compact_times())
        after = (t.info().n_nodes, t.info().n_mat_bytes // 2, t.garbage(), t.info().device_bytes)
        rd, bd = [], []
        for i in range(WARM + RUNS):
            u = patched(vol)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            u.read_volume((0, 0, 0), (E, E, E), out=dense)
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            f = rt.Tree.volume_gpu(LEVELS, dense, PAL)
            t2 = time.perf_counter()
            rd.append((t1 - t0) * 1e3)
            bd.append((t2 - t1) * 1e3)
            if i < WARM + RUNS - 1:
                del f
            del u
        for a, b in zip(t.export(), f.export()):
            assert a.tobytes() == b.tobytes(), "the compacted tree is not the rebuilt one"
        assert after[0] == f.info().n_nodes and after[3] == f.info().device_bytes and after[2] == (0, 0)
        ts, ph, rd, bd = np.array(ts[WARM:]), np.array(ph[WARM:]), np.array(rd[WARM:]), np.array(bd[WARM:])
        lines += ["world %d x %d x %d, %d levels (the dense extent: %.0f MB)" % (wx, wy, wz, LEVELS, 2.0 * E ** 3 / 1e6),
                  "  before: %d nodes, %d material entries (garbage %d nodes, %d material entries), %d device bytes"
                  % (before[0], before[1], before[2][0], before[2][1], before[3]),
                  "  after:  %d nodes, %d material entries, %d device bytes; equal to the rebuilt tree record for record"
                  % (after[0], after[1], after[3]),
                  "    svo_tree_compact_gpu             %s" % med(ts),
                  "      device passes                  %s" % med(ph[:, 0]),
                  "      host image + swap              %s" % med(ph[:, 1]),
                  "      release of scratch, old image  %s" % med(ph[:, 2]),
                  "    the route it replaces            %s" % med(rd + bd),
                  "      svo_tree_read_volume, %d^3   %s" % (E, med(rd)),
                  "      svo_build_volume_gpu of it     %s" % med(bd)]
        if (wx, wy, wz) == (1024, 1024, 1024):
            a, b = float(np.median(ts)), float(np.median(rd + bd))
            verdict = "condition (1024^3: the compaction's median is not above the replaced route's): %s (%.3f ms against %.3f ms)" % (
                "holds" if a <= b else "FAILED", a, b)
        del t, f, vol, dense
    lines.append(verdict)
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write(text)
    print(text, flush=True)


if __name__ == "__main__":
    main()
