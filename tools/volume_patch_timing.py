"""Time of a patch of a resident tree from a dense box of voxels in HBM (svo_tree_patch_volume_gpu), against the rebuild
it replaces: svo_build_volume_gpu over the whole world holding the same content.
  worlds   profiles/volume_build.txt's two volume trees: the generated 1024 x 128 x 1024 and 1024 x 1024 x 1024 volumes
           (tools/volume_build_timing.py generate), 5 levels
  boxes    64 x 64 x 64 and 256 x 64 x 256 voxels of seeded random content (half filled, three materials) at an origin
           off the brick grid on every axis, the same box into both worlds
  patch    host clock around the call (it synchronises the device on entry and is complete on return); 3 warm-ups, then
           the median of 10 (min .. max).  Every repetition patches a freshly built tree (built outside the clock), so
           each is the first patch of that tree and no tail of earlier repetitions is in the arrays.  The call's own phase clocks
           (svo_tree_patch_times) split it into the device passes, the commit with the copy back to the host image, and
           the host's ceiling update.
  rebuild  svo_build_volume_gpu of the whole world's volume with the box written into it, the same run and device:
           3 warm-ups, median of 10.
Writes profiles/volume_patch.txt (or the path given) with the library's svo_build_id().
usage: python tools/volume_patch_timing.py [out.txt]"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from volume_build_timing import PAL, generate  # noqa: E402

ORIGIN = (301, 62, 415)  # residues mod 4: 1, 2, 3
BOXES = ((64, 64, 64), (256, 64, 256))  # (nx, ny, nz)
WARM, RUNS = 3, 10


def med(a):
    a = np.asarray(a, float)
    return "%.3f ms (%.3f .. %.3f)" % (np.median(a), a.min(), a.max())


def main():
    import torch

    import raytracing_test_amd as rt

    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    out_path = args[0] if args else os.path.join(ROOT, "profiles", "volume_patch.txt")
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    dev = torch.device("cuda", 0)
    lines = ["svo_build_id %s" % rt.build_id(), "device %s" % torch.cuda.get_device_name(0),
             "boxes at origin %s (off the brick grid on every axis), random content, half filled; %d warm-ups, median of %d (min .. max)"
             % (ORIGIN, WARM, RUNS)]
    g = torch.Generator(device=dev)
    g.manual_seed(7)
    boxes = []
    for nx, ny, nz in BOXES:
        ids = torch.randint(1, 4, (nz, ny, nx), device=dev, generator=g, dtype=torch.int16)
        keep = torch.rand((nz, ny, nx), device=dev, generator=g) < 0.5
        boxes.append(torch.where(keep, ids, torch.zeros_like(ids)).contiguous())
    table = {}
    for wx, wy, wz in ((1024, 128, 1024), (1024, 1024, 1024)):
        vol = generate(torch, wx, wy, wz, dev)
        torch.cuda.synchronize()
        lines.append("world %d x %d x %d (%.0f MB dense), 5 levels" % (wx, wy, wz, 2.0 * wx * wy * wz / 1e6))
        for box in boxes:
            nz, ny, nx = box.shape
            ts, ph, first = [], [], None
            for i in range(WARM + RUNS):
                t = rt.Tree.volume_gpu(5, vol, PAL)
                n0, m0, b0 = t.info().n_nodes, t.info().n_mat_bytes // 2, t.info().device_bytes
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                t.patch_volume(box, ORIGIN)
                ts.append((time.perf_counter() - t0) * 1e3)
                ph.append(t.patch_times())
                if first is None:
                    first = (t.info().n_nodes - n0, t.info().n_mat_bytes // 2 - m0, t.garbage(), t.info().device_bytes != b0)
            ts, ph = np.array(ts[WARM:]), np.array(ph[WARM:])
            x, y, z = ORIGIN
            comp = vol.clone()
            comp[z:z + nz, y:y + ny, x:x + nx] = box
            assert torch.equal(t.read_volume((0, 0, 0), vol.shape), comp), "the patched tree does not hold the composite"
            rb = []
            for i in range(WARM + RUNS):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                f = rt.Tree.volume_gpu(5, comp, PAL)
                rb.append((time.perf_counter() - t0) * 1e3)
                fn = f.info().n_nodes
                del f
            rb = np.array(rb[WARM:])
            share = float(np.median(ph[:, 2]) / np.median(ts))
            table[(wx, wy, wz, nx, ny, nz)] = float(np.median(ts))
            lines += ["  box %d x %d x %d (%.1f MB): tree of %d nodes, %d material entries; the patch appended %d nodes, %d material entries; "
                      "garbage after it %d nodes, %d material entries; the tail %s"
                      % (nx, ny, nz, 2.0 * nx * ny * nz / 1e6, n0, m0, first[0], first[1], first[2][0], first[2][1],
                         "outgrew the slack: the device arrays were reallocated" if first[3] else "fitted the slack: nothing else was touched"),
                      "    svo_tree_patch_volume_gpu        %s" % med(ts),
                      "      device passes into scratch     %s" % med(ph[:, 0]),
                      "      commit + host image            %s" % med(ph[:, 1]),
                      "      host ceiling update            %s = %.0f %% of the call" % (med(ph[:, 2]), 100 * share),
                      "    svo_build_volume_gpu, whole world %s; its tree: %d nodes" % (med(rb), fn)]
            del t, comp
        del vol
    lines.append("the same box in the two worlds (median ms):")
    for nx, ny, nz in BOXES:
        a, b = table[(1024, 128, 1024, nx, ny, nz)], table[(1024, 1024, 1024, nx, ny, nz)]
        lines.append("  box %d x %d x %d: %.3f in the 268 MB world, %.3f in the 2147 MB world (x %.2f for 8 x the world)" % (nx, ny, nz, a, b, b / a))
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write(text)
    print(text, flush=True)


if __name__ == "__main__":
    main()
