"""Time of a tree build from a dense voxel volume in HBM (svo_build_volume_gpu), against the only route to arbitrary
content without it: World.put_blocks over every voxel + build + upload on the host.
  GPU route   a generated 1024 x 128 x 1024 volume (5 levels) and a generated 1024 x 1024 x 1024 volume (5 levels):
              svo_build_volume_gpu end to end (host clock around the call, which ends synchronised: its host image is
              copied back), and its level-1 classification pass alone by HIP events (svo_volume_classify_pass) — the
              pass that reads the whole volume; bytes read (2 per voxel) over its time, and that as a fraction of the
              HBM bandwidth measured on the MI355X by a float4 copy (6.29 TB/s; 8.0 TB/s is the specification).
              3 warm-ups, then the median of 10 runs.
  host route  the smaller volume: numpy indices of its non-zero voxels, World.put_blocks, build, upload (one run).
Writes profiles/volume_build.txt (or the path given) with the library's svo_build_id().
usage: python tools/volume_build_timing.py [out.txt] [--no-host]"""
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_MEASURED_TBS, HBM_SPEC_TBS = 6.29, 8.0
EMPTY = (0, 0xFFFFFFFFFFFFFFFF, 0.0)
PAL = [EMPTY, (1, 0x111, 0.0), (1, 0x222, 0.0), (1, 0x333, 0.0)]


def generate(torch, nx, ny, nz, dev):
    """ground (material 1) below row ny / 4, a band of mixed bricks (three materials and holes, from two aperiodic 1-D
    patterns) four rows thick at every 64th row above it, empty space elsewhere; built in z-slabs"""
    x, y, z = (torch.arange(n, device=dev, dtype=torch.int64) for n in (nx, ny, nz))
    px = ((x * 7) // 13 + x // 97).to(torch.int16)
    pz = ((z * 5) // 11 + z // 61).to(torch.int16)
    py = torch.where(y < ny // 4, 1, torch.where(y % 64 < 4, 2, 0)).to(torch.int16)[None, :, None]
    vol = torch.empty((nz, ny, nx), dtype=torch.int16, device=dev)
    for z0 in range(0, nz, 128):
        m = (px[None, None, :] + pz[z0:z0 + 128, None, None]) % 4
        vol[z0:z0 + 128] = torch.where(py == 1, torch.ones_like(m), torch.where(py == 2, m, torch.zeros_like(m)))
    return vol


def main():
    import torch

    import raytracing_test_amd as rt

    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    out_path = args[0] if args else os.path.join(ROOT, "profiles", "volume_build.txt")
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    dev = torch.device("cuda", 0)
    lines = ["svo_build_id %s" % rt.build_id(), "device %s" % torch.cuda.get_device_name(0),
             "GPU route: 3 warm-ups, median of 10 (min .. max); HBM reference %.2f TB/s measured (float4 copy), %.1f TB/s specification"
             % (HBM_MEASURED_TBS, HBM_SPEC_TBS)]
    small = None
    for nx, ny, nz in ((1024, 128, 1024), (1024, 1024, 1024)):
        vol = generate(torch, nx, ny, nz, dev)
        torch.cuda.synchronize()
        ts = []
        for i in range(13):
            t0 = time.perf_counter()
            t = rt.Tree.volume_gpu(5, vol, PAL)
            ts.append(time.perf_counter() - t0)
            info = t.info()
            del t
        ts = np.array(ts[3:]) * 1e3
        d, keep = rt.Tree.volume_desc(5, vol, PAL)
        ms = (C.c_float * 13)()
        rt._check(rt.lib().svo_volume_classify_pass(C.byref(d), 13, ms), "svo_volume_classify_pass")
        cs = np.array(list(ms)[3:])
        nbytes = 2.0 * nx * ny * nz
        tbs = nbytes / (float(np.median(cs)) * 1e-3) / 1e12
        lines += ["volume %d x %d x %d (%.0f MB): nodes %d (per level %s), bricks %d, material entries %d"
                  % (nx, ny, nz, nbytes / 1e6, info.n_nodes, list(info.nodes_per_level)[:6], info.n_bricks, info.n_mat_bytes // 2),
                  "  svo_build_volume_gpu end to end  %.3f ms (%.3f .. %.3f)" % (np.median(ts), ts.min(), ts.max()),
                  "  level-1 classification pass      %.4f ms (%.4f .. %.4f): %.0f bytes read, %.3f TB/s = %.0f %% of measured HBM, %.0f %% of specification"
                  % (np.median(cs), cs.min(), cs.max(), nbytes, tbs, 100 * tbs / HBM_MEASURED_TBS, 100 * tbs / HBM_SPEC_TBS)]
        if small is None:
            small = vol.cpu().numpy()
        del vol, keep
    if "--no-host" not in sys.argv:
        t0 = time.perf_counter()
        z, y, x = np.nonzero(small)
        ids = small[z, y, x]
        w = rt.World(5)
        w.put_blocks(np.stack([x, y, z], 1), np.zeros(len(ids), np.uint32), np.array([p[1] for p in PAL], np.uint64)[ids])
        t1 = time.perf_counter()
        h = w.build()
        t2 = time.perf_counter()
        h.upload(0)
        torch.cuda.synchronize()
        t3 = time.perf_counter()
        lines += ["host route, 1024 x 128 x 1024 (%d stored voxels), one run: put_blocks %.1f ms + build %.1f ms + upload %.1f ms = %.1f ms; nodes %d"
                  % (len(ids), (t1 - t0) * 1e3, (t2 - t1) * 1e3, (t3 - t2) * 1e3, (t3 - t0) * 1e3, h.info().n_nodes)]
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write(text)
    print(text, flush=True)


if __name__ == "__main__":
    main()
