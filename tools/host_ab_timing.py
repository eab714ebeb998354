"""Host-side A/B timing of two builds of libsvo_rt.so (no GPU): the reference world's full build in both views, 2000
single-voxel put_block + Tree.update pairs on the reference tree, Tree.terrain(6, 4096, 4096, nthreads=16) and
Tree.ceilings() of that tree.  Every repeat is a fresh process with SVO_LIB naming one library, A and B alternating;
the table gives each side's median and A's own max - min spread, the noise floor of the host it ran on.  B passes a row
when its median is no higher than A's median plus A's spread.
usage: python tools/host_ab_timing.py A.so B.so [repeats, default 9 [label_A label_B]]      (exit 1 unless every row passes)"""
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROWS = ["build_solid_ms", "build_all_ms", "edits_2000_ms", "terrain_6_4096_ms", "ceilings_ms"]


def one_run():
    sys.path.insert(0, ROOT)
    import numpy as np

    import raytracing_test_amd as rt

    def ms(fn):
        t0 = time.perf_counter()
        r = fn()
        return (time.perf_counter() - t0) * 1e3, r

    res = {}
    w = rt.World.reference()
    res["build_solid_ms"], tree = ms(lambda: w.build(rt.VIEW_SOLID))
    res["build_all_ms"], _ = ms(lambda: w.build(rt.VIEW_ALL))
    rng = np.random.default_rng(11)
    pts = np.stack([rng.integers(0, 200, 2000), rng.integers(1, 70, 2000), rng.integers(0, 200, 2000)], 1).astype(np.int32)

    def edits():
        for i in range(len(pts)):
            x, y, z = pts[i].tolist()
            w.put_block(x, y, z, 0, 77 + i % 5)
            tree.update(w, pts[i:i + 1])

    res["edits_2000_ms"], _ = ms(edits)
    res["terrain_6_4096_ms"], terrain = ms(lambda: rt.Tree.terrain(6, 4096, 4096, nthreads=16))
    res["ceilings_ms"], _ = ms(terrain.ceilings)
    res["nodes"] = [int(tree.info().n_nodes), int(terrain.info().n_nodes)]
    print(json.dumps(res))


def main():
    libs = [os.path.abspath(p) for p in sys.argv[1:3]]
    reps = int(sys.argv[3]) if len(sys.argv) > 3 else 9
    runs = [[], []]
    for _ in range(reps):
        for k in (0, 1):
            out = subprocess.run([sys.executable, os.path.abspath(__file__), "--one"], env=dict(os.environ, SVO_LIB=libs[k]),
                                 capture_output=True, text=True, check=True).stdout
            runs[k].append(json.loads(out.strip().split("\n")[-1]))
    assert all(r["nodes"] == runs[0][0]["nodes"] for side in runs for r in side), "the two libraries built different trees"
    names = sys.argv[4:6] if len(sys.argv) > 5 else sys.argv[1:3]
    print("A = %s\nB = %s\n%d alternating repeats, a fresh process each; ms" % (names[0], names[1], reps))
    print("%-20s %10s %10s %10s %10s %10s  %s" % ("", "A median", "A min", "A max", "B median", "B - A", "B <= A median + (A max - A min)"))
    ok = True
    for row in ROWS:
        a, b = [r[row] for r in runs[0]], [r[row] for r in runs[1]]
        ma, mb = statistics.median(a), statistics.median(b)
        good = mb <= ma + (max(a) - min(a))
        ok &= good
        print("%-20s %10.2f %10.2f %10.2f %10.2f %+10.2f  %s" % (row, ma, min(a), max(a), mb, mb - ma, "pass" if good else "FAIL"))
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(one_run() if "--one" in sys.argv else main())
