"""The host half of svo_tree_diff_gpu under AddressSanitizer + UndefinedBehaviorSanitizer: svo_diff_pair.h's pair logic (side
states, child slots, brick-depth voxel ids, the classification "both uniform"), which the kernels share, walked by a
recursive host driver over hand-built record arrays for two 2-level trees that cross seven side shapes at one slot each,
against brute force over all 16^3 voxels — the whole extent and boxes off the grid.  A stand-alone program
(tests/sanitize/diff_voxels_plan_sanitize.cpp, its own main) built with g++ and run directly, nothing preloaded; CPU only."""
import os
import shutil
import subprocess

import pytest

from raytracing_test_amd import build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAN = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-ffp-contract=off", "-pthread"]


def _run(cmd, **kw):
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=600, **kw)
    assert p.returncode == 0, (" ".join(cmd), p.stdout[-2000:], p.stderr[-4000:])
    return p.stdout


@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")
def test_diff_voxels_plan_clean_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "diff_voxels_plan_sanitize")
    srcs = [os.path.join(build.CSRC, s) for s in build.HOST_SRCS]  # svo_plan.cpp (list_box) and the host files it links against
    _run(["g++", "-std=c++17"] + SAN + ["-I" + os.path.join(ROOT, "include"),
                                        os.path.join(ROOT, "tests", "sanitize", "diff_voxels_plan_sanitize.cpp")] + srcs + ["-o", exe])
    out = _run([exe], env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    assert "diff voxels plan sanitize ok" in out
