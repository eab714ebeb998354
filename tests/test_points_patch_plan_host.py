"""The host half of svo_tree_patch_points_gpu under AddressSanitizer + UndefinedBehaviorSanitizer: svo_plan.cpp's
points_anchor (the key-prefix walk that finds the one record rewritten in place) and ceil_block_rects (the touched
16 x 16-column blocks merged into the rectangles whose ceilings are recomputed) on small hand-built node arrays and block
lists — one edit, two edits in one brick, two in opposite corners of the world, a path that meets a SOLID child or an
empty slot, a lone-SOLID root; blocks forming one run, two runs in a row, a full row, an unsorted list with duplicates.
A stand-alone program (tests/sanitize/points_patch_plan_sanitize.cpp, its own main) built with g++ and run directly,
nothing preloaded; CPU only."""
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
def test_points_patch_plan_clean_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "points_patch_plan_sanitize")
    srcs = [os.path.join(build.CSRC, s) for s in build.HOST_SRCS]  # svo_plan.cpp and the host files it links against
    _run(["g++", "-std=c++17"] + SAN + ["-I" + os.path.join(ROOT, "include"),
                                        os.path.join(ROOT, "tests", "sanitize", "points_patch_plan_sanitize.cpp")] + srcs + ["-o", exe])
    out = _run([exe], env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    assert "points patch plan sanitize ok" in out
