"""The host half of svo_tree_patch_volume_gpu under AddressSanitizer + UndefinedBehaviorSanitizer: svo_plan.cpp's
patch_anchor (the walk that finds the one record rewritten in place) and patch_superseded (the garbage count) on small
hand-built node arrays — a box inside one brick, inside one depth-1 child, across the world centre, a path that meets a
SOLID or an empty slot early, a lone-SOLID root, the whole extent.  A stand-alone program (tests/sanitize/
patch_plan_sanitize.cpp, its own main) built with g++ and run directly, nothing preloaded; CPU only."""
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
def test_patch_plan_clean_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "patch_plan_sanitize")
    srcs = [os.path.join(build.CSRC, s) for s in build.HOST_SRCS]  # svo_plan.cpp and the host files it links against
    _run(["g++", "-std=c++17"] + SAN + ["-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "sanitize", "patch_plan_sanitize.cpp")] +
         srcs + ["-o", exe])
    out = _run([exe], env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    assert "patch plan sanitize ok" in out
