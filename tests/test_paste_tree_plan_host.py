"""The host half of svo_tree_patch_tree_gpu under AddressSanitizer + UndefinedBehaviorSanitizer: svo_paste_cell.h's
paste_relation (OUT / IN(id) / CUT), paste_takes and paste_voxel against brute force over the voxels, for every aligned cell
of every level of a 64^3 destination against a 64^3 and a 16^3 source built by the host builder — offsets of 0, of a
multiple of 16, of a multiple of 4 only, of 1 / 2 / 3 mixed per axis, negative ones, both modes, src == dst — and
svo_plan.cpp's paste_plan (the checks) and paste_superseded (the garbage walk) over the same host images.
A stand-alone program (tests/sanitize/paste_tree_plan_sanitize.cpp, its own main) built with g++ and run directly,
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
def test_paste_tree_plan_clean_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "paste_tree_plan_sanitize")
    srcs = [os.path.join(build.CSRC, s) for s in build.HOST_SRCS]  # svo_plan.cpp and the host files it links against
    _run(["g++", "-std=c++17"] + SAN + ["-I" + os.path.join(ROOT, "include"),
                                        os.path.join(ROOT, "tests", "sanitize", "paste_tree_plan_sanitize.cpp")] + srcs + ["-o", exe])
    out = _run([exe], env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    assert "paste tree plan sanitize ok" in out
