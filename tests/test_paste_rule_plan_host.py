"""The host half of svo_tree_patch_tree_rule_gpu under AddressSanitizer + UndefinedBehaviorSanitizer: svo_paste_cell.h's
rule_relation (OUT / IN(id) / CUT), rule_takes and rule_voxel over a PasteRule against brute force over the voxels, for
every aligned cell of every level of a 64^3 destination and all 12 rules — the identity and two other orientations of an
off-grid box with three different dimensions out of a 16^3 and a 64^3 source built by the host builder, with and without a
map that merges two ids and drops one, with and without view bits, directed boxes, src == dst —, the rows of the cell table
that must answer OUT on directed 16^3 cells, svo_plan.cpp's paste_superseded for the record (the garbage walk) against a
count over the exported images, and paste_rule_check's statuses.
A stand-alone program (tests/sanitize/paste_rule_plan_sanitize.cpp, its own main) built with g++ and run directly, nothing
preloaded; CPU only."""
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
def test_paste_rule_plan_clean_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "paste_rule_plan_sanitize")
    srcs = [os.path.join(build.CSRC, s) for s in build.HOST_SRCS]  # svo_plan.cpp and the host files it links against
    _run(["g++", "-std=c++17"] + SAN + ["-I" + os.path.join(ROOT, "include"),
                                        os.path.join(ROOT, "tests", "sanitize", "paste_rule_plan_sanitize.cpp")] + srcs + ["-o", exe])
    out = _run([exe], env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    assert "paste rule plan sanitize ok" in out
