"""The fine column ceilings' host code under AddressSanitizer + UndefinedBehaviorSanitizer (+ LeakSanitizer): a
stand-alone program (tests/sanitize/ceil_fine_sanitize.cpp, its own main) compiled with every host file of the library —
the table's build and rectangle updates on small trees, the spans the sync copies, the launch's choice.  CPU only."""
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
def test_fine_ceilings_clean_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "ceil_fine_sanitize")
    srcs = [os.path.join(build.CSRC, s) for s in build.HOST_SRCS]
    _run(["g++", "-std=c++17"] + SAN + ["-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "sanitize", "ceil_fine_sanitize.cpp")] +
         srcs + ["-o", exe])
    out = _run([exe], env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    assert "ceil fine sanitize ok" in out
