"""The host half of the march's coarse levels.  No GPU.

The plan (svo_plan.cpp march_levels: which levels of the ceiling table a launch's march walks before its first) over every
(tree levels, table levels, first level) the ABI admits, and the offsets set_ceilings hands the kernel (march_params) over
small trees: a stand-alone program (tests/sanitize/ceil_coarse_plan_sanitize.cpp, its own main) built with g++ under
AddressSanitizer + UndefinedBehaviorSanitizer and run directly, nothing preloaded; it checks both against its own
restatement and prints the table, which is held here against a third statement of the rule.

The CPU model of the march (tools/ceil_march_model.py --levels) on a 256 x 256 heightfield: whatever the list of levels,
the march ends at the same DDA step for every ray — the levels change the trips, never the result — and so does the
event-level restatement the GPU test uses (tests/ceil_coarse_cases.py)."""
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

from raytracing_test_amd import build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import ceil_coarse_cases as cc  # noqa: E402

SAN = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-ffp-contract=off", "-pthread"]
CEIL_MAX, COARSE_MAX = 4, 2  # kCeilMax (svo_internal.h), kMarchCoarseMax (svo_plan.h)


def _run(cmd, **kw):
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=600, **kw)
    assert p.returncode == 0, (" ".join(cmd), p.stdout[-2000:], p.stderr[-4000:])
    return p.stdout


def want_plan(levels, ceil_levels, first, k0):
    """coarsest first: the table's levels above `first`, at most COARSE_MAX, whose blocks are at least 2 x 2 in the tree"""
    ls = [l for l in range(first + 1, first + COARSE_MAX + 1) if l < min(ceil_levels, CEIL_MAX) and (4 ** levels >> (2 * (k0 + l))) >= 2]
    return ls[::-1] if ceil_levels > first else []


@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")
def test_plan_and_offsets_clean_under_asan_ubsan(rt, tmp_path):
    exe = str(tmp_path / "ceil_coarse_plan_sanitize")
    srcs = [os.path.join(build.CSRC, s) for s in build.HOST_SRCS]
    _run(["g++", "-std=c++17"] + SAN + ["-I" + os.path.join(ROOT, "include"),
                                        os.path.join(ROOT, "tests", "sanitize", "ceil_coarse_plan_sanitize.cpp")] + srcs + ["-o", exe])
    out = _run([exe], env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    assert "ceil coarse plan sanitize ok" in out
    k0 = rt.ceiling_layout()[0]
    plan = {}
    for line in out.splitlines():
        if line.startswith("plan "):
            head, _, tail = line.partition(":")
            plan[tuple(int(v) for v in head.split()[1:])] = [int(v) for v in tail.split()]
    assert len(plan) == 7 * (CEIL_MAX + 1) * CEIL_MAX  # every tree depth, table size and first level
    for (levels, ceil_levels, first), got in plan.items():
        assert got == want_plan(levels, ceil_levels, first, k0), (levels, ceil_levels, first, got)
    # the trees the GPU test casts over: 5 levels march on 256-, 64-, 16- and 4-column blocks, 4 levels from 64, 3 levels from 16
    assert plan[(5, 3, 0)] == [2, 1] and plan[(4, 2, 0)] == [1] and plan[(3, 1, 0)] == [] and plan[(6, 4, 0)] == [2, 1]
    # ... and what the kernel is handed for them: the shifts, at the table's own offsets
    params = {tuple(int(v) for v in l.partition(":")[0].split()[1:]): l.partition(":")[2].split() for l in out.splitlines() if l.startswith("params ")}
    assert [p.split("@")[0] for p in params[(5, 0, 2)]] == ["8", "6"] and [p.split("@")[0] for p in params[(4, 0, 2)]] == ["6"]
    assert params[(5, 0, 0)] == [] and params[(3, 0, 1)] == [] and params[(2, 0, 1)] == []
    assert [int(p.split("@")[1]) for p in params[(5, 0, 2)]] == [64 * 64 + 16 * 16, 64 * 64]


def test_every_level_list_ends_at_the_same_dda_step(rt, oracle_mod):
    import ceil_march_model as model

    h = cc.heights(4).astype(np.int64)  # 256 x 256 columns [x][z]
    E = h.shape[0]
    mips = {cs: model.mip(h, cs) for cs in model.CELLS if cs <= E}
    cam = oracle_mod.normalize((1.0, -0.45, 1.0))
    ppx, ppy = oracle_mod.proj_plane(64, 32)
    dirs = [oracle_mod.pixel_dir(cam, ppx, ppy, 64, 32, px, py) for py in range(0, 32, 5) for px in range(0, 64, 7)]
    org = (4.0, 150.0, 4.0)
    ends, blocks = None, {}
    for sizes in ((16, 4), (16,), (64, 16, 4), (64, 16), (64, 4), (256, 64, 16, 4)):
        for top_first in (False, True):
            _, mb, end = model.run(h, mips, dirs, True, 1 << 30, sizes=sizes, top_first=top_first, org=org, steps=600)
            if sizes[-1] != 4:  # (a list that ends on 16 columns ends where the 16-column phase does)
                continue
            ends = end if ends is None else ends
            assert np.array_equal(end, ends), sizes
            blocks[(sizes, top_first)] = {s: int(b.sum()) for s, b in mb.items()}
    assert (ends > 0).sum() > len(dirs) // 2  # (-1: the ray's march outlasts the budget, under every list alike)
    # the coarse level passes blocks and takes them off the 16-column phase
    assert blocks[((64, 16, 4), False)][64] > 0 and blocks[((64, 16, 4), False)][16] < blocks[((16, 4), False)][16]
    # the event-level restatement agrees: for each ray the DDA steps up to its march's end do not depend on the levels
    t = rt.Tree.heightfield(4, h.astype(np.int32))
    tabs = cc.tables(t)
    for d in dirs[::3]:
        got = {ws: cc.march(org, d, 600, tabs, E, list(ws), pre_top=int(h.max())) for ws in ((16, 4), (64, 16, 4))}
        assert got[(16, 4)]["dda"] == got[(64, 16, 4)]["dda"] and got[(16, 4)]["stop"] == got[(64, 16, 4)]["stop"]
