"""Mixed outcomes in one wavefront: trace()'s loop (svo_trace.h) sorts every lane, once per iteration, into a SOLID
region, a brick, a spent budget, a closed-form crossing or a voxel walk, and its back-edge folds the hit, the budget's
end and the progress guard into one lane mask.  A frame whose budget ends among its hits puts rays that hit with steps
left, rays that hit on their last step and rays whose budget ends in the air into the same 16x4 footprint, in the same
iteration.

64x32 frames on the 3-level terrain and on the cavern (tests/cavern.py), every budget S = 1 .. 96, from an integral
camera (the octant instance without segments), a half-integral one and a fractional one (the segment instance), each
with flags 0, CAST_NO_CEILINGS and CAST_ITERATIVE: every field bit-exact against the oracle's castRayFromCam
(test_gpu_parity.compare), no ray on the progress guard.  That the frames do mix the outcomes is asserted on the oracle's
own results: per camera at least 10 budgets with a footprint that holds all three classes.  One AO frame and one shaded
frame per world at a few budgets: they run the same trace()."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cavern  # noqa: E402
from test_gpu_parity import compare  # noqa: E402

pytestmark = pytest.mark.gpu

W, H = 64, 32
FW, FH = 16, 4  # a wavefront's footprint (the default 16x4)
BUDGETS = range(1, 97)
MIN_MIXED = 10
# (camera position, direction) per world: integral, half-integral, fractional
CAMS = {
    "terrain": [((4.0, 60.0, 4.0), (1.0, -0.45, 1.0)), ((30.5, 50.5, 2.5), (-0.3, -0.6, 1.0)), ((7.3, 50.9, 60.1), (0.8, -0.7, -1.0))],
    "cavern": [((330.0, 60.0, 400.0), (1.0, -0.45, 1.0)), ((330.5, 60.5, 400.5), (-0.6, -0.4, -1.0)), ((290.7, 90.2, 300.4), (1.0, -0.5, 0.8))],
}
SHARED_BUDGETS = (5, 23, 48, 96)  # the AO and shaded frames


@pytest.fixture(scope="module")
def cuda():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


@pytest.fixture(scope="module")
def worlds(rt, oracle_mod, cuda):
    """{name: (uploaded Tree, oracle Tree)}, built once and left unchanged"""
    w, T = cavern.cavern(rt, oracle_mod, False)
    return {"terrain": (rt.Tree.terrain(3, 64, 64).upload(0), oracle_mod.Tree.terrain(3, 64, 64)), "cavern": (w.build().upload(0), T)}


def mixed_footprint(ref):
    """whether some footprint of the frame holds a hit with steps left, a hit on the last step and a miss"""
    hit = (ref["hit"] != 0).reshape(H, W)
    left = ref["steps"].reshape(H, W)

    def per_fp(m):
        return m.reshape(H // FH, FH, W // FW, FW).any(axis=(1, 3))

    return bool((per_fp(hit & (left > 0)) & per_fp(hit & (left == 0)) & per_fp(~hit)).any())


@pytest.mark.parametrize("cam", range(3))
@pytest.mark.parametrize("world", ["terrain", "cavern"])
def test_budget_sweep(rt, worlds, world, cam):
    tree, T = worlds[world]
    org, d = CAMS[world][cam]
    dn = rt.normalize(d)
    mixed = 0
    for S in BUDGETS:
        ref = T.cast_frame(org, dn, W, H, S)
        assert ref["rc"] == 0
        mixed += mixed_footprint(ref)
        for flags in (0, rt.CAST_NO_CEILINGS, rt.CAST_ITERATIVE):
            out = tree.cast_frame(org, dn, W, H, S, flags=flags)
            compare(rt, tree, out, ref, "%s cam%d S=%d flags=%d" % (world, cam, S, flags))
            assert (out["pos_steps"][:, 3] >= 0).all()
    # a condition on the inputs: the sweep does put the three outcomes into one wavefront
    assert mixed >= MIN_MIXED, "%s cam%d: %d budgets with a mixed footprint" % (world, cam, mixed)
    assert tree.guard_trips() == 0


@pytest.mark.parametrize("world", ["terrain", "cavern"])
def test_ao_frames(rt, worlds, world):
    tree, T = worlds[world]
    org, d = CAMS[world][0]
    dn = rt.normalize(d)
    for S in SHARED_BUDGETS:
        ao, hit = T.cast_frame_ao(org, dn, W, H, S, 16, 5)
        out = rt.decode_hits(tree.cast_frame(org, dn, W, H, S, ao_samples=16, ao_steps=5))
        assert np.array_equal(out["hit"], hit != 0), (world, S)
        assert np.array_equal(out["ao"], ao), (world, S)
    assert tree.guard_trips() == 0


@pytest.mark.parametrize("world", ["terrain", "cavern"])
def test_shaded_frames(rt, worlds, world):
    from test_gpu_shade import _check

    tree, T = worlds[world]
    org, d = CAMS[world][2]
    dn = rt.normalize(d)
    sun = rt.sun_dir()
    for S in SHARED_BUDGETS:
        ref = T.shade_frame(org, dn, W, H, S, sun)
        rgba, hits = tree.shade_frame(org, dn, W, H, S, sun=sun, with_hits=True)
        hit = rt.decode_hits(hits)["hit"]
        _check(rgba, ref, hit, "%s shaded S=%d" % (world, S))
        _check(tree.shade_frame(org, dn, W, H, S, sun=sun), ref, hit, "%s shaded S=%d, no records" % (world, S))
    assert tree.guard_trips() == 0
