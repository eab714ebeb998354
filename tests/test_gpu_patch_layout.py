"""The raw layout the device-side patches leave, pinned byte for byte: the trees of tests/patch_layout_cases.py — every
patch entry point over every path of the shared descent (csrc/svo_patch_cells.h), taken before any compaction — hash to
the digests of tests/golden/patch_layout_digests.json, which tools/record_patch_layout_digests.py recorded on the GPU with
the library of the commit the fixture names (before the volume patch and the points patch became clients of that descent).
The other GPU tests compare patched trees by content or after compaction: a tail emitted in another order passes them."""
import json
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import patch_layout_cases as plc  # noqa: E402

pytestmark = pytest.mark.gpu

with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "patch_layout_digests.json")) as f:
    GOLDEN = json.load(f)["digests"]


@pytest.fixture(scope="module")
def cuda(rt):
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


@pytest.mark.parametrize("cases, prefix, count", [
    (plc.volume_cases, "volume/", 22), (plc.points_cases, "points/", 22), (plc.cell_cases, ("shapes/", "paste/"), 12),
    (plc.sequence_cases, "sequence/", 8)])
def test_patched_trees_keep_the_recorded_layout(rt, cuda, cases, prefix, count):
    got = dict(cases(rt))
    want = {k: v for k, v in GOLDEN.items() if k.startswith(prefix)}
    assert len(got) == count and sorted(got) == sorted(want), "the cases differ from the recorded ones"
    wrong = [k for k in sorted(got) if got[k] != want[k]]
    assert not wrong, "%d of %d trees differ from the recorded layout, the first: %s" % (len(wrong), len(got), wrong[:4])


def test_every_recorded_case_is_checked():
    assert len(GOLDEN) == 64 and all(k.startswith(("volume/", "points/", "shapes/", "paste/", "sequence/")) for k in GOLDEN)
