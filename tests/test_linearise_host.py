"""The linearised layout, pinned byte for byte (CPU): the trees svo_build_view emits and the trees svo_tree_update
leaves, with what svo_tree_get_info reports of each, hash to the digests of tests/golden/linearised_digests.json, which
tools/record_linearised_digests.py recorded with the library of the commit the fixture names (before the world -> tree
lineariser became one emitter for builds and edits).  The cases: tests/linearise_cases.py."""
import json
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import linearise_cases as lc  # noqa: E402

with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "linearised_digests.json")) as f:
    GOLDEN = json.load(f)["digests"]


def check(got, prefix):
    want = {k: v for k, v in GOLDEN.items() if k.startswith(prefix)}
    assert sorted(got) == sorted(want), "the cases differ from the recorded ones"
    wrong = [k for k in sorted(got) if got[k] != want[k]]
    assert not wrong, "%d of %d trees differ from the recorded layout, the first: %s" % (len(wrong), len(got), wrong[:4])


def test_fresh_builds_keep_the_recorded_layout(rt):
    got = dict(lc.static_cases(rt))
    assert len(got) == 12
    check(got, ("reference/", "empty/", "root_leaf", "coarse_leaves_3/", "filled_16/"))


@pytest.mark.parametrize("levels", lc.LEVELS)
def test_patched_and_rebuilt_trees_keep_the_recorded_layout(rt, oracle_mod, levels):
    got = dict(lc.script_cases(rt, oracle_mod, levels))
    assert len(got) == 2 + 4 * lc.es.N_STAGES[levels]
    check(got, "script%d/" % levels)
