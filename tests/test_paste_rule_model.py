"""The numpy model of svo_tree_patch_tree_rule_gpu (tests/paste_rule_cases.py) against a plain triple loop written from the
header's table, for all 12 rules; RULE_REPLACE and RULE_OVER against the oriented paste's model; rule 0 as the identity;
the package's RULE_* constants against the model's.  CPU only."""
import numpy as np
import pytest

import paste_oriented_cases as poc
import paste_rule_cases as prc

ORIENTS = [poc.IDENTITY, poc.QUARTER_Y, ((1, 2, 0), (1, 0, 1))]


def _loop(dst, src, so, dims, do, axis, flip, id_map, rule, view_keep):
    """the header's table, one voxel at a time"""
    a, b, c = prc.fields(rule)
    out = dst.copy()
    dn = [dims[axis[i]] for i in range(3)]
    for qz in range(dn[2]):
        for qy in range(dn[1]):
            for qx in range(dn[0]):
                q = (qx, qy, qz)
                p = [0, 0, 0]
                for i in range(3):
                    j = axis[i]
                    p[j] = so[j] + (dims[j] - 1 - q[i] if flip[i] else q[i])
                s = int(src[p[2], p[1], p[0]])
                if id_map is not None:
                    s = int(id_map[s])
                rs = s if view_keep[s] else 0
                d = int(dst[do[2] + qz, do[1] + qy, do[0] + qx])
                if s != 0 and d == 0:
                    r = rs if a == prc.TAKE else 0
                elif s != 0 and d != 0:
                    r = d if b == prc.KEEP else (rs if b == prc.TAKE else 0)
                elif d != 0:
                    r = d if c == prc.KEEP else 0
                else:
                    r = 0
                out[do[2] + qz, do[1] + qy, do[0] + qx] = r
    return out


@pytest.fixture(scope="module")
def volumes():
    rng = np.random.default_rng(5)
    dst = rng.integers(0, 6, (12, 12, 12)).astype(np.uint16) * (rng.random((12, 12, 12)) < 0.5)
    src = rng.integers(0, 6, (10, 10, 10)).astype(np.uint16) * (rng.random((10, 10, 10)) < 0.5)
    return dst.astype(np.uint16), src.astype(np.uint16)


def test_the_twelve_rules_and_the_named_ones():
    assert sorted(prc.RULES) == [0, 1, 4, 5, 8, 9, 32, 33, 36, 37, 40, 41] and len(set(prc.RULES)) == 12
    assert prc.NAMED == {"UNDER": prc.rule_of(prc.TAKE, prc.KEEP, prc.KEEP), "PAINT": prc.rule_of(prc.KEEP, prc.TAKE, prc.KEEP),
                         "OVER": prc.rule_of(prc.TAKE, prc.TAKE, prc.KEEP), "ERASE": prc.rule_of(prc.KEEP, prc.CLEAR, prc.KEEP),
                         "XOR": prc.rule_of(prc.TAKE, prc.CLEAR, prc.KEEP), "MASK": prc.rule_of(prc.KEEP, prc.KEEP, prc.CLEAR),
                         "STENCIL": prc.rule_of(prc.KEEP, prc.TAKE, prc.CLEAR), "REPLACE": prc.rule_of(prc.TAKE, prc.TAKE, prc.CLEAR)}
    assert set(prc.NAMED.values()) <= set(prc.RULES)


@pytest.mark.parametrize("rule", prc.RULES)
def test_the_model_equals_a_triple_loop(volumes, rule):
    dst, src = volumes
    so, dims, do = (1, 2, 3), (6, 5, 4), (2, 1, 3)
    keep_all, keep_some = np.ones(6, bool), np.array([1, 1, 0, 1, 1, 0], bool)
    for axis, flip in ORIENTS:
        for id_map in (None, [0, 2, 2, 0, 5, 1]):
            for view_keep in (keep_all, keep_some):
                got = prc.apply_rule(dst, src, so, dims, do, axis, flip, id_map, rule, view_keep)
                assert np.array_equal(got, _loop(dst, src, so, dims, do, axis, flip, id_map, rule, view_keep)), (rule, axis, flip, id_map)
                outside = np.ones(dst.shape, bool)
                dn = poc.dst_dims(dims, axis)
                outside[do[2]:do[2] + dn[2], do[1]:do[1] + dn[1], do[0]:do[0] + dn[0]] = False
                assert np.array_equal(got[outside], dst[outside])
    assert all(n > 0 for n in prc.cases_in_box(dst, src, so, dims, do, (0, 1, 2), (0, 0, 0), None))


def test_replace_and_over_are_the_oriented_paste(volumes):
    dst, src = volumes
    so, dims, do = (1, 2, 3), (6, 5, 4), (2, 1, 3)
    keep_some = np.array([1, 1, 0, 1, 1, 0], bool)
    for axis, flip in poc.ORIENTATIONS:
        for id_map in (None, [0, 2, 2, 0, 5, 1]):
            for rule, keep in ((prc.REPLACE, False), (prc.OVER, True)):
                want = poc.apply_oriented(dst, src, so, dims, do, axis, flip, id_map, keep, keep_some)
                assert np.array_equal(prc.apply_rule(dst, src, so, dims, do, axis, flip, id_map, rule, keep_some), want)


def test_rule_0_is_the_identity(volumes):
    dst, src = volumes
    for axis, flip in ORIENTS:
        got = prc.apply_rule(dst, src, (0, 0, 0), (10, 10, 10), (1, 2, 0), axis, flip, [0, 1, 1, 2, 3, 0], 0, np.array([1, 0, 1, 0, 1, 0], bool))
        assert np.array_equal(got, dst)
    assert np.array_equal(prc.apply_rule(dst, src, None, None, (0, 0, 0), (0, 1, 2), (0, 0, 0), None, 0, np.ones(6, bool)), dst)


def test_the_python_constants_are_the_model_s(rt):
    assert (rt.RULE_KEEP, rt.RULE_TAKE, rt.RULE_CLEAR) == (prc.KEEP, prc.TAKE, prc.CLEAR)
    for name, value in prc.NAMED.items():
        assert getattr(rt, "RULE_" + name) == value
    assert [rt.paste_rule(a, b, c) for c in (0, 2) for b in (0, 1, 2) for a in (0, 1)] == prc.RULES
