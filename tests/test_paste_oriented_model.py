"""The numpy model of the oriented paste (tests/paste_oriented_cases.py) against numpy's own operations and against a loop
written from the content rule, over all 48 orientations; CPU only.  (The library itself runs against this model in
tests/test_gpu_paste_oriented.py and against brute force in tests/test_paste_oriented_plan_host.py.)"""
import numpy as np
import pytest

import paste_oriented_cases as poc

BOX = np.arange(1, 1 + 5 * 3 * 4, dtype=np.uint16).reshape(5, 3, 4)     # [nz, ny, nx] = 5, 3, 4: three different dimensions


def test_there_are_48_orientations_24_of_them_rotations():
    assert len(set(poc.ORIENTATIONS)) == 48
    assert sum(poc.determinant(*o) == 1 for o in poc.ORIENTATIONS) == 24
    assert poc.determinant(*poc.QUARTER_Y) == 1 and poc.determinant(*poc.MIRROR_X) == -1 and poc.determinant(*poc.INVERSION) == -1


@pytest.mark.parametrize("axis,flip", poc.ORIENTATIONS)
def test_model_against_transpose_and_flip(axis, flip):
    got = poc.orient_box(BOX, axis, flip)
    want = np.transpose(BOX, [2 - axis[2 - d] for d in range(3)])
    for a in range(3):
        if flip[a]:
            want = np.flip(want, 2 - a)
    assert got.shape == poc.dst_dims((4, 3, 5), axis)[::-1]
    assert np.array_equal(got, want)


@pytest.mark.parametrize("axis,flip", poc.ORIENTATIONS)
def test_model_against_a_loop(axis, flip):
    """the content rule, voxel by voxel, with a map, both modes and a view"""
    rng = np.random.default_rng(7)
    src = rng.integers(0, 5, (9, 8, 7)).astype(np.uint16)
    dst = rng.integers(0, 5, (10, 10, 10)).astype(np.uint16)
    so, n, do = (1, 2, 3), (4, 3, 5), (2, 1, 3)
    id_map, in_view = np.array([0, 2, 2, 0, 4], np.uint16), np.array([True, True, True, True, False])
    for keep in (False, True):
        want = dst.copy()
        dn = [n[axis[a]] for a in range(3)]
        for dz in range(dn[2]):
            for dy in range(dn[1]):
                for dx in range(dn[0]):
                    d, s = (dx, dy, dz), [0, 0, 0]
                    for a in range(3):
                        s[axis[a]] = so[axis[a]] + (n[axis[a]] - 1 - d[a] if flip[a] else d[a])
                    v = int(id_map[src[s[2], s[1], s[0]]])
                    if keep and v == 0:
                        continue
                    want[do[2] + dz, do[1] + dy, do[0] + dx] = v if in_view[v] else 0
                    assert poc.orient_point(tuple(s), so, n, do, axis, flip) == (do[0] + dx, do[1] + dy, do[2] + dz)
        assert np.array_equal(poc.apply_oriented(dst, src, so, n, do, axis, flip, id_map, keep, in_view), want)


def test_the_named_quarter_turn():
    assert np.array_equal(poc.orient_box(BOX, *poc.QUARTER_Y), np.rot90(BOX, 1, axes=(0, 2)))


@pytest.mark.parametrize("axis,flip", poc.ORIENTATIONS)
def test_inverse(axis, flip):
    assert np.array_equal(poc.orient_box(poc.orient_box(BOX, axis, flip), *poc.inverse(axis, flip)), BOX)
