"""The cavern fixture (tests/cavern.py) itself, on the CPU: the product's linearised tree holds the blocks the oracle's
tree holds, and its column ceilings (svo_tree_ceilings: what the casts' ceiling boxes and ceil_march rely on) are the
highest stored rows of a world where ceilings are not the whole story (overhangs, dust, a tower to the top row)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cavern  # noqa: E402

EMPTY = np.uint64(0xFFFFFFFFFFFFFFFF)


@pytest.fixture(scope="module", params=[False, True], ids=["low", "tall"])
def pair(request, rt, oracle_mod):
    w, T = cavern.cavern(rt, oracle_mod, request.param)
    return request.param, w.build(), T


def test_block_parity(rt, pair):
    """20,000 seeded voxels in and around every structure: the tree's palette entry (flags, colour) is the oracle's
    getBlock; empty on one side is empty on the other"""
    tall, tree, T = pair
    pts = cavern.probe_points(20000)
    ids = tree.get_blocks(pts)
    pal = tree.palette()
    pf = np.array([p[0] for p in pal], np.uint32)
    pc = np.array([p[1] for p in pal], np.uint64)
    ref = [T.get_block(int(x), int(y), int(z)) for x, y, z in pts]
    rf = np.array([r[0] for r in ref], np.uint32)
    rc = np.array([r[1] for r in ref], np.uint64)
    assert np.array_equal(ids == 0, rc == EMPTY)
    assert np.array_equal(pc[ids], rc) and np.array_equal(pf[ids], rf)
    stored = rc != EMPTY
    assert 0.2 < stored.mean() < 0.8  # the probe sees both
    kinds = set(cavern.ident(rc[stored]).tolist())
    for colour in (100, 200, 300, 400, 500, 600, 700, 800) + ((900, 950) if tall else ()):
        assert colour in kinds, colour  # floor, stairs, 64^3 block, arch, roof, mirror, glass, far voxels (tower, corners)
    assert sum(1000 <= k < 1037 for k in kinds) > 20  # dust
    assert (int(cavern.F_MIRROR) | 1) in set(rf[rc == cavern.colour(600)].tolist()) and (int(cavern.F_GLASS) | 1) in set(rf[rc == cavern.colour(700)].tolist())


def test_ceilings(rt, pair):
    """every level of tree.ceilings() against the highest stored row per aligned block, from the oracle's getBlock over
    the occupied columns (orc_dump_box in slabs); every block outside them must be -1"""
    tall, tree, T = pair
    top = np.full((cavern.E, cavern.E), -1, np.int64)  # [z][x]
    for x0, z0, nx, nz, ny in cavern.occupied_boxes(tall):
        for y0 in range(0, ny, 64):
            rc, _, c = T.dump_box(x0, y0, z0, nx, 64, nz)  # c: [z][y][x]
            assert rc == 0
            stored = c != EMPTY
            rows = np.where(stored, np.arange(y0, y0 + 64)[None, :, None], -1).max(axis=1)
            top[z0:z0 + nz, x0:x0 + nx] = np.maximum(top[z0:z0 + nz, x0:x0 + nx], rows)
    assert (top >= 0).sum() > 60000  # the floor's columns at least
    assert tall or cavern.ROOF_Y < top.max() <= cavern.DUST_TOP  # the low world's highest stored row stays low
    cs = tree.ceilings()
    assert len(cs) == cavern.LEVELS - tree.ceil_k0
    for j, c in enumerate(cs):
        B = 4 ** (tree.ceil_k0 + j)
        n = cavern.E // B
        want = top.reshape(n, B, n, B).max(axis=(1, 3))
        assert c.shape == want.shape and np.array_equal(c.astype(np.int64), want), j
        assert c.min() == -1 and c.max() == (cavern.E - 1 if tall else top.max()), j
        assert (c == -1).mean() > 0.5, j  # most blocks of the world hold nothing
    # overhangs: columns whose ceiling is far above the floor with empty space below it
    x, y, z = cavern.BIG
    assert top[z + 5, x + 5] >= y + 63 and T.get_block(x + 5, y - 1, z + 5)[1] == int(EMPTY)
