"""svo_tree_get_blocks_gpu against the host lookup svo_tree_get_blocks on resident trees from the other paths — a
world-built tree in each view, a terrain tree, a volume tree after an off-grid patch (superseded records, interior
records with mask 0) and the same tree compacted — over seeded positions that include negative and beyond-extent
coordinates, which wrap modulo the extent.  All comparisons are exact."""
import numpy as np
import pytest

import volume_cases as vc

pytestmark = pytest.mark.gpu

EMPTY = (0, 0xFFFFFFFFFFFFFFFF, 0.0)
PAL = [EMPTY] + [(1 | f, c, 0.0) for f, c in vc.TABLE[1:]]


@pytest.fixture(scope="module")
def cuda():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


def _positions(levels, seed, n=20000):
    """n seeded positions: most inside the extent, a quarter up to two extents outside it on either side, and the
    corners of the extent with their outer neighbours"""
    E = 4 ** levels
    rng = np.random.default_rng(seed)
    inside = rng.integers(0, E, (n - n // 4, 3))
    outside = rng.integers(-2 * E, 3 * E, (n // 4, 3))
    edge = np.array([(a, b, c) for a in (-1, 0, E - 1, E) for b in (-1, 0, E - 1, E) for c in (-1, 0, E - 1, E)])
    return np.ascontiguousarray(np.concatenate([inside, outside, edge]).astype(np.int32))


def _check(t, levels, seed, label, extra=None):
    p = _positions(levels, seed)
    if extra is not None:
        p = np.ascontiguousarray(np.concatenate([p, extra]).astype(np.int32))
    got = t.get_blocks_gpu(p).cpu().numpy().view(np.uint16)
    want = t.get_blocks(p)
    assert np.array_equal(got, want), "%s: %d of %d positions differ" % (label, int((got != want).sum()), len(p))
    E = 4 ** levels
    out = ((p < 0) | (p >= E)).any(1)
    assert (want[out] != 0).any() and (want[~out] != 0).any() and (want == 0).any(), label   # nothing vacuous
    assert np.array_equal(want[out], t.get_blocks(p[out] % E)), label                      # wrapped, as the host wraps
    return p, want


def _world(rt):
    w = rt.World(3)
    w.put_block(16, 32, 48, 0, int(vc.colour(11)), level=2)   # a 16^3 block: a K_SOLID record
    vol = vc.random_volume((64, 64, 64), 0.25, 81)
    vol[48:64, 32:48, 16:32] = 0
    z, y, x = np.nonzero(vol)
    ids = vol[z, y, x]
    flags = np.array([t[0] for t in vc.TABLE], np.uint32)
    cols = np.array([t[1] for t in vc.TABLE], np.uint64)
    w.put_blocks(np.stack([x, y, z], 1), flags[ids], cols[ids])
    return w


@pytest.mark.parametrize("view", [0, 1])
def test_world_built_tree(rt, cuda, view):
    t = _world(rt).build(view).upload(0)
    p, want = _check(t, 3, 82 + view, "world view %d" % view)
    liquid = [i for i, q in enumerate(t.palette()) if q[0] & 0x10]
    assert bool(np.isin(want, liquid).any()) == (view == 1)


def test_terrain_tree(rt, cuda):
    t = rt.Tree.terrain_gpu(4, 200, 200, 0)
    _check(t, 4, 84, "terrain")


def test_patched_volume_tree_and_its_compaction(rt, cuda):
    vol = vc.random_volume((64, 64, 64), 0.3, 85)
    vol[16:32, 16:32, 16:32] = 2                       # a K_SOLID region the patch cuts into
    vol[0:16, 0:16, 0:16] = 0                          # a 16^3 region whose only content ...
    vol[8:14, 13:16, 10:15] = 1                        # ... lies where the box will reach into it
    t = rt.Tree.volume_gpu(3, vol, PAL, view=1)
    box = vc.random_volume((21, 18, 27), 0.4, 86)
    box[0:10, 0:3, 0:7] = 0                            # and is emptied by it: a cut region left with nothing in it
    at = (9, 13, 6)                                    # off the brick grid on every axis
    t.patch_volume(box, at)
    assert t.garbage()[0] > 0 and t.garbage()[1] > 0   # superseded records and material entries stay in the arrays
    nodes = t.export()[0]
    interior = ((nodes[:, 1] >> np.uint64(32)) & np.uint64(3)) == 0
    assert ((nodes[:, 0] == 0) & interior).any()        # an interior record with mask 0
    z, y, x = np.nonzero(np.ones(box.shape, bool))
    inbox = np.stack([x + at[0], y + at[1], z + at[2]], 1)
    p, before = _check(t, 3, 87, "patched", extra=inbox)
    comp = vol.copy()
    comp[at[2]:at[2] + 21, at[1]:at[1] + 18, at[0]:at[0] + 27] = box
    q = p % 64
    assert np.array_equal(before, comp[q[:, 2], q[:, 1], q[:, 0]])
    t.compact()
    assert t.garbage() == (0, 0)
    got = t.get_blocks_gpu(p).cpu().numpy().view(np.uint16)
    assert np.array_equal(got, before) and np.array_equal(got, t.get_blocks(p))


def test_no_positions(rt, cuda):
    t = rt.Tree.volume_gpu(2, vc.random_volume((16, 16, 16), 0.3, 88), PAL)
    out = t.get_blocks_gpu(np.zeros((0, 3), np.int32))
    assert tuple(out.shape) == (0,) and out.dtype == cuda.int16
    assert rt.lib().svo_tree_get_blocks_gpu(t._h, None, 0, None, None) == 0


def test_callers_buffer_on_another_stream(rt, cuda):
    vol = vc.random_volume((16, 16, 16), 0.3, 89)
    t = rt.Tree.volume_gpu(2, vol, PAL, view=1)
    p = _positions(2, 90, 4000)
    s = cuda.cuda.Stream()
    with cuda.cuda.stream(s):
        dp = cuda.from_numpy(p).cuda()
        out = cuda.full((len(p),), -1, dtype=cuda.int16, device="cuda:0")
        back = t.get_blocks_gpu(dp, out=out, stream=s)
    s.synchronize()
    assert back is out
    q = p % 16
    assert np.array_equal(out.cpu().numpy().view(np.uint16), vol[q[:, 2], q[:, 1], q[:, 0]])
    with pytest.raises(ValueError, match="out"):
        t.get_blocks_gpu(dp, out=cuda.zeros(len(p) + 1, dtype=cuda.int16, device="cuda:0"))
    with pytest.raises(ValueError, match="out"):
        t.get_blocks_gpu(dp, out=cuda.zeros(len(p), dtype=cuda.int32, device="cuda:0"))
