"""svo_build_points_gpu / svo_tree_get_blocks_gpu without a device: the library exports them, every argument error is
reported by its own code (with the function's name in svo_last_error) before the first HIP call — never SVO_EDEVICE,
although this machine may have no GPU — and Tree.points_gpu rejects tensors it cannot hand over with ValueError before
the library is called."""
import ctypes as C

import numpy as np
import pytest

EINVAL, EDEVICE, ESTATE, ERANGE = -1, -3, -4, -5
EMPTY = (0, 0xFFFFFFFFFFFFFFFF, 0.0)


def _desc(rt, **kw):
    """a valid desc but for `kw`; the device pointers are never dereferenced by a failing call"""
    pal = kw.pop("palette", [EMPTY, (0, 5, 0.0), (0x14, 6, 0.0)])
    arr = (rt.Block * max(1, len(pal)))(*[rt.Block(*p) for p in pal])
    d = rt.PointsDesc()
    d.levels, d.n = 3, 100
    d.xyz, d.ids = 0x1000, 0x2000
    d.palette = arr
    d._keep = arr
    d.n_palette = len(pal)
    d.view, d.device = rt.VIEW_SOLID, 0
    for k, v in kw.items():
        if k == "palette_ptr":
            d.palette = C.POINTER(rt.Block)()
        else:
            setattr(d, k, v)
    return d


def _build(rt, d, out=True):
    h = C.c_void_p()
    rc = rt.lib().svo_build_points_gpu(C.byref(d) if d is not None else None, C.byref(h) if out else None)
    assert not h.value
    return rc, (rt.lib().svo_last_error() or b"").decode()


def test_library_exports_the_points_entry_points(rt):
    L = C.CDLL(rt.LIB_PATH)
    for s in ("svo_build_points_gpu", "svo_tree_get_blocks_gpu"):
        assert hasattr(L, s), s
        assert s in rt.ABI_SYMBOLS
    assert rt.lib().svo_version() == 7  # new entry points are detected by symbol, not by version


EINVAL_CASES = {
    "null xyz": dict(xyz=None),
    "null ids": dict(ids=None),
    "null palette": dict(palette_ptr=True),
    "levels 1": dict(levels=1),
    "levels 8": dict(levels=8),
    "n negative": dict(n=-1),
    "n negative, no lists": dict(n=-5, xyz=None, ids=None),
    "unknown view": dict(view=2),
    "palette[0] flags": dict(palette=[(1, 0xFFFFFFFFFFFFFFFF, 0.0), (0, 5, 0.0)]),
    "palette[0] colour": dict(palette=[(0, 7, 0.0), (0, 5, 0.0)]),
    "palette[0] metadata": dict(palette=[(0, 0xFFFFFFFFFFFFFFFF, 1.0)]),
}


@pytest.mark.parametrize("case", sorted(EINVAL_CASES))
def test_einval(rt, case):
    rc, msg = _build(rt, _desc(rt, **EINVAL_CASES[case]))
    assert rc == EINVAL and "svo_build_points_gpu" in msg, (rc, msg)


def test_null_desc_and_null_out(rt):
    rc, msg = _build(rt, None)
    assert rc == EINVAL and "svo_build_points_gpu" in msg
    rc, msg = _build(rt, _desc(rt), out=False)
    assert rc == EINVAL and "svo_build_points_gpu" in msg


@pytest.mark.parametrize("n", [0, 65536, 1 << 20])
def test_erange_palette_size(rt, n):
    rc, msg = _build(rt, _desc(rt, n_palette=n))
    assert rc == ERANGE and "svo_build_points_gpu" in msg and "n_palette" in msg, (rc, msg)


@pytest.mark.parametrize("n", [1 << 31, (1 << 40) + 3])
def test_erange_too_many_points(rt, n):
    rc, msg = _build(rt, _desc(rt, n=n))
    assert rc == ERANGE and "svo_build_points_gpu" in msg and "2^31" in msg, (rc, msg)


@pytest.mark.parametrize("kw", [dict(n=(1 << 31) - 1, levels=7), dict(n=0, xyz=None, ids=None, levels=2)], ids=["largest", "empty"])
def test_legal_extremes_pass_the_checks(rt, kw):
    """the largest legal list and the empty one with NULL lists get past the argument checks: what comes back is the
    device's answer (device 99 does not exist, with or without a GPU; the bogus pointers are never reached)"""
    rc, msg = _build(rt, _desc(rt, device=99, **kw))
    assert rc == EDEVICE, (rc, msg)


def test_get_blocks_gpu_argument_errors(rt):
    t = rt.World(2).build()
    f = rt.lib().svo_tree_get_blocks_gpu
    p, o = C.c_void_p(0x1000), C.c_void_p(0x2000)

    def err():
        return (rt.lib().svo_last_error() or b"").decode()

    assert f(None, p, 4, o, None) == EINVAL and "svo_tree_get_blocks_gpu" in err()
    assert f(t._h, None, 4, o, None) == EINVAL and "svo_tree_get_blocks_gpu" in err()
    assert f(t._h, p, 4, None, None) == EINVAL and "svo_tree_get_blocks_gpu" in err()
    assert f(t._h, p, -1, o, None) == EINVAL and "svo_tree_get_blocks_gpu" in err()
    assert f(t._h, p, 4, o, None) == ESTATE  # a host-only tree
    assert "svo_tree_get_blocks_gpu" in err() and "not uploaded" in err()


def test_points_gpu_value_errors(rt):
    import torch

    pal = [EMPTY, (1, 5, 0.0)]
    xyz = torch.zeros((8, 3), dtype=torch.int32)
    ids = torch.zeros(8, dtype=torch.int16)
    bad = [  # (what is wrong, xyz, ids, what the message names)
        ("xyz dtype", torch.zeros((8, 3), dtype=torch.int64), ids, "xyz: dtype"),
        ("xyz float", torch.zeros((8, 3), dtype=torch.float32), ids, "xyz: dtype"),
        ("xyz rank 1", torch.zeros(24, dtype=torch.int32), ids, "xyz: shape"),
        ("xyz (3, n)", torch.zeros((3, 8), dtype=torch.int32), ids, "xyz: shape"),
        ("xyz not contiguous", torch.zeros((8, 6), dtype=torch.int32)[:, ::2], ids, "xyz: .*contiguous"),
        ("ids dtype", xyz, torch.zeros(8, dtype=torch.int32), "ids: dtype"),
        ("ids rank 2", xyz, torch.zeros((8, 1), dtype=torch.int16), "ids: shape"),
        ("ids shorter", xyz, torch.zeros(7, dtype=torch.int16), "ids: length"),
        ("ids longer", xyz, torch.zeros(9, dtype=torch.int16), "ids: length"),
        ("ids not contiguous", xyz, torch.zeros(16, dtype=torch.int16)[::2], "ids: .*contiguous"),
        ("another device", xyz, ids, "cuda:0"),  # CPU tensors are not on cuda:0
        ("numpy xyz dtype", np.zeros((8, 3), np.int64), ids, "xyz: .*int32"),
        ("numpy xyz shape", np.zeros((8, 2), np.int32), ids, "xyz: .*shape"),
        ("numpy ids dtype", xyz, np.zeros(8, np.uint32), "ids: .*uint16"),
        ("numpy ids rank", xyz, np.zeros((8, 1), np.uint16), "ids: .*shape"),
        ("numpy length", np.zeros((8, 3), np.int32), np.zeros(5, np.uint16), "ids: length"),
        ("not tensors", [[0, 0, 0]], ids, "xyz: .*tensor"),
        ("ids not a tensor", xyz, [0] * 8, "ids: .*tensor"),
    ]
    for label, p, i, names in bad:
        with pytest.raises(ValueError, match=names):
            rt.Tree.points_gpu(2, p, i, pal)
    with pytest.raises(ValueError, match="cuda:1"):
        rt.Tree.points_gpu(2, xyz, ids, pal, device=1)
