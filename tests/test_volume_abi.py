"""svo_build_volume_gpu / svo_tree_read_volume without a device: the library exports them, every argument error is
reported by its own code (with a message in svo_last_error) before the first HIP call — never SVO_EDEVICE, although this
machine may have no GPU — and Tree.volume_gpu rejects tensors it cannot hand over with ValueError before the library is
called."""
import ctypes as C

import numpy as np
import pytest

EINVAL, EDEVICE, ESTATE, ERANGE = -1, -3, -4, -5
EMPTY = (0, 0xFFFFFFFFFFFFFFFF, 0.0)


def _desc(rt, **kw):
    """a valid desc but for `kw`; the voxel pointer is never dereferenced by a failing call"""
    pal = kw.pop("palette", [EMPTY, (0, 5, 0.0), (0x14, 6, 0.0)])
    arr = (rt.Block * max(1, len(pal)))(*[rt.Block(*p) for p in pal])
    d = rt.VolumeDesc()
    d.levels, d.nx, d.ny, d.nz = 3, 16, 8, 12
    d.origin[:] = [4, 0, 50]
    d.voxels = 0x1000
    d.palette = arr
    d._keep = arr
    d.n_palette = len(pal)
    d.view, d.device = rt.VIEW_SOLID, 0
    for k, v in kw.items():
        if k == "origin":
            d.origin[:] = v
        elif k == "palette_ptr":
            d.palette = C.POINTER(rt.Block)()
        else:
            setattr(d, k, v)
    return d


def _build(rt, d, out=True):
    h = C.c_void_p()
    rc = rt.lib().svo_build_volume_gpu(C.byref(d) if d is not None else None, C.byref(h) if out else None)
    assert not h.value
    return rc, (rt.lib().svo_last_error() or b"").decode()


def test_library_exports_the_volume_entry_points(rt):
    L = C.CDLL(rt.LIB_PATH)
    for s in ("svo_build_volume_gpu", "svo_tree_read_volume"):
        assert hasattr(L, s), s
        assert s in rt.ABI_SYMBOLS
    assert rt.lib().svo_version() == 7  # new entry points are detected by symbol, not by version


EINVAL_CASES = {
    "null voxels": dict(voxels=None),
    "null palette": dict(palette_ptr=True),
    "levels 1": dict(levels=1),
    "levels 8": dict(levels=8),
    "nx 0": dict(nx=0),
    "ny negative": dict(ny=-3),
    "nz 0": dict(nz=0),
    "negative origin": dict(origin=[-1, 0, 0]),
    "box past +x": dict(origin=[49, 0, 0]),
    "box past +y": dict(origin=[0, 57, 0]),
    "box past +z": dict(origin=[0, 0, 53]),
    "box far past (no int32 wrap)": dict(origin=[0x7FFFFFFF, 0, 0]),
    "unknown view": dict(view=2),
    "palette[0] flags": dict(palette=[(1, 0xFFFFFFFFFFFFFFFF, 0.0), (0, 5, 0.0)]),
    "palette[0] colour": dict(palette=[(0, 7, 0.0), (0, 5, 0.0)]),
    "palette[0] metadata": dict(palette=[(0, 0xFFFFFFFFFFFFFFFF, 1.0)]),
}


@pytest.mark.parametrize("case", sorted(EINVAL_CASES))
def test_einval(rt, case):
    rc, msg = _build(rt, _desc(rt, **EINVAL_CASES[case]))
    assert rc == EINVAL and "svo_build_volume_gpu" in msg, (rc, msg)


def test_null_desc_and_null_out(rt):
    rc, msg = _build(rt, None)
    assert rc == EINVAL and msg
    rc, msg = _build(rt, _desc(rt), out=False)
    assert rc == EINVAL and msg


@pytest.mark.parametrize("n", [0, 65536, 1 << 20])
def test_erange_palette_size(rt, n):
    rc, msg = _build(rt, _desc(rt, n_palette=n))
    assert rc == ERANGE and "n_palette" in msg, (rc, msg)


def test_a_box_that_fills_the_extent_passes_the_checks(rt):
    """the largest legal box gets past the argument checks: what comes back is the device's answer (no GPU here:
    SVO_EDEVICE; with one, the bogus voxel pointer is never reached because device 99 does not exist)"""
    d = _desc(rt, origin=[0, 0, 0], nx=64, ny=64, nz=64, device=99)
    rc, msg = _build(rt, d)
    assert rc == EDEVICE, (rc, msg)


def test_read_volume_argument_errors(rt):
    t = rt.World(2).build()
    o = (C.c_int32 * 3)(0, 0, 0)
    f = rt.lib().svo_tree_read_volume
    assert f(None, o, 4, 4, 4, C.c_void_p(0x1000), None) == EINVAL
    assert f(t._h, None, 4, 4, 4, C.c_void_p(0x1000), None) == EINVAL
    assert f(t._h, o, 4, 4, 4, None, None) == EINVAL
    for n in ((0, 4, 4), (4, -1, 4), (4, 4, 0)):
        assert f(t._h, o, n[0], n[1], n[2], C.c_void_p(0x1000), None) == EINVAL
    assert f(t._h, o, 4, 4, 4, C.c_void_p(0x1000), None) == ESTATE  # not uploaded
    assert b"not uploaded" in rt.lib().svo_last_error()


def test_volume_gpu_value_errors(rt):
    import torch

    pal = [EMPTY, (1, 5, 0.0)]
    ok = torch.zeros((4, 4, 4), dtype=torch.int16)
    bad = [  # (what is wrong, the tensor, what the message names)
        ("dtype", torch.zeros((4, 4, 4), dtype=torch.int32), "dtype"),
        ("float dtype", torch.zeros((4, 4, 4), dtype=torch.float16), "dtype"),
        ("rank 2", torch.zeros((4, 4), dtype=torch.int16), "shape"),
        ("rank 4", torch.zeros((1, 4, 4, 4), dtype=torch.int16), "shape"),
        ("not contiguous", torch.zeros((4, 4, 8), dtype=torch.int16)[:, :, ::2], "contiguous"),
        ("another device", ok, "cuda:0"),  # a CPU tensor is not on cuda:0
        ("numpy dtype", np.zeros((4, 4, 4), np.int32), "uint16"),
        ("numpy rank", np.zeros((4, 4), np.uint16), "shape"),
        ("not a tensor", [[[0]]], "tensor"),
    ]
    for label, v, names in bad:
        with pytest.raises(ValueError, match=names):
            rt.Tree.volume_gpu(2, v, pal)
    with pytest.raises(ValueError, match="cuda:1"):
        rt.Tree.volume_gpu(2, ok, pal, device=1)
