"""The numpy side of the shapes patch's tests (tests/test_gpu_shapes_patch.py): the model of svo_tree_patch_shapes_gpu's
list semantics — the shapes applied in order, a voxel holding the id of the last shape that contains it, an id of 0 or one
the tree's view does not hold writing 0 — over dense volumes and over point lists, an exact lattice-point count of a
clipped ball, and the closed-form number of aligned cells a box cuts.  A shape is a tuple ("box", origin, dims, id) or
("ball", centre, r2, id), coordinates (x, y, z); volumes are indexed [z, y, x]."""
import numpy as np


def to_abi(rt, shapes):
    """the tuples as rt.Shape objects"""
    return [rt.box(s[1], s[2], s[3]) if s[0] == "box" else rt.ball(s[1], s[2], s[3]) for s in shapes]


def stored_id(shape, in_view):
    """what the shape's voxels end up holding: its id, 0 where that is an id not in view (in_view: a bool per palette id)"""
    return int(shape[3]) if in_view[shape[3]] else 0


def contains(shape, xyz):
    """a bool per row of xyz (n, 3): the shape holds the position (exact integers)"""
    p = np.asarray(xyz, np.int64).reshape(-1, 3)
    if shape[0] == "box":
        lo = np.asarray(shape[1], np.int64)
        return ((p >= lo) & (p < lo + np.asarray(shape[2], np.int64))).all(1)
    d = p - np.asarray(shape[1], np.int64)
    return (d * d).sum(1) <= int(shape[2])


def mask(shape, extent):
    """the shape's voxels inside the extent^3 volume: (slices [z, y, x] of a box of the volume that holds them all, the
    bool array of that box).  The box only bounds the work: every voxel of it is tested against the definition."""
    if shape[0] == "box":
        lo, hi = np.asarray(shape[1], np.int64), np.asarray(shape[1], np.int64) + np.asarray(shape[2], np.int64)
    else:
        r = int(np.ceil(np.sqrt(float(shape[2])))) + 1
        lo, hi = np.asarray(shape[1], np.int64) - r, np.asarray(shape[1], np.int64) + r + 1
    lo, hi = np.clip(lo, 0, extent), np.clip(hi, 0, extent)
    x, y, z = (np.arange(a, b, dtype=np.int64) for a, b in zip(lo, hi))
    where = (slice(int(lo[2]), int(hi[2])), slice(int(lo[1]), int(hi[1])), slice(int(lo[0]), int(hi[0])))
    if shape[0] == "box":
        inx, iny, inz = ((c >= o) & (c < o + n) for c, o, n in zip((x, y, z), shape[1], shape[2]))
        return where, inz[:, None, None] & iny[None, :, None] & inx[None, None, :]
    cx, cy, cz = shape[1]
    return where, ((z - cz) ** 2)[:, None, None] + ((y - cy) ** 2)[None, :, None] + ((x - cx) ** 2)[None, None, :] <= int(shape[2])


def apply_shapes(dense, shapes, in_view):
    """the composite: a copy of `dense` (the tree's stored content) with the shapes applied in order"""
    expected = np.array(dense, np.uint16)
    for s in shapes:
        where, m = mask(s, expected.shape[0])
        expected[where][m] = stored_id(s, in_view)
    return expected


def lookup(points, shapes, in_view, where):
    """the composite at the positions `where` (n, 3) over a point list instead of a volume: points = (xyz, ids) of
    distinct positions with what each stores (points_patch_cases.resolve_edits), every other voxel empty"""
    where = np.asarray(where, np.int64).reshape(-1, 3)

    def key(p):  # coordinates are below 2^14
        return (p[:, 2] << 42) | (p[:, 1] << 21) | p[:, 0]

    pk = key(np.asarray(points[0], np.int64).reshape(-1, 3))
    order = np.argsort(pk)
    pk, pid = pk[order], np.asarray(points[1], np.uint16)[order]
    assert (np.diff(pk) > 0).all(), "positions listed twice"
    out = np.zeros(len(where), np.uint16)
    inside = ((where >= 0) & (where < (1 << 14))).all(1)
    if len(pk):
        wk = key(where[inside])
        at = np.minimum(np.searchsorted(pk, wk), len(pk) - 1)
        out[inside] = np.where(pk[at] == wk, pid[at], 0)
    for s in shapes:
        out[contains(s, where)] = stored_id(s, in_view)
    return out


def _isqrt(v):
    """floor(sqrt(v)) of a non-negative int64 array: np.sqrt, put right by one either way"""
    r = np.sqrt(v.astype(np.float64)).astype(np.int64)
    r -= r * r > v
    r += (r + 1) * (r + 1) <= v
    assert ((r * r <= v) & ((r + 1) * (r + 1) > v)).all()
    return r


def ball_count(centre, r2, lo, hi):
    """the number of lattice points p with |p - centre|^2 <= r2 inside the box lo <= p < hi, exactly: per (y, z) row the
    integer half-width floor(sqrt(r2 - dy^2 - dz^2)) of the row's run, clipped to the box"""
    cx, cy, cz = (int(c) for c in centre)
    r = int(np.sqrt(float(r2))) + 2                     # (rows farther from the centre are empty: they are not visited)
    y = np.arange(max(int(lo[1]), cy - r), min(int(hi[1]), cy + r + 1), dtype=np.int64)
    z = np.arange(max(int(lo[2]), cz - r), min(int(hi[2]), cz + r + 1), dtype=np.int64)
    rem = int(r2) - ((y - cy) ** 2)[None, :] - ((z - cz) ** 2)[:, None]
    ok = rem >= 0
    w = _isqrt(np.where(ok, rem, 0))
    x0 = np.maximum(cx - w, int(lo[0]))
    x1 = np.minimum(cx + w + 1, int(hi[0]))
    return int(np.where(ok, np.maximum(x1 - x0, 0), 0).sum())


def box_cut_cells(origin, dims, cs):
    """the number of aligned cells of cs^3 voxels that the box cuts: those it meets less those wholly inside it"""
    met = inside = 1
    for o, n in zip(origin, dims):
        a, b = int(o), int(o) + int(n)
        met *= -(-b // cs) - a // cs
        inside *= max(0, b // cs - -(-a // cs))
    return met - inside
