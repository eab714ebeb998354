"""Cast parity on 6- and 7-level worlds that are not heightfields (tests/deep_world.py; the rays and the conditions on them
in tests/deep_cases.py): the deep counterpart of tests/test_gpu_directed_rays.py, whose helpers it uses.

What only such worlds reach: the fourth column-ceiling level (1024-column blocks: the fourth slot of the ceiling quads, the
clamped top of the pair table) with overhangs, towers and dust over it; restarts of the LDS path at every depth of a
7-level tree, from rays that cross 1024- and 4096-wide regions in mid-air; SOLID regions of 256^3, 1024^3 and a whole root
child, and such a solid split by one voxel; skip_box over boxes up to 4096 wide from origins with 10 fraction bits, at
budgets that cross the world (3 E); and the wire formats' top bits — step counts of 16384 and more, displacements beyond
+-16383 — at their budget cap.

Every test compares with the oracle on the same inputs, every field bit-exact (test_gpu_parity.compare), no ray left
out, in the flag variants of its model battery, and ends with no ray on the progress guard.  Trees: the World-built tree
of each depth, and at 7 levels the point builder's tree of the light world (equal to the host-built tree of the same
list byte for byte), which is then patched in place."""
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import deep_cases as dc  # noqa: E402
import deep_world as dw  # noqa: E402
from test_gpu_directed_rays import (STAIR_DIRS, cast_frames, cat_refs, check_frames, frame_directions, no_guard, ref_frames, ref_rays,  # noqa: E402
                                    ref_zero_plane, stair_directions, take)
from test_gpu_edits import _pairs_of, _quads_of  # noqa: E402
from test_gpu_parity import compare  # noqa: E402
from test_gpu_volume_build import _same, _same_ceilings  # noqa: E402

pytestmark = pytest.mark.gpu

TREES = ("world6", "world7", "points7")


@pytest.fixture(scope="module")
def cuda():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


def _light_ids(pal, flags, colours):
    """the light list's palette ids in the host tree's palette, by (flags, colour)"""
    key = {(f, c): i for i, (f, c, _) in enumerate(pal)}
    uniq, inv = np.unique(colours, return_inverse=True)
    assert not flags.any()
    return np.array([key[(1, int(c))] for c in uniq], np.uint16)[inv]


@pytest.fixture(scope="module")
def trees(rt, oracle_mod, cuda):
    """{name: (levels, uploaded tree, oracle tree, ceiling model, ...)}, built once and left unchanged"""
    res = {}
    for levels in dw.LEVELS:
        w, T = dw.deep(rt, oracle_mod, levels)
        res["world%d" % levels] = SimpleNamespace(levels=levels, w=w, tree=w.build().upload(0), T=T, model=dw.ceiling_model(levels))
    xyz, flags, colours = dw.light_points(7)
    w = rt.World(7)
    w.put_blocks(xyz, flags, colours)  # the host-built twin of the same list, voxel by voxel
    host = w.build()
    pal = host.palette()
    ids = _light_ids(pal, flags, colours)
    res["points7"] = SimpleNamespace(levels=7, tree=rt.Tree.points_gpu(7, xyz, ids, pal), host=host, pal=pal, xyz=xyz, ids=ids,
                                     T=dw.oracle_tree(oracle_mod, 7, dw.light_puts(7)), model=dw.ceiling_model(7, light=True))
    return res


def test_points_tree_equals_the_host_built_tree(rt, cuda, trees):
    """Tree.points_gpu of light_points(7) against the host-built tree of the same list: nodes, materials, palette, and the
    ceiling tables in HBM"""
    s = trees["points7"]
    assert 400000 < len(s.xyz) <= 1200000 and (s.xyz[:, [0, 2]] >= 8192).mean() > 0.99
    _same(s.tree, s.host, "points7")
    s.host.upload(0)
    _same_ceilings(s.tree, s.host, "points7")
    for c, m in zip(s.tree.ceilings(), s.model):
        assert np.array_equal(c.astype(np.int64), m)


# -------------------------------------------------------------------------------------------------------- A: explicit --
def explicit_battery(rt, cuda, s, org, dirs, budgets, label):
    """explicit rays against the oracle at every budget, grouped and shuffled, in the three flag variants; the references"""
    n = len(org)
    perm = np.random.default_rng(33).permutation(n)
    gd = {False: cuda.from_numpy(dirs).cuda(), True: cuda.from_numpy(np.ascontiguousarray(dirs[perm])).cuda()}
    go = {False: cuda.from_numpy(org).cuda(), True: cuda.from_numpy(np.ascontiguousarray(org[perm])).cuda()}
    refs = {}
    for steps in budgets:
        ref = refs[steps] = ref_rays(s.T, org, dirs, steps)
        print("%s: S=%d oracle hit fraction %.3f" % (label, steps, (ref["hit"] != 0).mean()))
        for shuffled in (False, True):
            r = take(ref, perm) if shuffled else ref
            for flags in (0, rt.CAST_ITERATIVE, rt.CAST_NO_CEILINGS):
                out = s.tree.cast_rays(gd[shuffled], go[shuffled], steps=steps, flags=flags)
                compare(rt, s.tree, out, r, "%s S=%d shuffled=%d flags=%d" % (label, steps, shuffled, flags))
                no_guard(rt, s.tree, out)
    return refs


@pytest.mark.parametrize("which", TREES)
def test_explicit_tied_rays(rt, cuda, trees, which):
    """A: tied and nearly tied explicit rays from origins of every class around a centre in the cavern's air and one just
    below H, at budgets 0 .. 3 E"""
    s = trees[which]
    org, dirs = dc.battery_A(s.levels, light=which == "points7")
    dc.check_A(org, dirs)
    refs = explicit_battery(rt, cuda, s, org, dirs, dc.budgets_A(s.levels), "A " + which)
    assert 0.05 < (refs[3 * 4 ** s.levels]["hit"] != 0).mean() < 0.95


# ---------------------------------------------------------------------------------------------- B: the frame instances --
@pytest.mark.parametrize("kind", ["integral", "half", "fractional"])
@pytest.mark.parametrize("steps", [300, 3000])
def test_frame_instances_tied_rays(rt, oracle_mod, cuda, trees, kind, steps):
    """B: the tie set through the frame instances, 32 x 8 pixels of one direction per camera position"""
    s = trees["world7"]
    origins = dc.origin_lists_B(7)[kind]
    full, zero = frame_directions(rt)
    d = rt.Tree.frame_desc(origins[0], full[0], 32, 8, steps, ppx=0.0, ppy=0.0, frame_origins=origins)
    assert s.tree.wire_bytes(d) == (12 if kind == "fractional" else 8)
    launches = [(origins, dn) for dn in full + zero]
    ref = cat_refs([ref_zero_plane(oracle_mod, s.T, o, dn, 32, 8, steps) for o, dn in launches])
    check_frames(rt, cuda, s.tree, s.T, launches, 32, 8, steps, "B " + kind, ref=ref)
    print("B %s S=%d: %d rays, oracle hit fraction %.3f" % (kind, steps, len(ref["hit"]), (ref["hit"] != 0).mean()))
    assert 0.05 < (ref["hit"] != 0).mean() < 0.95


def test_narrow_fans_around_ties(rt, cuda, trees):
    """B: 64 x 32 fans of near-ties (pp = 2^-14) around a subset of the tie directions"""
    s = trees["world7"]
    L = dc.origin_lists_B(7)
    lin = np.concatenate([L["integral"][:2], L["half"][8:10]])
    seg = L["fractional"][1:4]
    full, zero = frame_directions(rt)
    launches = [(o, dn) for dn in full[::3] + zero[:2] for o in (lin, seg)]
    pp = 2.0 ** -14
    ref = check_frames(rt, cuda, s.tree, s.T, launches, 64, 32, 300, "fan", ppx=pp, ppy=pp)
    print("fans: %d rays, oracle hit fraction %.3f" % (len(ref["hit"]), (ref["hit"] != 0).mean()))


# ------------------------------------------------------------------------------ C: ceiling events at all four block sizes --
@pytest.mark.parametrize("which", TREES)
def test_device_ceiling_tables(rt, cuda, trees, which):
    """C: the tables the kernels read — ceilings, pairs, quads — equal the model at all four levels; the quads' fourth
    slot holds numbers (the 1024-column ceilings), not the 0x7FFF of a level that does not exist"""
    s = trees[which]
    E = 4 ** s.levels
    k0, pair_step = rt.ceiling_layout()
    lv, c, p = s.tree.device_ceilings()
    assert lv == 4 and k0 == 2
    full = np.concatenate([m.reshape(-1) for m in s.model]).astype(np.int16)
    assert np.array_equal(c, full)
    assert np.array_equal(p, _pairs_of(full, E, k0, lv, pair_step))
    q = s.tree.device_ceiling_quads()
    assert np.array_equal(q, _quads_of(full, E, k0, lv))
    fourth = ((q >> np.uint64(48)) & np.uint64(0xFFFF)).astype(np.uint16).view(np.int16).reshape(E >> 4, E >> 4)
    want = np.repeat(np.repeat(s.model[3], 64, 0), 64, 1)
    assert np.array_equal(fourth.astype(np.int64), want) and len(np.unique(fourth)) >= 3 and (fourth != 0x7FFF).all()


@pytest.mark.parametrize("levels", dw.LEVELS)
@pytest.mark.parametrize("w", [16, 64, 256, 1024])
@pytest.mark.parametrize("group", sorted(STAIR_DIRS))
@pytest.mark.parametrize("shift", [0.0, 0.5, 2.0 ** -3])
def test_ceiling_events_at_block_boundaries(rt, oracle_mod, cuda, trees, shift, group, w, levels):
    """C: descents over each staircase whose ceiling event ties with a block-boundary event of 16, 64, 256 and 1024
    columns (ceil_march and the in-loop ceiling boxes), from integral, half-integral and dyadic grids"""
    s = trees["world%d" % levels]
    dirs = stair_directions(rt, group)
    org = dc.stair_origins(levels, w, s.model, (-1, 0, 1) if group == "boundary" else (-2, -1, 0)) + np.float32(shift)
    S = dc.stair_budget(levels, w)
    launches = [(org[i:i + rt.MAX_FRAMES], dn) for dn in dirs for i in range(0, len(org), rt.MAX_FRAMES)]
    ref = cat_refs([ref_zero_plane(oracle_mod, s.T, o, dn, 8, 8, S) for o, dn in launches])
    check_frames(rt, cuda, s.tree, s.T, launches, 8, 8, S, "C levels %d %s w=%d shift %g" % (levels, group, w, shift), ref=ref)
    fr = (ref["hit"] != 0).mean()
    print("C levels %d %s w=%d shift=%g: %d origins x %d directions, S=%d, oracle hit fraction %.3f" % (levels, group, w, shift, len(org), len(dirs), S, fr))
    assert fr > 0.5


@pytest.mark.parametrize("which", TREES)
def test_ceiling_march_runs(rt, cuda, trees, which):
    """C: on a pose over each staircase the march crosses blocks (ceil_moves > 0) and no ray stalls"""
    s = trees[which]
    for w, (org, d, S) in dc.stair_poses(s.levels).items():
        if which == "points7" and w != 16:
            continue  # (the light world holds the 16-column staircase only)
        st = s.tree.cast_stats(org, rt.normalize(d), 96, 64, S)
        print("C %s w=%d: ceil_moves per ray %.3f, no_progress %g" % (which, w, st["ceil_moves"], st["no_progress"]))
        assert st["ceil_moves"] > 0 and st["no_progress"] == 0
    no_guard(rt, s.tree)


# --------------------------------------------------------------------------------------------------- D: overhang frames --
def overhang_frames(rt, cuda, s, org, label):
    fr = []
    for sg, dn in dc.dirs_D(rt):
        for S in (300, 3000):
            ref = check_frames(rt, cuda, s.tree, s.T, [([org], dn)], 96, 64, S, "%s %s" % (label, sg), ppx=None, ppy=None)
            fr.append((ref["hit"] != 0).mean())
        ao, hit = s.T.cast_frame_ao(org, dn, 96, 64, 300, 16, 5)
        for flags in (0, rt.CAST_NO_OCTANT):
            g = rt.decode_hits(s.tree.cast_frame(org, dn, 96, 64, 300, ao_samples=16, ao_steps=5, flags=flags))
            assert np.array_equal(g["hit"], hit != 0) and np.array_equal(g["ao"], ao), (label, sg, flags)
    no_guard(rt, s.tree)
    return fr


@pytest.mark.parametrize("cam", ["integral", "half", "fractional"])
def test_overhang_frames(rt, cuda, trees, cam):
    """D: 96 x 64 frames under the roof and beside the floating solids in all eight sign octants, S = 300 and 3000: every
    field, the AO counts and the flag variants against the oracle"""
    fr = overhang_frames(rt, cuda, trees["world7"], dc.cams_D(7)[cam], "D " + cam)
    dc.check_mixed(fr, "D " + cam)


def test_overhang_frames_points_tree(rt, cuda, trees):
    """D on the point builder's tree (the light world has no floor: hits and misses is all that is asked of the pose)"""
    fr = overhang_frames(rt, cuda, trees["points7"], dc.cams_D(7)["integral"], "D points7")
    print("D points7: oracle hit fractions per pose / budget: %s" % " ".join("%.2f" % f for f in fr))
    assert 0 < np.mean(fr) < 1 and sum(0 < f < 1 for f in fr) >= 2


def test_overhang_shading(rt, cuda, trees):
    """D: the shading pass over the mirror patch, the glass wall and the pool (the VIEW_ALL tree as the scene), with and
    without hit records"""
    from test_gpu_shade import _check

    s = trees["world7"]
    scene = s.w.build(rt.VIEW_ALL).upload(0)
    org, d = dc.shade_pose(7)
    dn = rt.normalize(d)
    sun = rt.sun_dir()
    ref = s.T.shade_frame(org, dn, 96, 64, 300, sun, liquid=True)
    prim = s.T.cast_frame(org, dn, 96, 64, 300)
    fl = prim["flags"][prim["hit"] != 0]
    water = int((ref != s.T.shade_frame(org, dn, 96, 64, 300, sun)).any(1).sum())
    print("D shade: primary hits on the mirror %d, on glass %d, pixels the water changes %d" % ((fl == (dw.F_MIRROR | 1)).sum(), (fl == (dw.F_GLASS | 1)).sum(), water))
    assert (fl == (dw.F_MIRROR | 1)).sum() > 100 and (fl == (dw.F_GLASS | 1)).sum() > 100 and water > 20
    rgba, hits = s.tree.shade_frame(org, dn, 96, 64, 300, sun=sun, with_hits=True, scene=scene)
    hit = rt.decode_hits(hits)["hit"]
    _check(rgba, ref, hit, "D shade")
    _check(s.tree.shade_frame(org, dn, 96, 64, 300, sun=sun, scene=scene), ref, hit, "D shade, no records")
    assert 0.1 < hit.mean() < 1.0
    no_guard(rt, s.tree)


# ---------------------------------------------------------------------------------------------------- E: across the world --
@pytest.mark.parametrize("levels", dw.LEVELS)
def test_across_the_world(rt, oracle_mod, cuda, trees, levels):
    """E: from far root children into the area, along the tower and through the wraps, from outside the extent, grazing
    the big solids, into and out of the split 256^3 block: explicit rays and the same rays as 8 x 8 zero-plane frames, at
    budgets 300, E + 100 and 3 E"""
    s = trees["world%d" % levels]
    rays = dc.edge_rays(rt, levels)
    org, dirs = dc.flat_rays(rays)
    budgets = dc.budgets_E(levels)
    refs = explicit_battery(rt, cuda, s, org, dirs, budgets, "E levels %d" % levels)
    dc.check_E(levels, org, refs[budgets[-1]])
    for steps in budgets:
        launches = [(os_[i:i + rt.MAX_FRAMES], d) for d, os_ in rays for i in range(0, len(os_), rt.MAX_FRAMES)]
        ref = cat_refs([ref_zero_plane(oracle_mod, s.T, o, d, 8, 8, steps) for o, d in launches])
        check_frames(rt, cuda, s.tree, s.T, launches, 8, 8, steps, "E frames levels %d" % levels, ref=ref)


# ------------------------------------------------------------------------------------------------------- F: path restarts --
def test_path_restarts(rt, cuda, trees):
    """F: a pose whose rays leave the cavern area sideways, across the top-bit boundary: the LDS path restarts below the
    root (path_starts) and at it (root_starts), and boxes of 256 and more are skipped; then the frame as in D"""
    s = trees["world7"]
    org, d = dc.pose_F(7)
    dn = rt.normalize(d)
    st = s.tree.cast_stats(org, dn, 96, 64, 3000)
    print("F: per ray path_starts %.3f root_starts %.3f skips_256plus %.3f no_progress %g" % (st["path_starts"], st["root_starts"], st["skips_256plus"], st["no_progress"]))
    assert st["path_starts"] > 0 and st["root_starts"] > 0 and st["skips_256plus"] > 0 and st["no_progress"] == 0
    for S in (300, 3000):
        ref = check_frames(rt, cuda, s.tree, s.T, [([org], dn)], 96, 64, S, "F", ppx=None, ppy=None)
        print("F S=%d: oracle hit fraction %.3f" % (S, (ref["hit"] != 0).mean()))
    ao, hit = s.T.cast_frame_ao(org, dn, 96, 64, 300, 16, 5)
    g = rt.decode_hits(s.tree.cast_frame(org, dn, 96, 64, 300, ao_samples=16, ao_steps=5))
    assert np.array_equal(g["hit"], hit != 0) and np.array_equal(g["ao"], ao)
    no_guard(rt, s.tree)


# ------------------------------------------------------------------------------------------------------ G: wire top bits --
def _bits(torch, t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def _same_records(torch, a, b, label):
    for k in ("pos_steps", "t", "info"):  # (t by its bits)
        assert torch.equal(_bits(torch, a[k]), _bits(torch, b[k])), (label, k)


def _blank(rt, torch, n):
    out = rt.Tree.alloc_hits(n, 0)
    for k in out:
        out[k].fill_(-1)
    return out


def test_wire_top_bits(rt, oracle_mod, cuda, trees):
    """G: at budget 32767, the formats' cap, rays along empty rows of the 7-level world, axis-dominant on each axis in both
    signs: cast_wire -> wire_scatter (unpack_hits for explicit rays) and pack_hits -> unpack_hits of the plain cast equal
    the plain cast bit for bit, and the plain cast equals the oracle.  Bit 14 of the compact step counts, the high part of
    n_z across the two words and int16 displacements beyond +-16383 are in use (dc.check_G, on the oracle's records)."""
    torch = cuda
    s = trees["world7"]
    tree, S = s.tree, dc.WIRE_STEPS
    seen = {a: ([], []) for a in range(3)}
    for axis, dn, kinds in dc.wire_rays(rt):
        for kind, origins in kinds.items():
            label = "G axis %d %s %s" % (axis, dn, kind)
            d, plain = cast_frames(rt, tree, origins, dn, 8, 8, S, ppx=0.0, ppy=0.0)
            wb = tree.wire_bytes(d)
            assert wb == (12 if kind == "fractional" else 8), label
            n = rt.Tree.count(d)
            ref = ref_zero_plane(oracle_mod, s.T, origins, dn, 8, 8, S)
            compare(rt, tree, plain, ref, label)
            wire = torch.zeros((n, wb), dtype=torch.uint8, device="cuda")
            tree.cast_wire(d, wire)
            back = _blank(rt, torch, n)
            tree.wire_scatter(d, wire, back)
            packed = torch.zeros((n, wb), dtype=torch.uint8, device="cuda")
            tree.pack_hits(d, plain, packed)
            back2 = _blank(rt, torch, n)
            tree.unpack_hits(d, packed, back2)
            torch.cuda.synchronize()
            assert torch.equal(packed, wire), label
            _same_records(torch, back, plain, label + " cast_wire -> wire_scatter")
            _same_records(torch, back2, plain, label + " pack_hits -> unpack_hits")
            seen[axis][0].append(np.repeat(origins, 64, 0))
            seen[axis][1].append(ref)
        # the same rays as explicit ones (12-byte records whatever the origin)
        org = np.concatenate(list(kinds.values())).astype(np.float32)
        dirs = np.tile(dn, (len(org), 1)).astype(np.float32)
        go, gd = torch.from_numpy(org).cuda(), torch.from_numpy(dirs).cuda()
        plain = tree.cast_rays(gd, go, steps=S)
        ref = ref_rays(s.T, org, dirs, S)
        compare(rt, tree, plain, ref, "G explicit axis %d" % axis)
        d = rt.CastDesc()
        d.ray_dirs, d.ray_origins, d.n_rays, d.steps = gd.data_ptr(), go.data_ptr(), len(org), S
        assert tree.wire_bytes(d) == 12
        wire = torch.zeros((len(org), 12), dtype=torch.uint8, device="cuda")
        tree.cast_wire(d, wire)
        packed = torch.zeros((len(org), 12), dtype=torch.uint8, device="cuda")
        tree.pack_hits(d, plain, packed)
        back, back2 = _blank(rt, torch, len(org)), _blank(rt, torch, len(org))
        tree.unpack_hits(d, wire, back)
        tree.unpack_hits(d, packed, back2)
        torch.cuda.synchronize()
        assert torch.equal(packed, wire)
        _same_records(torch, back, plain, "G explicit cast_wire -> unpack_hits")
        _same_records(torch, back2, plain, "G explicit pack_hits -> unpack_hits")
        seen[axis][0].append(org)
        seen[axis][1].append(ref)
    for a, (orgs, refs) in seen.items():
        dc.check_G(np.concatenate(orgs), cat_refs(refs), a)
    no_guard(rt, tree)


def test_wire_refuses_steps_above_its_cap(rt, cuda, trees):
    """G: steps = 32768 is refused with SVO_ERANGE by every wire entry point, and nothing is written"""
    torch = cuda
    tree = trees["world7"].tree
    axis, dn, kinds = dc.wire_rays(rt)[0]
    origins = kinds["integral"]
    good, plain = cast_frames(rt, tree, origins, dn, 8, 8, dc.WIRE_STEPS, ppx=0.0, ppy=0.0)
    n = rt.Tree.count(good)
    d = rt.Tree.frame_desc(origins[0], dn, 8, 8, dc.WIRE_STEPS + 1, ppx=0.0, ppy=0.0, frame_origins=origins)
    wire = torch.full((n, 12), 0xAB, dtype=torch.uint8, device="cuda")
    back = _blank(rt, torch, n)
    before = {k: v.clone() for k, v in back.items()}
    for call in (lambda: tree.cast_wire(d, wire), lambda: tree.pack_hits(d, plain, wire), lambda: tree.unpack_hits(d, wire, back),
                 lambda: tree.wire_scatter(d, wire, back)):
        with pytest.raises(rt.SvoError, match=r"\(-5\).*32767"):
            call()
    torch.cuda.synchronize()
    assert bool((wire == 0xAB).all())
    _same_records(torch, back, before, "refused calls")
    no_guard(rt, tree)


# --------------------------------------------------------------------------------------------------- H: a patched deep tree --
def test_patched_points_tree(rt, oracle_mod, cuda, trees):
    """H: one patch_points list of put-only edits at coordinates >= H on a points-built tree of the light world (one edit
    completes a brick, one lies inside the 64^3 block), the same voxels put into the oracle: the explicit battery, one
    frame, and ceilings equal to the model extended by the edits"""
    base = trees["points7"]
    g = dw.layout(7)
    tree = rt.Tree.points_gpu(7, base.xyz, base.ids, base.pal)  # (a tree of its own: the module's stay unchanged)
    T = dw.oracle_tree(oracle_mod, 7, dw.light_puts(7))
    xyz, cid = dc.patch_edits(7)
    key = {int(dw.ident(c)): (i, f, c) for i, (f, c, _) in enumerate(base.pal) if i}
    ids = np.array([key[int(c)][0] for c in cid], np.uint16)
    assert tree.patch_points(xyz, ids) is tree
    for (x, y, z), c in zip(xyz.tolist(), cid.tolist()):
        assert T.put_block(x, y, z, key[c][1] & ~1, key[c][2], 0.0, 8) == 0
    s = SimpleNamespace(levels=7, tree=tree, T=T, model=dw.ceiling_model(7, light=True, extra=xyz))
    bx, by, bz = g.brick63
    assert tree.get_block(bx + 3, by + 3, bz + 3)[1] == key[400][0] and tree.get_block(g.big64[0] + 31, g.big64[1] + 17, g.big64[2] + 40)[1] == key[1005][0]
    assert any(not np.array_equal(a, b) for a, b in zip(s.model, base.model))  # the edits raise ceilings
    for c, m in zip(tree.ceilings(), s.model):
        assert np.array_equal(c.astype(np.int64), m)
    lv, c, p = tree.device_ceilings()
    full = np.concatenate([m.reshape(-1) for m in s.model]).astype(np.int16)
    k0, pair_step = rt.ceiling_layout()
    assert lv == 4 and np.array_equal(c, full) and np.array_equal(p, _pairs_of(full, g.E, k0, lv, pair_step))
    assert np.array_equal(tree.device_ceiling_quads(), _quads_of(full, g.E, k0, lv))
    org, dirs = dc.battery_A(7, light=True)
    refs = explicit_battery(rt, cuda, s, org, dirs, (3, 300, 5000), "H")
    assert 0.05 < (refs[5000]["hit"] != 0).mean() < 0.95
    moved = (ref_rays(base.T, org, dirs, 300)["pos"] != refs[300]["pos"]).any(1).sum()
    print("H: %d of %d rays end elsewhere than before the patch (oracle, S=300)" % (moved, len(org)))
    assert moved >= 50
    fr = overhang_frames(rt, cuda, s, dc.cams_D(7)["fractional"], "H frame")
    assert 0 < np.mean(fr) < 1
