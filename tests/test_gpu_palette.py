"""Large palettes on the GPU (tests/palette_cases.py): material ids up to 65534 through the casts, AO, the shading pass, the
wire formats, svo_tree_sync, the volume builder and the volume patch.  Every other GPU test uses ids up to 22; a defect that
shows only from some id upward — an id shifted into the axis bits or the hit bit of a hit record's info, a sign-extended
16-bit id, a palette read at a masked index, a bit table read past its first word, the builders' MIXED marker 0xFFFF next
to the top id 0xFFFE — would pass them all.

  A  the hall with its ids shifted onto 31 / 32, 0x7FFF / 0x8000 and up to 65534: primary casts, AO and the shading pass
     against the oracle (which stores blocks per voxel and has no palette: the reference for any id);
  B  the wire formats at palette size 4096 (accepted, id 4095 in the 12-bit field) and 4097 (SVO_ERANGE, nothing written);
  C  svo_tree_update + svo_tree_sync after the palette grew across 4096 and across 0x8000;
  D  svo_build_volume_gpu with a 65535-entry palette (and a 65-entry one: a bit table with a partial last word) against
     the host-built twin byte for byte, read back, and cast against the oracle;
  E  svo_tree_patch_volume_gpu over such trees, by the checks (a)-(f) of tests/test_gpu_volume_patch.py.

Every comparison is exact in every field; the shading pass's sky pixels keep test_gpu_shade.SKY_ATOL through the existing
_check.  Each test prints the lowest and highest hit material id and which special ids were hit, and asserts from the
reference side that ids on both sides of its boundary occur."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hall  # noqa: E402
import palette_cases as pc  # noqa: E402
import volume_cases as vc  # noqa: E402
import wire_ref  # noqa: E402
import test_gpu_directed_shading as tds  # noqa: E402
import test_gpu_volume_patch as tvp  # noqa: E402
from test_gpu_degenerate_trees import CAMS  # noqa: E402
from test_gpu_parity import compare  # noqa: E402
from test_gpu_volume_build import _same  # noqa: E402

pytestmark = pytest.mark.gpu

TIME = tds.TIME
SENTINEL = 0x5A
POSES = {p[0]: p for p in hall.FRAME_POSES}
# a pose of this file: the 4^3 glass block at the wrap, the last material put (id K + M), from a fractional origin
POSES["wrap_glass"] = ("wrap_glass", (1006.3, 57.7, 598.6), (1.0, 0.05, 0.02), None)
PALW = pc.stored_palette(pc.WIDE_TABLE)
# (ids at or below, ids at or above) that the oracle must see for a shift: both sides of its boundary; the cap's is the top id
BOUNDARY = {"word": (31, 32), "sign": (0x7FFF, 0x8000), "cap": (pc.CAP - 1, pc.CAP)}


@pytest.fixture(scope="module")
def cuda():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


@pytest.fixture(scope="module")
def base(rt, oracle_mod, cuda):
    """(M, oracle Tree) of the unshifted hall: shared by every shift and left unchanged"""
    w, T = hall.hall(rt, oracle_mod)
    return pc.scene_materials(w), T


@pytest.fixture(scope="module")
def frames(oracle_mod):
    """{pose name: (pose, origins, dirs, cam, ppx, ppy)} of the 96 x 64 frames"""
    return {n: (p,) + hall.frame_rays(oracle_mod, p) for n, p in POSES.items() if n in ("room_fractional", "pool_wide", "wrap_glass")}


@pytest.fixture(scope="module")
def shifted(rt, oracle_mod, base):
    """shift name -> (K, solid Tree, VIEW_ALL Tree, their decoded palettes): built and uploaded once per shift"""
    M, T = base
    cache = {}

    def get(name):
        if name not in cache:
            K = pc.SHIFTS(M)[name]
            w, _ = hall.hall(rt, oracle_mod, preload=K, T=T)
            solid, scene = w.build().upload(0), w.build(rt.VIEW_ALL).upload(0)
            assert solid.info().n_materials == 1 + K + M
            cache[name] = (K, solid, scene, pc.decoded(solid), pc.decoded(scene))
        return cache[name]

    return get


@pytest.fixture(scope="module")
def oracle_refs(rt, base, frames):
    """the oracle's results, computed once and shared by the shifts (its tree is the same for each): primary frames, AO
    frames, shaded batteries and shaded frames, by key"""
    _, T = base
    cache = {}

    def get(kind, name, S=300, liquid=True):
        key = (kind, name, S, liquid)
        if key not in cache:
            sun = rt.sun_dir()
            if kind == "battery":
                org, dirs = hall.batteries()[name]
                cache[key] = T.shade_rays(org, dirs, S, sun, liquid=liquid, time=TIME if liquid else 0.0)
            else:
                pose, org, dirs, cam, ppx, ppy = frames[name]
                if kind == "primary":
                    cache[key] = T.cast_frame(pose[1], cam, hall.FRAME_W, hall.FRAME_H, S, ppx, ppy)
                    assert cache[key]["rc"] == 0
                elif kind == "ao":
                    cache[key] = T.cast_frame_ao(pose[1], cam, hall.FRAME_W, hall.FRAME_H, S, 16, 5, ppx, ppy)
                else:
                    cache[key] = T.shade_rays(org, dirs, S, sun, liquid=liquid, time=TIME if liquid else 0.0)
        return cache[key]

    return get


def ref_ids(ref, palette):
    """the ids the reference's hits must carry: its (flags, colour) looked up in the tree's palette"""
    pf, pcol = palette
    key = {(int(f), int(c)): i for i, (f, c) in enumerate(zip(pf.tolist(), pcol.tolist()))}
    hit = ref["hit"] != 0
    return np.array([key[(int(f), int(c))] for f, c in zip(ref["flags"][hit], ref["color"][hit])], np.int64)


def report(label, ids, pf):
    """print the span of hit ids and the special ones among them; returns (min, max)"""
    ids = np.asarray(ids, np.int64)
    if len(ids) == 0:
        print("%s: no hits" % label)
        return None, None
    f = pf[ids]
    print("%s: hit ids %d .. %d (%d distinct); mirror %s glass %s liquid %s" % (
        label, ids.min(), ids.max(), len(np.unique(ids)), sorted(set(ids[(f & 7) == 3].tolist())),
        sorted(set(ids[((f & 7) == 5) & ((f & 0x10) == 0)].tolist())), sorted(set(ids[(f & 0x10) != 0].tolist()))))
    return int(ids.min()), int(ids.max())


def info_of(out):
    return out["info"].cpu().numpy().view(np.uint32)


def check_info(out, lo, hi, label, bits=True):
    """the hit records' info words: material within [lo, hi] on hits, bits 19..30 zero everywhere (bits: primary casts);
    returns the hit ids"""
    info = info_of(out)
    assert not bits or ((info >> 19) & 0xFFF == 0).all(), label
    hit = (info >> 31) != 0
    ids = (info & 0xFFFF)[hit].astype(np.int64)
    assert len(ids) == 0 or (ids.min() >= lo and ids.max() <= hi), (label, ids.min(), ids.max())
    return ids


# ------------------------------------------------------------------------------------------------- A: the shifted hall --
A_SHIFTS = ("word", "sign", "cap")


@pytest.mark.parametrize("shift", A_SHIFTS)
def test_shifted_hall_primary_casts(rt, cuda, base, frames, shifted, oracle_refs, shift):
    M, T = base
    K, solid, scene, pal, _ = shifted(shift)
    solid.guard_trips(reset=True)
    seen = []
    for name in ("room_fractional", "pool_wide", "wrap_glass"):
        pose, _, _, cam, ppx, ppy = frames[name]
        ref = oracle_refs("primary", name)
        want = ref_ids(ref, pal)
        seen.append(want)
        for flags in (0, rt.CAST_ITERATIVE, rt.CAST_NO_OCTANT, rt.CAST_WIDE_ADDR):
            out = solid.cast_frame(pose[1], cam, hall.FRAME_W, hall.FRAME_H, 300, ppx=ppx, ppy=ppy, flags=flags)
            label = "A %s K=%d %s flags=%d" % (shift, K, name, flags)
            compare(rt, solid, out, ref, label, palette=pal)
            ids = check_info(out, K + 1, K + M, label)
            assert np.array_equal(ids, want), label
        report("A %s K=%d %s" % (shift, K, name), want, pal[0])
    seen = np.concatenate(seen)
    lo, hi = BOUNDARY[shift]
    assert (seen <= lo).any() and (seen >= hi).any(), (shift, seen.min(), seen.max())  # by the oracle: both sides occur
    if shift == "cap":
        assert seen.max() == pc.CAP
    # the pick ray onto a mirror voxel of the pool's bed (the water above it is not in the solid view)
    o, d = (630.5, 50.5, 630.5), (0.001, -1.0, 0.002)
    r = T.cast_ray(np.array(o, np.float32), np.array(d, np.float32), 30)
    assert r.hit == 1 and r.flags == 3 and r.color == int(hall.colour(hall.C_POOL_MIRROR))
    (pos, last, left), block = solid.cast_ray_from_cam(o, d, 30)
    assert pos == tuple(r.pos) and last == tuple(r.last) and left == r.steps
    assert block[:2] == (3, int(hall.colour(hall.C_POOL_MIRROR)))
    assert solid.guard_trips() == 0


@pytest.mark.parametrize("shift", A_SHIFTS)
def test_shifted_hall_ao(rt, cuda, frames, shifted, oracle_refs, shift):
    K, solid, _, pal, _ = shifted(shift)
    solid.guard_trips(reset=True)
    occluded = 0
    for name in ("room_fractional", "pool_wide"):
        pose, _, _, cam, ppx, ppy = frames[name]
        ao, hit = oracle_refs("ao", name)
        out = rt.decode_hits(solid.cast_frame(pose[1], cam, hall.FRAME_W, hall.FRAME_H, 300, ppx=ppx, ppy=ppy, ao_samples=16, ao_steps=5))
        assert np.array_equal(out["hit"], hit != 0), (shift, name)
        assert np.array_equal(out["ao"], ao), (shift, name)
        occluded += int(ao.sum())
        report("A %s K=%d AO %s" % (shift, K, name), out["material"][out["hit"]], pal[0])
    assert occluded > 0  # by the oracle (the pane the room pose looks at is flat: the pool's frame carries the counts)
    assert solid.guard_trips() == 0


@pytest.mark.parametrize("shift", A_SHIFTS)
def test_shifted_hall_shading(rt, cuda, base, frames, shifted, oracle_refs, shift):
    torch = cuda
    M, _ = base
    K, solid, scene, pal_solid, pal_scene = shifted(shift)
    solid.guard_trips(reset=True)
    scene.guard_trips(reset=True)
    total = {}
    seen = []
    for name in ("mirrors", "glass", "water"):
        org, dirs = hall.batteries()[name]
        n = len(org)
        go, gd = torch.from_numpy(org).cuda(), torch.from_numpy(dirs).cuda()
        for S in (3, 300):
            wet, dry = oracle_refs("battery", name, S, True), oracle_refs("battery", name, S, False)
            if S == 300:
                for k, v in hall.event_counts(wet).items():
                    total[k] = total.get(k, 0) + v
                seen.append(ref_ids(wet, pal_scene))
            for flags in (0, rt.CAST_WIDE_ADDR):
                label = "A %s K=%d %s S=%d flags=%d" % (shift, K, name, S, flags)
                rgba, out = tds.shade_desc(rt, torch, solid, tds.explicit_desc(rt, go, gd, S, flags), n, True, scene=scene, time=TIME)
                tds.check(rt, scene, rgba, out, wet, label, palette=pal_scene)
                check_info(out, K + 1, K + M, label, bits=False)
                rgba, out = tds.shade_desc(rt, torch, solid, tds.explicit_desc(rt, go, gd, S, flags), n, True)
                tds.check(rt, solid, rgba, out, dry, label + " dry", palette=pal_solid)
                check_info(out, K + 1, K + M, label + " dry", bits=False)
    for name in ("room_fractional", "pool_wide"):
        f = frames[name]
        n = len(f[1])
        wet, dry = oracle_refs("shaded", name, 300, True), oracle_refs("shaded", name, 300, False)
        for k, v in hall.event_counts(wet).items():
            total[k] = total.get(k, 0) + v
        seen.append(ref_ids(wet, pal_scene))
        for flags in (0, rt.CAST_WIDE_ADDR):
            label = "A %s K=%d frame %s flags=%d" % (shift, K, name, flags)
            d = tds.frame_desc(rt, f, 300, flags)
            rgba, out = tds.shade_desc(rt, torch, solid, d, n, True, scene=scene, time=TIME)
            tds.check(rt, scene, rgba, out, wet, label, palette=pal_scene)
            rgba, out = tds.shade_desc(rt, torch, solid, d, n, True)
            tds.check(rt, solid, rgba, out, dry, label + " dry", palette=pal_solid)
    # by the oracle alone: what was cast reflects, bends (in glass and in liquid) and tints
    print("A %s events: %s" % (shift, " ".join("%s=%d" % kv for kv in total.items())))
    assert total["refl1"] > 0 and total["refl3+"] > 0 and total["bent"] > 0 and total["liq_bend"] > 0 and total["tints8+"] > 0
    seen = np.concatenate(seen)
    report("A %s K=%d shaded end blocks" % (shift, K), seen, pal_scene[0])
    lo, hi = BOUNDARY[shift]  # (no ray of these sets ends on the last material, the glass at the wrap: the primary casts hit it)
    assert (seen <= lo).any() and (seen >= (hi if shift != "cap" else 0x8000)).any()
    tds.no_guard(solid, scene)


# ---------------------------------------------------------------------------------------------------- B: wire formats --
WIRE_CAMS = [((1006.0, 57.0, 598.0), 8), ((1006.3, 57.7, 598.6), 12)]  # integral: the compact records; fractional: the general ones
WIRE_DIR = (1.0, 0.05, 0.02)
WW, WH = 64, 32


def _filled(rt, torch, n, ao=False):
    out = rt.Tree.alloc_hits(n, 0, ao=ao)
    for k in out:
        out[k].view(torch.uint8).fill_(SENTINEL)
    return out


def _untouched(torch, out):
    return all(bool((v.view(torch.uint8) == SENTINEL).all()) for v in out.values())


def test_wire_formats_at_4096_materials(rt, cuda, oracle_mod, base, shifted):
    torch = cuda
    M, T = base
    K, solid, _, pal, _ = shifted("wire_last")
    assert solid.info().n_materials == 4096
    solid.guard_trips(reset=True)
    cam = rt.normalize(WIRE_DIR)
    for org, wb in WIRE_CAMS:
        d = rt.Tree.frame_desc(org, cam, WW, WH, 300)
        n = rt.Tree.count(d)
        assert solid.wire_bytes(d) == wb, org
        ref = T.cast_frame(org, cam, WW, WH, 300)
        want = ref_ids(ref, pal)
        lo, hi = report("B K=%d wire %d B" % (K, wb), want, pal[0])
        assert hi == 4095 and (want == 4095).sum() > 50  # by the oracle: the frame hits the last material
        out = rt.Tree.alloc_hits(n, 0)
        solid.cast(d, out)
        torch.cuda.synchronize()
        compare(rt, solid, out, ref, "B cast %d B" % wb, palette=pal)
        assert np.array_equal(check_info(out, K + 1, K + M, "B"), want)
        fused = torch.zeros((n, wb), dtype=torch.uint8, device="cuda")
        solid.cast_wire(d, fused)
        back = _filled(rt, torch, n)
        solid.wire_scatter(d, fused, back)
        wire = torch.zeros((n, wb), dtype=torch.uint8, device="cuda")
        solid.pack_hits(d, out, wire)
        unpacked = _filled(rt, torch, n)
        solid.unpack_hits(d, wire, unpacked)
        torch.cuda.synchronize()
        for k in ("pos_steps", "t", "info"):
            assert torch.equal(back[k].view(torch.int32), out[k].view(torch.int32)), (wb, k, "cast_wire + wire_scatter")
            assert torch.equal(unpacked[k].view(torch.int32), out[k].view(torch.int32)), (wb, k, "hits_unpack")
        assert torch.equal(fused, wire)
        ps, t, info = out["pos_steps"].cpu().numpy(), out["t"].cpu().numpy(), info_of(out)
        cells = np.tile(np.trunc(np.array(org, np.float32)).astype(np.int32), (n, 1))
        if wb == 12:
            assert np.array_equal(wire.cpu().numpy(), wire_ref.pack(ps, t, info, cells))
        else:
            assert np.array_equal(wire.cpu().numpy(), wire_ref.pack_compact(ps, info, cells))
    assert solid.guard_trips() == 0


def test_wire_formats_refuse_4097_materials(rt, cuda, oracle_mod, base, shifted):
    torch = cuda
    M, T = base
    K, solid, _, pal, _ = shifted("wire_over")
    assert solid.info().n_materials == 4097
    cam = rt.normalize(WIRE_DIR)
    err = r"\(-5\).*4096 materials"
    x = rt.Exchange(1, 0, rt.Exchange.unique_id(), 0)
    for org, _ in WIRE_CAMS:
        d = rt.Tree.frame_desc(org, cam, WW, WH, 300)
        n = rt.Tree.count(d)
        assert solid.wire_bytes(d) == 12, org
        ref = T.cast_frame(org, cam, WW, WH, 300)
        out = solid.cast_frame(org, cam, WW, WH, 300)
        compare(rt, solid, out, ref, "B 4097 cast", palette=pal)
        want = ref_ids(ref, pal)
        report("B K=%d 4097 materials" % K, want, pal[0])
        assert want.max() == 4096 and np.array_equal(check_info(out, K + 1, K + M, "B 4097"), want)
        wire = torch.full((n, 12), SENTINEL, dtype=torch.uint8, device="cuda")
        back = _filled(rt, torch, n)
        with pytest.raises(rt.SvoError, match=err):
            solid.pack_hits(d, out, wire)
        with pytest.raises(rt.SvoError, match=err):
            solid.unpack_hits(d, wire, back)
        with pytest.raises(rt.SvoError, match=err):
            solid.cast_wire(d, wire)
        with pytest.raises(rt.SvoError, match=err):
            solid.wire_scatter(d, wire, back)
        try:
            with pytest.raises(rt.SvoError, match=err):
                x.frames(solid, d, out, back)
            with pytest.raises(rt.SvoError, match=err):
                x.wire(solid, d, wire, back)
        except BaseException:
            x.close()
            raise
        torch.cuda.synchronize()
        assert bool((wire == SENTINEL).all()) and _untouched(torch, back)
    x.close()
    assert solid.guard_trips() == 0


# ---------------------------------------------------------------------------------------- C: sync after palette growth --
@pytest.mark.parametrize("size", [4095, 32767])
def test_sync_after_palette_growth(rt, cuda, oracle_mod, base, frames, size):
    torch = cuda
    M, _ = base
    w, T = hall.hall(rt, oracle_mod, preload=size - 1 - M)  # (an oracle tree of its own: it is edited below)
    solid, scene = w.build().upload(0), w.build(rt.VIEW_ALL).upload(0)
    assert solid.info().n_materials == size
    pts = pc.grow(w)
    for at, flags, cid in pc.GROWTH:
        assert T.put_block(*at, flags, int(hall.colour(cid)), 0.0, hall.LEVELS + 1) == 0
    for t in (solid, scene):
        t.update(w, pts)
        t.sync()
        assert t.info().n_materials == size + 3
    pal_solid, pal_scene = pc.decoded(solid), pc.decoded(scene)
    sun = rt.sun_dir()
    seen = []
    for name in ("room_fractional", "pool_wide"):
        f = frames[name]
        pose, org, dirs, cam, ppx, ppy = f
        n = len(org)
        ref = T.cast_frame(pose[1], cam, hall.FRAME_W, hall.FRAME_H, 300, ppx, ppy)
        out = solid.cast_frame(pose[1], cam, hall.FRAME_W, hall.FRAME_H, 300, ppx=ppx, ppy=ppy)
        compare(rt, solid, out, ref, "C %d %s" % (size, name), palette=pal_solid)
        want = ref_ids(ref, pal_solid)
        assert np.array_equal(check_info(out, 1, size + 2, "C"), want)
        seen.append(want)
        wet = T.shade_rays(org, dirs, 300, sun, liquid=True, time=TIME)
        rgba, out = tds.shade_desc(rt, torch, solid, tds.frame_desc(rt, f, 300), n, True, scene=scene, time=TIME)
        tds.check(rt, scene, rgba, out, wet, "C %d %s shaded" % (size, name), palette=pal_scene)
        seen.append(ref_ids(wet, pal_scene))
    seen = np.concatenate(seen)
    report("C %d" % size, seen, pal_scene[0])
    assert (seen == size + 2).any() and (seen == size).any() and (seen < size).any()  # by the oracle: the new mirror and plain voxel, and old ids
    tds.no_guard(solid, scene)


# ------------------------------------------------------------------------------------------------- D: volume builder --
D_VOLUMES = {"aligned": (64, 64, 64, (0, 0, 0), 7), "offgrid": (37, 29, 22, (9, 6, 3), 8)}  # (off the grid: cut by every face)


def _twin(rt, vol, origin, view, table, levels=3):
    """(volume-built tree, host-built twin, palette): the twin's world numbers its materials as the table does"""
    h, pal, ids = vc.host_twin(rt, levels, vol, origin, view, table=table, world=pc.world_with_palette(rt, levels, table))
    assert np.array_equal(ids, vol) and pal == pc.stored_palette(table)
    return rt.Tree.volume_gpu(levels, vol, pal, origin=origin, view=view), h, pal


@pytest.mark.parametrize("case", sorted(D_VOLUMES))
@pytest.mark.parametrize("lookup,view", [("HIGH", 0), ("HIGH", 1), ("WORD", 0), ("WORD", 1)],
                         ids=["HIGH-view0-classes_mapped", "HIGH-view1-classes_mapped", "WORD-view0-classes_mapped", "WORD-view1-classes_mapped"])
def test_volume_build_with_wide_ids(rt, cuda, oracle_mod, lookup, view, case):
    """the in-view bit table is consulted (k_vol_classes<true>): view 0 hides the liquid ids, and either view hides the ids
    without a colour"""
    nx, ny, nz, origin, seed = D_VOLUMES[case]
    table = pc.table_of(lookup)
    vol, src, has_big = pc.planted(nx, ny, nz, origin, seed, lookup)
    assert has_big == (case == "aligned")
    L = pc.LOOKUPS[lookup]
    assert set(L) | set(pc.extras_of(lookup)[0]) <= set(np.unique(vol).tolist())  # by numpy: every id of the case occurs
    label = "D %s view %d %s" % (lookup, view, case)
    g, h, pal = _twin(rt, vol, origin, view, table)
    _same(g, h, label)
    got = g.read_volume(origin, vol.shape).cpu().numpy().view(np.uint16)
    want = vc.in_view(vol, pal, view)
    assert np.array_equal(got, want), label
    pf = np.array([p[0] for p in pal], np.uint32)
    pcol = np.array([p[1] for p in pal], np.uint64)
    liquid, blank = (pf[vol] & 0x10) != 0, (pcol[vol] == pc.NO_COLOUR) & (vol != 0)
    assert liquid.sum() > 30 and blank.sum() >= 40
    assert not got[blank].any() and np.array_equal(got != vol, blank | (liquid if view == 0 else np.zeros_like(liquid)))
    report(label + " stored", got[got != 0], pf)
    nodes, mats = g.export()
    kind, mat = (nodes[:, 1] >> np.uint64(32)) & np.uint64(3), nodes[:, 1] >> np.uint64(48)
    ox, oy, oz = origin
    if case == "aligned":  # the 16^3 SOLID, and the 16^3 with one liquid voxel (the three bricks lie under the first)
        ni = int(g.node_indices([(1, 1, 1)])[0])
        assert (src[0:16, 0:16, 0:16] == 4).all() and kind[ni] == tvp.K_SOLID and mat[ni] == L[3]
        assert src[16 + 5, 9, 2] == 5 and g.get_block(2, 9, 21)[1] == (L[4] if view == 1 else 0) and g.get_block(2, 9, 22)[1] == L[2]
    else:          # the three bricks at the first aligned 4^3 of the box, (12, 8, 4): SOLID, uniform with a hole, mixed
        assert (src[4 - oz:8 - oz, 8 - oy:12 - oy, 12 - ox:16 - ox] == 2).all() and (src[4 - oz:8 - oz, 8 - oy:12 - oy, 16 - ox:20 - ox] == 3).sum() == 63
        na, nb, nc = (int(i) for i in g.node_indices([(13, 9, 5), (17, 9, 5), (21, 9, 5)]))
        assert kind[na] == tvp.K_SOLID and mat[na] == L[1]
        assert kind[nb] == tvp.K_BRICK and mat[nb] == L[2] and bin(int(nodes[nb, 0])).count("1") == 63
        assert kind[nc] == tvp.K_BRICK and nodes[nc, 0] == np.uint64(0xFFFFFFFFFFFFFFFF)
        run = mats[int(nodes[nc, 1]) & 0xFFFFFFFF:][:64]
        assert set(run.tolist()) == {L[0], L[3]}
    if view == 0:  # casts against the oracle, which holds the same voxels (none for an id without a colour)
        T = vc.oracle_twin(oracle_mod, 3, pc.voxel_puts(vol, origin, table), table=table)
        decoded = (pf, pcol)
        g.guard_trips(reset=True)
        seen = []
        for ci, (org, d) in enumerate(CAMS):
            dn = rt.normalize(d)
            ref = T.cast_frame(org, dn, 64, 32, 300)
            assert ref["rc"] == 0
            seen.append(ref_ids(ref, decoded))
            for flags in (0, rt.CAST_NO_CEILINGS, rt.CAST_ITERATIVE):
                out = g.cast_frame(org, dn, 64, 32, 300, flags=flags)
                compare(rt, g, out, ref, "%s cam%d flags=%d" % (label, ci, flags), palette=decoded)
                assert np.array_equal(check_info(out, 1, len(pal) - 1, label), seen[-1])
        seen = np.concatenate(seen)
        lo, hi = report(label + " casts", seen, pf)
        assert lo <= (0x7FFF if lookup == "HIGH" else 31) and hi >= (pc.CAP if lookup == "HIGH" else 32)  # by the oracle
        assert g.guard_trips() == 0


@pytest.mark.parametrize("case", sorted(D_VOLUMES))
def test_volume_build_without_the_bit_table(rt, cuda, case):
    """view 1 and the first 63 table entries (no entry without a colour below 63): every id is in view, so
    k_vol_classes<false> runs; ids 31 / 32 / 33 / 62"""
    nx, ny, nz, origin, seed = D_VOLUMES[case]
    table = pc.WIDE_TABLE[:63]
    vol = pc.through(vc.planted(nx, ny, nz, origin, seed)[0], (31, 32, 33, 62, 30))
    g, h, pal = _twin(rt, vol, origin, 1, table)
    assert all(c != pc.NO_COLOUR for _, c, _ in pal[1:])
    _same(g, h, "D classes_plain %s" % case)
    got = g.read_volume(origin, vol.shape).cpu().numpy().view(np.uint16)
    assert np.array_equal(got, vol)
    report("D classes_plain %s stored" % case, got[got != 0], np.array([p[0] for p in pal], np.uint32))


def test_uniform_volume_of_the_top_id(rt, cuda, oracle_mod):
    """a whole-extent volume of id 65534: a lone K_SOLID root of that material (one below the class pyramid's MIXED marker),
    hit by a ray that starts one extent away (coordinates wrap)"""
    vol = np.full((64, 64, 64), pc.CAP, np.uint16)
    g = rt.Tree.volume_gpu(3, vol, PALW)
    nodes, _ = g.export()
    assert len(nodes) == 1 and ((int(nodes[0, 1]) >> 32) & 3) == tvp.K_SOLID and int(nodes[0, 1]) >> 48 == pc.CAP
    assert cuda.equal(g.read_volume((0, 0, 0), (64, 64, 64)), cuda.from_numpy(vol.view(np.int16)).cuda())
    T = oracle_mod.Tree(3)
    oracle_mod.lib().orc_init_clean_root(T.h)
    assert T.put_block(0, 0, 0, pc.WIDE_TABLE[pc.CAP][0], pc.WIDE_TABLE[pc.CAP][1], 0.0, 1) == 0
    decoded = pc.decoded(g)
    g.guard_trips(reset=True)
    for org in ((70.5, 10.5, 10.5), (-90.25, 200.5, 3.0)):
        dn = rt.normalize((1.0, 0.1, 0.2))
        ref = T.cast_frame(org, dn, 64, 32, 300)
        out = g.cast_frame(org, dn, 64, 32, 300)
        compare(rt, g, out, ref, "D uniform %s" % (org,), palette=decoded)
        ids = check_info(out, pc.CAP, pc.CAP, "D uniform")
        assert (ref["hit"] != 0).all() and len(ids) == 64 * 32
    report("D uniform", ids, decoded[0])
    assert g.guard_trips() == 0


def test_volume_id_65535_is_reported(rt, cuda):
    vol = cuda.zeros((9, 10, 21), dtype=cuda.int16, device="cuda:0")
    vol[8, 9, 20] = -1  # 0xFFFF = n_palette
    assert len(PALW) == 65535
    with pytest.raises(rt.SvoError, match=r"\(-5\).*n_palette"):
        rt.Tree.volume_gpu(3, vol, PALW, origin=(3, 1, 2))
    vol[8, 9, 20] = -2  # 0xFFFE = 65534
    t = rt.Tree.volume_gpu(3, vol, PALW, origin=(3, 1, 2))
    assert t.get_block(23, 10, 10)[1] == pc.CAP and t.get_block(23, 10, 10)[0] == PALW[pc.CAP]


# ---------------------------------------------------------------------------------------------------- E: volume patch --
@pytest.fixture(scope="module")
def old64():
    """test_gpu_volume_patch's old world through HIGH"""
    vol, has_big = vc.planted(64, 64, 64, (0, 0, 0), 7)
    assert has_big
    vol[20:24, 20:24, 20:24] = 3
    vol[21, 22, 23] = 0
    vol[36:40, 24:28, 40:44] = 1
    vol[36:40, 24:26, 40:44] = 4
    vol = pc.through(vol, pc.HIGH)
    vol.setflags(write=False)
    return vol


CUT = "cuts the 16^3 SOLID"


def _cut(rt, old64, view):
    origin = tvp.BOXES[CUT]
    new = pc.through(vc.random_volume((22, 9, 13), 0.5, 11 + sorted(tvp.BOXES).index(CUT)), pc.HIGH)
    assert (new == pc.HIGH[4]).any()
    t = tvp._tree(rt, 3, old64, view, PALW)
    t.patch_volume(new, origin)
    return t, tvp._put(old64, new, origin), origin, new


@pytest.mark.parametrize("view", [0, 1])
def test_patch_cuts_the_solid_region(rt, cuda, old64, view):
    assert (old64[0:16, 0:16, 0:16] == pc.HIGH[3]).all()
    t, comp, origin, new = _cut(rt, old64, view)
    assert t.garbage()[0] > 0
    tvp.check_all(rt, cuda, t, comp, view, origin, new.shape, "E cut view %d" % view, pal=PALW)
    mats = set(t.export()[1].tolist())
    assert {0x7FFF, 4095} <= mats and ((0x8001 in mats) == (view == 1))
    mask, kind, mat = tvp._kinds(t)
    ni, nj = (int(i) for i in t.node_indices([(1, 1, 1), (5, 1, 1)]))
    assert kind[ni] == tvp.K_SOLID and mat[ni] == 4095 and kind[nj] == tvp.K_SOLID and ni != nj
    got = t.read_volume((0, 0, 0), (64, 64, 64)).cpu().numpy().view(np.uint16)
    report("E cut view %d stored" % view, got[got != 0], np.array([p[0] for p in PALW], np.uint32))
    assert np.array_equal(np.unique(got[got != 0]), np.unique(vc.in_view(comp, PALW, view))[1:])  # by numpy


def test_patch_fills_aligned_regions(rt, cuda, old64):
    t = tvp._tree(rt, 3, old64, 0, PALW)
    a = np.full((16, 16, 16), pc.CAP, np.uint16)
    t.patch_volume(a, (32, 16, 48))
    comp = tvp._put(old64, a, (32, 16, 48))
    mask, kind, mat = tvp._kinds(t)
    ni = t.node_indices([(32, 16, 48), (47, 31, 63), (40, 20, 50)])
    assert len(set(ni.tolist())) == 1 and kind[ni[0]] == tvp.K_SOLID and mat[ni[0]] == pc.CAP
    b = np.full((4, 4, 4), 0x8000, np.uint16)
    t.patch_volume(b, (20, 24, 28))
    comp = tvp._put(comp, b, (20, 24, 28))
    mask, kind, mat = tvp._kinds(t)
    ni = t.node_indices([(20, 24, 28), (23, 27, 31)])
    assert ni[0] == ni[1] and kind[ni[0]] == tvp.K_SOLID and mat[ni[0]] == 0x8000
    tvp.check_all(rt, cuda, t, comp, 0, (20, 24, 28), b.shape, "E filled", pal=PALW)
    solids = set(mat[kind == tvp.K_SOLID].tolist())
    print("E filled: K_SOLID materials", sorted(solids))
    assert {pc.CAP, 0x8000} <= solids


def test_patch_empties_a_populated_region(rt, cuda, old64):
    assert old64[7:27, 6:26, 5:25].any()
    t = tvp._tree(rt, 3, old64, 0, PALW)
    zero = np.zeros((20, 20, 20), np.uint16)
    t.patch_volume(zero, (5, 6, 7))
    comp = tvp._put(old64, zero, (5, 6, 7))
    fresh = tvp.check_all(rt, cuda, t, comp, 0, (5, 6, 7), zero.shape, "E emptied", pal=PALW)
    assert tvp.check_casts(rt, cuda, t, fresh, "E emptied, AO", ao=True) > 0


def test_patch_refuses_id_65535(rt, cuda, old64):
    t = tvp._tree(rt, 3, old64, 0, PALW)
    assert t.info().n_materials == 65535
    before = t.read_volume((0, 0, 0), (64, 64, 64)).clone()
    nodes, mats = t.export()
    g = t.garbage()
    bad = pc.through(vc.random_volume((22, 9, 13), 0.5, 62), pc.HIGH)
    bad[21, 8, 12] = 65535
    with pytest.raises(rt.SvoError, match=r"\(-5\).*palette"):
        t.patch_volume(bad, (9, 10, 3))
    assert cuda.equal(t.read_volume((0, 0, 0), (64, 64, 64)), before)
    n2, m2 = t.export()
    assert nodes.tobytes() == n2.tobytes() and mats.tobytes() == m2.tobytes() and t.garbage() == g


def test_shaded_frame_with_patched_wide_scene(rt, cuda, old64):
    t0, comp, _, _ = _cut(rt, old64, 0)
    t1 = _cut(rt, old64, 1)[0]
    f0, f1 = tvp._tree(rt, 3, comp, 0, PALW), tvp._tree(rt, 3, comp, 1, PALW)
    cam = rt.normalize((0.6, -0.45, 0.66))
    (a, ha), (b, hb) = (s.shade_frame((1.0, 40.0, 3.0), cam, 128, 64, 300, scene=sc, time=0.25, with_hits=True) for s, sc in ((t0, t1), (f0, f1)))
    assert cuda.equal(a, b)
    for k in ("pos_steps", "t", "info"):
        assert cuda.equal(ha[k], hb[k]), k
    ids = check_info(ha, 1, pc.CAP, "E shaded", bits=False)
    report("E shaded end blocks", ids, np.array([p[0] for p in PALW], np.uint32))
    assert (ids >= 0x8000).any() and (ids <= 0x7FFF).any()
    assert t0.guard_trips() == 0 and t1.guard_trips() == 0


def test_mini_cavern_with_wide_ids(rt, cuda, oracle_mod):
    """volume_cases.mini_cavern() through HIGH, 4 levels: casts and the AO frame against the oracle"""
    src, puts = vc.mini_cavern()
    vol = pc.through(src, pc.HIGH)
    g = rt.Tree.volume_gpu(4, vol, PALW)
    T = vc.oracle_twin(oracle_mod, 4, pc.puts_through(puts, pc.HIGH), table=pc.WIDE_TABLE)
    decoded = pc.decoded(g)
    g.guard_trips(reset=True)
    seen = []
    for ci, (org, d) in enumerate(CAMS):
        org = tuple(o + s for o, s in zip(org, (100.0, 36.0, 120.0)))
        dn = rt.normalize(d)
        ref = T.cast_frame(org, dn, 64, 32, 300)
        assert ref["rc"] == 0
        seen.append(ref_ids(ref, decoded))
        for flags in (0, rt.CAST_NO_CEILINGS, rt.CAST_ITERATIVE):
            out = g.cast_frame(org, dn, 64, 32, 300, flags=flags)
            compare(rt, g, out, ref, "E cavern cam%d flags=%d" % (ci, flags), palette=decoded)
            assert np.array_equal(check_info(out, 1, pc.CAP, "E cavern"), seen[-1])
    seen = np.concatenate(seen)
    lo, hi = report("E cavern casts", seen, decoded[0])
    assert lo <= 0x7FFF and hi == pc.CAP  # by the oracle
    org, dn = (101.0, 50.0, 123.0), rt.normalize((0.6, -0.45, 0.66))
    ao, hit = T.cast_frame_ao(org, dn, 64, 32, 400, 16, 5)
    out = rt.decode_hits(g.cast_frame(org, dn, 64, 32, 400, ao_samples=16, ao_steps=5))
    assert np.array_equal(out["hit"], hit != 0) and np.array_equal(out["ao"], ao) and int(ao.sum()) > 0
    assert g.guard_trips() == 0
