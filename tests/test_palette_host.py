"""Large palettes on the CPU (tests/palette_cases.py): the hall with its material ids shifted onto every boundary — 31 / 32,
4095 / 4096, 0x7FFF / 0x8000 and the cap 65534 — holds, in the World and in both linearised views, the blocks the oracle
holds (which stores flags and colour per voxel and has no palette: an independent reference for any id); the cap's error
leaves the world as it was; svo_tree_update takes over a palette that grew across 4096 and across 0x8000; a full palette
survives save and load; and tests/wire_ref.py packs and unpacks its own 12-bit material fields at their limit."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hall  # noqa: E402
import palette_cases as pc  # noqa: E402
import wire_ref  # noqa: E402

EMPTY = np.uint64(0xFFFFFFFFFFFFFFFF)
N_PALETTE_AT = 20  # the u32 n_palette of a tree file's header (svo_tree_file.cpp): after the magic, format, levels and view


@pytest.fixture(scope="module")
def base(rt, oracle_mod):
    """(M, oracle Tree, probe points, the oracle's flags and colours there): the unshifted hall, shared and left unchanged"""
    w, T = hall.hall(rt, oracle_mod)
    M = pc.scene_materials(w)
    pts = hall.probe_points(12000)
    ref = [T.get_block(int(x), int(y), int(z)) for x, y, z in pts]
    return M, T, pts, np.array([r[0] for r in ref], np.uint32), np.array([r[1] for r in ref], np.uint64)


def shifted(rt, oracle_mod, base, k):
    return hall.hall(rt, oracle_mod, preload=k, T=base[1])[0]


def test_preload_changes_no_content(rt, oracle_mod, base):
    """palette size 1 + k, nothing stored; the fillers collide with no scene colour; an emptied world linearises to the
    lone empty root (the canonical form: the volume builder's trees are compared with such worlds byte for byte)"""
    w = rt.World(hall.LEVELS)
    pc.preload(w, 100, hall.FILLER_AT)
    t = w.build()
    assert len(t.palette()) == 101 and t.get_blocks([hall.FILLER_AT])[0] == 0
    nodes, mats = t.export()
    assert len(nodes) == 1 and nodes[0, 0] == 0 and len(mats) == 0
    assert w.get_block(*hall.FILLER_AT)[1] == EMPTY
    used = set(np.concatenate([c for _, _, c, _ in hall._puts()]).tolist())
    assert not used & set(pc.filler_colours(pc.CAP).tolist()) and int(EMPTY) not in set(pc.filler_colours(pc.CAP).tolist())
    assert pc.cavern_is_clear_of_fillers()
    assert set(pc.SHIFTS(base[0])) == set(pc.SHIFT_NAMES)


def test_world_with_palette(rt):
    """the 65535-entry table becomes the palette entry for entry, and the world is empty"""
    w = pc.world_with_palette(rt, 3, pc.WIDE_TABLE)
    t = w.build(rt.VIEW_ALL)
    assert t.palette() == pc.stored_palette(pc.WIDE_TABLE)
    nodes, _ = t.export()
    assert len(nodes) == 1 and nodes[0, 0] == 0


@pytest.mark.parametrize("shift", pc.SHIFT_NAMES)
def test_block_parity(rt, oracle_mod, base, shift):
    """test_hall_host.test_block_parity's content check on the shifted hall: World.get_blocks is the oracle's getBlock; the
    solid tree's palette entry is the oracle's block with liquid taken as empty, the VIEW_ALL tree's is the block itself;
    and the stored ids are K + 1 .. K + M"""
    M, T, pts, rf, rc = base
    K = pc.SHIFTS(M)[shift]
    w = shifted(rt, oracle_mod, base, K)
    wf, wc, _ = w.get_blocks(pts)
    assert np.array_equal(wc, rc)
    assert np.array_equal(wf[rc != EMPTY], rf[rc != EMPTY])
    liquid = (rc != EMPTY) & ((rf & 0x10) != 0)
    assert liquid.sum() > 100
    for view, gone in ((rt.VIEW_SOLID, liquid), (rt.VIEW_ALL, np.zeros(len(pts), bool))):
        tree = w.build(view)
        ids = tree.get_blocks(pts)
        pf, pcol = pc.decoded(tree)
        assert len(pf) == 1 + K + M
        stored = (rc != EMPTY) & ~gone
        assert np.array_equal(ids != 0, stored), (shift, view)
        assert np.array_equal(pcol[ids][stored], rc[stored]) and np.array_equal(pf[ids][stored], rf[stored]), (shift, view)
        seen = ids[stored]
        print("%s K=%d view %d: stored ids %d .. %d" % (shift, K, view, seen.min(), seen.max()))
        # (every material of the hall is probed: test_hall_host.test_block_parity asserts that of these points)
        assert seen.min() == K + 1 and seen.max() == K + M  # (the first and the last material put are not liquid)
        if view == rt.VIEW_ALL:
            assert len(np.unique(seen)) == M


def test_the_cap(rt, oracle_mod, base):
    """a 65535th distinct block is refused with SVO_ERANGE and nothing changes; a batch stops at its first failure, with
    the entries before it stored; an interned block can still be put"""
    M = base[0]
    w = shifted(rt, oracle_mod, base, pc.SHIFTS(M)["cap"])
    assert len(w.build().palette()) == 65535
    at = (600, 100, 600)
    new = (0, 0x123456789)
    old = int(hall.colour(hall.C_PILLAR))
    nodes = w.node_count()
    assert w.get_block(*at)[1] == EMPTY
    with pytest.raises(rt.SvoError, match=r"\(-5\).*65534"):
        w.put_block(*at, *new)
    assert w.get_block(*at)[1] == EMPTY and w.node_count() == nodes
    there = hall.MIRROR4
    before = w.get_block(*there)
    with pytest.raises(rt.SvoError, match=r"\(-5\).*65534"):
        w.put_block(*there, *new)
    assert w.get_block(*there) == before and w.node_count() == nodes
    batch = [(600, 100, 600), (601, 100, 600), (602, 100, 600), (603, 100, 600)]
    with pytest.raises(rt.SvoError, match=r"\(-5\).*65534"):
        w.put_blocks(batch, [0, 0, 0, 0], [old, old, new[1], old])
    got = w.get_blocks(batch)[1]
    assert got.tolist() == [old, old, int(EMPTY), int(EMPTY)]  # svo_put_blocks stops at the first failure
    w.put_block(603, 100, 600, hall.F_MIRROR, int(hall.colour(hall.C_WALL)))
    assert w.get_block(603, 100, 600)[:2] == (3, int(hall.colour(hall.C_WALL)))
    assert len(w.build().palette()) == 65535


@pytest.mark.parametrize("size", [4095, 32767])
@pytest.mark.parametrize("view", [0, 1])
def test_update_with_palette_growth(rt, oracle_mod, base, size, view):
    """a tree built at palette size 4095 (32767) takes over, with svo_tree_update, a world whose palette grew by the ids
    4095, 4096, 4097 (32767, 32768, 32769): the same palette and the same blocks as a fresh build"""
    M = base[0]
    w = shifted(rt, oracle_mod, base, size - 1 - M)
    tree = w.build(view)
    assert tree.info().n_materials == size
    pts = pc.grow(w)
    tree.update(w, pts)
    fresh = w.build(view)
    assert tree.info().n_materials == size + 3 and tree.palette() == fresh.palette()
    g = np.arange(-4, 8)
    box = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)
    probe = np.concatenate([(p // 4) * 4 + box for p in pts] + [base[2]]).astype(np.int32)
    got, want = tree.get_blocks(probe), fresh.get_blocks(probe)
    assert np.array_equal(got, want)
    assert got[:3 * len(box)].max() == size + 2 and set(tree.get_blocks(pts).tolist()) == {size, size + 1, size + 2}


@pytest.mark.parametrize("view", [0, 1])
def test_save_and_load_a_full_palette(rt, oracle_mod, base, tmp_path, view):
    M, _, pts, _, _ = base
    w = shifted(rt, oracle_mod, base, pc.SHIFTS(M)["cap"])
    tree = w.build(view)
    path = str(tmp_path / "full.svo")
    tree.save(path)
    back = rt.Tree.load(path)
    assert back.palette() == tree.palette() and len(back.palette()) == 65535
    (na, ma), (nb, mb) = tree.export(), back.export()
    assert np.array_equal(na, nb) and np.array_equal(ma, mb) and int(ma.max()) >= 0x8000
    assert np.array_equal(back.get_blocks(pts), tree.get_blocks(pts)) and back.get_blocks(pts).max() == pc.CAP
    raw = bytearray(open(path, "rb").read())
    n = int.from_bytes(raw[N_PALETTE_AT:N_PALETTE_AT + 4], "little")
    assert n == 65535
    raw[N_PALETTE_AT:N_PALETTE_AT + 4] = (n - 1).to_bytes(4, "little")
    bad = str(tmp_path / "short.svo")
    with open(bad, "wb") as f:
        f.write(raw)
    with pytest.raises(rt.SvoError, match=r"\(-6\)"):
        rt.Tree.load(bad)


def test_wire_reference_at_the_material_limit():
    """tests/wire_ref.py against itself: unpack(pack(records)) gives back info for material ids 1, 4094 and 4095, in the
    12-B and the 8-B format, hits on every axis and sign, and a miss"""
    rng = np.random.default_rng(5)
    n, steps = 600, 300
    mats = np.array([1, 4094, 4095], np.uint32)[np.arange(n) % 3]
    axis = (np.arange(n) // 3 % 3).astype(np.uint32)
    dirs = rng.normal(size=(n, 3)).astype(np.float32)
    step = np.where(dirs < 0, -1, 1)
    neg = step[np.arange(n), axis] < 0
    hit = np.arange(n) % 7 != 0
    info = np.where(hit, np.uint32(wire_ref.HIT_BIT) | mats, np.uint32(0)) | (axis << np.uint32(wire_ref.AXIS_SHIFT)) | \
        np.where(neg, np.uint32(wire_ref.NEG_BIT), np.uint32(0))
    info = info.astype(np.uint32)
    assert {1, 4094, 4095} <= set((info[hit] & 0xFFFF).tolist()) and neg.any() and (~neg).any()
    origins = rng.integers(-40, 900, (n, 3)).astype(np.float32)
    cells = np.trunc(origins).astype(np.int32)
    nk = rng.integers(0, 60, (n, 3))
    pos = cells + step * nk
    left = np.where(hit, steps - nk.sum(1), 0)
    ps = np.concatenate([pos, left[:, None]], 1).astype(np.int32)
    t = rng.uniform(0, 90, n).astype(np.float32)
    ps2, t2, info2 = wire_ref.unpack(wire_ref.pack(ps, t, info, cells), cells, steps)
    assert np.array_equal(info2, info) and np.array_equal(ps2, ps) and np.array_equal(t2.view(np.uint32), t.view(np.uint32))
    ps3, _, info3 = wire_ref.unpack_compact(wire_ref.pack_compact(ps, info, cells), origins, dirs, steps)
    assert np.array_equal(info3, info) and np.array_equal(ps3, ps)
