"""The oracle and the product's host side pinned to the reference's own compiled code (oracle/REFERENCE_PINS.md).

tests/golden/pins_R.npz and pins_P.npz hold lookups, ray batteries and pixel fans on the reference application's world
(R) and on the pin world (P, tests/pin_world.py) with the answers of oracle/_ref/ref_core: the reference's
tetrahexa_tree.cpp, voxel_allocator.cpp, world_gen.cpp and ray_caster.cpp, compiled from where they lie.  The oracle
(oracle/oracle.c) must give every recorded answer, bit for bit, no entry left out; so must the product's getBlock.
Where ref_core has been built the same comparison runs live on freshly seeded, larger inputs, genWorld is compared voxel
for voxel, and deleteBlock in the two cases the reference can run (tests/pin_cases.py holds the inputs' construction)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cavern  # noqa: E402
import pin_cases as pc  # noqa: E402
import pin_world  # noqa: E402

WORLDS = ("R", "P")


@pytest.fixture(scope="module")
def oracle_worlds(oracle_mod):
    """{world: oracle Tree}, built once and left unchanged"""
    return {w: pc.oracle_world(oracle_mod, w) for w in WORLDS}


def need_ref_core(oracle_mod):
    if not os.path.exists(oracle_mod.REF_CORE):
        pytest.skip("oracle/_ref/ref_core has not been built (the reference's sources were absent at build time)")


def check_pools(T, pools, root):
    assert (T.nodes(), T.arrays()) == (pools["nodes"], pools["arrays"])
    assert pools["node_free"] == 0 and pools["array_free"] == 0
    assert T.root_bitmap() == root["bitmap"] and T.L.orc_root_flags(T.h) == root["flags"] and T.L.orc_root_children(T.h) == root["children"]


# ------------------------------------------------------------------------------------------------ oracle vs fixtures --
@pytest.mark.parametrize("world", WORLDS)
def test_fixture_holds_what_it_should(oracle_mod, world):
    """the recorded inputs cover the classes they are meant to, none left out, and on R nothing reaches root child 63"""
    inp, rec, pools, root = pc.load(world)
    n = len(inp["ray_org"])
    assert len(inp["probes"]) >= 4000 and n >= 2000 and len(rec["frame_steps"]) == 6 * pc.FRAME_W * pc.FRAME_H
    assert len(rec["probe_flags"]) == len(inp["probes"]) and len(rec["ray_steps"]) == n
    assert set(pc.BUDGETS) <= set(inp["ray_budget"].tolist())
    o, d = inp["ray_org"], inp["ray_dir"]
    assert (o == np.trunc(o)).all(1).sum() > 100 and ((o * 2 == np.trunc(o * 2)) & (o != np.trunc(o))).any(1).sum() > 100
    assert (o < 0).any(1).sum() > 100 and (o >= pc.E).any(1).sum() > 100  # negative (trunc, not floor) and beyond the extent
    bits = d.view(np.uint32)
    assert (bits == 0x80000000).any() and (bits == 0).any() and (bits == 1).any()  # -0.0, 0.0, the smallest denormal
    assert directed_ties(o, d) > 100
    assert (np.abs(np.linalg.norm(d.astype(np.float64), axis=1) - 1) > 0.5).sum() > 100  # un-normalised
    hit = pc.hit_of(rec["ray_flags"], rec["ray_color"], inp["ray_budget"])
    assert 0.1 < hit.mean() < 0.9
    assert (hit & (rec["ray_steps"] == 0)).any()  # a hit on the last step: only the block at pos tells it from a miss
    liquid = (rec["probe_flags"] & 0x10) != 0
    assert liquid.sum() > 10 and ((rec["probe_color"] != pc.EMPTY) & ~liquid).sum() > 400
    assert sorted(set(pc.dir_checksum(pc.frame_dirs(oracle_mod, dd, *inp["frame_pp"])) for dd in inp["frame_dir"])) == sorted(set(rec["frame_dirsum"]))
    fhit = pc.hit_of(rec["frame_flags"], rec["frame_color"], np.repeat(inp["frame_budget"], pc.FRAME_W * pc.FRAME_H))
    assert 0.1 < fhit.mean() < 0.9
    if world == "R":
        assert not pc.in_child63(inp["probes"]).any() and not pc.child63_on_path(o, d, inp["ray_budget"]).any()
    else:
        assert (rec["ray_flags"] & 0x10).any()  # a ray that ends inside liquid: a miss with a stored block at pos
        kinds = set(cavern.ident(rec["probe_color"][rec["probe_color"] != pc.EMPTY]).tolist())
        assert {100, 200, 300, 400, 600, 700, 900, 950, 1100, 1110, 1120, 1130, 1140, 1150} <= kinds


def directed_ties(org, dirs):
    """rays with at least 20 exact ties in 300 steps (test_gpu_directed_rays.tie_counts)"""
    return int((pc.directed.tie_counts(org, dirs) >= 20).sum())


@pytest.mark.parametrize("world", WORLDS)
def test_oracle_gives_the_recorded_reference_answers(oracle_mod, oracle_worlds, world):
    """every lookup, the pool counts and the root, and every ray record (pos, lastPos, steps left, the block at pos and
    with it the hit) of the fixture from the oracle, equal"""
    inp, rec, pools, root = pc.load(world)
    T = oracle_worlds[world]
    check_pools(T, pools, root)
    pc.same_records(rec, pc.oracle_records(oracle_mod, T, inp), "oracle vs recorded reference, world " + world)


@pytest.mark.parametrize("world", WORLDS)
def test_product_lookups_give_the_recorded_reference_answers(rt, world):
    """svo_get_blocks on the product's World (R: World.reference(); P: built with put_blocks) at the recorded probes.
    (On R the product also stores the (1000, 1000, 1000) debug block, which the reference's aliased root child array
    loses; it lies in root child 63, where the reference cannot be asked.)"""
    inp, rec, _, _ = pc.load(world)
    f, c, _ = pc.product_world(rt, world).get_blocks(inp["probes"])
    assert np.array_equal(f, rec["probe_flags"]) and np.array_equal(c, rec["probe_color"])


# -------------------------------------------------------------------------------------------------------------- live --
@pytest.mark.parametrize("world", WORLDS)
def test_live_oracle_against_the_compiled_reference(oracle_mod, oracle_worlds, world):
    """about 20,000 probes and 20,000 rays with seeds of their own (no fans: they have no seed), through ref_core and the oracle"""
    need_ref_core(oracle_mod)
    inp = pc.make_inputs(world, oracle_mod, 977 + len(world), 20000, 3100, fans=False)
    assert len(inp["ray_org"]) >= 20000
    rec, pools, root = pc.reference_records(oracle_mod, world, inp)
    T = oracle_worlds[world]
    check_pools(T, pools, root)
    pc.same_records(rec, pc.oracle_records(oracle_mod, T, inp), "live oracle vs reference, world " + world)


def test_live_fixtures_are_what_the_reference_says(oracle_mod):
    """the committed records equal what ref_core answers now on the committed inputs"""
    need_ref_core(oracle_mod)
    for world in WORLDS:
        inp, rec, pools, root = pc.load(world)
        now, pools_now, root_now = pc.reference_records(oracle_mod, world, inp)
        pc.same_records(rec, now, "fixture vs reference, world " + world)
        assert pools_now == pools and root_now == root


def test_live_gen_world_voxel_for_voxel(oracle_mod, oracle_worlds):
    """genWorld through the reference against orc_gen_world: the 200 x 72 x 200 box and a margin (columns past the
    terrain on every side, wrapping below 0; rows 0..75)"""
    need_ref_core(oracle_mod)
    lo, shape = (-4, 0, -4), (208, 76, 208)
    ref = oracle_mod.ref_core_run([("init",), ("gen",), ("box", lo, shape)])[2]
    rc, f, c = oracle_worlds["R"].dump_box(*lo, *shape)
    assert rc == 0 and f.shape == ref["flags"].shape
    assert np.array_equal(f, ref["flags"]) and np.array_equal(c, ref["color"])
    stored = c != pc.EMPTY
    assert 0.2 < stored.mean() < 0.5 and not stored[:4].any() and not stored[:, :, :4].any() and not stored[:, 73:].any()
    assert ((f & 0x10) != 0).sum() > 1000  # water


# ------------------------------------------------------------------------------------------------- the safety check --
def test_pin_world_is_reference_safe_and_unsafe_lists_are_rejected():
    """pin_world.check_reference_safe on the pin world, and on lists the reference must never be given (they are not given
    to it here either): a voxel inside a coarser leaf, a leaf over finer content, cavern's dust inside its 16^3 / 64^3 blocks"""
    assert pin_world.check_reference_safe(pin_world.puts()) > 10000
    one = lambda p, lv: (np.array([p]), np.zeros(1, np.uint32), cavern.colour([1]), lv)  # noqa: E731
    pin_world.check_reference_safe([one((16, 16, 16), 4), one((16, 16, 16), 4), one((32, 16, 16), 6), one((33, 16, 16), 6), one((36, 16, 16), 5)])
    for bad in ([one((16, 16, 16), 4), one((20, 17, 30), 6)],            # a voxel inside a 16^3 leaf
                [one((0, 0, 0), 3), one((60, 60, 60), 5)],              # a 4^3 block inside a 64^3 leaf
                [one((16, 16, 16), 5), one((16 + cavern.E, 17 - cavern.E, 18), 6)],  # the same through the wrap
                [one((33, 16, 16), 6), one((32, 16, 16), 5)],            # a 4^3 leaf over a stored voxel
                [one((300, 5, 5), 6), one((256, 0, 0), 2)],              # a 256^3 leaf over a stored voxel
                [one((1, 1, 1), 1)], [one((1, 1, 1), 7)]):               # the root itself; below the voxels
        with pytest.raises(ValueError):
            pin_world.check_reference_safe(bad)
    with pytest.raises(ValueError):
        pin_world.check_reference_safe(cavern._puts(True))
    with pytest.raises(ValueError):
        pin_world.check_reference_safe(pin_world.puts() + [one((cavern.BIG[0] + 3, cavern.BIG[1] + 3, cavern.BIG[2] + 3), 6)])


# ------------------------------------------------------------------------------------------------------- deleteBlock --
DELETE_CELL = np.array([40, 80, 120])  # a 4^3 cell; slot = z << 4 | y << 2 | x of a voxel's offset in it (tetrahexa_tree.cpp:309)


def slot_pos(slot):
    return DELETE_CELL + np.array([slot & 3, (slot >> 2) & 3, (slot >> 4) & 3])


@pytest.mark.parametrize("target", [5, 37])
def test_live_delete_block_one_voxel(oracle_mod, target):
    """deleteBlock as the last mutation of a fresh reference process, against orc_delete_block(ref_shift=True).

    Its level convention (tetrahexa_tree.cpp:343-354): it steps down, then compares the new depth with `level` without
    putBlock's decrement, so level 5 deletes a voxel (depth 5) and level 6 would write stack[maxDepth]: only level 5 is
    used.  The parent's bit is cleared with the int expression `1 << index` (:352).  For slot 5 that is bit 5.  For slot
    37 the compiled reference flips bit 37 & 31 = 5 instead: slot 5 is stored here too, so it is the one that
    disappears, slot 37 stays readable, and every lookup afterwards stays inside defined behaviour.  (Were slot 5 empty,
    the flip would set its bit over a null child: a later getBlock there walks into the root and exits.  Slot 31, where
    the int is negative and bits 31..63 flip, and deletes that free child arrays are left out: see REFERENCE_PINS.md.)"""
    need_ref_core(oracle_mod)
    slots = [5, 37, 10, 63]
    pts = np.array([slot_pos(s) for s in slots])
    flags = np.array([0, 2, 4, 0x14], np.uint32)
    cols = cavern.colour(np.arange(len(slots)) + 1)
    box = np.array([DELETE_CELL - 1 + np.array([x, y, z]) for z in range(6) for y in range(6) for x in range(6)])
    res = oracle_mod.ref_core_run([("clean",), ("put", pts, flags, cols, 6, 0.5), ("delete", slot_pos(target), 5), ("get", box), ("pools",)])
    gone, after, pools = res[2:]
    T = oracle_mod.Tree(5)
    oracle_mod.lib().orc_init_clean_root(T.h)
    for p, f, c in zip(pts.tolist(), flags.tolist(), cols.tolist()):
        assert T.put_block(*p, f, c, 0.5, 6) == 0
    rc, blk = T.delete_block(*[int(v) for v in slot_pos(target)], level=5, ref_shift=True)
    assert rc == 0 and blk == (int(gone["flags"][0]), int(gone["color"][0]), float(gone["meta"][0]))
    assert blk[1] == int(cols[slots.index(target)])
    got = [T.get_block(*[int(v) for v in p]) for p in box]
    assert np.array_equal(np.array([g[0] for g in got], np.uint32), after["flags"])
    assert np.array_equal(np.array([g[1] for g in got], np.uint64), after["color"])
    assert (T.nodes(), T.arrays(), T.L.orc_tree_error(T.h)) == (pools["nodes"], pools["arrays"], 0)
    assert pools["node_free"] == 1 and pools["array_free"] == 0
    left = set(cavern.ident(after["color"][after["color"] != pc.EMPTY]).tolist())
    assert left == {2, 3, 4}  # slot 5's voxel (id 1) is gone either way; slot 37's (id 2) stays even when it was the target
