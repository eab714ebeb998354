"""Every device-side tree edit mixed on two resident trees, against one model (tests/mixed_ops_cases.py): the six patches
(svo_tree_patch_volume_gpu, _points_gpu, _shapes_gpu, _tree_gpu, _tree_oriented_gpu, _tree_rule_gpu) and
svo_tree_compact_gpu.  Both trees run one order of kinds that holds every ordered pair of kinds once (50 kinds at 3 levels,
100 steps; 15 kinds at 2 and at 4 levels, 30 steps), tree A at the even steps and tree B at the odd ones, so that on each
tree every kind runs on what every kind left there; pastes read the other tree, the patched tree itself or a
static prefab.  What passes from one patch to the next is what is checked: the tail appended behind another kind's tail,
the anchor another kind rewrote, K_SOLID records the points patch synthesised and a shape or a paste cuts, records with
mask 0 and bricks that stayed bricks read as a paste's source, garbage counted on the device and by host walks, the
restart that zeroes it, the host image, the ceilings, a compaction between patches and the regrowth of the arrays.
tests/test_mixed_ops_host.py asserts the conditions on the inputs.

Five starts: two volume-built trees (A solid view, B full view; and the views swapped), a world-built A (edit_script's
tree after its last stage and sync()) with a points-built B, a heightfield-built A at 4 levels whose plateau holds a K_SOLID
64^3 that a points step, a shapes step and a paste cut in turn, and two volume-built trees of 2 levels.

After every step, on the tree it changed, all exact: (1) read_volume of the whole extent equals the model; (2) garbage()
equals the walk of the exported tree and no K_BRICK record has mask 0; (3) host get_blocks and get_blocks_gpu at 2,000
seeded positions and the step's box corners equal the model; (4) the fine ceilings in HBM equal the host tree's and the
16-column table is their 4 x 4 maxima; (5) the source of a paste is byte-identical afterwards.  After every compact and
after the last step: test_gpu_points_patch.check_patched against a fresh volume_gpu build of the model (ceilings, casts or
the shading pass, byte equality once compacted), count_voxels / list_voxels against the listing model, an empty diff
against the fresh tree, the diff from the previous checkpoint's model against the diff model and that older tree patched
with it and compacted byte for byte, an upward frame from below the world's top row, and save / load / upload.

Capacity (material entries; the 4161 node records of a 64^3 never pass the slack): mixed_ops_cases.expected_crossings
predicts from the model windows of steps within which a tree's arrays must be reallocated, counted from its fresh upload
or from a compaction (capacity n + n / 8 + 65536 either way), and device_bytes must grow inside each; where no step of
the window restarts the arrays the growth must fall on an appending patch, which keeps a prefix.  As run: at 3 levels B's
fresh upload holds 975 entries (777 in the solid view) with room for 66,632 (66,410) and regrows at the whole-extent
volume of step 7, a restart with about 131,000 (104,930); the world-built A does the same at step 6.  The appending
regrowths fell on an oriented paste (steps 38, 57, 87), a rule paste (43), a shapes patch (63) and plain pastes (12, 67,
72, 77); at 4 levels on A's oriented paste of step 14, the first patch after its compaction; at 2 levels nothing regrows."""
import numpy as np
import pytest

import diff_voxels_cases as dvc
import list_voxels_cases as lvc
import mixed_ops_cases as mc
import points_patch_cases as ppc
import shapes_patch_cases as spc
import volume_cases as vc
from test_gpu_points_patch import K_BRICK, K_SOLID, _stored, check_patched
from test_gpu_volume_build import _same
from test_gpu_volume_patch import _kinds

pytestmark = pytest.mark.gpu

SHIFT = {2: (0.0, 0.0, 0.0), 3: (0.0, 0.0, 0.0), 4: (30.0, 60.0, 30.0)}   # check_patched's cameras, moved over the terrain


@pytest.fixture(scope="module")
def cuda(rt):
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    assert hasattr(rt.lib(), "svo_tree_patch_tree_rule_gpu")
    return torch


@pytest.fixture(scope="module")
def prefabs(rt, cuda):
    """(mixed_ops_cases.prefab_volumes, {name: resident tree}): built once, only ever read"""
    data = mc.prefab_volumes(rt)
    trees = {"prefab2": rt.Tree.volume_gpu(2, np.array(data["prefab2"][3]), mc.PAL, view=1),
             "prefab1": vc.host_twin(rt, 1, data["prefab1"][3], (0, 0, 0), 1)[0].upload(0)}
    for name, t in trees.items():
        assert t.info().levels == data[name][0] and t.palette() == data[name][1] and np.array_equal(_stored(t), data[name][2]), name
    return data, trees


def _start_trees(rt, oracle_mod, st, content=True):
    """the resident trees A and B of a start, and the EditScript of a world-built A; content: compare what they store with
    the start model (the ids of a run that begin at a later step leave that to the one that begins at step 0)"""
    script = None
    if st.name == "L3-world":
        import edit_script

        script = edit_script.EditScript(rt, oracle_mod, 3)
        a = script.w.build().upload(0)
        script.trees.append(a)
        for _ in script.stages():
            a.sync()
        a.sync()
        b = rt.Tree.points_gpu(3, *lvc.model(mc.plc.sparse64()), mc.PAL, view=st.views[1])
    elif st.name == "L4-terrain":
        a = rt.Tree.heightfield_gpu(4, mc.terrain_heights())
        b = rt.Tree.volume_gpu(4, np.array(st.dense[1]), mc.PAL, view=st.views[1])
    else:
        raw = (mc.plc.old64(), mc.plc.sparse64()) if st.levels == 3 else tuple(np.array(d) for d in st.dense)
        a, b = (rt.Tree.volume_gpu(st.levels, np.array(v), mc.PAL, view=view) for v, view in zip(raw, st.views))
    for t, pal, dense, view in zip((a, b), st.pals, st.dense, st.views):
        assert t.palette() == pal and t.info().view == view and t.garbage() == ppc.expected_garbage(t), st.name
        assert not content or np.array_equal(_stored(t), dense), "%s: the start tree does not hold the start model" % st.name
    return [a, b], script


def _run_step(rt, step, trees, prefab_trees):
    t = trees[step["tree"]]
    kind = step["kind"]
    if kind == "compact":
        return t.compact()
    if kind == "volume":
        return t.patch_volume(np.array(step["voxels"]), step["origin"])
    if kind == "points":
        return t.patch_points(np.array(step["xyz"]), np.array(step["ids"]))
    if kind == "shapes":
        return t.patch_shapes(spc.to_abi(rt, step["shapes"]))
    src = {"other": trees[1 - step["tree"]], "self": t}.get(step["src"]) or prefab_trees[step["src"]]
    so, n, do = step["src_origin"], step["dims"], step["dst_origin"]
    if kind == "paste":
        return t.patch_tree(src, so, n, do, keep_empty=step["keep_empty"])
    if kind == "oriented":
        return t.patch_tree_oriented(src, so, n, do, axis=step["axis"], flip=step["flip"], id_map=step["id_map"], keep_empty=step["keep_empty"])
    return t.patch_tree_rule(src, so, n, do, step["rule"], axis=step["axis"], flip=step["flip"], id_map=step["id_map"])


def _identity(t):
    """what must not move in a tree that is only read"""
    nodes, mats = t.export()
    i = t.info()
    return (nodes.tobytes(), mats.tobytes(), int(i.n_nodes), int(i.n_mat_bytes), int(i.n_bricks), [int(x) for x in i.nodes_per_level],
            int(i.device_bytes), t.garbage())


def _check_step(cuda, t, comp, step, seed, label):
    """(1) .. (4) on the tree the step changed"""
    E = comp.shape[0]
    got = _stored(t)
    assert np.array_equal(got, comp), "(1) %s: %d voxels differ" % (label, int((got != comp).sum()))
    assert t.garbage() == ppc.expected_garbage(t), "(2) %s" % label
    mask, kind, _ = _kinds(t)
    assert not ((kind == K_BRICK) & (mask == 0)).any(), "(2) %s: a K_BRICK record with mask 0" % label
    where = np.random.default_rng(1000 * seed + step["i"]).integers(0, E, (2000, 3))
    if step["box"] is not None:
        lo, hi = step["box"]
        corners = [(x, y, z) for x in (lo[0], hi[0] - 1) for y in (lo[1], hi[1] - 1) for z in (lo[2], hi[2] - 1)]
        where = np.concatenate([where, np.array(corners)])
    where = np.ascontiguousarray(where.astype(np.int32))
    want = comp[where[:, 2], where[:, 1], where[:, 0]]
    assert np.array_equal(t.get_blocks(where), want), "(3) %s: the host image" % label
    assert np.array_equal(t.get_blocks_gpu(where).cpu().numpy().view(np.uint16), want), "(3) %s: the device copy" % label
    dev, host = t.device_ceilings_fine(), t.ceilings_fine()
    assert (dev is None) == (host is None), "(4) %s" % label
    if dev is not None:
        assert np.array_equal(dev, host), "(4) %s: fine ceilings" % label
        lv, c, _ = t.device_ceilings()
        n = dev.shape[0] // 4
        assert lv >= 1 and np.array_equal(c[:n * n].reshape(n, n), dev.reshape(n, 4, n, 4).max(axis=(1, 3))), "(4) %s: 16-column ceilings" % label


def _upward_frame(rt, t, comp, solid):
    """a frame that looks upward from below the world's top row: a solid-view tree's cast, or (solid: the solid view of
    the same content) the shading pass that walks a full-view tree as its scene"""
    E = comp.shape[0]
    org = (E / 2 + 0.5, max(mc.top_row(comp) - 2, 0) + 0.5, E / 2 + 0.5)
    d = rt.normalize((0.3, 0.8, 0.45))
    if solid is None:
        return t.cast_frame(org, d, 64, 32, 300)
    colours, hits = solid.shade_frame(org, d, 64, 32, 300, scene=t, time=0.25, with_hits=True)
    return dict(hits, colours=colours)


def _same_frames(cuda, a, b, label):
    for k in ("pos_steps", "t", "info") + (("colours",) if "colours" in a else ()):
        assert cuda.equal(a[k], b[k]), "%s %s" % (label, k)


def _checkpoint(rt, cuda, t, comp, older, levels, tmp_path, label, group):
    """the full comparison with a fresh build of the model, in two groups that a test id runs both or one of: "fresh"
    (check_patched, the upward frame, the empty diff against the fresh tree) and "lists" (the counts and the listing, save
    and load, the diff from `older`, the previous checkpoint's model of this tree, and that older tree patched with it).
    Either group leaves t compacted."""
    pal, view = t.palette(), t.info().view
    comp = np.array(comp)
    solid = rt.Tree.volume_gpu(levels, vc.in_view(comp, pal, 0), pal, view=0) if view else None
    up = _upward_frame(rt, t, comp, solid)
    if "lists" in group:
        assert t.count_voxels() == int((comp != 0).sum()), "count_voxels, " + label
        xyz, ids = t.list_voxels()
        xyz, ids = xyz.cpu().numpy(), ids.cpu().numpy().view(np.uint16)
        wx, wi = lvc.model(comp)
        assert np.array_equal(xyz, wx) and np.array_equal(ids, wi), "list_voxels, " + label
        assert (np.diff(lvc.key_of(xyz, levels)) > 0).all(), "list_voxels' order, " + label
        path = str(tmp_path / "mixed.svo")
        t.save(path)
        u = rt.Tree.load(path).upload(0)
        (n0, m0), (n1, m1) = t.export(), u.export()
        assert n0.tobytes() == n1.tobytes() and m0.tobytes() == m1.tobytes(), "save / load, " + label
        _same_frames(cuda, up, _upward_frame(rt, u, comp, solid), "save / load, " + label)
        del u
    if "fresh" in group:
        fresh = check_patched(rt, cuda, t, comp, label, casts=levels > 2, shift=SHIFT[levels])      # (compacts t)
        _same_frames(cuda, up, _upward_frame(rt, fresh, comp, solid), "upward frame, " + label)
        assert t.count_diff(fresh) == 0 and len(t.diff_voxels(fresh)[1]) == 0, "diff against the fresh tree, " + label
        assert fresh.guard_trips() == 0, label
    else:
        t.compact()
    if "lists" in group:
        older = np.array(older)
        old = rt.Tree.volume_gpu(levels, older, pal, view=view)
        dx, di = old.diff_voxels(t)
        wx, wi = dvc.model(older, comp)
        assert np.array_equal(dx.cpu().numpy(), wx) and np.array_equal(di.cpu().numpy().view(np.uint16), wi), "diff_voxels, " + label
        old.patch_points(dx, di)
        old.compact()
        _same(old, t, "the older tree patched with the diff, " + label)
    assert t.guard_trips() == 0, label


@pytest.fixture(scope="module")
def sequences(rt, oracle_mod, prefabs):
    """{name: (Start, [(step, models)], expected_crossings)}: the numpy side of every run, computed once and left unchanged"""
    out = {}
    for name in mc.NAMES:
        st = mc.start(name, rt, oracle_mod)
        run = list(mc.Sequence(st, prefabs[0]).run())
        out[name] = (st, run, mc.expected_crossings(st, run))
    return out


# (name, first step checked, one past the last): the steps before the first are run unchecked.  The 64^3 runs are cut in two
# and the 256^3 run at its checkpoints, whose comparisons of 16.7 million voxels each cost what half a 64^3 run does.
CUTS = {"L2-volume": (0, 30), "L3-volume": (0, 50, 100), "L3-volume-swapped": (0, 50, 100), "L3-world": (0, 50, 100),
        "L4-terrain": (0, 13, 14, 23, 24, 29, 30)}
BOTH = ("fresh", "lists")
# (at 256^3 each id makes one of the checkpoint's two groups of comparisons, and the checks after every step go with "fresh":
# a window of steps is covered only by both of its ids, so select them together, never with -k lists or -k fresh alone)
PARTS = [(n, a, b, g) for n in mc.NAMES for a, b in zip(CUTS[n], CUTS[n][1:]) for g in ([(x,) for x in BOTH] if n == "L4-terrain" else [BOTH])]


def _kind_at(t, kinds, p):
    return int(t.node_indices([p])[0]), int(kinds[int(t.node_indices([p])[0])])


def _check_planted(t, st, step):
    """the planted cell of a 4-level A is one K_SOLID record at depth 1 (step None: at the start); after the points step
    aimed into it, the 16^3 cells without an edit are K_SOLID siblings, and so are the bricks without an edit beside
    edited ones: the synthesis at two levels"""
    lo, side = st.planted
    _, kinds, _ = _kinds(t)
    if step is None:
        a, b = _kind_at(t, kinds, lo), _kind_at(t, kinds, tuple(v + side - 1 for v in lo))
        assert a == b and a[1] == K_SOLID, "the planted cell is not one K_SOLID record: %s %s" % (a, b)
        return
    cells, bricks = mc.untouched(step["xyz"], lo, side)
    for group, width in ((cells, side // 4), (bricks, 4)):
        nodes = set()
        for c in group:
            a, b = _kind_at(t, kinds, c), _kind_at(t, kinds, tuple(v + width - 1 for v in c))
            assert a == b and a[1] == K_SOLID, "not a K_SOLID sibling at %s: %s %s" % (c, a, b)
            nodes.add(a[0])
        assert len(nodes) == len(group) >= 2


@pytest.mark.parametrize("name,first,last,group", PARTS, ids=["%s-steps%d-%d-%s" % (n, a, b - 1, "+".join(g)) for n, a, b, g in PARTS])
def test_mixed_sequence(rt, oracle_mod, cuda, prefabs, sequences, tmp_path, name, first, last, group):
    data, prefab_trees = prefabs
    st, run, crossings = sequences[name]
    trees, script = _start_trees(rt, oracle_mod, st, content=first == 0)
    frozen = {k: _identity(t) for k, t in prefab_trees.items()}
    checkpoint = list(st.dense)                      # per tree: the model at its last checkpoint
    grew = []
    if st.levels == 4:
        _check_planted(trees[0], st, None)
    for step, models in run[:last]:
        i, k = step["i"], step["tree"]
        label = "%s, seed %d, step %d: %s" % (name, st.seed, i, mc.describe(step))
        t = trees[k]
        at_checkpoint = step["kind"] == "compact" or i >= len(run) - 2
        src = {"other": trees[1 - k], "self": None}.get(step.get("src"), prefab_trees.get(step.get("src")))
        before = _identity(src) if src is not None and i >= first else None
        bytes_before = t.info().device_bytes
        assert _run_step(rt, step, trees, prefab_trees) is t, label
        if t.info().device_bytes > bytes_before and step["kind"] != "compact":
            grew.append((i, "AB"[k], step["kind"], "restart" if mc.is_restart(st, step) else "append"))
        if st.levels == 4 and i == 0:
            _check_planted(t, st, step)
        if at_checkpoint and i < first:
            checkpoint[k] = models[k]
        if i < first:
            continue
        if "fresh" in group:
            _check_step(cuda, t, models[k], step, st.seed, label)
        if before is not None:
            assert _identity(src) == before, "(5) the source changed: " + label
        if script is not None and i == 0:           # the world-built tree no longer follows its world
            held = _identity(t)
            script.w.put_block(1, 1, 1, 0, int(vc.colour(3)))
            with pytest.raises(rt.SvoError, match=r"svo_tree_update failed \(-4\)"):
                t.update(script.w, [(1, 1, 1)])
            dust = script._abs(script.base)           # the script's base world again, on the host world alone
            script.w.put_blocks(dust, np.zeros(len(dust), np.uint32), np.full(len(dust), int(vc.colour(3)), np.uint64), level=4)
            assert _identity(t) == held, "a replay on the host world changed the resident tree: " + label
            _check_step(cuda, t, models[k], step, st.seed, label + " (after the refused update)")
        if at_checkpoint:
            assert step["kind"] != "compact" or t.garbage() == (0, 0), label
            # (check_patched compacts t.  After a compact step that changes nothing; the only other checkpoints are the last
            # step of each tree, which nothing follows: an order that ends otherwise must not let a later step read that tree.)
            _checkpoint(rt, cuda, t, models[k], checkpoint[k], st.levels, tmp_path, label, group)
            checkpoint[k] = models[k]
    assert len(run) == 2 * len(st.order) == (100 if st.levels == 3 else 30) and 0 <= first < last <= len(run)
    print("%s: steps %d .. %d checked, %d run; device arrays regrown at %s" % (name, first, last - 1, last, grew))
    for tree, after, by, total, cap, appended in crossings:      # the regrowths the inputs promise really happened
        if by < last:
            inside = [g for g in grew if "AB".index(g[1]) == tree and after < g[0] <= by]
            assert inside, "tree %s: %d entries against %d by step %d, regrown at %s" % ("AB"[tree], total, cap, by, grew)
            assert not appended or all(g[3] == "append" for g in inside), (tree, after, by, grew)
    for t in trees:
        assert t.guard_trips() == 0
    for key, t in prefab_trees.items():
        assert _identity(t) == frozen[key], key
