"""The inputs of tests/test_gpu_mixed_ops.py, without a GPU: conditions on the sequences tests/mixed_ops_cases.py generates
and on their model, asserted so that the GPU test cannot pass by doing nothing.

Both trees run the whole order, so the succession of kinds on each tree holds every ordered pair of the seven kinds
once (compact after compact included); the generator is deterministic; every parameter set is one the ABI accepts; few
steps leave the model unchanged (at most 5 of the 86 patches of both trees at 3 levels, 2 of the 24 at 2
and 4 levels); the 3-level run shows a whole-extent step, a restart to one id, a step confined to one brick and one
confined to a uniform aligned 16^3, a step across the centre, the world's top row falling and rising, a self-paste of
overlapping boxes and a paste across views; neither tree stays empty or uniform; the listing model and the diff model
agree with the dense model after every step; before its first compact the 3-level run appends more material entries than
a fresh upload's slack holds; and the numpy side of a whole run takes seconds.

Seeds (mixed_ops_cases.SEEDS): 1 was tried first for every start and met every condition below; the start with the views
swapped takes 2 so that the two volume-built runs differ in their parameters as well.  No seed was rejected."""
import time

import numpy as np
import pytest

import diff_voxels_cases as dvc
import list_voxels_cases as lvc
import mixed_ops_cases as mc
import paste_oriented_cases as poc
import paste_rule_cases as prc
import points_patch_cases as ppc

NOOP_CAP = {3: 5, 2: 2, 4: 2}


@pytest.fixture(scope="module")
def prefabs(rt):
    return mc.prefab_volumes(rt)


@pytest.fixture(scope="module")
def runs(rt, oracle_mod, prefabs):
    """{name: (Start, [(step, models)], seconds of the numpy side)}, generated once and left unchanged"""
    out = {}
    for name in mc.NAMES:
        t0 = time.perf_counter()
        st = mc.start(name, rt, oracle_mod)
        t1 = time.perf_counter()
        out[name] = (st, list(mc.Sequence(st, prefabs).run()), time.perf_counter() - t1, t1 - t0)
    return out


def test_each_tree_sees_every_ordered_pair_once():
    o = mc.ORDER50
    assert len(o) == 50 and set(o) == set(mc.KINDS)
    every = {(a, b) for a in mc.KINDS for b in mc.KINDS}
    assert len(set(zip(o, o[1:]))) == 49 == len(every)
    assert len(mc.ORDER15) == 15 and all(mc.ORDER15.count(k) >= 2 for k in mc.KINDS)
    for order in (mc.ORDER50, mc.ORDER15):
        steps = mc.ops(order)
        assert len(steps) == 2 * len(order) and [t for _, t in steps] == [i % 2 for i in range(len(steps))]
        for tree in (0, 1):    # the succession ON THE TREE is the order: what a kind runs on is what the kind before it left there
            assert mc.successions(order, tree) == list(zip(order, order[1:]))
    for tree in (0, 1):
        pairs = mc.successions(mc.ORDER50, tree)
        assert len(pairs) == 49 and set(pairs) == every and ("compact", "compact") in pairs
        assert len(set(mc.successions(mc.ORDER15, tree))) == 14


@pytest.mark.parametrize("name", mc.NAMES)
def test_the_generator_is_deterministic(runs, rt, oracle_mod, prefabs, name):
    st, run, _, _ = runs[name]
    again = mc.steps_of(mc.start(name, rt, oracle_mod), prefabs)
    assert mc.same_steps([s for s, _ in run], again)
    assert [(s["kind"], s["tree"]) for s in again] == mc.ops(st.order) and [s["i"] for s in again] == list(range(2 * len(st.order)))
    for tree in (0, 1):
        assert [s["kind"] for s in again if s["tree"] == tree] == list(st.order)


def _src(st, prefabs, step):
    """(extent, palette size) of a paste's source"""
    if step["src"] in ("other", "self"):
        return 4 ** st.levels, len(st.pals[1 - step["tree"] if step["src"] == "other" else step["tree"]])
    return 4 ** prefabs[step["src"]][0], len(prefabs[step["src"]][1])


@pytest.mark.parametrize("name", mc.NAMES)
def test_every_parameter_set_is_one_the_abi_accepts(runs, prefabs, name):
    st, run, _, _ = runs[name]
    E = 4 ** st.levels
    for step, _ in run:
        kind, label = step["kind"], mc.describe(step)
        npal = len(st.pals[step["tree"]])
        if kind == "compact":
            continue
        lo, hi = step["box"]
        assert min(lo) >= 0 and max(hi) <= E and all(a < b for a, b in zip(lo, hi)), label
        if kind == "volume":
            v = step["voxels"]
            assert v.dtype == np.uint16 and v.ndim == 3 and min(v.shape) >= 1 and v.max() < npal, label
            assert step["variant"].startswith("whole") or (max(v.shape) <= 40 and all(o % 4 == a + 1 for a, o in enumerate(step["origin"]))
                                                           and all(n % 2 for n in v.shape)), label
        elif kind == "points":
            xyz, ids = step["xyz"], step["ids"]
            assert xyz.dtype == np.int32 and ids.dtype == np.uint16 and 1 <= len(ids) == len(xyz) <= 400, label
            assert xyz.min() >= 0 and xyz.max() < E and ids.max() < npal, label
        elif kind == "shapes":
            assert 1 <= len(step["shapes"]) <= 4 <= 1024, label
            for s in step["shapes"]:
                assert 0 <= s[3] < npal, label
                if s[0] == "box":
                    assert min(s[1]) >= 0 and min(s[2]) >= 1 and all(o + n <= E for o, n in zip(s[1], s[2])), label
                else:
                    assert max(abs(c) for c in s[1]) <= 1 << 20 and 0 <= s[2] <= 1 << 42, label
        else:
            sE, spal = _src(st, prefabs, step)
            so, n = step["src_origin"], step["dims"]
            assert min(so) >= 0 and min(n) >= 1 and all(o + m <= sE for o, m in zip(so, n)), label
            axis, flip, id_map = step.get("axis", (0, 1, 2)), step.get("flip", (0, 0, 0)), step.get("id_map")
            assert (tuple(axis), tuple(flip)) in poc.ORIENTATIONS, label
            assert tuple(h - l for l, h in zip(lo, hi)) == poc.dst_dims(n, axis) and lo == step["dst_origin"], label
            if id_map is None:
                assert spal <= npal, label            # the plain paste's rule
            else:
                assert len(id_map) == spal and id_map[0] == 0 and max(id_map) < npal, label
            if kind == "rule":
                assert step["rule"] in prc.RULES and step["rule"] != 0, label


@pytest.mark.parametrize("name", mc.NAMES)
def test_few_steps_leave_the_model_unchanged(runs, name):
    st, run, _, _ = runs[name]
    prev, same = list(st.dense), []
    for step, models in run:
        t = step["tree"]
        assert models[1 - t] is prev[1 - t], "step %d changed the other tree's model" % step["i"]
        if step["kind"] == "compact":
            assert models[t] is prev[t]
        elif np.array_equal(models[t], prev[t]):
            same.append(step["i"])
        prev = models
    patches = sum(k != "compact" for k, _ in mc.ops(st.order))
    assert patches == (86 if st.levels == 3 else 24) and len(same) <= NOOP_CAP[st.levels], same   # (the caps of a 50- and a 15-step run, kept)


def _features(st, run):
    E, seen = 4 ** st.levels, {}
    prev = list(st.dense)
    for step, models in run:
        t = step["tree"]
        before, after = prev[t], models[t]
        prev = models
        if step["kind"] == "compact":
            continue
        lo, hi = step["box"]
        found = set()
        if (lo, hi) == ((0, 0, 0), (E, E, E)):
            found.add("whole extent")
            if after.min() == after.max() != 0:
                found.add("restart to one id")
        if all(a // 4 == (b - 1) // 4 for a, b in zip(lo, hi)):
            found.add("one brick")
        if all(a // 16 == (b - 1) // 16 for a, b in zip(lo, hi)):
            c = [a // 16 * 16 for a in lo]
            cell = before[c[2]:c[2] + 16, c[1]:c[1] + 16, c[0]:c[0] + 16]
            if cell.min() == cell.max() != 0 and not np.array_equal(before, after):
                found.add("inside a uniform aligned 16^3")
        if all(a < E // 2 < b for a, b in zip(lo, hi)):
            found.add("across the centre")
        if mc.top_row(after) < mc.top_row(before):
            found.add("top row falls")
        if mc.top_row(after) > mc.top_row(before):
            found.add("top row rises")
        if step["kind"] in mc.PASTES:
            so, n = step["src_origin"], step["dims"]
            if step["src"] == "self" and all(max(a, s) < min(b, s + m) for a, b, s, m in zip(lo, hi, so, n)):
                found.add("self-paste, overlapping")
            if step["src"] == "other" and st.views[0] != st.views[1]:
                found.add("paste across views")
        for f in found:
            seen.setdefault(f, []).append(step["i"])
    return seen


@pytest.mark.parametrize("name", [n for n in mc.NAMES if n.startswith("L3")])
def test_the_3_level_run_shows_every_situation(runs, name):
    st, run, _, _ = runs[name]
    seen = _features(st, run)
    want = {"whole extent", "restart to one id", "one brick", "inside a uniform aligned 16^3", "across the centre", "top row falls",
            "top row rises", "self-paste, overlapping", "paste across views"}
    assert want <= set(seen), sorted(want - set(seen))
    shapes = [s for step, _ in run if step["kind"] == "shapes" for s in step["shapes"]]
    assert any(s[3] == 0 for s in shapes) and any(s[0] == "ball" and not all(0 <= c < 64 for c in s[1]) for s in shapes)
    vols = [step for step, _ in run if step["kind"] == "volume"]
    assert any(not v["voxels"].any() for v in vols)
    pts = [step for step, _ in run if step["kind"] == "points"]
    assert any(len(np.unique(p["xyz"], axis=0)) < len(p["xyz"]) for p in pts) and any((p["ids"] == 0).any() for p in pts)
    pastes = [step for step, _ in run if step["kind"] in mc.PASTES]
    assert {p["src"] for p in pastes} == set(mc.SOURCES)
    assert {True, False} == {p["keep_empty"] for p in pastes if "keep_empty" in p}
    for cls, ok in (("m16", lambda d: d % 16 == 0), ("m4", lambda d: d % 4 == 0 and d % 16 != 0), ("odd", lambda d: d % 2 == 1)):
        assert any(all(ok(d - s) for d, s in zip(p["dst_origin"], p["src_origin"])) for p in pastes), cls


@pytest.mark.parametrize("name", [n for n in mc.NAMES if not n.startswith("L3")])
def test_the_short_runs_cut_the_planted_cell_and_cross_the_boundaries(runs, name):
    st, run, _, _ = runs[name]
    E, cs = 4 ** st.levels, 4 ** st.levels // 4
    crossing = [s["i"] for s, _ in run if s["box"] and any(a // cs != (b - 1) // cs for a, b in zip(*s["box"]))]
    centre = [s["i"] for s, _ in run if s["box"] and all(a < E // 2 < b for a, b in zip(*s["box"]))]
    assert len(crossing) >= 6 and centre, (crossing, centre)
    if st.planted:   # a points step, a shapes step and a paste cut the planted cell in turn
        lo, side = st.planted
        x, y, z = lo
        cut, prev = [], st.dense[0]
        for s, m in run:
            if s["tree"] == 0 and not np.array_equal(m[0][z:z + side, y:y + side, x:x + side], prev[z:z + side, y:y + side, x:x + side]):
                cut.append(s["kind"])
            prev = m[0] if s["tree"] == 0 else prev
        first = [cut.index(k) for k in ("points", "shapes", "paste")]
        assert cut[0] == "points" and first == sorted(first), cut
        # the points step leaves whole 16^3 cells and whole bricks of the cell alone: K_SOLID siblings at two levels
        cells, bricks = mc.untouched(run[0][0]["xyz"], lo, side)
        assert run[0][0]["kind"] == "points" and len(cells) >= 2 and len(bricks) >= 2


@pytest.mark.parametrize("name", mc.NAMES)
def test_neither_tree_stays_empty_or_uniform(runs, name):
    st, run, _, _ = runs[name]
    streak = [0, 0]
    for step, models in run:
        for t in (0, 1):
            streak[t] = streak[t] + 1 if models[t].min() == models[t].max() else 0
            assert streak[t] <= 2, "tree %d uniform for %d steps at step %d" % (t, streak[t], step["i"])


@pytest.mark.parametrize("name", mc.NAMES)
def test_the_listing_and_the_diff_models_agree_with_the_dense_model(runs, name):
    st, run, _, _ = runs[name]
    prev = list(st.dense)
    everything = np.ones(65536, bool)
    for step, models in run:
        t = step["tree"]
        comp = models[t]
        if comp is not prev[t]:
            xyz, ids = lvc.model(comp)
            back = np.zeros_like(comp)
            back[xyz[:, 2], xyz[:, 1], xyz[:, 0]] = ids
            assert np.array_equal(back, comp), step["i"]
            key = lvc.key_of(xyz, st.levels)
            assert (np.diff(key) > 0).all(), step["i"]
            dx, di = dvc.model(prev[t], comp)
            assert np.array_equal(ppc.apply_edits(prev[t], dx, di, everything), comp), step["i"]
        prev = models


@pytest.mark.parametrize("name", [n for n in mc.NAMES if n.startswith("L3")])
def test_one_tree_crosses_the_capacity_of_its_upload_before_the_first_compact(runs, prefabs, name):
    st, run, _, _ = runs[name]
    found = mc.expected_crossings(st, run)
    first_compact = [min(s["i"] for s, _ in run if s["kind"] == "compact" and s["tree"] == t) for t in (0, 1)]
    assert any(after == -1 and by < first_compact[tree] for tree, after, by, _, _, _ in found), "no tree passes the capacity of its upload"
    assert any(appended for _, _, _, _, _, appended in found), "no regrowth that keeps a prefix"
    for tree, after, by, total, cap, _ in found:
        assert total > cap and after < by and by % 2 == tree
    # (the node records cannot: 64^3 holds 4161 of them, the slack 65536)
    assert mc.mixed_material_entries(np.zeros((64, 64, 64), np.uint16)) == 0
    assert mc.mixed_material_entries(mc.plc.old64()[16:32, 16:32, 16:32]) > 0


@pytest.mark.parametrize("name", mc.NAMES)
def test_the_numpy_side_takes_seconds(runs, name):
    _, _, seconds, start_seconds = runs[name]
    print("%s: start %.2f s, sequence and model %.2f s" % (name, start_seconds, seconds))
    assert seconds + start_seconds < 8.0    # (measured: 0.02 s at 16^3, 0.2 to 0.4 s at 64^3, 2.4 to 3.9 s at 256^3)
