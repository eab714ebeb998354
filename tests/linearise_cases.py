"""The worlds whose linearised trees tests/golden/linearised_digests.json pins, byte for byte: shared by
tests/test_linearise_host.py (which recomputes the digests with the tree's own library) and tools/record_linearised_digests.py
(which recorded them with the library of the commit named in the fixture).

A digest is the sha256 over a tree's exported node bytes, its material bytes, its palette tuples and
(n_nodes, n_bricks, nodes_per_level) of info(): the layout svo_build_view emits and svo_tree_update leaves, and the
statistics each of them fills or leaves alone."""
import hashlib

import edit_script as es

LEVELS = (3, 4, 6)
F_WATER = 0x14


def digest(tree):
    nodes, mats = tree.export()
    i = tree.info()
    h = hashlib.sha256()
    h.update(nodes.tobytes())
    h.update(b"|" + mats.tobytes())
    h.update(b"|" + repr([(int(f), int(c), float(m)) for f, c, m in tree.palette()]).encode())
    h.update(b"|" + repr((int(i.n_nodes), int(i.n_bricks), [int(x) for x in i.nodes_per_level])).encode())
    return h.hexdigest()


def _both_views(rt, name, world):
    for view in (rt.VIEW_SOLID, rt.VIEW_ALL):
        yield "%s/view%d" % (name, view), digest(world.build(view))


def static_cases(rt):
    """(name, digest) of fresh builds: the reference world and the degenerate ones"""
    yield from _both_views(rt, "reference", rt.World.reference())
    yield from _both_views(rt, "empty", rt.World(5))
    w = rt.World(5)
    w.put_block(0, 0, 0, 0, 7, level=1)
    yield from _both_views(rt, "root_leaf", w)
    w = rt.World(5)
    w.put_block(0, 0, 0, F_WATER, 7, level=1)  # nothing to the solid view, the whole world to the other
    yield from _both_views(rt, "root_leaf_water", w)
    w = rt.World(3)  # only 16^3 and 4^3 leaves: no voxel-level node anywhere
    for k, (x, y, z, lv) in enumerate([(0, 0, 0, 2), (16, 0, 0, 3), (20, 4, 8, 3), (48, 48, 48, 2), (32, 16, 0, 3), (63, 63, 63, 3)]):
        w.put_block(x, y, z, F_WATER if k == 2 else 0, 100 + k % 3, level=lv)
    yield from _both_views(rt, "coarse_leaves_3", w)
    w = rt.World(4)  # a 16^3 filled by 64 equal 4^3 puts: a fresh build collapses it to one SOLID record
    for k in range(4):
        for j in range(4):
            for i in range(4):
                w.put_block(64 + 4 * i, 16 + 4 * j, 32 + 4 * k, 0, 9, level=4)
    w.put_block(3, 2, 1, 0, 11)
    yield from _both_views(rt, "filled_16", w)


def script_cases(rt, oracle_mod, levels):
    """(name, digest) over the edit script at `levels`: before the first stage and after every one, each patched tree
    and a fresh build of the same world, in both views"""
    s = es.EditScript(rt, oracle_mod, levels)
    views = (rt.VIEW_SOLID, rt.VIEW_ALL)
    s.trees += [s.w.build(v) for v in views]
    for tree, view in zip(s.trees, views):
        yield "script%d/stage0/view%d/patched" % (levels, view), digest(tree)
    for stage in s.stages():
        for tree, view in zip(s.trees, views):
            yield "script%d/stage%d/view%d/patched" % (levels, stage, view), digest(tree)
            yield "script%d/stage%d/view%d/fresh" % (levels, stage, view), digest(s.w.build(view))
