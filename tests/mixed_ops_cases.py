"""Mixed sequences of every device-side tree edit, and their model: the numpy side of tests/test_mixed_ops_host.py (the
conditions on the inputs) and tests/test_gpu_mixed_ops.py (the resident trees against the model, step by step).

Seven kinds: volume (svo_tree_patch_volume_gpu), points (svo_tree_patch_points_gpu), shapes (svo_tree_patch_shapes_gpu),
paste (svo_tree_patch_tree_gpu), oriented (svo_tree_patch_tree_oriented_gpu), rule (svo_tree_patch_tree_rule_gpu) and
compact (svo_tree_compact_gpu).  The order of the kinds is not drawn: ORDER50 is a de Bruijn sequence B(7, 2) unrolled,
50 kinds whose 49 consecutive pairs are the 49 ordered pairs of kinds, each once; ORDER15 (the 16^3 and 256^3 runs) holds
every kind at least twice.  Both trees run the whole order, tree A at the even steps and tree B at the odd ones (100 and
30 steps), so each tree sees every kind on what every kind left on that same tree; B's variants and sources are shifted
against A's so that the two differ.  A paste reads the other tree, the patched tree itself (overlapping boxes), or one of
two static prefabs (16^3 and 4^3).  Only the parameters of a step are drawn, from
numpy.random.default_rng(seed), and the generator looks at the model's current content so that it can aim: into a
uniform aligned cell, across the cell boundaries and the centre, at the world's top row.

The model is one dense uint16 volume per tree, holding what the tree stores in its own view, and every step applies the
existing model of its kind (points_patch_cases.apply_edits, shapes_patch_cases.apply_shapes, paste_tree_cases.apply_paste,
paste_oriented_cases.apply_oriented, paste_rule_cases.apply_rule, slicing for a volume): no operation is modelled anew.
Coordinates are (x, y, z); volumes are indexed [z, y, x]."""
import collections

import numpy as np

import paste_oriented_cases as poc
import paste_rule_cases as prc
import paste_tree_cases as ptc
import patch_layout_cases as plc
import points_patch_cases as ppc
import shapes_patch_cases as spc
import volume_cases as vc

KINDS = ("volume", "points", "shapes", "paste", "oriented", "rule", "compact")
PASTES = ("paste", "oriented", "rule")
PAL = plc.PAL                      # test_gpu_volume_patch's: ids 1 to 5, 5 liquid
ID_MAP = [0, 3, 0, 1, 5, 2]        # patch_layout_cases' map, over PAL
SOURCES = ("other", "self", "prefab2", "prefab1")
OFFSETS = ("m16", "m4", "odd")     # dst_origin - src_origin: multiples of 16, multiples of 4 only, odd


def de_bruijn_pairs(k):
    """B(k, 2) as the concatenation of the Lyndon words of length 1 and 2 over k symbols, unrolled by its first symbol:
    k * k + 1 symbols whose consecutive pairs are all the ordered pairs, each once"""
    seq = []
    for a in range(k):
        seq.append(a)
        for b in range(a + 1, k):
            seq += [a, b]
    return seq + seq[:1]


ORDER50 = tuple(KINDS[s] for s in de_bruijn_pairs(7))


def ops(order):
    """the steps of a run, (kind, tree): each tree runs the whole order, A at the even steps and B at the odd ones, so that
    the succession of kinds ON EACH TREE is the order itself.  (Alternating the trees along the order instead would hand
    each tree every second kind, and a kind would run on what the kind two places before it left: 17 of the 49 pairs.)"""
    return [(kind, tree) for kind in order for tree in (0, 1)]


def successions(order, tree):
    """the (previous kind on this tree, kind) pairs a run of `order` shows on `tree`"""
    mine = [k for k, t in ops(order) if t == tree]
    return list(zip(mine, mine[1:]))


ORDER15 = ("points", "volume", "shapes", "points", "paste", "rule", "compact", "oriented", "shapes", "volume", "oriented",
           "compact", "rule", "paste", "compact")

# what the k-th step of a kind does (cycled), per order
VARIANTS = {
    50: {"volume": ("box", "zeros", "whole_random", "centre", "whole_one_id", "whole_random", "straddle", "box"),
         "points": ("uniform_cell", "random", "brick", "random_aimed", "uniform_cell", "random", "random_aimed"),
         "shapes": ("cut_cell", "lower_top", "random", "raise_top", "random", "cut_cell", "random")},
    15: {"volume": ("centre", "straddle"),
         "points": ("uniform_cell", "random_aimed"),
         "shapes": ("cut_cell", "raise_top")},
}

Start = collections.namedtuple("Start", "name levels order seed views pals dense planted")
# views, pals, dense: one per tree (A, B); dense: what the tree stores, in its own view; planted: (lo, side) of a uniform
# aligned cell of A the aimed steps fall back on once it is cut, or None


def _ro(a):
    a = np.ascontiguousarray(a, np.uint16)
    a.setflags(write=False)
    return a


# --------------------------------------------------------------------------------------------------- start contents --
def world_start(rt, oracle_mod):
    """(the EditScript, its host tree after the last stage, the tree's content in its palette's ids): 3 levels"""
    import edit_script

    s = edit_script.EditScript(rt, oracle_mod, 3)
    tree = s.w.build()
    s.trees.append(tree)
    for _ in s.stages():
        pass
    return s, tree, tree.get_blocks(s.box_points()).reshape(64, 64, 64).astype(np.uint16)


def terrain_heights():
    """256 x 256 columns: hills of rows 2 .. 16 and a plateau of row 140 over the aligned 64 x 64 columns at (64, 64), whose
    rows 64 .. 127 are one material (row 0 is empty in every column): a K_SOLID 64^3 at depth 1"""
    x, z = np.meshgrid(np.arange(256), np.arange(256), indexing="ij")
    h = (9 + 4 * np.sin(x / 9.0) + 3 * np.cos(z / 7.0)).astype(np.int32)
    h[64:128, 64:128] = 140
    return h


def terrain_start(rt):
    """(host tree of terrain_heights(), its content over the whole extent in its palette's ids): the host tree looked up
    at every voxel up to its column's top and the row above it; nothing is stored higher in the solid view"""
    h = terrain_heights()
    t = rt.Tree.heightfield(4, h)
    rows = (h + 2).ravel()                                              # [x * 256 + z]
    col = np.repeat(np.arange(256 * 256), rows)
    y = np.arange(len(col)) - np.repeat(np.cumsum(rows) - rows, rows)
    x, z = col // 256, col % 256
    dense = np.zeros((256, 256, 256), np.uint16)
    dense[z, y, x] = t.get_blocks(np.stack([x, y, z], 1).astype(np.int32))
    assert top_row(dense) == int(h.max())
    return t, dense


def prefab_volumes(rt):
    """{name: (levels, palette, what the prefab stores in its view (1), the volume it is built from)}: the static sources.
    The 4^3 prefab is a tree of one level, which only the host builder makes (vc.host_twin numbers its materials)."""
    v2 = vc.random_volume((16, 16, 16), 0.5, 23)
    v2[4:8, 8:12, 0:4] = 2                             # a SOLID child of the root
    v2[8:12, 0:4, 12:16] = 0                           # an absent one
    v1 = np.zeros((4, 4, 4), np.uint16)
    v1[0:2, :, :] = 1
    v1[2, 1:3, 0:3] = 2
    v1[3, 3, 3] = 5
    _, pal1, dense1 = vc.host_twin(rt, 1, v1, (0, 0, 0), 1)
    return {"prefab2": (2, PAL, _ro(vc.in_view(v2, PAL, 1)), v2), "prefab1": (1, pal1, _ro(vc.in_view(dense1, pal1, 1)), v1)}


# The seeds: 1 was tried first for every start and kept where the input conditions of tests/test_mixed_ops_host.py held.
SEEDS = {"L3-volume": 1, "L3-volume-swapped": 2, "L3-world": 1, "L4-terrain": 1, "L2-volume": 1}
NAMES = tuple(sorted(SEEDS))


def start(name, rt=None, oracle_mod=None):
    """the Start of a configuration; L3-world and L4-terrain need the library's host builders (rt, oracle_mod)"""
    seed = SEEDS[name]
    if name in ("L3-volume", "L3-volume-swapped"):
        views = (0, 1) if name == "L3-volume" else (1, 0)
        dense = (vc.in_view(plc.old64(), PAL, views[0]), vc.in_view(plc.sparse64(), PAL, views[1]))
        return Start(name, 3, ORDER50, seed, views, (PAL, PAL), tuple(_ro(d) for d in dense), ((0, 0, 0), 16))
    if name == "L3-world":
        _, tree, dense = world_start(rt, oracle_mod)
        return Start(name, 3, ORDER50, seed, (0, 1), (tree.palette(), PAL), (_ro(dense), _ro(vc.in_view(plc.sparse64(), PAL, 1))), None)
    if name == "L4-terrain":
        tree, dense = terrain_start(rt)
        b = np.zeros((256, 256, 256), np.uint16)
        b[90:150, 10:60, 100:160] = vc.random_volume((60, 50, 60), 0.3, 31)
        b[0:64, 0:64, 192:256] = 2
        b[130:140, 70:75, 120:136] = 5
        assert (dense[64:128, 64:128, 64:128] == dense[64, 64, 64]).all() and dense[64, 64, 64] != 0
        return Start(name, 4, ORDER15, seed, (0, 1), (tree.palette(), PAL), (_ro(dense), _ro(b)), ((64, 64, 64), 64))
    if name == "L2-volume":
        b = vc.random_volume((16, 16, 16), 0.3, 1)
        b[4:8, 8:12, 0:4] = 2
        b[8:12, 0:4, 12:16] = 0
        dense = (vc.in_view(plc.old64()[16:32, 16:32, 16:32], PAL, 0), vc.in_view(b, PAL, 1))
        return Start(name, 2, ORDER15, seed, (0, 1), (PAL, PAL), tuple(_ro(d) for d in dense), None)
    raise ValueError(name)


# --------------------------------------------------------------------------------------------------------- helpers --
def top_row(vol):
    """the highest row that holds a voxel, -1 for an empty volume"""
    rows = np.nonzero(vol.any(axis=(0, 2)))[0]
    return int(rows[-1]) if len(rows) else -1


def uniform_cells(vol, side):
    """[(lo (x, y, z), id)] of the aligned cells of side^3 voxels that hold one id throughout, in z, y, x order"""
    n = vol.shape[0] // side
    c = vol.reshape(n, side, n, side, n, side)
    lo, hi = c.min(axis=(1, 3, 5)), c.max(axis=(1, 3, 5))
    z, y, x = np.nonzero(lo == hi)
    return [((int(a) * side, int(b) * side, int(d) * side), int(lo[d, b, a])) for a, b, d in zip(x, y, z)]


def mixed_material_entries(vol, lo=None, hi=None):
    """the material entries a tree holds for `vol`: the stored voxels of its bricks of two materials or more (a brick of
    one material has no run).  lo, hi (x, y, z): only the bricks wholly inside that box."""
    if lo is not None:
        a = [-(-int(v) // 4) * 4 for v in lo]
        b = [int(v) // 4 * 4 for v in hi]
        if min(q - p for p, q in zip(a, b)) <= 0:
            return 0
        vol = vol[a[2]:b[2], a[1]:b[1], a[0]:b[0]]
    nz, ny, nx = (s // 4 for s in vol.shape)
    c = vol.reshape(nz, 4, ny, 4, nx, 4).transpose(0, 2, 4, 1, 3, 5).reshape(-1, 64)
    big = c.max(1)
    small = np.where(c == 0, np.uint16(65535), c).min(1)
    return int((c != 0).sum(1)[(big != small) & (big != 0)].sum())


def untouched(xyz, lo, side):
    """of the aligned cell of side^3 voxels at lo that a points list was aimed into: (the low corners of those of its 64
    sub-cells that hold no edit, the low corners of the bricks without an edit inside sub-cells that do hold one)"""
    sub = side // 4
    p = np.asarray(xyz, np.int64) - np.asarray(lo)
    p = p[((p >= 0) & (p < side)).all(1)]
    hit = {tuple(c) for c in (p // sub).tolist()}
    hit_bricks = {tuple(c) for c in (p // 4).tolist()}
    cells = [tuple(int(l + sub * c) for l, c in zip(lo, (a, b, d))) for a in range(4) for b in range(4) for d in range(4) if (a, b, d) not in hit]
    n = sub // 4
    bricks = [tuple(int(l + sub * c + 4 * e) for l, c, e in zip(lo, cell, (a, b, d))) for cell in sorted(hit) for a in range(n) for b in range(n)
              for d in range(n) if tuple(c * n + e for c, e in zip(cell, (a, b, d))) not in hit_bricks]
    return cells, bricks


def describe(step):
    """a step's parameters as text, arrays by their shape and first rows: with the start's name and seed, what a failure
    message needs for the sequence to be replayed up to the step"""
    out = []
    for k, v in step.items():
        if isinstance(v, np.ndarray):
            v = "array%s %s.." % (v.shape, v.reshape(-1)[:6].tolist())
        out.append("%s=%s" % (k, v))
    return ", ".join(out)


def same_steps(a, b):
    if len(a) != len(b):
        return False
    for s, t in zip(a, b):
        if s.keys() != t.keys():
            return False
        for k in s:
            if isinstance(s[k], np.ndarray):
                if not (isinstance(t[k], np.ndarray) and s[k].dtype == t[k].dtype and np.array_equal(s[k], t[k])):
                    return False
            elif s[k] != t[k]:
                return False
    return True


# ------------------------------------------------------------------------------------------------------- generator --
class Sequence:
    """run() yields (step, models): the step's parameters (a dict) and the two models after it (arrays never written
    again).  A step holds i, kind, tree (0: A, 1: B), variant, box = (lo, hi) of the voxels it may change (None: compact)
    and the arguments of its call."""

    def __init__(self, st, prefabs):
        self.st, self.prefabs = st, prefabs
        self.E = 4 ** st.levels
        self.cs = self.E // 4                       # a child cell of the root
        self.keep = [ppc.view_keep(p, v) for p, v in zip(st.pals, st.views)]
        self.variants = VARIANTS[len(st.order)]

    # -- geometry
    def _sizes(self, rng, most):
        """three odd sizes, 1 .. most"""
        most = min(most, self.E - 3)
        return [int(2 * rng.integers(0, (most + 1) // 2) + 1) for _ in range(3)]

    def _origin(self, rng, size, axis, across=None):
        """an origin of residue axis + 1 mod 4 that keeps [origin, origin + size) inside the extent; across: a coordinate
        the interval must hold together with the one before it, where that is possible"""
        r = axis + 1
        all_ = [o for o in range(r, self.E - size + 1, 4)]
        if across is not None:
            hit = [o for o in all_ if o < across < o + size]
            all_ = hit or all_
        return int(all_[rng.integers(0, len(all_))])

    def _box(self, rng, most, mode):
        size = self._sizes(rng, most)
        if mode == "centre":
            size = [max(s, 5) for s in size]
            cross = [self.E // 2] * 3
        elif mode == "straddle":
            size = [max(s, 5) for s in size]
            cross = [int(self.cs * rng.integers(1, 4)) for _ in range(3)]
        else:
            cross = [None] * 3
        return tuple(self._origin(rng, size[a], a, cross[a]) for a in range(3)), tuple(size)

    def _cell(self, rng, model, tree):
        """(lo, id) of a uniform aligned child cell of the root to aim at: one of a material if the model holds one, else
        the planted cell of A (by now cut), else an empty one, else None"""
        cells = uniform_cells(model, self.cs)
        full = [c for c in cells if c[1] != 0]
        if full:
            return full[int(rng.integers(0, len(full)))]
        if tree == 0 and self.st.planted is not None:
            lo = self.st.planted[0]
            return lo, int(model[lo[2], lo[1], lo[0]])
        return cells[int(rng.integers(0, len(cells)))] if cells else None

    def _ids(self, rng, n, tree, zeros=0.3):
        top = min(len(self.st.pals[tree]), 6)
        ids = rng.integers(1, top, n).astype(np.uint16)
        ids[rng.random(n) < zeros] = 0
        return ids

    # -- the kinds
    def _volume(self, rng, variant, model, tree):
        E = self.E
        if variant.startswith("whole"):
            vox = vc.random_volume((E, E, E), 0.5, int(rng.integers(1 << 30))) if variant == "whole_random" else \
                np.full((E, E, E), int(rng.integers(1, 5)), np.uint16)
            origin = (0, 0, 0)
        else:
            origin, (nx, ny, nz) = self._box(rng, 39, variant)
            vox = np.zeros((nz, ny, nx), np.uint16) if variant == "zeros" else vc.random_volume((nz, ny, nx), 0.5, int(rng.integers(1 << 30)))
        vox = np.where(vox < len(self.st.pals[tree]), vox, 1).astype(np.uint16)
        return dict(voxels=np.ascontiguousarray(vox), origin=origin), (origin, tuple(o + n for o, n in zip(origin, vox.shape[::-1])))

    def _points(self, rng, variant, model, tree):
        E = self.E
        n = int(rng.integers(1, 401))
        lo, side = (0, 0, 0), E
        if variant in ("uniform_cell", "random_aimed"):
            cell = self._cell(rng, model, tree)
            if cell is not None:
                lo, side = cell[0], self.cs
        elif variant == "brick":
            lo, side, n = tuple(int(4 * v) for v in rng.integers(0, E // 4, 3)), 4, int(rng.integers(1, 65))
        pool = np.asarray(lo) + rng.integers(0, side, (n // 2 + 1, 3))
        if variant == "random_aimed":
            pool[::2] = rng.integers(0, E, (len(pool[::2]), 3))
        xyz = np.ascontiguousarray(pool[rng.integers(0, len(pool), n)].astype(np.int32))       # duplicates
        ids = self._ids(rng, n, tree)
        return dict(xyz=xyz, ids=ids), (tuple(int(v) for v in xyz.min(0)), tuple(int(v) + 1 for v in xyz.max(0)))

    def _shapes(self, rng, variant, model, tree):
        E, cs = self.E, self.cs
        top = min(len(self.st.pals[tree]), 6)
        shapes = []
        cell = self._cell(rng, model, tree) if variant == "cut_cell" else None
        t = top_row(model)
        if cell is not None:
            lo, ident = cell
            other = 1 + ident % (top - 1)
            o = tuple(min(v + cs // 2 + 1, E - 1) for v in lo)
            shapes.append(("box", o, tuple(min(cs - 1, E - v) for v in o), other))
            shapes.append(("ball", tuple(int(v) for v in lo), (cs // 3) ** 2 + 1, 0))
        elif variant == "lower_top" and t >= 4:
            shapes.append(("box", (0, t - 3, 0), (E, E - (t - 3), E), 0))
        elif variant == "raise_top":
            o, d = self._box(rng, 39, "box")
            shapes.append(("box", (o[0], E - 3, o[2]), (d[0], 3, d[2]), int(rng.integers(1, min(top, 5)))))
            shapes.append(("ball", (-5, E // 2, E + 3), int((E // 4 + 6) ** 2), int(rng.integers(0, top))))   # a centre outside
        count = int(rng.integers(1, 5))
        while len(shapes) < count:
            ident = 0 if len(shapes) == 1 else int(rng.integers(0, top))
            if rng.random() < 0.5:
                o, d = self._box(rng, 39, "straddle" if rng.random() < 0.5 else "box")
                shapes.append(("box", o, d, ident))
            else:
                shapes.append(("ball", tuple(int(v) for v in rng.integers(0, E, 3)), int(rng.integers(0, (E // 4) ** 2 + 1)), ident))
        lo, hi = [E] * 3, [0] * 3
        for s in shapes:
            where, m = spc.mask(s, E)
            if m.any():
                for a in range(3):
                    lo[a], hi[a] = min(lo[a], where[2 - a].start), max(hi[a], where[2 - a].stop)
        return dict(shapes=shapes), (tuple(lo), tuple(hi))

    def _paste(self, rng, kind, occ, models, tree):
        E = self.E
        pals = self.st.pals
        mapped = kind != "paste" and occ % 2 == (1 if kind == "oriented" else 0)
        first = (occ + PASTES.index(kind) + 2 * tree) % 4
        for name in SOURCES[first:] + SOURCES[:first]:
            src_pal = {"other": pals[1 - tree], "self": pals[tree]}.get(name) or self.prefabs[name][1]
            if name == "self" and models[tree].min() == models[tree].max():
                continue                                # (a uniform tree pasted into itself stays what it is)
            if name == "self" or mapped or len(src_pal) <= len(pals[tree]):
                break
        need_map = kind != "paste" and (mapped or len(src_pal) > len(pals[tree]))
        id_map = None
        if need_map:
            id_map = [m if m < len(pals[tree]) else 1 for m in ID_MAP][:len(src_pal)]
            id_map += [1 + i % (min(len(pals[tree]), 6) - 1) for i in range(len(id_map), len(src_pal))]
        sE = {"other": 4 ** self.st.levels, "self": E}.get(name) or 4 ** self.prefabs[name][0]
        most = min(sE, E)
        n = [int(rng.integers(max(1, most // 3), most + 1)) for _ in range(3)]
        src = models[1 - tree] if name == "other" else models[tree] if name == "self" else self.prefabs[name][2]
        axis, flip = poc.ORIENTATIONS[int(rng.integers(0, 48))] if kind != "paste" else poc.IDENTITY
        dn = poc.dst_dims(n, axis)
        cls = OFFSETS[(occ + tree) % 3]
        cell = self._cell(rng, models[tree], tree) if occ == 0 else None
        stored = np.flatnonzero(src)
        if name == "self" and cell is not None:         # around the cell's low corner, where the destination box starts
            so = [int(np.clip(cell[0][a] - n[a] // 2, 0, sE - n[a])) for a in range(3)]
        elif len(stored):                               # a box that holds a stored voxel
            at = np.unravel_index(int(stored[rng.integers(0, len(stored))]), src.shape)[::-1]
            so = [int(np.clip(at[a] - rng.integers(0, n[a]), 0, sE - n[a])) for a in range(3)]
        else:
            so = [int(rng.integers(0, sE - n[a] + 1)) for a in range(3)]
        do = []
        for a in range(3):
            cand = list(range(0, E - dn[a] + 1))
            filters = [{"m16": lambda d: (d - so[a]) % 16 == 0, "m4": lambda d: (d - so[a]) % 4 == 0 and (d - so[a]) % 16 != 0,
                        "odd": lambda d: (d - so[a]) % 2 == 1}[cls]]
            if name == "self":                          # the boxes overlap
                filters.insert(0, lambda d: abs(d - so[a]) < min(n[a], dn[a]))
            if cell is not None:                        # the box starts inside the cell: it cuts it
                filters.insert(0, lambda d: cell[0][a] < d < cell[0][a] + self.cs - 1)
            for f in filters:                           # (each where the ones before leave it a choice)
                cand = [d for d in cand if f(d)] or cand
            do.append(int(cand[rng.integers(0, len(cand))]))
        p = dict(src=name, src_origin=tuple(so), dims=tuple(n), dst_origin=tuple(do))
        if kind == "paste":
            p["keep_empty"] = bool(occ % 2)
        else:
            p.update(axis=tuple(axis), flip=tuple(flip), id_map=id_map)
            if kind == "oriented":
                p["keep_empty"] = bool((occ // 2) % 2)
            else:
                p["rule"] = prc.RULES[1 + (5 * occ) % 11]      # (rule 0 keeps everything)
        return p, (tuple(do), tuple(d + m for d, m in zip(do, dn)))

    def source_dense(self, step, models):
        """what the source of a paste stores, in its own view, as the call finds it"""
        if step["src"] in ("other", "self"):
            return models[1 - step["tree"]] if step["src"] == "other" else models[step["tree"]]
        return self.prefabs[step["src"]][2]

    def apply(self, step, models):
        """the patched tree's model after the step"""
        kind, tree = step["kind"], step["tree"]
        model, keep = models[tree], self.keep[tree]
        if kind == "compact":
            return model
        if kind == "volume":
            (x, y, z), vox = step["origin"], step["voxels"]
            out = np.array(model, np.uint16)
            out[z:z + vox.shape[0], y:y + vox.shape[1], x:x + vox.shape[2]] = np.where(keep[vox], vox, 0)
            return out
        if kind == "points":
            return ppc.apply_edits(model, step["xyz"], step["ids"], keep)
        if kind == "shapes":
            return spc.apply_shapes(model, step["shapes"], keep)
        src = self.source_dense(step, models)
        so, n, do = step["src_origin"], step["dims"], step["dst_origin"]
        if kind == "paste":
            return ptc.apply_paste(model, src, so, n, do, step["keep_empty"], keep)
        if kind == "oriented":
            return poc.apply_oriented(model, src, so, n, do, step["axis"], step["flip"], step["id_map"], step["keep_empty"], keep)
        return prc.apply_rule(model, src, so, n, do, step["axis"], step["flip"], step["id_map"], step["rule"], keep)

    def run(self):
        rng = np.random.default_rng(self.st.seed)
        models = list(self.st.dense)
        seen = collections.Counter()
        for i, (kind, tree) in enumerate(ops(self.st.order)):
            occ = seen[kind, tree]                  # per tree; B's cycles start three variants on, so that the trees differ
            seen[kind, tree] += 1
            step = dict(i=i, kind=kind, tree=tree)
            if kind == "compact":
                step.update(variant="", box=None)
            elif kind in PASTES:
                p, box = self._paste(rng, kind, occ, models, tree)
                step.update(variant="%s/%s" % (p["src"], OFFSETS[(occ + tree) % 3]), box=box, **p)
            else:
                variant = self.variants[kind][(occ + 3 * tree) % len(self.variants[kind])]
                p, box = getattr(self, "_" + kind)(rng, variant, models[tree], tree)
                step.update(variant=variant, box=box, **p)
            out = _ro(self.apply(step, models))
            models = [out if t == tree else m for t, m in enumerate(models)]
            yield step, models


def steps_of(st, prefabs):
    return [s for s, _ in Sequence(st, prefabs).run()]


def appended_entries(before, after):
    """a lower bound of the material entries a patch appends that makes `before` into `after`: a brick whose content
    changed is emitted again, and one of two materials or more brings its run along"""
    nz, ny, nx = (s // 4 for s in after.shape)
    changed = (before != after).reshape(nz, 4, ny, 4, nx, 4).any(axis=(1, 3, 5))
    z, y, x = np.nonzero(changed)
    if not len(z):
        return 0
    bricks = after.reshape(nz, 4, ny, 4, nx, 4).transpose(0, 2, 4, 1, 3, 5)[z, y, x].reshape(-1, 4, 4, 4)
    return mixed_material_entries(bricks.reshape(-1, 4, 4))


def is_restart(st, step):
    """the step restarts the arrays: a whole-extent volume, or paste that replaces (the rule paste never restarts)"""
    E = 4 ** st.levels
    return step["box"] == ((0, 0, 0), (E, E, E)) and (step["kind"] == "volume" or step.get("keep_empty") is False)


def expected_crossings(st, run):
    """run: the (step, models) of Sequence.run().  [(tree, after, by, material entries, capacity, appended)]: the device
    arrays of `tree` must be reallocated at a step in (after, by], because by then a lower bound of its material entries
    passes the capacity it had after step `after`: that of a fresh upload, n + n / 8 + 65536 (svo_patch_commit.h), which
    is also what a compaction leaves (after = -1: the start).  A restart begins again with the entries of its own mixed
    bricks; every other patch appends at least appended_entries().  appended: no step of the window is a restart, so the
    reallocation keeps a prefix of the arrays.  One window per tree and compaction, at most."""
    total = [mixed_material_entries(d) for d in st.dense]
    cap = [m + m // 8 + 65536 for m in total]
    since, pure, done = [-1, -1], [True, True], [False, False]
    prev, found = list(st.dense), []
    for step, models in run:
        t = step["tree"]
        if step["kind"] == "compact":
            total[t] = mixed_material_entries(models[t])
            cap[t] = total[t] + total[t] // 8 + 65536
            since[t], pure[t], done[t] = step["i"], True, False
        elif not done[t]:
            if is_restart(st, step):
                total[t], pure[t] = mixed_material_entries(models[t]), False
            else:
                total[t] += appended_entries(prev[t], models[t])
            if total[t] > cap[t]:
                found.append((t, since[t], step["i"], total[t], cap[t], pure[t]))
                done[t] = True
        prev = models
    return found
