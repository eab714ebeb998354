"""One scripted sequence of world edits, applied alike to the product's World, to every linearised Tree handed in
(svo_tree_update: a solid tree and a VIEW_ALL scene tree each get their own update call per edit) and to the oracle's
reference-layout tree: the fixture of tests/test_patched_host.py and tests/test_gpu_patched_trees.py.

The edits are chosen for the shapes only a patched tree holds (svo_linearise.cpp, "Incremental edits"): an interior node
whose mask went to 0 under a set bit of its parent (a lone voxel deleted), 64 SOLID siblings of one material (a 16^3
filled by 4^3 puts), child blocks rewritten at the tail of the node array, a record rewritten in place, ceilings that
rise and fall, and, at 3 levels, a world that becomes empty, uniform and mixed again through edits of the root.

Everything lies in the working box [OX, OX + 64) x [0, 64) x [0, 64) (OX = 2048 at 6 levels: the box is then root child
2 in x, behind three levels of one-child interior nodes), except the voxel stages 12 / 13 put above it where the
world is taller than the box.  Levels as putBlock numbers them: L + 1 = a voxel, L = 4^3, L - 1 = 16^3, 1 = the world.
On the oracle's side a delete of level lv <= L is deleteBlock(lv - 1) and a voxel delete deleteBlock(L + 1), as in
tests/test_edits.py::_oracle_edit_replay; the oracle cannot delete its root, so stage 16 replaces it by a new clean
root.  No voxel deleted on its own is edited again (the churn of stage 14 moves on to a new voxel with every pair):
the reference's deleteBlock leaves the freed node in its parent's child array, a later put over that parent frees it a
second time, and two later allocations then share one node (restated by the oracle, tetrahexa_tree.cpp:159-173, :350)."""
import numpy as np

import cavern

BOX = 64
OX_OF = {3: 0, 4: 0, 6: 2048}
F_MIRROR, F_GLASS, F_WATER = 0x2, 0x4, 0x14
EMPTY = np.uint64(0xFFFFFFFFFFFFFFFF)
N_BASE = 3000
CHURN_MAX = 400
CHURN_Y = 30
N_STAGES = {3: 19, 4: 14, 6: 14}
ABOVE_Y = 70  # stages 12 / 13 at 4 and 6 levels: a voxel above the box too (at 3 levels the box is the world, top row 63 from the start)
BOX_TOP = {3: BOX, 4: ABOVE_Y + 2, 6: ABOVE_Y + 2}  # rows the comparisons of the whole box cover


def churn_voxel(i):
    """the voxel of churn pair i (relative to OX), inside the dust: a new one every time"""
    assert 0 <= i < CHURN_MAX
    return (33 + i % 20, CHURN_Y, 10 + i // 20)


class EditScript:
    """w: the product's World, T: the oracle's tree (replaced at stage 16), trees: the Trees patched with every edit
    (append them after construction, built from w).  stages() applies one stage per iteration and yields its number."""

    def __init__(self, rt, oracle_mod, levels):
        assert levels in OX_OF
        self.rt, self.O, self.L, self.ox = rt, oracle_mod, levels, OX_OF[levels]
        self.w = rt.World(levels)
        self.T = self._clean_oracle()
        self.trees = []
        self.stage = 0
        self.churned = 0
        # voxels deleted one by one: the oracle's level L + 1 delete splits the voxel and drops copy 0, which its getBlock reads
        # for coordinates in [0, 2^30) only (oracle.c o_shr; tests/test_edits.py::_oracle_edit_replay) -- callers that hand
        # the oracle unwrapped negative coordinates leave these voxels out
        self.voxel_deletes = []
        rng = np.random.default_rng(2025)
        p = np.stack([rng.integers(32, 64, N_BASE), rng.integers(0, 64, N_BASE), rng.integers(0, 64, N_BASE)], 1)
        self.base = p
        self._put(p, 0, 1000 + np.arange(N_BASE) % 37, levels + 1, batch=True)

    def _clean_oracle(self):
        T = self.O.Tree(self.L)
        self.O.lib().orc_init_clean_root(T.h)
        return T

    # ------------------------------------------------------------------------------------------------------ edits --
    def _abs(self, pts):
        return np.asarray(pts, np.int32).reshape(-1, 3) + np.array([self.ox, 0, 0], np.int32)

    def _put(self, pts, flags, ids, level, batch=False):
        """pts relative to OX; one World put and one update per tree for every point (batch: the base world, before any tree)"""
        p = self._abs(pts)
        f = np.full(len(p), flags, np.uint32)
        c = np.broadcast_to(cavern.colour(ids), (len(p),)).copy()
        if batch:
            assert not self.trees
            self.w.put_blocks(p, f, c, level=level)
        for i, ((x, y, z), fl, co) in enumerate(zip(p.tolist(), f.tolist(), c.tolist())):
            if not batch:
                self.w.put_blocks(p[i:i + 1], f[i:i + 1], c[i:i + 1], level=level)
                for t in self.trees:
                    t.update(self.w, p[i:i + 1], level=level)
            assert self.T.put_block(x, y, z, fl, co, 0.0, level) == 0

    def _delete(self, pt, level):
        p = self._abs([pt])
        x, y, z = p[0].tolist()
        self.w.delete_block(x, y, z, level=level)
        for t in self.trees:
            t.update(self.w, p, level=level)
        if level == self.L + 1:
            self.voxel_deletes.append((x, y, z))
        assert self.T.delete_block(x, y, z, level=level if level == self.L + 1 else level - 1)[0] in (0, 1)

    # ----------------------------------------------------------------------------------------------------- stages --
    def _apply(self, s):
        L, vox = self.L, self.L + 1
        if s == 1:    # a lone voxel in an empty 16^3
            self._put([(8, 40, 8)], 0, 1, vox)
        elif s == 2:  # ... deleted: a mask-0 interior chain stays under the set bits above it
            self._delete((8, 40, 8), vox)
        elif s == 3:  # a brick filled voxel by voxel with one material
            self._put([(x, y, z) for z in range(8, 12) for y in range(8, 12) for x in range(8, 12)], 0, 2, vox)
        elif s == 4:  # a 16^3 filled by 64 puts of 4^3: 64 SOLID siblings of one material, never re-collapsed
            self._put([(16 + 4 * i, 4 * j, 4 * k) for k in range(4) for j in range(4) for i in range(4)], 0, 3, L)
        elif s == 5:
            self._delete((17, 3, 2), vox)
        elif s == 6:
            self._delete((20, 4, 8), L)
        elif s == 7:  # a 16^3 mirror
            self._put([(0, 16, 16)], F_MIRROR, 4, L - 1)
        elif s == 8:
            self._delete((0, 16, 16), L - 1)
        elif s == 9:  # water: empty to the solid view, stored in the scene
            self._put([(4 * i, 48, 32 + 4 * k) for k in range(4) for i in range(4)], F_WATER, 5, L)
        elif s == 10:  # a glass wall
            self._put([(12, 20 + j, 40 + k) for j in range(8) for k in range(8)], F_GLASS, 6, vox)
        elif s == 11:  # inside the dust: a free voxel put, a dust voxel deleted (neither on a face of the box)
            free = self._free_dust_voxel()
            self._put([free], 0, 7, vox)
            self._delete(next(tuple(p) for p in self.base[1000:].tolist() if 32 < p[0] < 63 and 0 < p[1] < 63 and 0 < p[2] < 63 and p[1] != CHURN_Y), vox)
        elif s == 12:  # the top rises: row 62 of the box's first column block, and (taller worlds) a row above every other
            self._put([(5, 62, 5)], 0, 8, vox)
            if L > 3:
                self._put([(5, ABOVE_Y, 5)], 0, 8, vox)
        elif s == 13:  # ... and falls again
            self._delete((5, 62, 5), vox)
            if L > 3:
                self._delete((5, ABOVE_Y, 5), vox)
        elif s == 14:  # churn until superseded blocks outweigh the array: the rebuild (full_upload: the svo_upload route)
            tree = self.trees[0]
            n = tree.info().n_nodes
            dropped = False
            for i in range(CHURN_MAX):
                for put in (True, False):  # (a pair is always completed: the voxel is gone again when the stage ends)
                    if put:
                        self._put([churn_voxel(i)], 0, 9, vox)
                    else:
                        self._delete(churn_voxel(i), vox)
                    m = tree.info().n_nodes
                    dropped |= m < n
                    n = m
                self.churned = i + 1
                if dropped:
                    break
            assert dropped, "stage 14: no rebuild within %d put / delete pairs (%d nodes)" % (CHURN_MAX, n)
        elif s == 15:  # the wrap corners by their unwrapped coordinates, and glass at a corner's edge
            self._put([(-1, -1, -1), (64, 64, 64)], 0, 10, vox)
            self._put([(0, 63, 63)], F_GLASS, 11, vox)
        elif s == 16:  # the whole world deleted
            self.w.delete_block(0, 0, 0, level=1)
            for t in self.trees:
                t.update(self.w, [[0, 0, 0]], level=1)
            self.T = self._clean_oracle()
            self.voxel_deletes = []
        elif s == 17:  # a voxel into the empty world
            self._put([(21, 22, 23)], 0, 12, vox)
        elif s == 18:  # the root itself SOLID
            self._put([(0, 0, 0)], 0, 13, 1)
        elif s == 19:  # ... and mixed again
            self._delete((63, 63, 63), vox)
        else:
            raise ValueError(s)

    def _free_dust_voxel(self):
        """the first voxel of x in [33, 63), y, z in [1, 63) (seeded order) that the base world leaves empty"""
        taken = set(map(tuple, self.base.tolist()))
        rng = np.random.default_rng(2026)
        while True:
            p = (int(rng.integers(33, 63)), int(rng.integers(1, 63)), int(rng.integers(1, 63)))
            if p not in taken and p[1] != CHURN_Y:
                return p

    def stages(self):
        assert self.trees, "append the trees to patch (built from .w) before running the stages"
        for s in range(1, N_STAGES[self.L] + 1):
            self._apply(s)
            self.stage = s
            yield s

    # ------------------------------------------------------------------------------------------------- references --
    def oracle_box(self, view, ny=BOX):
        """(flags, colour) of the oracle's getBlock over the working box, rows [0, ny), arrays [z][y][x]; the solid view drops
        liquid blocks"""
        rc, f, c = self.T.dump_box(self.ox, 0, 0, BOX, ny, BOX)
        assert rc == 0
        if view == self.rt.VIEW_SOLID:
            liquid = (f & 0x10) != 0
            f, c = np.where(liquid, 0, f).astype(np.uint32), np.where(liquid, EMPTY, c)
        return f, c

    def box_points(self, ny=BOX, shift=(0, 0, 0)):
        """the box's voxels in oracle_box's order (z slowest, x fastest), moved by `shift`"""
        z, y, x = np.meshgrid(np.arange(BOX), np.arange(ny), np.arange(BOX), indexing="ij")
        return (np.stack([x + self.ox, y, z], -1).reshape(-1, 3) + np.asarray(shift)).astype(np.int32)


def palette_arrays(tree):
    pal = tree.palette()
    return np.array([p[0] for p in pal], np.uint32), np.array([p[1] for p in pal], np.uint64)
