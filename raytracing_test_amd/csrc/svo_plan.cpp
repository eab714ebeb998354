// svo_plan.cpp — the host arithmetic of svo_plan.h: the AO plan's simulation, a frame launch's octant, segment and
// axis set-up, the ceiling pair / quad tables, what a sync has to move, the frame schedule's decisions, and a launch's
// block and ray counts (svo_cast_blocks, svo_cast_count).
#include "svo_plan.h"

#include <math.h>

#include <algorithm>

namespace svo {

// The AO plan of (n samples, `steps`) (see ao_count_plan): every (sample, face) ray simulated with
// the kernel's DDA from the centre of cell 0 — dda_axis, then dda_step's axis rule in double.
// Offsets are listed by step index, then sample, first appearance only.
std::vector<uint32_t> ao_plan_image(int32_t n, int32_t steps, const float* tab) {
    if (steps > 127 || n > 64) return {};  // offsets are packed in bytes, masks in 64 bits: rays
    std::vector<std::vector<std::pair<uint32_t, uint64_t>>> faces(6);
    for (int face = 0; face < 6; face++) {
        const uint32_t ax = (uint32_t)face >> 1;
        const int32_t sg = (face & 1) ? -1 : 1;
        std::vector<std::vector<uint32_t>> seq(n);
        for (int32_t i = 0; i < n; i++) {
            float dir[3];
            ao_dir(tab + 3 * i, ax, sg, dir);
            double T[3], A[3];
            int32_t st[3], pos[3] = {0, 0, 0};
            for (int k = 0; k < 3; k++) {
                const Dda1 a = dda_axis(0.5f, dir[k]);
                T[k] = a.dpos;
                A[k] = (double)(float)a.adelta;
                st[k] = a.step;
            }
            for (int32_t j = 0; j < steps; j++) {
                const bool cx = (T[0] < T[1]) && (T[0] < T[2]);
                const bool cy = !cx && (T[1] < T[2]);
                const int k = cx ? 0 : (cy ? 1 : 2);
                pos[k] += st[k];
                T[k] = T[k] + A[k];
                seq[i].push_back((uint32_t)(pos[0] + 128) | ((uint32_t)(pos[1] + 128) << 8) | ((uint32_t)(pos[2] + 128) << 16));
            }
        }
        auto& f = faces[face];
        for (int32_t j = 0; j < steps; j++)
            for (int32_t i = 0; i < n; i++) {
                const uint32_t key = seq[i][j];
                size_t e = 0;
                while (e < f.size() && f[e].first != key) e++;
                if (e == f.size()) f.push_back({key, 0ull});
                f[e].second |= 1ull << i;
            }
    }
    struct Brick {
        uint32_t key;
        uint64_t vm, um, sm[64];
    };
    std::vector<uint32_t> img(2 * 6 * 64, 0u);
    for (int face = 0; face < 6; face++)
        for (int al = 0; al < 64; al++) {
            const int32_t a[3] = {al & 3, (al >> 2) & 3, al >> 4};
            std::vector<Brick> bricks;  // in order of first use
            for (const auto& f : faces[face]) {
                uint32_t key = 0u, v = 0u;
                for (int k = 0; k < 3; k++) {
                    const int32_t p = a[k] + (int32_t)((f.first >> (8 * k)) & 255u) - 128;  // from lastPos's brick corner
                    key |= (uint32_t)((p >> 2) + 128) << (8 * k);                            // floor division
                    v |= (uint32_t)(p & 3) << (2 * k);
                }
                size_t b = 0;
                while (b < bricks.size() && bricks[b].key != key) b++;
                if (b == bricks.size()) {
                    bricks.push_back(Brick{});
                    bricks.back().key = key;
                }
                bricks[b].vm |= 1ull << v;
                bricks[b].um |= f.second;
                bricks[b].sm[v] |= f.second;
            }
            const size_t g = (size_t)face * 64 + (size_t)al;
            img[2 * g] = (uint32_t)(img.size() / 4);
            img[2 * g + 1] = (uint32_t)bricks.size();
            for (const Brick& b : bricks) {
                const uint32_t rec[8] = {b.key, 0u, (uint32_t)b.vm, (uint32_t)(b.vm >> 32), (uint32_t)b.um, (uint32_t)(b.um >> 32), 0u, 0u};
                img.insert(img.end(), rec, rec + 8);
                for (int v = 0; v < 64; v++)
                    if ((b.vm >> v) & 1ull) {
                        img.push_back((uint32_t)b.sm[v]);
                        img.push_back((uint32_t)(b.sm[v] >> 32));
                    }
                while (img.size() % 4) img.push_back(0u);
            }
        }
    return img;
}

// The launch's step-sign octant (1..8, dirs_sign) when every frame ray has the same step signs, else 0.
// A pixel's direction before normalisation (raygen_pixel) is an affine function of the pixel, so its
// extremes are at the frame's corners; a corner value beyond 1e-4 of the terms' magnitudes keeps
// every pixel's rounded value (errors of a few ulps of those terms) on the same side of zero, and
// normalisation keeps the sign.  (Explicit rays have none: 0 without a call.)
int frame_dirs(const RayGen& rg, int32_t width, int32_t height, int32_t flags) {
    if (flags & SVO_CAST_NO_OCTANT) return 0;
    int code = 1;
    for (int a = 0; a < 3; a++) {
        int pos = 0, neg = 0;
        for (int c = 0; c < 4; c++) {
            const int32_t px = (c & 1) ? width - 1 : 0, py = (c & 2) ? height - 1 : 0;
            const float fx = ((float)px + 0.5f) * rg.rw, fy = ((float)py + 0.5f) * rg.rh;
            const float sl = -(rg.ppx * (fx - 0.5f)), su = -fy + 0.5f;
            const float lt = rg.l[a] * sl, ut = (rg.u[a] * su) * rg.ppy;
            const float v = (rg.c[a] + lt) + ut;
            const float mag = fabsf(rg.c[a]) + fabsf(rg.l[a]) * fabsf(rg.ppx) + fabsf(rg.u[a] * rg.ppy);
            if (v > 1e-4f * mag) pos++;
            else if (v < -1e-4f * mag) neg++;
        }
        if (pos == 4) continue;
        if (neg == 4) code += 1 << a;
        else return 0;
    }
    return code;
}

// Can the launch hold rays that are not linear (svo_exact.h, "Exact closed-form skipping")?  From an
// integral or half-integral origin every ray is (lin_origin, with budgets below 2^28 every sum it
// takes is exact); explicit rays are not inspected.  The instance without segments relies on it
// (trace: TRACK); SVO_CAST_SEGMENTS forces the other one (the same results).
// org: the launch's n_org origins (a frame launch's frame origins, else the one origin).
bool need_seg(int32_t flags, bool explicit_rays, int32_t steps, const float* org, int32_t n_org) {
    if (flags & SVO_CAST_SEGMENTS) return true;
    if (explicit_rays || steps >= (1 << 28)) return true;
    for (int32_t i = 0; i < 3 * n_org; i++)
        if (!(2.0f * org[i] == __builtin_truncf(2.0f * org[i]) && __builtin_fabsf(org[i]) < 1073741824.0f)) return true;
    return false;
}

// the octant's frame set-up (FrameAxes, svo_cast_params.h) for a frame cast from org
void frame_axes(int dirs, const float org[3], double frac[3], int32_t cell[3]) {
    for (int k = 0; k < 3; k++) {
        const float o = org[k];
        cell[k] = (int32_t)__builtin_truncf(o);
        const double exact = ((dirs - 1) >> k) & 1 ? (double)o - 1.0 : (double)o;
        frac[k] = exact - (double)cell[k];
    }
}

// Diagnostics instances are generic (no octant); an AO launch has its counters but no timeline of its own (TIMELINE
// alone runs the plain AO instance).  The camera's octant (frame_dirs; a code outside 1..8 counts as 8) is compiled into
// narrow-node instances only.  Shading instances carry segment bounds — the bouncing trace needs them — except the
// straight trace of a launch without hit records whose every origin is exact (NOREC without SEG: shaded C3 0.2887 ->
// 0.2831 ms); shading launches take no AO rays.
CastInstance cast_instance(const CastRequest& q) {
    CastInstance k = {q.stats, q.stats || (q.timeline && (q.shade || !q.ao)), q.ao && !q.shade, q.shade, q.wide, q.seg, 0, false};
    const bool octant = !k.stats && !k.stamps && !q.wide && q.dirs != 0;
    if (octant) k.dirs = q.dirs >= 1 && q.dirs <= 8 ? q.dirs : 8;
    if (q.shade) {
        k.norec = octant && !q.records;
        k.seg = k.norec ? q.seg : true;
    }
    return k;
}

// The ceiling pairs of level j (its block's ceiling, low 16 bits; its level-(j + kCeilPairStep) block's, high, or the coarsest
// level's when the tree has fewer) over the blocks holding columns [x0, x1) x [z0, z1) — widened to whole parent blocks, whose change reaches
// every child's pair.  Returns per level the first and last row written (level j's rows of blocks, row-major [z][x]).
static void ceil_pairs(svo_tree* t, int32_t n, int64_t x0, int64_t z0, int64_t x1, int64_t z1, int64_t zr[kCeilMax][2]) {
    for (int32_t j = 0; j < n; j++) {
        const int64_t rows = (int64_t)1 << (2 * (t->levels - kCeilK0 - j));
        const int32_t up = std::min(j + kCeilPairStep, n - 1), sh = 2 * (up - j);
        const int32_t ush = 2 * (kCeilK0 + up), bsh = 2 * (kCeilK0 + j);
        const int64_t rows_up = rows >> sh;
        const int64_t bz0 = (z0 >> ush) << (ush - bsh), bz1 = std::min(rows, (((z1 - 1) >> ush) + 1) << (ush - bsh));
        const int64_t bx0 = (x0 >> ush) << (ush - bsh), bx1 = std::min(rows, (((x1 - 1) >> ush) + 1) << (ush - bsh));
        const int16_t* c = t->ceil_host.data();
        for (int64_t z = bz0; z < bz1; z++)
            for (int64_t x = bx0; x < bx1; x++)
                t->ceilp_host[t->ceil_off[j] + z * rows + x] = (uint32_t)(uint16_t)c[t->ceil_off[j] + z * rows + x] |
                                                                 ((uint32_t)(uint16_t)c[t->ceil_off[up] + (z >> sh) * rows_up + (x >> sh)] << 16);
        zr[j][0] = bz0;
        zr[j][1] = bz1;
    }
}

// The ceiling quads (svo_tree.d_ceilq) of the level-0 blocks holding columns [x0, x1) x [z0, z1), widened to whole blocks of
// the coarsest level (whose change reaches every level-0 block inside it).  Returns the first and last row written.
static void ceil_quads(svo_tree* t, int32_t n, int64_t x0, int64_t z0, int64_t x1, int64_t z1, int64_t zr[2]) {
    const int64_t rows = (int64_t)1 << (2 * (t->levels - kCeilK0));
    const int32_t tsh = 2 * (n - 1);  // the coarsest level's blocks, in level-0 blocks (log2)
    const int32_t bsh = 2 * kCeilK0 + tsh;
    const int64_t bz0 = (z0 >> bsh) << tsh, bz1 = std::min(rows, (((z1 - 1) >> bsh) + 1) << tsh);
    const int64_t bx0 = (x0 >> bsh) << tsh, bx1 = std::min(rows, (((x1 - 1) >> bsh) + 1) << tsh);
    const int16_t* c = t->ceil_host.data();
    for (int64_t z = bz0; z < bz1; z++)
        for (int64_t x = bx0; x < bx1; x++) {
            uint64_t q = 0;
            for (int32_t j = 0; j < kCeilMax; j++) {
                const int16_t v = j < n ? c[t->ceil_off[j] + (z >> (2 * j)) * (rows >> (2 * j)) + (x >> (2 * j))] : (int16_t)0x7FFF;
                q |= (uint64_t)(uint16_t)v << (16 * j);
            }
            t->ceilq_host[z * rows + x] = q;
        }
    zr[0] = bz0;
    zr[1] = bz1;
}

int32_t ceil_tables_build(svo_tree* t) {
    int64_t off[kCeilMax] = {0, 0, 0, 0}, zr[kCeilMax][2], qr[2];
    const int32_t n = tree_ceilings(t, t->ceil_host, off, &t->ceil_fine_host);  // (the fine table: empty when n == 0)
    for (int j = 0; j < kCeilMax; j++) t->ceil_off[j] = t->ceilp_off[j] = off[j];
    t->ceilp_host.assign(t->ceil_host.size(), 0u);
    t->ceilq_host.clear();
    if (n > 0) {
        const int64_t e = (int64_t)1 << (2 * t->levels);
        ceil_pairs(t, n, 0, 0, e, e, zr);
        t->ceilq_host.assign((size_t)1 << (4 * (t->levels - kCeilK0)), 0ull);
        ceil_quads(t, n, 0, 0, e, e, qr);
    }
    return n;
}

// row intervals [first, last) sorted and joined where they overlap or touch
static void merge_rows(std::vector<std::pair<int64_t, int64_t>>& v) {
    std::sort(v.begin(), v.end());
    size_t k = 0;
    for (size_t i = 0; i < v.size(); i++) {
        if (v[i].second <= v[i].first) continue;
        if (k > 0 && v[i].first <= v[k - 1].second) v[k - 1].second = std::max(v[k - 1].second, v[i].second);
        else v[k++] = v[i];
    }
    v.resize(k);
}

void ceil_tables_update(svo_tree* t, int32_t n, const std::array<int64_t, 4>& r, int64_t zr[kCeilMax][2], int64_t qr[2]) {
    ceilings_update_rect(t, t->ceil_host, t->ceil_off, n, r[0], r[1], r[2], r[3], &t->ceil_fine_host);
    ceil_pairs(t, n, r[0], r[1], r[2], r[3], zr);
    ceil_quads(t, n, r[0], r[1], r[2], r[3], qr);
}

bool ceil_fine_for(int32_t launch_levels, int32_t first_level) { return launch_levels > 0 && first_level == 0; }

MarchLevels march_levels(int32_t ceil_levels, int32_t first_level, int32_t levels) {
    MarchLevels m = {};
    if (first_level < 0 || ceil_levels <= first_level) return m;
    int32_t top = std::min(std::min(ceil_levels, (int32_t)kCeilMax) - 1, first_level + kMarchCoarseMax);
    while (top > first_level && levels - kCeilK0 - top < 1) top--;  // (4^(levels - kCeilK0 - l) blocks per row: at least 4)
    for (int32_t l = top; l > first_level; l--) m.level[m.n++] = l;
    return m;
}

MarchParams march_params(const svo_tree* t, int32_t launch_levels, int32_t first_level) {
    MarchParams p = {};
    if (launch_levels <= 0) return p;
    const MarchLevels ml = march_levels(t->ceil_levels, first_level, t->levels);
    p.n = ml.n;
    for (int32_t j = 0; j < ml.n; j++) {
        p.sh[j] = 2u * (uint32_t)(kCeilK0 + ml.level[j]);
        p.off[j] = t->ceil_off[ml.level[j]];
    }
    return p;
}

CeilFineSpan ceil_fine_span(const svo_tree* t, const std::pair<int64_t, int64_t>& level0_rows) {
    const int64_t w = (int64_t)1 << (2 * t->levels - kCeilFineSh);  // fine blocks per row
    const int64_t per = (int64_t)1 << (2 * kCeilK0 - kCeilFineSh);  // fine rows per level-0 row
    const int64_t lo = std::min(level0_rows.first * per, w), hi = std::min(level0_rows.second * per, w);
    return {lo * w, std::max<int64_t>(0, hi - lo) * w};
}

void ceil_tables_update_all(svo_tree* t, int32_t n, const std::vector<std::array<int64_t, 4>>& rects, CeilRows* rows) {
    // the quads of a rectangle are those of the coarsest level's blocks holding it: each distinct span of such blocks is
    // recomputed once, after every rectangle's ceilings are final (a list of scattered edits has thousands of rectangles
    // in a few hundred spans)
    const int32_t csh = 2 * (kCeilK0 + n - 1);
    std::vector<std::array<int64_t, 4>> spans;
    for (const auto& r : rects) {
        int64_t zr[kCeilMax][2];
        ceilings_update_rect(t, t->ceil_host, t->ceil_off, n, r[0], r[1], r[2], r[3], &t->ceil_fine_host);
        ceil_pairs(t, n, r[0], r[1], r[2], r[3], zr);
        for (int32_t j = 0; j < n; j++) rows->level[j].push_back({zr[j][0], zr[j][1]});
        spans.push_back({r[0] >> csh, r[1] >> csh, (r[2] - 1) >> csh, (r[3] - 1) >> csh});
    }
    std::sort(spans.begin(), spans.end());
    spans.erase(std::unique(spans.begin(), spans.end()), spans.end());
    for (const auto& s : spans) {
        int64_t qr[2];
        ceil_quads(t, n, s[0] << csh, s[1] << csh, (s[2] + 1) << csh, (s[3] + 1) << csh, qr);
        rows->quads.push_back({qr[0], qr[1]});
    }
    for (int32_t j = 0; j < n; j++) merge_rows(rows->level[j]);
    merge_rows(rows->quads);
}

std::vector<std::pair<uint32_t, uint32_t>> dirty_runs(std::vector<uint32_t>& dirty) {
    std::vector<std::pair<uint32_t, uint32_t>> runs;
    std::sort(dirty.begin(), dirty.end());
    for (size_t i = 0; i < dirty.size();) {
        size_t j = i + 1;
        while (j < dirty.size() && dirty[j] <= dirty[j - 1] + 1) j++;
        runs.push_back({dirty[i], dirty[j - 1]});
        i = j;
    }
    return runs;
}

bool tree_unsynced(const svo_tree* t) {
    return t->full_upload || t->nodes.size() != t->synced_nodes || t->mats.size() != t->synced_mats || !t->dirty_nodes.empty() ||
           t->palette_dirty || !t->ceil_dirty.empty();
}

PatchAnchor patch_anchor(const Node* nodes, int32_t levels, const int32_t lo[3], const int32_t hi[3]) {
    PatchAnchor a{0u, 0, {0, 0, 0}, P_NODE, 0u, true};
    const int32_t e = 1 << (2 * levels);
    for (int i = 0; i < 3; i++) a.whole = a.whole && lo[i] == 0 && hi[i] == e;
    if (node_kind(nodes[0].info) != K_INTERIOR) {  // a lone SOLID root (a BRICK root: a tree of one level, which is not patched)
        a.kind = P_UNIFORM;
        a.old = node_material(nodes[0].info);
        return a;
    }
    while (!a.whole && a.depth < levels - 2) {  // (a child at depth levels - 1 is a BRICK or SOLID record)
        const int32_t cs = 1 << (2 * (levels - 1 - a.depth));
        int32_t c[3];
        bool inside = true, fills = true;
        for (int i = 0; i < 3; i++) {
            c[i] = a.o[i] + ((lo[i] - a.o[i]) / cs) * cs;  // the child region holding the box's first voxel
            inside = inside && hi[i] <= c[i] + cs;
            fills = fills && lo[i] == c[i] && hi[i] == c[i] + cs;
        }
        if (!inside || fills) break;
        const Node& n = nodes[a.node];
        const uint32_t sl = (uint32_t)((((c[2] - a.o[2]) / cs) << 4) | (((c[1] - a.o[1]) / cs) << 2) | ((c[0] - a.o[0]) / cs));
        if (!((n.mask >> sl) & 1ull)) break;
        const uint32_t ci = packed_index(n, sl);
        if (node_kind(nodes[ci].info) != K_INTERIOR) break;
        a.node = ci;
        a.depth++;
        for (int i = 0; i < 3; i++) a.o[i] = c[i];
    }
    a.old = a.node;
    return a;
}

PatchAnchor points_anchor(const Node* nodes, int32_t levels, uint64_t key_first, uint64_t key_last) {
    PatchAnchor a{0u, 0, {0, 0, 0}, P_NODE, 0u, false};
    if (node_kind(nodes[0].info) != K_INTERIOR) {  // a lone SOLID root, as in patch_anchor
        a.kind = P_UNIFORM;
        a.old = node_material(nodes[0].info);
        return a;
    }
    while (a.depth < levels - 2) {  // (a child at depth levels - 1 is a BRICK or SOLID record)
        const int sh = 6 * (levels - 1 - a.depth);
        const uint32_t sl = (uint32_t)((key_first >> sh) & 63ull);
        if ((key_first >> sh) != (key_last >> sh)) break;  // the edits part here
        const Node& n = nodes[a.node];
        if (!((n.mask >> sl) & 1ull)) break;
        const uint32_t ci = packed_index(n, sl);
        if (node_kind(nodes[ci].info) != K_INTERIOR) break;
        const int32_t cs = 1 << (2 * (levels - 1 - a.depth));
        a.node = ci;
        a.depth++;
        a.o[0] += (int32_t)(sl & 3u) * cs;
        a.o[1] += (int32_t)((sl >> 2) & 3u) * cs;
        a.o[2] += (int32_t)(sl >> 4) * cs;
    }
    a.old = a.node;
    return a;
}

std::vector<std::array<int64_t, 4>> ceil_block_rects(std::vector<uint64_t>& blocks) {
    std::vector<std::array<int64_t, 4>> rects;
    std::sort(blocks.begin(), blocks.end());
    const int64_t w = (int64_t)1 << (2 * kCeilK0);
    std::vector<size_t> prev, cur;  // the rectangles (indices) that end at the row before / at the current row, ascending in x
    size_t pi = 0;
    int64_t row = -2;
    for (size_t i = 0; i < blocks.size();) {
        const int64_t bz = (int64_t)(blocks[i] >> 32), bx0 = (int64_t)(blocks[i] & 0xFFFFFFFFull);
        int64_t bx1 = bx0 + 1;
        size_t j = i + 1;
        while (j < blocks.size() && (int64_t)(blocks[j] >> 32) == bz && (int64_t)(blocks[j] & 0xFFFFFFFFull) <= bx1) {
            bx1 = std::max(bx1, (int64_t)(blocks[j] & 0xFFFFFFFFull) + 1);  // (a duplicate keeps bx1)
            j++;
        }
        i = j;
        if (bz != row) {  // a new row: only the rectangles of the row just before it can grow into it
            if (bz == row + 1) prev.swap(cur);
            else prev.clear();
            cur.clear();
            pi = 0;
            row = bz;
        }
        while (pi < prev.size() && rects[prev[pi]][0] < bx0 * w) pi++;
        if (pi < prev.size() && rects[prev[pi]][0] == bx0 * w && rects[prev[pi]][2] == bx1 * w) {  // the same span one row up
            rects[prev[pi]][3] = (bz + 1) * w;
            cur.push_back(prev[pi++]);
        } else {
            cur.push_back(rects.size());
            rects.push_back({bx0 * w, bz * w, bx1 * w, (bz + 1) * w});
        }
    }
    return rects;
}

namespace {
struct Superseded {
    const Node* nodes;
    int32_t levels;
    const int32_t *lo, *hi;
    uint64_t n_nodes = 0, n_mats = 0;
    // node ni's record is replaced: what hangs below it.  all: the region lies wholly inside the box
    void walk(uint32_t ni, const int32_t o[3], int depth, bool all) {
        const Node& n = nodes[ni];
        const uint32_t kind = node_kind(n.info);
        if (kind == K_SOLID) return;
        if (kind == K_BRICK) {
            if (!(n.info & K_UNIFORM)) n_mats += (uint64_t)__builtin_popcountll(n.mask);
            return;
        }
        n_nodes += (uint64_t)__builtin_popcountll(n.mask);
        const int32_t cs = 1 << (2 * (levels - 1 - depth));
        uint64_t m = n.mask;
        uint32_t ci = n.ref;
        while (m) {
            const uint32_t sl = (uint32_t)__builtin_ctzll(m);
            m &= m - 1;
            const uint32_t c = ci++;
            const int32_t co[3] = {o[0] + (int32_t)(sl & 3u) * cs, o[1] + (int32_t)((sl >> 2) & 3u) * cs, o[2] + (int32_t)(sl >> 4) * cs};
            bool out = false, in = true;
            for (int i = 0; i < 3; i++) {
                out = out || co[i] + cs <= lo[i] || co[i] >= hi[i];
                in = in && co[i] >= lo[i] && co[i] + cs <= hi[i];
            }
            if (all || in) walk(c, co, depth + 1, true);
            else if (!out) walk(c, co, depth + 1, false);  // (outside the box: the copied record keeps its subtree)
        }
    }
};
}  // namespace

void patch_superseded(const Node* nodes, int32_t levels, const PatchAnchor& a, const int32_t lo[3], const int32_t hi[3], uint64_t* n_nodes,
                      uint64_t* n_mats) {
    Superseded s{nodes, levels, lo, hi};
    s.walk(a.node, a.o, a.depth, a.whole);
    *n_nodes = s.n_nodes;
    *n_mats = s.n_mats;
}

// floor(sqrt(v)) for 0 <= v <= 2^42: the double root, put right by at most one either way
static int64_t isqrt_floor(int64_t v) {
    int64_t r = (int64_t)__builtin_sqrt((double)v);
    while (r > 0 && r * r > v) r--;
    while ((r + 1) * (r + 1) <= v) r++;
    return r;
}

int shapes_plan(int32_t levels, int32_t view, const std::vector<Material>& palette, const svo_shape* shapes, int32_t n, ShapesPlan* plan,
                int32_t* bad) {
    const int64_t E = (int64_t)1 << (2 * levels);
    plan->table.clear();
    plan->rects.clear();
    for (int a = 0; a < 3; a++) {
        plan->lo[a] = (int32_t)E;
        plan->hi[a] = 0;
    }
    for (int32_t i = 0; i < n; i++) {
        const svo_shape& s = shapes[i];
        *bad = i;
        int64_t lo[3], hi[3];
        if (s.kind == SVO_SHAPE_BOX) {
            for (int a = 0; a < 3; a++)
                if (s.b[a] <= 0) return SHAPES_BOX_DIM;
            for (int a = 0; a < 3; a++) {
                if (s.a[a] < 0 || (int64_t)s.a[a] + s.b[a] > E) return SHAPES_BOX_EXTENT;
                lo[a] = s.a[a];
                hi[a] = (int64_t)s.a[a] + s.b[a];
            }
        } else if (s.kind == SVO_SHAPE_BALL) {
            if (s.r2 < 0) return SHAPES_R2_NEG;
            for (int a = 0; a < 3; a++)
                if (s.a[a] > kShapeCentreMax || s.a[a] < -kShapeCentreMax) return SHAPES_CENTRE;
            if (s.r2 > kShapeR2Max) return SHAPES_R2_BIG;
            const int64_t r = isqrt_floor(s.r2);
            for (int a = 0; a < 3; a++) {
                lo[a] = std::max<int64_t>(0, (int64_t)s.a[a] - r);
                hi[a] = std::min<int64_t>(E, (int64_t)s.a[a] + r + 1);
            }
        } else {
            return SHAPES_KIND;
        }
        if ((size_t)s.id >= palette.size()) return SHAPES_ID;
        if (lo[0] >= hi[0] || lo[1] >= hi[1] || lo[2] >= hi[2]) continue;  // clipped away
        ShapeRec r{s.kind == SVO_SHAPE_BOX ? kShapeBox : kShapeBall, {s.a[0], s.a[1], s.a[2]}, {0, 0, 0}, 0u, 0};
        if (s.kind == SVO_SHAPE_BOX)
            for (int a = 0; a < 3; a++) r.b[a] = (int32_t)hi[a];
        else r.r2 = s.r2;
        r.id = s.id != 0 && material_in_view(palette[s.id], view) ? (uint32_t)s.id : 0u;
        plan->table.push_back(r);
        plan->rects.push_back({lo[0], lo[2], hi[0], hi[2]});
        for (int a = 0; a < 3; a++) {
            plan->lo[a] = std::min(plan->lo[a], (int32_t)lo[a]);
            plan->hi[a] = std::max(plan->hi[a], (int32_t)hi[a]);
        }
    }
    *bad = -1;
    return SHAPES_OK;
}

namespace {
// The walk shapes_superseded and paste_superseded share: rel(co, cs, k) is the device pass's own question about the child
// cell at co, cs = 4^k voxels wide, answered SHAPE_OUT / SHAPE_IN / SHAPE_CUT (PASTE_* are the same numbers)
template <class Rel>
struct CellSuperseded {
    const Node* nodes;
    int32_t levels;
    Rel rel;
    uint64_t n_nodes = 0, n_mats = 0;
    // node ni's record is replaced: what hangs below it.  all: the cell lies wholly inside what replaces it
    void walk(uint32_t ni, const int32_t o[3], int depth, bool all) {
        const Node& nd = nodes[ni];
        const uint32_t kind = node_kind(nd.info);
        if (kind == K_SOLID) return;
        if (kind == K_BRICK) {
            if (!(nd.info & K_UNIFORM)) n_mats += (uint64_t)__builtin_popcountll(nd.mask);
            return;
        }
        n_nodes += (uint64_t)__builtin_popcountll(nd.mask);
        const int k = levels - 1 - depth;
        const int32_t cs = 1 << (2 * k);
        uint64_t m = nd.mask;
        uint32_t ci = nd.ref;
        while (m) {
            const uint32_t sl = (uint32_t)__builtin_ctzll(m);
            m &= m - 1;
            const uint32_t c = ci++;
            const int32_t co[3] = {o[0] + (int32_t)(sl & 3u) * cs, o[1] + (int32_t)((sl >> 2) & 3u) * cs, o[2] + (int32_t)(sl >> 4) * cs};
            const uint32_t r = all ? (uint32_t)SHAPE_IN : rel(co, cs, k);
            if (r == SHAPE_IN) walk(c, co, depth + 1, true);
            else if (r == SHAPE_CUT) walk(c, co, depth + 1, false);  // (untouched: the copied record keeps its subtree)
        }
    }
};
static_assert((uint32_t)PASTE_OUT == (uint32_t)SHAPE_OUT && (uint32_t)PASTE_IN == (uint32_t)SHAPE_IN &&
                  (uint32_t)PASTE_CUT == (uint32_t)SHAPE_CUT,
              "one walk serves both cell logics");
}  // namespace

void shapes_superseded(const Node* nodes, int32_t levels, const PatchAnchor& a, const ShapeRec* shapes, int32_t n, uint64_t* n_nodes,
                       uint64_t* n_mats) {
    auto rel = [=](const int32_t co[3], int32_t cs, int) {
        uint32_t id;
        return cell_relation(shapes, n, co[0], co[1], co[2], cs, &id);
    };
    CellSuperseded<decltype(rel)> s{nodes, levels, rel};
    s.walk(a.node, a.o, a.depth, false);
    *n_nodes = s.n_nodes;
    *n_mats = s.n_mats;
}

int paste_plan(int32_t dst_levels, int32_t src_levels, const int32_t* src_origin, int32_t nx, int32_t ny, int32_t nz, const int32_t dst_origin[3],
               uint32_t flags, PastePlan* plan, const uint8_t* axis, const uint8_t* flip) {
    if (flags & ~(uint32_t)SVO_PASTE_KEEP_EMPTY) return PASTE_FLAGS;
    PasteTurn& r = plan->rec;
    uint32_t seen = 0u;
    for (int a = 0; a < 3; a++) {
        r.axis[a] = axis ? axis[a] : (uint8_t)a;
        if (r.axis[a] > 2) return PASTE_AXIS;
        seen |= 1u << r.axis[a];
    }
    if (seen != 7u) return PASTE_AXIS;
    for (int a = 0; a < 3; a++) {
        if (flip && flip[a] > 1) return PASTE_FLIP;
        r.sign[a] = flip && flip[a] ? -1 : 1;
    }
    ListBox sb;
    switch (list_box(src_levels, src_origin, nx, ny, nz, &sb)) {
        case LIST_BOX_DIM: return PASTE_DIM;
        case LIST_BOX_EXTENT: return PASTE_SRC_EXTENT;
        default: break;
    }
    const int64_t E = (int64_t)1 << (2 * dst_levels);
    plan->whole = !(flags & SVO_PASTE_KEEP_EMPTY);
    for (int a = 0; a < 3; a++) {
        const int j = r.axis[a];
        const int64_t dim = (int64_t)sb.hi[j] - sb.lo[j];
        if (dst_origin[a] < 0 || (int64_t)dst_origin[a] + dim > E) return PASTE_DST_EXTENT;
        r.lo[a] = dst_origin[a];
        r.hi[a] = (int32_t)(dst_origin[a] + dim);
        r.shift[a] = r.sign[a] > 0 ? sb.lo[j] - dst_origin[a] : sb.hi[j] - 1 + dst_origin[a];  // (both extents are at most 2^14)
        plan->whole = plan->whole && r.lo[a] == 0 && r.hi[a] == E;
    }
    r.keep_empty = flags & SVO_PASTE_KEEP_EMPTY;
    r.in_view = nullptr;
    r.id_map = nullptr;
    return PASTE_OK;
}

int paste_rule_check(uint32_t flags, uint32_t rule) {
    if (flags) return RULE_FLAGS;
    if (rule >> 6) return RULE_BITS;
    const uint32_t A = rule & 3u, B = (rule >> 2) & 3u, C = (rule >> 4) & 3u;
    if (A != RULE_KEEP && A != RULE_TAKE) return RULE_SRC_ONLY;
    if (B > RULE_CLEAR) return RULE_BOTH;
    if (C != RULE_KEEP && C != RULE_CLEAR) return RULE_DST_ONLY;
    return RULE_OK;
}

bool paste_view_bits(const std::vector<Material>& palette, int32_t view, std::vector<uint32_t>* bits) {
    bits->assign((palette.size() + 31) / 32, 0u);
    bool all = true;
    for (size_t i = 0; i < palette.size(); i++) {
        const bool in = i == 0 || material_in_view(palette[i], view);
        if (in) (*bits)[i >> 5] |= 1u << (i & 31u);
        all = all && in;
    }
    return all;
}

namespace {
template <class Rec>
void paste_superseded_as(const Node* nodes, int32_t levels, const PatchAnchor& a, const Rec& rec, const PasteTree& src, uint64_t* n_nodes,
                         uint64_t* n_mats) {
    auto rel = [&](const int32_t co[3], int32_t cs, int k) {
        uint32_t id;
        return relation_of(rec, src, co[0], co[1], co[2], cs, k, &id);
    };
    CellSuperseded<decltype(rel)> s{nodes, levels, rel};
    s.walk(a.node, a.o, a.depth, false);
    *n_nodes = s.n_nodes;
    *n_mats = s.n_mats;
}
}  // namespace

void paste_superseded(const Node* nodes, int32_t levels, const PatchAnchor& a, const PasteRec& rec, const PasteTree& src, uint64_t* n_nodes,
                      uint64_t* n_mats) {
    paste_superseded_as(nodes, levels, a, rec, src, n_nodes, n_mats);
}

void paste_superseded(const Node* nodes, int32_t levels, const PatchAnchor& a, const PasteTurn& rec, const PasteTree& src, uint64_t* n_nodes,
                      uint64_t* n_mats) {
    paste_superseded_as(nodes, levels, a, rec, src, n_nodes, n_mats);
}

void paste_superseded(const Node* nodes, int32_t levels, const PatchAnchor& a, const PasteRule& rec, const PasteTree& src, uint64_t* n_nodes,
                      uint64_t* n_mats) {
    paste_superseded_as(nodes, levels, a, rec, src, n_nodes, n_mats);
}

int list_box(int32_t levels, const int32_t* origin, int32_t nx, int32_t ny, int32_t nz, ListBox* B) {
    const int64_t E = (int64_t)1 << (2 * levels);
    if (!origin) {
        for (int a = 0; a < 3; a++) {
            B->lo[a] = 0;
            B->hi[a] = (int32_t)E;
        }
        return LIST_BOX_OK;
    }
    const int32_t dim[3] = {nx, ny, nz};
    for (int a = 0; a < 3; a++)
        if (dim[a] <= 0) return LIST_BOX_DIM;
    for (int a = 0; a < 3; a++) {
        if (origin[a] < 0 || (int64_t)origin[a] + dim[a] > E) return LIST_BOX_EXTENT;
        B->lo[a] = origin[a];
        B->hi[a] = origin[a] + dim[a];
    }
    return LIST_BOX_OK;
}

SchedPlan sched_decide(svo_tree::Sched& s, int64_t blocks, const int64_t sig[7], const float cam[6]) {
    if (s.blocks != blocks || !std::equal(sig, sig + 7, s.sig)) {
        s.blocks = blocks;
        std::copy(sig, sig + 7, s.sig);
        s.primed = false;
    }
    const auto close = [&](const float* c) {
        const float dx = cam[0] - c[0], dy = cam[1] - c[1], dz = cam[2] - c[2];
        return dx * dx + dy * dy + dz * dz <= kSchedMove * kSchedMove && cam[3] * c[3] + cam[4] * c[4] + cam[5] * c[5] >= kSchedTurnCos;
    };
    const bool near_last = close(s.last_cam);          // (a frame far from the last one is not sorted after)
    const bool near_sorted = s.primed && close(s.cam);  // (the order is used only near the frame it was sorted from)
    std::copy(cam, cam + 6, s.last_cam);
    if (!near_last) {  // (a moving camera: no sort after this frame; the first frame near it sorts for the next)
        s.primed = false;
        return SchedPlan{near_sorted, false, false};
    }
    // sorted after this frame: an order missing or sorted from a camera this one has drifted from, else every
    // kSchedEvery-th frame.  Only the frames sorted after write their durations, so the stored order is always the sort of
    // the stored durations (svo_tree_schedule)
    const bool sort = !near_sorted || ++s.since >= kSchedEvery;
    if (sort) {
        s.since = 0;
        std::copy(cam, cam + 6, s.cam);
    }
    return SchedPlan{near_sorted, sort, sort};
}

}  // namespace svo

// frames of a frame-mode desc (validated: 1 .. SVO_MAX_FRAMES, origins given for more than one)
static int desc_frames(const svo_cast_desc* d, const char* fn, int32_t* nf) {
    *nf = d->n_frames <= 1 ? 1 : d->n_frames;
    if (d->n_frames < 0 || d->n_frames > SVO_MAX_FRAMES) SVO_FAIL(SVO_EINVAL, std::string(fn) + ": n_frames outside [0, SVO_MAX_FRAMES]");
    if (d->n_frames > 1 && !d->frame_origins) SVO_FAIL(SVO_EINVAL, std::string(fn) + ": n_frames > 1 without frame_origins");
    return SVO_OK;
}

extern "C" int svo_cast_blocks(const svo_cast_desc* d, int64_t* n) {
    if (!d || !n) SVO_FAIL(SVO_EINVAL, "svo_cast_blocks: NULL argument");
    if (d->ray_dirs) {
        *n = d->n_rays > 0 ? ((int64_t)d->n_rays + 63) / 64 : 0;
        return SVO_OK;
    }
    if (d->width <= 0 || d->height <= 0 || d->tile_row_step <= 0 || d->tile_row_start < 0)
        SVO_FAIL(SVO_EINVAL, "svo_cast_blocks: bad frame geometry");
    int32_t nf = 1;
    int rc = desc_frames(d, "svo_cast_blocks", &nf);
    if (rc) return rc;
    const int32_t tile_rows = (d->height + 7) / 8;
    const int64_t rows = d->tile_row_start < tile_rows ? (tile_rows - d->tile_row_start + d->tile_row_step - 1) / d->tile_row_step : 0;
    const int32_t lh = svo::frame_wave_lh(d->flags), cols = svo::frame_wave_cols(d->width, lh);
    *n = (rows + svo::frame_half_rows((int32_t)rows, d->flags, lh, cols, nf)) * cols * nf;
    return SVO_OK;
}

extern "C" int svo_cast_count(const svo_cast_desc* d, int64_t* n) {
    if (!d || !n) SVO_FAIL(SVO_EINVAL, "svo_cast_count: NULL argument");
    if (d->ray_dirs) {
        *n = d->n_rays;
        return SVO_OK;
    }
    if (d->width <= 0 || d->height <= 0 || d->tile_row_step <= 0 || d->tile_row_start < 0)
        SVO_FAIL(SVO_EINVAL, "svo_cast_count: bad frame geometry");
    int32_t nf = 1;
    int rc = desc_frames(d, "svo_cast_count", &nf);
    if (rc) return rc;
    const int32_t tile_rows = (d->height + 7) / 8;
    int64_t rows = 0;
    for (int32_t r = d->tile_row_start; r < tile_rows; r += d->tile_row_step) rows += std::min(8, d->height - r * 8);
    *n = rows * d->width * nf;
    return SVO_OK;
}
