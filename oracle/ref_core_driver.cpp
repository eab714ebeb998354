// ORACLE (test infrastructure only): a command interpreter over the reference's own voxel tree, world generator and
// CPU ray caster, linked with the reference's translation units where they lie into oracle/_ref/ref_core
// (oracle/Makefile; the stand-in headers of oracle/ref_stub/ take the place of GLM / GLEW / GLFW / Win32).
// Nothing here restates reference code: it calls initTetraHexaTree, genWorld, putBlock, getBlock, deleteBlock,
// allocNode, allocArray and RAY_CASTER::castRayFromCam, and reads the allocator's counters.
//
//   ref_core <command file> <result file>
//
// Both files are little-endian u32 words.  A command is CMD_WORDS words {op, a1 ..}, a result RES_WORDS words
// {op, r1 ..}; every command writes one result, zeros where it has nothing to report:
//   OP_INIT                                  initTetraHexaTree()
//   OP_CLEAN                                 an empty root from allocNode() + allocArray() (orc_init_clean_root's analogue)
//   OP_GEN                                   genWorld()
//   OP_PUT    x y z level flags clo chi meta putBlock
//   OP_GET    x y z                          getBlock                -> flags clo chi meta
//   OP_DELETE x y z level                    deleteBlock             -> flags clo chi meta (the returned Block)
//   OP_CAST   ox oy oz dx dy dz steps        cameraPos / cameraDir from the six f32 bit patterns, castRayFromCam(steps)
//                                            -> pos[3] lastPos[3] steps, then getBlock(pos): flags clo chi meta
//   OP_POOLS                                 -> nodeNextAllocIndex arrayNextAllocIndex nodeFreeListPop arrayFreeListPop
//   OP_ROOT                                  -> root flags, bitmap lo hi, children
//   OP_BOX    x0 y0 z0 nx ny nz              -> the voxel count, and after this result 3 words {flags clo chi} per voxel:
//                                            getBlock over the box, z outermost, x innermost
// One process is one world: the reference's state is global.  The reference prints to stdout, some of it
// unconditionally, so stdout goes to /dev/null here and DEBUG_LEVEL to 0.  castRayFromCam leaves lastPos without a
// value when the budget is 0 (its loop body never runs): such a result carries zeros there.  A getBlock that reaches
// the maximum depth ends the process with exit(1), inside the reference.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "globals.hpp"
#include "ray_caster.hpp"
#include "voxel_data/tetrahexa_tree.hpp"
#include "voxel_data/voxel_allocator.hpp"
#include "world_gen.hpp"

enum { OP_INIT = 1, OP_CLEAN, OP_GEN, OP_PUT, OP_GET, OP_DELETE, OP_CAST, OP_POOLS, OP_ROOT, OP_BOX };
enum { CMD_WORDS = 10, RES_WORDS = 12 };

static float f32_of(uint32_t bits) {
    float f;
    memcpy(&f, &bits, 4);
    return f;
}

static uint32_t bits_of(float f) {
    uint32_t b;
    memcpy(&b, &f, 4);
    return b;
}

static void put_block_words(uint32_t* r, const Block& b) {
    r[0] = b.flags;
    r[1] = (uint32_t)(b.color & 0xFFFFFFFFull);
    r[2] = (uint32_t)(b.color >> 32);
    r[3] = bits_of(b.metadata);
}

int main(int argc, char** argv) {
    if (argc != 3) {
        fprintf(stderr, "usage: ref_core <command file> <result file>\n");
        return 2;
    }
    FILE* in = fopen(argv[1], "rb");
    if (!in) {
        fprintf(stderr, "ref_core: cannot read %s\n", argv[1]);
        return 2;
    }
    std::vector<uint32_t> cmd;
    uint32_t buf[CMD_WORDS * 1024];
    size_t got;
    while ((got = fread(buf, 4, CMD_WORDS * 1024, in)) > 0) cmd.insert(cmd.end(), buf, buf + got);
    fclose(in);
    if (cmd.size() % CMD_WORDS) {
        fprintf(stderr, "ref_core: %s is not a whole number of commands\n", argv[1]);
        return 2;
    }
    FILE* out = fopen(argv[2], "wb");
    if (!out) {
        fprintf(stderr, "ref_core: cannot write %s\n", argv[2]);
        return 2;
    }
    if (!freopen("/dev/null", "w", stdout)) return 2;
    DEBUG_LEVEL = 0;

    const size_t n = cmd.size() / CMD_WORDS;
    std::vector<uint32_t> res;
    res.reserve(n * RES_WORDS);
    for (size_t i = 0; i < n; i++) {
        const uint32_t* a = &cmd[i * CMD_WORDS];
        uint32_t r[RES_WORDS] = {a[0]};
        std::vector<uint32_t> more;
        const Pos p = Pos{(int)a[1], (int)a[2], (int)a[3]};
        switch (a[0]) {
        case OP_INIT:
            initTetraHexaTree();
            break;
        case OP_CLEAN: {
            root = allocNode();
            Ptr arr = allocArray();
            memset(arr.ptr, 0, sizeof(u32) * 64);
            root.ptr->branch.bitmap = 0;
            root.ptr->branch.flags = 0;
            root.ptr->branch.children = arr.index;
            break;
        }
        case OP_GEN:
            genWorld();
            break;
        case OP_PUT: {
            Block b;
            b.flags = a[5];
            b.color = (u64)a[6] | ((u64)a[7] << 32);
            b.metadata = f32_of(a[8]);
            putBlock(p, b, (int)a[4]);
            break;
        }
        case OP_GET:
            put_block_words(r + 1, getBlock(p));
            break;
        case OP_DELETE:
            put_block_words(r + 1, deleteBlock(p, (int)a[4]));
            break;
        case OP_CAST: {
            const int steps = (int)a[7];
            if (steps < 0) {
                fprintf(stderr, "ref_core: command %zu: a negative budget never ends\n", i);
                return 2;
            }
            cameraPos = glm::vec3(f32_of(a[1]), f32_of(a[2]), f32_of(a[3]));
            cameraDir = glm::vec3(f32_of(a[4]), f32_of(a[5]), f32_of(a[6]));
            RayResult rr = RAY_CASTER::castRayFromCam(steps);
            r[1] = (uint32_t)rr.pos.x;
            r[2] = (uint32_t)rr.pos.y;
            r[3] = (uint32_t)rr.pos.z;
            if (steps > 0) {
                r[4] = (uint32_t)rr.lastPos.x;
                r[5] = (uint32_t)rr.lastPos.y;
                r[6] = (uint32_t)rr.lastPos.z;
            }
            r[7] = (uint32_t)rr.steps;
            put_block_words(r + 8, getBlock(Pos{rr.pos.x, rr.pos.y, rr.pos.z}));
            break;
        }
        case OP_POOLS:
            r[1] = nodeNextAllocIndex;
            r[2] = arrayNextAllocIndex;
            r[3] = (uint32_t)nodeFreeListPop;
            r[4] = (uint32_t)arrayFreeListPop;
            break;
        case OP_ROOT:
            r[1] = root.ptr->branch.flags;
            r[2] = (uint32_t)(root.ptr->branch.bitmap & 0xFFFFFFFFull);
            r[3] = (uint32_t)(root.ptr->branch.bitmap >> 32);
            r[4] = root.ptr->branch.children;
            break;
        case OP_BOX: {
            const int nx = (int)a[4], ny = (int)a[5], nz = (int)a[6];
            if (nx < 0 || ny < 0 || nz < 0 || (int64_t)nx * ny * nz > (1 << 26)) {
                fprintf(stderr, "ref_core: command %zu: box too large\n", i);
                return 2;
            }
            r[1] = (uint32_t)(nx * ny * nz);
            more.reserve((size_t)r[1] * 3);
            for (int z = 0; z < nz; z++)
                for (int y = 0; y < ny; y++)
                    for (int x = 0; x < nx; x++) {
                        uint32_t w[4];
                        put_block_words(w, getBlock(Pos{p.x + x, p.y + y, p.z + z}));
                        more.insert(more.end(), w, w + 3);
                    }
            break;
        }
        default:
            fprintf(stderr, "ref_core: command %zu: unknown op %u\n", i, a[0]);
            return 2;
        }
        res.insert(res.end(), r, r + RES_WORDS);
        res.insert(res.end(), more.begin(), more.end());
    }
    if (fwrite(res.data(), 4, res.size(), out) != res.size() || fclose(out) != 0) {
        fprintf(stderr, "ref_core: short write to %s\n", argv[2]);
        return 2;
    }
    return 0;
}
