// The device side that every lattice builder shares (gfx950): a tree built level by level from the root, in breadth-first order,
// from a value(p) that each builder brings.  Who uses what:
//   level_body       the first pass of a level, a template on the value: k_place_level (place_kernels.h, the placement's map),
//                    k_offset_level (distance_kernels.h, dist - delta or the shell) and k_blend_level (blend_kernels.h, the blend of
//                    two distances) are one-line wrappers round it
//   LevelSplitWords  the level's split bitmap as the shared bitmap scan reads it (scan_device.h's k_rank_scan_*)
//   k_level_emit     the second pass: the links and the next level's blocks
// The host's loop over the levels -- these two passes, the scan between them, the arrays that grow -- is level_build.h's
// build_levels, which place.hip, distance.hip and blend.hip call.  k_level_emit is not a template: it is `static`, so each of the
// three translation units has its own.  Nothing here knows a scene: the search, the cursors and the tetrahedra stay with the values.
//
// The construct rule is sdfhip_trimesh_build's: byte = FromFloat(value(corner), S), a node splits iff
// fabsf(value(centre)) < 2 S above the depth limit; fp32, each operation rounded on its own, in the order written.
//
// A BLOCK is the eight children of one node (the root's block: the root alone, as child 0 of a cell of edge 2 at the origin).  Its
// 35 points are the 27 corners of its 3x3x3 lattice (spacing S, the children's edge) and the 8 child centres: every corner and
// centre of the eight siblings, each looked up once.  A wave takes a block, lane = point: the look-ups of a wave are those of eight
// neighbouring cells, and a level's blocks follow in the order of their parents, which is the order of the level above in space.
#pragma once
#include "sdf_bytes.h"       // from_float
#include "scan_device.h"     // rank_in_bitmap
#include <hip/hip_vector_types.h>

namespace sdfhip {

constexpr int LEVEL_POINTS = 35;
constexpr int LEVEL_THREADS = 256;        // four waves, a block of siblings each: 32 nodes, one word of the split bitmap

// A block's parent cell: its integer coordinates at its own depth (< 2^11), {x | y << 16, z}
typedef uint2 LevelBlock;

// Pass 1 of a level (its nblocks blocks of nchild nodes -- 8, or 1 for the root -- cells of edge S): a wave per block, lane p < 35
// looks point p up; then lane c < nchild gathers child c's eight corner values from the lattice (wave shuffles) and stores its bytes
// as one 8-byte word, V[8 b + c] (V: the level's first node), and the block's split flags leave as one byte of the level's bitmap,
// split[b]: node 8 b + c is bit 8 b + c, so a workgroup's four waves fill one 32-bit word and the bitmap needs no clearing (the
// bytes behind the last block are masked by LevelSplitWords).  The loop's bound is wave-uniform: the lanes are together at the
// shuffles and the ballot.
// Value: SOURCES, the number of surfaces a point is searched against (0: none, and nothing is counted); value_of(px, py, pz,
// lane_stack, seen) -> value(p), which adds the records each search loaded to seen[0 .. SOURCES - 1]; value_of.visited, SOURCES
// counters in device memory: the records the level's searches loaded, added up per block in 64 bits.  lane_stack: the lane's slice
// of its workgroup's search stack, handed on to value_of untouched (nullptr where the value searches nothing).
template <class Value>
__device__ __forceinline__ void level_body(const Value &value_of, const LevelBlock *__restrict__ blocks, uint32_t nblocks, uint32_t nchild, float S,
                                           int may_split, uint2 *__restrict__ V, uint8_t *__restrict__ split, uint2 *lane_stack)
{
    constexpr uint32_t WAVES = LEVEL_THREADS / 64;
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t li = lane % 3u, lj = lane / 3u % 3u, lk = lane / 9u;           // the lattice corner of a lane < 27
    const uint32_t c = lane & 7u, ci = c & 1u, cj = c >> 1 & 1u, ck = c >> 2;     // the child of a lane >= 27, and of a lane < 8
    for (uint32_t b = blockIdx.x * WAVES + wave; b < nblocks; b += gridDim.x * WAVES) {
        const LevelBlock B = blocks[b];
        const uint32_t bx = B.x & 0xFFFFu, by = B.x >> 16, bz = B.y;
        // the root's block: the root's own eight corners and its centre
        const bool wanted = nchild == 8u ? lane < (uint32_t)LEVEL_POINTS : lane < 27u ? (li < 2u && lj < 2u && lk < 2u) : lane == 27u;
        float value = 0.0f;
        uint32_t seen[Value::SOURCES ? Value::SOURCES : 1] = {};
        if (wanted) {
            float px, py, pz;
            if (lane < 27u) {
                px = (float)(2u * bx + li) * S; py = (float)(2u * by + lj) * S; pz = (float)(2u * bz + lk) * S;
            } else {
                const uint32_t m = (lane - 27u) & 7u;
                const float H = S * 0.5f;
                px = (float)(2u * (2u * bx + (m & 1u)) + 1u) * H;
                py = (float)(2u * (2u * by + (m >> 1 & 1u)) + 1u) * H;
                pz = (float)(2u * (2u * bz + (m >> 2)) + 1u) * H;
            }
            value = value_of(px, py, pz, lane_stack, seen);
        }
        uint32_t w[2] = { 0u, 0u };
#pragma unroll
        for (int k = 0; k < 8; k++) {
            const int src = (int)((ci + (uint32_t)(k & 1)) + 3u * (cj + (uint32_t)(k >> 1 & 1)) + 9u * (ck + (uint32_t)(k >> 2 & 1)));
            w[k >> 2] |= from_float(__shfl(value, src), S) << (8 * (k & 3));
        }
        const float cv = fabsf(__shfl(value, 27 + (int)c));
        const bool splits = lane < nchild && may_split && cv < 2.0f * S;
        const unsigned long long mask = __ballot(splits);
        if (lane < nchild) V[8ull * b + lane] = make_uint2(w[0], w[1]);
        if (lane == 0) split[b] = (uint8_t)mask;
        // the block's records, added once per block and source: a search may load up to n_nodes < 2^31 of them, so the wave's sum is
        // made of the lanes' low and high 16 bits apart (each below 2^22) and put together in 64 bits
        if constexpr (Value::SOURCES > 0) {
#pragma unroll
            for (int s = 0; s < Value::SOURCES; s++) {
                uint32_t lo = seen[s] & 0xFFFFu, hi = seen[s] >> 16;
#pragma unroll
                for (int o = 32; o >= 1; o >>= 1) { lo += (uint32_t)__shfl_xor((int)lo, o); hi += (uint32_t)__shfl_xor((int)hi, o); }
                if (lane == 0 && (lo | hi)) atomicAdd(value_of.visited + s, ((unsigned long long)hi << 16) + lo);
            }
        }
    }
}

// The split bitmap of a level of n nodes, words 0 .. ceil(n / 32) - 1, to k_rank_scan_words (scan_device.h): the bits from n on
// were never written
struct LevelSplitWords {
    const uint32_t *split;
    uint32_t n;
    __device__ __forceinline__ uint32_t operator()(uint32_t i) const
    {
        const uint32_t rest = n - 32u * i;
        return rest >= 32u ? split[i] : split[i] & ((1u << rest) - 1u);
    }
};

// Pass 2 of a level (its n nodes; the result's nodes first .. first + n - 1): eight lanes per node, lane i the node's child i.  A
// splitting node of rank r (the splits before it in the level's order, = the order of the result's indices) gets the block
// first + n + 8 r, appended behind the level: its children link, the eight children's {parent, -1}, and the next level's block r with
// the node's own coordinates.  cap_out / cap_next: the room in links[] and next[].
static __global__ __launch_bounds__(256) void k_level_emit(const LevelBlock *__restrict__ blocks, uint32_t n, uint32_t nchild, uint32_t first,
                                                           const uint32_t *__restrict__ split, const uint32_t *__restrict__ pre,
                                                           const uint32_t *__restrict__ chunk, int2 *__restrict__ links, uint32_t cap_out,
                                                           LevelBlock *__restrict__ next, uint32_t cap_next)
{
    const uint64_t total = 8ull * n;
    for (uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; j < total; j += (uint64_t)gridDim.x * blockDim.x) {
        const uint32_t t = (uint32_t)(j >> 3), i = (uint32_t)j & 7u;
        const uint32_t word = split[t >> 5];
        if (!((word >> (t & 31u)) & 1u)) continue;
        const uint32_t r = rank_in_bitmap(chunk, pre, t >> 5, word, t & 31u);
        const uint32_t self = first + t;
        const uint64_t child = (uint64_t)first + n + 8ull * r + i;
        if (child >= cap_out || r >= cap_next) continue;                       // (a guard: the host sized both from the scan's total)
        links[child] = make_int2((int32_t)self, -1);
        if (i == 0) {
            links[self].y = (int32_t)child;
            const LevelBlock B = blocks[nchild == 8u ? t >> 3 : 0u];
            const uint32_t c = nchild == 8u ? t & 7u : 0u;
            const uint32_t x = 2u * (B.x & 0xFFFFu) + (c & 1u), y = 2u * (B.x >> 16) + (c >> 1 & 1u), z = 2u * B.y + (c >> 2);
            next[r] = make_uint2(x | y << 16, z);
        }
    }
}

}  // namespace sdfhip
