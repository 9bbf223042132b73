// The placement's kernels (gfx950): a resident tree resampled under a rotation, a uniform scale and a translation, level by level
// from the root, into a new tree in breadth-first order.  k_place_emit is not a template: included by place.hip ONLY.
//
// The arithmetic is the contract of include/sdfhip.h (sdfhip_scene_place) and DESIGN.md section 8 (N11): fp32, each operation rounded
// on its own, in the order written (-ffp-contract=off); tests/place_restatement.py restates it with numpy.  The source's distance is
// what k_query_sample reads (find_fresh + sample_after_find, raymarch_device.h, untouched), the construct rule and the point lattice
// of a block of eight siblings are k_tri_eval's (trigen_kernels.h), the splits are ranked by the shared bitmap scan (scan_device.h).
//
// A BLOCK is the eight children of one node (the root's block: the root alone, as child 0 of a cell of edge 2 at the origin).  Its
// 35 points are the 27 corners of its 3x3x3 lattice (spacing S, the children's edge) and the 8 child centres: every corner and
// centre of the eight siblings, each looked up once.  A wave takes a block, lane = point: the look-ups of a wave are those of eight
// neighbouring cells, and a level's blocks follow in the order of their parents, which is the order of the level above in space.
#pragma once
#include "query_kernels.h"   // QueryScene, grid_of; raymarch_device.h: the cursors, find_fresh, sample_after_find
#include "sdf_bytes.h"
#include "scan_device.h"     // k_rank_scan_*, rank_in_bitmap

namespace sdfhip {

constexpr int PLACE_POINTS = 35;
constexpr int PLACE_THREADS = 256;        // four waves, a block of siblings each: 32 nodes, one word of the split bitmap

// p = s R x + t, as the kernels use it: R row-major, inv = 1.0f / s (one IEEE division, on the host)
struct PlaceMap {
    float r[3][3];
    float s, inv;
    float tx, ty, tz;
};

// A block's parent cell: its integer coordinates at its own depth (< 2^11), {x | y << 16, z}
typedef uint2 PlaceBlock;

// value(p) of the rule: the inverse map, the clamp to the source's cube, the source's distance there (what sdfhip_scene_sample
// returns), continued outside the cube at slope 1 from the nearest point of its surface, times s.  Inside the cube e is 0 and the
// value is D * s bit for bit (x + 0 = x, sqrtf(0) = 0).  The clamped point lies in [0, 1]^3 whatever the arguments are (fmaxf / fminf
// take a NaN to 0), so the look-up never leaves the source's arrays.
template <class CursorT>
__device__ __forceinline__ float place_value(const QueryScene &Q, const PlaceMap &M, float px, float py, float pz)
{
    const float d0 = px - M.tx, d1 = py - M.ty, d2 = pz - M.tz;
    const float qx = ((M.r[0][0] * d0 + M.r[1][0] * d1) + M.r[2][0] * d2) * M.inv;
    const float qy = ((M.r[0][1] * d0 + M.r[1][1] * d1) + M.r[2][1] * d2) * M.inv;
    const float qz = ((M.r[0][2] * d0 + M.r[1][2] * d1) + M.r[2][2] * d2) * M.inv;
    const float cx = __builtin_fminf(__builtin_fmaxf(qx, 0.0f), 1.0f);
    const float cy = __builtin_fminf(__builtin_fmaxf(qy, 0.0f), 1.0f);
    const float cz = __builtin_fminf(__builtin_fmaxf(qz, 0.0f), 1.0f);
    const float ex = qx - cx, ey = qy - cy, ez = qz - cz;
    CursorT c;
    c.loads = 0;
    c.reset(Q.nodes[0]);
    typename CursorT::Pos u;
    find_fresh(c, Q.nodes, grid_of(Q), Q.n_nodes, nullptr, 0u, cx, cy, cz, u);
    const float D = sample_after_find(c, u, cx, cy, cz);
    return (D + sqrtf((ex * ex + ey * ey) + ez * ez)) * M.s;
}

// Pass 1 of a level (its nblocks blocks of nchild nodes -- 8, or 1 for the root -- cells of edge S): a wave per block, lane p < 35
// looks point p up; then lane c < nchild gathers child c's eight corner values from the lattice (wave shuffles) and stores its bytes
// as one 8-byte word, V[8 b + c] (V: the level's first node), and the block's split flags -- fabsf(value(centre)) < 2 S, above the
// depth limit -- leave as one byte of the level's bitmap, split[b]: node 8 b + c is bit 8 b + c, so a workgroup's four waves fill
// one 32-bit word and the bitmap needs no clearing (the bytes behind the last block are masked by PlaceSplitWords).  The loop's
// bound is wave-uniform: the lanes are together at the shuffles and the ballot.
template <class CursorT>
__global__ __launch_bounds__(PLACE_THREADS) void k_place_level(QueryScene Q, PlaceMap M, const PlaceBlock *__restrict__ blocks, uint32_t nblocks,
                                                               uint32_t nchild, float S, int may_split, uint2 *__restrict__ V,
                                                               uint8_t *__restrict__ split)
{
    constexpr uint32_t WAVES = PLACE_THREADS / 64;
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t li = lane % 3u, lj = lane / 3u % 3u, lk = lane / 9u;           // the lattice corner of a lane < 27
    const uint32_t c = lane & 7u, ci = c & 1u, cj = c >> 1 & 1u, ck = c >> 2;     // the child of a lane >= 27, and of a lane < 8
    for (uint32_t b = blockIdx.x * WAVES + wave; b < nblocks; b += gridDim.x * WAVES) {
        const PlaceBlock B = blocks[b];
        const uint32_t bx = B.x & 0xFFFFu, by = B.x >> 16, bz = B.y;
        // the root's block: the root's own eight corners and its centre
        const bool wanted = nchild == 8u ? lane < (uint32_t)PLACE_POINTS : lane < 27u ? (li < 2u && lj < 2u && lk < 2u) : lane == 27u;
        float value = 0.0f;
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
            value = place_value<CursorT>(Q, M, px, py, pz);
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
    }
}

// The split bitmap of a level of n nodes, words 0 .. ceil(n / 32) - 1, to k_rank_scan_words (scan_device.h): the bits from n on
// were never written
struct PlaceSplitWords {
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
__global__ __launch_bounds__(256) void k_place_emit(const PlaceBlock *__restrict__ blocks, uint32_t n, uint32_t nchild, uint32_t first,
                                                    const uint32_t *__restrict__ split, const uint32_t *__restrict__ pre,
                                                    const uint32_t *__restrict__ chunk, int2 *__restrict__ links, uint32_t cap_out,
                                                    PlaceBlock *__restrict__ next, uint32_t cap_next)
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
            const PlaceBlock B = blocks[nchild == 8u ? t >> 3 : 0u];
            const uint32_t c = nchild == 8u ? t & 7u : 0u;
            const uint32_t x = 2u * (B.x & 0xFFFFu) + (c & 1u), y = 2u * (B.x >> 16) + (c >> 1 & 1u), z = 2u * B.y + (c >> 2);
            next[r] = make_uint2(x | y << 16, z);
        }
    }
}

}  // namespace sdfhip
