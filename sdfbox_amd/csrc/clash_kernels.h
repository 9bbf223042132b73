// The clash check of an assembly of placed instances (gfx950): k_clash_init (the pair table) and k_clash (one pass over a cubic
// lattice: which instances contain each point, and per pair of instances the count, the lowest index, the bounds and the coordinate
// sums of the points both contain).  Host side, C ABI: clash.hip.
//
// Replaces: nothing in the reference's code -- its shader marches ONE immutable tree and knows no parts.
//
// The rule is the contract of include/sdfhip.h (sdfhip_instances_clash) and DESIGN.md section 8 (N19): fp32, each operation rounded
// on its own, in the order written; tests/clash_restatement.py restates it with numpy on place_restatement.value.
//   p_a       fmaf((float)i_a + 0.5f, pitch, origin_a) for the lattice point (x, y, z), 0 <= x, y, z < 2^d, pitch = side * 2^-d
//   index     (z << 2d) | (y << d) | x
//   contains  instance k contains p iff u_k(p) < 0, u_k = compose_instance_value (sdfhip_scene_place's value); the ops are ignored
//   pair      for a < b: points = #{p : both contain p}, first = the lowest index among them, lo / hi their inclusive bounds, sum the
//             sums of their x, y and z.  Everything is an integer, accumulated with integer atomicAdd / atomicMin / atomicMax only: the
//             bytes do not depend on the order in which the waves arrive
//
// The exact skip.  b_k = place_lower_bound (compose_instance.h; instances_kernels.h has the argument) is (-0.5625f + e) * s <= u_k with no error
// term, so b_k >= 0 implies u_k >= 0: the instance does not contain the point and is not looked up.  The test is written
// !(b_k >= 0): a NaN bound is looked up (and its NaN value contains nothing).  No margin is involved, so the skip changes no byte of
// any record (tests/test_gpu_clash.py runs every case with and without it).
//
// Shape.  A wave is a 4 x 4 x 4 block of the lattice, lane = lz * 16 + ly * 4 + lx; a workgroup is four blocks that follow each other
// in block order (x fastest).  At d < 2 the one block is partial: lanes outside the lattice stay in the wave (the ballots below need
// no special case) and are candidates of nothing.
//   1  candidates: the instance loop is wave-uniform, every lane computes b_k and keeps a 64-bit candidate mask; the ballot of each
//      instance's candidates gives the wave's OR mask in scalar registers.  A wave whose OR mask names fewer than two instances
//      returns: no pair can have a point in it, and nothing was looked up
//   2  look-ups: wave-uniform over the bits of the OR mask; the lanes whose candidate bit is set look u_k up and keep a 64-bit
//      containment mask.  The ballot of u_k < 0 gives the wave's containment OR mask
//   3  pairs: wave-uniform over the pairs a < b of the containment OR mask: both = ballot(bit a) & ballot(bit b).  Because the lane
//      number IS the point's place in the block, everything the record needs comes from that one 64-bit scalar without a cross-lane
//      reduction: the count is its popcount, the lowest index belongs to its lowest set lane (the index is monotone in the lane), the
//      bounds and sums follow from its intersections with the twelve masks "lx = j", "ly = j", "lz = j".  Lane 0 issues the eleven
//      atomics of the pair
// SDFHIP_CLASH_NO_SKIP makes every lane inside the lattice a candidate of every instance; steps 2 and 3 are the same code.
// No coarser pre-reject (a 16^3 block's centre bound minus its half-diagonal) is built: it needs a rounding margin argued on its own
// and an A/B to keep it, and step 1 already costs a wave about thirty VALU operations per instance and no memory access.
// The look-up counters go to CLASH_STAT_SLOTS slots by block number, so that a lattice of 2^18 blocks does not queue on one address.
#pragma once
#include "compose_instance.h"   // ComposeInstance, compose_instance_value, place_lower_bound; place_kernels.h, query_kernels.h
#include "scan_device.h"        // block_axis (shared with components_kernels.h)

namespace sdfhip {

constexpr int CLASH_THREADS = 256;
constexpr uint32_t CLASH_MAX_INSTANCES = 64, CLASH_STAT_SLOTS = 64;

// sdfhip_clash of include/sdfhip.h, and one entry of the pair table
struct ClashPair {
    uint32_t a, b, points, first;
    uint32_t lo[3], hi[3];
    unsigned long long sum[3];
};
static_assert(sizeof(ClashPair) == 64, "sdfhip_clash of include/sdfhip.h");

struct ClashStat {
    unsigned long long lookups;
    uint32_t blocks_looked, pad;
};

// the call's lattice as the kernel reads it
struct ClashLattice {
    float ox, oy, oz, pitch;
    uint32_t depth;         // 0..10
    uint32_t n_blocks;      // 8^max(depth - 2, 0)
    uint32_t n_instances;   // 1..64
    uint32_t skip;          // 0: SDFHIP_CLASH_NO_SKIP
};

// entry a * K - a (a + 1) / 2 + (b - a - 1) of the table is pair (a, b), a < b < K: the table's order is the records' order
__device__ __forceinline__ uint32_t clash_pair_index(uint32_t a, uint32_t b, uint32_t K) { return a * K - a * (a + 1u) / 2u + (b - a - 1u); }

// the table empty, and the counters zero: one thread per pair
__global__ __launch_bounds__(CLASH_THREADS) void k_clash_init(ClashPair *__restrict__ pairs, uint32_t K, ClashStat *__restrict__ stats)
{
    const uint32_t i = blockIdx.x * CLASH_THREADS + threadIdx.x;
    if (i < CLASH_STAT_SLOTS) stats[i] = ClashStat{0ull, 0u, 0u};
    if (i >= K * K) return;
    const uint32_t a = i / K, b = i % K;
    if (a >= b) return;
    ClashPair P;
    P.a = a; P.b = b; P.points = 0u; P.first = 0xFFFFFFFFu;
    for (int k = 0; k < 3; k++) { P.lo[k] = 0xFFFFFFFFu; P.hi[k] = 0u; P.sum[k] = 0ull; }
    pairs[clash_pair_index(a, b, K)] = P;
}

__global__ __launch_bounds__(CLASH_THREADS) void k_clash(const ComposeInstance *__restrict__ table, ClashLattice L, ClashPair *__restrict__ pairs,
                                                         ClashStat *__restrict__ stats)
{
    const uint32_t block = blockIdx.x * (CLASH_THREADS / 64) + (threadIdx.x >> 6);      // wave-uniform
    if (block >= L.n_blocks) return;
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t d = L.depth, bd = d > 2u ? d - 2u : 0u, bmask = (1u << bd) - 1u;
    const uint32_t bx = (block & bmask) * 4u, by = ((block >> bd) & bmask) * 4u, bz = (block >> (2u * bd)) * 4u;
    const uint32_t x = bx + (lane & 3u), y = by + ((lane >> 2) & 3u), z = bz + (lane >> 4);
    const uint32_t side = 1u << d;
    const bool inside = x < side && y < side && z < side;
    const float px = __builtin_fmaf((float)x + 0.5f, L.pitch, L.ox), py = __builtin_fmaf((float)y + 0.5f, L.pitch, L.oy),
                pz = __builtin_fmaf((float)z + 0.5f, L.pitch, L.oz);
    const uint32_t K = L.n_instances;

    // 1  candidates
    unsigned long long cand = 0ull, wave_cand = 0ull;
    for (uint32_t k = 0; k < K; k++) {
        bool c = inside;
        if (L.skip) c = c && !(place_lower_bound(table[k].M, px, py, pz) >= 0.0f);
        if (c) cand |= 1ull << k;
        if (__ballot(c)) wave_cand |= 1ull << k;
    }
    if (L.skip && __popcll(wave_cand) < 2) return;

    // 2  look-ups
    unsigned long long held = 0ull, wave_held = 0ull, lookups = 0ull;
    for (unsigned long long left = wave_cand; left; left &= left - 1ull) {
        const uint32_t k = (uint32_t)__ffsll((long long)left) - 1u;
        const bool c = (cand >> k) & 1ull;
        bool in = false;
        if (c) in = compose_instance_value(table[k], px, py, pz) < 0.0f;
        if (in) held |= 1ull << k;
        lookups += (unsigned long long)__popcll(__ballot(c));
        if (__ballot(in)) wave_held |= 1ull << k;
    }
    if (lane == 0u && lookups) {
        ClashStat *s = stats + (block & (CLASH_STAT_SLOTS - 1u));
        atomicAdd(&s->lookups, lookups);
        atomicAdd(&s->blocks_looked, 1u);
    }

    // 3  pairs
    for (unsigned long long la = wave_held; la; la &= la - 1ull) {
        const uint32_t a = (uint32_t)__ffsll((long long)la) - 1u;
        const unsigned long long ma = __ballot((held >> a) & 1ull);
        for (unsigned long long lb = la & (la - 1ull); lb; lb &= lb - 1ull) {
            const uint32_t b = (uint32_t)__ffsll((long long)lb) - 1u;
            const unsigned long long both = ma & __ballot((held >> b) & 1ull);
            if (!both) continue;
            const uint32_t n = (uint32_t)__popcll(both), low = (uint32_t)__ffsll((long long)both) - 1u;
            uint32_t lo[3], hi[3], sum[3];
            block_axis(both, 0x1111111111111111ull, 1, lo[0], hi[0], sum[0]);
            block_axis(both, 0x000F000F000F000Full, 4, lo[1], hi[1], sum[1]);
            block_axis(both, 0x000000000000FFFFull, 16, lo[2], hi[2], sum[2]);
            if (lane == 0u) {
                const uint32_t base[3] = {bx, by, bz};
                const uint32_t first = ((bz + (low >> 4)) << (2u * d)) | ((by + ((low >> 2) & 3u)) << d) | (bx + (low & 3u));
                ClashPair *P = pairs + clash_pair_index(a, b, K);
                atomicAdd(&P->points, n);
                atomicMin(&P->first, first);
                for (int k = 0; k < 3; k++) {
                    atomicMin(&P->lo[k], base[k] + lo[k]);
                    atomicMax(&P->hi[k], base[k] + hi[k]);
                    atomicAdd(&P->sum[k], (unsigned long long)base[k] * n + sum[k]);
                }
            }
        }
    }
}

}  // namespace sdfhip
