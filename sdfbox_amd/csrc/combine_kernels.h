// The combination's kernels (gfx950): two resident trees walked together level by level from the root, the result's bytes a min or
// max of the operands' bytes at the same cell, its blocks placed by the shared bitmap scan (scan_device.h).  Non-template kernels:
// included by combine.hip ONLY.
//
// The arithmetic is the contract of include/sdfhip.h (sdfhip_scene_combine) and DESIGN.md section 8 (N10): fp32, each operation
// rounded on its own, in the order written (-ffp-contract=off); tests/combine_restatement.py restates it with numpy, level by level.
// Where an operand has no node at a cell its bytes are those k_edit_new gives a new child before the brush, and k_prune_decide compares
// a block with (to_float, trilerp, from_float: the same three functions), applied once per level below the operand's leaf.
#pragma once
#include "raymarch_device.h"
#include "sdf_bytes.h"
#include "sdf_interp.h"
#include "scan_device.h"     // k_rank_scan_*, rank_in_bitmap

namespace sdfhip {

constexpr uint32_t COMBINE_NONE = 0xFFFFFFFFu;      // an item's ia / ib where the operand has no node at the cell

// One cell of a level of the result: the operands' nodes there (or COMBINE_NONE) and their bytes at this cell, own or inherited
struct CombineItem {
    uint32_t ia, ib;
    uint2 va, vb;
};
static_assert(sizeof(CombineItem) == 24, "three 8-byte words");

__device__ __forceinline__ uint32_t combine_byte(uint2 v, int k) { return ((k < 4 ? v.x : v.y) >> (8 * (k & 3))) & 0xFFu; }

// The first child of the operand's node i, or COMBINE_NONE: the operand has no node here, the node is a leaf, or its link does not
// name a block inside the array (in range in every tree the upload calls consistent: a guard, not a case).  Both passes decide by
// this one function, so a cell splits in pass 1 exactly when pass 2 finds children to hand down.
__device__ __forceinline__ uint32_t combine_children(const NodeRec *__restrict__ nodes, uint32_t n, uint32_t i)
{
    if (i >= n) return COMBINE_NONE;
    const uint32_t first = nodes[i].y;
    return ((int32_t)first >= 0 && first < n && n - first >= 8u) ? first : COMBINE_NONE;
}

// neg(b) = from_float(-to_float(b, S), S) per byte: 63 <-> 64, the sign flips exactly at the surface
__device__ __forceinline__ uint2 combine_negate(uint2 v, float S)
{
    uint32_t w[2] = { 0u, 0u };
#pragma unroll
    for (int k = 0; k < 8; k++) w[k >> 2] |= from_float(-to_float(combine_byte(v, k), S), S) << (8 * (k & 3));
    return make_uint2(w[0], w[1]);
}

// per byte: min (UNION) or max (INTERSECT, SUBTRACT)
__device__ __forceinline__ uint2 combine_bytes(uint2 a, uint2 b, bool take_min)
{
    uint32_t w[2] = { 0u, 0u };
#pragma unroll
    for (int k = 0; k < 8; k++) {
        const uint32_t x = combine_byte(a, k), y = combine_byte(b, k);
        w[k >> 2] |= (take_min ? min(x, y) : max(x, y)) << (8 * (k & 3));
    }
    return make_uint2(w[0], w[1]);
}

// The bytes child i of a cell of edge S inherits from the cell's bytes v: prune's q(i, k), the edit's rule for a new child
__device__ __forceinline__ uint2 combine_inherit(uint2 v, uint32_t i, float S)
{
    float f[8];
#pragma unroll
    for (int k = 0; k < 8; k++) f[k] = to_float(combine_byte(v, k), S);
    uint32_t w[2] = { 0u, 0u };
#pragma unroll
    for (int k = 0; k < 8; k++) {
        const float tx = (float)((i & 1u) + (uint32_t)(k & 1)) * 0.5f;
        const float ty = (float)(((i >> 1) & 1u) + (uint32_t)((k >> 1) & 1)) * 0.5f;
        const float tz = (float)((i >> 2) + (uint32_t)((k >> 2) & 1)) * 0.5f;
        w[k >> 2] |= from_float(trilerp(f, tx, ty, tz), S * 0.5f) << (8 * (k & 3));
    }
    return make_uint2(w[0], w[1]);
}

// Level 0: the root is a node of both operands, with their own bytes; the result's root has no parent
__global__ __launch_bounds__(64) void k_combine_root(const NodeRec *__restrict__ A, const NodeRec *__restrict__ B, CombineItem *__restrict__ items,
                                                     int2 *__restrict__ links)
{
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        const NodeRec ra = A[0], rb = B[0];
        items[0] = CombineItem{ 0u, 0u, make_uint2(ra.z, ra.w), make_uint2(rb.z, rb.w) };
        links[0] = make_int2(-1, -1);
    }
}

// Pass 1 of a level (its n items; the result's nodes first .. first + n - 1, cells of edge S): the result's bytes; whether the cell
// splits (an operand has children here, and the level lies above the cut), published as a bitmap -- one ballot per wave, its two
// words written whole by lane 0, so split[] needs no clearing: 2 * ceil(n / 64) words; and the cells that are nodes of both operands,
// counted.  op: 0 union, 1 intersect, 2 subtract (include/sdfhip.h).  Lanes stay converged through the ballots: the loop's bound is
// wave-uniform.
__global__ __launch_bounds__(256) void k_combine_level(const NodeRec *__restrict__ A, uint32_t nA, const NodeRec *__restrict__ B, uint32_t nB,
                                                       const CombineItem *__restrict__ items, uint32_t n, uint32_t first, uint32_t cap_out, int op,
                                                       int may_split, float S, uint2 *__restrict__ V, uint32_t *__restrict__ split,
                                                       uint32_t *__restrict__ shared_count)
{
    const uint32_t lane = threadIdx.x & 63u;
    uint32_t shared_waves = 0;
    for (uint32_t base0 = blockIdx.x * blockDim.x; base0 < n; base0 += gridDim.x * blockDim.x) {
        const uint32_t j = base0 + threadIdx.x;
        bool splits = false, both = false;
        if (j < n) {
            const CombineItem it = items[j];
            const uint2 vb = op == 2 ? combine_negate(it.vb, S) : it.vb;
            if (first + j < cap_out) V[first + j] = combine_bytes(it.va, vb, op == 0);
            both = it.ia < nA && it.ib < nB;
            splits = may_split && (combine_children(A, nA, it.ia) != COMBINE_NONE || combine_children(B, nB, it.ib) != COMBINE_NONE);
        }
        const unsigned long long m = __ballot(splits), mb = __ballot(both);
        if (lane == 0 && j < n) {                               // (a wave that starts past the end has no words in split[])
            split[2u * (j >> 6)] = (uint32_t)m;
            split[2u * (j >> 6) + 1u] = (uint32_t)(m >> 32);
            shared_waves += (uint32_t)__popcll(mb);
        }
    }
    if (shared_waves) atomicAdd(shared_count, shared_waves);
}

// The split bitmap, words 0 .. m - 1, to k_rank_scan_words (scan_device.h)
struct CombineSplitWords {
    const uint32_t *split;
    __device__ __forceinline__ uint32_t operator()(uint32_t i) const { return split[i]; }
};

// Pass 2 of a level: eight lanes per item, lane i the item's child i.  A splitting item of rank r (the splits before it in the
// level's order, = the order of the result's indices) gets the block end + 8 r, end = first + n the level's end: its children link,
// the eight children's {parent, -1}, and the next level's items 8 r .. 8 r + 7 -- an operand's child is its own record where the
// operand has children here, else the cell's bytes carried one level down (combine_inherit).  cap_out / cap_next: the room in S[]
// and next[].
__global__ __launch_bounds__(256) void k_combine_emit(const NodeRec *__restrict__ A, uint32_t nA, const NodeRec *__restrict__ B, uint32_t nB,
                                                      const CombineItem *__restrict__ items, uint32_t n, uint32_t first, uint32_t cap_out, float S,
                                                      const uint32_t *__restrict__ split, const uint32_t *__restrict__ pre,
                                                      const uint32_t *__restrict__ chunk, int2 *__restrict__ links,
                                                      CombineItem *__restrict__ next, uint32_t cap_next)
{
    const uint64_t total = 8ull * n;
    for (uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; j < total; j += (uint64_t)gridDim.x * blockDim.x) {
        const uint32_t t = (uint32_t)(j >> 3), i = (uint32_t)j & 7u;
        const uint32_t word = split[t >> 5];
        if (!((word >> (t & 31u)) & 1u)) continue;
        const uint32_t r = rank_in_bitmap(chunk, pre, t >> 5, word, t & 31u);
        const uint32_t self = first + t;
        const uint64_t child = (uint64_t)first + n + 8ull * r + i;
        if (child >= cap_out || 8ull * r + i >= cap_next) continue;            // (a guard: the host sized both from the scan's total)
        if (i == 0) links[self].y = (int32_t)(child);
        links[child] = make_int2((int32_t)self, -1);
        const CombineItem it = items[t];
        CombineItem c;
        const uint32_t ka = combine_children(A, nA, it.ia), kb = combine_children(B, nB, it.ib);
        if (ka != COMBINE_NONE) { const NodeRec rec = A[ka + i]; c.ia = ka + i; c.va = make_uint2(rec.z, rec.w); }
        else { c.ia = COMBINE_NONE; c.va = combine_inherit(it.va, i, S); }
        if (kb != COMBINE_NONE) { const NodeRec rec = B[kb + i]; c.ib = kb + i; c.vb = make_uint2(rec.z, rec.w); }
        else { c.ib = COMBINE_NONE; c.vb = combine_inherit(it.vb, i, S); }
        next[8u * r + i] = c;
    }
}

}  // namespace sdfhip
