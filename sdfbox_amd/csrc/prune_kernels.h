// The prune's kernels (gfx950): the internal nodes brought to their levels, the blocks of eight judged level by level from the deepest
// up, the survivors' ranks by the shared bitmap scan (scan_device.h) and one compaction.  Non-template kernels: included by prune.hip ONLY.
//
// The arithmetic is the contract of include/sdfhip.h (sdfhip_scene_prune) and DESIGN.md section 8 (N9): fp32, each operation rounded
// on its own, in the order written (-ffp-contract=off); tests/prune_restatement.py restates it with numpy, level by level.  The
// bytes a block is compared with are those k_edit_new gives a new child before the brush (to_float, trilerp, from_float: the same
// three functions).
#pragma once
#include "raymarch_device.h"
#include "sdf_bytes.h"
#include "sdf_interp.h"
#include "scan_device.h"     // k_rank_scan_*, rank_in_bitmap, lane_rank

namespace sdfhip {

// per level d: the internal nodes of depth d (= the blocks whose parents they are), and how many of those blocks were removed
struct PruneCounters { uint32_t n_blocks, removed; };

__device__ __forceinline__ bool prune_bit(const uint32_t *bitmap, uint32_t i) { return (bitmap[i >> 5] >> (i & 31u)) & 1u; }

// The internal nodes of one level (in[0 .. n_in - 1], any order) -> those of the next: eight lanes per node, one per child; a
// child that has children of its own takes a slot of next[] (ballot + mbcnt and one atomic per wave).  cap: the room in next[].
__global__ __launch_bounds__(256) void k_prune_expand(const NodeRec *__restrict__ nodes, uint32_t n, const uint32_t *__restrict__ in, uint32_t n_in,
                                                      uint32_t *__restrict__ next, uint32_t cap, PruneCounters *__restrict__ cnt_next)
{
    const uint32_t lane = threadIdx.x & 63u, total = 8u * n_in;
    for (uint32_t base0 = blockIdx.x * blockDim.x; base0 < total; base0 += gridDim.x * blockDim.x) {
        const uint32_t j = base0 + threadIdx.x;
        bool inner = false;
        uint32_t child = 0;
        if (j < total) {
            child = nodes[in[j >> 3]].y + (j & 7u);
            inner = child < n && (int32_t)nodes[child].y >= 0;   // (in range in every tree the upload accepts: a guard, not a case)
        }
        const unsigned long long m = __ballot(inner);
        if (m) {
            uint32_t base = 0;
            if (lane == 0) base = atomicAdd(&cnt_next->n_blocks, (uint32_t)__popcll(m));
            base = (uint32_t)__builtin_amdgcn_readfirstlane((int)base);
            const uint32_t slot = base + lane_rank(m);
            if (inner && slot < cap) next[slot] = child;
        }
    }
}

// The blocks of one level (their parents P of depth d, edge S = 2^-d, in list[]): eight lanes per block, lane i judges child i --
// a leaf, or a node whose own block was removed by a deeper level's launch; and, unless the level lies below the cut, every one of
// its eight bytes within `tol` of q(i, k), the byte P's decoded corners interpolate to at the child's corner k.  The block's
// verdict is the ballot's byte of its eight lanes; a redundant block's eight bits are set in removed[] (blocks start at any index:
// the byte may straddle two words).  Lanes stay converged through the ballots: the loop's bound is wave-uniform.
// removed[] is read (bits of deeper levels, final) and written (bits of this level) in one launch: different bits, plain loads.
__global__ __launch_bounds__(256) void k_prune_decide(const NodeRec *__restrict__ nodes, uint32_t n, const uint32_t *__restrict__ list, uint32_t n_blocks,
                                                      float S, int cut, int tol, uint32_t *removed, PruneCounters *__restrict__ cnt)
{
    const uint32_t lane = threadIdx.x & 63u, total = 8u * n_blocks;
    uint32_t gone_blocks = 0;
    for (uint32_t base0 = blockIdx.x * blockDim.x; base0 < total; base0 += gridDim.x * blockDim.x) {
        const uint32_t j = base0 + threadIdx.x, i = j & 7u;
        bool ok = false;
        uint32_t first = 0;
        const NodeRec pr = j < total ? nodes[list[j >> 3]] : NodeRec{};
        first = pr.y;
        if (j < total && first < n && n - first >= 8u) {                                 // (the second: a guard, as in k_prune_expand)
            const NodeRec cr = nodes[first + i];
            ok = (int32_t)cr.y < 0 || (cr.y < n && prune_bit(removed, cr.y));
            if (ok && !cut) {
                float f[8];
#pragma unroll
                for (int k = 0; k < 8; k++) f[k] = to_float(((k < 4 ? pr.z : pr.w) >> (8 * (k & 3))) & 0xFFu, S);
#pragma unroll
                for (int k = 0; k < 8; k++) {
                    const float tx = (float)((i & 1u) + (uint32_t)(k & 1)) * 0.5f;
                    const float ty = (float)(((i >> 1) & 1u) + (uint32_t)((k >> 1) & 1)) * 0.5f;
                    const float tz = (float)((i >> 2) + (uint32_t)((k >> 2) & 1)) * 0.5f;
                    const int q = (int)from_float(trilerp(f, tx, ty, tz), S * 0.5f);
                    const int b = (int)(((k < 4 ? cr.z : cr.w) >> (8 * (k & 3))) & 0xFFu);
                    ok = ok && abs(b - q) <= tol;
                }
            }
        }
        const unsigned long long m = __ballot(ok);
        const bool gone = ((m >> (lane & 56u)) & 0xFFull) == 0xFFull;       // (lanes past the end voted no: 8 | total)
        if (gone && i == 0) {
            const uint32_t w = first >> 5, s = first & 31u;
            atomicOr(&removed[w], 0xFFu << s);
            if (s > 24u) atomicOr(&removed[w + 1], 0xFFu >> (32u - s));
            gone_blocks++;
        }
    }
    if (gone_blocks) atomicAdd(&cnt->removed, gone_blocks);
}

// the survivors among nodes 32 w .. 32 w + 31 (n nodes in all)
__device__ __forceinline__ uint32_t prune_keep_word(const uint32_t *__restrict__ removed, uint32_t w, uint32_t n)
{
    const uint32_t left = n - 32u * w;
    return ~removed[w] & (left >= 32u ? 0xFFFFFFFFu : (1u << left) - 1u);
}

// The survivors' bitmap, words 0 .. m - 1, to k_rank_scan_words (scan_device.h): the complement of removed[]
struct PruneKeepWords {
    const uint32_t *removed;
    uint32_t n;
    __device__ __forceinline__ uint32_t operator()(uint32_t i) const { return prune_keep_word(removed, i, n); }
};

// a survivor's new index: the survivors with a lower old index
__device__ __forceinline__ uint32_t prune_rank(const uint32_t *__restrict__ removed, const uint32_t *__restrict__ pre,
                                               const uint32_t *__restrict__ chunk, uint32_t i)
{
    return rank_in_bitmap(chunk, pre, i >> 5, ~removed[i >> 5], i & 31u);
}

// The survivors, in their order, to the arrays of the result: {parent, children} remapped -- a node whose block was removed becomes
// a leaf (children -1) -- and the bytes as they are
__global__ __launch_bounds__(256) void k_prune_compact(const NodeRec *__restrict__ nodes, uint32_t n, const uint32_t *__restrict__ removed,
                                                       const uint32_t *__restrict__ pre, const uint32_t *__restrict__ chunk, uint32_t n_out,
                                                       int2 *__restrict__ S, uint2 *__restrict__ V)
{
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        if (prune_bit(removed, i)) continue;
        const NodeRec r = nodes[i];
        const uint32_t at = prune_rank(removed, pre, chunk, i);
        int32_t parent = (int32_t)r.x, children = (int32_t)r.y;
        if (parent >= 0 && (uint32_t)parent < n) parent = (int32_t)prune_rank(removed, pre, chunk, (uint32_t)parent);
        if (children >= 0 && (uint32_t)children < n) children = prune_bit(removed, (uint32_t)children) ? -1 : (int32_t)prune_rank(removed, pre, chunk, (uint32_t)children);
        if (at < n_out) {
            S[at] = make_int2(parent, children);
            V[at] = make_uint2(r.z, r.w);
        }
    }
}

}  // namespace sdfhip
