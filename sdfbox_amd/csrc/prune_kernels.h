// The prune's kernels (gfx950): the internal nodes brought to their levels, the blocks of eight judged level by level from the deepest
// up, a prefix scan over the bitmap of survivors and one compaction.  Non-template kernels: included by prune.hip ONLY.
//
// The arithmetic is the contract of include/sdfhip.h (sdfhip_scene_prune) and DESIGN.md section 8 (N9): fp32, each operation rounded
// on its own, in the order written (-ffp-contract=off); tests/prune_restatement.py restates it with numpy, level by level.  The
// bytes a block is compared with are those k_edit_new gives a new child before the brush (to_float, trilerp, from_float: the same
// three functions).
#pragma once
#include "raymarch_device.h"
#include "sdf_bytes.h"
#include "sdf_interp.h"

namespace sdfhip {

// per level d: the internal nodes of depth d (= the blocks whose parents they are), and how many of those blocks were removed
struct PruneCounters { uint32_t n_blocks, removed; };

__device__ __forceinline__ uint32_t prune_lane_rank(unsigned long long m)
{
    return __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
}

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
            const uint32_t slot = base + prune_lane_rank(m);
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

// The prefix counts of the survivors' bitmap, words 0 .. m - 1: per word, the survivors of the words before it in its chunk of 1024
// words (pre[]), and per chunk its total (chunk[]) -- the edit's scan (k_edit_scan_words) over the complement of removed[]
__global__ __launch_bounds__(256) void k_prune_scan_words(const uint32_t *__restrict__ removed, uint32_t n, uint32_t m,
                                                          uint32_t *__restrict__ pre, uint32_t *__restrict__ chunk)
{
    __shared__ uint32_t part[256];
    const uint32_t t = threadIdx.x, first = blockIdx.x * 1024u + 4u * t;
    uint32_t c[4], sum = 0;
#pragma unroll
    for (int k = 0; k < 4; k++) { c[k] = first + k < m ? (uint32_t)__popc(prune_keep_word(removed, first + k, n)) : 0u; sum += c[k]; }
    part[t] = sum;
    __syncthreads();
    for (uint32_t o = 1; o < 256; o <<= 1) {          // inclusive scan of the threads' sums (Hillis-Steele)
        const uint32_t v = t >= o ? part[t - o] : 0u;
        __syncthreads();
        part[t] += v;
        __syncthreads();
    }
    uint32_t run = part[t] - sum;
#pragma unroll
    for (int k = 0; k < 4; k++) { if (first + k < m) pre[first + k] = run; run += c[k]; }
    if (t == 255) chunk[blockIdx.x] = part[255];
}

// ... the chunks' totals -> exclusive prefix, in one workgroup (at most 65 536 chunks: 2^31 nodes); chunk[nchunk] = the survivors
__global__ __launch_bounds__(1024) void k_prune_scan_chunks(uint32_t *__restrict__ chunk, uint32_t nchunk)
{
    __shared__ uint32_t part[1024];
    const uint32_t t = threadIdx.x, per = (nchunk + 1023u) / 1024u, lo = t * per;
    uint32_t sum = 0;
    for (uint32_t k = 0; k < per; k++) if (lo + k < nchunk) sum += chunk[lo + k];
    part[t] = sum;
    __syncthreads();
    for (uint32_t o = 1; o < 1024; o <<= 1) {
        const uint32_t v = t >= o ? part[t - o] : 0u;
        __syncthreads();
        part[t] += v;
        __syncthreads();
    }
    uint32_t run = part[t] - sum;
    for (uint32_t k = 0; k < per; k++) if (lo + k < nchunk) { const uint32_t v = chunk[lo + k]; chunk[lo + k] = run; run += v; }
    if (t == 1023) chunk[nchunk] = part[1023];
}

// a survivor's new index: the survivors with a lower old index
__device__ __forceinline__ uint32_t prune_rank(const uint32_t *__restrict__ removed, const uint32_t *__restrict__ pre,
                                               const uint32_t *__restrict__ chunk, uint32_t i)
{
    const uint32_t w = i >> 5;
    return chunk[w >> 10] + pre[w] + (uint32_t)__popc(~removed[w] & ((1u << (i & 31u)) - 1u));
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
