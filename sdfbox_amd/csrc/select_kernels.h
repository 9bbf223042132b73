// Selection (gfx950): a scene's components kept, dropped or filled, and the result built as a new tree.  The decision on the records
// of the labelling (components_host.h), the two bitmaps it leaves on the lattice, and the level pass that reads them.  Host side, C
// ABI: select.hip.
//
// Replaces: nothing in the reference's code -- a tree there is immutable, and nothing in it knows that a model has pieces.
//
// The rule is the contract of include/sdfhip.h (sdfhip_scene_select) and DESIGN.md section 8 (N21): fp32, each operation rounded on
// its own, in the order written; tests/select_restatement.py restates it with numpy.
//   F[i], T[i]   lattice point i's component flips; its target phase, inside XOR F
//   v            components_value at the tree point p: the placement's value at the identity
//   N(p)         per axis g = (p_a - origin_a) / pitch - 0.5f, f = floorf(g), {f} if g == f else {f, f + 1}, each clamped into
//                0 .. 2^d - 1 in float: the lattice points with non-zero trilinear weight at p
//   v'           -fmaxf(fabsf(v), h) if some point of N(p) has F and all have T; fmaxf(fabsf(v), h) if some has F and none has T; else v;
//                h = 2^-8
//
//   k_select_largest  a thread per record: the solids' 64-bit atomicMax on (points << 32) | ~label -- most points, then lowest label
//   k_select_decide   a thread per record: the rule bits -> one byte per record, bit 0 = F, bit 1 = T; the flipped components and
//                     their points are counted here, from the records, with integer atomics (the order cannot change a sum).  The
//                     same threads, one per listed label: a label that is no root is counted and the lowest is kept for the message
//   k_select_mark     a thread per lattice point: label -> record slot (rank_in_bitmap) -> the byte; a wave's 64 consecutive indices
//                     leave as one ballot word of F and one of T.  No atomics, nothing to clear: every word is written whole (at
//                     depth 0 and 1 the lattice is part of word 0, and the lanes behind it vote 0)
//   k_select_level    level_body on SelectValue: one look-up, then F's bits -- the two x-neighbours of a row share a word unless the
//                     row crosses one, so a point away from every change reads at most 4 words and returns v -- and T's only then
// No kernel uses scratch or LDS (profiles/select_kernel_resources.txt).
#pragma once
#include "components_host.h" // Component, COMP_SOLID, components_value
#include "level_kernels.h"   // LevelBlock, level_body
#include "scan_device.h"     // rank_in_bitmap

namespace sdfhip {

constexpr int SELECT_THREADS = 256;
constexpr uint32_t SELECT_KEEP_LARGEST = 1u, SELECT_DROP_SMALL = 2u, SELECT_FILL_ENCLOSED = 4u, SELECT_FLIP_LISTED = 8u, SELECT_KEEP_LISTED = 16u;
constexpr uint32_t SELECT_F = 1u, SELECT_T = 2u;        // a record's byte
constexpr float SELECT_H = 0.00390625f;                 // h = 2^-8

// what the decision counts, read by the host in one copy
struct SelectHead {
    unsigned long long largest;         // max over the solids of (points << 32) | ~label
    unsigned long long points_flipped;
    uint32_t solids, flipped_solids, flipped_voids;
    uint32_t not_roots, first_not_root; // listed labels that name no component: how many, the lowest
    uint32_t listed_voids, first_void;  // voids listed under KEEP_LISTED
    uint32_t pad;
};

// the lattice and its bitmaps as the level pass reads them
struct SelectLattice {
    float ox, oy, oz, pitch;
    uint32_t depth;
    const unsigned long long *F, *T;
};

__global__ __launch_bounds__(SELECT_THREADS) void k_select_largest(const Component *__restrict__ rec, uint32_t total, SelectHead *__restrict__ head)
{
    const uint32_t r = blockIdx.x * SELECT_THREADS + threadIdx.x;
    if (r >= total) return;
    if (rec[r].flags & COMP_SOLID) atomicMax(&head->largest, ((unsigned long long)rec[r].points << 32) | (unsigned long long)(~rec[r].label));
}

// is `label` in the sorted list?
__device__ __forceinline__ bool select_listed(const uint32_t *__restrict__ list, uint32_t n_list, uint32_t label)
{
    uint32_t lo = 0u, hi = n_list;
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2u;
        if (list[mid] < label) lo = mid + 1u; else hi = mid;
    }
    return lo < n_list && list[lo] == label;
}

// n = 8^d points; list: sorted, no label twice
__global__ __launch_bounds__(SELECT_THREADS) void k_select_decide(const Component *__restrict__ rec, uint32_t total, uint32_t flags, uint32_t min_points,
                                                                  uint32_t depth, const uint32_t *__restrict__ list, uint32_t n_list,
                                                                  const uint32_t *__restrict__ roots, uint32_t n, uint8_t *__restrict__ decided,
                                                                  SelectHead *__restrict__ head)
{
    const uint32_t r = blockIdx.x * SELECT_THREADS + threadIdx.x;
    if (r < n_list) {
        const uint32_t label = list[r];
        if (label >= n || !((roots[label >> 5] >> (label & 31u)) & 1u)) {
            atomicAdd(&head->not_roots, 1u);
            atomicMin(&head->first_not_root, label);
        }
    }
    if (r >= total) return;
    const Component C = rec[r];
    const bool solid = C.flags & COMP_SOLID;
    const uint32_t last = (1u << depth) - 1u;
    const bool listed = n_list && select_listed(list, n_list, C.label);
    bool flip = false;
    if ((flags & SELECT_KEEP_LARGEST) && solid && C.label != ~(uint32_t)head->largest) flip = true;
    if ((flags & SELECT_DROP_SMALL) && solid && C.points < min_points) flip = true;
    if ((flags & SELECT_FILL_ENCLOSED) && !solid && C.lo[0] != 0u && C.lo[1] != 0u && C.lo[2] != 0u && C.hi[0] != last && C.hi[1] != last && C.hi[2] != last)
        flip = true;
    if ((flags & SELECT_FLIP_LISTED) && listed) flip = true;
    if (flags & SELECT_KEEP_LISTED) {
        if (solid && !listed) flip = true;
        if (!solid && listed) {
            atomicAdd(&head->listed_voids, 1u);
            atomicMin(&head->first_void, C.label);
        }
    }
    decided[r] = (uint8_t)((flip ? SELECT_F : 0u) | ((solid != flip) ? SELECT_T : 0u));
    if (solid) atomicAdd(&head->solids, 1u);
    if (flip) {
        atomicAdd(solid ? &head->flipped_solids : &head->flipped_voids, 1u);
        atomicAdd(&head->points_flipped, (unsigned long long)C.points);
    }
}

// n = 8^d points, a thread each; F, T: max(n / 64, 1) words
__global__ __launch_bounds__(SELECT_THREADS) void k_select_mark(const uint32_t *__restrict__ labels, uint32_t n, const uint32_t *__restrict__ roots,
                                                                const uint32_t *__restrict__ pre, const uint32_t *__restrict__ chunk,
                                                                const uint8_t *__restrict__ decided, unsigned long long *__restrict__ F,
                                                                unsigned long long *__restrict__ T)
{
    const uint32_t i = blockIdx.x * SELECT_THREADS + threadIdx.x;
    uint32_t byte = 0u;
    if (i < n) {
        const uint32_t label = labels[i], word = roots[label >> 5];
        byte = decided[rank_in_bitmap(chunk, pre, label >> 5, word, label & 31u)];
    }
    const unsigned long long f = __ballot(byte & SELECT_F), t = __ballot(byte & SELECT_T);
    if ((threadIdx.x & 63u) == 0u && i < n) { F[i >> 6] = f; T[i >> 6] = t; }
}

// one axis of N(p): the lower candidate and the upper (the same index where g == f, or where the clamp brings them together)
__device__ __forceinline__ void select_axis(float p, float o, float pitch, float last, uint32_t &i0, uint32_t &i1)
{
    const float g = (p - o) / pitch - 0.5f, f = floorf(g);
    const float c0 = __builtin_fminf(__builtin_fmaxf(f, 0.0f), last);
    const float c1 = g == f ? c0 : __builtin_fminf(__builtin_fmaxf(f + 1.0f, 0.0f), last);
    i0 = (uint32_t)c0; i1 = (uint32_t)c1;
}

// the bits of the lattice points row + x0 and row + x1 of bitmap W: bit 0 and bit 1 (one load where they share a word)
__device__ __forceinline__ uint32_t select_pair(const unsigned long long *__restrict__ W, uint32_t row, uint32_t x0, uint32_t x1)
{
    const uint32_t a = row + x0, b = row + x1;
    const unsigned long long wa = W[a >> 6], wb = (b >> 6) == (a >> 6) ? wa : W[b >> 6];
    return ((uint32_t)(wa >> (a & 63u)) & 1u) | (((uint32_t)(wb >> (b & 63u)) & 1u) << 1);
}

template <class CursorT> struct SelectValue {
    static constexpr int SOURCES = 0;
    QueryScene Q;
    SelectLattice L;
    __device__ __forceinline__ float operator()(float px, float py, float pz, uint2 *, uint32_t *) const
    {
        const float v = components_value<CursorT>(Q, px, py, pz);
        const uint32_t d = L.depth;
        const float last = (float)((1u << d) - 1u);
        uint32_t x[2], y[2], z[2];
        select_axis(px, L.ox, L.pitch, last, x[0], x[1]);
        select_axis(py, L.oy, L.pitch, last, y[0], y[1]);
        select_axis(pz, L.oz, L.pitch, last, z[0], z[1]);
        uint32_t row[4];
#pragma unroll
        for (int k = 0; k < 4; k++) row[k] = (z[k >> 1] << (2u * d)) | (y[k & 1] << d);
        uint32_t any = 0u;
#pragma unroll
        for (int k = 0; k < 4; k++) any |= select_pair(L.F, row[k], x[0], x[1]);
        if (!any) return v;
        uint32_t all = 3u, some = 0u;
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const uint32_t t = select_pair(L.T, row[k], x[0], x[1]);
            all &= t; some |= t;
        }
        const float far = __builtin_fmaxf(fabsf(v), SELECT_H);
        return all == 3u ? -far : some == 0u ? far : v;
    }
};

template <class CursorT>
__global__ __launch_bounds__(LEVEL_THREADS) void k_select_level(QueryScene Q, SelectLattice L, const LevelBlock *__restrict__ blocks, uint32_t nblocks,
                                                                uint32_t nchild, float S, int may_split, uint2 *__restrict__ V,
                                                                uint8_t *__restrict__ split)
{
    level_body(SelectValue<CursorT>{Q, L}, blocks, nblocks, nchild, S, may_split, V, split, nullptr);
}

}  // namespace sdfhip
