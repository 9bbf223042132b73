// The components of a resident scene on a cubic lattice (gfx950): the face-connected pieces of the inside phase (solids) and of the
// outside phase (voids), labelled by a concurrent union-find, and one integer record per piece.  Host side, C ABI: components.hip.
//
// Replaces: nothing in the reference's code -- its shader marches one immutable tree and never asks how many pieces it has.
//
// The rule is the contract of include/sdfhip.h (sdfhip_scene_components) and DESIGN.md section 8 (N20): fp32, each operation rounded
// on its own, in the order written; tests/components_restatement.py restates it with numpy on place_restatement.value.
//   p_a        fmaf((float)i_a + 0.5f, pitch, origin_a) for the lattice point (x, y, z), 0 <= x, y, z < 2^d, pitch = side * 2^-d: the
//              clash check's lattice
//   index      (z << 2d) | (y << d) | x
//   inside     value(p) < 0 (a NaN is outside), value = sdfhip_scene_place's at the identity: components_value below
//   connected  two points that differ by 1 in exactly one coordinate and are both inside or both outside
//   label      the lowest index of a point's component; record: label, phase, points, bounds, coordinate sums -- integers,
//              accumulated with integer atomicAdd / atomicMin / atomicMax only: the bytes do not depend on the waves' timing
//
// Shape.  As in k_clash a wave is a 4 x 4 x 4 block of the lattice, lane = lz * 16 + ly * 4 + lx, and a workgroup is four blocks that
// follow each other in block order (x fastest); at d < 2 the one block is partial and the lanes outside the lattice take no part.
// The index is monotone in the lane, so "the lowest lane" of a set of lanes of one block is its lowest index.
//   k_comp_local     one look-up per point; the ballot of "inside" is the block's sign word (sign[block], kept for the passes
//                    below).  The block's own components are found on that one 64-bit scalar: a flood from the lowest remaining
//                    bit, grown by the six shifts under the face masks until it stops.  Each point's parent = the lowest index
//                    of its block-local component, a plain store
//   k_comp_merge     a launch of its own, so that every plain store above is visible on every XCD.  For every pair of equal phase
//                    across a block face: comp_union.  Every read of parent[] here is an agent-scope relaxed atomic load, every
//                    write an agent-scope atomicMin.
//                    Invariants: parent[i] <= i, always (the local pass stores a lowest index, a hook or a compression stores a
//                    smaller value with atomicMin, nothing else writes); a value parent[i] ever held is the index of a point that
//                    ends in i's component (unions only ever merge).  So a read that is stale -- an older value from the XCD's
//                    own L2 -- is still a valid ancestor, and nothing below depends on a read being fresh, only on atomicMin
//                    being one indivisible operation on the word.
//                    Termination: comp_find walks strictly decreasing indices until parent[x] == x.  comp_union's loop hooks the
//                    larger root under the smaller by atomicMin on the larger root's own word; the old value tells whether it
//                    still was a root (old == hi: done).  If not, someone lowered the word first: whichever of old and lo the
//                    word now holds, the other lost its link, so the loop carries on with the pair (old, lo) -- both below hi.
//                    The larger index of the pair strictly decreases with every retry and is bounded by 0: no loop waits for
//                    another wave, and a wave that runs alone finishes.
//                    When all unions have returned, each adjacent pair of equal phase has one root (a union returns only on
//                    seeing equal roots or on hooking a root, and a link it drops it re-establishes before it returns), and the
//                    root of a component is its lowest index (that point can be hooked under nothing).
//   k_comp_flatten   (another launch) every point replaces its parent by its root; plain loads are enough -- the roots' words
//                    do not change, and every other value a word may show is an ancestor.  The ballot of "is a root" is the
//                    root bitmap, two words per wave of 64 consecutive indices
//   k_rank_scan_*    (scan_device.h) the rank of a root among the roots = its record's slot: ascending label order for free
//   k_comp_init      a thread per point: a root writes its record empty (label, phase) and the solids are counted
//   k_comp_records   a wave per run of blocks: for each distinct root among a block's lanes (loop on the first remaining lane's root,
//                    one ballot per iteration) the count, bounds and sums follow from the ballot by scalar arithmetic (block_axis);
//                    the share of the component the wave is in stays in its scalars from block to block, and lane 0 issues the ten
//                    integer atomics when the wave leaves it.  A wave wholly inside one component issues one set for its whole run
// No kernel uses scratch (profiles/components_kernel_resources.txt).
#pragma once
#include "components_host.h" // Component, CompStat, CompLattice, components_value (shared with select.hip); query_kernels.h: the cursors
#include "scan_device.h"     // k_rank_scan_*, rank_in_bitmap, block_axis

namespace sdfhip {

constexpr int COMP_THREADS = 256;

// The root bitmap, words 0 .. m - 1, to k_rank_scan_words (scan_device.h)
struct CompRootWords {
    const uint32_t *roots;
    __device__ __forceinline__ uint32_t operator()(uint32_t i) const { return roots[i]; }
};

// a wave's block and a lane's point in it
struct CompPoint {
    uint32_t bx, by, bz;    // the block's first point
    uint32_t x, y, z, index;
    bool in;                // inside the lattice (d < 2: the block is partial)
};
__device__ __forceinline__ CompPoint comp_point(uint32_t block, uint32_t lane, uint32_t d)
{
    const uint32_t bd = d > 2u ? d - 2u : 0u, bmask = (1u << bd) - 1u, side = 1u << d;
    CompPoint P;
    P.bx = (block & bmask) * 4u; P.by = ((block >> bd) & bmask) * 4u; P.bz = (block >> (2u * bd)) * 4u;
    P.x = P.bx + (lane & 3u); P.y = P.by + ((lane >> 2) & 3u); P.z = P.bz + (lane >> 4);
    P.in = P.x < side && P.y < side && P.z < side;
    P.index = (P.z << (2u * d)) | (P.y << d) | P.x;
    return P;
}

// the lanes of a block that touch the lanes of r across a face inside the block
__device__ __forceinline__ unsigned long long comp_grow(unsigned long long r)
{
    constexpr unsigned long long X0 = 0x1111111111111111ull, X3 = X0 << 3, Y0 = 0x000F000F000F000Full, Y3 = Y0 << 12;
    return ((r & ~X3) << 1) | ((r & ~X0) >> 1) | ((r & ~Y3) << 4) | ((r & ~Y0) >> 4) | (r << 16) | (r >> 16);
}

template <class CursorT>
__global__ __launch_bounds__(COMP_THREADS) void k_comp_local(QueryScene Q, CompLattice L, uint32_t *__restrict__ parent,
                                                             unsigned long long *__restrict__ sign, CompStat *__restrict__ stats)
{
    const uint32_t block = blockIdx.x * (COMP_THREADS / 64) + (threadIdx.x >> 6);       // wave-uniform
    if (block >= L.n_blocks) return;
    const uint32_t lane = threadIdx.x & 63u;
    const CompPoint P = comp_point(block, lane, L.depth);
    const float px = __builtin_fmaf((float)P.x + 0.5f, L.pitch, L.ox), py = __builtin_fmaf((float)P.y + 0.5f, L.pitch, L.oy),
                pz = __builtin_fmaf((float)P.z + 0.5f, L.pitch, L.oz);
    bool inside = false;
    if (P.in) inside = components_value<CursorT>(Q, px, py, pz) < 0.0f;
    const unsigned long long valid = __ballot(P.in), solid = __ballot(inside);
    if (lane == 0u) {
        sign[block] = solid;
        if (solid) atomicAdd(&stats[block & (COMP_STAT_SLOTS - 1u)].inside, (unsigned long long)__popcll(solid));
    }
    // the block's own components, phase by phase, on the wave's scalars: at most 64 floods, each at most 64 growths
    uint32_t low = lane;
    for (int phase = 0; phase < 2; phase++) {
        const unsigned long long of = phase ? valid & ~solid : solid;
        for (unsigned long long left = of; left;) {
            unsigned long long r = left & (~left + 1ull);
            const uint32_t first = (uint32_t)__ffsll((long long)r) - 1u;
            for (;;) {
                const unsigned long long grown = (r | comp_grow(r)) & of;
                if (grown == r) break;
                r = grown;
            }
            if ((r >> lane) & 1ull) low = first;
            left &= ~r;
        }
    }
    if (P.in) {
        const CompPoint R = comp_point(block, low, L.depth);
        parent[P.index] = R.index;
    }
}

__device__ __forceinline__ uint32_t comp_load(const uint32_t *parent, uint32_t i)
{
    return __hip_atomic_load(parent + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// The root above `start`: a walk along strictly decreasing indices.  A walk of more than one step leaves its result in parent[start]
// (atomicMin: the word only ever decreases, and to an ancestor)
__device__ __forceinline__ uint32_t comp_find(uint32_t *parent, uint32_t start)
{
    uint32_t x = comp_load(parent, start);
    if (x == start) return x;
    uint32_t p = comp_load(parent, x);
    if (p == x) return x;
    while (p != x) { x = p; p = comp_load(parent, x); }
    atomicMin(parent + start, x);
    return x;
}

// a and b are one component from now on (the header has the termination argument: max(a, b) decreases with every retry)
__device__ __forceinline__ void comp_union(uint32_t *parent, uint32_t a, uint32_t b)
{
    for (;;) {
        a = comp_find(parent, a);
        b = comp_find(parent, b);
        if (a == b) return;
        const uint32_t hi = max(a, b), lo = min(a, b);
        const uint32_t old = atomicMin(parent + hi, lo);
        if (old == hi) return;              // hi was a root and now hangs under lo
        a = old; b = lo;                    // hi had been hooked already: its old parent and lo are still to be joined
    }
}

__global__ __launch_bounds__(COMP_THREADS) void k_comp_merge(CompLattice L, uint32_t *parent, const unsigned long long *__restrict__ sign)
{
    const uint32_t block = blockIdx.x * (COMP_THREADS / 64) + (threadIdx.x >> 6);       // wave-uniform
    if (block >= L.n_blocks) return;
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t d = L.depth, bd = d - 2u, per_axis = 1u << bd;        // (launched at d > 2 only: a smaller lattice is one block)
    const CompPoint P = comp_point(block, lane, d);
    const unsigned long long mine = sign[block];
    const uint32_t solid = (uint32_t)(mine >> lane) & 1u;
    const uint32_t local[3] = {lane & 3u, (lane >> 2) & 3u, lane >> 4}, at[3] = {P.bx >> 2, P.by >> 2, P.bz >> 2};
#pragma unroll
    for (int a = 0; a < 3; a++) {
        if (at[a] + 1u >= per_axis) continue;                           // wave-uniform: the lattice ends here
        const unsigned long long theirs = sign[block + (1u << (a * bd))];
        const uint32_t step = 1u << (2 * a);                            // a lane's neighbour along the axis
        const bool on_face = local[a] == 3u;
        const bool joins = on_face && (((uint32_t)(theirs >> (on_face ? lane - 3u * step : 0u)) & 1u) == solid);
        uint32_t u = 0u, v = 0u;
        if (joins) {
            u = comp_load(parent, P.index);
            v = comp_load(parent, P.index + (1u << (a * d)));
        }
        // the lane before this one in the face (along x, or along y on the face across x) joins the same two local components:
        // its union is this one's
        const uint32_t before_step = a == 0 ? 4u : 1u;
        const bool has_before = (a == 0 ? local[1] : local[0]) > 0u;
        const uint32_t before = has_before ? lane - before_step : lane;
        const uint32_t bu = (uint32_t)__shfl((int)u, (int)before), bv = (uint32_t)__shfl((int)v, (int)before);
        const bool bj = __shfl((int)joins, (int)before) != 0;
        if (joins && !(has_before && bj && bu == u && bv == v)) comp_union(parent, u, v);
    }
}

// n = 8^d points, a thread each
__global__ __launch_bounds__(COMP_THREADS) void k_comp_flatten(uint32_t *parent, uint32_t n, uint32_t *__restrict__ roots)
{
    const uint32_t i = blockIdx.x * COMP_THREADS + threadIdx.x;
    bool root = false;
    if (i < n) {
        uint32_t x = i, p = parent[x];
        while (p != x) { x = p; p = parent[x]; }
        if (x != i) parent[i] = x;
        root = x == i;
    }
    const unsigned long long m = __ballot(root);
    if ((threadIdx.x & 63u) == 0u && i < n) {           // (n < 64: the second word is allocated and never read)
        roots[i >> 5] = (uint32_t)m;
        roots[(i >> 5) + 1u] = (uint32_t)(m >> 32);
    }
}

// a thread per point: a root's record, empty
__global__ __launch_bounds__(COMP_THREADS) void k_comp_init(CompLattice L, uint32_t n, const uint32_t *__restrict__ roots,
                                                            const uint32_t *__restrict__ pre, const uint32_t *__restrict__ chunk,
                                                            const unsigned long long *__restrict__ sign, Component *__restrict__ out,
                                                            CompStat *__restrict__ stats)
{
    const uint32_t i = blockIdx.x * COMP_THREADS + threadIdx.x;
    bool solid_root = false;
    if (i < n) {
        const uint32_t word = roots[i >> 5];
        if ((word >> (i & 31u)) & 1u) {
            const uint32_t d = L.depth, bd = d > 2u ? d - 2u : 0u, mask = (1u << d) - 1u;
            const uint32_t x = i & mask, y = (i >> d) & mask, z = i >> (2u * d);
            const uint32_t block = ((z >> 2) << (2u * bd)) | ((y >> 2) << bd) | (x >> 2), lane = (z & 3u) * 16u + (y & 3u) * 4u + (x & 3u);
            solid_root = (sign[block] >> lane) & 1ull;
            Component C;
            C.label = i; C.flags = solid_root ? COMP_SOLID : 0u; C.points = 0u; C.reserved = 0u;
            for (int k = 0; k < 3; k++) { C.lo[k] = 0xFFFFFFFFu; C.hi[k] = 0u; C.sum[k] = 0ull; }
            out[rank_in_bitmap(chunk, pre, i >> 5, word, i & 31u)] = C;
        }
    }
    const unsigned long long m = __ballot(solid_root);
    if ((threadIdx.x & 63u) == 0u && m) atomicAdd(&stats[(i >> 6) & (COMP_STAT_SLOTS - 1u)].solids, (uint32_t)__popcll(m));
}

// a component's share of some blocks, in the wave's scalars: what the ten atomics of a record take
struct CompPart {
    uint32_t label, points;             // points == 0: empty
    uint32_t lo[3], hi[3];
    unsigned long long sum[3];
};

__device__ __forceinline__ void comp_flush(const CompPart &S, uint32_t lane, const uint32_t *__restrict__ roots, const uint32_t *__restrict__ pre,
                                           const uint32_t *__restrict__ chunk, Component *__restrict__ out)
{
    if (lane != 0u || !S.points) return;
    Component *C = out + rank_in_bitmap(chunk, pre, S.label >> 5, roots[S.label >> 5], S.label & 31u);
    atomicAdd(&C->points, S.points);
    for (int k = 0; k < 3; k++) {
        atomicMin(&C->lo[k], S.lo[k]);
        atomicMax(&C->hi[k], S.hi[k]);
        atomicAdd(&C->sum[k], S.sum[k]);
    }
}

// A wave takes `run` blocks that follow each other and holds TWO components' shares across them -- in most waves the outer void and
// the body it surrounds, whose records would otherwise take ten atomics from every block they are in, all on one 64-byte line each
// (measured at depth 8: 30 of the call's 32 ms with no share held, 4.4 of 5.4 ms with one).  A component that finds both places taken
// puts out one that is not in its block, or else goes out at once; both go out at the end of the run.  Integer add / min / max
// commute: the bytes do not depend on `run`.
__global__ __launch_bounds__(COMP_THREADS) void k_comp_records(CompLattice L, uint32_t run, const uint32_t *__restrict__ labels,
                                                               const uint32_t *__restrict__ roots, const uint32_t *__restrict__ pre,
                                                               const uint32_t *__restrict__ chunk, Component *__restrict__ out)
{
    const uint32_t first = (blockIdx.x * (COMP_THREADS / 64) + (threadIdx.x >> 6)) * run;        // wave-uniform; run * waves < 2^32
    if (first >= L.n_blocks) return;
    const uint32_t end = min(first + run, L.n_blocks), lane = threadIdx.x & 63u;
    CompPart held[2];
    held[0].label = held[1].label = 0u;
    held[0].points = held[1].points = 0u;
    for (uint32_t block = first; block < end; block++) {
        const CompPoint P = comp_point(block, lane, L.depth);
        const uint32_t mine = P.in ? labels[P.index] : 0xFFFFFFFFu;
        const bool here[2] = {held[0].points && __ballot(mine == held[0].label), held[1].points && __ballot(mine == held[1].label)};
        for (unsigned long long left = __ballot(P.in); left;) {
            const uint32_t label = (uint32_t)__builtin_amdgcn_readfirstlane((int)__shfl((int)mine, __ffsll((long long)left) - 1));
            const unsigned long long of = __ballot(mine == label);
            const uint32_t base[3] = {P.bx, P.by, P.bz};
            uint32_t lo[3], hi[3], sum[3];
            block_axis(of, 0x1111111111111111ull, 1, lo[0], hi[0], sum[0]);
            block_axis(of, 0x000F000F000F000Full, 4, lo[1], hi[1], sum[1]);
            block_axis(of, 0x000000000000FFFFull, 16, lo[2], hi[2], sum[2]);
            CompPart S;
            S.label = label; S.points = (uint32_t)__popcll(of);
            for (int k = 0; k < 3; k++) { S.lo[k] = base[k] + lo[k]; S.hi[k] = base[k] + hi[k]; S.sum[k] = (unsigned long long)base[k] * S.points + sum[k]; }
            left &= ~of;
            // the place that holds this component, else an empty one, else one whose component is not in this block
            int at = -1;
#pragma unroll
            for (int h = 1; h >= 0; h--) if (!here[h]) at = h;
#pragma unroll
            for (int h = 1; h >= 0; h--) if (!held[h].points) at = h;
#pragma unroll
            for (int h = 1; h >= 0; h--) if (here[h] && held[h].label == label) at = h;
            if (at < 0) { comp_flush(S, lane, roots, pre, chunk, out); continue; }
#pragma unroll
            for (int h = 0; h < 2; h++) {
                if (h != at) continue;
                if (here[h] && held[h].label == label) {
                    held[h].points += S.points;
                    for (int k = 0; k < 3; k++) { held[h].lo[k] = min(held[h].lo[k], S.lo[k]); held[h].hi[k] = max(held[h].hi[k], S.hi[k]); held[h].sum[k] += S.sum[k]; }
                } else {
                    comp_flush(held[h], lane, roots, pre, chunk, out);          // (nothing when the place is empty)
                    held[h] = S;
                }
            }
        }
    }
    comp_flush(held[0], lane, roots, pre, chunk, out);
    comp_flush(held[1], lane, roots, pre, chunk, out);
}

}  // namespace sdfhip
