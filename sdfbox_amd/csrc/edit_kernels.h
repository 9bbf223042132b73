// The space-carving edit's kernels (gfx950): a frontier walk over the original nodes near a brush, bytes edited in place, and new
// blocks of eight for the leaves the brush refines, level by level.  Non-template kernels: included by edit.hip ONLY.
//
// The arithmetic is the contract of include/sdfhip.h (sdfhip_scene_edit) and DESIGN.md section 8 (N5): fp32, each operation rounded
// on its own, in the order written (-ffp-contract=off); tests/edit_restatement.py restates it with numpy, node for node.
#pragma once
#include "raymarch_device.h"
#include "sdf_bytes.h"
#include "sdf_interp.h"      // edit_lerp, trilerp
#include "scan_device.h"     // k_rank_scan_*, rank_in_bitmap, lane_rank

namespace sdfhip {

struct EditBrush {
    int32_t carve;              // 1: SDFHIP_EDIT_CARVE (g = -s, bytes max(p, q(g))), 0: SDFHIP_EDIT_ADD (g = s, min)
    int32_t box;                // 1: SDFHIP_BRUSH_BOX, 0: SDFHIP_BRUSH_SPHERE
    float cx, cy, cz, a, b, c;  // centre; sphere: a = r; box: half extents a b c
    float cull;                 // a node whose centre has s >= cull * S, and its whole subtree, keeps its bytes and splits nothing
    int32_t max_depth;
};

// a node of the frontier of original nodes: index and integer cell coordinates of its level (lower corner = cell * S, exact)
struct EditEntry { uint32_t idx, ix, iy, iz; };
// a node the edit splits: the same, and its 8 pre-edit corner values (the interpolation its new children start from)
struct EditSplit { uint32_t idx, ix, iy, iz; float f[8]; };
// per level: original nodes pushed to the next level, splits, the lowest (as ~index) and highest split index, nodes visited,
// original nodes whose bytes changed
struct EditCounters { uint32_t n_next, n_split, lo_inv, hi, visited, changed, pad_[2]; };

__device__ __forceinline__ float brush_distance(const EditBrush &B, float px, float py, float pz)
{
    const float dx = px - B.cx, dy = py - B.cy, dz = pz - B.cz;
    if (!B.box) return sqrtf((dx * dx + dy * dy) + dz * dz) - B.a;
    const float qx = fabsf(dx) - B.a, qy = fabsf(dy) - B.b, qz = fabsf(dz) - B.c;
    const float ox = fmaxf(qx, 0.0f), oy = fmaxf(qy, 0.0f), oz = fmaxf(qz, 0.0f);
    return sqrtf((ox * ox + oy * oy) + oz * oz) + fminf(fmaxf(qx, fmaxf(qy, qz)), 0.0f);
}

// The edit of one node: pre-edit corner values pre[8] and bytes p (8 x 8 bits) in, edited bytes out; whether the brush refines it
// (a leaf above max_depth, its centre within the builder's band of the brush, Model.cs:44, and the brush winning there)
__device__ __forceinline__ uint2 edit_bytes(const EditBrush &B, uint2 p, float lx, float ly, float lz, float S)
{
    uint32_t out[2] = { 0u, 0u };
#pragma unroll
    for (int k = 0; k < 8; k++) {
        const float s = brush_distance(B, lx + (float)(k & 1) * S, ly + (float)((k >> 1) & 1) * S, lz + (float)((k >> 2) & 1) * S);
        const uint32_t qg = from_float(B.carve ? -s : s, S);
        const uint32_t pb = ((k < 4 ? p.x : p.y) >> (8 * (k & 3))) & 0xFFu;
        const uint32_t nb = B.carve ? max(pb, qg) : min(pb, qg);
        out[k >> 2] |= nb << (8 * (k & 3));
    }
    return make_uint2(out[0], out[1]);
}

__device__ __forceinline__ bool edit_splits(const EditBrush &B, const float pre[8], float sc, float S, int depth)
{
    if (depth >= B.max_depth || !(fabsf(sc) < 2.0f * S)) return false;
    const float vc = trilerp(pre, 0.5f, 0.5f, 0.5f);
    return B.carve ? -sc > vc : sc < vc;
}

// One wave's splits to the level's list: slots by ballot + lane_rank (scan_device.h) and one atomic; the split's bit in the index bitmap (its block's
// rank among the level's splits is the bitmap's prefix count, edit.hip); the level's lowest and highest split index
__device__ __forceinline__ void push_split(bool split, const EditSplit &e, EditSplit *__restrict__ list, uint32_t *__restrict__ bitmap,
                                           EditCounters *__restrict__ cnt)
{
    const unsigned long long m = __ballot(split);
    if (!m) return;
    const uint32_t lane = threadIdx.x & 63u;
    uint32_t base = 0, hi = split ? e.idx : 0u, lo_inv = split ? ~e.idx : 0u;
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        hi = max(hi, (uint32_t)__shfl_xor((int)hi, o));
        lo_inv = max(lo_inv, (uint32_t)__shfl_xor((int)lo_inv, o));
    }
    if (lane == 0) {
        base = atomicAdd(&cnt->n_split, (uint32_t)__popcll(m));
        atomicMax(&cnt->hi, hi);
        atomicMax(&cnt->lo_inv, lo_inv);
    }
    base = (uint32_t)__builtin_amdgcn_readfirstlane((int)base);
    if (split) {
        list[base + lane_rank(m)] = e;
        atomicOr(&bitmap[e.idx >> 5], 1u << (e.idx & 31u));
    }
}

// The input's fused records -> the {parent, children} and byte arrays the edit works on (and hands to scene_from_arrays)
__global__ __launch_bounds__(256) void k_edit_unfuse(const NodeRec *__restrict__ nodes, int2 *__restrict__ S, uint2 *__restrict__ V, uint32_t n)
{
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        const NodeRec r = nodes[i];
        S[i] = make_int2((int32_t)r.x, (int32_t)r.y);
        V[i] = make_uint2(r.z, r.w);
    }
}

// Original nodes of level `depth` (scale S): skip what the brush cannot reach (and with it the subtree), edit the bytes of the
// rest in place, push internal nodes' children, collect the leaves that split.  Lanes stay converged through the ballots: the
// loop's bound is wave-uniform.
__global__ __launch_bounds__(256) void k_edit_original(EditBrush B, const EditEntry *__restrict__ in, uint32_t n, int depth, float S,
                                                       int2 *__restrict__ Sarr, uint2 *__restrict__ V, EditEntry *__restrict__ next,
                                                       EditSplit *__restrict__ splits, uint32_t *__restrict__ bitmap,
                                                       EditCounters *__restrict__ cnt)
{
    const uint32_t lane = threadIdx.x & 63u;
    uint32_t visited = 0, changed = 0;
    for (uint32_t base0 = blockIdx.x * blockDim.x; base0 < n; base0 += gridDim.x * blockDim.x) {
        const uint32_t i = base0 + threadIdx.x;
        bool inner = false, split = false;
        EditEntry e = { 0u, 0u, 0u, 0u };
        EditSplit sp = {};
        int2 st = make_int2(-1, -1);
        if (i < n) {
            e = in[i];
            const float lx = (float)e.ix * S, ly = (float)e.iy * S, lz = (float)e.iz * S;
            const float sc = brush_distance(B, lx + 0.5f * S, ly + 0.5f * S, lz + 0.5f * S);
            if (sc < B.cull * S) {
                st = Sarr[e.idx];
                const uint2 p = V[e.idx];
                const uint2 nb = edit_bytes(B, p, lx, ly, lz, S);
                if (nb.x != p.x || nb.y != p.y) { V[e.idx] = nb; changed++; }
                inner = st.y >= 0;
                if (!inner) {
#pragma unroll
                    for (int k = 0; k < 8; k++) sp.f[k] = to_float(((k < 4 ? p.x : p.y) >> (8 * (k & 3))) & 0xFFu, S);
                    split = edit_splits(B, sp.f, sc, S, depth);
                    sp.idx = e.idx; sp.ix = e.ix; sp.iy = e.iy; sp.iz = e.iz;
                }
                visited++;
            }
        }
        const unsigned long long m = __ballot(inner);
        if (m) {
            uint32_t base = 0;
            if (lane == 0) base = atomicAdd(&cnt->n_next, 8u * (uint32_t)__popcll(m));
            base = (uint32_t)__builtin_amdgcn_readfirstlane((int)base);
            if (inner) {
                EditEntry *o = next + base + 8u * lane_rank(m);
#pragma unroll
                for (uint32_t c = 0; c < 8; c++)
                    o[c] = EditEntry{ (uint32_t)st.y + c, 2u * e.ix + (c & 1u), 2u * e.iy + ((c >> 1) & 1u), 2u * e.iz + (c >> 2) };
            }
        }
        push_split(split, sp, splits, bitmap, cnt);
    }
    if (visited) atomicAdd(&cnt->visited, visited);
    if (changed) atomicAdd(&cnt->changed, changed);
}

// The new nodes of level `depth`: n = 8 x (blocks emitted under the splits of the level above, parents[]), at indices first ..
// first + n - 1.  Pre-edit values: the parent's, interpolated; pre-edit bytes: their quantisation; then the edit, and the split
// rule again.
__global__ __launch_bounds__(256) void k_edit_new(EditBrush B, const EditSplit *__restrict__ parents, uint32_t first, uint32_t n, int depth,
                                                  float S, int2 *__restrict__ Sarr, uint2 *__restrict__ V, EditSplit *__restrict__ splits,
                                                  uint32_t *__restrict__ bitmap, EditCounters *__restrict__ cnt)
{
    uint32_t visited = 0;
    for (uint32_t base0 = blockIdx.x * blockDim.x; base0 < n; base0 += gridDim.x * blockDim.x) {
        const uint32_t j = base0 + threadIdx.x;
        bool split = false;
        EditSplit sp = {};
        if (j < n) {
            const EditSplit &P = parents[j >> 3];
            const uint32_t c = j & 7u;
            sp.idx = first + j;
            sp.ix = 2u * P.ix + (c & 1u); sp.iy = 2u * P.iy + ((c >> 1) & 1u); sp.iz = 2u * P.iz + (c >> 2);
            float pf[8];
#pragma unroll
            for (int k = 0; k < 8; k++) pf[k] = P.f[k];
            uint32_t pb[2] = { 0u, 0u };
#pragma unroll
            for (int k = 0; k < 8; k++) {
                const float tx = (float)((c & 1u) + (uint32_t)(k & 1)) * 0.5f;
                const float ty = (float)(((c >> 1) & 1u) + (uint32_t)((k >> 1) & 1)) * 0.5f;
                const float tz = (float)((c >> 2) + (uint32_t)((k >> 2) & 1)) * 0.5f;
                sp.f[k] = trilerp(pf, tx, ty, tz);
                pb[k >> 2] |= from_float(sp.f[k], S) << (8 * (k & 3));
            }
            const float lx = (float)sp.ix * S, ly = (float)sp.iy * S, lz = (float)sp.iz * S;
            V[sp.idx] = edit_bytes(B, make_uint2(pb[0], pb[1]), lx, ly, lz, S);
            Sarr[sp.idx] = make_int2((int32_t)P.idx, -1);
            const float sc = brush_distance(B, lx + 0.5f * S, ly + 0.5f * S, lz + 0.5f * S);
            split = edit_splits(B, sp.f, sc, S, depth);
            visited++;
        }
        push_split(split, sp, splits, bitmap, cnt);
    }
    if (visited) atomicAdd(&cnt->visited, visited);
}

// The split bitmap's words w0 .. w0 + m - 1 to k_rank_scan_words (scan_device.h): only the words between the level's lowest and
// highest split are ranked, so word i of the scan is word w0 + i of the bitmap
struct EditWindowWords {
    const uint32_t *bitmap;
    uint32_t w0;
    __device__ __forceinline__ uint32_t operator()(uint32_t i) const { return bitmap[w0 + i]; }
};

// The level's splits, in any order -> their blocks, in the order of their indices: block rank r = the number of splits of this
// level with a lower index; the block starts at first + 8 r, its parent's children field points there, and the parent's entry
// goes to parents_next[r] for the next level's k_edit_new
__global__ __launch_bounds__(256) void k_edit_emit(const EditSplit *__restrict__ splits, uint32_t n, const uint32_t *__restrict__ bitmap,
                                                   uint32_t w0, const uint32_t *__restrict__ pre, const uint32_t *__restrict__ chunk,
                                                   uint32_t first, int2 *__restrict__ Sarr, EditSplit *__restrict__ parents_next)
{
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        const EditSplit e = splits[i];
        const uint32_t w = (e.idx >> 5) - w0;
        const uint32_t r = rank_in_bitmap(chunk, pre, w, bitmap[e.idx >> 5], e.idx & 31u);
        Sarr[e.idx].y = (int32_t)(first + 8u * r);
        parents_next[r] = e;
    }
}

}  // namespace sdfhip
