// Smooth blends and morphs of two resident scenes on the exact distance (gfx950): the value of sdfhip_scene_blend and its level
// pass.  k_blend_level is not a template: included by blend.hip ONLY.  Host side, C ABI: blend.hip.
//
// Replaces: nothing in the reference's code -- a tree there is immutable once built, and its field is only ever read as stored.
//
// The rule is the contract of include/sdfhip.h (sdfhip_scene_blend) and DESIGN.md section 8 (N14): fp32, each operation rounded on its
// own, in the order written (-ffp-contract=off); tests/blend_restatement.py restates it with numpy, by brute force.
//   a, b      dist_A(p), dist_B(p): distance_kernels.h's dist, each operand's own surface, level and sign; +-inf on an empty surface
//   smin      h = k > 0 ? fmaxf(k - fabsf(a - b), 0) / k : 0;  smin = fminf(a, b) - ((h * h) * k) * 0.25f
//             (fmaxf / fminf return the operand that is no NaN: inf - inf gives h = 0)
//   value     UNION smin(a, b, k); INTERSECT -smin(-a, -b, k); SUBTRACT -smin(-a, b, k); MORPH a + (b - a) * t
//   tree      the construct rule and node order of the offset: k_blend_level is level_body (level_kernels.h) on BlendValue
//
// k_blend_level.  A lane searches A's surface and then B's, one after the other through the SAME slice of the workgroup's stack
// ([level][lane], 24 576 bytes per workgroup, as the offset's: the first search has left nothing on it that the second needs), keeps
// of each search d2 and the records it loaded, then looks up the two signs and computes the value.  Both look-ups walk the links
// (CursorG) whatever grids the handles have: both forms give the same bytes, the look-up is one find beside a search of about a
// hundred records, and a kernel per pair of forms would be nine copies of the heaviest kernel in the library.
#pragma once
#include "distance_kernels.h"   // nearest_search, inside_at, DistScene
#include "level_kernels.h"      // LevelBlock, LEVEL_THREADS, level_body

namespace sdfhip {

enum { BLEND_UNION = 0, BLEND_INTERSECT = 1, BLEND_SUBTRACT = 2, BLEND_MORPH = 3 };      // SDFHIP_BLEND_* of include/sdfhip.h

// smin(a, b, k) of the rule
__device__ __forceinline__ float smooth_min(float a, float b, float k)
{
    const float h = k > 0.0f ? fmaxf(k - fabsf(a - b), 0.0f) / k : 0.0f;
    return fminf(a, b) - ((h * h) * k) * 0.25f;
}

// value by op from the two distances
__device__ __forceinline__ float blend_value(int op, float a, float b, float amount)
{
    switch (op) {
    case BLEND_UNION: return smooth_min(a, b, amount);
    case BLEND_INTERSECT: return -smooth_min(-a, -b, amount);
    case BLEND_SUBTRACT: return -smooth_min(-a, b, amount);
    default: return a + (b - a) * amount;
    }
}

struct BlendValue {
    static constexpr int SOURCES = 2;
    QueryScene QA;
    DistScene DA;
    QueryScene QB;
    DistScene DB;
    int op;
    float amount;
    unsigned long long *visited;          // [2]: A's searches, B's searches
    __device__ __forceinline__ float operator()(float px, float py, float pz, uint2 *stk, uint32_t *seen) const
    {
        float root[2];
        {
            Nearest best;
            nearest_search<LEVEL_THREADS>(DA, px, py, pz, stk, best);
            root[0] = sqrtf(best.d2);
            seen[0] = best.visited;
        }
        {
            Nearest best;
            nearest_search<LEVEL_THREADS>(DB, px, py, pz, stk, best);
            root[1] = sqrtf(best.d2);
            seen[1] = best.visited;
        }
        const float a = (inside_at<CursorG>(QA, px, py, pz) ? -1.0f : 1.0f) * root[0];
        const float b = (inside_at<CursorG>(QB, px, py, pz) ? -1.0f : 1.0f) * root[1];
        return blend_value(op, a, b, amount);
    }
};

__global__ __launch_bounds__(LEVEL_THREADS) void k_blend_level(QueryScene QA, DistScene DA, QueryScene QB, DistScene DB, int op, float amount,
                                                               const LevelBlock *__restrict__ blocks, uint32_t nblocks, uint32_t nchild, float S,
                                                               int may_split, uint2 *__restrict__ V, uint8_t *__restrict__ split,
                                                               unsigned long long *__restrict__ visited)
{
    __shared__ uint2 stack[MESH_MAX_DEPTH * LEVEL_THREADS];
    level_body(BlendValue{QA, DA, QB, DB, op, amount, visited}, blocks, nblocks, nchild, S, may_split, V, split, stack + threadIdx.x);
}

}  // namespace sdfhip
