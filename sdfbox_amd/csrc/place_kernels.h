// The placement's value and its level pass (gfx950): a resident tree resampled under a rotation, a uniform scale and a translation.
// The lattice, the construct rule, the emit and the node order are level_kernels.h's; the host's loop is level_build.h's.
//
// The arithmetic is the contract of include/sdfhip.h (sdfhip_scene_place) and DESIGN.md section 8 (N11): fp32, each operation rounded
// on its own, in the order written (-ffp-contract=off); tests/place_restatement.py restates it with numpy.  The source's distance is
// what k_query_sample reads (find_fresh + sample_after_find, raymarch_device.h, untouched).
#pragma once
#include "query_kernels.h"   // QueryScene, grid_of; raymarch_device.h: the cursors, find_fresh, sample_after_find
#include "level_kernels.h"   // LevelBlock, level_body

namespace sdfhip {

// p = s R x + t, as the kernels use it: R row-major, inv = 1.0f / s (one IEEE division, on the host)
struct PlaceMap {
    float r[3][3];
    float s, inv;
    float tx, ty, tz;
};

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

// place_value as level_body takes it: no surface is searched, so there is no stack and nothing to count
template <class CursorT> struct PlaceValue {
    static constexpr int SOURCES = 0;
    QueryScene Q;
    PlaceMap M;
    __device__ __forceinline__ float operator()(float px, float py, float pz, uint2 *, uint32_t *) const
    {
        return place_value<CursorT>(Q, M, px, py, pz);
    }
};

template <class CursorT>
__global__ __launch_bounds__(LEVEL_THREADS) void k_place_level(QueryScene Q, PlaceMap M, const LevelBlock *__restrict__ blocks, uint32_t nblocks,
                                                               uint32_t nchild, float S, int may_split, uint2 *__restrict__ V,
                                                               uint8_t *__restrict__ split)
{
    level_body(PlaceValue<CursorT>{Q, M}, blocks, nblocks, nchild, S, may_split, V, split, nullptr);
}

}  // namespace sdfhip
