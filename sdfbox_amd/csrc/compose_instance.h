// One placed instance as the device sees it (gfx950): the table entry and the value of one instance, shared by the composition's
// level pass (compose_kernels.h, compose.hip) and the assembly's consumers (instances_kernels.h, instances.hip).  Everything here is
// inline: the header may be included by any number of translation units.
//
// Replaces: nothing in the reference's code.  The rule is sdfhip_scene_compose's (include/sdfhip.h).
#pragma once
#include "place_kernels.h"      // place_value, PlaceMap; query_kernels.h: QueryScene, the cursors

namespace sdfhip {

enum { COMPOSE_UNION = 0, COMPOSE_INTERSECT = 1, COMPOSE_SUBTRACT = 2 };              // SDFHIP_COMBINE_* of include/sdfhip.h
enum { COMPOSE_FORM_GENERIC = 0, COMPOSE_FORM_GRID = 1, COMPOSE_FORM_SPLIT = 2 };     // levels::Form of level_build.h

// One entry of the call's instance table, in device memory: what place_value reads of the source, the map, how the instance joins
// what precedes it, and the cursor its look-ups take
struct ComposeInstance {
    QueryScene Q;
    PlaceMap M;
    int32_t op, form;
};

// u_k(p) by the instance's cursor form: all three give the same bytes
__device__ __forceinline__ float compose_instance_value(const ComposeInstance &I, float px, float py, float pz)
{
    switch (I.form) {
    case COMPOSE_FORM_GRID: return place_value<CursorFT<false, false>>(I.Q, I.M, px, py, pz);
    case COMPOSE_FORM_SPLIT: return place_value<CursorFT<false, true>>(I.Q, I.M, px, py, pz);
    default: return place_value<CursorG>(I.Q, I.M, px, py, pz);
    }
}

// The exact lower bound of u_k that needs no look-up (the argument: instances_kernels.h, "The exact skip"), shared by the assembly's
// consumers (instances_kernels.h) and the clash check (clash_kernels.h)
constexpr float INSTANCES_SKIP_FLOOR = -0.5625f;

// b_k(p) = (-0.5625f + e) * s: place_value's lines up to e, word for word
__device__ __forceinline__ float place_lower_bound(const PlaceMap &M, float px, float py, float pz)
{
    const float d0 = px - M.tx, d1 = py - M.ty, d2 = pz - M.tz;
    const float qx = ((M.r[0][0] * d0 + M.r[1][0] * d1) + M.r[2][0] * d2) * M.inv;
    const float qy = ((M.r[0][1] * d0 + M.r[1][1] * d1) + M.r[2][1] * d2) * M.inv;
    const float qz = ((M.r[0][2] * d0 + M.r[1][2] * d1) + M.r[2][2] * d2) * M.inv;
    const float cx = __builtin_fminf(__builtin_fmaxf(qx, 0.0f), 1.0f);
    const float cy = __builtin_fminf(__builtin_fmaxf(qy, 0.0f), 1.0f);
    const float cz = __builtin_fminf(__builtin_fmaxf(qz, 0.0f), 1.0f);
    const float ex = qx - cx, ey = qy - cy, ez = qz - cz;
    return (INSTANCES_SKIP_FLOOR + sqrtf((ex * ex + ey * ey) + ez * ez)) * M.s;
}

}  // namespace sdfhip
