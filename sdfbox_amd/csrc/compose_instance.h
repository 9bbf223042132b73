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

}  // namespace sdfhip
