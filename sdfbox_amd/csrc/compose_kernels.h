// Composition of placed instances (gfx950): the value of sdfhip_scene_compose and its level pass.  k_compose_level is not a
// template: included by compose.hip ONLY.  Host side, C ABI: compose.hip.
//
// Replaces: nothing in the reference's code -- a tree there is immutable once built and sits where its builder put it.
//
// The rule is the contract of include/sdfhip.h (sdfhip_scene_compose) and DESIGN.md section 8 (N16): fp32, each operation rounded on
// its own, in the order written (-ffp-contract=off); tests/compose_restatement.py restates it with numpy on place_restatement.value.
//   u_k(p)    place_value (place_kernels.h) of instance k's source under instance k's map: the placement's value, untouched
//   fold      v = u_0; then in list order UNION fminf(v, u_k), INTERSECT fmaxf(v, u_k), SUBTRACT fmaxf(v, -u_k)
//   tree      the construct rule and node order of the placement: k_compose_level is level_body (level_kernels.h) on ComposeValue
//
// k_compose_level.  A lane walks the whole instance list for its point: the list, and so the loop's bound, the table index and each
// instance's cursor form, is the same for every lane of every wave, and the table is read through a uniform index (the compiler may
// take it through the scalar cache).  The instances of one call may have different cursor forms -- a source with a full-depth grid
// beside one without -- so the form is a uniform switch inside the loop and not a template parameter of the kernel.  Every instance
// is looked up at every point: nothing is skipped, the bytes are the rule's whatever the arrangement.
#pragma once
#include "compose_instance.h"   // ComposeInstance, compose_instance_value, the op and form codes (shared with instances_kernels.h)
#include "level_kernels.h"      // LevelBlock, LEVEL_THREADS, level_body

namespace sdfhip {

// the fold as level_body takes it: no surface is searched, so there is no stack and nothing to count
struct ComposeValue {
    static constexpr int SOURCES = 0;
    const ComposeInstance *table;
    uint32_t n;
    __device__ __forceinline__ float operator()(float px, float py, float pz, uint2 *, uint32_t *) const
    {
        float v = 0.0f;
        for (uint32_t k = 0; k < n; k++) {
            const float u = compose_instance_value(table[k], px, py, pz);
            if (k == 0) { v = u; continue; }                  // (the host has made sure that instance 0 is a union)
            switch (table[k].op) {
            case COMPOSE_UNION: v = fminf(v, u); break;
            case COMPOSE_INTERSECT: v = fmaxf(v, u); break;
            default: v = fmaxf(v, -u); break;
            }
        }
        return v;
    }
};

__global__ __launch_bounds__(LEVEL_THREADS) void k_compose_level(const ComposeInstance *__restrict__ table, uint32_t n_instances,
                                                                 const LevelBlock *__restrict__ blocks, uint32_t nblocks, uint32_t nchild, float S,
                                                                 int may_split, uint2 *__restrict__ V, uint8_t *__restrict__ split)
{
    level_body(ComposeValue{table, n_instances}, blocks, nblocks, nchild, S, may_split, V, split, nullptr);
}

}  // namespace sdfhip
