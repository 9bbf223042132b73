// libsdfhip.so, composition: sdfhip_scene_compose -- one scene from many placed instances of resident scenes, in a single pass; the
// result a new handle (kernel: compose_kernels.h).
//
// Replaces: nothing in the reference's code; a tree there is immutable once built and sits where its builder put it.
//
// The rule, pinned (include/sdfhip.h; fp32, each operation rounded on its own in the order written):
//   u_k(p)           sdfhip_scene_place's value of instance k's source under instance k's placement, word for word (place_value)
//   fold             v = u_0; then in list order UNION fminf(v, u_k), INTERSECT fmaxf(v, u_k), SUBTRACT fmaxf(v, -u_k)
//   tree             sdfhip_scene_place's construct rule with this value: byte = FromFloat(v(corner), S), a node splits iff
//                    fabsf(v(centre)) < 2 S && d < depth
//   node order       breadth first: a level's blocks in ascending index of their parents, child i at block + i
//
// Per call: the instance table ({QueryScene, PlaceMap, op, form} per instance) goes to device memory on the call's stream, then the
// shared level loop (level_build.h's build_levels) runs with k_compose_level as its first pass, as place.hip runs it with
// k_place_level.  Each distinct source is read once, under its own lock, one after the other.  The call runs on a stream of its own
// with memory of its own; nothing is kept on the handles.
#include "compose_kernels.h"
#include "compose_host.h"     // check_instance, read_instance (shared with instances.hip); level_build.h: Source, build_levels
#include "abi_guard.h"

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <utility>
#include <vector>

using namespace sdfhip;
using namespace sdfhip::levels;

static_assert(sizeof(sdfhip_instance) == 64 && sizeof(sdfhip_compose_options) == 8 && sizeof(sdfhip_compose_stats) == 40,
              "the composition's records of include/sdfhip.h");
static_assert(SDFHIP_COMBINE_UNION == COMPOSE_UNION && SDFHIP_COMBINE_INTERSECT == COMPOSE_INTERSECT && SDFHIP_COMBINE_SUBTRACT == COMPOSE_SUBTRACT,
              "compose_kernels.h restates the header's codes");
static_assert(FORM_GENERIC == COMPOSE_FORM_GENERIC && FORM_GRID == COMPOSE_FORM_GRID && FORM_SPLIT == COMPOSE_FORM_SPLIT,
              "compose_kernels.h restates level_build.h's forms");

extern "C" int sdfhip_scene_compose(const sdfhip_instance *instances, uint32_t n_instances, const sdfhip_compose_options *opt, sdfhip_scene **out,
                                    sdfhip_octdata *host_out, sdfhip_compose_stats *stats)
try {
    const auto t0 = std::chrono::steady_clock::now();
    if (out) *out = nullptr;
    if (const int rc = check_instance_count("scene_compose", instances, n_instances)) return rc;
    if (!out && !host_out) return fail(SDFHIP_ERR_ARG, "scene_compose: both outputs are null");
    int depth_opt = -1;
    if (opt) {
        if (const int rc = check_options_size("scene_compose", opt, sizeof(sdfhip_compose_options), "size = sizeof(sdfhip_compose_options)")) return rc;
        if (opt->depth < -1 || opt->depth > TREE_MAX_DEPTH)
            return fail(SDFHIP_ERR_ARG, "scene_compose: depth %d is neither -1 nor 0..%d", opt->depth, TREE_MAX_DEPTH);
        depth_opt = opt->depth;
    }
    for (uint32_t k = 0; k < n_instances; k++)
        if (const int rc = check_instance("scene_compose", instances + k, k)) return rc;

    // What the call uses of each distinct handle is read under that handle's lock, one handle after the other and never two locks
    // at once, and the lock is released before any work is issued, as sdfhip_scene_place does: the records are only ever read.
    InstanceSources sources;
    std::vector<ComposeInstance> table(n_instances);          // (before `call`: alive until the stream that copies it is drained)
    uint64_t nodes_sum = 0;
    uint32_t deepest = 0;
    for (uint32_t k = 0; k < n_instances; k++) {
        const Source *src = nullptr;
        bool fresh = false;
        if (const int rc = read_instance("scene_compose", sources, instances[k], k, table[k], &src, &fresh)) return rc;
        if (fresh) nodes_sum += src->Q.n_nodes;
        if (depth_opt < 0 && src->depth > (uint32_t)TREE_MAX_DEPTH)
            return fail(SDFHIP_ERR_BAD_TREE,
                        "scene_compose: instance %u: the source is not a consistent tree of at most %d levels, so it has no depth to take: give one", k,
                        TREE_MAX_DEPTH);
        deepest = std::max(deepest, src->depth);
    }
    const int depth = depth_opt < 0 ? (int)deepest : depth_opt;
    const int device = sources.front().second.device;

    CallFrame<2> call("scene_compose", device, "SDFHIP_COMPOSE_FAIL_ALLOC", t0);
    LevelBuild R;
    if (const int rc = call.run("the sources are untouched", [&](hipStream_t st) -> int {
        ComposeInstance *d_table = call.bufs.get<ComposeInstance>(n_instances);
        HIP_TRY(hipMemcpyAsync(d_table, table.data(), n_instances * sizeof(ComposeInstance), hipMemcpyHostToDevice, st));
        const auto level = [&](const LevelBlock *blocks, uint32_t nblocks, uint32_t nchild, float S, int may_split, uint2 *V, uint8_t *split) {
            hipLaunchKernelGGL(k_compose_level, grid_stride_blocks(64ull * nblocks, LEVEL_MAX_WORKGROUPS), dim3(LEVEL_THREADS), 0, st, d_table, n_instances,
                               blocks, nblocks, nchild, S, may_split, V, split);
        };
        // (the arrays start from the distinct sources' sizes together; kernel_ms starts once the first of them are there: ev[0])
        const uint32_t nodes_in = (uint32_t)std::min<uint64_t>(nodes_sum, 0x7FFFFFFFull);
        if (const int rc = build_levels(call.what, call.bufs, st, nodes_in, depth, level, R, call.cs.ev[0])) return rc;
        HIP_TRY(hipEventRecord(call.cs.ev[1], st));
        HIP_TRY(hipStreamSynchronize(st));
        return SDFHIP_OK;
    })) return rc;

    float kernel_ms = 0.0f, scene_ms = 0.0f;
    if (const int rc = call.elapsed(&kernel_ms, 0, 1)) return rc;
    if (const int rc = call.finish(R.dS, R.dV, R.n_out, (int)R.depth_out, out, host_out, &scene_ms)) return rc;
    if (stats) {
        stats->nodes_out = R.n_out; stats->depth_out = R.depth_out; stats->levels = R.depth_out + 1; stats->instances = n_instances;
        stats->samples = (uint64_t)n_instances * R.points;
        stats->kernel_ms = kernel_ms; stats->scene_ms = scene_ms;
        stats->total_ms = call.total_ms();
        stats->pad_ = 0;
    }
    return SDFHIP_OK;
}
SDFHIP_ABI_CATCH(sdfhip_scene_compose)
