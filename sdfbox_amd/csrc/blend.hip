// libsdfhip.so, smooth blends and morphs: sdfhip_scene_blend -- the smooth union, intersection or difference of two resident scenes,
// or the in-between of the two, on their exact distances; the result a new handle (kernel: blend_kernels.h).
//
// Replaces: nothing in the reference's code; a tree there is immutable once built, and its only consumer draws one tree.
//
// The rule, pinned (include/sdfhip.h; fp32, each operation rounded on its own in the order written):
//   a, b      sdfhip_scene_offset's dist on each operand: the surface of level_a / level_b, the operand's own sign
//   smin      h = k > 0 ? fmaxf(k - fabsf(a - b), 0) / k : 0;  smin(a, b, k) = fminf(a, b) - ((h * h) * k) * 0.25f
//   value     UNION smin(a, b, k); INTERSECT -smin(-a, -b, k); SUBTRACT -smin(-a, b, k); MORPH a + (b - a) * t
//   tree      sdfhip_scene_offset's construct rule and node order, with this value
//
// Per call: the "surface below" bitmap of each operand (k_dist_mark; one when a == b and the levels agree), for a morph one 4-byte
// read per operand of the root's bit (an empty surface is refused), then the shared level loop (level_build.h's build_levels) with
// k_blend_level as its first pass.  The call runs on a stream of its own with memory of its own; nothing is kept on the handles.
#include "blend_kernels.h"
#include "distance_host.h"    // check_source, launch_mark; level_build.h: Source, build_levels
#include "abi_guard.h"

#include <algorithm>
#include <chrono>
#include <cmath>

using namespace sdfhip;
using namespace sdfhip::levels;

static_assert(sizeof(sdfhip_blend_options) == 24 && sizeof(sdfhip_blend_stats) == 64, "the blend records of include/sdfhip.h");
static_assert(SDFHIP_BLEND_UNION == BLEND_UNION && SDFHIP_BLEND_INTERSECT == BLEND_INTERSECT && SDFHIP_BLEND_SUBTRACT == BLEND_SUBTRACT &&
              SDFHIP_BLEND_MORPH == BLEND_MORPH, "blend_kernels.h restates the header's codes");

namespace {

// what the header refuses of the options, before any device call
int check_blend_options(const sdfhip_blend_options *opt)
{
    if (const int rc = check_options_size("scene_blend", opt, sizeof(sdfhip_blend_options), "size = sizeof(sdfhip_blend_options)")) return rc;
    if (opt->op < SDFHIP_BLEND_UNION || opt->op > SDFHIP_BLEND_MORPH) return fail(SDFHIP_ERR_ARG, "scene_blend: unknown op %d", opt->op);
    if (!std::isfinite(opt->amount)) return fail(SDFHIP_ERR_ARG, "scene_blend: the amount must be finite");
    if (opt->op == SDFHIP_BLEND_MORPH) {
        if (!(opt->amount >= 0.0f && opt->amount <= 1.0f)) return fail(SDFHIP_ERR_ARG, "scene_blend: a morph's t %g is outside [0, 1]", (double)opt->amount);
    } else if (!(opt->amount >= 0.0f)) {
        return fail(SDFHIP_ERR_ARG, "scene_blend: a blend radius %g is below 0", (double)opt->amount);
    }
    if (opt->depth < -1 || opt->depth > TREE_MAX_DEPTH)
        return fail(SDFHIP_ERR_ARG, "scene_blend: depth %d is neither -1 nor 0..%d", opt->depth, TREE_MAX_DEPTH);
    if (const int rc = check_level("scene_blend", opt->level_a)) return rc;
    return check_level("scene_blend", opt->level_b);
}

}  // namespace

extern "C" int sdfhip_scene_blend(sdfhip_scene *a, sdfhip_scene *b, const sdfhip_blend_options *opt, sdfhip_scene **out, sdfhip_octdata *host_out,
                                  sdfhip_blend_stats *stats)
try {
    const char *what = "scene_blend";
    const auto t0 = std::chrono::steady_clock::now();
    if (out) *out = nullptr;
    if (!opt) return fail(SDFHIP_ERR_ARG, "%s: null options", what);
    if (!out && !host_out) return fail(SDFHIP_ERR_ARG, "%s: both outputs are null", what);
    if (const int rc = check_blend_options(opt)) return rc;
    if (!a || !b) return fail(SDFHIP_ERR_ARG, "%s: null scene", what);
    // What the call uses of each handle is read under that handle's lock, one after the other, and the lock is released before any
    // work is issued, as sdfhip_scene_offset does: the records are only ever read.
    const Source A = read_source(a);
    const Source B = a == b ? A : read_source(b);
    if (A.device != B.device) return fail(SDFHIP_ERR_ARG, "%s: the operands live on devices %d and %d: one device", what, A.device, B.device);
    if (const int rc = check_source(what, A)) return rc;
    if (const int rc = check_source(what, B)) return rc;
    const int depth = opt->depth < 0 ? (int)std::max(A.depth, B.depth) : opt->depth;
    const int op = opt->op;
    const float amount = opt->amount;
    const bool one_bitmap = a == b && opt->level_a == opt->level_b;

    CallFrame<2> call(what, A.device, "SDFHIP_BLEND_FAIL_ALLOC", t0);
    DeviceBuffers &bufs = call.bufs;
    LevelBuild R;
    unsigned long long visited[2] = { 0, 0 };
    if (const int rc = call.run("both operands are untouched", [&](hipStream_t st) -> int {
        uint32_t *below_a = bufs.get<uint32_t>(bitmap_words(A.Q.n_nodes));
        uint32_t *below_b = one_bitmap ? below_a : bufs.get<uint32_t>(bitmap_words(B.Q.n_nodes));
        unsigned long long *d_visited = bufs.get<unsigned long long>(2);
        HIP_TRY(hipMemsetAsync(d_visited, 0, 2 * sizeof *d_visited, st));
        HIP_TRY(hipEventRecord(call.cs.ev[0], st));
        if (const int rc = launch_mark(A, opt->level_a, below_a, st)) return rc;
        if (!one_bitmap)
            if (const int rc = launch_mark(B, opt->level_b, below_b, st)) return rc;
        if (op == SDFHIP_BLEND_MORPH) {
            // inf * 0 and inf - inf mean nothing: a surface below the root or none at all, one word per operand
            uint32_t root_a = 0, root_b = 0;
            HIP_TRY(hipMemcpyAsync(&root_a, below_a, sizeof root_a, hipMemcpyDeviceToHost, st));
            HIP_TRY(hipMemcpyAsync(&root_b, below_b, sizeof root_b, hipMemcpyDeviceToHost, st));
            HIP_TRY(hipStreamSynchronize(st));
            if (!(root_a & 1u) || !(root_b & 1u))
                return fail(SDFHIP_ERR_ARG, "%s: operand %s has an empty surface at its level: there is no distance to morph", what, root_a & 1u ? "b" : "a");
        }
        const DistScene DA{A.Q.nodes, A.Q.n_nodes, below_a, opt->level_a}, DB{B.Q.nodes, B.Q.n_nodes, below_b, opt->level_b};
        const auto level = [&](const LevelBlock *blocks, uint32_t nblocks, uint32_t nchild, float S, int may_split, uint2 *V, uint8_t *split) {
            hipLaunchKernelGGL(k_blend_level, grid_stride_blocks(64ull * nblocks, LEVEL_MAX_WORKGROUPS), dim3(LEVEL_THREADS), 0, st, A.Q, DA, B.Q, DB, op, amount,
                               blocks, nblocks, nchild, S, may_split, V, split, d_visited);
        };
        // (the arrays start from the two operands' sizes together)
        const uint32_t nodes_in = (uint32_t)std::min<uint64_t>((uint64_t)A.Q.n_nodes + B.Q.n_nodes, 0x7FFFFFFFull);
        if (const int rc = build_levels(what, bufs, st, nodes_in, depth, level, R)) return rc;
        HIP_TRY(hipEventRecord(call.cs.ev[1], st));
        HIP_TRY(hipMemcpyAsync(visited, d_visited, sizeof visited, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        return SDFHIP_OK;
    })) return rc;

    float kernel_ms = 0.0f, scene_ms = 0.0f;
    if (const int rc = call.elapsed(&kernel_ms, 0, 1)) return rc;
    if (const int rc = call.finish(R.dS, R.dV, R.n_out, (int)R.depth_out, out, host_out, &scene_ms)) return rc;
    if (stats) {
        stats->nodes_a = A.Q.n_nodes; stats->nodes_b = B.Q.n_nodes; stats->nodes_out = R.n_out; stats->depth_out = R.depth_out;
        stats->levels = R.depth_out + 1; stats->pad0_ = 0;
        stats->points = R.points; stats->visited_a = visited[0]; stats->visited_b = visited[1];
        stats->kernel_ms = kernel_ms; stats->scene_ms = scene_ms;
        stats->total_ms = call.total_ms();
        stats->pad_ = 0;
    }
    return SDFHIP_OK;
}
SDFHIP_ABI_CATCH(sdfhip_scene_blend)
