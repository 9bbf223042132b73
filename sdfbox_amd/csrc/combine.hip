// libsdfhip.so, combination: sdfhip_scene_combine -- the union, intersection or difference of two resident scenes, the result a new
// handle.
//
// Replaces: nothing in the reference's code; a tree there is immutable once built, and its only consumer draws one tree.
//
// The rule, pinned (include/sdfhip.h; fp32, each operation rounded on its own in the order written):
//   cells            a cell is a node of the result iff it is a node of A or of B; a result node has children iff A's node there
//                    has, or B's has, and its depth is below max_depth (when one is given)
//   operand bytes    the operand's own eight bytes where it has the node; else its leaf's bytes carried down to the cell, one level
//                    at a time by prune's inherited byte q(i, k) (sdf_interp.h, sdf_bytes.h), quantised at every level
//   negation         SUBTRACT only, on B's bytes at the cell, after the inheritance: neg(b) = from_float(-to_float(b, S), S)
//   result byte      UNION min(a, b), INTERSECT max(a, b), SUBTRACT max(a, neg(b)), per corner
//   node order       breadth first: a level's blocks in ascending result index of their parents, child i at block + i
//
// The passes, per level from the root, on the operands' fused records (kernels: combine_kernels.h).  The levels' items lie one
// behind the other in one array, an item's place its node's index in the result:
//   k_combine_level     the level's bytes, its split bitmap (one ballot per wave), the cells both operands have
//   k_rank_scan_*       the splits' ranks: the shared bitmap prefix (scan_device.h), its total the level's blocks (one host
//                       synchronisation per level: the count sizes the next level's launches)
//   k_combine_emit      eight lanes per splitting item: the links, and the next level's items
// Then the arrays go to scene_from_arrays (grids, fused records) as the edit's and the prune's do.
#include "combine_kernels.h"
#include "host_support.h"
#include "abi_guard.h"

#include <algorithm>
#include <chrono>
#include <cmath>
#include <functional>
#include <initializer_list>
#include <mutex>

using namespace sdfhip;

static_assert(sizeof(sdfhip_combine_options) == 8 && sizeof(sdfhip_combine_stats) == 32, "the combine records of include/sdfhip.h");

namespace {

int check_options(const sdfhip_combine_options *opt, int *max_depth)
{
    *max_depth = -1;
    if (!opt) return SDFHIP_OK;
    if (const int rc = check_options_size("scene_combine", opt, sizeof(sdfhip_combine_options), "size = sizeof(sdfhip_combine_options)")) return rc;
    if (opt->max_depth < -1 || opt->max_depth > TREE_MAX_DEPTH)
        return fail(SDFHIP_ERR_ARG, "scene_combine: max_depth %d is neither -1 nor 0..%d", opt->max_depth, TREE_MAX_DEPTH);
    *max_depth = opt->max_depth;
    return SDFHIP_OK;
}

}  // namespace

extern "C" int sdfhip_scene_combine(sdfhip_scene *a, sdfhip_scene *b, int32_t op, const sdfhip_combine_options *opt, sdfhip_scene **out,
                                    sdfhip_octdata *host_out, sdfhip_combine_stats *stats)
try {
    const auto t0 = std::chrono::steady_clock::now();
    if (!out) return fail(SDFHIP_ERR_ARG, "scene_combine: null argument");
    *out = nullptr;
    int maxd = -1;
    if (const int rc = check_options(opt, &maxd)) return rc;
    if (op != SDFHIP_COMBINE_UNION && op != SDFHIP_COMBINE_INTERSECT && op != SDFHIP_COMBINE_SUBTRACT)
        return fail(SDFHIP_ERR_ARG, "scene_combine: unknown op %d", op);
    if (!a || !b) return fail(SDFHIP_ERR_ARG, "scene_combine: null argument");
    // What the call uses of the handles -- records, length, depth, device, verdict: fixed at upload -- is read under both handles'
    // locks, taken in address order (one when a == b: two calls with the operands exchanged cannot wait for each other), and the
    // locks are released before any work is issued.  The records are only ever read, as sdfhip_scene_prune reads its input's
    // without a lock: renders, queries and meshes of the operands on other threads do not wait for the combination.
    struct Operand { const NodeRec *nodes; uint32_t n, depth; int device, stack_ok; } A, B;
    {
        sdfhip_scene *lo = std::min(a, b, std::less<sdfhip_scene *>()), *hi = std::max(a, b, std::less<sdfhip_scene *>());
        std::unique_lock<std::mutex> lk_lo(lo->lock), lk_hi;
        if (hi != lo) lk_hi = std::unique_lock<std::mutex>(hi->lock);
        A = Operand{ a->nodes, a->n, a->depth, a->device, a->stack_ok };
        B = Operand{ b->nodes, b->n, b->depth, b->device, b->stack_ok };
    }
    if (A.device != B.device)
        return fail(SDFHIP_ERR_ARG, "scene_combine: the operands live on devices %d and %d: one device", A.device, B.device);
    for (const Operand *x : { &A, &B })
        if (!x->stack_ok || x->depth > (uint32_t)TREE_MAX_DEPTH)
            return fail(SDFHIP_ERR_BAD_TREE, "scene_combine: operand %s is not a consistent tree (or deeper than %d levels): no combination",
                        x == &A ? "a" : "b", TREE_MAX_DEPTH);

    CallFrame<2> call("scene_combine", A.device, "SDFHIP_COMBINE_FAIL_ALLOC", t0);
    DeviceBuffers &bufs = call.bufs;

    const uint32_t nA = A.n, nB = B.n;
    // nothing is pruned and nothing invented: every result node is a node of A or of B, and the root is one of both; under a cut, no
    // more than the full tree of that depth
    uint64_t bound = (uint64_t)nA + nB - 1;
    if (maxd >= 0) bound = std::min<uint64_t>(bound, ((1ull << (3 * (maxd + 1))) - 1) / 7);
    const uint32_t cap = (uint32_t)std::min<uint64_t>(bound, 0x7FFFFFFFull);
    const uint32_t words = 2 * ((cap + 63) / 64), nchunk_max = (words + 1023) / 1024;
    uint32_t n_out = 1, depth_out = 0, shared = 0;
    int2 *dS = nullptr; uint2 *dV = nullptr;
    if (const int rc = call.run("both operands are untouched", [&](hipStream_t st) -> int {
        dS = bufs.get<int2>(cap);
        dV = bufs.get<uint2>(cap);
        CombineItem *items = bufs.get<CombineItem>(cap);
        uint32_t *split = bufs.get<uint32_t>(words);
        uint32_t *pre = bufs.get<uint32_t>(words);
        uint32_t *chunk = bufs.get<uint32_t>((size_t)nchunk_max + 1);         // (+ 1: the level's blocks)
        uint32_t *shared_count = bufs.get<uint32_t>(1);
        HIP_TRY(hipMemsetAsync(shared_count, 0, sizeof(uint32_t), st));

        HIP_TRY(hipEventRecord(call.cs.ev[0], st));
        hipLaunchKernelGGL(k_combine_root, dim3(1), dim3(64), 0, st, A.nodes, B.nodes, items, dS);
        HIP_TRY(hipGetLastError());
        uint32_t first = 0, n = 1;
        for (int d = 0;; d++) {
            if (d > TREE_MAX_DEPTH) return fail(SDFHIP_ERR_BAD_TREE, "scene_combine: the walk went deeper than %d levels", TREE_MAX_DEPTH);
            depth_out = (uint32_t)d;
            const float S = ldexpf(1.0f, -d);
            const int may_split = maxd < 0 || d < maxd ? 1 : 0;
            hipLaunchKernelGGL(k_combine_level, grid_stride_blocks(n), dim3(256), 0, st, A.nodes, nA, B.nodes, nB, items + first, n, first, cap, (int)op,
                               may_split, S, dV, split, shared_count);
            HIP_TRY(hipGetLastError());
            if (!may_split) break;
            const uint32_t m = (n + 31) / 32, nchunk = (m + 1023) / 1024;
            hipLaunchKernelGGL(k_rank_scan_words<CombineSplitWords>, dim3(nchunk), dim3(256), 0, st, CombineSplitWords{ split }, m, pre, chunk);
            hipLaunchKernelGGL(k_rank_scan_chunks<true>, dim3(1), dim3(1024), 0, st, chunk, nchunk);
            HIP_TRY(hipGetLastError());
            uint32_t n_split = 0;
            HIP_TRY(hipMemcpyAsync(&n_split, chunk + nchunk, sizeof n_split, hipMemcpyDeviceToHost, st));
            HIP_TRY(hipStreamSynchronize(st));
            if (!n_split) break;
            const uint64_t total = (uint64_t)n_out + 8ull * n_split;
            if (total > 0x7FFFFFFFull) return fail(SDFHIP_ERR_ARG, "scene_combine: the result would have more than 2^31 - 1 nodes");
            if (total > cap)
                return fail(SDFHIP_ERR_BAD_TREE, "scene_combine: more nodes than two consistent trees of %u and %u nodes combine to", nA, nB);
            hipLaunchKernelGGL(k_combine_emit, grid_stride_blocks(8ull * n), dim3(256), 0, st, A.nodes, nA, B.nodes, nB, items + first, n, first, cap, S,
                               split, pre, chunk, dS, items + first + n, 8u * n_split);
            HIP_TRY(hipGetLastError());
            first += n;
            n = 8u * n_split;
            n_out = (uint32_t)total;
        }
        HIP_TRY(hipEventRecord(call.cs.ev[1], st));
        HIP_TRY(hipMemcpyAsync(&shared, shared_count, sizeof shared, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        return SDFHIP_OK;
    })) return rc;

    float kernel_ms = 0.0f, scene_ms = 0.0f;
    if (const int rc = call.elapsed(&kernel_ms, 0, 1)) return rc;
    if (const int rc = call.finish(dS, dV, n_out, (int)depth_out, out, host_out, &scene_ms)) return rc;
    if (stats) {
        stats->nodes_a = nA; stats->nodes_b = nB; stats->nodes_out = n_out; stats->depth_out = depth_out;
        stats->nodes_shared = shared;
        stats->kernel_ms = kernel_ms; stats->scene_ms = scene_ms;
        stats->total_ms = call.total_ms();
    }
    return SDFHIP_OK;
}
SDFHIP_ABI_CATCH(sdfhip_scene_combine)
