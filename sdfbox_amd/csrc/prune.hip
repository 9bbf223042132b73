// libsdfhip.so, pruning: sdfhip_scene_prune -- the blocks of a resident scene that their parent already describes are removed, the
// result a new handle.
//
// Replaces: nothing in the reference's code; a tree there is immutable once built, and sdfhip_scene_edit (edit.hip) only grows one.
//
// The rule, pinned (include/sdfhip.h; fp32, each operation rounded on its own in the order written):
//   inherited byte   for an internal node P of depth d, S = 2^-d, bytes b[0..7]: f[j] = ((b[j] / 255.0f) - 0.25f) * S * 2.0f; child i's
//                    corner k sits at t_a = ((i >> a & 1) + (k >> a & 1)) * 0.5f; v = trilerp(f, t_x, t_y, t_z), lerp(a, b, t) =
//                    a + (b - a) * t along x, then y, then z; q(i, k) = floorf(saturate(v / 2 / (S * 0.5f) + 0.25f) * 255) -- what
//                    the edit gives a new child before the brush touches it
//   redundant block  P's eight children, iff every child is a leaf or has become one by this rule, and either their depth d + 1
//                    exceeds max_depth (when max_depth >= 0) or all 64 bytes have |byte(i, k) - q(i, k)| <= tolerance (integers)
//   cascade          a redundant block is removed, P becomes a leaf with its own bytes; decided bottom-up
//   node order       survivors keep their relative order (new index = survivors with a lower old index), links remapped, bytes kept
//
// The passes, on the input's fused records (kernels: prune_kernels.h):
//   k_prune_expand      the internal nodes of level d -> those of level d + 1, from the root down: one list, the levels one
//                       behind the other (one host synchronisation per level: its count sizes the next launch)
//   k_prune_decide      per level from the deepest up: eight lanes per block, the verdict a ballot, a removed block's bits set
//   k_rank_scan_*       the survivors' ranks: the shared bitmap prefix (scan_device.h), over the complement of the removed bits
//   k_prune_compact     the survivors to the result's arrays, links remapped
// Then the arrays go to scene_from_arrays (grids, fused records) as the edit's do.
#include "prune_kernels.h"
#include "host_support.h"
#include "abi_guard.h"

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdlib>
#include <vector>

using namespace sdfhip;

static_assert(sizeof(sdfhip_prune_options) == 12 && sizeof(sdfhip_prune_stats) == 28, "the prune records of include/sdfhip.h");

namespace {

constexpr int PRUNE_LEVELS = 16;            // counters (levels 0 .. TREE_MAX_DEPTH)

int check_options(const sdfhip_prune_options *opt, int *tolerance, int *max_depth)
{
    *tolerance = 0; *max_depth = -1;
    if (!opt) return SDFHIP_OK;
    if (const int rc = check_options_size("scene_prune", opt, sizeof(sdfhip_prune_options), "size = sizeof(sdfhip_prune_options)")) return rc;
    if (opt->tolerance < -1 || opt->tolerance > 255)
        return fail(SDFHIP_ERR_ARG, "scene_prune: tolerance %d is neither -1 nor 0..255", opt->tolerance);
    if (opt->max_depth < -1 || opt->max_depth > TREE_MAX_DEPTH)
        return fail(SDFHIP_ERR_ARG, "scene_prune: max_depth %d is neither -1 nor 0..%d", opt->max_depth, TREE_MAX_DEPTH);
    *tolerance = opt->tolerance < 0 ? 0 : opt->tolerance;
    *max_depth = opt->max_depth;
    return SDFHIP_OK;
}

}  // namespace

extern "C" int sdfhip_scene_prune(sdfhip_scene *scene, const sdfhip_prune_options *opt, sdfhip_scene **out, sdfhip_octdata *host_out,
                                  sdfhip_prune_stats *stats)
try {
    const auto t0 = std::chrono::steady_clock::now();
    if (!out) return fail(SDFHIP_ERR_ARG, "scene_prune: null argument");
    *out = nullptr;
    int tol = 0, maxd = -1;
    if (const int rc = check_options(opt, &tol, &maxd)) return rc;
    if (!scene) return fail(SDFHIP_ERR_ARG, "scene_prune: null argument");
    if (!scene->stack_ok || scene->depth > (uint32_t)TREE_MAX_DEPTH)
        return fail(SDFHIP_ERR_BAD_TREE, "scene_prune: the input tree is not consistent (or deeper than %d levels): no prune", TREE_MAX_DEPTH);

    CallFrame<4> call("scene_prune", scene->device, "SDFHIP_PRUNE_FAIL_ALLOC", t0);
    DeviceBuffers &bufs = call.bufs;
    const hipEvent_t *ev = call.cs.ev;

    const uint32_t n = scene->n;
    const uint32_t cap = (n - 1) / 8;                       // a consistent tree's internal nodes: every other node lies in one's block
    const uint32_t words = (n + 31) / 32, nchunk = (words + 1023) / 1024;
    uint32_t n_out = 0, depth_out = 0, blocks_removed = 0;
    int2 *dS = nullptr; uint2 *dV = nullptr;
    if (const int rc = call.run("the input scene is untouched", [&](hipStream_t st) -> int {
        uint32_t *list = bufs.get<uint32_t>(cap);
        uint32_t *removed = bufs.get<uint32_t>((size_t)words + 1);        // (+ 1: a block's byte may straddle the last word's end)
        uint32_t *pre = bufs.get<uint32_t>(words);
        uint32_t *chunk = bufs.get<uint32_t>((size_t)nchunk + 1);         // (+ 1: the survivors' count)
        PruneCounters *cnt = bufs.get<PruneCounters>(PRUNE_LEVELS);
        HIP_TRY(hipMemsetAsync(removed, 0, ((size_t)words + 1) * sizeof(uint32_t), st));
        HIP_TRY(hipMemsetAsync(cnt, 0, PRUNE_LEVELS * sizeof(PruneCounters), st));

        // the blocks to their levels: level d's parents at list[off[d] .. off[d] + count[d])
        NodeRec root;
        HIP_TRY(hipMemcpyAsync(&root, scene->nodes, sizeof root, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        uint32_t off[PRUNE_LEVELS + 1] = { 0 }, count[PRUNE_LEVELS] = { 0 };
        int levels = 0;
        HIP_TRY(hipEventRecord(ev[0], st));
        if ((int32_t)root.y >= 0 && cap) {
            HIP_TRY(hipMemsetAsync(list, 0, sizeof(uint32_t), st));            // the root: index 0
            count[0] = 1;
        }
        for (int d = 0; count[d]; d++) {
            levels = d + 1;
            off[d + 1] = off[d] + count[d];
            if (d >= TREE_MAX_DEPTH) return fail(SDFHIP_ERR_BAD_TREE, "scene_prune: the walk went deeper than %d levels", TREE_MAX_DEPTH);
            hipLaunchKernelGGL(k_prune_expand, grid_stride_blocks(8ull * count[d]), dim3(256), 0, st, scene->nodes, n, list + off[d], count[d],
                               list + off[d + 1], cap - off[d + 1], cnt + d + 1);
            HIP_TRY(hipGetLastError());
            PruneCounters c;
            HIP_TRY(hipMemcpyAsync(&c, cnt + d + 1, sizeof c, hipMemcpyDeviceToHost, st));
            HIP_TRY(hipStreamSynchronize(st));
            if (c.n_blocks > cap - off[d + 1])
                return fail(SDFHIP_ERR_BAD_TREE, "scene_prune: more internal nodes than a consistent tree of %u nodes has", n);
            count[d + 1] = c.n_blocks;
        }
        // the verdicts, from the deepest level up
        for (int d = levels - 1; d >= 0; d--) {
            const int cut = maxd >= 0 && d + 1 > maxd ? 1 : 0;
            hipLaunchKernelGGL(k_prune_decide, grid_stride_blocks(8ull * count[d]), dim3(256), 0, st, scene->nodes, n, list + off[d], count[d],
                               ldexpf(1.0f, -d), cut, tol, removed, cnt + d);
        }
        // the survivors' ranks
        hipLaunchKernelGGL(k_rank_scan_words<PruneKeepWords>, dim3(nchunk), dim3(256), 0, st, PruneKeepWords{ removed, n }, words, pre, chunk);
        hipLaunchKernelGGL(k_rank_scan_chunks<true>, dim3(1), dim3(1024), 0, st, chunk, nchunk);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipEventRecord(ev[1], st));
        PruneCounters c[PRUNE_LEVELS];
        HIP_TRY(hipMemcpyAsync(c, cnt, sizeof c, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(&n_out, chunk + nchunk, sizeof n_out, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        for (int d = 0; d < levels; d++) {
            blocks_removed += c[d].removed;
            if (c[d].removed < count[d]) depth_out = (uint32_t)(d + 1);
        }
        if (n_out == 0 || n_out > n || (uint64_t)n_out + 8ull * blocks_removed != n)
            return fail(SDFHIP_ERR_BAD_TREE, "scene_prune: %u of %u nodes survive %u removed blocks: the tree's blocks overlap", n_out, n, blocks_removed);

        dS = bufs.get<int2>(n_out);
        dV = bufs.get<uint2>(n_out);
        HIP_TRY(hipEventRecord(ev[2], st));
        hipLaunchKernelGGL(k_prune_compact, grid_stride_blocks(n), dim3(256), 0, st, scene->nodes, n, removed, pre, chunk, n_out, dS, dV);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipEventRecord(ev[3], st));
        HIP_TRY(hipStreamSynchronize(st));
        return SDFHIP_OK;
    })) return rc;

    float ms_a = 0.0f, ms_b = 0.0f, scene_ms = 0.0f;
    if (const int rc = call.elapsed(&ms_a, 0, 1)) return rc;
    if (const int rc = call.elapsed(&ms_b, 2, 3)) return rc;
    if (const int rc = call.finish(dS, dV, n_out, (int)depth_out, out, host_out, &scene_ms)) return rc;
    if (stats) {
        stats->nodes_in = n; stats->nodes_out = n_out;
        stats->blocks_removed = blocks_removed; stats->depth_out = depth_out;
        stats->kernel_ms = ms_a + ms_b; stats->scene_ms = scene_ms;
        stats->total_ms = call.total_ms();
    }
    return SDFHIP_OK;
}
SDFHIP_ABI_CATCH(sdfhip_scene_prune)
