// libsdfhip.so, space carving: sdfhip_scene_edit -- sphere and box brushes applied to a resident scene, the result a new handle.
//
// Replaces: nothing in the reference's code.  Its README lists "Add support for modeling, as efficient space carving is one of the
// main benefits of distance fields" under "Plans"; a tree there is immutable once built (SdfGen/dllmain.cpp:295-319).
//
// Per edit, level by level from the root (kernels: edit_kernels.h):
//   k_edit_original   the frontier of original nodes: a node the brush cannot reach is skipped with its subtree, the others get
//                     their bytes edited in place, internal ones push their children, leaves the brush refines are collected
//   k_edit_new        the new nodes of the level (blocks emitted under the level above's splits): interpolated pre-edit values,
//                     the edit, the split rule
//   k_rank_scan_*     the splits' ranks by index, from a bitmap over the node indices (scan_device.h; only the words between the
//   k_edit_emit       lowest and the highest split are scanned) -> blocks appended at the end in the order (depth, parent index)
// One host synchronisation per level that has work, per edit: the counts of the next level size its launches and buffers.
// Then the arrays go to scene_from_arrays (grids, fused records) as the point-cloud builder's do.
#include "edit_kernels.h"
#include "host_support.h"
#include "abi_guard.h"

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <new>
#include <utility>
#include <vector>

using namespace sdfhip;

namespace {

constexpr int EDIT_LEVELS = 16;             // counters per edit (levels 0 .. TREE_MAX_DEPTH)
constexpr float HALF_SQRT3 = 0.866025404f;  // SdfGen's HalfSqrt3

int check_edit(const sdfhip_edit &e, uint32_t i)
{
    if (e.op != SDFHIP_EDIT_CARVE && e.op != SDFHIP_EDIT_ADD) return fail(SDFHIP_ERR_ARG, "scene_edit: edit %u: unknown op %d", i, e.op);
    if (e.brush != SDFHIP_BRUSH_SPHERE && e.brush != SDFHIP_BRUSH_BOX)
        return fail(SDFHIP_ERR_ARG, "scene_edit: edit %u: unknown brush %d", i, e.brush);
    const int np = e.brush == SDFHIP_BRUSH_SPHERE ? 4 : 6;
    for (int k = 0; k < np; k++)
        if (!std::isfinite(e.params[k])) return fail(SDFHIP_ERR_ARG, "scene_edit: edit %u: parameter %d is not finite", i, k);
    for (int k = 3; k < np; k++)
        if (!(e.params[k] > 0.0f)) return fail(SDFHIP_ERR_ARG, "scene_edit: edit %u: a brush radius or half extent must be > 0", i);
    return SDFHIP_OK;
}

}  // namespace

extern "C" int sdfhip_scene_edit(sdfhip_scene *scene, const sdfhip_edit *edits, uint32_t n_edits, int32_t max_depth, sdfhip_scene **out,
                                 sdfhip_octdata *host_out, sdfhip_edit_stats *stats)
try {
    const auto t0 = std::chrono::steady_clock::now();
    if (!scene || !out || (n_edits && !edits)) return fail(SDFHIP_ERR_ARG, "scene_edit: null argument");
    *out = nullptr;
    if (max_depth < -1 || max_depth > TREE_MAX_DEPTH)
        return fail(SDFHIP_ERR_ARG, "scene_edit: max_depth %d is neither -1 nor 0..%d", max_depth, TREE_MAX_DEPTH);
    for (uint32_t i = 0; i < n_edits; i++)
        if (const int rc = check_edit(edits[i], i)) return rc;
    if (!scene->stack_ok || scene->depth > (uint32_t)TREE_MAX_DEPTH)
        return fail(SDFHIP_ERR_BAD_TREE, "scene_edit: the input tree is not consistent (or deeper than %d levels): no edit", TREE_MAX_DEPTH);
    const int maxd = max_depth < 0 ? (int)scene->depth : max_depth;

    CallFrame<2> call("scene_edit", scene->device, "SDFHIP_EDIT_FAIL_ALLOC", t0);
    DeviceBuffers &ws = call.bufs;

    uint64_t n_cur = scene->n;
    uint32_t depth_out = scene->depth;
    uint64_t visited = 0, changed = 0, blocks = 0;
    int2 *dS = nullptr; uint2 *dV = nullptr;
    size_t cap_nodes = 0;
    if (const int rc = call.run("the input scene is untouched", [&](hipStream_t st) -> int {
        // the arrays: the input's records, unfused, with room to grow
        cap_nodes = (size_t)n_cur + (n_cur >> 4) + 4096;
        dS = ws.get<int2>(cap_nodes);
        dV = ws.get<uint2>(cap_nodes);
        EditEntry *fr_cur = nullptr, *fr_next = nullptr;
        EditSplit *splits = nullptr, *par_cur = nullptr, *par_next = nullptr;
        uint32_t *bitmap = nullptr, *pre = nullptr, *chunk = nullptr;
        size_t c_fr_cur = 0, c_fr_next = 0, c_splits = 0, c_par_cur = 0, c_par_next = 0, c_bitmap = 0, c_pre = 0, c_chunk = 0;
        EditCounters *cnt = ws.get<EditCounters>(EDIT_LEVELS);

        HIP_TRY(hipEventRecord(call.cs.ev[0], st));
        hipLaunchKernelGGL(k_edit_unfuse, grid_stride_blocks(n_cur, 8192), dim3(256), 0, st, scene->nodes, dS, dV, (uint32_t)n_cur);
        HIP_TRY(hipGetLastError());
        for (uint32_t ei = 0; ei < n_edits; ei++) {
            const sdfhip_edit &E = edits[ei];
            EditBrush B;
            B.carve = E.op == SDFHIP_EDIT_CARVE ? 1 : 0;
            B.box = E.brush == SDFHIP_BRUSH_BOX ? 1 : 0;
            B.cx = E.params[0]; B.cy = E.params[1]; B.cz = E.params[2];
            B.a = E.params[3]; B.b = B.box ? E.params[4] : 0.0f; B.c = B.box ? E.params[5] : 0.0f;
            // beyond this every corner's brush byte is 0 (carve) or 255 (add): s is 1-Lipschitz, a corner lies sqrt(3)/2 S from the
            // centre, and q(g) saturates for g <= -S/2 and g >= 3S/2 -- no byte changes, and the brush cannot win at the centre
            B.cull = HALF_SQRT3 + (B.carve ? 0.5f : 1.5f) + 0.015625f;
            B.max_depth = maxd;

            HIP_TRY(hipMemsetAsync(cnt, 0, EDIT_LEVELS * sizeof(EditCounters), st));
            ws.ensure(fr_cur, c_fr_cur, 1);
            HIP_TRY(hipMemsetAsync(fr_cur, 0, sizeof(EditEntry), st));          // the root: index 0, cell (0, 0, 0)
            uint64_t n_orig = 1, n_new = 0, first_new = 0;
            for (int d = 0; n_orig || n_new; d++) {
                if (d >= EDIT_LEVELS - 1) return fail(SDFHIP_ERR_BAD_TREE, "scene_edit: the walk went deeper than %d levels", EDIT_LEVELS - 1);
                const float S = ldexpf(1.0f, -d);
                ws.ensure(fr_next, c_fr_next, 8 * n_orig);
                ws.ensure(splits, c_splits, n_orig + n_new);
                if (c_bitmap < (n_cur >> 5) + 1) {                                 // (all zero between levels: a new one is zeroed once)
                    ws.ensure(bitmap, c_bitmap, (n_cur >> 5) + 1);
                    HIP_TRY(hipMemsetAsync(bitmap, 0, c_bitmap * sizeof(uint32_t), st));
                }
                if (n_orig)
                    hipLaunchKernelGGL(k_edit_original, grid_stride_blocks(n_orig), dim3(256), 0, st, B, fr_cur, (uint32_t)n_orig, d, S, dS, dV, fr_next,
                                       splits, bitmap, cnt + d);
                if (n_new)
                    hipLaunchKernelGGL(k_edit_new, grid_stride_blocks(n_new), dim3(256), 0, st, B, par_cur, (uint32_t)first_new, (uint32_t)n_new, d, S,
                                       dS, dV, splits, bitmap, cnt + d);
                HIP_TRY(hipGetLastError());
                EditCounters c;
                HIP_TRY(hipMemcpyAsync(&c, cnt + d, sizeof c, hipMemcpyDeviceToHost, st));
                HIP_TRY(hipStreamSynchronize(st));
                visited += c.visited; changed += c.changed;
                n_orig = c.n_next;
                n_new = 0;
                if (c.n_split) {
                    if (n_cur + 8ull * c.n_split > 0x7FFFFFFFull)
                        return fail(SDFHIP_ERR_ARG, "scene_edit: the result would have more than 2^31 - 1 nodes");
                    if (n_cur + 8ull * c.n_split > cap_nodes) {                    // grow the arrays, keeping what they hold
                        const size_t cap = (size_t)(n_cur + 8ull * c.n_split) + (size_t)(n_cur >> 2);
                        int2 *nS = ws.get<int2>(cap);
                        uint2 *nV = ws.get<uint2>(cap);
                        HIP_TRY(hipMemcpyAsync(nS, dS, n_cur * sizeof(int2), hipMemcpyDeviceToDevice, st));
                        HIP_TRY(hipMemcpyAsync(nV, dV, n_cur * sizeof(uint2), hipMemcpyDeviceToDevice, st));
                        HIP_TRY(hipStreamSynchronize(st));
                        ws.drop(dS); ws.drop(dV);
                        dS = nS; dV = nV; cap_nodes = cap;
                    }
                    const uint32_t lo = ~c.lo_inv, w0 = lo >> 5, m = (c.hi >> 5) - w0 + 1, nchunk = (m + 1023) / 1024;
                    ws.ensure(pre, c_pre, m);
                    ws.ensure(chunk, c_chunk, nchunk);
                    ws.ensure(par_next, c_par_next, c.n_split);
                    hipLaunchKernelGGL(k_rank_scan_words<EditWindowWords>, dim3(nchunk), dim3(256), 0, st, EditWindowWords{ bitmap, w0 }, m, pre, chunk);
                    hipLaunchKernelGGL(k_rank_scan_chunks<false>, dim3(1), dim3(1024), 0, st, chunk, nchunk);
                    hipLaunchKernelGGL(k_edit_emit, grid_stride_blocks(c.n_split), dim3(256), 0, st, splits, c.n_split, bitmap, w0, pre, chunk,
                                       (uint32_t)n_cur, dS, par_next);
                    HIP_TRY(hipGetLastError());
                    HIP_TRY(hipMemsetAsync(bitmap + w0, 0, (size_t)m * sizeof(uint32_t), st));
                    first_new = n_cur;
                    n_new = 8ull * c.n_split;
                    n_cur += n_new;
                    blocks += c.n_split;
                    if ((uint32_t)(d + 1) > depth_out) depth_out = (uint32_t)(d + 1);
                    std::swap(par_cur, par_next); std::swap(c_par_cur, c_par_next);
                }
                std::swap(fr_cur, fr_next); std::swap(c_fr_cur, c_fr_next);
            }
        }
        HIP_TRY(hipEventRecord(call.cs.ev[1], st));
        HIP_TRY(hipStreamSynchronize(st));
        return SDFHIP_OK;
    })) return rc;

    float edit_ms = 0.0f, scene_ms = 0.0f;
    if (const int rc = call.elapsed(&edit_ms, 0, 1)) return rc;
    if (const int rc = call.finish(dS, dV, (uint32_t)n_cur, (int)depth_out, out, host_out, &scene_ms)) return rc;
    if (stats) {
        stats->nodes_in = scene->n; stats->nodes_out = (uint32_t)n_cur;
        stats->nodes_visited = (uint32_t)std::min<uint64_t>(visited, 0xFFFFFFFFu);
        stats->nodes_changed = (uint32_t)std::min<uint64_t>(changed, 0xFFFFFFFFu);
        stats->blocks_added = (uint32_t)blocks; stats->depth_out = depth_out;
        stats->edit_ms = edit_ms; stats->scene_ms = scene_ms;
        stats->total_ms = call.total_ms();
    }
    return SDFHIP_OK;
}
SDFHIP_ABI_CATCH(sdfhip_scene_edit)
