// libsdfhip.so, placement: sdfhip_scene_place -- a resident scene rotated, scaled and moved by resampling it into a new tree, the
// result a new handle.
//
// Replaces: nothing in the reference's code; a tree there is immutable once built and sits where its builder put it.
//
// The rule, pinned (include/sdfhip.h; fp32, each operation rounded on its own in the order written):
//   inverse map      d = p - t, inv = 1.0f / s, q_a = ((R[0][a] d_0 + R[1][a] d_1) + R[2][a] d_2) * inv
//   value            qc = min(max(q, 0), 1), e = q - qc, D = sdfhip_scene_sample's distance at qc,
//                    value(p) = (D + sqrtf((e_0 e_0 + e_1 e_1) + e_2 e_2)) * s
//   tree             sdfhip_trimesh_build's construct rule with this value: byte = FromFloat(value(corner), S), a node splits iff
//                    fabsf(value(centre)) < 2 S && d < depth
//   node order       breadth first: a level's blocks in ascending index of their parents, child i at block + i
//
// The passes, per level from the root (kernels: place_kernels.h).  A level's blocks of eight siblings carry their parent's integer
// coordinates; the result's arrays grow as the levels arrive:
//   k_place_level      a wave per block, a lane per point of its lattice: the level's bytes and its split bitmap
//   k_rank_scan_*      the splits' ranks: the shared bitmap prefix (scan_device.h), its total the next level's blocks (one host
//                      synchronisation per level: the count sizes the next level's memory and launches)
//   k_place_emit       eight lanes per splitting node: the links, appended behind the level, and the next level's blocks
// Then the arrays go to scene_from_arrays (grids, fused records) as the edit's, the prune's and the combination's do.
#include "place_kernels.h"
#include "host_support.h"
#include "abi_guard.h"

#include <algorithm>
#include <chrono>
#include <cmath>
#include <mutex>
#include <type_traits>

using namespace sdfhip;

static_assert(sizeof(sdfhip_placement) == 60 && sizeof(sdfhip_place_stats) == 40, "the placement records of include/sdfhip.h");

namespace {

// Which cursor a look-up takes: no cell index is wanted, so the choice is the march's (query.hip's form_of for a march): the grid
// wherever the handle has a full-depth one -- dense, or coarse level + fine blocks -- else the shader's walk along the links
enum Form { FORM_GENERIC = 0, FORM_GRID = 1, FORM_SPLIT = 2 };
Form form_of(const sdfhip_scene *s)
{
    if (!scene_has_full_depth_grid(s)) return FORM_GENERIC;
    return s->fine_bits ? FORM_SPLIT : FORM_GRID;
}
QueryScene scene_of(const sdfhip_scene *s)
{
    return QueryScene{s->nodes, s->n, s->d_top, s->d_fine, s->top_level, s->fine_bits};
}

// Both passes stride over their level with at most this many workgroups of four waves: 8 waves on each of the 1024 SIMDs of 256
// compute units, a level of more than 65 536 nodes in more than one sweep
constexpr uint32_t PLACE_MAX_WORKGROUPS = 2048;

// what the header refuses of a placement, before any device call
int check_placement(const sdfhip_placement *pl)
{
    if (const int rc = check_options_size("scene_place", pl, sizeof(sdfhip_placement), "size = sizeof(sdfhip_placement)")) return rc;
    bool finite = std::isfinite(pl->scale);
    for (int i = 0; i < 3; i++) {
        finite = finite && std::isfinite(pl->translation[i]);
        for (int j = 0; j < 3; j++) finite = finite && std::isfinite(pl->rotation[i][j]);
    }
    if (!finite) return fail(SDFHIP_ERR_ARG, "scene_place: rotation, scale and translation must be finite");
    if (!(pl->scale > 0.0f)) return fail(SDFHIP_ERR_ARG, "scene_place: scale %g is not above 0", (double)pl->scale);
    double worst = 0.0;
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) {
            double dot = 0.0;
            for (int k = 0; k < 3; k++) dot += (double)pl->rotation[i][k] * (double)pl->rotation[j][k];
            worst = std::max(worst, std::fabs(dot - (i == j ? 1.0 : 0.0)));
        }
    if (worst > 1e-4) return fail(SDFHIP_ERR_ARG, "scene_place: the rotation is not orthogonal (max |R R^T - I| = %g, the bound 1e-4)", worst);
    if (pl->depth < -1 || pl->depth > TREE_MAX_DEPTH)
        return fail(SDFHIP_ERR_ARG, "scene_place: depth %d is neither -1 nor 0..%d", pl->depth, TREE_MAX_DEPTH);
    return SDFHIP_OK;
}

void launch_level(Form form, const QueryScene &Q, const PlaceMap &M, const PlaceBlock *blocks, uint32_t nblocks, uint32_t nchild, float S,
                  int may_split, uint2 *V, uint8_t *split, hipStream_t st)
{
    const dim3 grid = grid_stride_blocks(64ull * nblocks, PLACE_MAX_WORKGROUPS), wg(PLACE_THREADS);
    switch (form) {
    case FORM_GRID: hipLaunchKernelGGL((k_place_level<CursorFT<false, false>>), grid, wg, 0, st, Q, M, blocks, nblocks, nchild, S, may_split, V, split); break;
    case FORM_SPLIT: hipLaunchKernelGGL((k_place_level<CursorFT<false, true>>), grid, wg, 0, st, Q, M, blocks, nblocks, nchild, S, may_split, V, split); break;
    default: hipLaunchKernelGGL((k_place_level<CursorG>), grid, wg, 0, st, Q, M, blocks, nblocks, nchild, S, may_split, V, split); break;
    }
}

}  // namespace

extern "C" int sdfhip_scene_place(sdfhip_scene *scene, const sdfhip_placement *pl, sdfhip_scene **out, sdfhip_octdata *host_out,
                                  sdfhip_place_stats *stats)
try {
    const auto t0 = std::chrono::steady_clock::now();
    if (out) *out = nullptr;
    if (!pl) return fail(SDFHIP_ERR_ARG, "scene_place: null placement");
    if (!out && !host_out) return fail(SDFHIP_ERR_ARG, "scene_place: both outputs are null");
    if (const int rc = check_placement(pl)) return rc;
    if (!scene) return fail(SDFHIP_ERR_ARG, "scene_place: null scene");
    // What the call uses of the handle -- records, grids, length, depth, device: fixed at upload -- is read under the handle's lock,
    // which is released before any work is issued, as sdfhip_scene_combine does.  The records and the grids are only ever read:
    // renders, queries and meshes of the source on other threads do not wait for the placement.
    QueryScene Q;
    Form form;
    uint32_t src_depth;
    int device;
    {
        std::lock_guard<std::mutex> lk(scene->lock);
        Q = scene_of(scene);
        form = form_of(scene);
        src_depth = scene->depth;
        device = scene->device;
    }
    if (pl->depth < 0 && src_depth > (uint32_t)TREE_MAX_DEPTH)
        return fail(SDFHIP_ERR_BAD_TREE, "scene_place: the source is not a consistent tree of at most %d levels, so it has no depth to take: give one",
                    TREE_MAX_DEPTH);
    const int depth = pl->depth < 0 ? (int)src_depth : pl->depth;
    PlaceMap M;
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) M.r[i][j] = pl->rotation[i][j];
    M.s = pl->scale; M.inv = 1.0f / pl->scale;
    M.tx = pl->translation[0]; M.ty = pl->translation[1]; M.tz = pl->translation[2];

    DeviceGuard g(device);
    if (!g.ok) return (void)hipGetLastError(), fail(SDFHIP_ERR_DEVICE, "scene_place: hipSetDevice(%d) failed", device);
    DeviceBuffers bufs("SDFHIP_PLACE_FAIL_ALLOC");
    CallStream<2> cs;                       // (after `bufs`: drained before the buffers are freed)
    if (const int rc = cs.open("")) return rc;
    const hipStream_t st = cs.st;

    uint32_t n_out = 1, depth_out = 0;
    uint64_t samples = 0;
    int2 *dS = nullptr; uint2 *dV = nullptr;
    try {
        // The result's arrays start with room for a tree of the source's size and double when a level does not fit: the levels
        // already written are copied over.  The per-level buffers are sized for what the arrays can hold -- a level is part of the
        // result -- and follow when those grow.  Every buffer is replaced only while the stream is idle.
        size_t cap = std::min<size_t>(std::max<size_t>((size_t)Q.n_nodes + Q.n_nodes / 2, 4096), 0x7FFFFFFFull);
        dS = bufs.get<int2>(cap);
        dV = bufs.get<uint2>(cap);
        bool idle = true;
        const auto room = [&](auto *&p, size_t &have, size_t need) -> int {       // contents not kept
            if (need <= have) return SDFHIP_OK;
            if (!idle) { HIP_TRY(hipStreamSynchronize(st)); idle = true; }
            if (p) bufs.drop(p);
            p = nullptr; have = 0;
            p = bufs.get<typename std::remove_reference<decltype(*p)>::type>(need);
            have = need;
            return SDFHIP_OK;
        };
        const auto grown = [&](auto *&p, size_t new_cap, size_t keep) -> int {    // the stream is idle
            auto *q = bufs.get<typename std::remove_reference<decltype(*p)>::type>(new_cap);
            HIP_TRY(hipMemcpyAsync(q, p, keep * sizeof *p, hipMemcpyDeviceToDevice, st));
            HIP_TRY(hipStreamSynchronize(st));
            bufs.drop(p);
            p = q;
            return SDFHIP_OK;
        };
        const auto words_of = [](size_t nodes) { return (nodes + 31) / 32; };
        PlaceBlock *cur = nullptr, *next = nullptr;
        uint32_t *split = nullptr, *pre = nullptr, *chunk = nullptr;
        size_t cur_cap = 0, next_cap = 0, split_cap = 0, pre_cap = 0, chunk_cap = 0;
        if (const int rc = room(cur, cur_cap, cap / 8 + 1)) return rc;
        HIP_TRY(hipMemsetAsync(cur, 0, sizeof(PlaceBlock), st));                 // the root's block: the cell at the origin
        HIP_TRY(hipMemsetAsync(dS, 0xFF, sizeof(int2), st));                     // the root: {-1, -1}

        HIP_TRY(hipEventRecord(cs.ev[0], st));
        uint32_t first = 0, n = 1, nblocks = 1, nchild = 1;
        for (int d = 0;; d++) {
            depth_out = (uint32_t)d;
            const float S = ldexpf(1.0f, -d);
            const int may_split = d < depth ? 1 : 0;
            const uint32_t m = (n + 31) / 32, nchunk = (m + 1023) / 1024;
            if (const int rc = room(split, split_cap, words_of(cap))) return rc;
            if (const int rc = room(pre, pre_cap, words_of(cap))) return rc;
            if (const int rc = room(chunk, chunk_cap, (words_of(cap) + 1023) / 1024 + 1)) return rc;        // (+ 1: the level's splits)
            idle = false;
            launch_level(form, Q, M, cur, nblocks, nchild, S, may_split, dV + first, reinterpret_cast<uint8_t *>(split), st);
            HIP_TRY(hipGetLastError());
            samples += nchild == 1 ? 9u : (uint64_t)PLACE_POINTS * nblocks;
            if (!may_split) break;
            hipLaunchKernelGGL(k_rank_scan_words<PlaceSplitWords>, dim3(nchunk), dim3(256), 0, st, PlaceSplitWords{ split, n }, m, pre, chunk);
            hipLaunchKernelGGL(k_rank_scan_chunks<true>, dim3(1), dim3(1024), 0, st, chunk, nchunk);
            HIP_TRY(hipGetLastError());
            uint32_t n_split = 0;
            HIP_TRY(hipMemcpyAsync(&n_split, chunk + nchunk, sizeof n_split, hipMemcpyDeviceToHost, st));
            HIP_TRY(hipStreamSynchronize(st));
            idle = true;
            if (!n_split) break;
            if (n_split > n) return fail(SDFHIP_ERR_DEVICE, "scene_place: %u splits among %u nodes", n_split, n);
            const uint64_t total = (uint64_t)n_out + 8ull * n_split;
            if (total > 0x7FFFFFFFull) return fail(SDFHIP_ERR_ARG, "scene_place: the result would have more than 2^31 - 1 nodes");
            if (total > cap) {
                const size_t new_cap = (size_t)std::min<uint64_t>(std::max<uint64_t>(total, 2ull * cap), 0x7FFFFFFFull);
                if (const int rc = grown(dS, new_cap, n_out)) return rc;
                if (const int rc = grown(dV, new_cap, n_out)) return rc;
                cap = new_cap;
            }
            if (const int rc = room(next, next_cap, cap / 8 + 1)) return rc;
            idle = false;
            hipLaunchKernelGGL(k_place_emit, grid_stride_blocks(8ull * n, PLACE_MAX_WORKGROUPS), dim3(256), 0, st, cur, n, nchild, first, split, pre, chunk, dS, (uint32_t)cap,
                               next, n_split);
            HIP_TRY(hipGetLastError());
            std::swap(cur, next);
            std::swap(cur_cap, next_cap);
            first += n;
            n = 8u * n_split; nblocks = n_split; nchild = 8;
            n_out = (uint32_t)total;
        }
        HIP_TRY(hipEventRecord(cs.ev[1], st));
        HIP_TRY(hipStreamSynchronize(st));
    } catch (const NoMem &) {
        return fail(SDFHIP_ERR_NOMEM, "scene_place: out of device memory (the source is untouched)");
    }
    float kernel_ms = 0.0f;
    HIP_TRY(hipEventElapsedTime(&kernel_ms, cs.ev[0], cs.ev[1]));

    float scene_ms = 0.0f;
    if (const int rc = finish_tree("scene_place", device, dS, dV, n_out, (int)depth_out, out, host_out, &scene_ms)) return rc;
    if (stats) {
        stats->nodes_in = Q.n_nodes; stats->nodes_out = n_out; stats->depth_out = depth_out; stats->levels = depth_out + 1;
        stats->samples = samples;
        stats->kernel_ms = kernel_ms; stats->scene_ms = scene_ms;
        stats->total_ms = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
        stats->pad_ = 0;
    }
    return SDFHIP_OK;
}
SDFHIP_ABI_CATCH(sdfhip_scene_place)
