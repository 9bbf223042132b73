// The host side that every lattice builder shares: place.hip (sdfhip_scene_place), compose.hip (sdfhip_scene_compose), volume.hip
// (sdfhip_volume_build), distance.hip (sdfhip_scene_offset) and blend.hip (sdfhip_scene_blend).  What a call reads of a handle, the cursor a look-up takes, and the level loop (build_levels: a template on
// the launch of a level's first pass, so each caller brings its own kernel round level_kernels.h's level_body; the shared bitmap
// scan and k_level_emit do the rest).  Everything here is inline or a template.  What only the builders on the exact distance need
// -- their refusals, the "surface below" bitmap -- is distance_host.h's.
#pragma once
#include "level_kernels.h"
#include "query_kernels.h"   // QueryScene; raymarch_device.h: the cursors
#include "host_support.h"

#include <algorithm>
#include <cmath>
#include <mutex>
#include <type_traits>

namespace sdfhip {
namespace levels {

constexpr uint32_t LEVEL_MAX_WORKGROUPS = 2048;     // every pass strides with at most this many workgroups of four waves: 8 waves on each of the 1024 SIMDs

// Which cursor a look-up takes: no cell index is wanted, so the choice is the march's (query.hip's form_of for a march): the grid
// wherever the handle has a full-depth one -- dense, or coarse level + fine blocks -- else the shader's walk along the links.  All
// give the same bytes.
enum Form { FORM_GENERIC = 0, FORM_GRID = 1, FORM_SPLIT = 2 };
inline Form form_of(const sdfhip_scene *s)
{
    if (!scene_has_full_depth_grid(s)) return FORM_GENERIC;
    return s->fine_bits ? FORM_SPLIT : FORM_GRID;
}
inline QueryScene scene_of(const sdfhip_scene *s)
{
    return QueryScene{s->nodes, s->n, s->d_top, s->d_fine, s->top_level, s->fine_bits};
}

// f(CursorOf<C>{}) with C the cursor of the form: a kernel that is a template on the cursor is launched as
// k<typename decltype(c)::type>
template <class CursorT> struct CursorOf { using type = CursorT; };
template <class F> void with_cursor(Form form, F f)
{
    switch (form) {
    case FORM_GRID: f(CursorOf<CursorFT<false, false>>{}); break;
    case FORM_SPLIT: f(CursorOf<CursorFT<false, true>>{}); break;
    default: f(CursorOf<CursorG>{}); break;
    }
}

// What a call reads of the handle, under its lock, which is released before any work is issued: the records and the grids are fixed
// at upload and only ever read, so renders, queries and meshes of the source on other threads do not wait for the builder.
struct Source {
    QueryScene Q;
    Form form;
    uint32_t depth;
    int device, stack_ok;
};
inline Source read_source(sdfhip_scene *s)
{
    std::lock_guard<std::mutex> lk(s->lock);
    return Source{scene_of(s), form_of(s), s->depth, s->device, s->stack_ok};
}

// What sdfhip_scene_place and sdfhip_scene_compose refuse of a similarity p = s R x + t, before any device call: a non-finite field,
// s <= 0, a rotation with max |(R R^T - I)_ij| > 1e-4 (in double; the bound defines the interface, mirrors pass).  what: the
// message's prefix -- the entry point's name, and for an instance its index.
inline int check_similarity(const char *what, const float (*rotation)[3], float scale, const float *translation)
{
    bool finite = std::isfinite(scale);
    for (int i = 0; i < 3; i++) {
        finite = finite && std::isfinite(translation[i]);
        for (int j = 0; j < 3; j++) finite = finite && std::isfinite(rotation[i][j]);
    }
    if (!finite) return fail(SDFHIP_ERR_ARG, "%s: rotation, scale and translation must be finite", what);
    if (!(scale > 0.0f)) return fail(SDFHIP_ERR_ARG, "%s: scale %g is not above 0", what, (double)scale);
    double worst = 0.0;
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) {
            double dot = 0.0;
            for (int k = 0; k < 3; k++) dot += (double)rotation[i][k] * (double)rotation[j][k];
            worst = std::max(worst, std::fabs(dot - (i == j ? 1.0 : 0.0)));
        }
    if (worst > 1e-4) return fail(SDFHIP_ERR_ARG, "%s: the rotation is not orthogonal (max |R R^T - I| = %g, the bound 1e-4)", what, worst);
    return SDFHIP_OK;
}

struct LevelBuild {
    int2 *dS = nullptr;            // the result's links and bytes, in `bufs`
    uint2 *dV = nullptr;
    uint32_t n_out = 1, depth_out = 0;
    uint64_t points = 0;           // 9 for the root and 35 for every block of eight siblings
};

// The level loop.  what: the entry point's name for the messages.  nodes_in: the source's size, which the arrays start from.
// launch_level(blocks, nblocks, nchild, S, may_split, V, split): launches the level's first pass on `st`.  started: if given,
// recorded on `st` once the first arrays are allocated and the root is queued, before the first level (the placement's kernel_ms
// starts there: the allocations' host time is not part of it).  Allocates, in this order, dS, dV, the blocks, split, pre, chunk, then
// the next level's blocks and whatever grows.  Throws NoMem (DeviceBuffers).  The last level may still be in flight on `st` when it
// returns: the caller waits.
template <class LaunchLevel>
int build_levels(const char *what, DeviceBuffers &bufs, hipStream_t st, uint32_t nodes_in, int depth, LaunchLevel launch_level, LevelBuild &R,
                 hipEvent_t started = nullptr)
{
    // The result's arrays start with room for a tree of the source's size and double when a level does not fit: the levels
    // already written are copied over.  The per-level buffers are sized for what the arrays can hold -- a level is part of the
    // result -- and follow when those grow.  Every buffer is replaced only while the stream is idle.
    size_t cap = std::min<size_t>(std::max<size_t>((size_t)nodes_in + nodes_in / 2, 4096), 0x7FFFFFFFull);
    R.dS = bufs.get<int2>(cap);
    R.dV = bufs.get<uint2>(cap);
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
    LevelBlock *cur = nullptr, *next = nullptr;
    uint32_t *split = nullptr, *pre = nullptr, *chunk = nullptr;
    size_t cur_cap = 0, next_cap = 0, split_cap = 0, pre_cap = 0, chunk_cap = 0;
    if (const int rc = room(cur, cur_cap, cap / 8 + 1)) return rc;
    HIP_TRY(hipMemsetAsync(cur, 0, sizeof(LevelBlock), st));                  // the root's block: the cell at the origin
    HIP_TRY(hipMemsetAsync(R.dS, 0xFF, sizeof(int2), st));                   // the root: {-1, -1}
    if (started) HIP_TRY(hipEventRecord(started, st));

    uint32_t first = 0, n = 1, nblocks = 1, nchild = 1;
    for (int d = 0;; d++) {
        R.depth_out = (uint32_t)d;
        const float S = ldexpf(1.0f, -d);
        const int may_split = d < depth ? 1 : 0;
        const uint32_t m = (n + 31) / 32, nchunk = (m + 1023) / 1024;
        if (const int rc = room(split, split_cap, words_of(cap))) return rc;
        if (const int rc = room(pre, pre_cap, words_of(cap))) return rc;
        if (const int rc = room(chunk, chunk_cap, (words_of(cap) + 1023) / 1024 + 1)) return rc;        // (+ 1: the level's splits)
        idle = false;
        launch_level(cur, nblocks, nchild, S, may_split, R.dV + first, reinterpret_cast<uint8_t *>(split));
        HIP_TRY(hipGetLastError());
        R.points += nchild == 1 ? 9u : (uint64_t)LEVEL_POINTS * nblocks;
        if (!may_split) break;
        hipLaunchKernelGGL(k_rank_scan_words<LevelSplitWords>, dim3(nchunk), dim3(256), 0, st, LevelSplitWords{ split, n }, m, pre, chunk);
        hipLaunchKernelGGL(k_rank_scan_chunks<true>, dim3(1), dim3(1024), 0, st, chunk, nchunk);
        HIP_TRY(hipGetLastError());
        uint32_t n_split = 0;
        HIP_TRY(hipMemcpyAsync(&n_split, chunk + nchunk, sizeof n_split, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        idle = true;
        if (!n_split) break;
        if (n_split > n) return fail(SDFHIP_ERR_DEVICE, "%s: %u splits among %u nodes", what, n_split, n);
        const uint64_t total = (uint64_t)R.n_out + 8ull * n_split;
        if (total > 0x7FFFFFFFull) return fail(SDFHIP_ERR_ARG, "%s: the result would have more than 2^31 - 1 nodes", what);
        if (total > cap) {
            const size_t new_cap = (size_t)std::min<uint64_t>(std::max<uint64_t>(total, 2ull * cap), 0x7FFFFFFFull);
            if (const int rc = grown(R.dS, new_cap, R.n_out)) return rc;
            if (const int rc = grown(R.dV, new_cap, R.n_out)) return rc;
            cap = new_cap;
        }
        if (const int rc = room(next, next_cap, cap / 8 + 1)) return rc;
        idle = false;
        hipLaunchKernelGGL(k_level_emit, grid_stride_blocks(8ull * n, LEVEL_MAX_WORKGROUPS), dim3(256), 0, st, cur, n, nchild, first, split, pre,
                           chunk, R.dS, (uint32_t)cap, next, n_split);
        HIP_TRY(hipGetLastError());
        std::swap(cur, next);
        std::swap(cur_cap, next_cap);
        first += n;
        n = 8u * n_split; nblocks = n_split; nchild = 8;
        R.n_out = (uint32_t)total;
    }
    return SDFHIP_OK;
}

}  // namespace levels
}  // namespace sdfhip
