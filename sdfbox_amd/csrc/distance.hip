// libsdfhip.so, exact distance: sdfhip_scene_distance / _distance_device -- how far n points are from the surface a resident scene
// describes, at any range -- and sdfhip_scene_offset -- the scene grown, shrunk or hollowed into a new tree, the result a new handle
// (kernels: distance_kernels.h).
//
// Replaces: nothing in the reference's code; its field is only ever read as stored, a distance in a thin band round the surface.
//
// The rule, pinned (include/sdfhip.h; fp32, each operation rounded on its own in the order written):
//   surface   sdfhip_scene_mesh's triangles for the level          d2(p)   the minimum of tri_dist2 over them (+inf: none)
//   sign(p)   sdfhip_scene_sample's distance at clamp(p) < 0       dist    sign * sqrtf(d2)
//   value     GROW dist - delta; SHELL fabsf(dist) - thickness * 0.5f      tree    sdfhip_scene_place's construct rule and node order
//
// Per call: the "surface below" bitmap (k_dist_mark: 4 bytes per 32 nodes, zeroed and rebuilt every time -- nothing is kept on the
// handle), then either k_dist_query, or the placement's level loop (build_levels below) with k_offset_level as its first pass, the
// shared bitmap scan and k_offset_emit.  The _device form launches on the caller's stream and returns; its bitmap is one block per device kept here, and a
// call waits for the query that last read it -- through the library's own event, never the caller's stream -- before it writes it
// again (as mesh.hip's chunk totals).  The host form and the offset run on a stream of their own with memory of their own.
#include "distance_kernels.h"
#include "host_support.h"
#include "abi_guard.h"

#include <algorithm>
#include <chrono>
#include <cmath>
#include <mutex>
#include <type_traits>

using namespace sdfhip;

static_assert(sizeof(sdfhip_clearance) == 32 && sizeof(sdfhip_offset_options) == 20 && sizeof(sdfhip_offset_stats) == 48,
              "the distance records of include/sdfhip.h");
static_assert(SDFHIP_OFFSET_GROW == OFFSET_GROW && SDFHIP_OFFSET_SHELL == OFFSET_SHELL && SDFHIP_QUERY_HIT == QUERY_HIT &&
              SDFHIP_QUERY_INVALID == QUERY_INVALID, "distance_kernels.h restates the header's codes");

namespace {

constexpr int MAX_DEVICES = 64;
constexpr uint32_t DIST_MAX_WORKGROUPS = 2048;      // every pass strides with at most this many workgroups of four waves: 8 waves on each of the 1024 SIMDs

// The sign's look-up takes the march's cursor, as the placement's value does: the grid wherever the handle has a full-depth one,
// else the walk along the links.  Both give the same bytes.
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

// what a call reads of the handle, under its lock
struct Source {
    QueryScene Q;
    Form form;
    uint32_t depth;
    int device, stack_ok;
};
Source read_source(sdfhip_scene *s)
{
    std::lock_guard<std::mutex> lk(s->lock);
    return Source{scene_of(s), form_of(s), s->depth, s->device, s->stack_ok};
}
// sdfhip_scene_mesh's refusal: the surface is its triangles
int check_source(const char *what, const Source &src)
{
    if (!src.stack_ok || src.depth > (uint32_t)MESH_MAX_DEPTH)
        return fail(SDFHIP_ERR_BAD_TREE, "%s: the tree is not consistent (or deeper than %d levels): it has no mesh, so no surface to measure from", what,
                    MESH_MAX_DEPTH);
    if (src.device < 0 || src.device >= MAX_DEVICES) return fail(SDFHIP_ERR_ARG, "%s: device %d", what, src.device);
    return SDFHIP_OK;
}
int check_level(const char *what, int32_t level)
{
    if (level < -1 || level > MESH_MAX_DEPTH) return fail(SDFHIP_ERR_ARG, "%s: level %d is neither -1 nor 0..%d", what, level, MESH_MAX_DEPTH);
    return SDFHIP_OK;
}

size_t bitmap_words(uint32_t n) { return ((size_t)n + 31) / 32 + 1; }     // (+ 1: sibling_bits reads one word past a block's first)

// (a) on `st`: the bitmap zeroed and marked
int launch_mark(const Source &src, int32_t level, uint32_t *below, hipStream_t st)
{
    HIP_TRY(hipMemsetAsync(below, 0, bitmap_words(src.Q.n_nodes) * sizeof(uint32_t), st));
    hipLaunchKernelGGL(k_dist_mark, grid_stride_blocks(src.Q.n_nodes, DIST_MAX_WORKGROUPS), dim3(DIST_THREADS), 0, st, src.Q.nodes, src.Q.n_nodes, (int)level, below);
    HIP_TRY(hipGetLastError());
    return SDFHIP_OK;
}

int launch_query(const Source &src, const DistScene &D, const float *d_xyz, uint32_t n, sdfhip_clearance *d_out, hipStream_t st)
{
    const dim3 grid = grid_stride_blocks(n, DIST_MAX_WORKGROUPS), wg(DIST_THREADS);
    uint4 *out = reinterpret_cast<uint4 *>(d_out);
    switch (src.form) {
    case FORM_GRID: hipLaunchKernelGGL((k_dist_query<CursorFT<false, false>>), grid, wg, 0, st, src.Q, D, d_xyz, n, out); break;
    case FORM_SPLIT: hipLaunchKernelGGL((k_dist_query<CursorFT<false, true>>), grid, wg, 0, st, src.Q, D, d_xyz, n, out); break;
    default: hipLaunchKernelGGL((k_dist_query<CursorG>), grid, wg, 0, st, src.Q, D, d_xyz, n, out); break;
    }
    HIP_TRY(hipGetLastError());
    return SDFHIP_OK;
}

void launch_level(const Source &src, const DistScene &D, int mode, float amount, const OffsetBlock *blocks, uint32_t nblocks, uint32_t nchild,
                  float S, int may_split, uint2 *V, uint8_t *split, unsigned long long *visited, hipStream_t st)
{
    const dim3 grid = grid_stride_blocks(64ull * nblocks, DIST_MAX_WORKGROUPS), wg(OFFSET_THREADS);
    switch (src.form) {
    case FORM_GRID: hipLaunchKernelGGL((k_offset_level<CursorFT<false, false>>), grid, wg, 0, st, src.Q, D, mode, amount, blocks, nblocks, nchild, S, may_split, V, split, visited); break;
    case FORM_SPLIT: hipLaunchKernelGGL((k_offset_level<CursorFT<false, true>>), grid, wg, 0, st, src.Q, D, mode, amount, blocks, nblocks, nchild, S, may_split, V, split, visited); break;
    default: hipLaunchKernelGGL((k_offset_level<CursorG>), grid, wg, 0, st, src.Q, D, mode, amount, blocks, nblocks, nchild, S, may_split, V, split, visited); break;
    }
}

// The _device form's bitmap: one block per device, busy until the query that reads it has run.  It stays allocated for the life of
// the process, as large as the largest scene queried so (4 bytes per 32 nodes: 3.5 MB for 28 M nodes): the query that reads it is
// still in flight when the call returns, so there is no point in the call at which it could be given back.
struct Temp {
    std::mutex lock;
    uint32_t *buf = nullptr;
    size_t cap = 0;                                 // bytes
    hipEvent_t busy = nullptr;
    bool pending = false;
};
Temp g_temp[MAX_DEVICES];

struct LevelBuild {
    int2 *dS = nullptr;            // the result's links and bytes, in `bufs`
    uint2 *dV = nullptr;
    uint32_t n_out = 1, depth_out = 0;
    uint64_t points = 0;           // 9 for the root and 35 for every block of eight siblings
};

// The level loop, as place.hip runs it for the placement (a sibling: that translation unit stays as it was).
// what: the entry point's name for the messages.  nodes_in: the source's size, which the arrays start from.  launch_level(blocks,
// nblocks, nchild, S, may_split, V, split): launches the level's first pass on `st`.  Throws NoMem (DeviceBuffers).  The last
// level may still be in flight on `st` when it returns: the caller waits.
template <class LaunchLevel>
int build_levels(const char *what, DeviceBuffers &bufs, hipStream_t st, uint32_t nodes_in, int depth, LaunchLevel launch_level, LevelBuild &R)
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
    OffsetBlock *cur = nullptr, *next = nullptr;
    uint32_t *split = nullptr, *pre = nullptr, *chunk = nullptr;
    size_t cur_cap = 0, next_cap = 0, split_cap = 0, pre_cap = 0, chunk_cap = 0;
    if (const int rc = room(cur, cur_cap, cap / 8 + 1)) return rc;
    HIP_TRY(hipMemsetAsync(cur, 0, sizeof(OffsetBlock), st));                 // the root's block: the cell at the origin
    HIP_TRY(hipMemsetAsync(R.dS, 0xFF, sizeof(int2), st));                   // the root: {-1, -1}

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
        R.points += nchild == 1 ? 9u : (uint64_t)OFFSET_POINTS * nblocks;
        if (!may_split) break;
        hipLaunchKernelGGL(k_rank_scan_words<OffsetSplitWords>, dim3(nchunk), dim3(256), 0, st, OffsetSplitWords{ split, n }, m, pre, chunk);
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
        hipLaunchKernelGGL(k_offset_emit, grid_stride_blocks(8ull * n, DIST_MAX_WORKGROUPS), dim3(256), 0, st, cur, n, nchild, first, split, pre,
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

// what the header refuses of the options, before any device call
int check_offset_options(const sdfhip_offset_options *opt)
{
    if (const int rc = check_options_size("scene_offset", opt, sizeof(sdfhip_offset_options), "size = sizeof(sdfhip_offset_options)")) return rc;
    if (opt->mode != SDFHIP_OFFSET_GROW && opt->mode != SDFHIP_OFFSET_SHELL) return fail(SDFHIP_ERR_ARG, "scene_offset: unknown mode %d", opt->mode);
    if (!std::isfinite(opt->amount)) return fail(SDFHIP_ERR_ARG, "scene_offset: the amount must be finite");
    if (opt->mode == SDFHIP_OFFSET_SHELL && !(opt->amount > 0.0f))
        return fail(SDFHIP_ERR_ARG, "scene_offset: a shell's thickness %g is not above 0", (double)opt->amount);
    if (opt->depth < -1 || opt->depth > TREE_MAX_DEPTH)
        return fail(SDFHIP_ERR_ARG, "scene_offset: depth %d is neither -1 nor 0..%d", opt->depth, TREE_MAX_DEPTH);
    return check_level("scene_offset", opt->level);
}

}  // namespace

extern "C" int sdfhip_scene_distance_device(sdfhip_scene *scene, const float *d_xyz, uint32_t n, int32_t level, sdfhip_clearance *d_out,
                                            void *stream)
try {
    const char *what = "scene_distance_device";
    if (!scene) return fail(SDFHIP_ERR_ARG, "%s: null scene", what);
    if (const int rc = check_level(what, level)) return rc;
    if (n && (!d_xyz || !d_out)) return fail(SDFHIP_ERR_ARG, "%s: null argument", what);
    const Source src = read_source(scene);
    if (const int rc = check_source(what, src)) return rc;
    if (n == 0) return SDFHIP_OK;
    Temp &t = g_temp[src.device];
    std::lock_guard<std::mutex> hold(t.lock);
    DeviceGuard g(src.device);
    if (!g.ok) return (void)hipGetLastError(), fail(SDFHIP_ERR_DEVICE, "%s: hipSetDevice(%d) failed", what, src.device);
    const hipStream_t st = (hipStream_t)stream;
    if (!t.busy) HIP_TRY(hipEventCreateWithFlags(&t.busy, hipEventDisableTiming));
    if (t.pending) { HIP_TRY(hipEventSynchronize(t.busy)); t.pending = false; }
    const size_t need = bitmap_words(src.Q.n_nodes) * sizeof(uint32_t);
    if (grow_buffer(t.buf, t.cap, need) != hipSuccess) {
        (void)hipGetLastError();
        return fail(SDFHIP_ERR_NOMEM, "%s: out of device memory for %zu bytes of bitmap", what, need);
    }
    int rc = launch_mark(src, level, t.buf, st);
    if (rc == SDFHIP_OK) {
        t.pending = true;                           // (whatever the launch says: the wait is harmless)
        rc = launch_query(src, DistScene{src.Q.nodes, src.Q.n_nodes, t.buf, level}, d_xyz, n, d_out, st);
        HIP_TRY(hipEventRecord(t.busy, st));
    }
    return rc;
}
SDFHIP_ABI_CATCH(sdfhip_scene_distance_device)

extern "C" int sdfhip_scene_distance(sdfhip_scene *scene, const float *xyz, uint32_t n, int32_t level, sdfhip_clearance *out)
try {
    const char *what = "scene_distance";
    if (!scene) return fail(SDFHIP_ERR_ARG, "%s: null scene", what);
    if (const int rc = check_level(what, level)) return rc;
    if (n && (!xyz || !out)) return fail(SDFHIP_ERR_ARG, "%s: null argument", what);
    const Source src = read_source(scene);
    if (const int rc = check_source(what, src)) return rc;
    if (n == 0) return SDFHIP_OK;
    DeviceGuard g(src.device);
    if (!g.ok) return (void)hipGetLastError(), fail(SDFHIP_ERR_DEVICE, "%s: hipSetDevice(%d) failed", what, src.device);
    DeviceBuffers bufs("SDFHIP_DISTANCE_FAIL_ALLOC");
    CallStream<1> cs;                      // (after `bufs`: drained before the buffers are freed)
    if (const int rc = cs.open("")) return rc;
    const hipStream_t st = cs.st;
    try {
        float *d_xyz = bufs.get<float>(3 * (size_t)n);
        sdfhip_clearance *d_out = bufs.get<sdfhip_clearance>(n);
        uint32_t *below = bufs.get<uint32_t>(bitmap_words(src.Q.n_nodes));
        HIP_TRY(hipMemcpyAsync(d_xyz, xyz, (size_t)n * 12, hipMemcpyHostToDevice, st));
        if (const int rc = launch_mark(src, level, below, st)) return rc;
        if (const int rc = launch_query(src, DistScene{src.Q.nodes, src.Q.n_nodes, below, level}, d_xyz, n, d_out, st)) return rc;
        HIP_TRY(hipMemcpyAsync(out, d_out, (size_t)n * sizeof(sdfhip_clearance), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
    } catch (const NoMem &) {
        return fail(SDFHIP_ERR_NOMEM, "%s: out of device memory (the scene is untouched)", what);
    }
    return SDFHIP_OK;
}
SDFHIP_ABI_CATCH(sdfhip_scene_distance)

extern "C" int sdfhip_scene_offset(sdfhip_scene *scene, const sdfhip_offset_options *opt, sdfhip_scene **out, sdfhip_octdata *host_out,
                                   sdfhip_offset_stats *stats)
try {
    const char *what = "scene_offset";
    const auto t0 = std::chrono::steady_clock::now();
    if (out) *out = nullptr;
    if (!opt) return fail(SDFHIP_ERR_ARG, "%s: null options", what);
    if (!out && !host_out) return fail(SDFHIP_ERR_ARG, "%s: both outputs are null", what);
    if (const int rc = check_offset_options(opt)) return rc;
    if (!scene) return fail(SDFHIP_ERR_ARG, "%s: null scene", what);
    // What the call uses of the handle is read under the handle's lock, which is released before any work is issued, as
    // sdfhip_scene_place does: the records and the grids are only ever read.
    const Source src = read_source(scene);
    if (const int rc = check_source(what, src)) return rc;
    const int depth = opt->depth < 0 ? (int)src.depth : opt->depth;
    const int mode = opt->mode;
    const float amount = mode == SDFHIP_OFFSET_SHELL ? opt->amount * 0.5f : opt->amount;

    DeviceGuard g(src.device);
    if (!g.ok) return (void)hipGetLastError(), fail(SDFHIP_ERR_DEVICE, "%s: hipSetDevice(%d) failed", what, src.device);
    DeviceBuffers bufs("SDFHIP_OFFSET_FAIL_ALLOC");
    CallStream<2> cs;                       // (after `bufs`: drained before the buffers are freed)
    if (const int rc = cs.open("")) return rc;
    const hipStream_t st = cs.st;

    LevelBuild R;
    unsigned long long visited = 0;
    try {
        uint32_t *below = bufs.get<uint32_t>(bitmap_words(src.Q.n_nodes));
        unsigned long long *d_visited = bufs.get<unsigned long long>(1);
        HIP_TRY(hipMemsetAsync(d_visited, 0, sizeof *d_visited, st));
        HIP_TRY(hipEventRecord(cs.ev[0], st));
        if (const int rc = launch_mark(src, opt->level, below, st)) return rc;
        const DistScene D{src.Q.nodes, src.Q.n_nodes, below, opt->level};
        const auto level = [&](const OffsetBlock *blocks, uint32_t nblocks, uint32_t nchild, float S, int may_split, uint2 *V, uint8_t *split) {
            launch_level(src, D, mode, amount, blocks, nblocks, nchild, S, may_split, V, split, d_visited, st);
        };
        if (const int rc = build_levels(what, bufs, st, src.Q.n_nodes, depth, level, R)) return rc;
        HIP_TRY(hipEventRecord(cs.ev[1], st));
        HIP_TRY(hipMemcpyAsync(&visited, d_visited, sizeof visited, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
    } catch (const NoMem &) {
        return fail(SDFHIP_ERR_NOMEM, "%s: out of device memory (the source is untouched)", what);
    }
    float kernel_ms = 0.0f;
    HIP_TRY(hipEventElapsedTime(&kernel_ms, cs.ev[0], cs.ev[1]));

    float scene_ms = 0.0f;
    if (const int rc = finish_tree(what, src.device, R.dS, R.dV, R.n_out, (int)R.depth_out, out, host_out, &scene_ms)) return rc;
    if (stats) {
        stats->nodes_in = src.Q.n_nodes; stats->nodes_out = R.n_out; stats->depth_out = R.depth_out; stats->levels = R.depth_out + 1;
        stats->points = R.points; stats->visited = visited;
        stats->kernel_ms = kernel_ms; stats->scene_ms = scene_ms;
        stats->total_ms = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
        stats->pad_ = 0;
    }
    return SDFHIP_OK;
}
SDFHIP_ABI_CATCH(sdfhip_scene_offset)
