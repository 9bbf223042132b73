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
// handle), then either k_dist_query, or the shared level loop (level_build.h's build_levels) with k_offset_level as its first pass.
// The _device form launches on the caller's stream and returns; its bitmap is one block per device kept here, and a
// call waits for the query that last read it -- through the library's own event, never the caller's stream -- before it writes it
// again (as mesh.hip's chunk totals).  The host form and the offset run on a stream of their own with memory of their own.
#include "distance_host.h"    // distance_kernels.h; check_source, launch_mark; level_build.h: Source, with_cursor, build_levels
#include "abi_guard.h"

#include <algorithm>
#include <chrono>
#include <cmath>
#include <mutex>
#include <type_traits>

using namespace sdfhip;
using namespace sdfhip::levels;

static_assert(sizeof(sdfhip_clearance) == 32 && sizeof(sdfhip_offset_options) == 20 && sizeof(sdfhip_offset_stats) == 48,
              "the distance records of include/sdfhip.h");
static_assert(SDFHIP_OFFSET_GROW == OFFSET_GROW && SDFHIP_OFFSET_SHELL == OFFSET_SHELL && SDFHIP_QUERY_HIT == QUERY_HIT &&
              SDFHIP_QUERY_INVALID == QUERY_INVALID, "distance_kernels.h restates the header's codes");

namespace {

int launch_query(const Source &src, const DistScene &D, const float *d_xyz, uint32_t n, sdfhip_clearance *d_out, hipStream_t st)
{
    const dim3 grid = grid_stride_blocks(n, LEVEL_MAX_WORKGROUPS), wg(DIST_THREADS);
    uint4 *out = reinterpret_cast<uint4 *>(d_out);
    with_cursor(src.form, [&](auto c) { hipLaunchKernelGGL((k_dist_query<typename decltype(c)::type>), grid, wg, 0, st, src.Q, D, d_xyz, n, out); });
    HIP_TRY(hipGetLastError());
    return SDFHIP_OK;
}

void launch_level(const Source &src, const DistScene &D, int mode, float amount, const LevelBlock *blocks, uint32_t nblocks, uint32_t nchild,
                  float S, int may_split, uint2 *V, uint8_t *split, unsigned long long *visited, hipStream_t st)
{
    const dim3 grid = grid_stride_blocks(64ull * nblocks, LEVEL_MAX_WORKGROUPS), wg(LEVEL_THREADS);
    with_cursor(src.form, [&](auto c) {
        hipLaunchKernelGGL((k_offset_level<typename decltype(c)::type>), grid, wg, 0, st, src.Q, D, mode, amount, blocks, nblocks, nchild, S, may_split, V, split, visited);
    });
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
    CallFrame<1> call(what, src.device, "SDFHIP_DISTANCE_FAIL_ALLOC");
    return call.run("the scene is untouched", [&](hipStream_t st) -> int {
        float *d_xyz = call.bufs.get<float>(3 * (size_t)n);
        sdfhip_clearance *d_out = call.bufs.get<sdfhip_clearance>(n);
        uint32_t *below = call.bufs.get<uint32_t>(bitmap_words(src.Q.n_nodes));
        HIP_TRY(hipMemcpyAsync(d_xyz, xyz, (size_t)n * 12, hipMemcpyHostToDevice, st));
        if (const int rc = launch_mark(src, level, below, st)) return rc;
        if (const int rc = launch_query(src, DistScene{src.Q.nodes, src.Q.n_nodes, below, level}, d_xyz, n, d_out, st)) return rc;
        HIP_TRY(hipMemcpyAsync(out, d_out, (size_t)n * sizeof(sdfhip_clearance), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        return SDFHIP_OK;
    });
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

    CallFrame<2> call(what, src.device, "SDFHIP_OFFSET_FAIL_ALLOC", t0);
    LevelBuild R;
    unsigned long long visited = 0;
    if (const int rc = call.run("the source is untouched", [&](hipStream_t st) -> int {
        uint32_t *below = call.bufs.get<uint32_t>(bitmap_words(src.Q.n_nodes));
        unsigned long long *d_visited = call.bufs.get<unsigned long long>(1);
        HIP_TRY(hipMemsetAsync(d_visited, 0, sizeof *d_visited, st));
        HIP_TRY(hipEventRecord(call.cs.ev[0], st));
        if (const int rc = launch_mark(src, opt->level, below, st)) return rc;
        const DistScene D{src.Q.nodes, src.Q.n_nodes, below, opt->level};
        const auto level = [&](const LevelBlock *blocks, uint32_t nblocks, uint32_t nchild, float S, int may_split, uint2 *V, uint8_t *split) {
            launch_level(src, D, mode, amount, blocks, nblocks, nchild, S, may_split, V, split, d_visited, st);
        };
        if (const int rc = build_levels(what, call.bufs, st, src.Q.n_nodes, depth, level, R)) return rc;
        HIP_TRY(hipEventRecord(call.cs.ev[1], st));
        HIP_TRY(hipMemcpyAsync(&visited, d_visited, sizeof visited, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        return SDFHIP_OK;
    })) return rc;

    float kernel_ms = 0.0f, scene_ms = 0.0f;
    if (const int rc = call.elapsed(&kernel_ms, 0, 1)) return rc;
    if (const int rc = call.finish(R.dS, R.dV, R.n_out, (int)R.depth_out, out, host_out, &scene_ms)) return rc;
    if (stats) {
        stats->nodes_in = src.Q.n_nodes; stats->nodes_out = R.n_out; stats->depth_out = R.depth_out; stats->levels = R.depth_out + 1;
        stats->points = R.points; stats->visited = visited;
        stats->kernel_ms = kernel_ms; stats->scene_ms = scene_ms;
        stats->total_ms = call.total_ms();
        stats->pad_ = 0;
    }
    return SDFHIP_OK;
}
SDFHIP_ABI_CATCH(sdfhip_scene_offset)
