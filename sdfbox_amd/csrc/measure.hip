// libsdfhip.so, the measure: sdfhip_scene_measure -- volume, area, first and second moments, tight bounds and cell counts of the solid
// a resident scene describes (kernels: measure_kernels.h).
//
// Replaces: nothing in the reference's code.  Its tree only ever becomes pixels; a scene carved, combined or pruned here could be
// compared with another only by pixels and node counts, and a placement had no bounds or centroid to fit from.
//
// Per call, on the scene's own stream: k_measure_cells (one partial of 17 doubles per 1024 nodes), then k_measure_fold until one
// partial is left -- the result record, which the host reads in one copy with the counts beside it.  The temporaries (136 bytes per
// 1024 nodes, 1/1024 of that again for the folds' other side, a 256-byte header) are one DeviceScratch per device (host_support.h),
// kept between calls as the mesh keeps its own; the call is synchronous, so the block is idle again when it returns.
#include "measure_kernels.h"
#include "host_support.h"
#include "abi_guard.h"

#include <chrono>
#include <cstring>
#include <limits>
#include <mutex>

using namespace sdfhip;

static_assert(sizeof(sdfhip_measure_options) == 8 && sizeof(sdfhip_measure) == 216, "the measure records of include/sdfhip.h");

namespace {

constexpr size_t PARTIAL_BYTES = MEASURE_DOUBLES * sizeof(double);

DeviceScratch g_temp[MAX_DEVICES];

int check_options(const char *what, const sdfhip_measure_options *opt, int32_t *level)
{
    *level = -1;
    if (!opt) return SDFHIP_OK;
    if (const int rc = check_options_size(what, opt, sizeof(sdfhip_measure_options), "sdfhip_measure_options_default sets the size")) return rc;
    if (const int rc = check_level(what, opt->level)) return rc;
    *level = opt->level;
    return SDFHIP_OK;
}

uint32_t blocks_of(uint32_t n, uint32_t per) { return (uint32_t)(((uint64_t)n + per - 1) / per); }

// Under the DeviceScratch's lock and the handle's lock, on its device: the kernels on the scene's stream, the header on the host when
// this returns
int measure_pass(sdfhip_scene *s, const char *what, DeviceScratch &t, AllocFault &fault, int32_t level, MeasureHeader *h, float *ms)
{
    const hipStream_t st = s->stream;
    const uint32_t nchunk = blocks_of(s->n, MEASURE_CHUNK), nfold = blocks_of(nchunk, MEASURE_FOLD);
    if (const int rc = t.begin(what, fault, HEAD_BYTES + ((size_t)nchunk + nfold) * PARTIAL_BYTES, "partial sums", st)) return rc;
    return t.count(st, [&] {
        MeasureHeader *head = t.head<MeasureHeader>();
        double *a = t.behind_head<double>(), *b = a + (size_t)nchunk * MEASURE_DOUBLES;
        hipLaunchKernelGGL(k_measure_cells, dim3(nchunk), dim3(MEASURE_THREADS), 0, st, s->nodes, s->n, level, a, head);
        // a holds m partials; the round that leaves one writes the header.  The other side needs ceil(m / 1024) <= nfold records, and
        // the side that was read is free again by then (one stream, in order).
        for (uint32_t m = nchunk;;) {
            const uint32_t left = blocks_of(m, MEASURE_FOLD);
            hipLaunchKernelGGL(k_measure_fold, dim3(left), dim3(MEASURE_FOLD), 0, st, a, m, left == 1 ? head->v : b);
            if (left == 1) break;
            std::swap(a, b);
            m = left;
        }
    }, h, ms);
}

}  // namespace

extern "C" void sdfhip_measure_options_default(sdfhip_measure_options *opt)
try {
    if (!opt) { (void)fail(SDFHIP_ERR_ARG, "measure_options_default: null argument"); return; }
    opt->size = (uint32_t)sizeof(sdfhip_measure_options);
    opt->level = -1;
}
SDFHIP_ABI_CATCH_VOID(sdfhip_measure_options_default)

extern "C" int sdfhip_scene_measure(sdfhip_scene *scene, const sdfhip_measure_options *opt, sdfhip_measure *out)
try {
    const char *what = "scene_measure";
    const auto t0 = std::chrono::steady_clock::now();
    if (!out) return fail(SDFHIP_ERR_ARG, "%s: null argument", what);
    memset(out, 0, sizeof *out);
    if (!scene) return fail(SDFHIP_ERR_ARG, "%s: null argument", what);
    int32_t level;
    if (const int rc = check_options(what, opt, &level)) return rc;
    if (const int rc = check_cell_scene(what, scene, "no measure")) return rc;
    DeviceScratch &t = g_temp[scene->device];
    AllocFault fault("SDFHIP_MEASURE_FAIL_ALLOC");  // laboratory library: fails the call's k-th allocation (0 = the first)
    std::lock_guard<std::mutex> hold(t.lock);
    DeviceGuard g(scene->device);
    if (!g.ok) return fail(SDFHIP_ERR_DEVICE, "%s: hipSetDevice(%d) failed", what, scene->device);
    MeasureHeader h;
    float kernel_ms = 0.0f;
    const int rc = [&]() -> int {
        std::lock_guard<std::mutex> lk(scene->lock);
        const int r = measure_pass(scene, what, t, fault, level, &h, &kernel_ms);
        if (r != SDFHIP_OK) (void)hipStreamSynchronize(scene->stream);          // nothing of this call is in flight when its block goes
        return r;
    }();
    t.release();
    if (rc != SDFHIP_OK) return rc;
    out->volume = h.v[0]; out->area = h.v[1];
    for (int k = 0; k < 3; k++) { out->moment1[k] = h.v[2 + k]; out->bounds_min[k] = h.v[11 + k]; out->bounds_max[k] = h.v[14 + k]; }
    for (int k = 0; k < 6; k++) out->moment2[k] = h.v[5 + k];
    out->nodes = scene->n; out->depth = scene->depth;
    out->cells_cut = h.cut; out->cells_inside = h.inside;
    for (int d = 0; d <= MESH_MAX_DEPTH; d++) { out->cells_at_depth[d] = h.at_depth[d]; out->cells += h.at_depth[d]; }
    out->kernel_ms = kernel_ms;
    out->total_ms = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
    return SDFHIP_OK;
}
SDFHIP_ABI_CATCH(sdfhip_scene_measure)
