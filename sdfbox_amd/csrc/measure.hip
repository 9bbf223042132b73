// libsdfhip.so, the measure: sdfhip_scene_measure -- volume, area, first and second moments, tight bounds and cell counts of the solid
// a resident scene describes (kernels: measure_kernels.h).
//
// Replaces: nothing in the reference's code.  Its tree only ever becomes pixels; a scene carved, combined or pruned here could be
// compared with another only by pixels and node counts, and a placement had no bounds or centroid to fit from.
//
// Per call, on the scene's own stream: k_measure_cells (one partial of 17 doubles per 1024 nodes), then k_measure_fold until one
// partial is left -- the result record, which the host reads in one copy with the counts beside it.  The temporaries (136 bytes per
// 1024 nodes, 1/1024 of that again for the folds' other side, a 256-byte header) are one block per device, kept between calls as the
// mesh keeps its own; the call is synchronous, so the block is idle again when it returns.
#include "measure_kernels.h"
#include "host_support.h"
#include "abi_guard.h"

#include <chrono>
#include <cstring>
#include <limits>
#include <mutex>

using namespace sdfhip;

static_assert(sizeof(sdfhip_measure_options) == 8 && sizeof(sdfhip_measure) == 216, "the measure records of include/sdfhip.h");
static_assert(sizeof(MeasureHeader) <= 256, "the header's room in front of the partials");

namespace {

constexpr int MAX_DEVICES = 64;
constexpr size_t HEAD_BYTES = 256;                  // the result record, in front of the partials
constexpr size_t KEEP_BYTES = (size_t)16 << 20;     // a block up to this size stays allocated between calls
constexpr size_t PARTIAL_BYTES = MEASURE_DOUBLES * sizeof(double);

struct Temp {
    std::mutex lock;
    char *buf = nullptr;
    size_t cap = 0;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
};
Temp g_temp[MAX_DEVICES];

int check_options(const char *what, const sdfhip_measure_options *opt, int32_t *level)
{
    *level = -1;
    if (!opt) return SDFHIP_OK;
    if (const int rc = check_options_size(what, opt, sizeof(sdfhip_measure_options), "sdfhip_measure_options_default sets the size")) return rc;
    if (opt->level < -1 || opt->level > MESH_MAX_DEPTH)
        return fail(SDFHIP_ERR_ARG, "%s: level %d is neither -1 nor 0..%d", what, opt->level, MESH_MAX_DEPTH);
    *level = opt->level;
    return SDFHIP_OK;
}

uint32_t blocks_of(uint32_t n, uint32_t per) { return (uint32_t)(((uint64_t)n + per - 1) / per); }

// Under the device's Temp lock and the handle's lock, on its device: the kernels on the scene's stream, the header on the host when
// this returns
int measure_pass(sdfhip_scene *s, const char *what, Temp &t, AllocFault &fault, int32_t level, MeasureHeader *h, float *ms)
{
    if (!t.ev0) HIP_TRY(hipEventCreate(&t.ev0));     // each on its own: one may fail and the next call tries again
    if (!t.ev1) HIP_TRY(hipEventCreate(&t.ev1));
    const hipStream_t st = s->stream;
    const uint32_t nchunk = blocks_of(s->n, MEASURE_CHUNK), nfold = blocks_of(nchunk, MEASURE_FOLD);
    const size_t need = HEAD_BYTES + ((size_t)nchunk + nfold) * PARTIAL_BYTES;
    if (fault.next() || grow_buffer(t.buf, t.cap, need) != hipSuccess) {
        (void)hipGetLastError();
        return fail(SDFHIP_ERR_NOMEM, "%s: out of device memory for %zu bytes of partial sums", what, need);
    }
    MeasureHeader *head = reinterpret_cast<MeasureHeader *>(t.buf);
    double *a = reinterpret_cast<double *>(t.buf + HEAD_BYTES), *b = a + (size_t)nchunk * MEASURE_DOUBLES;
    HIP_TRY(hipMemsetAsync(t.buf, 0, HEAD_BYTES, st));
    HIP_TRY(hipEventRecord(t.ev0, st));
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
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(t.ev1, st));
    HIP_TRY(hipMemcpyAsync(h, t.buf, sizeof(MeasureHeader), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    HIP_TRY(hipEventElapsedTime(ms, t.ev0, t.ev1));
    return SDFHIP_OK;
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
    if (!scene->stack_ok || scene->depth > (uint32_t)MESH_MAX_DEPTH)
        return fail(SDFHIP_ERR_BAD_TREE, "%s: the tree is not consistent (or deeper than %d levels): no measure", what, MESH_MAX_DEPTH);
    if (scene->device < 0 || scene->device >= MAX_DEVICES) return fail(SDFHIP_ERR_ARG, "%s: device %d", what, scene->device);
    Temp &t = g_temp[scene->device];
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
    release_buffer(t.buf, t.cap, KEEP_BYTES);
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
