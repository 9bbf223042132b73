// libsdfhip.so, cross-sections: sdfhip_scene_slice / sdfhip_scene_slice_device -- the contours of a resident scene in a stack of
// parallel planes, as directed segments (kernels: slice_kernels.h).
//
// Replaces: nothing that runs in the reference.  Its tree only ever becomes pixels; the outline of a solid in a plane, which a
// printer's slicer, a section view and a fit check start from, had to be picked out of sdfhip_scene_mesh's triangles on the host.
//
// Per call, as the mesh (mesh.hip): k_slice_count and the chunk scan on the call's stream, one host synchronisation for the record total
// (it sizes the output and is what the _device form always returns), then k_slice_emit.  The _device form leaves the emit in flight on
// the caller's stream; the host form runs on the scene's own stream, copies the records and the per-layer counts out and waits.  The
// temporaries (four bytes per 1024 nodes, a header and, for the host form, four bytes per layer) are one DeviceScratch per device; the
// steps round the launches are its (host_support.h).
#include "slice_kernels.h"
#include "host_support.h"
#include "abi_guard.h"

#include <chrono>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <mutex>

using namespace sdfhip;

static_assert(sizeof(sdfhip_slice_options) == 32 && sizeof(sdfhip_segment) == 32 && sizeof(sdfhip_slice_stats) == 28 && sizeof(sdfhip_slice) == 32,
              "the slice records of include/sdfhip.h");

namespace {

constexpr unsigned long long MAX_SEGMENTS = 0x7FFFFFFFull;
constexpr uint32_t MAX_LAYERS = 65536;

DeviceScratch g_temp[MAX_DEVICES];

// laboratory library: SDFHIP_SLICE_FAIL_ALLOC=k fails the call's k-th allocation (0 = the first)
struct Knobs { AllocFault alloc{ "SDFHIP_SLICE_FAIL_ALLOC" }; };

struct Request { int32_t level; SlicePlanes pl; };

int check_options(const char *what, const sdfhip_slice_options *opt, Request *rq)
{
    rq->level = -1;
    rq->pl = SlicePlanes{ 0.0f, 0.0f, 1.0f, 0.5f, 0.0f, 1u };
    if (!opt) return SDFHIP_OK;
    if (const int rc = check_options_size(what, opt, sizeof(sdfhip_slice_options), "sdfhip_slice_options_default sets the size")) return rc;
    if (const int rc = check_level(what, opt->level)) return rc;
    const float *nr = opt->normal;
    if (!std::isfinite(nr[0]) || !std::isfinite(nr[1]) || !std::isfinite(nr[2]) || (nr[0] == 0.0f && nr[1] == 0.0f && nr[2] == 0.0f))
        return fail(SDFHIP_ERR_ARG, "%s: the normal (%g, %g, %g) is not finite or is zero", what, nr[0], nr[1], nr[2]);
    if (!std::isfinite(opt->offset)) return fail(SDFHIP_ERR_ARG, "%s: the offset %g is not finite", what, opt->offset);
    if (opt->layers == 0u || opt->layers > MAX_LAYERS) return fail(SDFHIP_ERR_ARG, "%s: %u layers, neither 1 nor up to %u", what, opt->layers, MAX_LAYERS);
    if (!std::isfinite(opt->pitch) || (opt->layers > 1u && !(opt->pitch > 0.0f)))
        return fail(SDFHIP_ERR_ARG, "%s: the pitch %g is not finite, or not above zero for %u layers", what, opt->pitch, opt->layers);
    rq->level = opt->level;
    rq->pl = SlicePlanes{ nr[0], nr[1], nr[2], opt->offset, opt->pitch, opt->layers };
    return SDFHIP_OK;
}

uint32_t chunks_of(uint32_t n) { return (uint32_t)(((uint64_t)n + SLICE_CHUNK - 1) / SLICE_CHUNK); }
SliceHeader *header(DeviceScratch &t) { return t.head<SliceHeader>(); }
uint32_t *chunk_array(DeviceScratch &t) { return t.behind_head<uint32_t>(); }
// the host form's per-layer counts, behind the chunk totals
uint32_t *count_array(DeviceScratch &t, uint32_t nchunk) { return chunk_array(t) + nchunk; }

// Under the DeviceScratch's lock and the handle's lock, on its device: count and scan on `st`, the header on the host when this returns.
// own_counts: the per-layer counts go to the block's own array (the host form); otherwise to d_counts, which may be null.
int count_pass(sdfhip_scene *s, const char *what, DeviceScratch &t, Knobs &knobs, const Request &rq, bool want_stats, bool own_counts, uint32_t *d_counts,
               hipStream_t st, SliceHeader *h, float *ms)
{
    const uint32_t nchunk = chunks_of(s->n);
    const size_t need = HEAD_BYTES + ((size_t)nchunk + (own_counts ? rq.pl.layers : 0u)) * sizeof(uint32_t);
    if (const int rc = t.begin(what, knobs.alloc, need, "chunk totals and layer counts", st)) return rc;
    if (own_counts) d_counts = count_array(t, nchunk);
    if (d_counts) HIP_TRY(hipMemsetAsync(d_counts, 0, (size_t)rq.pl.layers * sizeof(uint32_t), st));
    const auto launch = [&] {
        if (want_stats) hipLaunchKernelGGL(k_slice_count<true>, dim3(nchunk), dim3(SLICE_THREADS), 0, st, s->nodes, s->n, rq.level, rq.pl, chunk_array(t), header(t), d_counts);
        else hipLaunchKernelGGL(k_slice_count<false>, dim3(nchunk), dim3(SLICE_THREADS), 0, st, s->nodes, s->n, rq.level, rq.pl, chunk_array(t), header(t), d_counts);
        hipLaunchKernelGGL(k_scan_chunk_totals<unsigned long long>, dim3(1), dim3(1024), 0, st, chunk_array(t), nchunk, &header(t)->n_segments);
    };
    if (const int rc = t.count(st, launch, h, ms)) return rc;
    if (h->n_segments > MAX_SEGMENTS)
        return fail(SDFHIP_ERR_ARG, "%s: the slice would have %llu segments, more than 2^31 - 1", what, h->n_segments);
    return SDFHIP_OK;
}

// ... the emit's launch behind it on `st`
void launch_emit(sdfhip_scene *s, DeviceScratch &t, const Request &rq, sdfhip_segment *d_segments, hipStream_t st)
{
    hipLaunchKernelGGL(k_slice_emit, dim3(chunks_of(s->n)), dim3(SLICE_THREADS), 0, st, s->nodes, s->n, rq.level, rq.pl, chunk_array(t), d_segments);
}

}  // namespace

extern "C" void sdfhip_slice_options_default(sdfhip_slice_options *opt)
try {
    if (!opt) { (void)fail(SDFHIP_ERR_ARG, "slice_options_default: null argument"); return; }
    opt->size = (uint32_t)sizeof(sdfhip_slice_options);
    opt->level = -1;
    opt->normal[0] = 0.0f; opt->normal[1] = 0.0f; opt->normal[2] = 1.0f;
    opt->offset = 0.5f;
    opt->pitch = 0.0f;
    opt->layers = 1u;
}
SDFHIP_ABI_CATCH_VOID(sdfhip_slice_options_default)

extern "C" void sdfhip_slice_free(sdfhip_slice *slice)
try {
    if (!slice) { (void)fail(SDFHIP_ERR_ARG, "slice_free: null argument"); return; }
    free(slice->segments);
    free(slice->layer_counts);
    slice->segments = nullptr; slice->layer_counts = nullptr; slice->n_segments = 0; slice->layers = 0;
}
SDFHIP_ABI_CATCH_VOID(sdfhip_slice_free)

extern "C" int sdfhip_scene_slice_device(sdfhip_scene *scene, const sdfhip_slice_options *opt, sdfhip_segment *d_segments, uint32_t capacity_segments,
                                         uint32_t *d_layer_counts, uint32_t *n_segments, void *stream)
try {
    const char *what = "scene_slice_device";
    if (!scene || !n_segments) return fail(SDFHIP_ERR_ARG, "%s: null argument", what);
    *n_segments = 0;
    Request rq;
    if (const int rc = check_options(what, opt, &rq)) return rc;
    if (capacity_segments && !d_segments) return fail(SDFHIP_ERR_ARG, "%s: a capacity of %u segments and no buffer", what, capacity_segments);
    if (reinterpret_cast<uintptr_t>(d_segments) & 15u) return fail(SDFHIP_ERR_ARG, "%s: the segment buffer is not 16-byte aligned", what);
    if (const int rc = check_cell_scene(what, scene, "no slice")) return rc;
    DeviceScratch &t = g_temp[scene->device];
    Knobs knobs;
    std::lock_guard<std::mutex> hold(t.lock);
    std::lock_guard<std::mutex> lk(scene->lock);
    DeviceGuard g(scene->device);
    if (!g.ok) return fail(SDFHIP_ERR_DEVICE, "%s: hipSetDevice(%d) failed", what, scene->device);
    const hipStream_t st = (hipStream_t)stream;
    SliceHeader h;
    int rc = count_pass(scene, what, t, knobs, rq, false, false, d_layer_counts, st, &h, nullptr);
    if (rc == SDFHIP_OK) {
        *n_segments = (uint32_t)h.n_segments;
        if (h.n_segments && h.n_segments <= capacity_segments) rc = t.emit(st, [&] { launch_emit(scene, t, rq, d_segments, st); });
    }
    t.release();
    return rc;
}
SDFHIP_ABI_CATCH(sdfhip_scene_slice_device)

extern "C" int sdfhip_scene_slice(sdfhip_scene *scene, const sdfhip_slice_options *opt, sdfhip_slice *out, sdfhip_slice_stats *stats)
try {
    const char *what = "scene_slice";
    const auto t0 = std::chrono::steady_clock::now();
    if (out) { out->n_segments = 0; out->segments = nullptr; out->layers = 0; out->layer_counts = nullptr; }
    if (!scene || !out) return fail(SDFHIP_ERR_ARG, "%s: null argument", what);
    Request rq;
    if (const int rc = check_options(what, opt, &rq)) return rc;
    if (const int rc = check_cell_scene(what, scene, "no slice")) return rc;
    DeviceScratch &t = g_temp[scene->device];
    Knobs knobs;
    std::lock_guard<std::mutex> hold(t.lock);
    DeviceGuard g(scene->device);
    if (!g.ok) return fail(SDFHIP_ERR_DEVICE, "%s: hipSetDevice(%d) failed", what, scene->device);
    SliceHeader h;
    float count_ms = 0.0f, emit_ms = 0.0f;
    sdfhip_segment *d_segs = nullptr, *segs = nullptr;
    uint32_t *counts = nullptr;
    size_t d_cap = 0;
    const size_t count_bytes = (size_t)rq.pl.layers * sizeof(uint32_t);
    const int rc = [&]() -> int {
        std::lock_guard<std::mutex> lk(scene->lock);
        const hipStream_t st = scene->stream;
        if (const int r = count_pass(scene, what, t, knobs, rq, stats != nullptr, true, nullptr, st, &h, &count_ms)) return r;
        counts = knobs.alloc.next() ? nullptr : static_cast<uint32_t *>(malloc(count_bytes));
        if (!counts) return fail(SDFHIP_ERR_NOMEM, "%s: out of host memory for the counts of %u layers", what, rq.pl.layers);
        const uint32_t *d_counts = count_array(t, chunks_of(scene->n));
        if (!h.n_segments) {
            HIP_TRY(hipMemcpyAsync(counts, d_counts, count_bytes, hipMemcpyDeviceToHost, st));
            HIP_TRY(hipStreamSynchronize(st));
            return SDFHIP_OK;
        }
        const size_t bytes = (size_t)h.n_segments * sizeof(sdfhip_segment);
        if (knobs.alloc.next() || grow_buffer(d_segs, d_cap, bytes) != hipSuccess) {
            (void)hipGetLastError();
            return fail(SDFHIP_ERR_NOMEM, "%s: out of device memory for %llu segments (%zu bytes)", what, h.n_segments, bytes);
        }
        segs = knobs.alloc.next() ? nullptr : static_cast<sdfhip_segment *>(malloc(bytes));
        if (!segs) return fail(SDFHIP_ERR_NOMEM, "%s: out of host memory for %llu segments (%zu bytes)", what, h.n_segments, bytes);
        const auto copy_out = [&]() -> int {
            HIP_TRY(hipMemcpyAsync(segs, d_segs, bytes, hipMemcpyDeviceToHost, st));
            HIP_TRY(hipMemcpyAsync(counts, d_counts, count_bytes, hipMemcpyDeviceToHost, st));
            return SDFHIP_OK;
        };
        return t.emit_to_host(st, [&] { launch_emit(scene, t, rq, d_segs, st); }, copy_out, &emit_ms);
    }();
    t.settle(scene->stream);
    release_buffer(d_segs, d_cap);
    t.release();
    if (rc != SDFHIP_OK) { free(segs); free(counts); return rc; }
    out->n_segments = (uint32_t)h.n_segments;
    out->segments = segs;
    out->layers = rq.pl.layers;
    out->layer_counts = counts;
    if (stats) {
        stats->nodes = scene->n; stats->cells = h.cells; stats->cells_cut = h.cells_cut; stats->cells_crossed = h.cells_crossed;
        stats->n_segments = (uint32_t)h.n_segments;
        stats->kernel_ms = count_ms + emit_ms;
        stats->total_ms = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
    }
    return SDFHIP_OK;
}
SDFHIP_ABI_CATCH(sdfhip_scene_slice)
