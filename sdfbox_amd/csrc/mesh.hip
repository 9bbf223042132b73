// libsdfhip.so, surface extraction: sdfhip_scene_mesh / sdfhip_scene_mesh_device -- a resident scene as a triangle soup of
// {position, normal} vertices, the layout of sdfhip_points.data (kernels: mesh_kernels.h; the .ply / .obj writers: mesh_io.cpp).
//
// Replaces: nothing in the reference's code.  Its tree only ever becomes pixels; a scene built, carved and picked here had no way
// out as geometry.
//
// Per call: k_mesh_count and the chunk scan on the call's stream, one host synchronisation for the triangle total (it sizes the output
// and is what the _device form always returns), then k_mesh_emit.  The _device form leaves the emit in flight on the caller's stream;
// the host form runs on the scene's own stream, copies the vertices out and waits.  The temporaries (four bytes per 1024 nodes and a
// 16-byte header) are one DeviceScratch per device; the steps round the launches are its (host_support.h).
#include "mesh_kernels.h"
#include "host_support.h"
#include "abi_guard.h"

#include <chrono>
#include <cstdlib>
#include <cstring>
#include <mutex>

using namespace sdfhip;

static_assert(sizeof(sdfhip_mesh_options) == 8 && sizeof(sdfhip_mesh_stats) == 24, "the mesh records of include/sdfhip.h");

namespace {

constexpr unsigned long long MAX_TRIANGLES = 0x7FFFFFFFull;

DeviceScratch g_temp[MAX_DEVICES];

// The vertices are stored with plain 16-byte stores: 2.15 against 2.92 ms with non-temporal ones for the 27.5 M triangles of the 28 M-node
// scene, 4.59 ms with 8-byte stores (count + emit; profiles/mesh_bench.json) -- unlike the query records, a lane's triangles are neighbours of the next
// lane's, and the caches merge them into whole lines.
// laboratory library: SDFHIP_MESH_STORE=nt stores them non-temporally, SDFHIP_MESH_VEC=8 with 8-byte stores only (the A/Bs of
// DESIGN.md N7); SDFHIP_MESH_FAIL_ALLOC=k fails the call's k-th allocation (0 = the first)
struct Knobs {
    bool nt = false, wide = true;
    AllocFault alloc{ "SDFHIP_MESH_FAIL_ALLOC" };
    Knobs()
    {
        if (const char *e = lab_env("SDFHIP_MESH_STORE")) nt = strcmp(e, "nt") == 0;
        if (const char *e = lab_env("SDFHIP_MESH_VEC")) wide = strcmp(e, "8") != 0;
    }
};

int check_options(const char *what, const sdfhip_mesh_options *opt, int32_t *level)
{
    *level = -1;
    if (!opt) return SDFHIP_OK;
    if (const int rc = check_options_size(what, opt, sizeof(sdfhip_mesh_options), "sdfhip_mesh_options_default sets the size")) return rc;
    if (const int rc = check_level(what, opt->level)) return rc;
    *level = opt->level;
    return SDFHIP_OK;
}

uint32_t chunks_of(uint32_t n) { return (uint32_t)(((uint64_t)n + MESH_CHUNK - 1) / MESH_CHUNK); }
uint32_t *chunk_array(DeviceScratch &t) { return t.behind_head<uint32_t>(); }
MeshHeader *header(DeviceScratch &t) { return t.head<MeshHeader>(); }

// Under the DeviceScratch's lock and the handle's lock, on its device: count and scan on `st`, the header on the host when this returns.
int count_pass(sdfhip_scene *s, const char *what, DeviceScratch &t, Knobs &knobs, int32_t level, bool want_stats, hipStream_t st, MeshHeader *h, float *ms)
{
    const uint32_t nchunk = chunks_of(s->n);
    if (const int rc = t.begin(what, knobs.alloc, HEAD_BYTES + (size_t)nchunk * sizeof(uint32_t), "chunk totals", st)) return rc;
    const auto launch = [&] {
        if (want_stats) hipLaunchKernelGGL(k_mesh_count<true>, dim3(nchunk), dim3(MESH_THREADS), 0, st, s->nodes, s->n, level, chunk_array(t), header(t));
        else hipLaunchKernelGGL(k_mesh_count<false>, dim3(nchunk), dim3(MESH_THREADS), 0, st, s->nodes, s->n, level, chunk_array(t), header(t));
        hipLaunchKernelGGL(k_scan_chunk_totals<unsigned long long>, dim3(1), dim3(1024), 0, st, chunk_array(t), nchunk, &header(t)->n_triangles);
    };
    if (const int rc = t.count(st, launch, h, ms)) return rc;
    if (h->n_triangles > MAX_TRIANGLES)
        return fail(SDFHIP_ERR_ARG, "%s: the mesh would have %llu triangles, more than 2^31 - 1", what, h->n_triangles);
    return SDFHIP_OK;
}

// ... the emit's launch behind it on `st`
void launch_emit(sdfhip_scene *s, DeviceScratch &t, const Knobs &knobs, int32_t level, float *d_verts6, hipStream_t st)
{
    const dim3 grid(chunks_of(s->n)), block(MESH_THREADS);
    if (knobs.nt && knobs.wide) hipLaunchKernelGGL((k_mesh_emit<true, true>), grid, block, 0, st, s->nodes, s->n, level, chunk_array(t), d_verts6);
    else if (knobs.nt) hipLaunchKernelGGL((k_mesh_emit<true, false>), grid, block, 0, st, s->nodes, s->n, level, chunk_array(t), d_verts6);
    else if (knobs.wide) hipLaunchKernelGGL((k_mesh_emit<false, true>), grid, block, 0, st, s->nodes, s->n, level, chunk_array(t), d_verts6);
    else hipLaunchKernelGGL((k_mesh_emit<false, false>), grid, block, 0, st, s->nodes, s->n, level, chunk_array(t), d_verts6);
}

}  // namespace

extern "C" void sdfhip_mesh_options_default(sdfhip_mesh_options *opt)
try {
    if (!opt) { (void)fail(SDFHIP_ERR_ARG, "mesh_options_default: null argument"); return; }
    opt->size = (uint32_t)sizeof(sdfhip_mesh_options);
    opt->level = -1;
}
SDFHIP_ABI_CATCH_VOID(sdfhip_mesh_options_default)

extern "C" int sdfhip_scene_mesh_device(sdfhip_scene *scene, const sdfhip_mesh_options *opt, float *d_verts6, uint32_t capacity_triangles,
                                        uint32_t *n_triangles, void *stream)
try {
    const char *what = "scene_mesh_device";
    if (!scene || !n_triangles) return fail(SDFHIP_ERR_ARG, "%s: null argument", what);
    *n_triangles = 0;
    int32_t level;
    if (const int rc = check_options(what, opt, &level)) return rc;
    if (capacity_triangles && !d_verts6) return fail(SDFHIP_ERR_ARG, "%s: a capacity of %u triangles and no buffer", what, capacity_triangles);
    if (const int rc = check_cell_scene(what, scene, "no mesh")) return rc;
    DeviceScratch &t = g_temp[scene->device];
    Knobs knobs;
    std::lock_guard<std::mutex> hold(t.lock);
    std::lock_guard<std::mutex> lk(scene->lock);
    DeviceGuard g(scene->device);
    if (!g.ok) return fail(SDFHIP_ERR_DEVICE, "%s: hipSetDevice(%d) failed", what, scene->device);
    const hipStream_t st = (hipStream_t)stream;
    MeshHeader h;
    int rc = count_pass(scene, what, t, knobs, level, false, st, &h, nullptr);
    if (rc == SDFHIP_OK) {
        *n_triangles = (uint32_t)h.n_triangles;
        if (h.n_triangles && h.n_triangles <= capacity_triangles) rc = t.emit(st, [&] { launch_emit(scene, t, knobs, level, d_verts6, st); });
    }
    t.release();
    return rc;
}
SDFHIP_ABI_CATCH(sdfhip_scene_mesh_device)

extern "C" int sdfhip_scene_mesh(sdfhip_scene *scene, const sdfhip_mesh_options *opt, sdfhip_mesh *out, sdfhip_mesh_stats *stats)
try {
    const char *what = "scene_mesh";
    const auto t0 = std::chrono::steady_clock::now();
    if (!scene || !out) return fail(SDFHIP_ERR_ARG, "%s: null argument", what);
    out->n_triangles = 0; out->verts6 = nullptr;
    int32_t level;
    if (const int rc = check_options(what, opt, &level)) return rc;
    if (const int rc = check_cell_scene(what, scene, "no mesh")) return rc;
    DeviceScratch &t = g_temp[scene->device];
    Knobs knobs;
    std::lock_guard<std::mutex> hold(t.lock);
    DeviceGuard g(scene->device);
    if (!g.ok) return fail(SDFHIP_ERR_DEVICE, "%s: hipSetDevice(%d) failed", what, scene->device);
    MeshHeader h;
    float count_ms = 0.0f, emit_ms = 0.0f;
    float *d_verts = nullptr, *verts = nullptr;
    size_t d_cap = 0;
    const int rc = [&]() -> int {
        std::lock_guard<std::mutex> lk(scene->lock);
        const hipStream_t st = scene->stream;
        if (const int r = count_pass(scene, what, t, knobs, level, stats != nullptr, st, &h, &count_ms)) return r;
        if (!h.n_triangles) return SDFHIP_OK;
        const size_t bytes = (size_t)h.n_triangles * 18 * sizeof(float);
        if (knobs.alloc.next() || grow_buffer(d_verts, d_cap, bytes) != hipSuccess) {
            (void)hipGetLastError();
            return fail(SDFHIP_ERR_NOMEM, "%s: out of device memory for %llu triangles (%zu bytes)", what, h.n_triangles, bytes);
        }
        verts = knobs.alloc.next() ? nullptr : static_cast<float *>(malloc(bytes));
        if (!verts) return fail(SDFHIP_ERR_NOMEM, "%s: out of host memory for %llu triangles (%zu bytes)", what, h.n_triangles, bytes);
        const auto copy_out = [&]() -> int { HIP_TRY(hipMemcpyAsync(verts, d_verts, bytes, hipMemcpyDeviceToHost, st)); return SDFHIP_OK; };
        return t.emit_to_host(st, [&] { launch_emit(scene, t, knobs, level, d_verts, st); }, copy_out, &emit_ms);
    }();
    t.settle(scene->stream);
    release_buffer(d_verts, d_cap);
    t.release();
    if (rc != SDFHIP_OK) { free(verts); return rc; }
    out->n_triangles = (uint32_t)h.n_triangles;
    out->verts6 = verts;
    if (stats) {
        stats->nodes = scene->n; stats->cells = h.cells; stats->cells_cut = h.cells_cut; stats->n_triangles = (uint32_t)h.n_triangles;
        stats->kernel_ms = count_ms + emit_ms;
        stats->total_ms = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
    }
    return SDFHIP_OK;
}
SDFHIP_ABI_CATCH(sdfhip_scene_mesh)
