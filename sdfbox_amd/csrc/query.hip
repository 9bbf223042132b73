// libsdfhip.so, point and ray queries: sdfhip_scene_sample / _raycast / _pick and the _device forms of the first two -- what a
// resident scene answers without drawing a frame (kernels: query_kernels.h).
//
// Replaces: nothing in the reference's code.  Its only consumer of the tree is Compute.hlsl; a host that wants the distance at a
// point or the surface under the cursor has no call to make there.  (This project's own tests and scripts placed their brushes
// with a numpy walk over every deepest leaf, on the host.)
//
// The _device forms launch on the caller's stream and return; the host forms stage their records through device buffers on the
// scene's own stream and wait.  The staging buffers cannot live in the scene handle (scene.h belongs to the renderer's measured
// sources), so small ones are kept per device here and large ones live for the call.
#include "query_kernels.h"
#include "host_support.h"
#include "abi_guard.h"

#include <cmath>
#include <cstring>
#include <mutex>

using namespace sdfhip;

static_assert(sizeof(sdfhip_probe) == 32 && sizeof(sdfhip_ray) == 32 && sizeof(sdfhip_hit) == 48, "the query records are 2, 2 and 3 x 16 bytes");
static_assert(SDFHIP_QUERY_HIT == QUERY_HIT && SDFHIP_QUERY_ESCAPED == QUERY_ESCAPED && SDFHIP_QUERY_EXHAUSTED == QUERY_EXHAUSTED &&
              SDFHIP_QUERY_INVALID == QUERY_INVALID, "query_kernels.h restates the header's status codes");

namespace {

constexpr uint32_t QUERY_MAX_STEPS = 4096;
constexpr int MAX_DEVICES = 64;
constexpr size_t KEEP_BYTES = (size_t)16 << 20;     // staging buffers up to this size stay allocated between calls

enum Form { FORM_GENERIC = 0, FORM_GRID = 1, FORM_SPLIT = 2 };

// The march takes the renderer's SDFHIP_KERNEL_AUTO: the grid lookup wherever the handle has a full-depth grid -- 0.155 against 0.58 ms
// for a 1080p frame's rays on the 28 M-node scene.  A sample is ONE lookup per point and wants the cell's index with it: the walk from
// the root yields distance and index in `level` loads, while the grid yields the bytes in one or two and then pays that same walk for
// the index -- 0.058 against 0.043 ms per 1 M uniform points, so sample walks the links on every scene (profiles/query_bench.json).
// (laboratory library: SDFHIP_QUERY_FORM=generic / grid forces one form for both -- the A/B above, and the tests' second form;
// SDFHIP_QUERY_STORE=plain stores the records with plain stores)
Form form_of(const sdfhip_scene *s, bool sample)
{
    if (!scene_has_full_depth_grid(s)) return FORM_GENERIC;
    bool grid = !sample;
    if (const char *e = lab_env("SDFHIP_QUERY_FORM")) {
        if (!strcmp(e, "generic")) grid = false;
        else if (!strcmp(e, "grid")) grid = true;
    }
    return !grid ? FORM_GENERIC : s->fine_bits ? FORM_SPLIT : FORM_GRID;
}
bool nt_stores()
{
    const char *e = lab_env("SDFHIP_QUERY_STORE");
    return !(e && !strcmp(e, "plain"));
}

QueryScene scene_of(const sdfhip_scene *s)
{
    return QueryScene{s->nodes, s->n, s->d_top, s->d_fine, s->top_level, s->fine_bits};
}

dim3 blocks_of(uint32_t n) { return dim3((n + QUERY_THREADS - 1) / QUERY_THREADS); }

template <class CursorT>
void launch_sample_as(const QueryScene &Q, const float *d_xyz, uint32_t n, sdfhip_probe *d_out, hipStream_t st, bool nt)
{
    uint4 *out = reinterpret_cast<uint4 *>(d_out);
    if (nt) hipLaunchKernelGGL((k_query_sample<CursorT, true>), blocks_of(n), dim3(QUERY_THREADS), 0, st, Q, d_xyz, n, out);
    else hipLaunchKernelGGL((k_query_sample<CursorT, false>), blocks_of(n), dim3(QUERY_THREADS), 0, st, Q, d_xyz, n, out);
}
template <class CursorT, bool PICK>
void launch_march_as(const QueryScene &Q, const void *d_in, uint32_t n, const FrameInfo &I, uint32_t max_steps, sdfhip_hit *d_out,
                     hipStream_t st, bool nt)
{
    uint4 *out = reinterpret_cast<uint4 *>(d_out);
    if (nt) hipLaunchKernelGGL((k_query_march<CursorT, PICK, true>), blocks_of(n), dim3(QUERY_THREADS), 0, st, Q, d_in, n, I, max_steps, out);
    else hipLaunchKernelGGL((k_query_march<CursorT, PICK, false>), blocks_of(n), dim3(QUERY_THREADS), 0, st, Q, d_in, n, I, max_steps, out);
}

// under the handle's lock, on its device
int launch_sample(sdfhip_scene *s, const float *d_xyz, uint32_t n, sdfhip_probe *d_out, hipStream_t st)
{
    const QueryScene Q = scene_of(s);
    const bool nt = nt_stores();
    switch (form_of(s, true)) {
    case FORM_GRID: launch_sample_as<CursorFT<false, false>>(Q, d_xyz, n, d_out, st, nt); break;
    case FORM_SPLIT: launch_sample_as<CursorFT<false, true>>(Q, d_xyz, n, d_out, st, nt); break;
    default: launch_sample_as<CursorG>(Q, d_xyz, n, d_out, st, nt); break;
    }
    HIP_TRY(hipGetLastError());
    return SDFHIP_OK;
}
template <bool PICK>
int launch_march(sdfhip_scene *s, const void *d_in, uint32_t n, const FrameInfo &I, uint32_t max_steps, sdfhip_hit *d_out, hipStream_t st)
{
    const QueryScene Q = scene_of(s);
    const bool nt = nt_stores();
    switch (form_of(s, false)) {
    case FORM_GRID: launch_march_as<CursorFT<false, false>, PICK>(Q, d_in, n, I, max_steps, d_out, st, nt); break;
    case FORM_SPLIT: launch_march_as<CursorFT<false, true>, PICK>(Q, d_in, n, I, max_steps, d_out, st, nt); break;
    default: launch_march_as<CursorG, PICK>(Q, d_in, n, I, max_steps, d_out, st, nt); break;
    }
    HIP_TRY(hipGetLastError());
    return SDFHIP_OK;
}

int check_march_args(const char *what, float margin, float limit, uint32_t max_steps)
{
    if (max_steps < 1u || max_steps > QUERY_MAX_STEPS) return fail(SDFHIP_ERR_ARG, "%s: max_steps %u outside 1..%u", what, max_steps, QUERY_MAX_STEPS);
    if (!std::isfinite(margin) || !std::isfinite(limit)) return fail(SDFHIP_ERR_ARG, "%s: margin and limit must be finite", what);
    return SDFHIP_OK;
}

// The host forms' staging buffers: one pair per device, grown on demand; a call holds its device's pair until its answer is on
// the host.  A pair larger than KEEP_BYTES is given back when the call ends.
struct Staging {
    std::mutex lock;
    void *in = nullptr, *out = nullptr;
    size_t in_cap = 0, out_cap = 0;
};
Staging g_staging[MAX_DEVICES];

int grow(void *&p, size_t &cap, size_t need, const char *what)
{
    if (grow_buffer(p, cap, need) == hipSuccess) return SDFHIP_OK;
    (void)hipGetLastError();
    return fail(SDFHIP_ERR_NOMEM, "%s: out of device memory for %zu bytes of query records", what, need);
}

// host records in -> launch -> host records out, on the scene's own stream.  launch(d_in, d_out) runs under the handle's lock.
template <class Launch>
int through_staging(sdfhip_scene *s, const char *what, const void *h_in, size_t in_bytes, void *h_out, size_t out_bytes, Launch launch)
{
    if (s->device < 0 || s->device >= MAX_DEVICES) return fail(SDFHIP_ERR_ARG, "%s: device %d", what, s->device);
    Staging &b = g_staging[s->device];
    std::lock_guard<std::mutex> hold(b.lock);
    DeviceGuard g(s->device);
    if (!g.ok) return fail(SDFHIP_ERR_DEVICE, "%s: hipSetDevice(%d) failed", what, s->device);
    int rc = grow(b.in, b.in_cap, in_bytes, what);
    if (rc == SDFHIP_OK) rc = grow(b.out, b.out_cap, out_bytes, what);
    if (rc == SDFHIP_OK) {
        std::lock_guard<std::mutex> lk(s->lock);
        const hipStream_t st = s->stream;
        rc = [&]() -> int {
            HIP_TRY(hipMemcpyAsync(b.in, h_in, in_bytes, hipMemcpyHostToDevice, st));
            const int r = launch(b.in, b.out, st);
            if (r != SDFHIP_OK) return r;
            HIP_TRY(hipMemcpyAsync(h_out, b.out, out_bytes, hipMemcpyDeviceToHost, st));
            HIP_TRY(hipStreamSynchronize(st));
            return SDFHIP_OK;
        }();
        if (rc != SDFHIP_OK) (void)hipStreamSynchronize(st);      // nothing of this call is in flight when the buffers are handed on
    }
    release_buffer(b.in, b.in_cap, KEEP_BYTES);
    release_buffer(b.out, b.out_cap, KEEP_BYTES);
    return rc;
}

// a launch on the caller's stream, under the handle's lock
template <class Launch>
int on_device(sdfhip_scene *s, const char *what, Launch launch)
{
    std::lock_guard<std::mutex> lk(s->lock);
    DeviceGuard g(s->device);
    if (!g.ok) return fail(SDFHIP_ERR_DEVICE, "%s: hipSetDevice(%d) failed", what, s->device);
    return launch();
}

}  // namespace

extern "C" int sdfhip_scene_sample_device(sdfhip_scene *scene, const float *d_xyz, uint32_t n, sdfhip_probe *d_out, void *stream)
try {
    if (!scene) return fail(SDFHIP_ERR_ARG, "scene_sample_device: null scene");
    if (n == 0) return SDFHIP_OK;
    if (!d_xyz || !d_out) return fail(SDFHIP_ERR_ARG, "scene_sample_device: null argument");
    return on_device(scene, "scene_sample_device", [&]() { return launch_sample(scene, d_xyz, n, d_out, (hipStream_t)stream); });
}
SDFHIP_ABI_CATCH(sdfhip_scene_sample_device)

extern "C" int sdfhip_scene_sample(sdfhip_scene *scene, const float *xyz, uint32_t n, sdfhip_probe *out)
try {
    if (!scene) return fail(SDFHIP_ERR_ARG, "scene_sample: null scene");
    if (n == 0) return SDFHIP_OK;
    if (!xyz || !out) return fail(SDFHIP_ERR_ARG, "scene_sample: null argument");
    return through_staging(scene, "scene_sample", xyz, (size_t)n * 12, out, (size_t)n * sizeof(sdfhip_probe),
                           [&](void *d_in, void *d_out, hipStream_t st) {
                               return launch_sample(scene, static_cast<const float *>(d_in), n, static_cast<sdfhip_probe *>(d_out), st);
                           });
}
SDFHIP_ABI_CATCH(sdfhip_scene_sample)

extern "C" int sdfhip_scene_raycast_device(sdfhip_scene *scene, const sdfhip_ray *d_rays, uint32_t n, float margin, float limit,
                                           uint32_t max_steps, sdfhip_hit *d_out, void *stream)
try {
    if (!scene) return fail(SDFHIP_ERR_ARG, "scene_raycast_device: null scene");
    if (const int rc = check_march_args("scene_raycast_device", margin, limit, max_steps)) return rc;
    if (n == 0) return SDFHIP_OK;
    if (!d_rays || !d_out) return fail(SDFHIP_ERR_ARG, "scene_raycast_device: null argument");
    FrameInfo I;
    memset(&I, 0, sizeof I);
    I.margin = margin; I.margin2 = margin * 2.0f; I.limit = limit;
    return on_device(scene, "scene_raycast_device", [&]() { return launch_march<false>(scene, d_rays, n, I, max_steps, d_out, (hipStream_t)stream); });
}
SDFHIP_ABI_CATCH(sdfhip_scene_raycast_device)

extern "C" int sdfhip_scene_raycast(sdfhip_scene *scene, const sdfhip_ray *rays, uint32_t n, float margin, float limit, uint32_t max_steps,
                                    sdfhip_hit *out)
try {
    if (!scene) return fail(SDFHIP_ERR_ARG, "scene_raycast: null scene");
    if (const int rc = check_march_args("scene_raycast", margin, limit, max_steps)) return rc;
    if (n == 0) return SDFHIP_OK;
    if (!rays || !out) return fail(SDFHIP_ERR_ARG, "scene_raycast: null argument");
    FrameInfo I;
    memset(&I, 0, sizeof I);
    I.margin = margin; I.margin2 = margin * 2.0f; I.limit = limit;
    return through_staging(scene, "scene_raycast", rays, (size_t)n * sizeof(sdfhip_ray), out, (size_t)n * sizeof(sdfhip_hit),
                           [&](void *d_in, void *d_out, hipStream_t st) {
                               return launch_march<false>(scene, d_in, n, I, max_steps, static_cast<sdfhip_hit *>(d_out), st);
                           });
}
SDFHIP_ABI_CATCH(sdfhip_scene_raycast)

extern "C" int sdfhip_scene_pick(sdfhip_scene *scene, const sdfhip_info *info, const uint32_t *pixels_xy, uint32_t n, uint32_t max_steps,
                                 sdfhip_hit *out)
try {
    if (!scene || !info) return fail(SDFHIP_ERR_ARG, "scene_pick: null argument");
    if (const int rc = check_march_args("scene_pick", info->margin, info->limit, max_steps)) return rc;
    if (n == 0) return SDFHIP_OK;
    if (!pixels_xy || !out) return fail(SDFHIP_ERR_ARG, "scene_pick: null argument");
    FrameInfo I;
    unpack_camera(info, I);
    return through_staging(scene, "scene_pick", pixels_xy, (size_t)n * 8, out, (size_t)n * sizeof(sdfhip_hit),
                           [&](void *d_in, void *d_out, hipStream_t st) {
                               return launch_march<true>(scene, d_in, n, I, max_steps, static_cast<sdfhip_hit *>(d_out), st);
                           });
}
SDFHIP_ABI_CATCH(sdfhip_scene_pick)
