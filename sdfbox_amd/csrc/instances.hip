// libsdfhip.so, an assembly of placed instances consumed without baking: sdfhip_instances_sample / _raycast / _pick / _render and
// the _device forms of sample, raycast and render (kernels: instances_kernels.h).
//
// Replaces: nothing in the reference's code; its shader marches one immutable tree.
//
// The rule, pinned (include/sdfhip.h): F is sdfhip_scene_compose's fold evaluated at the marched point,
// w the winner tracked beside it, G six taps of F at distance normal_step; the march is sdfhip_scene_raycast's and the pixel is
// main() of Compute.hlsl with F and G in the places of find + interpol_world and gradient().
//
// Per call: the list is checked as compose.hip checks it, each distinct source is read once under its own lock (read_source), and
// the instance table ({QueryScene, PlaceMap, op, form} per instance) goes to device memory.  A host form works on a stream of its
// own (CallFrame), stages its records through memory of the call and waits.  A _device form copies the table and enqueues the
// kernel on the caller's stream, waits for that stream and frees the table.  Nothing is kept on the handles.
// (place_kernels.h and compose_host.h bring the level loop's kernels with them; this translation unit reads sources and builds no level)
#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Wunneeded-internal-declaration"
#include "instances_kernels.h"
#include "compose_host.h"     // check_instance, read_instance (shared with compose.hip); level_build.h, host_support.h
#pragma clang diagnostic pop
#include "abi_guard.h"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <utility>
#include <vector>

using namespace sdfhip;
using namespace sdfhip::levels;

static_assert(sizeof(sdfhip_instances_options) == 16 && sizeof(sdfhip_part_probe) == 32 && sizeof(sdfhip_part_hit) == 48,
              "the assembly's records of include/sdfhip.h");
static_assert(SDFHIP_COMBINE_UNION == COMPOSE_UNION && SDFHIP_COMBINE_INTERSECT == COMPOSE_INTERSECT && SDFHIP_COMBINE_SUBTRACT == COMPOSE_SUBTRACT,
              "compose_instance.h restates the header's codes");
static_assert(FORM_GENERIC == COMPOSE_FORM_GENERIC && FORM_GRID == COMPOSE_FORM_GRID && FORM_SPLIT == COMPOSE_FORM_SPLIT,
              "compose_instance.h restates level_build.h's forms");
static_assert(SDFHIP_QUERY_HIT == QUERY_HIT && SDFHIP_QUERY_ESCAPED == QUERY_ESCAPED && SDFHIP_QUERY_EXHAUSTED == QUERY_EXHAUSTED &&
              SDFHIP_QUERY_INVALID == QUERY_INVALID, "query_kernels.h restates the header's status codes");

namespace {

constexpr uint32_t INSTANCES_MAX_STEPS = 4096, INSTANCES_MAX_SIDE = 16384;
const char *const FAIL_ALLOC = "SDFHIP_INSTANCES_FAIL_ALLOC";      // laboratory library: AllocFault

// what the call took from its arguments before any device call
struct Assembly {
    std::vector<ComposeInstance> table;
    int device = 0;
    uint32_t max_steps = 100;
    uint32_t skip = 1;
    float h = 0x1p-10f;
};

// the options and everything of the list that needs no handle
int check_call(const char *name, const sdfhip_instance *instances, uint32_t n_instances, const sdfhip_instances_options *opt, Assembly &A)
{
    if (const int rc = check_instance_count(name, instances, n_instances)) return rc;
    if (opt) {
        if (const int rc = check_options_size(name, opt, sizeof(sdfhip_instances_options), "size = sizeof(sdfhip_instances_options)")) return rc;
        if (opt->flags & ~(uint32_t)SDFHIP_INSTANCES_NO_SKIP) return fail(SDFHIP_ERR_ARG, "%s: unknown flags %#x", name, opt->flags);
        if (opt->max_steps > INSTANCES_MAX_STEPS) return fail(SDFHIP_ERR_ARG, "%s: max_steps %u outside 1..%u (0 = 100)", name, opt->max_steps, INSTANCES_MAX_STEPS);
        if (!std::isfinite(opt->normal_step) || opt->normal_step < 0.0f)
            return fail(SDFHIP_ERR_ARG, "%s: normal_step %g is neither 0 nor finite and above 0", name, (double)opt->normal_step);
        if (opt->max_steps) A.max_steps = opt->max_steps;
        if (opt->normal_step != 0.0f) A.h = opt->normal_step;
        A.skip = (opt->flags & SDFHIP_INSTANCES_NO_SKIP) ? 0u : 1u;
    }
    for (uint32_t k = 0; k < n_instances; k++)
        if (const int rc = check_instance(name, instances + k, k)) return rc;
    return SDFHIP_OK;
}

// The table, entry by entry as sdfhip_scene_compose reads it (read_instance)
int read_table(const char *name, const sdfhip_instance *instances, uint32_t n_instances, Assembly &A)
{
    InstanceSources sources;
    A.table.resize(n_instances);
    for (uint32_t k = 0; k < n_instances; k++) {
        const Source *src = nullptr;
        bool fresh = false;
        if (const int rc = read_instance(name, sources, instances[k], k, A.table[k], &src, &fresh)) return rc;
    }
    A.device = sources.front().second.device;
    return SDFHIP_OK;
}

int check_march(const char *name, float margin, float limit)
{
    if (!std::isfinite(margin) || !std::isfinite(limit)) return fail(SDFHIP_ERR_ARG, "%s: margin and limit must be finite", name);
    return SDFHIP_OK;
}
int check_frame(const char *name, uint32_t width, uint32_t height)
{
    if (width > INSTANCES_MAX_SIDE || height > INSTANCES_MAX_SIDE)
        return fail(SDFHIP_ERR_ARG, "%s: a %u x %u frame: each side at most %u", name, width, height, INSTANCES_MAX_SIDE);
    return SDFHIP_OK;
}

FrameInfo march_info(float margin, float limit)
{
    FrameInfo I;
    memset(&I, 0, sizeof I);
    I.margin = margin; I.margin2 = margin * 2.0f; I.limit = limit;
    return I;
}

dim3 blocks_of(uint32_t n) { return dim3((uint32_t)(((uint64_t)n + INSTANCES_THREADS - 1) / INSTANCES_THREADS)); }
PartField field_of(const Assembly &A, const ComposeInstance *d_table) { return PartField{d_table, (uint32_t)A.table.size(), A.skip, A.h}; }

// the three launches: (table on the device, records in, records out, stream)
auto sample_launch(const Assembly &A, uint32_t n)
{
    return [&A, n](const ComposeInstance *d_table, const void *d_in, void *d_out, hipStream_t st) {
        hipLaunchKernelGGL(k_instances_sample, blocks_of(n), dim3(INSTANCES_THREADS), 0, st, field_of(A, d_table), static_cast<const float *>(d_in), n,
                           static_cast<uint4 *>(d_out));
    };
}
template <bool PICK> auto march_launch(const Assembly &A, uint32_t n, const FrameInfo &I)
{
    return [&A, n, I](const ComposeInstance *d_table, const void *d_in, void *d_out, hipStream_t st) {
        hipLaunchKernelGGL(k_instances_march<PICK>, blocks_of(n), dim3(INSTANCES_THREADS), 0, st, field_of(A, d_table), d_in, n, I, A.max_steps,
                           static_cast<uint4 *>(d_out));
    };
}
auto render_launch(const Assembly &A, const FrameInfo &I, uint32_t width, uint32_t height)
{
    return [&A, I, width, height](const ComposeInstance *d_table, const void *, void *d_out, hipStream_t st) {
        const uint32_t tiles_x = (width + 7) / 8, n_tiles = tiles_x * ((height + 7) / 8);
        hipLaunchKernelGGL(k_instances_render, dim3((n_tiles + INSTANCES_THREADS / 64 - 1) / (INSTANCES_THREADS / 64)), dim3(INSTANCES_THREADS), 0, st,
                           field_of(A, d_table), I, A.max_steps, width, height, tiles_x, n_tiles, static_cast<uint4 *>(d_out));
    };
}

// host records in -> launch -> host records out, on a stream of the call's own with memory of the call's own
template <class Launch>
int host_call(const char *name, const Assembly &A, const void *h_in, size_t in_bytes, void *h_out, size_t out_bytes, Launch launch)
{
    CallFrame<1> call(name, A.device, FAIL_ALLOC);
    return call.run("nothing was written", [&](hipStream_t st) -> int {
        ComposeInstance *d_table = call.bufs.get<ComposeInstance>(A.table.size());
        char *d_in = in_bytes ? call.bufs.get<char>(in_bytes) : nullptr;
        char *d_out = call.bufs.get<char>(out_bytes);
        HIP_TRY(hipMemcpyAsync(d_table, A.table.data(), A.table.size() * sizeof(ComposeInstance), hipMemcpyHostToDevice, st));
        if (in_bytes) HIP_TRY(hipMemcpyAsync(d_in, h_in, in_bytes, hipMemcpyHostToDevice, st));
        launch(d_table, d_in, d_out, st);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(h_out, d_out, out_bytes, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        return SDFHIP_OK;
    });
}

// Waits for the caller's stream on whatever path a _device form returns once something of the call may be in flight there: the
// table is freed only afterwards (declared after the buffers, so destroyed before them)
struct Drain {
    hipStream_t st;
    bool waited = false;
    ~Drain() { if (!waited) (void)hipStreamSynchronize(st); }
};

// device records in -> launch -> device records out, on the caller's stream; the table is the call's
template <class Launch>
int device_call(const char *name, const Assembly &A, const void *d_in, void *d_out, hipStream_t st, Launch launch)
try {
    DeviceGuard guard(A.device);
    if (!guard.ok) return fail(SDFHIP_ERR_DEVICE, "%s: hipSetDevice(%d) failed", name, A.device);
    DeviceBuffers bufs(FAIL_ALLOC);
    ComposeInstance *d_table = bufs.get<ComposeInstance>(A.table.size());
    Drain drain{st};
    HIP_TRY(hipMemcpyAsync(d_table, A.table.data(), A.table.size() * sizeof(ComposeInstance), hipMemcpyHostToDevice, st));
    launch(d_table, d_in, d_out, st);
    HIP_TRY(hipGetLastError());
    const hipError_t e = hipStreamSynchronize(st);
    drain.waited = e == hipSuccess;
    HIP_TRY(e);
    return SDFHIP_OK;
} catch (const NoMem &) {
    return fail(SDFHIP_ERR_NOMEM, "%s: out of device memory (nothing was written)", name);
}

}  // namespace

extern "C" int sdfhip_instances_sample(const sdfhip_instance *instances, uint32_t n_instances, const sdfhip_instances_options *opt,
                                       const float *xyz, uint32_t n, sdfhip_part_probe *out)
try {
    Assembly A;
    if (const int rc = check_call("instances_sample", instances, n_instances, opt, A)) return rc;
    if (n == 0) return SDFHIP_OK;
    if (!xyz || !out) return fail(SDFHIP_ERR_ARG, "instances_sample: null argument");
    if (const int rc = read_table("instances_sample", instances, n_instances, A)) return rc;
    return host_call("instances_sample", A, xyz, (size_t)n * 12, out, (size_t)n * sizeof(sdfhip_part_probe), sample_launch(A, n));
}
SDFHIP_ABI_CATCH(sdfhip_instances_sample)

extern "C" int sdfhip_instances_sample_device(const sdfhip_instance *instances, uint32_t n_instances, const sdfhip_instances_options *opt,
                                              const float *d_xyz, uint32_t n, sdfhip_part_probe *d_out, void *stream)
try {
    Assembly A;
    if (const int rc = check_call("instances_sample_device", instances, n_instances, opt, A)) return rc;
    if (n == 0) return SDFHIP_OK;
    if (!d_xyz || !d_out) return fail(SDFHIP_ERR_ARG, "instances_sample_device: null argument");
    if (const int rc = read_table("instances_sample_device", instances, n_instances, A)) return rc;
    return device_call("instances_sample_device", A, d_xyz, d_out, (hipStream_t)stream, sample_launch(A, n));
}
SDFHIP_ABI_CATCH(sdfhip_instances_sample_device)

extern "C" int sdfhip_instances_raycast(const sdfhip_instance *instances, uint32_t n_instances, const sdfhip_instances_options *opt,
                                        const sdfhip_ray *rays, uint32_t n, float margin, float limit, sdfhip_part_hit *out)
try {
    Assembly A;
    if (const int rc = check_call("instances_raycast", instances, n_instances, opt, A)) return rc;
    if (const int rc = check_march("instances_raycast", margin, limit)) return rc;
    if (n == 0) return SDFHIP_OK;
    if (!rays || !out) return fail(SDFHIP_ERR_ARG, "instances_raycast: null argument");
    if (const int rc = read_table("instances_raycast", instances, n_instances, A)) return rc;
    return host_call("instances_raycast", A, rays, (size_t)n * sizeof(sdfhip_ray), out, (size_t)n * sizeof(sdfhip_part_hit),
                     march_launch<false>(A, n, march_info(margin, limit)));
}
SDFHIP_ABI_CATCH(sdfhip_instances_raycast)

extern "C" int sdfhip_instances_raycast_device(const sdfhip_instance *instances, uint32_t n_instances, const sdfhip_instances_options *opt,
                                               const sdfhip_ray *d_rays, uint32_t n, float margin, float limit, sdfhip_part_hit *d_out,
                                               void *stream)
try {
    Assembly A;
    if (const int rc = check_call("instances_raycast_device", instances, n_instances, opt, A)) return rc;
    if (const int rc = check_march("instances_raycast_device", margin, limit)) return rc;
    if (n == 0) return SDFHIP_OK;
    if (!d_rays || !d_out) return fail(SDFHIP_ERR_ARG, "instances_raycast_device: null argument");
    if (const int rc = read_table("instances_raycast_device", instances, n_instances, A)) return rc;
    return device_call("instances_raycast_device", A, d_rays, d_out, (hipStream_t)stream, march_launch<false>(A, n, march_info(margin, limit)));
}
SDFHIP_ABI_CATCH(sdfhip_instances_raycast_device)

extern "C" int sdfhip_instances_pick(const sdfhip_instance *instances, uint32_t n_instances, const sdfhip_instances_options *opt,
                                     const sdfhip_info *info, const uint32_t *pixels_xy, uint32_t n, sdfhip_part_hit *out)
try {
    Assembly A;
    if (const int rc = check_call("instances_pick", instances, n_instances, opt, A)) return rc;
    if (!info) return fail(SDFHIP_ERR_ARG, "instances_pick: null info");
    if (const int rc = check_march("instances_pick", info->margin, info->limit)) return rc;
    if (n == 0) return SDFHIP_OK;
    if (!pixels_xy || !out) return fail(SDFHIP_ERR_ARG, "instances_pick: null argument");
    if (const int rc = read_table("instances_pick", instances, n_instances, A)) return rc;
    FrameInfo I;
    unpack_camera(info, I);
    return host_call("instances_pick", A, pixels_xy, (size_t)n * 8, out, (size_t)n * sizeof(sdfhip_part_hit), march_launch<true>(A, n, I));
}
SDFHIP_ABI_CATCH(sdfhip_instances_pick)

extern "C" int sdfhip_instances_render(const sdfhip_instance *instances, uint32_t n_instances, const sdfhip_instances_options *opt,
                                       const sdfhip_info *info, uint32_t width, uint32_t height, float *rgba)
try {
    Assembly A;
    if (const int rc = check_call("instances_render", instances, n_instances, opt, A)) return rc;
    if (!info) return fail(SDFHIP_ERR_ARG, "instances_render: null info");
    if (const int rc = check_march("instances_render", info->margin, info->limit)) return rc;
    if (const int rc = check_frame("instances_render", width, height)) return rc;
    if (width == 0 || height == 0) return SDFHIP_OK;
    if (!rgba) return fail(SDFHIP_ERR_ARG, "instances_render: null argument");
    if (const int rc = read_table("instances_render", instances, n_instances, A)) return rc;
    FrameInfo I;
    unpack_camera(info, I);
    return host_call("instances_render", A, nullptr, 0, rgba, (size_t)width * height * 16, render_launch(A, I, width, height));
}
SDFHIP_ABI_CATCH(sdfhip_instances_render)

extern "C" int sdfhip_instances_render_device(const sdfhip_instance *instances, uint32_t n_instances, const sdfhip_instances_options *opt,
                                              const sdfhip_info *info, uint32_t width, uint32_t height, float *d_rgba, void *stream)
try {
    Assembly A;
    if (const int rc = check_call("instances_render_device", instances, n_instances, opt, A)) return rc;
    if (!info) return fail(SDFHIP_ERR_ARG, "instances_render_device: null info");
    if (const int rc = check_march("instances_render_device", info->margin, info->limit)) return rc;
    if (const int rc = check_frame("instances_render_device", width, height)) return rc;
    if (width == 0 || height == 0) return SDFHIP_OK;
    if (!d_rgba) return fail(SDFHIP_ERR_ARG, "instances_render_device: null argument");
    if (const int rc = read_table("instances_render_device", instances, n_instances, A)) return rc;
    FrameInfo I;
    unpack_camera(info, I);
    return device_call("instances_render_device", A, nullptr, d_rgba, (hipStream_t)stream, render_launch(A, I, width, height));
}
SDFHIP_ABI_CATCH(sdfhip_instances_render_device)
