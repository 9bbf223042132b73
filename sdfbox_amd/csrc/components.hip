// libsdfhip.so, the components of a scene: sdfhip_scene_components[_device] -- the face-connected solids and voids of a resident scene
// on a cubic lattice, one integer record each and, if asked, every point's label (kernels: components_kernels.h).
//
// Replaces: nothing in the reference's code; its shader marches one immutable tree and never asks how many pieces it has.
//
// The rule, pinned (include/sdfhip.h): a point is inside iff sdfhip_scene_place's value at the identity is
// < 0; points that differ by 1 in one coordinate and share a phase are connected; a point's label is its component's lowest index.
//
// Per call: the options are checked, the scene is read under its lock (read_source), and on a stream of the call's own (CallFrame)
// k_comp_local looks every point up and labels each 4 x 4 x 4 block on its own, k_comp_merge joins the blocks across their faces
// (a concurrent union-find), k_comp_flatten gives every point its root and the root bitmap, the shared bitmap scan ranks the roots,
// and -- after the one host synchronisation, whose count sizes the record table -- k_comp_init and k_comp_records fill the table.
// Records, labels and counters come back in one copy each, after the last allocation: a call that runs out of memory has written
// nothing.  Nothing is built and nothing is kept on the handle.
//
// The passes up to and including k_comp_records are label_components below, which sdfhip_scene_select (select.hip) calls too, with the
// lattice's refusals (check_comp_lattice); components_host.h declares both.
#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Wunneeded-internal-declaration"
#include "components_kernels.h"
#include "level_build.h"      // host_support.h; Source, read_source, with_cursor (its k_level_emit is not launched here)
#pragma clang diagnostic pop
#include "abi_guard.h"

#include <chrono>
#include <cmath>
#include <cstring>

using namespace sdfhip;
using namespace sdfhip::levels;

static_assert(sizeof(sdfhip_components_options) == 28 && sizeof(sdfhip_component) == 64 && sizeof(sdfhip_components_stats) == 32,
              "the components' records of include/sdfhip.h");
static_assert(sizeof(sdfhip_component) == sizeof(Component) && offsetof(sdfhip_component, lo) == offsetof(Component, lo) &&
              offsetof(sdfhip_component, sum) == offsetof(Component, sum), "components_kernels.h restates the record");
static_assert(SDFHIP_COMPONENT_SOLID == COMP_SOLID, "components_kernels.h restates the header's flag");

namespace {

const char *const FAIL_ALLOC = "SDFHIP_COMPONENTS_FAIL_ALLOC";     // laboratory library: AllocFault
constexpr uint32_t RECORD_WAVES = 2048;                            // k_comp_records: 2 waves on each of the 1024 SIMDs

int check_call(const char *name, const sdfhip_scene *scene, const sdfhip_components_options *opt, const sdfhip_component *out, uint32_t capacity,
               const uint32_t *n_components, CompLattice &L)
{
    const float unit[3] = {0.0f, 0.0f, 0.0f};
    if (opt) {
        if (const int rc = check_options_size(name, opt, sizeof(sdfhip_components_options), "sdfhip_components_options_default sets the size")) return rc;
        if (opt->flags) return fail(SDFHIP_ERR_ARG, "%s: unknown flags %#x", name, opt->flags);
    }
    if (const int rc = check_comp_lattice(name, "depth", opt ? opt->depth : 6u, opt ? opt->origin : unit, opt ? opt->side : 1.0f, L)) return rc;
    if (!n_components) return fail(SDFHIP_ERR_ARG, "%s: null n_components", name);
    if (!out && capacity > 0) return fail(SDFHIP_ERR_ARG, "%s: null out with capacity %u", name, capacity);
    if (!scene) return fail(SDFHIP_ERR_ARG, "%s: null scene", name);
    return SDFHIP_OK;
}

// labels: host memory, or memory of the scene's device (on_device); either may be null
int components(const char *name, sdfhip_scene *scene, const sdfhip_components_options *opt, sdfhip_component *out, uint32_t capacity,
               uint32_t *n_components, uint32_t *labels, bool on_device, sdfhip_components_stats *stats)
{
    const auto t0 = std::chrono::steady_clock::now();
    CompLattice L;
    if (const int rc = check_call(name, scene, opt, out, capacity, n_components, L)) return rc;
    const Source src = read_source(scene);
    CompLabels C;
    CompStat slots[COMP_STAT_SLOTS];
    float kernel_ms = 0.0f;
    CallFrame<2> call(name, src.device, FAIL_ALLOC, t0);
    const int rc = call.run("nothing was written", [&](hipStream_t st) -> int {
        if (const int rc = label_components(call.bufs, st, src, L, call.cs.ev[0], C)) return rc;
        HIP_TRY(hipEventRecord(call.cs.ev[1], st));
        // (nothing is allocated from here on)
        const uint32_t kept = std::min(capacity, C.total);
        if (kept) HIP_TRY(hipMemcpyAsync(out, C.d_out, (size_t)kept * sizeof(Component), hipMemcpyDeviceToHost, st));
        if (labels) HIP_TRY(hipMemcpyAsync(labels, C.d_parent, (size_t)C.n * sizeof(uint32_t), on_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(slots, C.d_stats, sizeof slots, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        return call.elapsed(&kernel_ms, 0, 1);
    });
    if (rc != SDFHIP_OK) return rc;
    *n_components = C.total;
    if (stats) {
        memset(stats, 0, sizeof *stats);
        stats->points = C.n;
        stats->components = C.total;
        for (const CompStat &s : slots) { stats->inside += s.inside; stats->solids += s.solids; }
        stats->kernel_ms = kernel_ms;
        stats->total_ms = call.total_ms();
    }
    return SDFHIP_OK;
}

}  // namespace

// ---- what sdfhip_scene_select shares (components_host.h) --------------------------------------------------------------------------

int sdfhip::check_comp_lattice(const char *name, const char *field, uint32_t depth, const float *origin, float side, CompLattice &L)
{
    if (depth > SDFHIP_COMPONENTS_MAX_DEPTH)
        return fail(SDFHIP_ERR_ARG, "%s: %s %u outside 0..%d (the call keeps 4 bytes per lattice point: 512 MB at depth 9, 4 GB at depth 10)", name, field,
                    depth, (int)SDFHIP_COMPONENTS_MAX_DEPTH);
    if (!std::isfinite(origin[0]) || !std::isfinite(origin[1]) || !std::isfinite(origin[2]))
        return fail(SDFHIP_ERR_ARG, "%s: the origin (%g, %g, %g) is not finite", name, (double)origin[0], (double)origin[1], (double)origin[2]);
    if (!std::isfinite(side) || !(side > 0.0f)) return fail(SDFHIP_ERR_ARG, "%s: the side %g is not finite and above 0", name, (double)side);
    for (int a = 0; a < 3; a++)
        if (!std::isfinite(origin[a] + side))
            return fail(SDFHIP_ERR_ARG, "%s: the cube's far corner, origin + side = %g + %g, is not finite", name, (double)origin[a], (double)side);
    L.ox = origin[0]; L.oy = origin[1]; L.oz = origin[2];
    L.depth = depth;
    L.pitch = side * std::ldexp(1.0f, -(int)depth);
    L.n_blocks = 1u << (3u * (depth > 2u ? depth - 2u : 0u));
    return SDFHIP_OK;
}

int sdfhip::label_components(DeviceBuffers &bufs, hipStream_t st, const Source &src, const CompLattice &L, hipEvent_t started, CompLabels &C)
{
    const uint32_t n = 1u << (3u * L.depth), m = std::max(1u, n >> 5), nchunk = (m + 1023u) / 1024u;
    const uint32_t per = COMP_THREADS / 64, by_block = (L.n_blocks + per - 1u) / per, by_point = (n + COMP_THREADS - 1u) / COMP_THREADS;
    C.n = n; C.m = m; C.nchunk = nchunk;
    uint32_t *d_parent = C.d_parent = bufs.get<uint32_t>(n);
    unsigned long long *d_sign = C.d_sign = bufs.get<unsigned long long>(L.n_blocks);
    uint32_t *d_roots = C.d_roots = bufs.get<uint32_t>(m + 1u);
    uint32_t *d_pre = C.d_pre = bufs.get<uint32_t>(m);
    uint32_t *d_chunk = C.d_chunk = bufs.get<uint32_t>(nchunk + 1u);
    CompStat *d_stats = C.d_stats = bufs.get<CompStat>(COMP_STAT_SLOTS);
    HIP_TRY(hipMemsetAsync(d_stats, 0, sizeof(CompStat) * COMP_STAT_SLOTS, st));
    HIP_TRY(hipEventRecord(started, st));
    with_cursor(src.form, [&](auto c) {
        hipLaunchKernelGGL((k_comp_local<typename decltype(c)::type>), dim3(by_block), dim3(COMP_THREADS), 0, st, src.Q, L, d_parent, d_sign, d_stats);
    });
    HIP_TRY(hipGetLastError());
    if (L.n_blocks > 1u) hipLaunchKernelGGL(k_comp_merge, dim3(by_block), dim3(COMP_THREADS), 0, st, L, d_parent, d_sign);
    hipLaunchKernelGGL(k_comp_flatten, dim3(by_point), dim3(COMP_THREADS), 0, st, d_parent, n, d_roots);
    hipLaunchKernelGGL(k_rank_scan_words<CompRootWords>, dim3(nchunk), dim3(256), 0, st, CompRootWords{ d_roots }, m, d_pre, d_chunk);
    hipLaunchKernelGGL(k_rank_scan_chunks<true>, dim3(1), dim3(1024), 0, st, d_chunk, nchunk);
    HIP_TRY(hipGetLastError());
    // the one host synchronisation: the count sizes the record table
    uint32_t total = 0;
    HIP_TRY(hipMemcpyAsync(&total, d_chunk + nchunk, sizeof total, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    C.total = total;
    Component *d_out = C.d_out = bufs.get<Component>(total);
    hipLaunchKernelGGL(k_comp_init, dim3(by_point), dim3(COMP_THREADS), 0, st, L, n, d_roots, d_pre, d_chunk, d_sign, d_out, d_stats);
    // (a run of blocks per wave: at most RECORD_WAVES waves flush the outer void's share)
    const uint32_t run = (L.n_blocks + RECORD_WAVES - 1u) / RECORD_WAVES, waves = (L.n_blocks + run - 1u) / run;
    hipLaunchKernelGGL(k_comp_records, dim3((waves + per - 1u) / per), dim3(COMP_THREADS), 0, st, L, run, d_parent, d_roots, d_pre, d_chunk, d_out);
    HIP_TRY(hipGetLastError());
    return SDFHIP_OK;
}

extern "C" void sdfhip_components_options_default(sdfhip_components_options *opt)
try {
    if (!opt) { (void)fail(SDFHIP_ERR_ARG, "components_options_default: null argument"); return; }
    opt->size = (uint32_t)sizeof(sdfhip_components_options);
    opt->flags = 0u;
    opt->depth = 6u;
    opt->origin[0] = 0.0f; opt->origin[1] = 0.0f; opt->origin[2] = 0.0f;
    opt->side = 1.0f;
}
SDFHIP_ABI_CATCH_VOID(sdfhip_components_options_default)

extern "C" int sdfhip_scene_components(sdfhip_scene *scene, const sdfhip_components_options *opt, sdfhip_component *out, uint32_t capacity,
                                       uint32_t *n_components, uint32_t *labels, sdfhip_components_stats *stats)
try {
    return components("scene_components", scene, opt, out, capacity, n_components, labels, false, stats);
}
SDFHIP_ABI_CATCH(sdfhip_scene_components)

extern "C" int sdfhip_scene_components_device(sdfhip_scene *scene, const sdfhip_components_options *opt, sdfhip_component *out, uint32_t capacity,
                                              uint32_t *n_components, uint32_t *d_labels, sdfhip_components_stats *stats)
try {
    return components("scene_components_device", scene, opt, out, capacity, n_components, d_labels, true, stats);
}
SDFHIP_ABI_CATCH(sdfhip_scene_components_device)
