// libsdfhip.so, volumes in and out: sdfhip_volume_build[_device] -- a dense lattice of distances (a neural SDF on a grid, a TSDF, a
// level set, a distance transform) as a new scene -- and sdfhip_scene_volume[_device] -- a resident scene read back on a lattice.
//
// Replaces: nothing in the reference's code; its builder takes a point cloud and its tree only ever becomes pixels.
//
// The rule, pinned (include/sdfhip.h; fp32, each operation rounded on its own in the order written):
//   build, per axis  g = (p - origin) * inv (inv = 1.0f / spacing), gc = min(max(g, 0), n - 1), e = (g - gc) * spacing,
//                    i = min((int)gc, n - 2), f = gc - (float)i
//   build, value     D = the eight samples at i .. i + 1 under lerp(u, v, f) = u * (1.0f - f) + v * f, four times along x, two along
//                    y, one along z; value(p) = D * value_scale + sqrtf((e_0 e_0 + e_1 e_1) + e_2 e_2)
//   tree             sdfhip_scene_place's, word for word, with this value (level_kernels.h's level_body, level_build.h's build_levels)
//   out              p = origin + (float)i * spacing per axis, qc = min(max(p, 0), 1), e = p - qc, D = sdfhip_scene_sample's distance
//                    at qc, element = D + sqrtf((e_0 e_0 + e_1 e_1) + e_2 e_2): the placement's value at the identity
//
// The passes of a build: k_volume_check (the grid's non-finite samples, counted: any refuses the call), then per level k_volume_level,
// the shared bitmap scan and k_level_emit, then scene_from_arrays as the placement's.  The out direction is one launch of k_volume_out,
// a thread per element, with the cursor the placement would take for the scene.
#include "volume_kernels.h"
#include "level_build.h"      // host_support.h; Source, with_cursor, build_levels
#include "abi_guard.h"

#include <algorithm>
#include <chrono>
#include <cmath>

using namespace sdfhip;
using namespace sdfhip::levels;

static_assert(sizeof(sdfhip_volume) == 44 && sizeof(sdfhip_volume_stats) == 40, "the volume records of include/sdfhip.h");

namespace {

constexpr uint32_t VOLUME_MAX_SIDE = 4096;
constexpr uint64_t VOLUME_MAX_ELEMENTS = 1ull << 31;
constexpr uint32_t VOLUME_OUT_MAX_WORKGROUPS = 1u << 16;    // k_volume_out strides beyond 2^24 threads

// what the header refuses of a lattice, before any device call.  build: the record describes a grid to build from (n_a >= 2, a
// scale and a depth); else one to fill (n_a >= 1, scale and depth 0).
int check_volume(const char *what, const sdfhip_volume *vol, bool build, uint64_t *total)
{
    if (const int rc = check_options_size(what, vol, sizeof(sdfhip_volume), "size = sizeof(sdfhip_volume)")) return rc;
    const uint32_t least = build ? 2u : 1u;
    for (int a = 0; a < 3; a++)
        if (vol->n[a] < least || vol->n[a] > VOLUME_MAX_SIDE)
            return fail(SDFHIP_ERR_ARG, "%s: n[%d] = %u outside %u..%u", what, a, vol->n[a], least, VOLUME_MAX_SIDE);
    *total = (uint64_t)vol->n[0] * vol->n[1] * vol->n[2];
    if (*total > VOLUME_MAX_ELEMENTS)
        return fail(SDFHIP_ERR_ARG, "%s: %u x %u x %u samples are more than 2^31", what, vol->n[0], vol->n[1], vol->n[2]);
    if (!std::isfinite(vol->spacing) || !(vol->spacing > 0.0f))
        return fail(SDFHIP_ERR_ARG, "%s: spacing %g is not a finite number above 0", what, (double)vol->spacing);
    for (int a = 0; a < 3; a++)
        if (!std::isfinite(vol->origin[a])) return fail(SDFHIP_ERR_ARG, "%s: the origin must be finite", what);
    if (vol->dtype != SDFHIP_VOLUME_F32 && vol->dtype != SDFHIP_VOLUME_F16)
        return fail(SDFHIP_ERR_ARG, "%s: dtype %d is neither SDFHIP_VOLUME_F32 nor SDFHIP_VOLUME_F16", what, vol->dtype);
    if (build) {
        if (!std::isfinite(vol->value_scale) || vol->value_scale == 0.0f)
            return fail(SDFHIP_ERR_ARG, "%s: value_scale %g is not a finite number other than 0", what, (double)vol->value_scale);
        if (vol->depth < 0 || vol->depth > TREE_MAX_DEPTH)
            return fail(SDFHIP_ERR_ARG, "%s: depth %d outside 0..%d", what, vol->depth, TREE_MAX_DEPTH);
    } else {
        if (vol->value_scale != 0.0f || vol->depth != 0)
            return fail(SDFHIP_ERR_ARG, "%s: value_scale and depth describe a build: both must be 0 here", what);
    }
    return SDFHIP_OK;
}

VolumeGrid grid_of_record(const sdfhip_volume *vol)
{
    return VolumeGrid{vol->n[0], vol->n[1], vol->n[2], vol->origin[0], vol->origin[1], vol->origin[2],
                      vol->spacing, 1.0f / vol->spacing, vol->value_scale};
}

// The build on the samples' type.  grid: host memory (staged) or, with on_device, memory of `device` that is complete.
template <class T>
int build_as(const char *what, int device, const void *grid, bool on_device, const sdfhip_volume *vol, uint64_t total, sdfhip_scene **out,
             sdfhip_octdata *host_out, sdfhip_volume_stats *stats, std::chrono::steady_clock::time_point t0)
{
    const VolumeGrid G = grid_of_record(vol);
    CallFrame<4> call(what, device, "SDFHIP_VOLUME_FAIL_ALLOC", t0);
    DeviceBuffers &bufs = call.bufs;
    const CallStream<4> &cs = call.cs;

    LevelBuild R;
    if (const int rc = call.run("the grid is untouched", [&](hipStream_t st) -> int {
        const T *d_grid = static_cast<const T *>(grid);
        if (!on_device) {
            T *staged = bufs.get<T>((size_t)total);
            HIP_TRY(hipMemcpyAsync(staged, grid, (size_t)total * sizeof(T), hipMemcpyHostToDevice, st));
            d_grid = staged;
        }
        // the finite check: a NaN or an infinity among the samples would reach the bytes of every node round it
        uint32_t *d_bad = bufs.get<uint32_t>(1);
        HIP_TRY(hipMemsetAsync(d_bad, 0, sizeof(uint32_t), st));
        HIP_TRY(hipEventRecord(cs.ev[0], st));
        hipLaunchKernelGGL((k_volume_check<T>), grid_stride_blocks(total, LEVEL_MAX_WORKGROUPS), dim3(VOLUME_THREADS), 0, st, d_grid, (uint32_t)total, d_bad);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipEventRecord(cs.ev[1], st));
        uint32_t bad = 0;
        HIP_TRY(hipMemcpyAsync(&bad, d_bad, sizeof bad, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        if (bad) return fail(SDFHIP_ERR_ARG, "%s: %u of the grid's %llu samples are not finite", what, bad, (unsigned long long)total);

        const auto level = [&](const LevelBlock *blocks, uint32_t nblocks, uint32_t nchild, float S, int may_split, uint2 *V, uint8_t *split) {
            hipLaunchKernelGGL((k_volume_level<T>), grid_stride_blocks(64ull * nblocks, LEVEL_MAX_WORKGROUPS), dim3(LEVEL_THREADS), 0, st,
                               d_grid, G, blocks, nblocks, nchild, S, may_split, V, split);
        };
        // The arrays' starting room, from the grid: a surface that crosses the grid's box cuts about as many of its cells as a face of
        // the box has, per level a quarter of the level below; eight nodes to a cut cell and the three faces' sizes cover the levels'
        // sum for a surface of a few sheets.  The arrays grow as they do for every builder when that is not enough.
        const uint64_t faces = (uint64_t)G.nx * G.ny + (uint64_t)G.ny * G.nz + (uint64_t)G.nz * G.nx;
        const uint32_t start = (uint32_t)std::min<uint64_t>(8ull * faces, 0x7FFFFFFFull);
        if (const int rc = build_levels(what, bufs, st, start, vol->depth, level, R, cs.ev[2])) return rc;
        HIP_TRY(hipEventRecord(cs.ev[3], st));
        HIP_TRY(hipStreamSynchronize(st));
        return SDFHIP_OK;
    })) return rc;

    float check_ms = 0.0f, kernel_ms = 0.0f, scene_ms = 0.0f;
    if (const int rc = call.elapsed(&check_ms, 0, 1)) return rc;
    if (const int rc = call.elapsed(&kernel_ms, 2, 3)) return rc;
    if (const int rc = call.finish(R.dS, R.dV, R.n_out, (int)R.depth_out, out, host_out, &scene_ms)) return rc;
    if (stats) {
        stats->nodes_out = R.n_out; stats->depth_out = R.depth_out; stats->levels = R.depth_out + 1; stats->pad_ = 0;
        stats->samples = R.points;
        stats->check_ms = check_ms; stats->kernel_ms = kernel_ms; stats->scene_ms = scene_ms;
        stats->total_ms = call.total_ms();
    }
    return SDFHIP_OK;
}

int build(const char *what, int device, const void *grid, bool on_device, const sdfhip_volume *vol, sdfhip_scene **out, sdfhip_octdata *host_out,
          sdfhip_volume_stats *stats)
{
    const auto t0 = std::chrono::steady_clock::now();
    if (out) *out = nullptr;
    if (host_out) { host_out->length = 0; host_out->structs = nullptr; host_out->values = nullptr; }
    if (!vol) return fail(SDFHIP_ERR_ARG, "%s: null volume record", what);
    if (!grid) return fail(SDFHIP_ERR_ARG, "%s: null grid", what);
    if (!out && !host_out) return fail(SDFHIP_ERR_ARG, "%s: both outputs are null", what);
    uint64_t total = 0;
    if (const int rc = check_volume(what, vol, true, &total)) return rc;

    int ndev = 0;
    HIP_TRY(hipGetDeviceCount(&ndev));
    if (device < 0 || device >= ndev) return fail(SDFHIP_ERR_DEVICE, "%s: device %d of %d does not exist", what, device, ndev);
    if (vol->dtype == SDFHIP_VOLUME_F16) return build_as<__half>(what, device, grid, on_device, vol, total, out, host_out, stats, t0);
    return build_as<float>(what, device, grid, on_device, vol, total, out, host_out, stats, t0);
}

// k_volume_out on `st`, with the cursor of the scene's form and the output's type
void launch_out(const Source &src, const VolumeGrid &L, uint64_t total, int32_t dtype, void *d_out, hipStream_t st)
{
    const dim3 blocks = grid_stride_blocks(total, VOLUME_OUT_MAX_WORKGROUPS);
    with_cursor(src.form, [&](auto c) {
        using CursorT = typename decltype(c)::type;
        if (dtype == SDFHIP_VOLUME_F16)
            hipLaunchKernelGGL((k_volume_out<CursorT, __half>), blocks, dim3(VOLUME_THREADS), 0, st, src.Q, L, (uint32_t)total, static_cast<__half *>(d_out));
        else
            hipLaunchKernelGGL((k_volume_out<CursorT, float>), blocks, dim3(VOLUME_THREADS), 0, st, src.Q, L, (uint32_t)total, static_cast<float *>(d_out));
    });
}

// what both out forms refuse, before any device call
int check_out(const char *what, sdfhip_scene *scene, const sdfhip_volume *lattice, const void *out, uint64_t *total)
{
    if (!lattice) return fail(SDFHIP_ERR_ARG, "%s: null lattice record", what);
    if (!out) return fail(SDFHIP_ERR_ARG, "%s: null output", what);
    if (const int rc = check_volume(what, lattice, false, total)) return rc;
    if (!scene) return fail(SDFHIP_ERR_ARG, "%s: null scene", what);
    return SDFHIP_OK;
}

}  // namespace

extern "C" int sdfhip_volume_build(int device, const void *grid, const sdfhip_volume *vol, sdfhip_scene **out, sdfhip_octdata *host_out,
                                   sdfhip_volume_stats *stats)
try {
    return build("volume_build", device, grid, false, vol, out, host_out, stats);
}
SDFHIP_ABI_CATCH(sdfhip_volume_build)

extern "C" int sdfhip_volume_build_device(int device, const void *d_grid, const sdfhip_volume *vol, sdfhip_scene **out, sdfhip_octdata *host_out,
                                          sdfhip_volume_stats *stats)
try {
    return build("volume_build_device", device, d_grid, true, vol, out, host_out, stats);
}
SDFHIP_ABI_CATCH(sdfhip_volume_build_device)

extern "C" int sdfhip_scene_volume_device(sdfhip_scene *scene, const sdfhip_volume *lattice, void *d_out, void *stream)
try {
    uint64_t total = 0;
    if (const int rc = check_out("scene_volume_device", scene, lattice, d_out, &total)) return rc;
    const Source src = read_source(scene);
    DeviceGuard g(src.device);
    if (!g.ok) return fail(SDFHIP_ERR_DEVICE, "scene_volume_device: hipSetDevice(%d) failed", src.device);
    // (the scene's records and grids are fixed at upload and only ever read: the launch needs no lock)
    launch_out(src, grid_of_record(lattice), total, lattice->dtype, d_out, (hipStream_t)stream);
    HIP_TRY(hipGetLastError());
    return SDFHIP_OK;
}
SDFHIP_ABI_CATCH(sdfhip_scene_volume_device)

extern "C" int sdfhip_scene_volume(sdfhip_scene *scene, const sdfhip_volume *lattice, void *out)
try {
    uint64_t total = 0;
    if (const int rc = check_out("scene_volume", scene, lattice, out, &total)) return rc;
    const Source src = read_source(scene);
    DeviceGuard g(src.device);
    if (!g.ok) return fail(SDFHIP_ERR_DEVICE, "scene_volume: hipSetDevice(%d) failed", src.device);
    const size_t bytes = (size_t)total * (lattice->dtype == SDFHIP_VOLUME_F16 ? 2 : 4);
    DeviceBuffers bufs("SDFHIP_VOLUME_FAIL_ALLOC");
    CallStream<1> cs;                       // (after `bufs`: drained before the buffer is freed)
    if (const int rc = cs.open("")) return rc;
    try {
        uint8_t *d_out = bufs.get<uint8_t>(bytes);
        launch_out(src, grid_of_record(lattice), total, lattice->dtype, d_out, cs.st);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(out, d_out, bytes, hipMemcpyDeviceToHost, cs.st));
        HIP_TRY(hipStreamSynchronize(cs.st));
    } catch (const NoMem &) {
        return fail(SDFHIP_ERR_NOMEM, "scene_volume: out of device memory for %zu bytes (the scene is untouched)", bytes);
    }
    return SDFHIP_OK;
}
SDFHIP_ABI_CATCH(sdfhip_scene_volume)
