// libsdfhip.so, placement: sdfhip_scene_place -- a resident scene rotated, scaled and moved by resampling it into a new tree, the
// result a new handle.
//
// Replaces: nothing in the reference's code; a tree there is immutable once built and sits where its builder put it.
//
// The rule, pinned (include/sdfhip.h; fp32, each operation rounded on its own in the order written):
//   inverse map      d = p - t, inv = 1.0f / s, q_a = ((R[0][a] d_0 + R[1][a] d_1) + R[2][a] d_2) * inv
//   value            qc = min(max(q, 0), 1), e = q - qc, D = sdfhip_scene_sample's distance at qc,
//                    value(p) = (D + sqrtf((e_0 e_0 + e_1 e_1) + e_2 e_2)) * s
//   tree             sdfhip_trimesh_build's construct rule with this value: byte = FromFloat(value(corner), S), a node splits iff
//                    fabsf(value(centre)) < 2 S && d < depth
//   node order       breadth first: a level's blocks in ascending index of their parents, child i at block + i
//
// The passes, per level from the root (level_build.h's build_levels, which the offset and the blend run too).  A level's blocks of
// eight siblings carry their parent's integer coordinates; the result's arrays grow as the levels arrive:
//   k_place_level      a wave per block, a lane per point of its lattice: the level's bytes and its split bitmap (place_kernels.h:
//                      level_kernels.h's level_body on the placement's value)
//   k_rank_scan_*      the splits' ranks: the shared bitmap prefix (scan_device.h), its total the next level's blocks (one host
//                      synchronisation per level: the count sizes the next level's memory and launches)
//   k_level_emit       eight lanes per splitting node: the links, appended behind the level, and the next level's blocks
// Then the arrays go to scene_from_arrays (grids, fused records) as the edit's, the prune's and the combination's do.
#include "place_kernels.h"
#include "level_build.h"      // host_support.h; Source, with_cursor, build_levels
#include "abi_guard.h"

#include <algorithm>
#include <chrono>
#include <cmath>

using namespace sdfhip;
using namespace sdfhip::levels;

static_assert(sizeof(sdfhip_placement) == 60 && sizeof(sdfhip_place_stats) == 40, "the placement records of include/sdfhip.h");

namespace {

// what the header refuses of a placement, before any device call
int check_placement(const sdfhip_placement *pl)
{
    if (const int rc = check_options_size("scene_place", pl, sizeof(sdfhip_placement), "size = sizeof(sdfhip_placement)")) return rc;
    if (const int rc = check_similarity("scene_place", pl->rotation, pl->scale, pl->translation)) return rc;
    if (pl->depth < -1 || pl->depth > TREE_MAX_DEPTH)
        return fail(SDFHIP_ERR_ARG, "scene_place: depth %d is neither -1 nor 0..%d", pl->depth, TREE_MAX_DEPTH);
    return SDFHIP_OK;
}

}  // namespace

extern "C" int sdfhip_scene_place(sdfhip_scene *scene, const sdfhip_placement *pl, sdfhip_scene **out, sdfhip_octdata *host_out,
                                  sdfhip_place_stats *stats)
try {
    const auto t0 = std::chrono::steady_clock::now();
    if (out) *out = nullptr;
    if (!pl) return fail(SDFHIP_ERR_ARG, "scene_place: null placement");
    if (!out && !host_out) return fail(SDFHIP_ERR_ARG, "scene_place: both outputs are null");
    if (const int rc = check_placement(pl)) return rc;
    if (!scene) return fail(SDFHIP_ERR_ARG, "scene_place: null scene");
    // (the placement resamples the field, not a surface: it takes whatever tree the sampler takes, and refuses only a depth it
    // cannot take over)
    const Source src = read_source(scene);
    if (pl->depth < 0 && src.depth > (uint32_t)TREE_MAX_DEPTH)
        return fail(SDFHIP_ERR_BAD_TREE, "scene_place: the source is not a consistent tree of at most %d levels, so it has no depth to take: give one",
                    TREE_MAX_DEPTH);
    const int depth = pl->depth < 0 ? (int)src.depth : pl->depth;
    PlaceMap M;
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) M.r[i][j] = pl->rotation[i][j];
    M.s = pl->scale; M.inv = 1.0f / pl->scale;
    M.tx = pl->translation[0]; M.ty = pl->translation[1]; M.tz = pl->translation[2];

    CallFrame<2> call("scene_place", src.device, "SDFHIP_PLACE_FAIL_ALLOC", t0);
    LevelBuild R;
    if (const int rc = call.run("the source is untouched", [&](hipStream_t st) -> int {
        const auto level = [&](const LevelBlock *blocks, uint32_t nblocks, uint32_t nchild, float S, int may_split, uint2 *V, uint8_t *split) {
            with_cursor(src.form, [&](auto c) {
                hipLaunchKernelGGL((k_place_level<typename decltype(c)::type>), grid_stride_blocks(64ull * nblocks, LEVEL_MAX_WORKGROUPS), dim3(LEVEL_THREADS), 0, st,
                                   src.Q, M, blocks, nblocks, nchild, S, may_split, V, split);
            });
        };
        // (nothing is allocated before the loop's own arrays; kernel_ms starts once the first of them are there: ev[0])
        if (const int rc = build_levels(call.what, call.bufs, st, src.Q.n_nodes, depth, level, R, call.cs.ev[0])) return rc;
        HIP_TRY(hipEventRecord(call.cs.ev[1], st));
        HIP_TRY(hipStreamSynchronize(st));
        return SDFHIP_OK;
    })) return rc;

    float kernel_ms = 0.0f, scene_ms = 0.0f;
    if (const int rc = call.elapsed(&kernel_ms, 0, 1)) return rc;
    if (const int rc = call.finish(R.dS, R.dV, R.n_out, (int)R.depth_out, out, host_out, &scene_ms)) return rc;
    if (stats) {
        stats->nodes_in = src.Q.n_nodes; stats->nodes_out = R.n_out; stats->depth_out = R.depth_out; stats->levels = R.depth_out + 1;
        stats->samples = R.points;
        stats->kernel_ms = kernel_ms; stats->scene_ms = scene_ms;
        stats->total_ms = call.total_ms();
        stats->pad_ = 0;
    }
    return SDFHIP_OK;
}
SDFHIP_ABI_CATCH(sdfhip_scene_place)
