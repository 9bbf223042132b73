// The host side that only the callers of the exact distance share: distance.hip (sdfhip_scene_distance, sdfhip_scene_offset) and
// blend.hip (sdfhip_scene_blend).  What they refuse of a handle and of a level, and the "surface below" bitmap's launch.  Everything
// here is inline; k_dist_mark is distance_kernels.h's static one.
#pragma once
#include "distance_kernels.h"
#include "level_build.h"      // Source, LEVEL_MAX_WORKGROUPS

namespace sdfhip {
namespace levels {

// sdfhip_scene_mesh's refusal: the surface is its triangles
inline int check_source(const char *what, const Source &src)
{
    if (!src.stack_ok || src.depth > (uint32_t)MESH_MAX_DEPTH)
        return fail(SDFHIP_ERR_BAD_TREE, "%s: the tree is not consistent (or deeper than %d levels): it has no mesh, so no surface to measure from", what,
                    MESH_MAX_DEPTH);
    if (src.device < 0 || src.device >= MAX_DEVICES) return fail(SDFHIP_ERR_ARG, "%s: device %d", what, src.device);
    return SDFHIP_OK;
}

inline size_t bitmap_words(uint32_t n) { return ((size_t)n + 31) / 32 + 1; }     // (+ 1: sibling_bits reads one word past a block's first)

// (a) on `st`: the bitmap zeroed and marked
inline int launch_mark(const Source &src, int32_t level, uint32_t *below, hipStream_t st)
{
    HIP_TRY(hipMemsetAsync(below, 0, bitmap_words(src.Q.n_nodes) * sizeof(uint32_t), st));
    hipLaunchKernelGGL(k_dist_mark, grid_stride_blocks(src.Q.n_nodes, LEVEL_MAX_WORKGROUPS), dim3(DIST_THREADS), 0, st, src.Q.nodes, src.Q.n_nodes, (int)level, below);
    HIP_TRY(hipGetLastError());
    return SDFHIP_OK;
}

}  // namespace levels
}  // namespace sdfhip
