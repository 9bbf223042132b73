// The trilinear interpolation of a node's corner values, shared by the space-carving edit (edit_kernels.h: a new child's values
// before the brush) and the prune (prune_kernels.h: the bytes a block is compared with).  One definition, so the two cannot drift.
#pragma once
#include <hip/hip_runtime.h>

namespace sdfhip {

__device__ __forceinline__ float edit_lerp(float a, float b, float t) { return a + (b - a) * t; }

// trilinear interpolation of corner values c[x + 2y + 4z] at (tx, ty, tz): along x, then y, then z
__device__ __forceinline__ float trilerp(const float c[8], float tx, float ty, float tz)
{
    const float e00 = edit_lerp(c[0], c[1], tx), e10 = edit_lerp(c[2], c[3], tx);
    const float e01 = edit_lerp(c[4], c[5], tx), e11 = edit_lerp(c[6], c[7], tx);
    const float f0 = edit_lerp(e00, e10, ty), f1 = edit_lerp(e01, e11, ty);
    return edit_lerp(f0, f1, tz);
}

}  // namespace sdfhip
