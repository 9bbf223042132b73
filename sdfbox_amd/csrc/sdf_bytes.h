// The byte codec of a node's corner values, shared by the point-cloud builder (k_emit) and the space-carving edit (edit_kernels.h).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace sdfhip {

// FromFloat, SdfGen/dllmain.cpp:192-196: a corner distance of a node of edge `scale` -> its byte
__device__ __forceinline__ uint32_t from_float(float v, float scale)
{
    const float normd = v / 2 / scale;
    const float sat = fminf(fmaxf(normd + 0.25f, 0.0f), 1.0f);
    return (uint32_t)floorf(sat * 255);
}

// ... and back, as the shader reads it (o_sample_at's formula; the texture's unorm8 is bit-identical to b / 255.0f)
__device__ __forceinline__ float to_float(uint32_t b, float scale)
{
    return (((float)b / 255.0f) - 0.25f) * scale * 2.0f;
}

}  // namespace sdfhip
