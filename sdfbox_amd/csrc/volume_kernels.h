// Volumes in and out (gfx950): a dense lattice of distances as a tree's value -- the fourth client of level_kernels.h's level_body --
// and a resident tree read back on a lattice.  The lattice, the construct rule, the emit and the node order are level_kernels.h's; the
// host's loop is level_build.h's.
//
// The arithmetic is the contract of include/sdfhip.h (sdfhip_volume_build, sdfhip_scene_volume) and DESIGN.md section 8 (N15): fp32,
// each operation rounded on its own, in the order written (-ffp-contract=off); tests/volume_restatement.py restates it with numpy.
// The out direction's distance is what k_query_sample reads (find_fresh + sample_after_find, raymarch_device.h, untouched).
#pragma once
#include "query_kernels.h"   // QueryScene, grid_of; raymarch_device.h: the cursors, find_fresh, sample_after_find
#include "level_kernels.h"   // LevelBlock, level_body
#include <hip/hip_fp16.h>

namespace sdfhip {

constexpr int VOLUME_THREADS = 256;

// sdfhip_volume as the kernels use it: inv = 1.0f / spacing (one IEEE division, on the host).  nx * ny * nz <= 2^31, so an element's
// index fits 32 bits.
struct VolumeGrid {
    uint32_t nx, ny, nz;
    float ox, oy, oz;
    float spacing, inv, scale;
};

// a sample as float: the F16 conversion is exact
__device__ __forceinline__ float volume_sample(const float *g, uint32_t i) { return g[i]; }
__device__ __forceinline__ float volume_sample(const __half *g, uint32_t i) { return __half2float(g[i]); }

// finite <=> the exponent field is not all ones
__device__ __forceinline__ bool volume_finite(const float *g, uint32_t i) { return (__float_as_uint(g[i]) & 0x7F800000u) != 0x7F800000u; }
__device__ __forceinline__ bool volume_finite(const __half *g, uint32_t i)
{
    return (reinterpret_cast<const uint16_t *>(g)[i] & 0x7C00u) != 0x7C00u;
}

// One axis of the rule: the lattice coordinate g of p, clamped to the lattice; the cell i and the weight f in it; e, how far p lies
// outside along this axis.  gc lies in [0, n - 1] whatever the arguments are (fmaxf / fminf take a NaN to 0), so i and i + 1 are
// samples of the grid: i <= n - 2, and on the last plane i = n - 2 with f = 1.
__device__ __forceinline__ void volume_axis(float p, float o, float inv, float spacing, uint32_t n, uint32_t &i, float &f, float &e)
{
    const float g = (p - o) * inv;
    const float gc = __builtin_fminf(__builtin_fmaxf(g, 0.0f), (float)(n - 1u));
    e = (g - gc) * spacing;
    i = min((uint32_t)(int)gc, n - 2u);
    f = gc - (float)i;
}

// u at f = 0 and v at f = 1, exactly (u * 1 + v * 0: the samples are finite)
__device__ __forceinline__ float volume_lerp(float u, float v, float f) { return u * (1.0f - f) + v * f; }

// value(p) of the rule: the trilinear interpolant of the eight samples round p -- four x-adjacent pairs -- times value_scale,
// continued outside the grid's box at slope 1 from the nearest point of the box.  Inside the box e is 0 and the value is D * scale
// bit for bit (x + 0 = x, sqrtf(0) = 0).
template <class T>
__device__ __forceinline__ float volume_value(const T *__restrict__ grid, const VolumeGrid &G, float px, float py, float pz)
{
    uint32_t i, j, k;
    float fx, fy, fz, ex, ey, ez;
    volume_axis(px, G.ox, G.inv, G.spacing, G.nx, i, fx, ex);
    volume_axis(py, G.oy, G.inv, G.spacing, G.ny, j, fy, ey);
    volume_axis(pz, G.oz, G.inv, G.spacing, G.nz, k, fz, ez);
    const uint32_t row = G.nx, slab = G.nx * G.ny;
    const uint32_t b00 = (k * G.ny + j) * G.nx + i, b10 = b00 + row, b01 = b00 + slab, b11 = b01 + row;
    const float c00 = volume_lerp(volume_sample(grid, b00), volume_sample(grid, b00 + 1u), fx);
    const float c10 = volume_lerp(volume_sample(grid, b10), volume_sample(grid, b10 + 1u), fx);
    const float c01 = volume_lerp(volume_sample(grid, b01), volume_sample(grid, b01 + 1u), fx);
    const float c11 = volume_lerp(volume_sample(grid, b11), volume_sample(grid, b11 + 1u), fx);
    const float c0 = volume_lerp(c00, c10, fy), c1 = volume_lerp(c01, c11, fy);
    const float D = volume_lerp(c0, c1, fz);
    return D * G.scale + sqrtf((ex * ex + ey * ey) + ez * ez);
}

// volume_value as level_body takes it: no surface is searched, so there is no stack and nothing to count
template <class T> struct VolumeValue {
    static constexpr int SOURCES = 0;
    const T *grid;
    VolumeGrid G;
    __device__ __forceinline__ float operator()(float px, float py, float pz, uint2 *, uint32_t *) const
    {
        return volume_value<T>(grid, G, px, py, pz);
    }
};

template <class T>
__global__ __launch_bounds__(LEVEL_THREADS) void k_volume_level(const T *__restrict__ grid, VolumeGrid G, const LevelBlock *__restrict__ blocks,
                                                                uint32_t nblocks, uint32_t nchild, float S, int may_split,
                                                                uint2 *__restrict__ V, uint8_t *__restrict__ split)
{
    level_body(VolumeValue<T>{grid, G}, blocks, nblocks, nchild, S, may_split, V, split, nullptr);
}

// The grid's non-finite samples, counted: grid-stride, a lane's own count, the wave's by shuffles, the workgroup's through LDS, one
// integer atomicAdd per workgroup that saw any.  total <= 2^31 and the grid's stride is below 2^20 threads, so the index stays in
// 32 bits.
template <class T>
__global__ __launch_bounds__(VOLUME_THREADS) void k_volume_check(const T *__restrict__ grid, uint32_t total, uint32_t *__restrict__ bad)
{
    __shared__ uint32_t per_wave[VOLUME_THREADS / 64];
    uint32_t mine = 0u;
    for (uint32_t i = blockIdx.x * VOLUME_THREADS + threadIdx.x; i < total; i += gridDim.x * VOLUME_THREADS)
        mine += volume_finite(grid, i) ? 0u : 1u;
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) mine += (uint32_t)__shfl_xor((int)mine, o);
    if ((threadIdx.x & 63u) == 0u) per_wave[threadIdx.x >> 6] = mine;
    __syncthreads();
    if (threadIdx.x == 0u) {
        uint32_t sum = 0u;
#pragma unroll
        for (int w = 0; w < VOLUME_THREADS / 64; w++) sum += per_wave[w];
        if (sum) atomicAdd(bad, sum);
    }
}

__device__ __forceinline__ void volume_store(float *out, uint32_t i, float v) { out[i] = v; }
__device__ __forceinline__ void volume_store(__half *out, uint32_t i, float v) { out[i] = __float2half_rn(v); }

// The out direction: element (i, j, k) of the lattice L is the placement's value at the identity -- the scene's distance at the
// element's position clamped to the cube (what sdfhip_scene_sample returns there), continued outside the cube at slope 1.  A thread
// per element, x fastest: a wave's stores are contiguous and its look-ups are neighbours.  total = nx * ny * nz <= 2^31; the loop
// counts in 64 bits and an element's index fits 32.
template <class CursorT, class T>
__global__ __launch_bounds__(VOLUME_THREADS) void k_volume_out(QueryScene Q, VolumeGrid L, uint32_t total, T *__restrict__ out)
{
    const uint32_t slab = L.nx * L.ny;
    for (uint64_t at = (uint64_t)blockIdx.x * VOLUME_THREADS + threadIdx.x; at < total; at += (uint64_t)gridDim.x * VOLUME_THREADS) {
        const uint32_t e = (uint32_t)at;
        const uint32_t k = e / slab, r = e - k * slab, j = r / L.nx, i = r - j * L.nx;
        const float px = L.ox + (float)i * L.spacing, py = L.oy + (float)j * L.spacing, pz = L.oz + (float)k * L.spacing;
        const float cx = __builtin_fminf(__builtin_fmaxf(px, 0.0f), 1.0f);
        const float cy = __builtin_fminf(__builtin_fmaxf(py, 0.0f), 1.0f);
        const float cz = __builtin_fminf(__builtin_fmaxf(pz, 0.0f), 1.0f);
        const float ex = px - cx, ey = py - cy, ez = pz - cz;
        CursorT c;
        c.loads = 0;
        c.reset(Q.nodes[0]);
        typename CursorT::Pos u;
        find_fresh(c, Q.nodes, grid_of(Q), Q.n_nodes, nullptr, 0u, cx, cy, cz, u);
        const float D = sample_after_find(c, u, cx, cy, cz);
        volume_store(out, e, D + sqrtf((ex * ex + ey * ey) + ez * ez));
    }
}

}  // namespace sdfhip
