// Point and ray queries on a resident scene (gfx950): k_query_sample (distance, cell and gradient at n points) and k_query_march
// (the primary march of Compute.hlsl:194-203 for n rays, or for n pixels of a camera block).  Host side, C ABI: query.hip.
//
// Replaces: nothing in the reference's code -- its only consumer of the tree is Compute.hlsl, whose find (:88-108), interpol_world
// (:54-58), gradient (:112-130), ray (:163-168) and first loop (:194-203) these kernels run for arbitrary points and rays instead of
// a frame's pixels.  The arithmetic is raymarch_device.h's, untouched: a query reads the bytes the shader would read.
//
// One lane per query, 256 lanes per workgroup.  Queries are incoherent -- no tile, no XCD label -- so a lane loads its record, walks
// and stores its answer; nothing is shared.  Two forms of each kernel:
//   grid     CursorFT: every find() is a lookup in the scene's full-depth grid (dense, or coarse level + fine blocks).  A grid cell
//            holds a leaf's level and bytes but not its index, so the index is resolved once per query, after the last lookup, by a
//            descent along the children links with the cell's own coordinates (node_of below: `level` loads, most of them of the
//            top levels every query shares);
//   generic  CursorG: the shader's own walk through parent and children links; the cursor carries the index.
// The march takes the grid form wherever the handle has such a grid, as the renderer's SDFHIP_KERNEL_AUTO does; sample, one lookup per
// point with the index wanted, is faster walking (query.hip's form_of has the figures).  Both forms give the same bytes
// (tests/test_gpu_query.py runs both on the same trees).
#pragma once
#include "raymarch_device.h"

namespace sdfhip {

constexpr int QUERY_THREADS = 256;
enum { QUERY_HIT = 0, QUERY_ESCAPED = 1, QUERY_EXHAUSTED = 2, QUERY_INVALID = 3 };    // SDFHIP_QUERY_* of include/sdfhip.h

// what a query kernel reads of the scene
struct QueryScene {
    const NodeRec *nodes;
    uint32_t n_nodes;
    const TopCell *top, *fine;
    int32_t top_level, fine_bits;
};
__device__ __forceinline__ GridRef grid_of(const QueryScene &Q) { return GridRef{Q.top, Q.fine, Q.top_level, Q.fine_bits, 0}; }

// The records leave once and are never read back by the kernel: non-temporal stores, as the frame's (frame_store,
// raymarch_kernels.h); NT = false keeps the plain store for the A/B.  A template parameter for the reason given there.
template <bool NT>
__device__ __forceinline__ void record_store(uint4 *p, const uint4 &v)
{
    typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
    if (NT) __builtin_nontemporal_store((u32x4){v.x, v.y, v.z, v.w}, reinterpret_cast<u32x4 *>(p));
    else *p = v;
}

// finite <=> the exponent field is not all ones
__device__ __forceinline__ bool finite3(float x, float y, float z)
{
    const uint32_t m = 0x7F800000u;
    return (__float_as_uint(x) & m) != m && (__float_as_uint(y) & m) != m && (__float_as_uint(z) & m) != m;
}

// The index of the node a cursor sits on.
__device__ __forceinline__ uint32_t node_of(const CursorG &c, const QueryScene &) { return c.index; }
// A grid cursor knows its cell's level and coordinates: the cell's node is where the descent from the root along those
// coordinates' octant bits arrives after `level` steps (k_top_grid / k_fine_blocks walked the same way to fill the cell).  The
// guards only bind on a tree the upload would have refused.
template <bool SPLIT>
__device__ __forceinline__ uint32_t node_of(const CursorFT<false, SPLIT> &c, const QueryScene &Q)
{
    if (c.ax == CursorFT<false, SPLIT>::ROOT_MARK) return 0u;          // never looked up: the root
    const int4 k = c.pack();                                            // coordinates in units of 2^-LM
    const int level = LM - (int)(c.s & 15u);
    uint32_t index = 0u;
    int32_t children = (int32_t)Q.nodes[0].y;
    for (int l = 0; l < level && children >= 0; l++) {
        const int sb = LM - 1 - l;
        index = (uint32_t)children + (((uint32_t)k.x >> sb & 1u) | (((uint32_t)k.y >> sb & 1u) << 1) | (((uint32_t)k.z >> sb & 1u) << 2));
        if (index >= Q.n_nodes) return 0u;
        children = (int32_t)Q.nodes[index].y;
    }
    return index;
}

// sample: for point i the distance the shader would read there (find from the root + interpol_world, == oracle_distance_at), the
// cell it read it from and gradient() in that cell.  A non-finite coordinate: SDFHIP_QUERY_INVALID and zeros, nothing looked up.
// xyz: n x 3 floats, packed; out: n records of two uint4 {distance, node, scale, status | gradient, 0}
template <class CursorT, bool NT>
__global__ __launch_bounds__(QUERY_THREADS) void k_query_sample(QueryScene Q, const float *__restrict__ xyz, uint32_t n, uint4 *__restrict__ out)
{
    const uint32_t i = blockIdx.x * QUERY_THREADS + threadIdx.x;
    if (i >= n) return;
    const float px = xyz[3 * (size_t)i], py = xyz[3 * (size_t)i + 1], pz = xyz[3 * (size_t)i + 2];
    uint4 a = make_uint4(0u, 0u, 0u, (uint32_t)QUERY_INVALID), b = make_uint4(0u, 0u, 0u, 0u);
    if (finite3(px, py, pz)) {
        CursorT c;
        c.loads = 0;
        c.reset(Q.nodes[0]);
        typename CursorT::Pos u;
        find_fresh(c, Q.nodes, grid_of(Q), Q.n_nodes, nullptr, 0u, px, py, pz, u);
        const float d = sample_after_find(c, u, px, py, pz);
        const Cell cell = c.cell();
        float gx, gy, gz;
        gradient(cell, px, py, pz, gx, gy, gz);
        a = make_uint4(__float_as_uint(d), node_of(c, Q), __float_as_uint(cell.scale), (uint32_t)QUERY_HIT);
        b = make_uint4(__float_as_uint(gx), __float_as_uint(gy), __float_as_uint(gz), 0u);
    }
    record_store<NT>(out + 2 * (size_t)i, a);
    record_store<NT>(out + 2 * (size_t)i + 1, b);
}

// march: Compute.hlsl:194-203 (oracle/sdf_oracle.c o_pixel's first loop) for query i, nothing added but t:
//     prox = 1; i = 0; t = 0; cursor at the root
//     while ((prox > margin2 || prox < 0) && i < max_steps) {
//         if (dot(pos, pos) > limit) -> ESCAPED
//         find(pos); prox = interpol_world(pos); pos = fma(dir, prox, pos); t = t + prox; i++ }
//     -> HIT if !(prox > margin2 || prox < 0) (a NaN prox ends the loop so, as it ends the shader's), else EXHAUSTED
// The cursor is carried from step to step (a position on a cell face belongs to the cell the cursor came from).
// PICK = false: `in` = n rays {origin, pad, dir, pad}, two float4 each; dir is used as given.
// PICK = true:  `in` = n pixels {x, y}; origin = the camera's position, direction = ray() of raymarch_device.h for that pixel.
// A non-finite origin or direction, or a direction of all zeros: SDFHIP_QUERY_INVALID and zeros, nothing looked up.
// out: n records of three uint4 {position, t | normal, prox | status, steps, node, scale}
template <class CursorT, bool PICK, bool NT>
__global__ __launch_bounds__(QUERY_THREADS) void k_query_march(QueryScene Q, const void *__restrict__ in, uint32_t n, FrameInfo I,
                                                               uint32_t max_steps, uint4 *__restrict__ out)
{
    const uint32_t i = blockIdx.x * QUERY_THREADS + threadIdx.x;
    if (i >= n) return;
    float px, py, pz, dx, dy, dz;
    if (PICK) {
        const uint2 xy = static_cast<const uint2 *>(in)[i];
        px = I.posx; py = I.posy; pz = I.posz;
        ray(I, xy.x, xy.y, dx, dy, dz);
    } else {
        const float4 o = static_cast<const float4 *>(in)[2 * (size_t)i], d = static_cast<const float4 *>(in)[2 * (size_t)i + 1];
        px = o.x; py = o.y; pz = o.z; dx = d.x; dy = d.y; dz = d.z;
    }
    uint4 a = make_uint4(0u, 0u, 0u, 0u), b = a, e = make_uint4((uint32_t)QUERY_INVALID, 0u, 0u, 0u);
    if (finite3(px, py, pz) && finite3(dx, dy, dz) && !(dx == 0.0f && dy == 0.0f && dz == 0.0f)) {
        const GridRef g = grid_of(Q);
        CursorT c;
        c.loads = 0;
        c.reset(Q.nodes[0]);
        float prox = 1.0f, t = 0.0f;
        uint32_t steps = 0u;
        auto marching = [&]() { return (prox > I.margin2 || prox < 0.0f) && steps < max_steps; };
        auto go_on = [&]() { return marching() && !(dot3(px, py, pz, px, py, pz) > I.limit); };
        auto advance = [&](const typename CursorT::Pos &u) {
            prox = sample_after_find(c, u, px, py, pz);
            px = __builtin_fmaf(dx, prox, px); py = __builtin_fmaf(dy, prox, py); pz = __builtin_fmaf(dz, prox, pz);
            t = t + prox;
            steps++;
        };
        if (go_on()) {                                   // the first step, from the root, apart: see find_fresh
            typename CursorT::Pos u;
            find_fresh(c, Q.nodes, g, Q.n_nodes, nullptr, 0u, px, py, pz, u);
            advance(u);
            while (go_on()) {
                find(c, Q.nodes, g, Q.n_nodes, nullptr, 0u, px, py, pz, u);
                advance(u);
            }
        }
        // header first, then the escape test, as the shader orders them: a lane the header stopped did not escape
        const uint32_t status = marching() ? (uint32_t)QUERY_ESCAPED : (prox > I.margin2 || prox < 0.0f) ? (uint32_t)QUERY_EXHAUSTED : (uint32_t)QUERY_HIT;
        const Cell cell = c.cell();
        float nx = 0.0f, ny = 0.0f, nz = 0.0f;
        if (status != (uint32_t)QUERY_ESCAPED) {
            float gx, gy, gz;
            gradient(cell, px, py, pz, gx, gy, gz);
            const float rg = 1.0f / sqrtf(dot3(gx, gy, gz, gx, gy, gz));    // Compute.hlsl:209's normalize
            nx = gx * rg; ny = gy * rg; nz = gz * rg;
        }
        a = make_uint4(__float_as_uint(px), __float_as_uint(py), __float_as_uint(pz), __float_as_uint(t));
        b = make_uint4(__float_as_uint(nx), __float_as_uint(ny), __float_as_uint(nz), __float_as_uint(prox));
        e = make_uint4(status, steps, node_of(c, Q), __float_as_uint(cell.scale));
    }
    record_store<NT>(out + 3 * (size_t)i, a);
    record_store<NT>(out + 3 * (size_t)i + 1, b);
    record_store<NT>(out + 3 * (size_t)i + 2, e);
}

}  // namespace sdfhip
