// Surface extraction from a resident scene (gfx950): marching tetrahedra on the Kuhn decomposition of every cell whose bytes are
// mixed, as a triangle soup of {position, normal} vertices in a pinned order.  Non-template helpers (the cells and their tetrahedra:
// cell_tets.h) and three kernels: included by mesh.hip ONLY.  Host side, C ABI: mesh.hip; the writers: mesh_io.cpp.
//
// Replaces: nothing in the reference's code -- its tree only ever becomes pixels.
//
// The rule is the contract of include/sdfhip.h (sdfhip_scene_mesh) and DESIGN.md section 8 (N7): fp32, each operation rounded on its
// own, in the order written (-ffp-contract=off); tests/mesh_restatement.py restates it with numpy, node for node.  The normal is
// raymarch_device.h's gradient(), untouched, with the cell as the cursor's cell.
//
// The order (cells by node index, then tetrahedron, then triangle) must not depend on which wave finished first, so the pass is
// count -> scan -> emit, and both ends stream the records:
//   k_mesh_count   one lane per node, MESH_CHUNK nodes per workgroup: one 16-byte load gives links and bytes; the chunk's triangle
//                  total goes to chunk[]; cells and cut cells are counted beside it
//   the scan       scan_device.h's k_scan_chunk_totals: the chunks' totals -> exclusive prefix (one workgroup), the grand total as 64 bits
//   k_mesh_emit    the same lanes read the same records again, recount, take their offset from the chunk's prefix and a scan inside
//                  the workgroup (shuffles within a wave, LDS across the four), and the lanes whose cell is cut walk up the parent
//                  links for their coordinates (at most 12 dependent 8-byte loads) and write their triangles
// Reading the records twice (2 x 16 bytes per node) is cheaper than a per-node count array written, scanned and read back, and
// keeps the temporary memory at four bytes per 1024 nodes.
#pragma once
#include "cell_tets.h"      // the cells, their tetrahedra and triangles, the climb, the streamed record
#include "scan_device.h"     // k_scan_chunk_totals, wave_sum, wave_scan, ordered_first

namespace sdfhip {

constexpr int MESH_THREADS = 256;
constexpr int MESH_ROWS = 4;                                  // rows of MESH_THREADS consecutive nodes per workgroup
constexpr uint32_t MESH_CHUNK = MESH_THREADS * MESH_ROWS;

// what the passes count beside the triangles: 64-bit triangle total (the scan's), cells of the level, cells whose bytes are mixed
struct MeshHeader { unsigned long long n_triangles; uint32_t cells, cells_cut; };
static_assert(offsetof(MeshHeader, n_triangles) == 0, "the scan writes the total to the header's first eight bytes");

// A node's triangle count, and whether it is a cell and a cut one (for the statistics)
__device__ __forceinline__ uint32_t node_triangles(const NodeRec *__restrict__ nodes, uint32_t n, const NodeRec &r, int level, bool &cell, bool &cut)
{
    const uint32_t in8 = inside_bits(r.z, r.w);
    // (the statistics count the level's cells, so for a level >= 0 the flat nodes walk for their depth too)
    cell = is_cell(nodes, n, r, level);
    cut = cell && is_mixed(in8);
    return cut ? cell_triangles(in8) : 0u;
}

// STATS: also count the level's cells and cut cells into the header (the flat nodes of a level >= 0 then walk for their depth too)
template <bool STATS>
__global__ __launch_bounds__(MESH_THREADS) void k_mesh_count(const NodeRec *__restrict__ nodes, uint32_t n, int level, uint32_t *__restrict__ chunk,
                                                             MeshHeader *__restrict__ head)
{
    __shared__ uint32_t part[3][MESH_THREADS / 64];
    const uint32_t base = blockIdx.x * MESH_CHUNK + threadIdx.x;
    NodeRec r[MESH_ROWS];
#pragma unroll
    for (int k = 0; k < MESH_ROWS; k++) {
        const uint32_t i = base + (uint32_t)k * MESH_THREADS;
        r[k] = cell_record(nodes, n, i);
    }
    uint32_t tris = 0, cells = 0, cuts = 0;
#pragma unroll
    for (int k = 0; k < MESH_ROWS; k++) {
        const uint32_t i = base + (uint32_t)k * MESH_THREADS;
        if (i >= n) continue;
        bool cell = false, cut = false;
        if (STATS || level < 0) {
            tris += node_triangles(nodes, n, r[k], level, cell, cut);
        } else {
            const uint32_t in8 = inside_bits(r[k].z, r[k].w);
            if (is_cut_cell(nodes, n, r[k], level, in8)) tris += cell_triangles(in8);
        }
        cells += cell ? 1u : 0u; cuts += cut ? 1u : 0u;
    }
    tris = wave_sum(tris);
    if (STATS) { cells = wave_sum(cells); cuts = wave_sum(cuts); }
    const uint32_t wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63u) == 0u) { part[0][wave] = tris; part[1][wave] = cells; part[2][wave] = cuts; }
    __syncthreads();
    if (threadIdx.x == 0) {
        chunk[blockIdx.x] = part[0][0] + part[0][1] + part[0][2] + part[0][3];
        if (STATS) {
            const uint32_t c = part[1][0] + part[1][1] + part[1][2] + part[1][3], u = part[2][0] + part[2][1] + part[2][2] + part[2][3];
            if (c) atomicAdd(&head->cells, c);
            if (u) atomicAdd(&head->cells_cut, u);
        }
    }
}

// A triangle is 72 bytes, so triangle k starts 8 bytes past a 16-byte boundary when k is odd: 16-byte stores with one 8-byte store in
// front (odd) or behind (even).  WIDE = false: nine 8-byte stores; NT = true: non-temporal stores, as the query records
// (query_kernels.h) -- both measured slower here (mesh.hip has the figures) and kept for the A/B.
template <bool NT> __device__ __forceinline__ void store2(float *p, float a, float b)
{
    typedef float f32x2 __attribute__((ext_vector_type(2)));
    if (NT) __builtin_nontemporal_store((f32x2){a, b}, reinterpret_cast<f32x2 *>(p));
    else *reinterpret_cast<f32x2 *>(p) = (f32x2){a, b};
}
template <bool NT> __device__ __forceinline__ void store4(float *p, float a, float b, float c, float d)
{
    typedef float f32x4 __attribute__((ext_vector_type(4)));
    if (NT) __builtin_nontemporal_store((f32x4){a, b, c, d}, reinterpret_cast<f32x4 *>(p));
    else *reinterpret_cast<f32x4 *>(p) = (f32x4){a, b, c, d};
}
template <bool NT, bool WIDE>
__device__ __forceinline__ void store_triangle(float *__restrict__ verts6, uint32_t tri, const float (&f)[18])
{
    float *p = verts6 + (size_t)tri * 18;
    if (!WIDE) {
#pragma unroll
        for (int k = 0; k < 9; k++) store2<NT>(p + 2 * k, f[2 * k], f[2 * k + 1]);
    } else if (tri & 1u) {
        store2<NT>(p, f[0], f[1]);
#pragma unroll
        for (int k = 0; k < 4; k++) store4<NT>(p + 2 + 4 * k, f[2 + 4 * k], f[3 + 4 * k], f[4 + 4 * k], f[5 + 4 * k]);
    } else {
#pragma unroll
        for (int k = 0; k < 4; k++) store4<NT>(p + 4 * k, f[4 * k], f[4 * k + 1], f[4 * k + 2], f[4 * k + 3]);
        store2<NT>(p + 16, f[16], f[17]);
    }
}

// The vertex on the cut edge from cube corner lo to cube corner hi (the bits of lo are a subset of hi's) of the cell with integer
// coordinates (cx, cy, cz) of its depth, edge S: position (cut_position, cell_tets.h), then gradient() there times 1 / sqrt(dot(g, g)), as sdfhip_hit.normal
__device__ __forceinline__ void cut_vertex(const Cell &cell, uint32_t cx, uint32_t cy, uint32_t cz, uint32_t lo, uint32_t hi, float *o)
{
    float px, py, pz;
    cut_position(cell.v0, cell.v1, cell.scale, cx, cy, cz, lo, hi, px, py, pz);
    float gx, gy, gz;
    gradient(cell, px, py, pz, gx, gy, gz);
    const float rg = 1.0f / sqrtf(dot3(gx, gy, gz, gx, gy, gz));
    o[0] = px; o[1] = py; o[2] = pz; o[3] = gx * rg; o[4] = gy * rg; o[5] = gz * rg;
}

// chunk[]: the exclusive prefix the scan left.  Every lane stays in the kernel through the workgroup's scans; only the vertex work
// is under the lane's own condition.
template <bool NT, bool WIDE>
__global__ __launch_bounds__(MESH_THREADS) void k_mesh_emit(const NodeRec *__restrict__ nodes, uint32_t n, int level, const uint32_t *__restrict__ chunk,
                                                            float *__restrict__ verts6)
{
    __shared__ uint32_t part[MESH_ROWS][MESH_THREADS / 64];
    const uint32_t base = blockIdx.x * MESH_CHUNK + threadIdx.x;
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    NodeRec r[MESH_ROWS];
#pragma unroll
    for (int k = 0; k < MESH_ROWS; k++) {
        const uint32_t i = base + (uint32_t)k * MESH_THREADS;
        r[k] = cell_record(nodes, n, i);
    }
    uint32_t cnt[MESH_ROWS], incl[MESH_ROWS];
#pragma unroll
    for (int k = 0; k < MESH_ROWS; k++) {
        const uint32_t i = base + (uint32_t)k * MESH_THREADS;
        const uint32_t in8 = inside_bits(r[k].z, r[k].w);
        cnt[k] = 0u;
        if (i < n && is_cut_cell(nodes, n, r[k], level, in8)) cnt[k] = cell_triangles(in8);
        incl[k] = wave_scan(cnt[k]);
        if (lane == 63u) part[k][wave] = incl[k];
    }
    __syncthreads();
    uint32_t run = chunk[blockIdx.x];                     // the first triangle of this row's first wave
#pragma unroll
    for (int k = 0; k < MESH_ROWS; k++) {
        uint32_t first = ordered_first(incl[k], cnt[k], part[k], wave, run);
        if (cnt[k] == 0u) continue;
        uint32_t cx, cy, cz;
        const int depth = cell_climb(nodes, n, base + (uint32_t)k * MESH_THREADS, (int32_t)r[k].x, cx, cy, cz);
        Cell cell;
        cell.scale = __int_as_float((127 - depth) << 23);                           // 2^-depth
        cell.inv = __int_as_float((127 + depth) << 23);
        cell.lx = (float)cx * cell.scale; cell.ly = (float)cy * cell.scale; cell.lz = (float)cz * cell.scale;       // exact
        cell.v0 = r[k].z; cell.v1 = r[k].w;
        const uint32_t in8 = inside_bits(r[k].z, r[k].w);
        for (int t = 0; t < 6; t++) {
            const uint32_t corners = tet_corners(t);
            const uint32_t e = MESH_TRIANGLES[t * 16 + (int)tet_mask(in8, t)];
            const uint32_t nt = e & 3u;
            for (uint32_t j = 0; j < nt; j++) {
                float f[18];
#pragma unroll
                for (int v = 0; v < 3; v++) {
                    const uint32_t ij = (e >> (4u + 4u * (3u * j + (uint32_t)v))) & 15u;
                    const uint32_t lo = (corners >> (4u * (ij & 3u))) & 7u, hi = (corners >> (4u * (ij >> 2))) & 7u;
                    cut_vertex(cell, cx, cy, cz, lo, hi, f + 6 * v);
                }
                store_triangle<NT, WIDE>(verts6, first, f);
                first++;
            }
        }
    }
}

}  // namespace sdfhip
