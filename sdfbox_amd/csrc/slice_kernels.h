// Cross-sections of a resident scene (gfx950): the contours of a stack of parallel planes, as directed segments -- plane k cuts N7's
// triangles, which are never written anywhere.  Non-template helpers and three kernels: included by slice.hip ONLY.  Host side, C ABI:
// slice.hip.  The cells, the inside bits, the six tetrahedra, the triangle table and cut_position are cell_tets.h's, shared with the
// mesh, the measure and the nearest-surface search.
//
// Replaces: nothing that runs in the reference -- its tree only ever becomes pixels (its Layers.hlsl, a z-slice viewer, is dead code).
//
// The rule is the contract of include/sdfhip.h (sdfhip_scene_slice) and DESIGN.md section 8 (N18): fp32, each operation rounded on its
// own, in the order written (-ffp-contract=off); tests/slice_restatement.py restates it with numpy on the mesh restatement's
// triangles, every triangle against every layer.
//
// The order (node index, then tetrahedron, then triangle, then layer) must not depend on which wave finished first, so the pass has
// the shape of the mesh's (mesh_kernels.h): count -> scan -> emit, the records streamed at both ends.
//   k_slice_count   one lane per node, SLICE_CHUNK nodes per workgroup in rows of SLICE_THREADS consecutive nodes: one 16-byte load
//                   gives links and bytes; a lane whose cell is cut climbs the links for its coordinates, finds the layers its box can
//                   meet (candidate_layers: the reject) and counts its triangles' crossings; the chunk's total goes to chunk[], the
//                   records per layer to layer_counts[] (integers: through an LDS histogram up to SLICE_LDS_LAYERS layers, one global
//                   atomic per layer and workgroup; straight to global memory above), the cells beside them.  Most lanes idle, as in
//                   the measure: a cut cell is one node in some tens
//   the scan        scan_device.h's k_scan_chunk_totals, as the mesh's
//   k_slice_emit    the same lanes read the same records again, row by row: recount, the offset from the chunk's prefix and a scan
//                   inside the workgroup (shuffles within a wave, LDS across the four), then the crossings again, each written as two
//                   16-byte stores
// One copy of the triangle walk (slice_cell<EMIT>) serves both passes, so that what is counted is what is written.
#pragma once
#include "../../include/sdfhip.h"      // sdfhip_segment
#include "cell_tets.h"      // the cells, their tetrahedra and triangles, the climb, the streamed record
#include "scan_device.h"     // k_scan_chunk_totals, wave_sum, wave_scan, ordered_first

namespace sdfhip {

constexpr int SLICE_THREADS = 256;
constexpr int SLICE_ROWS = 4;                                   // rows of SLICE_THREADS consecutive nodes per workgroup
constexpr uint32_t SLICE_CHUNK = SLICE_THREADS * SLICE_ROWS;    // 1024 nodes, the mesh's MESH_CHUNK
constexpr uint32_t SLICE_LDS_LAYERS = 1024;                     // up to this many layers the per-layer counts gather in LDS

// 64-bit record total (the scan's), the level's cells, those with mixed bytes, those that emit at least one record
struct SliceHeader { unsigned long long n_segments; uint32_t cells, cells_cut, cells_crossed, pad_; };
static_assert(offsetof(SliceHeader, n_segments) == 0, "the scan writes the total to the header's first eight bytes");

// plane k: dot(normal, p) = offset + (float)k * pitch, the normal as given
struct SlicePlanes { float nx, ny, nz, offset, pitch; uint32_t layers; };

__device__ __forceinline__ float plane_height(const SlicePlanes &pl, uint32_t k) { return pl.offset + (float)k * pl.pitch; }
__device__ __forceinline__ float point_height(const SlicePlanes &pl, float x, float y, float z) { return ((pl.nx * x) + (pl.ny * y)) + (pl.nz * z); }

// ---- the reject and its margin ---------------------------------------------------------------------------------------------------
// A cell is skipped unless some h_k lies in [lo, hi], and only the layers with h_k in [lo, hi] are tested against its triangles.  That
// must lose no record: a triangle gives one for plane k only if d_i < h_k <= d_j for two of its vertices, so lo <= d <= hi for the
// COMPUTED height d of every vertex of the cell is enough.  Derivation (u = 2^-24, the unit roundoff; A = |nx| + |ny| + |nz|):
//   the vertex   cut_position gives ((float)(c + bit) + t) * S per axis with 0 <= t <= 1: the sum is rounded between two
//                representable ends and S is a power of two, so the vertex lies in the cell's closed box [c S, (c + 1) S], within
//                [0, 1]; with the centre m = (c + 0.5) S (exact) and e = S / 2 its true height is within e A of dot(n, m)
//   d            three products and two sums, all of terms |n_a p_a| <= |n_a|:  |d - dot(n, p)| <= 3u A (1 + 3u)
//   mid          the same expression at the centre:                              |mid - dot(n, m)| <= 3u A (1 + 3u)
//   r = e * A'   A' = (|nx| + |ny|) + |nz| is at least A (1 - u)^2 and e <= 1/2 is a power of two:  r >= e A - u A
//   lo, hi       (mid -+ r) -+ margin: two roundings of values below 2 A, 2u A each
// together less than 11.001 u A; the margin is 2^-19 A' >= 31 u A.  Products that underflow (a normal below 2^-100 or so) lose at most
// 2^-149 each, which SLICE_TINY covers.  Heights that overflow (a normal near 2^127) make lo or hi infinite or NaN: then nothing is
// rejected and every layer is a candidate.
// The candidates come from a division, floor((lo - offset) / pitch) - 1 .. ceil((hi - offset) / pitch) + 1, clamped to the stack.  The
// quotient is only an estimate of where the COMPUTED h_k = offset + (float)k * pitch fall (where offset is large against the pitch,
// many k share one h_k), so the range is then corrected against the heights themselves: h_k never decreases with k ((float)k is
// exact, a product with pitch > 0 and a sum are monotonic), so the layers inside [lo, hi] are one run, the two `while` pairs below
// first grow the range until its neighbours are outside and then shrink it until its ends are inside, and what is left is exactly
// that run.  The exact comparisons on d_i and h_k decide within it.
constexpr float SLICE_MARGIN = 1.9073486328125e-6f;            // 2^-19
constexpr float SLICE_TINY = 7.888609052210118e-31f;           // 2^-100

// the layers k0 .. k1 whose planes can meet the box of the cell (cx, cy, cz) of edge S; false: none
__device__ __forceinline__ bool candidate_layers(const SlicePlanes &pl, uint32_t cx, uint32_t cy, uint32_t cz, float S, uint32_t &k0, uint32_t &k1)
{
    const uint32_t last = pl.layers - 1u;
    const float mid = point_height(pl, ((float)cx + 0.5f) * S, ((float)cy + 0.5f) * S, ((float)cz + 0.5f) * S);
    const float A = (fabsf(pl.nx) + fabsf(pl.ny)) + fabsf(pl.nz);
    const float r = (0.5f * S) * A, margin = A * SLICE_MARGIN + SLICE_TINY;
    const float lo = (mid - r) - margin, hi = (mid + r) + margin;
    k0 = 0u; k1 = last;
    if (!(fabsf(lo) < __int_as_float(0x7F800000)) || !(fabsf(hi) < __int_as_float(0x7F800000))) return true;
    if (last != 0u) {
        const float fl = (float)last;
        k0 = (uint32_t)fminf(fmaxf(floorf((lo - pl.offset) / pl.pitch) - 1.0f, 0.0f), fl);        // (a NaN quotient: 0)
        k1 = (uint32_t)fminf(fmaxf(ceilf((hi - pl.offset) / pl.pitch) + 1.0f, 0.0f), fl);
        if (k1 < k0) k1 = k0;
        while (k0 > 0u && plane_height(pl, k0 - 1u) >= lo) k0--;
        while (k1 < last && plane_height(pl, k1 + 1u) <= hi) k1++;
    }
    while (k0 <= k1 && plane_height(pl, k0) < lo) k0++;
    while (k0 <= k1 && plane_height(pl, k1) > hi) {
        if (k1 == 0u) return false;
        k1--;
    }
    return k0 <= k1;
}

// the point of plane h on the edge from its below end a (height da < h) to its above end b (db >= h)
__device__ __forceinline__ void crossing(float ax, float ay, float az, float da, float bx, float by, float bz, float db, float h,
                                         float &qx, float &qy, float &qz)
{
    const float sa = da - h, sb = db - h;
    const float t = sa / (sa - sb);
    qx = ax + (bx - ax) * t; qy = ay + (by - ay) * t; qz = az + (bz - az) * t;
}

__device__ __forceinline__ void store_segment(sdfhip_segment *__restrict__ out, uint32_t at, float ax, float ay, float az, uint32_t layer,
                                              float bx, float by, float bz, uint32_t node)
{
    uint4 *p = reinterpret_cast<uint4 *>(out + at);
    p[0] = make_uint4(__float_as_uint(ax), __float_as_uint(ay), __float_as_uint(az), layer);
    p[1] = make_uint4(__float_as_uint(bx), __float_as_uint(by), __float_as_uint(bz), node);
}

// The crossings of the cut cell (bytes v0 v1, inside bits in8, coordinates (cx, cy, cz) of its depth, edge S) with the layers k0 .. k1,
// in the pinned order: tetrahedron, triangle, layer.  Returns their number.  EMIT: writes them from out[first] on; otherwise adds
// them to hist[layer] when hist is given (LDS or global memory).
template <bool EMIT>
__device__ __forceinline__ uint32_t slice_cell(const SlicePlanes &pl, uint32_t v0, uint32_t v1, uint32_t in8, uint32_t cx, uint32_t cy, uint32_t cz,
                                               float S, uint32_t k0, uint32_t k1, uint32_t node, uint32_t first, sdfhip_segment *__restrict__ out,
                                               uint32_t *hist)
{
    uint32_t count = 0;
#pragma unroll 1
    for (int t = 0; t < 6; t++) {
        const uint32_t corners = tet_corners(t);
        const uint32_t e = MESH_TRIANGLES[t * 16 + (int)tet_mask(in8, t)];
        const uint32_t nt = e & 3u;
#pragma unroll 1
        for (uint32_t j = 0; j < nt; j++) {
            float px[3], py[3], pz[3], d[3];
#pragma unroll
            for (int v = 0; v < 3; v++) {
                const uint32_t ij = (e >> (4u + 4u * (3u * j + (uint32_t)v))) & 15u;
                const uint32_t lo = (corners >> (4u * (ij & 3u))) & 7u, hi = (corners >> (4u * (ij >> 2))) & 7u;
                cut_position(v0, v1, S, cx, cy, cz, lo, hi, px[v], py[v], pz[v]);
                d[v] = point_height(pl, px[v], py[v], pz[v]);
            }
#pragma unroll 1
            for (uint32_t k = k0; k <= k1; k++) {
                const float h = plane_height(pl, k);
                const bool a0 = d[0] >= h, a1 = d[1] >= h, a2 = d[2] >= h;
                if (a0 == a1 && a1 == a2) continue;
                if (!EMIT) {
                    if (hist) atomicAdd(&hist[k], 1u);
                } else {
                    // the vertex alone on its side, the one after it and the one before it on the walk 0 -> 1 -> 2 -> 0.  Alone above:
                    // the edge to the next goes above -> below (a) and the edge from the one before below -> above (b); alone
                    // below: the edge from the one before goes above -> below (a) and the edge to the next below -> above (b)
                    const int odd = a1 == a2 ? 0 : (a0 == a2 ? 1 : 2);
                    const bool up = odd == 0 ? a0 : (odd == 1 ? a1 : a2);
                    const float ox = odd == 0 ? px[0] : (odd == 1 ? px[1] : px[2]), oy = odd == 0 ? py[0] : (odd == 1 ? py[1] : py[2]);
                    const float oz = odd == 0 ? pz[0] : (odd == 1 ? pz[1] : pz[2]), od = odd == 0 ? d[0] : (odd == 1 ? d[1] : d[2]);
                    const float nx = odd == 0 ? px[1] : (odd == 1 ? px[2] : px[0]), ny = odd == 0 ? py[1] : (odd == 1 ? py[2] : py[0]);
                    const float nz = odd == 0 ? pz[1] : (odd == 1 ? pz[2] : pz[0]), nd = odd == 0 ? d[1] : (odd == 1 ? d[2] : d[0]);
                    const float rx = odd == 0 ? px[2] : (odd == 1 ? px[0] : px[1]), ry = odd == 0 ? py[2] : (odd == 1 ? py[0] : py[1]);
                    const float rz = odd == 0 ? pz[2] : (odd == 1 ? pz[0] : pz[1]), rd = odd == 0 ? d[2] : (odd == 1 ? d[0] : d[1]);
                    // the far ends of a's and of b's edge
                    const float fax = up ? nx : rx, fay = up ? ny : ry, faz = up ? nz : rz, fad = up ? nd : rd;
                    const float fbx = up ? rx : nx, fby = up ? ry : ny, fbz = up ? rz : nz, fbd = up ? rd : nd;
                    float ax, ay, az, bx, by, bz;
                    if (up) {                                   // the far ends are below
                        crossing(fax, fay, faz, fad, ox, oy, oz, od, h, ax, ay, az);
                        crossing(fbx, fby, fbz, fbd, ox, oy, oz, od, h, bx, by, bz);
                    } else {
                        crossing(ox, oy, oz, od, fax, fay, faz, fad, h, ax, ay, az);
                        crossing(ox, oy, oz, od, fbx, fby, fbz, fbd, h, bx, by, bz);
                    }
                    store_segment(out, first + count, ax, ay, az, k, bx, by, bz, node);
                }
                count++;
            }
        }
    }
    return count;
}

// What a lane knows of its node after the record and, where needed, the climb: is it a cell of the level, is it cut, and for a cut
// cell the coordinates of its depth.  WALK_ALL: the nodes that are not cut climb for their depth too where the level needs it (the
// statistics count the level's cells); otherwise only cut candidates climb.
struct SliceNode { bool cell, cut; uint32_t cx, cy, cz; int depth; };
template <bool WALK_ALL>
__device__ __forceinline__ SliceNode slice_node(const NodeRec *__restrict__ nodes, uint32_t n, uint32_t i, const NodeRec &rec, int level, uint32_t in8)
{
    SliceNode s;
    s.cell = false; s.cut = false; s.cx = 0; s.cy = 0; s.cz = 0; s.depth = 0;
    if (i >= n) return s;
    // (is_mixed's test, cell_tets.h, written out: as a call it reaches the compiler's first simplification of the two early returns
    // below opaque, the kernels' control flow comes out in another order, and k_slice_emit was measurably slower)
    const bool leaf = (int32_t)rec.y < 0, mixed = in8 != 0u && in8 != 0xFFu;
    if (level < 0 && !(leaf && mixed)) { s.cell = leaf; return s; }
    if (!mixed && !WALK_ALL) return s;
    s.depth = cell_climb(nodes, n, i, (int32_t)rec.x, s.cx, s.cy, s.cz);
    s.cell = is_cell((int32_t)rec.y, level, s.depth);
    s.cut = s.cell && mixed;
    return s;
}

// STATS: also count the level's cells, the cut ones and the crossed ones into the header.  layer_counts: layers words, zeroed by the
// host side, or null
template <bool STATS>
__global__ __launch_bounds__(SLICE_THREADS) void k_slice_count(const NodeRec *__restrict__ nodes, uint32_t n, int level, SlicePlanes pl,
                                                               uint32_t *__restrict__ chunk, SliceHeader *__restrict__ head,
                                                               uint32_t *__restrict__ layer_counts)
{
    __shared__ uint32_t part[4][SLICE_THREADS / 64];
    __shared__ uint32_t hist[SLICE_LDS_LAYERS];
    const bool in_lds = layer_counts != nullptr && pl.layers <= SLICE_LDS_LAYERS;            // (uniform over the grid)
    if (in_lds) for (uint32_t k = threadIdx.x; k < pl.layers; k += SLICE_THREADS) hist[k] = 0u;
    const uint32_t base = blockIdx.x * SLICE_CHUNK + threadIdx.x;
    NodeRec ahead = cell_record(nodes, n, base);
    __syncthreads();
    uint32_t segs = 0, cells = 0, cuts = 0, crossed = 0;
    // (one copy of the cell arithmetic, not one per row; the next row's record is in flight meanwhile)
#pragma unroll 1
    for (int row = 0; row < SLICE_ROWS; row++) {
        const uint32_t i = base + (uint32_t)row * SLICE_THREADS;
        const NodeRec rec = ahead;
        if (row + 1 < SLICE_ROWS) ahead = cell_record(nodes, n, i + SLICE_THREADS);
        const uint32_t in8 = inside_bits(rec.z, rec.w);
        const SliceNode s = slice_node<STATS>(nodes, n, i, rec, level, in8);
        cells += s.cell ? 1u : 0u; cuts += s.cut ? 1u : 0u;
        if (!s.cut) continue;
        const float S = __int_as_float((127 - s.depth) << 23);                              // 2^-depth
        uint32_t k0, k1;
        if (!candidate_layers(pl, s.cx, s.cy, s.cz, S, k0, k1)) continue;
        const uint32_t c = slice_cell<false>(pl, rec.z, rec.w, in8, s.cx, s.cy, s.cz, S, k0, k1, i, 0u, nullptr,
                                             in_lds ? hist : layer_counts);
        segs += c; crossed += c ? 1u : 0u;
    }
    segs = wave_sum(segs);
    if (STATS) { cells = wave_sum(cells); cuts = wave_sum(cuts); crossed = wave_sum(crossed); }
    const uint32_t wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63u) == 0u) { part[0][wave] = segs; part[1][wave] = cells; part[2][wave] = cuts; part[3][wave] = crossed; }
    __syncthreads();
    if (threadIdx.x == 0) {
        chunk[blockIdx.x] = part[0][0] + part[0][1] + part[0][2] + part[0][3];
        if (STATS) {
            const uint32_t c = part[1][0] + part[1][1] + part[1][2] + part[1][3], u = part[2][0] + part[2][1] + part[2][2] + part[2][3];
            const uint32_t x = part[3][0] + part[3][1] + part[3][2] + part[3][3];
            if (c) atomicAdd(&head->cells, c);
            if (u) atomicAdd(&head->cells_cut, u);
            if (x) atomicAdd(&head->cells_crossed, x);
        }
    }
    if (in_lds)
        for (uint32_t k = threadIdx.x; k < pl.layers; k += SLICE_THREADS) {
            const uint32_t v = hist[k];
            if (v) atomicAdd(&layer_counts[k], v);
        }
}

// chunk[]: the exclusive prefix the scan left.  Every lane stays in the kernel through the workgroup's scans (one barrier per row);
// only the cell work is under the lane's own condition.  out holds at least the total's records (the host side checked).
__global__ __launch_bounds__(SLICE_THREADS) void k_slice_emit(const NodeRec *__restrict__ nodes, uint32_t n, int level, SlicePlanes pl,
                                                              const uint32_t *__restrict__ chunk, sdfhip_segment *__restrict__ out)
{
    __shared__ uint32_t part[SLICE_ROWS][SLICE_THREADS / 64];
    const uint32_t base = blockIdx.x * SLICE_CHUNK + threadIdx.x;
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    NodeRec ahead = cell_record(nodes, n, base);
    uint32_t run = chunk[blockIdx.x];                           // the first record of this row's first wave
#pragma unroll 1
    for (int row = 0; row < SLICE_ROWS; row++) {
        const uint32_t i = base + (uint32_t)row * SLICE_THREADS;
        const NodeRec rec = ahead;
        if (row + 1 < SLICE_ROWS) ahead = cell_record(nodes, n, i + SLICE_THREADS);
        const uint32_t in8 = inside_bits(rec.z, rec.w);
        const SliceNode s = slice_node<false>(nodes, n, i, rec, level, in8);
        const float S = __int_as_float((127 - s.depth) << 23);
        uint32_t k0 = 0, k1 = 0, cnt = 0;
        if (s.cut && candidate_layers(pl, s.cx, s.cy, s.cz, S, k0, k1))
            cnt = slice_cell<false>(pl, rec.z, rec.w, in8, s.cx, s.cy, s.cz, S, k0, k1, i, 0u, nullptr, nullptr);
        const uint32_t incl = wave_scan(cnt);
        if (lane == 63u) part[row][wave] = incl;
        __syncthreads();
        const uint32_t first = ordered_first(incl, cnt, part[row], wave, run);
        if (cnt) slice_cell<true>(pl, rec.z, rec.w, in8, s.cx, s.cy, s.cz, S, k0, k1, i, first, out, nullptr);
    }
}

}  // namespace sdfhip
