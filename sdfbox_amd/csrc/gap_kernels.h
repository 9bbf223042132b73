// The clearance of an assembly of placed instances (gfx950): how far apart the surfaces of each pair of parts lie, and where they are
// nearest.  k_gap_cells (the cut-cell list of one source, as a count and as an emit, and its tight box), k_gap_search (one lane per
// cut cell of one part, a bounded nearest-surface search into the other part for each of the cell's cut vertices), k_gap_record (the
// records).  Host side, C ABI: gap.hip.
//
// Replaces: nothing in the reference's code -- its shader marches ONE immutable tree and knows no parts.
//
// The rule is the contract of include/sdfhip.h (sdfhip_instances_gap) and DESIGN.md section 8 (N23): fp32, each operation rounded on
// its own, in the order written (-ffp-contract=off); tests/gap_restatement.py restates it with numpy, by brute force.
//   surface     of part k: sdfhip_scene_mesh's triangles of its source at level -1, in emitted order (node, then triangle k, then vertex v)
//   world w     ((R[i][0] x + R[i][1] y) + R[i][2] z) * s + t_i of an emitted position (cut_position of cell_tets.h: the same bits)
//   r_k(w)      the penetration's, word for word: q = the placement's inverse map of w, no clamp; r_k = sqrtf(d2_k(q)) * s_k
//   gap(a, b)   the minimum of r_b over the vertices of a's triangles (direction 0) and of r_a over those of b's (direction 1); a NaN
//               never wins, +inf is no record, a record iff gap <= limit; witness = the lowest (direction, node, 3 k + v) attaining it
// The minimum with its tie rule is a 64-bit integer atomicMin of (float bits << 32) | (direction << 31 | node): the values are >= 0 and
// never a NaN, so their bits are monotone; node indices fit 31 bits (links are int32).  The key starts at (bits(limit) << 32) |
// 0xFFFFFFFF, which no candidate equals: a key that moved is a record.  `corner` is resolved by the one lane of k_gap_record that owns
// the witness cell, from the cell alone.  No float is ever accumulated as a float: two calls give the same records.
//
// ---- the bound of a search ---------------------------------------------------------------------------------------------------------
// A lane holds B, a world value that some candidate of its pair attains or the limit (the pair's key, read at any time: the key only
// ever falls, so a stale read is a looser bound, never a wrong one).  A vertex matters only if its r <= B: a larger r can neither
// lower the key nor win a tie.  r = fl(fl(sqrtf(t)) * s) with t the search's d2; sqrtf and the multiplication by s > 0 are monotone
// (correctly rounded, non-decreasing), so r is non-decreasing in t.  Hence a source-space D with fl(fl(sqrtf(D)) * s) > B has: t >= D
// implies r(t) >= r(D) > B.  The search starts from best.d2 = D with no triangle, and skips a box only on gap2 * SEARCH_KEEP > best.d2
// (strict), which by the derivation at SEARCH_KEEP (distance_kernels.h) implies t > best.d2 for every triangle in the box: every
// triangle with t <= D is still visited, ties at the bound included, and the fold keeps the lowest (node, tri) of those that tie --
// the same triangle the unbounded search keeps whenever its d2 <= D.  So a vertex with r <= B gets the bits the unbounded search gives
// it, and a vertex with r > B gets either those bits or "nothing found"; neither can move the key wrongly.
// gap_bound finds such a D: x = B / s and D = x * x are within a few ulps of the exact (B / s)^2; D is stepped up one ulp at a time
// and VERIFIED by computing fl(fl(sqrtf(D)) * s) > B, at most GAP_BOUND_STEPS times; if none verifies (B = +inf, an overflow, a value
// the flush of denormals keeps at 0) the bound is +inf, which prunes nothing.  The verification, not the estimate, is what the
// argument rests on.
// SDFHIP_GAP_NO_PRUNE: B is never read, D = +inf, and every triangle vertex is searched, repeated cut vertices included.
//
// The search itself is RESTATED here (gap_search_from: nearest_search of distance_kernels.h from its first descent on, the start
// given) rather than split out of nearest_search: that function is compiled into the kernels of distance.hip, blend.hip and
// penetration.hip, whose resource lines are committed measurements.  fold_cell, sibling_bits, axis_gap2 and the margin are shared.
//
// Shape.
//   k_gap_cells<false>   one lane per node of a source, 256 to a workgroup: is it a cut cell of level -1; the workgroup's count goes to
//                        chunk[blockIdx.x].  scan_device.h's k_scan_chunk_totals turns the counts into offsets and the total
//   k_gap_cells<true>    the same test again; the lane's place is chunk[blockIdx.x] + its rank in the workgroup (block_exclusive_scan):
//                        node order.  It climbs for the cell's depth and coordinates, writes the 16-byte item, and folds the cell's box
//                        in units of 2^-MESH_MAX_DEPTH into six integers: a wave's min / max by shuffles, then one atomicMin /
//                        atomicMax per wave and bound
//   k_gap_search         one workgroup per entry of the host's work table = (ordered pair, chunk of 256 cells of its first part): the
//                        pair is uniform across the workgroup.  One lane per cut cell, the search's stack in LDS laid out
//                        [level][lane] as k_dist_query has it
//   k_gap_record         one lane per pair of the list whose key moved: the corner, the far side's cell and point, the flags
#pragma once
#include "compose_instance.h"   // ComposeInstance, compose_instance_value, PlaceMap
#include "distance_kernels.h"   // DistScene, Nearest, fold_cell, sibling_bits, axis_gap2, SEARCH_KEEP, nearest_search, k_dist_mark (static)
#include "scan_device.h"        // block_exclusive_scan, k_scan_chunk_totals

namespace sdfhip {

constexpr int GAP_THREADS = 256;
constexpr uint32_t GAP_MAX_INSTANCES = 64;
constexpr int GAP_BOUND_STEPS = 16;
constexpr uint32_t GAP_NO_PRUNE = 1u;           // SDFHIP_GAP_NO_PRUNE of include/sdfhip.h

// one cut cell of a source: its node, its integer coordinates of its depth, its depth
struct GapCell {
    uint32_t node, xy, z, depth;                // xy = x | y << 16
};
static_assert(sizeof(GapCell) == 16, "the host allocates 16 bytes per cut cell");

// the tight box of a source's cut cells in units of 2^-MESH_MAX_DEPTH; lo starts at 0xFFFFFFFF, hi at 0
struct GapBox {
    uint32_t lo[3], hi[3];
};

// one entry of the call's table: the clash check's, what the search reads of the same source, and the source's cut cells
struct GapInstance {
    ComposeInstance I;
    DistScene D;
    const GapCell *cells;
    uint32_t n_cells, pad;
};

// one ordered pair the broad phase kept: the cells of `from` are held against `to`; e = the pair's entry in the key table
struct GapOrdered {
    uint32_t from, to, e, direction;
};
// one workgroup of k_gap_search
struct GapWork {
    uint32_t ordered, chunk;
};

// sdfhip_gap of include/sdfhip.h
struct GapRecord {
    uint32_t a, b;
    float gap;
    uint32_t flags, node_a, node_b, corner;
    float point_a[3], point_b[3];
    uint32_t pad[3];
};
static_assert(sizeof(GapRecord) == 64, "sdfhip_gap of include/sdfhip.h");

// the call's counters, zeroed
struct GapCounters {
    unsigned long long searches;    // the vertex searches k_gap_search ran
    unsigned long long visited;     // the node records they loaded
};

// ---- the cut-cell list --------------------------------------------------------------------------------------------------------------

template <bool EMIT>
__global__ __launch_bounds__(GAP_THREADS) void k_gap_cells(const NodeRec *__restrict__ nodes, uint32_t n, uint32_t *__restrict__ chunk,
                                                           GapCell *__restrict__ cells, uint32_t n_cells, GapBox *__restrict__ box)
{
    __shared__ uint32_t part[GAP_THREADS];
    const uint64_t at = (uint64_t)blockIdx.x * GAP_THREADS + threadIdx.x;
    const uint32_t i = at < n ? (uint32_t)at : 0u;
    const NodeRec r = cell_record(nodes, n, at < n ? i : n);
    const bool cut = at < n && is_cut_cell(nodes, n, r, -1, inside_bits(r.z, r.w));
    uint32_t total;
    const uint32_t rank = block_exclusive_scan<uint32_t, GAP_THREADS>(cut ? 1u : 0u, part, total);
    if (!EMIT) {
        if (threadIdx.x == 0) chunk[blockIdx.x] = total;
        return;
    }
    uint32_t lo[3] = {0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu}, hi[3] = {0u, 0u, 0u};
    if (cut) {
        uint32_t c[3];
        const int depth = cell_climb(nodes, n, i, (int32_t)r.x, c[0], c[1], c[2]);
        const uint64_t to = (uint64_t)chunk[blockIdx.x] + rank;
        if (to < n_cells) cells[to] = GapCell{i, c[0] | (c[1] << 16), c[2], (uint32_t)depth};      // (always: the count pass counted the same cells)
        if (depth <= MESH_MAX_DEPTH) {                                                              // (always, on a tree the host side takes)
            const uint32_t up = (uint32_t)(MESH_MAX_DEPTH - depth);
#pragma unroll
            for (int a = 0; a < 3; a++) { lo[a] = c[a] << up; hi[a] = (c[a] + 1u) << up; }
        }
    }
#pragma unroll
    for (int a = 0; a < 3; a++) {
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) {
            lo[a] = min(lo[a], (uint32_t)__shfl_xor((int)lo[a], o));
            hi[a] = max(hi[a], (uint32_t)__shfl_xor((int)hi[a], o));
        }
    }
    if ((threadIdx.x & 63u) == 0u && lo[0] != 0xFFFFFFFFu) {
#pragma unroll
        for (int a = 0; a < 3; a++) { atomicMin(&box->lo[a], lo[a]); atomicMax(&box->hi[a], hi[a]); }
    }
}

// ---- the maps -------------------------------------------------------------------------------------------------------------------------

// the forward map of the record's points: ((R[i][0] x + R[i][1] y) + R[i][2] z) * s + t_i
__device__ __forceinline__ void gap_forward(const PlaceMap &M, float x, float y, float z, float &wx, float &wy, float &wz)
{
    wx = ((M.r[0][0] * x + M.r[0][1] * y) + M.r[0][2] * z) * M.s + M.tx;
    wy = ((M.r[1][0] * x + M.r[1][1] * y) + M.r[1][2] * z) * M.s + M.ty;
    wz = ((M.r[2][0] * x + M.r[2][1] * y) + M.r[2][2] * z) * M.s + M.tz;
}

// the placement's inverse map: place_value's first three lines, no clamp (penetration_kernels.h's pen_inverse)
__device__ __forceinline__ void gap_inverse(const PlaceMap &M, float px, float py, float pz, float &qx, float &qy, float &qz)
{
    const float d0 = px - M.tx, d1 = py - M.ty, d2 = pz - M.tz;
    qx = ((M.r[0][0] * d0 + M.r[1][0] * d1) + M.r[2][0] * d2) * M.inv;
    qy = ((M.r[0][1] * d0 + M.r[1][1] * d1) + M.r[2][1] * d2) * M.inv;
    qz = ((M.r[0][2] * d0 + M.r[1][2] * d1) + M.r[2][2] * d2) * M.inv;
}

// ---- the bounded search ------------------------------------------------------------------------------------------------------------

// D of "the bound of a search" above for the world value B and the scale s of the part searched: fl(fl(sqrtf(D)) * s) > B, or +inf
__device__ __forceinline__ float gap_bound(float B, float s)
{
    const float x = B / s;
    float D = x * x;
#pragma unroll 1
    for (int k = 0; k < GAP_BOUND_STEPS; k++) {
        if (!(D < __int_as_float(0x7F800000))) break;
        if (sqrtf(D) * s > B) return D;
        D = __uint_as_float(__float_as_uint(D) + 1u);          // (D >= +0 and finite: the next float up)
    }
    return __int_as_float(0x7F800000);
}

// nearest_search of distance_kernels.h with the start given: best.d2 = the bound D, best.node = 0xFFFFFFFF (no triangle).  Afterwards
// best.node != 0xFFFFFFFF iff some triangle has tri_dist2 <= D (and below +inf is the caller's test), and then best is the unbounded
// search's.  best.visited is added to.
template <int THREADS>
__device__ __forceinline__ void gap_search_from(const DistScene &D, float px, float py, float pz, uint2 *stk, Nearest &best)
{
    if (!(D.below[0] & 1u)) return;
    {                                                       // (6 of the margin's derivation: every distance overflows)
        const float k = 0x1p-32f;
        const float fx = fmaxf(fmaxf(0.0f - px, px - 1.0f) - SEARCH_SLACK, 0.0f) * k, fy = fmaxf(fmaxf(0.0f - py, py - 1.0f) - SEARCH_SLACK, 0.0f) * k,
                    fz = fmaxf(fmaxf(0.0f - pz, pz - 1.0f) - SEARCH_SLACK, 0.0f) * k;
        if ((fx * fx + fy * fy) + fz * fz >= 0x1p65f) return;
    }
    const NodeRec root = D.nodes[0];
    best.visited++;
    if (is_cell((int32_t)root.y, D.level, 0)) { fold_cell(root, 0u, 0, 0u, 0u, 0u, px, py, pz, best); return; }
    int d = 0;
    uint32_t cx = 0u, cy = 0u, cz = 0u, base = root.y;
    if ((uint64_t)base + 8u > D.n) return;
    uint32_t todo = sibling_bits(D.below, base);
    for (;;) {
        if (todo == 0u) {                                   // the way back
            if (d == 0) break;
            d--;
            cx >>= 1; cy >>= 1; cz >>= 1;
            const uint2 e = stk[d * THREADS];
            base = e.x; todo = e.y;
            continue;
        }
        const float S = __int_as_float((127 - (d + 1)) << 23);
        const float x0 = (float)(2u * cx) * S, x1 = (float)(2u * cx + 1u) * S, x2 = (float)(2u * cx + 2u) * S;
        const float y0 = (float)(2u * cy) * S, y1 = (float)(2u * cy + 1u) * S, y2 = (float)(2u * cy + 2u) * S;
        const float z0 = (float)(2u * cz) * S, z1 = (float)(2u * cz + 1u) * S, z2 = (float)(2u * cz + 2u) * S;
        const float gx[2] = { axis_gap2(px, x0, x1), axis_gap2(px, x1, x2) };
        const float gy[2] = { axis_gap2(py, y0, y1), axis_gap2(py, y1, y2) };
        const float gz[2] = { axis_gap2(pz, z0, z1), axis_gap2(pz, z1, z2) };
        float near2 = 0.0f;
        uint32_t c = 8u;
#pragma unroll
        for (uint32_t k = 0; k < 8u; k++) {
            const float g = (gx[k & 1u] + gy[k >> 1 & 1u]) + gz[k >> 2];
            if ((todo >> k & 1u) && (c == 8u || g < near2)) { c = k; near2 = g; }
        }
        if (fminf(near2, 3.402823466e+38f) * SEARCH_KEEP > best.d2) { todo = 0u; continue; }      // strict: a tie at the bound is still found
        todo &= ~(1u << c);
        const uint32_t node = base + c;
        const NodeRec r = D.nodes[node];
        best.visited++;
        const uint32_t nx = 2u * cx + (c & 1u), ny = 2u * cy + (c >> 1 & 1u), nz = 2u * cz + (c >> 2);
        if (is_cell((int32_t)r.y, D.level, d + 1)) {
            const uint32_t in8 = inside_bits(r.z, r.w);
            if (in8 != 0u && in8 != 0xFFu) fold_cell(r, node, d + 1, nx, ny, nz, px, py, pz, best);
            continue;
        }
        if ((int32_t)r.y < 0 || (uint64_t)r.y + 8u > D.n || d + 1 >= MESH_MAX_DEPTH) continue;
        stk[d * THREADS] = make_uint2(base, todo);
        d++;
        cx = nx; cy = ny; cz = nz;
        base = r.y;
        todo = sibling_bits(D.below, base);
    }
}

// r_to(w) of the world point w with the search bounded by D; false: no triangle within the bound (or none nearer than +inf).  near:
// q - r of the winning triangle in the source's coordinates
__device__ __forceinline__ bool gap_radius(const GapInstance &to, float wx, float wy, float wz, float D, uint2 *stk, Nearest &best, float &r,
                                           float *near)
{
    float qx, qy, qz;
    gap_inverse(to.I.M, wx, wy, wz, qx, qy, qz);
    best.d2 = D;
    best.node = 0xFFFFFFFFu; best.tri = 0u;
    best.rx = 0.0f; best.ry = 0.0f; best.rz = 0.0f;
    gap_search_from<GAP_THREADS>(to.D, qx, qy, qz, stk, best);
    if (best.node == 0xFFFFFFFFu) return false;
    r = sqrtf(best.d2) * to.I.M.s;
    near[0] = qx - best.rx; near[1] = qy - best.ry; near[2] = qz - best.rz;
    return r < __int_as_float(0x7F800000);                  // (an overflow, or a d2 of +inf: no candidate)
}

// vertex (triangle j of tetrahedron t's entry e, vertex v) of a cut cell: its cube corners lo < hi and its emitted position
__device__ __forceinline__ void gap_vertex(const NodeRec &r, float scale, uint32_t cx, uint32_t cy, uint32_t cz, uint32_t corners, uint32_t e, uint32_t j,
                                           uint32_t v, uint32_t &lo, uint32_t &hi, float &x, float &y, float &z)
{
    const uint32_t ij = (e >> (4u + 4u * (3u * j + v))) & 15u;
    lo = (corners >> (4u * (ij & 3u))) & 7u; hi = (corners >> (4u * (ij >> 2))) & 7u;
    cut_position(r.z, r.w, scale, cx, cy, cz, lo, hi, x, y, z);
}

// One lane per cut cell of the ordered pair's first part.  The lane's minimum over its cell's vertices, the first of those that tie;
// one atomicMin if it is at or under what the lane last read of the key
__global__ __launch_bounds__(GAP_THREADS) void k_gap_search(const GapInstance *__restrict__ table, const GapOrdered *__restrict__ ordered,
                                                            const GapWork *__restrict__ work, uint32_t n_work, uint32_t flags,
                                                            unsigned long long *__restrict__ keys, GapCounters *__restrict__ C)
{
    __shared__ uint2 stack[MESH_MAX_DEPTH * GAP_THREADS];
    unsigned long long seen = 0ull;
    uint32_t ran = 0u;
    if (blockIdx.x < n_work) {
        const GapWork W = work[blockIdx.x];
        const GapOrdered O = ordered[W.ordered];
        const GapInstance &from = table[O.from], &to = table[O.to];
        const uint64_t at = (uint64_t)W.chunk * GAP_THREADS + threadIdx.x;
        if (at < from.n_cells && to.D.below) {
            const GapCell cell = from.cells[at];
            const NodeRec r = from.D.nodes[cell.node];
            const uint32_t cx = cell.xy & 0xFFFFu, cy = cell.xy >> 16, cz = cell.z;
            const float scale = __int_as_float((127 - (int)cell.depth) << 23);
            const uint32_t in8 = inside_bits(r.z, r.w);
            const bool prune = !(flags & GAP_NO_PRUNE);
            const PlaceMap M = from.I.M;
            const float s_to = to.I.M.s;
            uint32_t mine = 0x7F800000u;                    // the lane's minimum so far, as bits: +inf
            unsigned long long done = 0ull;                 // the cut edges already searched: bit 8 lo + hi
            Nearest best;
            best.visited = 0u;
            for (int t = 0; t < 6; t++) {
                const uint32_t corners = tet_corners(t);
                const uint32_t e = MESH_TRIANGLES[t * 16 + (int)tet_mask(in8, t)];
                const uint32_t nt = e & 3u;
                for (uint32_t j = 0; j < nt; j++)
                    for (uint32_t v = 0; v < 3u; v++) {
                        uint32_t lo, hi;
                        float x, y, z, wx, wy, wz, rr, near[3];
                        gap_vertex(r, scale, cx, cy, cz, corners, e, j, v, lo, hi, x, y, z);
                        float D = __int_as_float(0x7F800000);
                        if (prune) {
                            // a vertex met before has the same position, so the same r: it cannot be a lower corner of the minimum
                            const unsigned long long bit = 1ull << (8u * lo + hi);
                            if (done & bit) continue;
                            done |= bit;
                            const uint32_t key_bits = (uint32_t)(__hip_atomic_load(keys + O.e, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) >> 32);
                            D = gap_bound(__uint_as_float(min(key_bits, mine)), s_to);
                        }
                        gap_forward(M, x, y, z, wx, wy, wz);
                        ran++;
                        if (!gap_radius(to, wx, wy, wz, D, stack + threadIdx.x, best, rr, near)) continue;
                        const uint32_t bits = __float_as_uint(rr);
                        if (bits < mine) mine = bits;
                    }
            }
            seen = best.visited;
            if (mine < 0x7F800000u) {
                const unsigned long long key = ((unsigned long long)mine << 32) | (unsigned long long)((O.direction << 31) | cell.node);
                // (a plain read first: most lanes lose, and a lost atomic is still a trip to memory)
                if (key < __hip_atomic_load(keys + O.e, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMin(keys + O.e, key);
            }
        }
    }
    // the counters: the lanes' sums, one atomicAdd per wave
    uint32_t lo = (uint32_t)seen, hi = (uint32_t)(seen >> 32);
    unsigned long long sum = seen;
    for (uint32_t o = 32u; o; o >>= 1) {
        const uint32_t vlo = __shfl_xor(lo, o), vhi = __shfl_xor(hi, o);
        sum += ((unsigned long long)vhi << 32) | vlo;
        lo = (uint32_t)sum; hi = (uint32_t)(sum >> 32);
    }
    const uint32_t searches = wave_sum(ran);
    if ((threadIdx.x & 63u) == 0u && searches) {
        atomicAdd(&C->searches, (unsigned long long)searches);
        atomicAdd(&C->visited, sum);
    }
}

// The records: lane e for entry e of the pair table (pair_a / pair_b: its parts).  `out` was zeroed; an entry whose key never moved
// stays zero and the host drops it (its low word is still 0xFFFFFFFF).  The lane owns the witness cell: it walks the cell's vertices
// in 3 k + v order, each with the search bounded by the gap itself, and the first whose r has the gap's bits is the corner; then one
// unbounded search at the witness for the far side's cell and point, and the clash check's containment of each of the two points in
// the other point's part for bit 1
__global__ __launch_bounds__(GAP_THREADS) void k_gap_record(const GapInstance *__restrict__ table, uint32_t K, const unsigned long long *__restrict__ keys,
                                                            uint32_t n_table, GapRecord *__restrict__ out)
{
    __shared__ uint2 stack[MESH_MAX_DEPTH * GAP_THREADS];
    const uint32_t e = blockIdx.x * GAP_THREADS + threadIdx.x;
    if (e >= n_table) return;
    const unsigned long long key = keys[e];
    const uint32_t low = (uint32_t)key;
    if (low == 0xFFFFFFFFu) return;
    uint32_t a = 0u, rem = e;
    while (a + 2u < K && rem >= K - 1u - a) { rem -= K - 1u - a; a++; }
    const uint32_t b = a + 1u + rem;
    const uint32_t second = low >> 31, node = low & 0x7FFFFFFFu;
    const GapInstance &from = table[second ? b : a], &to = table[second ? a : b];
    if (b >= K || node >= from.D.n || !to.D.below) return;      // (never)
    const float gap = __uint_as_float((uint32_t)(key >> 32));
    const NodeRec r = from.D.nodes[node];
    uint32_t cx, cy, cz;
    const int depth = cell_climb(from.D.nodes, from.D.n, node, (int32_t)r.x, cx, cy, cz);
    const float scale = __int_as_float((127 - depth) << 23);
    const uint32_t in8 = inside_bits(r.z, r.w);
    const float D = gap_bound(gap, to.I.M.s);
    Nearest best;
    best.visited = 0u;
    uint32_t corner = 0u, k = 0u;
    float wx = 0.0f, wy = 0.0f, wz = 0.0f;
    bool found = false;
    for (int t = 0; t < 6 && !found; t++) {
        const uint32_t corners = tet_corners(t);
        const uint32_t en = MESH_TRIANGLES[t * 16 + (int)tet_mask(in8, t)];
        const uint32_t nt = en & 3u;
        for (uint32_t j = 0; j < nt && !found; j++, k++)
            for (uint32_t v = 0; v < 3u && !found; v++) {
                uint32_t lo, hi;
                float x, y, z, rr, near[3];
                gap_vertex(r, scale, cx, cy, cz, corners, en, j, v, lo, hi, x, y, z);
                gap_forward(from.I.M, x, y, z, wx, wy, wz);
                if (gap_radius(to, wx, wy, wz, D, stack + threadIdx.x, best, rr, near) && __float_as_uint(rr) == (uint32_t)(key >> 32)) {
                    found = true;
                    corner = 3u * k + v;
                }
            }
    }
    if (!found) return;                                         // (never: the key's value is some vertex's of this cell)
    float rr, near[3], fx, fy, fz;
    if (!gap_radius(to, wx, wy, wz, __int_as_float(0x7F800000), stack + threadIdx.x, best, rr, near)) return;     // (never)
    gap_forward(to.I.M, near[0], near[1], near[2], fx, fy, fz);
    const bool held = compose_instance_value(to.I, wx, wy, wz) < 0.0f || compose_instance_value(from.I, fx, fy, fz) < 0.0f;
    GapRecord *R = out + e;
    R->a = a; R->b = b; R->gap = gap;
    R->flags = second | (held ? 2u : 0u);
    R->corner = corner;
    if (!second) {
        R->node_a = node; R->node_b = best.node;
        R->point_a[0] = wx; R->point_a[1] = wy; R->point_a[2] = wz;
        R->point_b[0] = fx; R->point_b[1] = fy; R->point_b[2] = fz;
    } else {
        R->node_b = node; R->node_a = best.node;
        R->point_b[0] = wx; R->point_b[1] = wy; R->point_b[2] = wz;
        R->point_a[0] = fx; R->point_a[1] = fy; R->point_a[2] = fz;
    }
    R->pad[0] = 0u; R->pad[1] = 0u; R->pad[2] = 0u;
}

}  // namespace sdfhip
