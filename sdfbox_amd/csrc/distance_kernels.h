// The exact distance from a point to the surface a resident scene describes (gfx950): the nearest-surface search, the clearance
// query built on it, and the value and level pass of offset and shell.  Included by distance.hip and, for the search, by blend.hip:
// k_dist_mark, which is not a template, is `static` -- each of the two translation units has its own.  Host side, C ABI: distance.hip.
//
// Replaces: nothing in the reference's code -- its field is only ever read as stored, a distance in a thin band round the surface.
//
// The rule is the contract of include/sdfhip.h (sdfhip_scene_distance, sdfhip_scene_offset) and DESIGN.md section 8 (N13): fp32, each
// operation rounded on its own, in the order written (-ffp-contract=off); tests/distance_restatement.py restates it with numpy, by
// brute force.  The surface is sdfhip_scene_mesh's triangles: the cells, their tetrahedra and the cut vertices are cell_tets.h's, read
// by the mesh and by this search alike; the distance to a triangle is tri_dist.h's, the mesh builder's; the sign is
// sdfhip_scene_sample's distance (find_fresh + sample_after_find, raymarch_device.h, untouched) at the point clamped to the cube.
//
//   k_dist_mark     (a) one lane per node: a cut cell of the level sets its bit of the "surface below" bitmap and climbs its parent
//                   links, setting bits, until it meets one already set (whoever set that one goes on to the root).  Bit sets commute:
//                   the bitmap does not depend on which wave ran first
//   nearest_search  (b) one lane per point, depth first from the root, the children of a node nearest first; a child is skipped when
//                   its bit is clear or its box cannot hold anything nearer than the best so far (box_gap2 and SEARCH_KEEP below: the
//                   margin and its derivation); at a cut cell the lane recomputes the cell's triangles and folds tri_dist2 into the best
//   k_offset_level  (c) level_kernels.h's level_body with value(p) = dist(p) - delta, or fabsf(dist(p)) - thickness / 2; the rest
//                   of a level (the scan, k_level_emit) is level_build.h's
//   k_dist_query    (d) n points in, n sdfhip_clearance records out, a grid-stride loop over the same search
//
// The search's stack.  A lane that descends from a node keeps {the node's children block, the children not yet looked at} for its way
// back: one entry per level, MESH_MAX_DEPTH entries of 8 bytes.  Indexed by the depth, which differs from lane to lane, an array in
// registers would go to scratch; it lives in LDS instead, one slice per lane, laid out [level][lane] (a wave's access to one level is
// 64 consecutive 8-byte words: no bank is met twice within a half-wave): 12 x 256 x 8 = 24 KiB per workgroup of 256, six workgroups
// in a compute unit's 160 KiB.  The coordinates of the node a lane is at need no stack: a descent shifts the octant's bits in, the way
// back shifts them out.
#pragma once
#include "query_kernels.h"   // QueryScene, grid_of, finite3, record_store; raymarch_device.h: the cursors, find_fresh, sample_after_find
#include "level_kernels.h"   // LevelBlock, LEVEL_THREADS, level_body
#include "cell_tets.h"       // the cells, their tetrahedra and triangles, cut_position
#include "tri_dist.h"        // tri_dist2

namespace sdfhip {

constexpr int DIST_THREADS = 256;
enum { OFFSET_GROW = 0, OFFSET_SHELL = 1 };                  // SDFHIP_OFFSET_* of include/sdfhip.h

// what the search reads of the scene: the records, the bitmap of (a) -- ceil(n / 32) + 1 words, the last one zero -- and the level
struct DistScene {
    const NodeRec *nodes;
    uint32_t n;
    const uint32_t *below;
    int32_t level;
};

// (a).  `below` was zeroed.  The climb is bounded as node_depth's is: the host side refuses trees that are not consistent.
static __global__ __launch_bounds__(DIST_THREADS) void k_dist_mark(const NodeRec *__restrict__ nodes, uint32_t n, int level, uint32_t *__restrict__ below)
{
    for (uint64_t j = (uint64_t)blockIdx.x * DIST_THREADS + threadIdx.x; j < n; j += (uint64_t)gridDim.x * DIST_THREADS) {
        const NodeRec r = nodes[j];
        // the mesh's own test (k_mesh_emit): mixed bytes, and a cell of the level
        const uint32_t in8 = inside_bits(r.z, r.w);
        if (!is_cut_cell(nodes, n, r, level, in8)) continue;
        uint32_t cur = (uint32_t)j;
        int32_t parent = (int32_t)r.x;
        for (int d = 0; d <= MESH_MAX_DEPTH; d++) {
            const uint32_t bit = 1u << (cur & 31u);
            if (atomicOr(&below[cur >> 5], bit) & bit) break;
            if (parent < 0 || (uint32_t)parent >= n) break;
            cur = (uint32_t)parent;
            parent = (int32_t)nodes[cur].x;
        }
    }
}

// The best triangle so far: its tri_dist2, its cell's node and its index among the cell's triangles -- (node, tri) ascending is the
// mesh's emitted order, and of the triangles that tie on d2 the lowest in that order is kept -- and r = p - q of tri_dist2.
struct Nearest {
    float d2;
    uint32_t node, tri;
    float rx, ry, rz;
    uint32_t visited;          // records the search loaded
};

// ---- the pruning margin ------------------------------------------------------------------------------------------------------
// A box is skipped iff box_gap2(box) * SEARCH_KEEP > best.  That must imply t > best for the tri_dist2 value t of EVERY triangle of
// every cell inside the box: only then can no such triangle lower the minimum or win a tie.  Derivation (u = 2^-24, the unit
// roundoff; a node's box [lo, hi] per axis has exact fp32 bounds, (float)c * S with c < 2^13 and S a power of two):
//  1. A cut vertex lies in its cell's closed box: t of cut_position is in (0, 1) (|63.75 - b_lo| < |b_hi - b_lo|, and the quotient
//     is at most 254.75 / 255 < 1 - u), (float)c + t rounds into [c, c + 1] because rounding is monotone and both ends are floats,
//     and the scaling by S is exact.  A cell's box lies in its ancestors' boxes.
//  2. tri_dist2 returns t = fl(|r|^2), r = fl(p - q), where q is its computed closest point.  In the vertex regions q is a vertex.
//     In the edge regions the parameter is a quotient x / (x + y) of non-negative floats, so it rounds into [0, 1], and
//     q = a + (b - a) * v is three roundings of values of magnitude at most 1 away from a point of the segment: |q - hull| <= 3u per
//     axis.  In the face region q = (a + ab * v) + ac * w with v = vb * den, w = vc * den: where the computed va, vb, vc are all
//     non-negative v, w and v + w round into [0, 1 + 2u] and q is within 8u per axis of the triangle.  (Where rounding leaves the
//     face branch with a negative va, vb or vc -- exact arithmetic excludes it; in which triangles and for which points rounding
//     allows it is not worked out here -- q is not bounded by this argument.  DESIGN.md N13 says so.)
//     So q lies in the box widened by SEARCH_SLACK = 2^-20 = 16u per side, twice what the argument needs.
//  3. box_gap2 computes, per axis, g = max(fl(fl(max(lo - p, p - hi)) - SLACK), 0): two roundings, so g <= G (1 + u)^2 with G the
//     exact gap from p to the widened box; then fl(fl(gx gx + gy gy) + gz gz): a product and two sums of non-negative terms.  Hence
//     gap2 <= |p - widened box|^2 (1 + u)^7.
//  4. t = fl(|r|^2) with r = fl(p - q): t >= |p - q|^2 (1 - u)^5 >= |p - widened box|^2 (1 - u)^5.
//  5. Together t >= gap2 (1 - u)^5 / (1 + u)^7 > gap2 (1 - 13u).  SEARCH_KEEP = 1 - 2^-19 = 1 - 32u, and the product
//     gap2 * SEARCH_KEEP is itself rounded once (1 + u): gap2 * SEARCH_KEEP rounded <= gap2 (1 - 31u) < t.  So
//     gap2 * SEARCH_KEEP > best implies t > best.  A gap2 that overflows is taken as FLT_MAX, for which the chain still holds
//     (t >= FLT_MAX (1 - 13u) in that case); a gap that underflows was clamped to 0 by the slack first.
//  6. A point so far away that every tri_dist2 overflows has d2 = +inf, and no finite best would ever prune its search.  Such a
//     point is answered without a search: with g the gaps to the root's box scaled by 2^-32 (exact), s = fl(|g|^2) >= 2^65 means
//     |p - q|^2 >= 2^129 (1 - 7u) for every q in the widened cube, so the sum of squares in tri_dist2, whose terms are not
//     negative, passes FLT_MAX and rounds to +inf.
constexpr float SEARCH_SLACK = 0x1p-20f;
constexpr float SEARCH_KEEP = 1.0f - 0x1p-19f;

// one axis of box_gap2: the squared gap from p to [lo - SLACK, hi + SLACK]
__device__ __forceinline__ float axis_gap2(float p, float lo, float hi)
{
    const float g = fmaxf(fmaxf(lo - p, p - hi) - SEARCH_SLACK, 0.0f);
    return g * g;
}

// The triangles of the cut cell `node` (record r, depth `depth`, integer coordinates c) against p, folded into the best so far
__device__ __forceinline__ void fold_cell(const NodeRec &r, uint32_t node, int depth, uint32_t cx, uint32_t cy, uint32_t cz, float px, float py,
                                          float pz, Nearest &best)
{
    const float scale = __int_as_float((127 - depth) << 23);                            // 2^-depth
    const uint32_t in8 = inside_bits(r.z, r.w);
    uint32_t k = 0;
    for (int t = 0; t < 6; t++) {
        const uint32_t corners = tet_corners(t);
        const uint32_t e = MESH_TRIANGLES[t * 16 + (int)tet_mask(in8, t)];
        const uint32_t nt = e & 3u;
        for (uint32_t j = 0; j < nt; j++, k++) {
            float T[9];
#pragma unroll
            for (int v = 0; v < 3; v++) {
                const uint32_t ij = (e >> (4u + 4u * (3u * j + (uint32_t)v))) & 15u;
                const uint32_t lo = (corners >> (4u * (ij & 3u))) & 7u, hi = (corners >> (4u * (ij >> 2))) & 7u;
                cut_position(r.z, r.w, scale, cx, cy, cz, lo, hi, T[3 * v], T[3 * v + 1], T[3 * v + 2]);
            }
            float rx, ry, rz;
            int region;
            const float d = tri_dist2(T, px, py, pz, rx, ry, rz, region);
            // (a NaN never wins; within a cell k ascends, so a tie inside it keeps the first; across cells the lower node wins)
            if (d < best.d2 || (d == best.d2 && node < best.node)) {
                best.d2 = d; best.node = node; best.tri = k;
                best.rx = rx; best.ry = ry; best.rz = rz;
            }
        }
    }
}

// the bits of the eight siblings base .. base + 7 in the bitmap (which has one word more than the nodes need)
__device__ __forceinline__ uint32_t sibling_bits(const uint32_t *__restrict__ below, uint32_t base)
{
    const uint32_t w = base >> 5, s = base & 31u;
    uint32_t bits = below[w] >> s;
    if (s > 24u) bits |= below[w + 1] << (32u - s);
    return bits & 0xFFu;
}

// (b).  stk: the lane's slice of the workgroup's stack, stk[level * THREADS].  best.d2 = +inf when no triangle was nearer than +inf
// (an empty surface, or a point so far away that every distance overflows); then node and r mean nothing.
template <int THREADS>
__device__ __forceinline__ void nearest_search(const DistScene &D, float px, float py, float pz, uint2 *stk, Nearest &best)
{
    best.d2 = __int_as_float(0x7F800000);
    best.node = 0xFFFFFFFFu; best.tri = 0u;
    best.rx = 0.0f; best.ry = 0.0f; best.rz = 0.0f;
    best.visited = 0u;
    if (!(D.below[0] & 1u)) return;
    {                                                       // (6 above)
        const float k = 0x1p-32f;
        const float fx = fmaxf(fmaxf(0.0f - px, px - 1.0f) - SEARCH_SLACK, 0.0f) * k, fy = fmaxf(fmaxf(0.0f - py, py - 1.0f) - SEARCH_SLACK, 0.0f) * k,
                    fz = fmaxf(fmaxf(0.0f - pz, pz - 1.0f) - SEARCH_SLACK, 0.0f) * k;
        if ((fx * fx + fy * fy) + fz * fz >= 0x1p65f) return;
    }
    const NodeRec root = D.nodes[0];
    best.visited = 1u;
    if (is_cell((int32_t)root.y, D.level, 0)) { fold_cell(root, 0u, 0, 0u, 0u, 0u, px, py, pz, best); return; }
    // the node the lane is at: depth d, coordinates c, its children block `base`, and the children still to look at
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
        // the nearest of the children still to look at: child c's box is [2 cx + c_x, 2 cx + c_x + 1] * S per axis (exact)
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
        if (fminf(near2, 3.402823466e+38f) * SEARCH_KEEP > best.d2) { todo = 0u; continue; }      // the nearest cannot win: none of the rest can
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
        // an internal node above the level's cells: down, if the tree allows it (the guards only bind on a tree the host side
        // would have refused)
        if ((int32_t)r.y < 0 || (uint64_t)r.y + 8u > D.n || d + 1 >= MESH_MAX_DEPTH) continue;
        stk[d * THREADS] = make_uint2(base, todo);
        d++;
        cx = nx; cy = ny; cz = nz;
        base = r.y;
        todo = sibling_bits(D.below, base);
    }
}

// sign(p) of the rule: negative iff the distance sdfhip_scene_sample returns at p clamped to the cube is below zero
template <class CursorT>
__device__ __forceinline__ bool inside_at(const QueryScene &Q, float px, float py, float pz)
{
    const float cx = __builtin_fminf(__builtin_fmaxf(px, 0.0f), 1.0f);
    const float cy = __builtin_fminf(__builtin_fmaxf(py, 0.0f), 1.0f);
    const float cz = __builtin_fminf(__builtin_fmaxf(pz, 0.0f), 1.0f);
    CursorT c;
    c.loads = 0;
    c.reset(Q.nodes[0]);
    typename CursorT::Pos u;
    find_fresh(c, Q.nodes, grid_of(Q), Q.n_nodes, nullptr, 0u, cx, cy, cz, u);
    return sample_after_find(c, u, cx, cy, cz) < 0.0f;
}

// dist(p) of the rule: sign(p) * sqrtf(d2(p))
template <class CursorT, int THREADS>
__device__ __forceinline__ float dist_at(const QueryScene &Q, const DistScene &D, float px, float py, float pz, uint2 *stk, Nearest &best)
{
    nearest_search<THREADS>(D, px, py, pz, stk, best);
    const float sign = inside_at<CursorT>(Q, px, py, pz) ? -1.0f : 1.0f;
    return sign * sqrtf(best.d2);
}

// The offset's value.  mode: OFFSET_GROW value = dist - amount; OFFSET_SHELL value = fabsf(dist) - amount, amount = thickness * 0.5f
// (the host's one multiplication).
template <class CursorT> struct OffsetValue {
    static constexpr int SOURCES = 1;
    QueryScene Q;
    DistScene D;
    int mode;
    float amount;
    unsigned long long *visited;
    __device__ __forceinline__ float operator()(float px, float py, float pz, uint2 *stk, uint32_t *seen) const
    {
        Nearest best;
        const float dist = dist_at<CursorT, LEVEL_THREADS>(Q, D, px, py, pz, stk, best);
        seen[0] = best.visited;
        return mode == OFFSET_SHELL ? fabsf(dist) - amount : dist - amount;
    }
};

template <class CursorT>
__global__ __launch_bounds__(LEVEL_THREADS) void k_offset_level(QueryScene Q, DistScene D, int mode, float amount, const LevelBlock *__restrict__ blocks,
                                                                uint32_t nblocks, uint32_t nchild, float S, int may_split, uint2 *__restrict__ V,
                                                                uint8_t *__restrict__ split, unsigned long long *__restrict__ visited)
{
    __shared__ uint2 stack[MESH_MAX_DEPTH * LEVEL_THREADS];
    level_body(OffsetValue<CursorT>{Q, D, mode, amount, visited}, blocks, nblocks, nchild, S, may_split, V, split, stack + threadIdx.x);
}

// (d) xyz: n x 3 floats, packed; out: n sdfhip_clearance records as two uint4 {distance, node, nearest.x, nearest.y | nearest.z,
// status, visited, 0}.  A non-finite coordinate: SDFHIP_QUERY_INVALID and zeros, nothing searched.
template <class CursorT>
__global__ __launch_bounds__(DIST_THREADS) void k_dist_query(QueryScene Q, DistScene D, const float *__restrict__ xyz, uint32_t n, uint4 *__restrict__ out)
{
    __shared__ uint2 stack[MESH_MAX_DEPTH * DIST_THREADS];
    for (uint64_t i = (uint64_t)blockIdx.x * DIST_THREADS + threadIdx.x; i < n; i += (uint64_t)gridDim.x * DIST_THREADS) {
        const float px = xyz[3 * i], py = xyz[3 * i + 1], pz = xyz[3 * i + 2];
        uint4 a = make_uint4(0u, 0u, 0u, 0u), b = make_uint4(0u, (uint32_t)QUERY_INVALID, 0u, 0u);
        if (finite3(px, py, pz)) {
            Nearest best;
            const float dist = dist_at<CursorT, DIST_THREADS>(Q, D, px, py, pz, stack + threadIdx.x, best);
            const bool found = best.d2 < __int_as_float(0x7F800000);          // (d2 is never a NaN: one never wins)
            const float qx = found ? px - best.rx : 0.0f, qy = found ? py - best.ry : 0.0f, qz = found ? pz - best.rz : 0.0f;
            a = make_uint4(__float_as_uint(dist), found ? best.node : 0u, __float_as_uint(qx), __float_as_uint(qy));
            b = make_uint4(__float_as_uint(qz), (uint32_t)QUERY_HIT, best.visited, 0u);
        }
        record_store<true>(out + 2 * i, a);
        record_store<true>(out + 2 * i + 1, b);
    }
}

}  // namespace sdfhip
