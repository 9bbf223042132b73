// The cells of a resident scene and their Kuhn tetrahedra (gfx950): what surface extraction (mesh_kernels.h), the measure
// (measure_kernels.h), the cross-sections (slice_kernels.h) and the nearest-surface search (distance_kernels.h, so blend.hip too)
// share, so that the contracts read one definition -- which nodes are cells of a level and which of those are cut, which corners
// are inside, the six tetrahedra and their triangles, where a cut edge's vertex sits, the climb for a node's depth and coordinates,
// the record a pass streams.  Non-template device helpers and one constant table; no kernel.  The rule is N7's (include/sdfhip.h, sdfhip_scene_mesh).
#pragma once
#include "raymarch_device.h"

namespace sdfhip {

constexpr int MESH_MAX_DEPTH = LM;                            // the deepest tree the walk is sized for (checked by the host side)

// The six tetrahedra round the diagonal 0-7, one per axis permutation in lexicographic order: corners {0, v1, v2, 7} with
// v1 = 1 << a0, v2 = v1 | 1 << a1.  Packed four bits per local corner.
__device__ __forceinline__ uint32_t tet_corners(int t)
{
    // (x,y,z) 0137  (x,z,y) 0157  (y,x,z) 0237  (y,z,x) 0267  (z,x,y) 0457  (z,y,x) 0467
    const uint32_t v1 = 0x442211u, v2 = 0x656353u;
    return 0x7000u | (((v2 >> (4 * t)) & 7u) << 8) | (((v1 >> (4 * t)) & 7u) << 4);
}

// The triangles of (tetrahedron, inside mask): bits 0-1 their number; vertex k of the (up to) six at bits 4 + 4k: the cut edge's
// local corners i (bits 0-1) < j (bits 2-3).  Cut edges in ascending (i, j) order for one or three inside corners, the quad
// (i0,o0) (i0,o1) (i1,o1) (i1,o0) split along its first diagonal for two; the last two vertices of a triangle swapped where the
// orientation test on the unit tetrahedron with cuts at the edge midpoints asks for it (counter-clockwise seen from outside:
// dot(cross(p1 - p0, p2 - p0), mean(outside corners) - mean(inside corners)) > 0).  Worked out once from that rule; the
// restatement derives its own and the GPU tests compare the vertices.
static __device__ const uint32_t MESH_TRIANGLES[6 * 16] = {
    0x0000000u, 0x000c841u, 0x0009d41u, 0x9d8dc82u, 0x000e981u, 0xe94ce42u, 0x8e4ed42u, 0x000edc1u, 0x000dec1u, 0xde4e842u, 0xec49e42u, 0x0009e81u, 0xcd8d982u, 0x000d941u, 0x0008c41u, 0x0000000u,
    0x0000000u, 0x0008c41u, 0x000d941u, 0xd98cd82u, 0x0009e81u, 0x9e4ec42u, 0xe84de42u, 0x000dec1u, 0x000edc1u, 0xed48e42u, 0xce4e942u, 0x000e981u, 0xdc89d82u, 0x0009d41u, 0x000c841u, 0x0000000u,
    0x0000000u, 0x0008c41u, 0x000d941u, 0xd98cd82u, 0x0009e81u, 0x9e4ec42u, 0xe84de42u, 0x000dec1u, 0x000edc1u, 0xed48e42u, 0xce4e942u, 0x000e981u, 0xdc89d82u, 0x0009d41u, 0x000c841u, 0x0000000u,
    0x0000000u, 0x000c841u, 0x0009d41u, 0x9d8dc82u, 0x000e981u, 0xe94ce42u, 0x8e4ed42u, 0x000edc1u, 0x000dec1u, 0xde4e842u, 0xec49e42u, 0x0009e81u, 0xcd8d982u, 0x000d941u, 0x0008c41u, 0x0000000u,
    0x0000000u, 0x000c841u, 0x0009d41u, 0x9d8dc82u, 0x000e981u, 0xe94ce42u, 0x8e4ed42u, 0x000edc1u, 0x000dec1u, 0xde4e842u, 0xec49e42u, 0x0009e81u, 0xcd8d982u, 0x000d941u, 0x0008c41u, 0x0000000u,
    0x0000000u, 0x0008c41u, 0x000d941u, 0xd98cd82u, 0x0009e81u, 0x9e4ec42u, 0xe84de42u, 0x000dec1u, 0x000edc1u, 0xed48e42u, 0xce4e942u, 0x000e981u, 0xdc89d82u, 0x0009d41u, 0x000c841u, 0x0000000u,
};

// bit k: corner k is inside (byte <= 63; the surface is at 63.75, which no byte equals)
__device__ __forceinline__ uint32_t inside_bits(uint32_t v0, uint32_t v1)
{
    uint32_t m = 0;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        m |= (((v0 >> (8 * k)) & 0xFFu) <= 63u ? 1u : 0u) << k;
        m |= (((v1 >> (8 * k)) & 0xFFu) <= 63u ? 1u : 0u) << (4 + k);
    }
    return m;
}
// the four inside bits of tetrahedron t's local corners
__device__ __forceinline__ uint32_t tet_mask(uint32_t in8, int t)
{
    const uint32_t c = tet_corners(t);
    return (in8 & 1u) | (((in8 >> ((c >> 4) & 7u)) & 1u) << 1) | (((in8 >> ((c >> 8) & 7u)) & 1u) << 2) | (((in8 >> 7) & 1u) << 3);
}
// triangles of a cell with these inside bits: per tetrahedron 1 for one or three inside corners, 2 for two
__device__ __forceinline__ uint32_t cell_triangles(uint32_t in8)
{
    uint32_t n = 0;
#pragma unroll
    for (int t = 0; t < 6; t++) {
        const uint32_t pc = (uint32_t)__popc(tet_mask(in8, t));
        n += pc == 2u ? 2u : (pc & 1u);
    }
    return n;
}

// The position of the vertex on the cut edge from cube corner lo to cube corner hi (the bits of lo are a subset of hi's) of the cell
// with bytes (v0, v1), integer coordinates (cx, cy, cz) of its depth and edge `scale`: the surface's crossing at byte 63.75 along the
// edge.  The emitted position of sdfhip_scene_mesh (cut_vertex, mesh_kernels.h) and the triangle corner the nearest-surface search
// recomputes (distance_kernels.h): one definition, so the two are the same bits.
__device__ __forceinline__ void cut_position(uint32_t v0, uint32_t v1, float scale, uint32_t cx, uint32_t cy, uint32_t cz, uint32_t lo, uint32_t hi,
                                             float &px, float &py, float &pz)
{
    const unsigned long long bytes = ((unsigned long long)v1 << 32) | v0;
    const float b_lo = (float)(uint32_t)((bytes >> (8u * lo)) & 0xFFull), b_hi = (float)(uint32_t)((bytes >> (8u * hi)) & 0xFFull);
    const float t = (63.75f - b_lo) / (b_hi - b_lo);
    const uint32_t d = lo ^ hi;
    px = ((float)(cx + (lo & 1u)) + ((d & 1u) ? t : 0.0f)) * scale;
    py = ((float)(cy + ((lo >> 1) & 1u)) + ((d & 2u) ? t : 0.0f)) * scale;
    pz = ((float)(cz + ((lo >> 2) & 1u)) + ((d & 4u) ? t : 0.0f)) * scale;
}

// depth of node i: the links up to the root (mixed nodes of a level >= 0 pass only)
__device__ __forceinline__ int node_depth(const NodeRec *__restrict__ nodes, uint32_t n, int32_t parent)
{
    int d = 0;
    while (parent >= 0 && (uint32_t)parent < n && d <= MESH_MAX_DEPTH) {
        parent = (int32_t)nodes[parent].x;
        d++;
    }
    return d;
}

// ... and, for the passes that place the cell, its integer coordinates of that depth too: the octant within the parent is index -
// parent.children, three bits per level.  The same bound and the same links as node_depth, so the two agree on every tree.
__device__ __forceinline__ int cell_climb(const NodeRec *__restrict__ nodes, uint32_t n, uint32_t i, int32_t parent, uint32_t &cx, uint32_t &cy, uint32_t &cz)
{
    int depth = 0;
    cx = 0; cy = 0; cz = 0;
    while (parent >= 0 && (uint32_t)parent < n && depth <= MESH_MAX_DEPTH) {
        const uint2 p = *reinterpret_cast<const uint2 *>(nodes + parent);        // {its parent, its children}
        const uint32_t oct = i - p.y;
        cx |= (oct & 1u) << depth; cy |= ((oct >> 1) & 1u) << depth; cz |= ((oct >> 2) & 1u) << depth;
        i = (uint32_t)parent;
        parent = (int32_t)p.x;
        depth++;
    }
    return depth;
}

// Record i as a cell pass streams it.  Past the end: an internal node with no parent and bytes 0.  Every user also tests i < n
// before it counts or emits anything, so what stands past the end decides nothing: bytes of 0xFF (no inside corner) would do as well.
__device__ __forceinline__ NodeRec cell_record(const NodeRec *__restrict__ nodes, uint32_t n, uint32_t i)
{
    return i < n ? nodes[i] : make_uint4(0xFFFFFFFFu, 0u, 0u, 0u);
}

// is node (children, depth) a cell of `level`: -1 = the leaves; L = the leaves of depth <= L and the internal nodes of depth L
__device__ __forceinline__ bool is_cell(int32_t children, int level, int depth)
{
    const bool leaf = children < 0;
    return level < 0 ? leaf : (leaf ? depth <= level : depth == level);
}
// ... for a pass that has not climbed: the links are walked only where the level needs the depth
__device__ __forceinline__ bool is_cell(const NodeRec *__restrict__ nodes, uint32_t n, const NodeRec &r, int level)
{
    return level < 0 ? (int32_t)r.y < 0 : is_cell((int32_t)r.y, level, node_depth(nodes, n, (int32_t)r.x));
}
// are the bytes mixed (some corner inside, some outside): a cell is cut when they are.  is_cut_cell tests the bytes first, so
// that only mixed nodes walk
__device__ __forceinline__ bool is_mixed(uint32_t in8) { return in8 != 0u && in8 != 0xFFu; }
__device__ __forceinline__ bool is_cut_cell(const NodeRec *__restrict__ nodes, uint32_t n, const NodeRec &r, int level, uint32_t in8)
{
    return is_mixed(in8) && is_cell(nodes, n, r, level);
}

}  // namespace sdfhip
