// The measure of a resident scene (gfx950): volume, area, first and second moments and the tight bounds of the solid that N7's
// marching tetrahedra bound -- sums over cells of closed-form terms, in fp64.  Two kernels: included by measure.hip ONLY.  Host side,
// C ABI: measure.hip.  The cells, the inside bits, the six tetrahedra and the triangle table are cell_tets.h's, shared with the mesh.
//
// Replaces: nothing in the reference's code -- its tree only ever becomes pixels; no call there says anything quantitative about it.
//
// The rule is the contract of include/sdfhip.h (sdfhip_scene_measure) and DESIGN.md section 8 (N12): fp64, each operation rounded on
// its own, in the order written (-ffp-contract=off), the triangle area's root alone in fp32; tests/measure_restatement.py restates it
// with numpy, cell for cell.
//
// The eleven sums must not depend on which wave finished first and use no atomics on doubles: they are the adjacent-pair tree over
// node index (x[i] = node i's contribution, +0.0 for a node that contributes nothing; x = x[0::2] + x[1::2] until one is left).
//   k_measure_cells   one lane per node, MEASURE_CHUNK nodes per workgroup in rows of MEASURE_THREADS consecutive nodes, the 16-byte
//                     records streamed as k_mesh_count streams them.  A cell climbs the links for its depth (cells_at_depth) and its
//                     coordinates; one with an inside corner computes its eleven doubles and its bounds.  A wave folds with xor
//                     shuffles at offsets 1, 2, ..., 32 (adjacent lanes first: the tree), the sixteen (row, wave) results fold
//                     through LDS in the same pairing: one partial of 17 doubles (11 sums, 6 bounds) per chunk.  A wave with no
//                     contributing lane writes +0.0 / +-inf without folding (sums of +0.0 are +0.0).  The counts are integers:
//                     ballots, LDS and one global atomic per counter and workgroup.
//   k_measure_fold    1024 partials -> one, by the same tree (an aligned run of 1024 chunks is a subtree); relaunched until one is
//                     left, which is the result record.
#pragma once
#include "cell_tets.h"

namespace sdfhip {

constexpr int MEASURE_THREADS = 256;
constexpr int MEASURE_ROWS = 4;
constexpr uint32_t MEASURE_CHUNK = MEASURE_THREADS * MEASURE_ROWS;           // 1024 nodes: one partial
constexpr int MEASURE_SUMS = 11;                                             // volume, area, m1 x y z, m2 xx yy zz xy xz yz
constexpr int MEASURE_DOUBLES = MEASURE_SUMS + 6;                            // + bounds min x y z, max x y z
constexpr int MEASURE_FOLD = 1024;                                           // partials per workgroup of k_measure_fold
constexpr int MEASURE_SLOTS = 16;                                            // wave results per workgroup, both kernels

// the result record: the folded doubles, then the counts (cells = the sum of at_depth)
struct MeasureHeader { double v[MEASURE_DOUBLES]; uint32_t cut, inside, at_depth[14]; };

struct D3 { double x, y, z; };
__device__ __forceinline__ D3 sub3(const D3 &a, const D3 &b) { return D3{ a.x - b.x, a.y - b.y, a.z - b.z }; }

// what one lane holds: the sums and the bounds
struct Measure17 {
    double vol, area, m1x, m1y, m1z, xx, yy, zz, xy, xz, yz;
    double lox, loy, loz, hix, hiy, hiz;
};
__device__ __forceinline__ Measure17 measure_nothing()
{
    const double inf = __longlong_as_double(0x7FF0000000000000ll);
    return Measure17{ 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, inf, inf, inf, -inf, -inf, -inf };
}
__device__ __forceinline__ void bound(Measure17 &m, const D3 &p)
{
    m.lox = fmin(m.lox, p.x); m.loy = fmin(m.loy, p.y); m.loz = fmin(m.loz, p.z);
    m.hix = fmax(m.hix, p.x); m.hiy = fmax(m.hiy, p.y); m.hiz = fmax(m.hiz, p.z);
}

// The cell a lane measures: integer coordinates of its depth, S = 2^-depth, the eight bytes
struct MeasureCell { uint32_t cx, cy, cz; double S; unsigned long long bytes; };

// A vertex of a piece, six bits: the cube corners a (bits 0-2) and b (bits 3-5) of one tetrahedron.  a != b: the cut point on that edge
// (the bits of the smaller are a subset of the larger's), N7's vertex in fp64; a == b: the cube corner itself,
// ((double)c_a + bit_a(a)) * S, which is the same expression with nothing added
__device__ __forceinline__ D3 vertex_at(const MeasureCell &c, uint32_t code)
{
    const uint32_t a = code & 7u, b = (code >> 3) & 7u;
    const uint32_t lo = a < b ? a : b, hi = a < b ? b : a;
    const uint32_t d = lo ^ hi;
    double t = 0.0;
    if (d) {
        const double b_lo = (double)(uint32_t)((c.bytes >> (8u * lo)) & 0xFFull), b_hi = (double)(uint32_t)((c.bytes >> (8u * hi)) & 0xFFull);
        t = (63.75 - b_lo) / (b_hi - b_lo);
    }
    return D3{ ((double)(c.cx + (lo & 1u)) + ((d & 1u) ? t : 0.0)) * c.S,
               ((double)(c.cy + ((lo >> 1) & 1u)) + ((d & 2u) ? t : 0.0)) * c.S,
               ((double)(c.cz + ((lo >> 2) & 1u)) + ((d & 4u) ? t : 0.0)) * c.S };
}
__device__ __forceinline__ uint32_t corner_code(uint32_t a) { return a | (a << 3); }
__device__ __forceinline__ uint32_t cut_code(uint32_t a, uint32_t b) { return a | (b << 3); }
__device__ __forceinline__ uint32_t piece_code(uint32_t v0, uint32_t v1, uint32_t v2, uint32_t v3) { return v0 | (v1 << 6) | (v2 << 12) | (v3 << 18); }

// the tetrahedron (a, b, c, d) added to the cell-local sums, or (minus) taken from them: x + (-y) is x - y, bit for bit
__device__ __forceinline__ void tetrahedron(Measure17 &m, const D3 &a, const D3 &b, const D3 &c, const D3 &d, bool minus)
{
    const D3 e1 = sub3(b, a), e2 = sub3(c, a), e3 = sub3(d, a);
    const double det = (e1.x * (e2.y * e3.z - e2.z * e3.y) - e1.y * (e2.x * e3.z - e2.z * e3.x)) + e1.z * (e2.x * e3.y - e2.y * e3.x);
    const double V = fabs(det) / 6.0;
    const D3 s = D3{ ((a.x + b.x) + c.x) + d.x, ((a.y + b.y) + c.y) + d.y, ((a.z + b.z) + c.z) + d.z };
    const double q = V * 0.25, w = V * 0.05;
    const double t1x = q * s.x, t1y = q * s.y, t1z = q * s.z;
    const double txx = w * ((((a.x * a.x + b.x * b.x) + c.x * c.x) + d.x * d.x) + s.x * s.x);
    const double tyy = w * ((((a.y * a.y + b.y * b.y) + c.y * c.y) + d.y * d.y) + s.y * s.y);
    const double tzz = w * ((((a.z * a.z + b.z * b.z) + c.z * c.z) + d.z * d.z) + s.z * s.z);
    const double txy = w * ((((a.x * a.y + b.x * b.y) + c.x * c.y) + d.x * d.y) + s.x * s.y);
    const double txz = w * ((((a.x * a.z + b.x * b.z) + c.x * c.z) + d.x * d.z) + s.x * s.z);
    const double tyz = w * ((((a.y * a.z + b.y * b.z) + c.y * c.z) + d.y * d.z) + s.y * s.z);
    m.vol += minus ? -V : V; m.m1x += minus ? -t1x : t1x; m.m1y += minus ? -t1y : t1y; m.m1z += minus ? -t1z : t1z;
    m.xx += minus ? -txx : txx; m.yy += minus ? -tyy : tyy; m.zz += minus ? -tzz : tzz;
    m.xy += minus ? -txy : txy; m.xz += minus ? -txz : txz; m.yz += minus ? -tyz : tyz;
}

// vertex `ij` of MESH_TRIANGLES: the cut edge between the tetrahedron's local corners i (bits 0-1) < j (bits 2-3)
__device__ __forceinline__ D3 table_vertex(const MeasureCell &c, uint32_t corners, uint32_t ij)
{
    return vertex_at(c, cut_code((corners >> (4u * (ij & 3u))) & 7u, (corners >> (4u * (ij >> 2))) & 7u));
}

// a cell with all eight bytes <= 63: the box
__device__ __forceinline__ void measure_box(Measure17 &m, const MeasureCell &c)
{
    const D3 lo = D3{ (double)c.cx * c.S, (double)c.cy * c.S, (double)c.cz * c.S };
    const D3 hi = D3{ ((double)c.cx + 1.0) * c.S, ((double)c.cy + 1.0) * c.S, ((double)c.cz + 1.0) * c.S };
    const double V = (c.S * c.S) * c.S;
    const D3 mid = D3{ (lo.x + hi.x) * 0.5, (lo.y + hi.y) * 0.5, (lo.z + hi.z) * 0.5 };
    m.vol = V;
    m.m1x = V * mid.x; m.m1y = V * mid.y; m.m1z = V * mid.z;
    m.xx = V * (((lo.x * lo.x + lo.x * hi.x) + hi.x * hi.x) / 3.0);
    m.yy = V * (((lo.y * lo.y + lo.y * hi.y) + hi.y * hi.y) / 3.0);
    m.zz = V * (((lo.z * lo.z + lo.z * hi.z) + hi.z * hi.z) / 3.0);
    m.xy = V * (mid.x * mid.y); m.xz = V * (mid.x * mid.z); m.yz = V * (mid.y * mid.z);
    bound(m, lo); bound(m, hi);
}

// a cell with mixed bytes: its six tetrahedra clipped to the inside, their triangles' areas, the bounds of what is added.  One copy
// of the tetrahedron's arithmetic: the pieces of a case are codes (integers), and one loop measures them.
__device__ __forceinline__ void measure_cut(Measure17 &m, const MeasureCell &c, uint32_t in8)
{
#pragma unroll 1
    for (int t = 0; t < 6; t++) {
        const uint32_t corners = tet_corners(t), m4 = tet_mask(in8, t);
        if (m4 == 0u) continue;
        // the tetrahedron's cube corners, the inside ones first, each group in ascending local order: four bits each
        uint32_t ins = 0, outs = 0, nin = 0, nout = 0;
#pragma unroll
        for (uint32_t k = 0; k < 4; k++) {
            const uint32_t cube = (corners >> (4u * k)) & 7u;
            if ((m4 >> k) & 1u) { ins |= cube << (4u * nin); nin++; }
            else { outs |= cube << (4u * nout); nout++; }
        }
        const uint32_t i0 = ins & 7u, i1 = (ins >> 4) & 7u, i2 = (ins >> 8) & 7u, o0 = outs & 7u, o1 = (outs >> 4) & 7u, o2 = (outs >> 8) & 7u;
        const uint32_t whole = piece_code(corner_code(0u), corner_code((corners >> 4) & 7u), corner_code((corners >> 8) & 7u), corner_code(7u));
        uint32_t piece0 = whole, piece1 = 0, piece2 = 0, pieces = 1, minus = 0;
        if (nin == 1u) {
            piece0 = piece_code(corner_code(i0), cut_code(i0, o0), cut_code(i0, o1), cut_code(i0, o2));
        } else if (nin == 3u) {
            piece1 = piece_code(corner_code(o0), cut_code(i0, o0), cut_code(i1, o0), cut_code(i2, o0));
            pieces = 2; minus = 2u;                     // the second is taken away
        } else if (nin == 2u) {
            const uint32_t q0 = cut_code(i0, o0), q1 = cut_code(i0, o1), q2 = cut_code(i1, o1), q3 = cut_code(i1, o0);
            piece0 = piece_code(corner_code(i0), q0, q1, q2);
            piece1 = piece_code(corner_code(i0), q0, q3, q2);
            piece2 = piece_code(corner_code(i0), corner_code(i1), q3, q2);
            pieces = 3;
        }
#pragma unroll 1
        for (uint32_t j = 0; j < pieces; j++) {
            const uint32_t code = j == 0u ? piece0 : (j == 1u ? piece1 : piece2);
            tetrahedron(m, vertex_at(c, code & 63u), vertex_at(c, (code >> 6) & 63u), vertex_at(c, (code >> 12) & 63u), vertex_at(c, (code >> 18) & 63u),
                        ((minus >> j) & 1u) != 0u);
        }
        // the bounds: the inside corners here, the cut points with the triangles below (the table's vertices are all of them)
#pragma unroll 1
        for (uint32_t k = 0; k < nin; k++) bound(m, vertex_at(c, corner_code((ins >> (4u * k)) & 7u)));
        // the area: N7's triangles of this tetrahedron and mask, vertices in the table's order
        const uint32_t e = MESH_TRIANGLES[t * 16 + (int)m4];
        const uint32_t nt = e & 3u;
#pragma unroll 1
        for (uint32_t j = 0; j < nt; j++) {
            const uint32_t e3 = e >> (4u + 12u * j);                             // the triangle's three cut edges, four bits each
            const D3 p0 = table_vertex(c, corners, e3 & 15u), p1 = table_vertex(c, corners, (e3 >> 4) & 15u), p2 = table_vertex(c, corners, (e3 >> 8) & 15u);
            const D3 u = sub3(p1, p0), w = sub3(p2, p0);
            const double nx = u.y * w.z - u.z * w.y, ny = u.z * w.x - u.x * w.z, nz = u.x * w.y - u.y * w.x;
            const double n2 = (nx * nx + ny * ny) + nz * nz;
            m.area += 0.5 * (double)sqrtf((float)n2);
            bound(m, p0); bound(m, p1); bound(m, p2);
        }
    }
}

__device__ __forceinline__ double shfl_xor_f64(double v, int o) { return __shfl_xor(v, o); }

// the wave's lanes folded by the tree (every lane ends with the wave's result)
__device__ __forceinline__ void wave_fold(Measure17 &m)
{
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        m.vol += shfl_xor_f64(m.vol, o); m.area += shfl_xor_f64(m.area, o);
        m.m1x += shfl_xor_f64(m.m1x, o); m.m1y += shfl_xor_f64(m.m1y, o); m.m1z += shfl_xor_f64(m.m1z, o);
        m.xx += shfl_xor_f64(m.xx, o); m.yy += shfl_xor_f64(m.yy, o); m.zz += shfl_xor_f64(m.zz, o);
        m.xy += shfl_xor_f64(m.xy, o); m.xz += shfl_xor_f64(m.xz, o); m.yz += shfl_xor_f64(m.yz, o);
        m.lox = fmin(m.lox, shfl_xor_f64(m.lox, o)); m.loy = fmin(m.loy, shfl_xor_f64(m.loy, o)); m.loz = fmin(m.loz, shfl_xor_f64(m.loz, o));
        m.hix = fmax(m.hix, shfl_xor_f64(m.hix, o)); m.hiy = fmax(m.hiy, shfl_xor_f64(m.hiy, o)); m.hiz = fmax(m.hiz, shfl_xor_f64(m.hiz, o));
    }
}

__device__ __forceinline__ void store_slot(double (*slot)[MEASURE_DOUBLES], int k, const Measure17 &m)
{
    double *s = slot[k];
    s[0] = m.vol; s[1] = m.area; s[2] = m.m1x; s[3] = m.m1y; s[4] = m.m1z; s[5] = m.xx; s[6] = m.yy; s[7] = m.zz; s[8] = m.xy; s[9] = m.xz; s[10] = m.yz;
    s[11] = m.lox; s[12] = m.loy; s[13] = m.loz; s[14] = m.hix; s[15] = m.hiy; s[16] = m.hiz;
}

// The workgroup's sixteen wave results (ascending node index) -> one record of 17 doubles at out: quantity q by thread q, the same
// pairing.  Call after a __syncthreads() behind the stores.
__device__ __forceinline__ void fold_slots(const double (*slot)[MEASURE_DOUBLES], double *__restrict__ out)
{
    const int q = (int)threadIdx.x;
    if (q >= MEASURE_DOUBLES) return;
    double v[MEASURE_SLOTS];
#pragma unroll
    for (int k = 0; k < MEASURE_SLOTS; k++) v[k] = slot[k][q];
#pragma unroll
    for (int width = MEASURE_SLOTS; width > 1; width >>= 1)
#pragma unroll
        for (int k = 0; k < width / 2; k++)
            v[k] = q < MEASURE_SUMS ? v[2 * k] + v[2 * k + 1] : (q < MEASURE_SUMS + 3 ? fmin(v[2 * k], v[2 * k + 1]) : fmax(v[2 * k], v[2 * k + 1]));
    out[q] = v[0];
}

__global__ __launch_bounds__(MEASURE_THREADS) void k_measure_cells(const NodeRec *__restrict__ nodes, uint32_t n, int level, double *__restrict__ partial,
                                                                    MeasureHeader *__restrict__ head)
{
    __shared__ double slot[MEASURE_SLOTS][MEASURE_DOUBLES];
    __shared__ uint32_t hist[16];                       // cells by depth 0..12, [13] spare, [14] cut cells, [15] inside cells
    const uint32_t base = blockIdx.x * MEASURE_CHUNK + threadIdx.x;
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    if (threadIdx.x < 16u) hist[threadIdx.x] = 0u;
    // the next row's record is in flight while this row's cell is measured
    NodeRec ahead = cell_record(nodes, n, base);
    __syncthreads();
    // (one copy of the cell arithmetic, not one per row)
#pragma unroll 1
    for (int k = 0; k < MEASURE_ROWS; k++) {
        const uint32_t i = base + (uint32_t)k * MEASURE_THREADS;
        const NodeRec rec = ahead;
        if (k + 1 < MEASURE_ROWS) ahead = cell_record(nodes, n, i + MEASURE_THREADS);
        const bool leaf = (int32_t)rec.y < 0;
        MeasureCell c;
        c.cx = 0; c.cy = 0; c.cz = 0;
        int depth = 0;
        bool cell = false;
        if (i < n && (level >= 0 || leaf)) {
            depth = cell_climb(nodes, n, i, (int32_t)rec.x, c.cx, c.cy, c.cz);
            cell = is_cell((int32_t)rec.y, level, depth);
        }
        const uint32_t in8 = inside_bits(rec.z, rec.w);
        const bool has = cell && in8 != 0u;
        // the counts: cells by depth (a wave's cells are mostly of one depth: one ballot per depth present), cut and inside cells
        unsigned long long todo = __ballot(cell);
        while (todo) {
            const int lead = __ffsll((long long)todo) - 1;
            const int d = __shfl(depth, lead);
            const unsigned long long same = __ballot(cell && depth == d);
            if (lane == 0u) atomicAdd(&hist[d < 13 ? d : 13], (uint32_t)__popcll(same));
            todo &= ~same;
        }
        const unsigned long long any = __ballot(has), full = __ballot(has && in8 == 0xFFu);
        if (lane == 0u && any) {
            if (any != full) atomicAdd(&hist[14], (uint32_t)__popcll(any & ~full));
            if (full) atomicAdd(&hist[15], (uint32_t)__popcll(full));
        }
        Measure17 m = measure_nothing();
        if (any) {                                      // (wave-uniform)
            if (has) {
                c.S = __longlong_as_double((long long)(1023 - depth) << 52);            // 2^-depth
                c.bytes = ((unsigned long long)rec.w << 32) | rec.z;
                if (in8 == 0xFFu) measure_box(m, c);
                else measure_cut(m, c, in8);
            }
            wave_fold(m);
        }
        if (lane == 0u) store_slot(slot, k * (MEASURE_THREADS / 64) + (int)wave, m);
    }
    __syncthreads();
    fold_slots(slot, partial + (size_t)blockIdx.x * MEASURE_DOUBLES);
    if (threadIdx.x >= 32u && threadIdx.x < 48u) {
        const uint32_t h = threadIdx.x - 32u, v = hist[h];
        if (v) atomicAdd(h < 14u ? &head->at_depth[h] : (h == 14u ? &head->cut : &head->inside), v);
    }
}

// in[0 .. m) -> out[0 .. ceil(m / MEASURE_FOLD)): workgroup b folds the aligned block b of 1024 partials (past the end: +0.0, +-inf)
__global__ __launch_bounds__(MEASURE_FOLD) void k_measure_fold(const double *__restrict__ in, uint32_t m, double *__restrict__ out)
{
    __shared__ double slot[MEASURE_SLOTS][MEASURE_DOUBLES];
    const uint32_t i = blockIdx.x * MEASURE_FOLD + threadIdx.x;
    Measure17 v = measure_nothing();
    if (i < m) {
        const double *p = in + (size_t)i * MEASURE_DOUBLES;
        v = Measure17{ p[0], p[1], p[2], p[3], p[4], p[5], p[6], p[7], p[8], p[9], p[10], p[11], p[12], p[13], p[14], p[15], p[16] };
    }
    wave_fold(v);
    if ((threadIdx.x & 63u) == 0u) store_slot(slot, (int)(threadIdx.x >> 6), v);
    __syncthreads();
    fold_slots(slot, out + (size_t)blockIdx.x * MEASURE_DOUBLES);
}

}  // namespace sdfhip
