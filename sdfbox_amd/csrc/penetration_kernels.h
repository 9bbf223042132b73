// The penetration depth of an assembly of placed instances (gfx950): how far each overlapping pair of parts reaches into the other,
// where, and which way to push.  k_pen_contain (the clash check's containment pass, as a count and as an emit of the (point, part)
// searches to run), k_pen_search (one exact nearest-surface search per item), k_pen_fold (the pair table) and k_pen_witness (the
// records).  Host side, C ABI: penetration.hip.
//
// Replaces: nothing in the reference's code -- its shader marches ONE immutable tree and knows no parts.
//
// The rule is the contract of include/sdfhip.h (sdfhip_instances_penetration) and DESIGN.md section 8 (N22): fp32, each operation
// rounded on its own, in the order written (-ffp-contract=off); tests/penetration_restatement.py restates it with numpy, by brute force.
//   lattice, index, contains   sdfhip_instances_clash's, word for word (clash_kernels.h)
//   r_k(p)      q = the placement's inverse map of p (place_value's first three lines: d = p - t, q = (R^T d) * inv, no clamp);
//               r_k(p) = sqrtf(d2_k(q)) * s_k, d2_k = sdfhip_scene_distance's d2 on instance k's source at level -1 (nearest_search of
//               distance_kernels.h: the minimum of tri_dist2, a NaN never wins, +inf for an empty surface).  Unsigned: containment is
//               the clash rule's, no sign function is involved
//   depth(a, b) the maximum of fminf(r_a(p), r_b(p)) over the lattice points both contain; witness = the lowest index attaining it
//   nearest     q - r of the search (lowest (node, tri) on ties), mapped forward: ((r[i][0] x + r[i][1] y) + r[i][2] z) * s + t_i
// Integers only.  The maximum is taken with a 64-bit atomicMax on the key (float bits << 32) | (0xFFFFFFFF - index): the values are
// >= 0 and never NaN, so their bits are monotone, and of two points with the same value the lower index has the larger key.  points
// is an integer atomicAdd.  No float is ever accumulated as a float: two calls give the same bytes.
//
// Steps 1 and 2 of k_clash (candidates by the exact skip, look-ups) are RESTATED in k_pen_contain, not shared: k_clash is an ordinary
// (non-template, external) kernel of clash_kernels.h, so that header cannot be included by a second translation unit, and moving its
// steps into a device function of a shared header would recompile k_clash -- its resource line (profiles/clash_kernel_resources.txt)
// is a committed measurement.  tests/test_gpu_penetration.py holds `points` of every record to the clash check's.
//
// Shape.
//   k_pen_contain<false>  a wave per 4 x 4 x 4 block: the containment mask of every lane; a lane inside >= 2 parts has popcount(mask)
//                         searches to run.  The wave's total goes to one 64-bit counter, the parts it names into a 64-bit mask
//                         (atomicOr), the look-up counters to slots as the clash check's
//   k_pen_contain<true>   the same pass again (a value depends on the point alone: the masks are the same); the wave reserves its run
//                         of the item array with one atomicAdd and writes {index, k, -, -}, point-major, a point's items consecutive
//                         in ascending k.  WHERE a wave's run lands depends on timing; no output does: the fold keys on (a, b) and the
//                         index, and `visited` is a sum.  Overlaps are sparse: this compaction keeps the search waves full
//   k_pen_search          one lane per item, grid-stride: p from the index, q, nearest_search with the LDS stack slice laid out
//                         [level][lane] as k_dist_query has it; r is stored into the item.  The DistScene is per lane
//   k_pen_fold            one lane per item: fminf(r_i, r_j) with every later item j of its point's run into pair (k_i, k_j)
//   k_pen_witness         one lane per (pair, side): the search again at the witness; ra / rb, the cells and the nearest points
#pragma once
#include "compose_instance.h"   // ComposeInstance, compose_instance_value, place_lower_bound
#include "distance_kernels.h"   // DistScene, Nearest, nearest_search, k_dist_mark (static: this unit's own)

namespace sdfhip {

constexpr int PEN_THREADS = 256;
constexpr uint32_t PEN_MAX_INSTANCES = 64, PEN_STAT_SLOTS = 64;

// one entry of the call's table: the clash check's, and what the search reads of the same source (D.below null until it is marked)
struct PenInstance {
    ComposeInstance I;
    DistScene D;
};

// one search: lattice point `index` against instance k; r = r_k(p) once k_pen_search has run
struct PenItem {
    uint32_t index, k;
    float r;
    uint32_t pad;
};
static_assert(sizeof(PenItem) == 16, "the host allocates 16 bytes per search");

// one entry of the pair table, zeroed: points == 0 is "no record", and every key of a point is above 0
struct PenPair {
    unsigned long long key;     // (bits of fminf(r_a, r_b) << 32) | (0xFFFFFFFF - index)
    uint32_t points, pad;
};

// sdfhip_penetration of include/sdfhip.h
struct PenRecord {
    uint32_t a, b, points, witness;
    float depth, ra, rb;
    uint32_t node_a, node_b;
    float nearest_a[3], nearest_b[3];
    uint32_t pad;
};
static_assert(sizeof(PenRecord) == 64, "sdfhip_penetration of include/sdfhip.h");

struct PenStat {
    unsigned long long lookups;
    uint32_t blocks_looked, pad;
};

// the call's counters, zeroed
struct PenCounters {
    unsigned long long searches;    // the count pass: sum of popcount(mask) over the points inside >= 2 parts
    unsigned long long cursor;      // the emit pass: the item array's fill (== searches afterwards)
    unsigned long long visited;     // the records k_pen_search loaded
    unsigned long long searched;    // the instances that have at least one search
    PenStat slot[PEN_STAT_SLOTS];
};

// the call's lattice as the kernels read it (the clash check's)
struct PenLattice {
    float ox, oy, oz, pitch;
    uint32_t depth;         // 0..10
    uint32_t n_blocks;      // 8^max(depth - 2, 0)
    uint32_t n_instances;   // 1..64
    uint32_t skip;          // 0: SDFHIP_PENETRATION_NO_SKIP
};

// entry a * K - a (a + 1) / 2 + (b - a - 1) of the table is pair (a, b), a < b < K (clash_kernels.h's clash_pair_index)
__device__ __forceinline__ uint32_t pen_pair_index(uint32_t a, uint32_t b, uint32_t K) { return a * K - a * (a + 1u) / 2u + (b - a - 1u); }

// lattice point `index`: p_a = fmaf((float)i_a + 0.5f, pitch, origin_a)
__device__ __forceinline__ void pen_point(const PenLattice &L, uint32_t index, float &px, float &py, float &pz)
{
    const uint32_t d = L.depth, m = (1u << d) - 1u;
    const uint32_t x = index & m, y = (index >> d) & m, z = index >> (2u * d);
    px = __builtin_fmaf((float)x + 0.5f, L.pitch, L.ox);
    py = __builtin_fmaf((float)y + 0.5f, L.pitch, L.oy);
    pz = __builtin_fmaf((float)z + 0.5f, L.pitch, L.oz);
}

// the placement's inverse map: place_value's first three lines, no clamp
__device__ __forceinline__ void pen_inverse(const PlaceMap &M, float px, float py, float pz, float &qx, float &qy, float &qz)
{
    const float d0 = px - M.tx, d1 = py - M.ty, d2 = pz - M.tz;
    qx = ((M.r[0][0] * d0 + M.r[1][0] * d1) + M.r[2][0] * d2) * M.inv;
    qy = ((M.r[0][1] * d0 + M.r[1][1] * d1) + M.r[2][1] * d2) * M.inv;
    qz = ((M.r[0][2] * d0 + M.r[1][2] * d1) + M.r[2][2] * d2) * M.inv;
}

template <bool EMIT>
__global__ __launch_bounds__(PEN_THREADS) void k_pen_contain(const PenInstance *__restrict__ table, PenLattice L, PenCounters *__restrict__ C,
                                                             PenItem *__restrict__ items, unsigned long long n_items)
{
    const uint32_t block = blockIdx.x * (PEN_THREADS / 64) + (threadIdx.x >> 6);        // wave-uniform
    if (block >= L.n_blocks) return;
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t d = L.depth, bd = d > 2u ? d - 2u : 0u, bmask = (1u << bd) - 1u;
    const uint32_t bx = (block & bmask) * 4u, by = ((block >> bd) & bmask) * 4u, bz = (block >> (2u * bd)) * 4u;
    const uint32_t x = bx + (lane & 3u), y = by + ((lane >> 2) & 3u), z = bz + (lane >> 4);
    const uint32_t side = 1u << d;
    const bool inside = x < side && y < side && z < side;
    const float px = __builtin_fmaf((float)x + 0.5f, L.pitch, L.ox), py = __builtin_fmaf((float)y + 0.5f, L.pitch, L.oy),
                pz = __builtin_fmaf((float)z + 0.5f, L.pitch, L.oz);
    const uint32_t K = L.n_instances;

    // 1  candidates (k_clash's step 1)
    unsigned long long cand = 0ull, wave_cand = 0ull;
    for (uint32_t k = 0; k < K; k++) {
        bool c = inside;
        if (L.skip) c = c && !(place_lower_bound(table[k].I.M, px, py, pz) >= 0.0f);
        if (c) cand |= 1ull << k;
        if (__ballot(c)) wave_cand |= 1ull << k;
    }
    if (L.skip && __popcll(wave_cand) < 2) return;

    // 2  look-ups (k_clash's step 2)
    unsigned long long held = 0ull, lookups = 0ull;
    for (unsigned long long left = wave_cand; left; left &= left - 1ull) {
        const uint32_t k = (uint32_t)__ffsll((long long)left) - 1u;
        const bool c = (cand >> k) & 1ull;
        bool in = false;
        if (c) in = compose_instance_value(table[k].I, px, py, pz) < 0.0f;
        if (in) held |= 1ull << k;
        lookups += (unsigned long long)__popcll(__ballot(c));
    }
    if (!EMIT && lane == 0u && lookups) {
        PenStat *s = C->slot + (block & (PEN_STAT_SLOTS - 1u));
        atomicAdd(&s->lookups, lookups);
        atomicAdd(&s->blocks_looked, 1u);
    }

    // 3  the searches of each lane, and the lanes' inclusive scan
    const uint32_t parts = (uint32_t)__popcll(held), mine = parts >= 2u ? parts : 0u;
    uint32_t incl = mine;
    for (uint32_t o = 1u; o < 64u; o <<= 1) {
        const uint32_t v = __shfl_up(incl, o);
        if (lane >= o) incl += v;
    }
    const uint32_t total = __shfl(incl, 63);
    if (total == 0u) return;
    if (!EMIT) {
        unsigned long long searched = 0ull;
        for (uint32_t k = 0; k < K; k++)
            if (__ballot(mine != 0u && ((held >> k) & 1ull))) searched |= 1ull << k;
        if (lane == 0u) {
            atomicAdd(&C->searches, (unsigned long long)total);
            atomicOr(&C->searched, searched);
        }
        return;
    }
    uint32_t lo = 0u, hi = 0u;
    if (lane == 0u) {
        const unsigned long long base = atomicAdd(&C->cursor, (unsigned long long)total);
        lo = (uint32_t)base; hi = (uint32_t)(base >> 32);
    }
    lo = __shfl(lo, 0); hi = __shfl(hi, 0);
    unsigned long long at = (((unsigned long long)hi << 32) | lo) + (incl - mine);
    const uint32_t index = (z << (2u * d)) | (y << d) | x;
    for (unsigned long long left = mine ? held : 0ull; left; left &= left - 1ull, at++) {
        const uint32_t k = (uint32_t)__ffsll((long long)left) - 1u;
        if (at < n_items) items[at] = PenItem{index, k, 0.0f, 0u};      // (always: the count pass counted the same masks)
    }
}

// r_k(p) of every item.  visited: the lanes' sums, one atomicAdd per wave
__global__ __launch_bounds__(PEN_THREADS) void k_pen_search(const PenInstance *__restrict__ table, PenLattice L, PenItem *__restrict__ items,
                                                            unsigned long long n_items, PenCounters *__restrict__ C)
{
    __shared__ uint2 stack[MESH_MAX_DEPTH * PEN_THREADS];
    unsigned long long seen = 0ull;
    for (uint64_t i = (uint64_t)blockIdx.x * PEN_THREADS + threadIdx.x; i < n_items; i += (uint64_t)gridDim.x * PEN_THREADS) {
        const PenItem it = items[i];
        if (it.k >= L.n_instances || !table[it.k].D.below) continue;        // (never: the emit pass wrote every item, of marked sources)
        float px, py, pz, qx, qy, qz;
        pen_point(L, it.index, px, py, pz);
        const PlaceMap M = table[it.k].I.M;
        pen_inverse(M, px, py, pz, qx, qy, qz);
        const DistScene D = table[it.k].D;
        Nearest best;
        nearest_search<PEN_THREADS>(D, qx, qy, qz, stack + threadIdx.x, best);
        items[i].r = sqrtf(best.d2) * M.s;
        seen += best.visited;
    }
    uint32_t lo = (uint32_t)seen, hi = (uint32_t)(seen >> 32);
    unsigned long long sum = seen;
    for (uint32_t o = 32u; o; o >>= 1) {
        const uint32_t vlo = __shfl_xor(lo, o), vhi = __shfl_xor(hi, o);
        sum += ((unsigned long long)vhi << 32) | vlo;
        lo = (uint32_t)sum; hi = (uint32_t)(sum >> 32);
    }
    if ((threadIdx.x & 63u) == 0u && sum) atomicAdd(&C->visited, sum);
}

// the pair table: item i with every later item of its point (their k ascend, so k_i < k_j)
__global__ __launch_bounds__(PEN_THREADS) void k_pen_fold(const PenItem *__restrict__ items, unsigned long long n_items, uint32_t K,
                                                          PenPair *__restrict__ pairs)
{
    for (uint64_t i = (uint64_t)blockIdx.x * PEN_THREADS + threadIdx.x; i < n_items; i += (uint64_t)gridDim.x * PEN_THREADS) {
        const PenItem it = items[i];
        for (uint64_t j = i + 1u; j < n_items; j++) {
            const PenItem other = items[j];
            if (other.index != it.index) break;
            if (!(it.k < other.k && other.k < K)) break;    // (never)
            const float v = fminf(it.r, other.r);
            const unsigned long long key = ((unsigned long long)__float_as_uint(v) << 32) | (unsigned long long)(0xFFFFFFFFu - it.index);
            PenPair *P = pairs + pen_pair_index(it.k, other.k, K);
            atomicMax(&P->key, key);
            atomicAdd(&P->points, 1u);
        }
    }
}

// the records: lane 2 e + side for entry e of the pair table; side 0 writes the pair's own fields and part a's, side 1 part b's.
// `out` was zeroed: an entry without points stays zero.  A side whose part has no surface (r = +inf): node 0, nearest 0
__global__ __launch_bounds__(PEN_THREADS) void k_pen_witness(const PenInstance *__restrict__ table, PenLattice L, const PenPair *__restrict__ pairs,
                                                             uint32_t n_table, PenRecord *__restrict__ out)
{
    __shared__ uint2 stack[MESH_MAX_DEPTH * PEN_THREADS];
    const uint32_t t = blockIdx.x * PEN_THREADS + threadIdx.x;
    if (t >= 2u * n_table) return;
    const uint32_t e = t >> 1, second = t & 1u, K = L.n_instances;
    const PenPair P = pairs[e];
    if (!P.points) return;
    uint32_t a = 0u, rem = e;
    while (a + 2u < K && rem >= K - 1u - a) { rem -= K - 1u - a; a++; }
    const uint32_t b = a + 1u + rem;
    const uint32_t k = second ? b : a;
    if (k >= K || !table[k].D.below) return;                 // (never)
    const uint32_t index = 0xFFFFFFFFu - (uint32_t)P.key;
    float px, py, pz, qx, qy, qz;
    pen_point(L, index, px, py, pz);
    const PlaceMap M = table[k].I.M;
    pen_inverse(M, px, py, pz, qx, qy, qz);
    const DistScene D = table[k].D;
    Nearest best;
    nearest_search<PEN_THREADS>(D, qx, qy, qz, stack + threadIdx.x, best);
    const float r = sqrtf(best.d2) * M.s;
    const bool found = best.d2 < __int_as_float(0x7F800000);
    float w[3] = {0.0f, 0.0f, 0.0f};
    if (found) {
        const float nx = qx - best.rx, ny = qy - best.ry, nz = qz - best.rz;
        w[0] = ((M.r[0][0] * nx + M.r[0][1] * ny) + M.r[0][2] * nz) * M.s + M.tx;
        w[1] = ((M.r[1][0] * nx + M.r[1][1] * ny) + M.r[1][2] * nz) * M.s + M.ty;
        w[2] = ((M.r[2][0] * nx + M.r[2][1] * ny) + M.r[2][2] * nz) * M.s + M.tz;
    }
    PenRecord *R = out + e;
    const uint32_t node = found ? best.node : 0u;
    if (!second) {
        R->a = a; R->b = b; R->points = P.points; R->witness = index;
        R->depth = __uint_as_float((uint32_t)(P.key >> 32));
        R->ra = r; R->node_a = node;
        R->nearest_a[0] = w[0]; R->nearest_a[1] = w[1]; R->nearest_a[2] = w[2];
        R->pad = 0u;
    } else {
        R->rb = r; R->node_b = node;
        R->nearest_b[0] = w[0]; R->nearest_b[1] = w[1]; R->nearest_b[2] = w[2];
    }
}

}  // namespace sdfhip
