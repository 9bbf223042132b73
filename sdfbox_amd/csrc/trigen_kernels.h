// Kernels of sdfhip_trimesh_build (trigen.hip): the exact signed distance of a triangle mesh, level by level.
//
// A BLOCK is the eight children of one node (the root's block: the root alone, as child 0 of a cell of edge 2 at the origin).  Its
// 35 points are the 27 corners of its 3x3x3 lattice (spacing S, the children's edge) and the 8 child centres: every corner and
// centre of the eight siblings, each evaluated once.  A block carries the candidate list it inherited from its parent.
//   k_tri_eval    a workgroup per block: the list's records are staged through LDS a chunk at a time (one coalesced gather per
//                 chunk), every wave takes 64 of them, lane = point; the waves' (D, list position) minima meet in LDS; then the
//                 bytes, the centre distances and the split flags
//   k_tri_count   lanes over the list: which of the block's splitting children keeps the record (one mask byte per entry), and
//                 the children's list lengths
//   k_tri_scan_*  exclusive scans of the split flags (-> the children blocks' ranks) and of the list lengths (-> their offsets)
//   k_tri_fill    a wave per block: the next level's lists (stable: ascending record index, so a tie keeps going to the lowest
//                 record), block descriptors and parent / children links
// The arithmetic of tri_dist2 and of the value in k_tri_eval is the pinned rule of include/sdfhip.h, operation for operation (-ffp-contract=off).
#pragma once
#include "sdf_bytes.h"
#include "scan_device.h"     // block_exclusive_scan
#include "tri_dist.h"        // tri_dot, tri_dist2

namespace sdfhip {

constexpr int TRI_REC = 32;               // floats per record
constexpr int TRI_POINTS = 35;
constexpr int TRI_COUNT_THREADS = 256;
constexpr int TRI_SCAN_THREADS = 256, TRI_SCAN_CHUNK = 1024;

struct TriBlock {                         // 32 bytes
    uint32_t x, y, z;                     // the parent cell's integer coordinates at its own depth
    uint32_t first;                       // index of child 0 within the level
    unsigned long long off;               // the candidate list: list[off .. off + cnt)
    uint32_t cnt, nchild;                 // nchild: 8, or 1 for the root
};

// tri_dot and tri_dist2 (D of the rule, r = p - q and the region): tri_dist.h, shared with the nearest-surface search

// point `p` of a block: 0..26 lattice corner i + 3j + 9k, 27..34 the centre of child p - 27
__device__ __forceinline__ void tri_point(const TriBlock &B, int p, float S, float &px, float &py, float &pz)
{
    if (p < 27) {
        px = (float)(2u * B.x + (uint32_t)(p % 3)) * S;
        py = (float)(2u * B.y + (uint32_t)(p / 3 % 3)) * S;
        pz = (float)(2u * B.z + (uint32_t)(p / 9)) * S;
    } else {
        const uint32_t c = (uint32_t)(p - 27);
        const float H = S * 0.5f;
        px = (float)(2u * (2u * B.x + (c & 1u)) + 1u) * H;
        py = (float)(2u * (2u * B.y + (c >> 1 & 1u)) + 1u) * H;
        pz = (float)(2u * (2u * B.z + (c >> 2 & 1u)) + 1u) * H;
    }
}

// NW waves per block.  V, cdist, split: the level's arrays (values, |value(centre)|, 1 where the node splits).
template <int NW>
__global__ __launch_bounds__(64 * NW) void k_tri_eval(const float *__restrict__ records, const uint32_t *__restrict__ list,
                                                      const TriBlock *__restrict__ blocks, float S, int may_split, uint2 *V,
                                                      float *cdist, uint32_t *split)
{
    constexpr int CH = 64 * NW;                       // records per chunk
    __shared__ float sRec[CH][9];                     // a, b, c (an odd stride: the staging stores meet no bank twice)
    __shared__ uint32_t sIdx[CH];
    __shared__ float sD[NW][TRI_POINTS];
    __shared__ uint32_t sPos[NW][TRI_POINTS];
    __shared__ float sVal[TRI_POINTS];
    const TriBlock B = blocks[blockIdx.x];
    const int lane = (int)(threadIdx.x & 63u), wave = (int)(threadIdx.x >> 6);
    const int p = lane < TRI_POINTS ? lane : 0;       // (the idle lanes follow point 0 and write nothing)
    float px, py, pz;
    tri_point(B, p, S, px, py, pz);

    float bestD = INFINITY, brx = 0.0f, bry = 0.0f, brz = 0.0f;
    uint32_t bestPos = 0xFFFFFFFFu, bestRec = 0;
    int bestRegion = 0;
    for (uint32_t base = 0; base < B.cnt; base += CH) {
        const uint32_t m = min((uint32_t)CH, B.cnt - base);
        __syncthreads();                              // the chunk before is read
        if (threadIdx.x < m) {
            const uint32_t ri = list[B.off + base + threadIdx.x];
            const float4 *src = reinterpret_cast<const float4 *>(records + (size_t)ri * TRI_REC);
            const float4 r0 = src[0], r1 = src[1], r2 = src[2];
            float *dst = sRec[threadIdx.x];
            dst[0] = r0.x; dst[1] = r0.y; dst[2] = r0.z; dst[3] = r0.w; dst[4] = r1.x; dst[5] = r1.y; dst[6] = r1.z; dst[7] = r1.w;
            dst[8] = r2.x;
            sIdx[threadIdx.x] = ri;
        }
        __syncthreads();
        const uint32_t lo = (uint32_t)wave * 64u, hi = min(lo + 64u, m);
        for (uint32_t t = lo; t < hi; t++) {
            float rx, ry, rz; int region;
            const float D = tri_dist2(sRec[t], px, py, pz, rx, ry, rz, region);
            if (D < bestD) { bestD = D; bestPos = base + t; bestRec = sIdx[t]; brx = rx; bry = ry; brz = rz; bestRegion = region; }
        }
    }
    if (lane < TRI_POINTS) { sD[wave][lane] = bestD; sPos[wave][lane] = bestPos; }
    __syncthreads();
    if (lane < TRI_POINTS) {
        int w = 0;                                    // the wave that holds the winner: smallest D, then the lowest list position
        float wD = sD[0][lane]; uint32_t wPos = sPos[0][lane];
        for (int k = 1; k < NW; k++) {
            const float D = sD[k][lane]; const uint32_t pos = sPos[k][lane];
            if (D < wD || (D == wD && pos < wPos)) { w = k; wD = D; wPos = pos; }
        }
        if (w == wave) {
            float value = INFINITY;                   // no winner (an empty list, or NaN everywhere)
            if (bestPos != 0xFFFFFFFFu) {
                const float *N = records + (size_t)bestRec * TRI_REC + 9 + 3 * bestRegion;
                const float s = tri_dot(brx, bry, brz, N[0], N[1], N[2]);
                const float d = sqrtf(bestD);
                value = s < 0.0f ? -d : d;
            }
            sVal[lane] = value;
        }
    }
    __syncthreads();
    if (threadIdx.x < B.nchild) {
        const int c = (int)threadIdx.x, ci = c & 1, cj = c >> 1 & 1, ck = c >> 2 & 1;
        uint32_t b[8];
        for (int k = 0; k < 8; k++) b[k] = from_float(sVal[(ci + (k & 1)) + 3 * (cj + (k >> 1 & 1)) + 9 * (ck + (k >> 2 & 1))], S);
        V[B.first + c] = make_uint2(b[0] | b[1] << 8 | b[2] << 16 | b[3] << 24, b[4] | b[5] << 8 | b[6] << 16 | b[7] << 24);
        const float cv = fabsf(sVal[27 + c]);
        cdist[B.first + c] = cv;
        split[B.first + c] = (cv < 2.0f * S && may_split) ? 1u : 0u;
    }
}

// Which records can own a point of child c's cell: those whose computed distance to its centre m is at most
// (the smallest computed distance to m) + 2h + slack, h the cell's half diagonal (DESIGN.md N8 derives it).  prune = 0: all.
// mask[off + j] bit c; cnt[node] = the child's list length (0 where it does not split).
__global__ __launch_bounds__(TRI_COUNT_THREADS) void k_tri_count(const float *__restrict__ records, const uint32_t *__restrict__ list,
                                                                const TriBlock *__restrict__ blocks, float S, int prune, float slack_abs,
                                                                const float *__restrict__ cdist, const uint32_t *__restrict__ split,
                                                                uint8_t *mask, uint32_t *cnt)
{
    __shared__ float sT[8];
    __shared__ uint32_t sSplit[8], sCnt[8];
    const TriBlock B = blocks[blockIdx.x];
    if (threadIdx.x < 8) {
        const bool live = threadIdx.x < B.nchild && split[B.first + threadIdx.x] != 0;
        float T = INFINITY;
        if (live && prune) {
            const float reach = cdist[B.first + threadIdx.x] + 2.0f * (S * 0.8660255f);      // 0.8660255f > sqrt(3) / 2
            T = reach + (slack_abs + reach * 0.0009765625f);
        }
        sT[threadIdx.x] = T; sSplit[threadIdx.x] = live ? 1u : 0u; sCnt[threadIdx.x] = 0;
    }
    __syncthreads();
    uint32_t any = 0;
    for (int c = 0; c < 8; c++) any |= sSplit[c];
    if (any) {
        uint32_t mine[8] = { 0, 0, 0, 0, 0, 0, 0, 0 };
        for (uint32_t j = threadIdx.x; j < B.cnt; j += TRI_COUNT_THREADS) {
            const uint32_t ri = list[B.off + j];
            const float4 *src = reinterpret_cast<const float4 *>(records + (size_t)ri * TRI_REC);
            const float4 r0 = src[0], r1 = src[1], r2 = src[2];
            const float T9[9] = { r0.x, r0.y, r0.z, r0.w, r1.x, r1.y, r1.z, r1.w, r2.x };
            uint32_t bits = 0;
            for (int c = 0; c < 8; c++) {
                if (!sSplit[c]) continue;
                float px, py, pz, rx, ry, rz; int region;
                tri_point(B, 27 + c, S, px, py, pz);
                const float D = tri_dist2(T9, px, py, pz, rx, ry, rz, region);
                if (!prune || sqrtf(D) <= sT[c]) { bits |= 1u << c; mine[c]++; }
            }
            mask[B.off + j] = (uint8_t)bits;
        }
        for (int c = 0; c < 8; c++)
            if (mine[c]) atomicAdd(&sCnt[c], mine[c]);
    }
    __syncthreads();
    if (threadIdx.x < B.nchild) cnt[B.first + threadIdx.x] = sCnt[threadIdx.x];
}

// ---- exclusive scan of n uint32 into uint64, with the total --------------------------------------------------------------------
// (block_exclusive_scan, scan_device.h, over the workgroup's TRI_SCAN_THREADS partial sums)
__global__ __launch_bounds__(TRI_SCAN_THREADS) void k_tri_scan_sums(const uint32_t *__restrict__ in, uint32_t n, unsigned long long *sums)
{
    __shared__ unsigned long long sh[TRI_SCAN_THREADS];
    const uint32_t i0 = blockIdx.x * TRI_SCAN_CHUNK + threadIdx.x * 4u;
    unsigned long long v = 0;
    for (uint32_t k = 0; k < 4; k++) if (i0 + k < n) v += in[i0 + k];
    unsigned long long total;
    (void)block_exclusive_scan<unsigned long long, TRI_SCAN_THREADS>(v, sh, total);
    if (threadIdx.x == 0) sums[blockIdx.x] = total;
}

// one workgroup: the chunk sums to their exclusive prefixes, in place; *total_out = the sum of all
__global__ __launch_bounds__(TRI_SCAN_THREADS) void k_tri_scan_chunks(unsigned long long *sums, uint32_t nchunk, unsigned long long *total_out)
{
    __shared__ unsigned long long sh[TRI_SCAN_THREADS];
    unsigned long long carry = 0;
    for (uint32_t base = 0; base < nchunk; base += TRI_SCAN_THREADS) {
        const uint32_t i = base + threadIdx.x;
        const unsigned long long v = i < nchunk ? sums[i] : 0ull;
        unsigned long long total;
        const unsigned long long excl = block_exclusive_scan<unsigned long long, TRI_SCAN_THREADS>(v, sh, total);
        if (i < nchunk) sums[i] = carry + excl;
        carry += total;
    }
    if (threadIdx.x == 0) *total_out = carry;
}

__global__ __launch_bounds__(TRI_SCAN_THREADS) void k_tri_scan_apply(const uint32_t *__restrict__ in, uint32_t n,
                                                                    const unsigned long long *__restrict__ sums, unsigned long long *out)
{
    __shared__ unsigned long long sh[TRI_SCAN_THREADS];
    const uint32_t i0 = blockIdx.x * TRI_SCAN_CHUNK + threadIdx.x * 4u;
    uint32_t x[4];
    unsigned long long v = 0;
    for (uint32_t k = 0; k < 4; k++) { x[k] = i0 + k < n ? in[i0 + k] : 0u; v += x[k]; }
    unsigned long long total;
    unsigned long long run = sums[blockIdx.x] + block_exclusive_scan<unsigned long long, TRI_SCAN_THREADS>(v, sh, total);
    for (uint32_t k = 0; k < 4; k++) { if (i0 + k < n) out[i0 + k] = run; run += x[k]; }
}

// A wave per block.  rank / coff: the scans of split / cnt over the level.  base_cur / base_next: the global index of the level's
// (the next level's) first node.  Writes, per splitting child: its children's block descriptor, their candidate list (the records
// whose mask bit is set, in list order), the child's `children` link and the eight new nodes' {parent, -1}.
__global__ __launch_bounds__(64) void k_tri_fill(const uint32_t *__restrict__ list, const uint8_t *__restrict__ mask,
                                                 const TriBlock *__restrict__ blocks, const uint32_t *__restrict__ split,
                                                 const uint32_t *__restrict__ cnt, const unsigned long long *__restrict__ rank,
                                                 const unsigned long long *__restrict__ coff, uint32_t base_cur, uint32_t base_next,
                                                 int2 *S_cur, int2 *S_next, TriBlock *next_blocks, uint32_t *next_list)
{
    const TriBlock B = blocks[blockIdx.x];
    const uint32_t lane = threadIdx.x;
    uint32_t live = 0;                                // bit c: child c splits
    for (uint32_t c = 0; c < B.nchild; c++) live |= (split[B.first + c] ? 1u : 0u) << c;
    if (!live) return;
    if (lane < B.nchild && (live >> lane & 1u)) {
        const uint32_t node = B.first + lane, nb = (uint32_t)rank[node];
        next_blocks[nb] = TriBlock{ 2u * B.x + (lane & 1u), 2u * B.y + (lane >> 1 & 1u), 2u * B.z + (lane >> 2 & 1u), 8u * nb, coff[node],
                                    cnt[node], 8u };
        S_cur[node].y = (int)(base_next + 8u * nb);
        for (uint32_t k = 0; k < 8; k++) S_next[8u * nb + k] = make_int2((int)(base_cur + node), -1);
    }
    unsigned long long at[8];
    for (uint32_t c = 0; c < 8; c++) at[c] = (c < B.nchild && (live >> c & 1u)) ? coff[B.first + c] : 0ull;
    const unsigned long long below = (1ull << lane) - 1ull;
    for (uint32_t base = 0; base < B.cnt; base += 64) {
        const uint32_t j = base + lane;
        const uint32_t bits = j < B.cnt ? mask[B.off + j] : 0u;
        const uint32_t ri = j < B.cnt ? list[B.off + j] : 0u;
        for (uint32_t c = 0; c < 8; c++) {
            if (!(live >> c & 1u)) continue;
            const bool keep = bits >> c & 1u;
            const unsigned long long vote = __ballot(keep);
            if (keep) next_list[at[c] + (unsigned long long)__popcll(vote & below)] = ri;
            at[c] += (unsigned long long)__popcll(vote);
        }
    }
}

__global__ void k_tri_iota(uint32_t *list, uint32_t n)
{
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) list[i] = i;
}

}  // namespace sdfhip
