// The workgroup scan and the bitmap rank that the tree rewriters share, and the chunk scan, the wave sums and the ordered offset of
// the passes over a scene's cells (mesh, slice; the lane rank is the edit's and the prune's), and the axis sums of a wave that is a
// block of a lattice (clash, components) (gfx950).  Everything here is a template or
// __device__ __forceinline__, so any .hip may include it -- unlike the kernel headers (edit_kernels.h, prune_kernels.h, ...), whose
// kernels are not templates and which are therefore included by one translation unit ONLY.  That rule stays: a kernel that is not a
// template does not belong here.
//
// The rank of a set bit (the set bits before it) comes from two launches over the bitmap's words 0 .. m - 1:
//   k_rank_scan_words    256 threads, 4 words each: per word, the set bits of the words before it in its chunk of 1024 (pre[]),
//                        and per chunk its total (chunk[])
//   k_rank_scan_chunks   one workgroup: the chunks' totals -> their exclusive prefix, in place
//   rank_in_bitmap       chunk[] + pre[] + the bits below it in its own word
// (sdfgen_kernels.h's k_scan_sums / k_scan_apply are another form -- wave shuffles, the report to page-locked memory -- on the
// point-cloud builder's measured path, and stay there.)
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

namespace sdfhip {

// Exclusive scan of one value per thread over a workgroup of THREADS (inclusive Hillis-Steele in sh[THREADS]); total = the sum of
// all.  Every thread of the workgroup calls it; it ends with a barrier, so sh may be used again at once (a loop of scans).
template <class T, uint32_t THREADS> __device__ __forceinline__ T block_exclusive_scan(T v, T *sh, T &total)
{
    const uint32_t t = threadIdx.x;
    sh[t] = v;
    __syncthreads();
    for (uint32_t d = 1; d < THREADS; d <<= 1) {
        const T add = t >= d ? sh[t - d] : T(0);
        __syncthreads();
        sh[t] += add;
        __syncthreads();
    }
    total = sh[THREADS - 1];
    const T excl = sh[t] - v;
    __syncthreads();
    return excl;
}

// words(i): word i of the bitmap being ranked, 0 <= i < m (a functor, by value: the edit's window of its split bitmap, the
// prune's complement of removed[])
template <class Words> __global__ __launch_bounds__(256) void k_rank_scan_words(Words words, uint32_t m, uint32_t *__restrict__ pre,
                                                                                uint32_t *__restrict__ chunk)
{
    __shared__ uint32_t part[256];
    const uint32_t t = threadIdx.x, first = blockIdx.x * 1024u + 4u * t;
    uint32_t c[4], sum = 0;
#pragma unroll
    for (int k = 0; k < 4; k++) { c[k] = first + k < m ? (uint32_t)__popc(words(first + k)) : 0u; sum += c[k]; }
    uint32_t total;
    uint32_t run = block_exclusive_scan<uint32_t, 256>(sum, part, total);
#pragma unroll
    for (int k = 0; k < 4; k++) { if (first + k < m) pre[first + k] = run; run += c[k]; }
    if (t == 255) chunk[blockIdx.x] = total;
}

// ... the chunks' totals -> exclusive prefix, in one workgroup (at most 65 536 chunks: 2^31 nodes).  TOTAL: chunk[nchunk] = the
// sum of all (the array then has nchunk + 1 entries)
template <bool TOTAL> __global__ __launch_bounds__(1024) void k_rank_scan_chunks(uint32_t *__restrict__ chunk, uint32_t nchunk)
{
    __shared__ uint32_t part[1024];
    const uint32_t t = threadIdx.x, per = (nchunk + 1023u) / 1024u, lo = t * per;
    uint32_t sum = 0;
    for (uint32_t k = 0; k < per; k++) if (lo + k < nchunk) sum += chunk[lo + k];
    uint32_t total;
    uint32_t run = block_exclusive_scan<uint32_t, 1024>(sum, part, total);
    for (uint32_t k = 0; k < per; k++) if (lo + k < nchunk) { const uint32_t v = chunk[lo + k]; chunk[lo + k] = run; run += v; }
    if (TOTAL && t == 1023) chunk[nchunk] = total;
}

// ... the same with the sums in 64 bits and the grand total at *total (at most 2^21 chunks of 1024: 2^31 nodes): the scan of the
// cell passes (count -> scan -> emit: mesh_kernels.h, slice_kernels.h).  The low words are the offsets the emit uses, which the
// host side only launches when the total fits 31 bits.  A pass's header keeps the total as its first member.
template <class Total> __global__ __launch_bounds__(1024) void k_scan_chunk_totals(uint32_t *__restrict__ chunk, uint32_t nchunk, Total *__restrict__ total_out)
{
    __shared__ Total part[1024];
    const uint32_t t = threadIdx.x, per = (nchunk + 1023u) / 1024u, lo = t * per;
    Total sum = 0;
    for (uint32_t k = 0; k < per; k++) if (lo + k < nchunk) sum += chunk[lo + k];
    Total total;
    Total run = block_exclusive_scan<Total, 1024>(sum, part, total);
    for (uint32_t k = 0; k < per; k++) if (lo + k < nchunk) { const uint32_t v = chunk[lo + k]; chunk[lo + k] = (uint32_t)run; run += v; }
    if (t == 1023) *total_out = total;
}

// ---- within a wave, and from a wave to its workgroup ------------------------------------------------------------------------------

// a lane's rank among the set bits of the ballot m: the set bits below its own
__device__ __forceinline__ uint32_t lane_rank(unsigned long long m)
{
    return __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
}

__device__ __forceinline__ uint32_t wave_sum(uint32_t v)
{
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += (uint32_t)__shfl_xor((int)v, o);
    return v;
}
// inclusive prefix sum over the wave's lanes
__device__ __forceinline__ uint32_t wave_scan(uint32_t v)
{
    const uint32_t lane = threadIdx.x & 63u;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t u = (uint32_t)__shfl_up((int)v, o);
        if (lane >= (uint32_t)o) v += u;
    }
    return v;
}

// A wave that is a 4 x 4 x 4 block of a lattice, lane = lz * 16 + ly * 4 + lx (clash_kernels.h, components_kernels.h): of the lanes of
// the ballot `both`, along the axis whose lanes with coordinate 0 are `base` and whose neighbours are `step` lanes apart, the lowest
// / highest coordinate j in 0..3 and the sum of j -- scalar arithmetic on the one 64-bit word, no cross-lane reduction
__device__ __forceinline__ void block_axis(unsigned long long both, unsigned long long base, int step, uint32_t &lo, uint32_t &hi, uint32_t &sum)
{
    lo = 3u; hi = 0u; sum = 0u;
#pragma unroll
    for (int j = 3; j >= 0; j--)
        if (both & (base << (j * step))) lo = (uint32_t)j;
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const unsigned long long m = both & (base << (j * step));
        if (m) hi = (uint32_t)j;
        sum += (uint32_t)j * (uint32_t)__popcll(m);
    }
}

// The first output index of a lane that writes cnt records in lane order: incl = wave_scan(cnt); totals[w] = wave w's last incl, stored
// to LDS before a barrier; run = the first index of the row's first wave on entry, of the next row's on return.  The order is the
// lanes', whichever wave ran first.
template <uint32_t WAVES> __device__ __forceinline__ uint32_t ordered_first(uint32_t incl, uint32_t cnt, const uint32_t (&totals)[WAVES], uint32_t wave,
                                                                            uint32_t &run)
{
    uint32_t first = run + incl - cnt;
#pragma unroll
    for (uint32_t w = 0; w < WAVES; w++) {
        if (w < wave) first += totals[w];
        run += totals[w];
    }
    return first;
}

// The set bits before bit `bit` of the bitmap's word w_rel (counted from the first word that was scanned), whose value is `word`
__device__ __forceinline__ uint32_t rank_in_bitmap(const uint32_t *__restrict__ chunk, const uint32_t *__restrict__ pre, uint32_t w_rel,
                                                   uint32_t word, uint32_t bit)
{
    return chunk[w_rel >> 10] + pre[w_rel] + (uint32_t)__popc(word & ((1u << bit) - 1u));
}

}  // namespace sdfhip
