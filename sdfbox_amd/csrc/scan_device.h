// The workgroup scan and the bitmap rank that the tree rewriters share (gfx950).  Everything here is a template or
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

// The set bits before bit `bit` of the bitmap's word w_rel (counted from the first word that was scanned), whose value is `word`
__device__ __forceinline__ uint32_t rank_in_bitmap(const uint32_t *__restrict__ chunk, const uint32_t *__restrict__ pre, uint32_t w_rel,
                                                   uint32_t word, uint32_t bit)
{
    return chunk[w_rel >> 10] + pre[w_rel] + (uint32_t)__popc(word & ((1u << bit) - 1u));
}

}  // namespace sdfhip
