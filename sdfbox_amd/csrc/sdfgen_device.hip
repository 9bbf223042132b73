// Point cloud -> ASDF on the GPU: SdfGen's builder (SdfGen/dllmain.cpp:67-207,295-319),
// level-synchronous instead of recursive: a wavefront per block of eight siblings (which share one candidate list), several
// workgroups per node on the first levels.
//
// What the reference does per node (construct, dllmain.cpp:163-190), and where it is here:
//   centerValue = distance from the cell centre to the nearest candidate   k_center_*
//   possible    = candidates within (centerValue + sqrt(3)/2 * scale)       k_center_* (count),
//                 of the centre, in list order                              k_corners_* (stable compaction)
//   corner i    = signed distance to the nearest *surviving* point, unless  k_corners_*
//                 inherited from the parent (child i inherits corner i; an
//                 inherited +inf is recomputed, as every corner still at
//                 INFINITY is, dllmain.cpp:171-172)
//   split       = centerValue < 2 * scale && depth < MaxDepth               k_corners_*
// (levels of fewer than 16 384 nodes: k_center_seg_min / _seg_count, k_corners_seg / _fin -- several workgroups per node;
//  the others: k_center_sib / k_corners_sib -- a wavefront per sibling block, the shared list staged through LDS)
//   children    = 8 new nodes whose candidates are this node's `possible`   k_children
// The recursion becomes a loop over levels; the reference's node order (children blocks
// appended in depth-first pre-order) is restored afterwards, still on the GPU, from subtree
// counts (k_subtree, bottom-up) and pre-order ranks (k_emit, top-down), and k_emit also
// quantises the values as FromFloat / WriteBytes do (dllmain.cpp:192-207): the host receives
// the finished {parent, children} and byte arrays in one copy each.
// Device memory comes from three bump arenas (results that live until the end; per-level
// scratch and candidate lists, ping-ponged between levels), not from one hipMalloc per array.
//
// Bit-exactness with oracle/sdfgen_oracle.c (the CPU restatement): same fp32 expressions
// in the same order, no contraction (-ffp-contract=off), IEEE sqrt and divide; ties in the
// nearest-point search go to the earliest list position, as the reference's strict `<`
// scan does; `minDistance < 0.015` is a double comparison, as there.
#include "sdfgen_kernels.h"
#include "host_support.h"
#include "abi_guard.h"

#include <chrono>
#include <cmath>
#include <cstring>
#include <cstdlib>
#include <sys/mman.h>
#include <new>
#include <vector>

using namespace sdfhip;

namespace {

// scratch: arrays only the level itself and k_children read; keep: what the final ordering needs
bool alloc_level(Arena &scratch, Arena &keep, LevelArrays &L, size_t n)
{
    L.px = scratch.alloc<float>(n); L.py = scratch.alloc<float>(n); L.pz = scratch.alloc<float>(n);
    L.inherit = scratch.alloc<float>(n); L.slot = scratch.alloc<int32_t>(n);
    L.cand_off = scratch.alloc<uint32_t>(n); L.cand_cnt = scratch.alloc<uint32_t>(n);
    L.center_value = scratch.alloc<float>(n); L.pcount = scratch.alloc<uint32_t>(n);
    L.parent = keep.alloc<int32_t>(n); L.vals = keep.alloc<float>(8 * n);
    L.split = keep.alloc<uint32_t>(n); L.block_of = keep.alloc<uint32_t>(n);
    return L.px && L.py && L.pz && L.inherit && L.slot && L.parent && L.cand_off && L.cand_cnt &&
           L.center_value && L.pcount && L.vals && L.split && L.block_of;
}

bool scan_u32(Arena &scratch, const uint32_t *in, uint32_t *out, uint32_t n, const uint32_t *d_err, sdfhip::Report *report, uint32_t seq)
{
    const uint32_t chunks = (n + sdfhip::SCAN_CHUNK - 1) / sdfhip::SCAN_CHUNK;
    uint32_t *sums = scratch.alloc<uint32_t>(chunks);
    if (!sums) return false;
    hipLaunchKernelGGL(sdfhip::k_scan_sums, dim3(chunks), dim3(sdfhip::SCAN_CHUNK), 0, 0, in, sums, n);
    hipLaunchKernelGGL(sdfhip::k_scan_apply, dim3(chunks), dim3(sdfhip::SCAN_CHUNK), 0, 0, in, sums, out, n, d_err, report, seq);
    return true;
}

// Wait for the scan numbered `seq` to have reported: spin on the page-locked word (the kernels in front of it are microseconds to a
// millisecond of work); after 20 ms of that, ask the runtime -- a kernel that faulted never reports, and the runtime says why.
hipError_t wait_report(const sdfhip::Report *report, uint32_t seq)
{
    const auto t0 = std::chrono::steady_clock::now();
    for (uint32_t spins = 0;; spins++) {
        if (report->seq == seq) return hipSuccess;
        cpu_relax();
        if ((spins & 1023u) == 1023u && std::chrono::steady_clock::now() - t0 > std::chrono::milliseconds(20)) break;
    }
    const hipError_t e = hipStreamSynchronize(0);
    if (e != hipSuccess) return e;
    return report->seq == seq ? hipSuccess : hipErrorUnknown;
}

constexpr uint32_t WIDE_LEVEL = 16384;
constexpr unsigned long long WIDE_MAX_LIST = 8192;
struct KeptLevel { LevelArrays L; uint32_t n; uint32_t *cnt, *rank; int32_t *index; };

#define GEN_TRY(expr) HIP_TRY_AS("sdfgen: ", expr, #expr)
#define GEN_NOMEM() fail(SDFHIP_ERR_NOMEM, "sdfgen: out of device memory")

// One build on the current device: what its steps share, and the steps in the order sdfgen_impl calls them.  Everything runs on the
// null stream.
struct Build {
    const float *const verts6;
    const uint32_t n;                                    // points
    const int32_t depth;                                 // MaxDepth
    const std::chrono::steady_clock::time_point t0;
    Arena keep{(size_t)64 << 20}, scratch[2] = { Arena((size_t)32 << 20), Arena((size_t)32 << 20) },
          lists[2] = { Arena((size_t)64 << 20), Arena((size_t)64 << 20) };
    GenParams P;
    float *d_verts = nullptr;
    uint32_t *d_err = nullptr;
    Report *report = nullptr;                            // where the scans report to the host, and their numbering
    uint32_t report_seq = 0;
    LevelArrays L;                                       // the level at hand: its arrays, its candidate lists, its nodes
    Cand *cand = nullptr;
    uint32_t n_nodes = 1;
    unsigned long long cand_entries = n, list_entries = n;      // all lists so far; the lists of the level at hand
    // the levels done, and the tree made from them
    std::vector<KeptLevel> levels;
    size_t total_nodes = 0;
    int32_t *d_S = nullptr;                              // {parent, children} and bytes in the reference's node order
    uint8_t *d_V = nullptr;
    // (SDFHIP_GEN_WIDE=n: the sibling-block form from n nodes on -- tests set 8 to run small trees through it)
    const bool wide_forced = lab_env("SDFHIP_GEN_WIDE") != nullptr;
    const uint32_t wide_level = wide_forced ? (uint32_t)atoi(lab_env("SDFHIP_GEN_WIDE")) : WIDE_LEVEL;
    const uint32_t seg_target = lab_env("SDFHIP_GEN_SEGS") ? (uint32_t)max(1, atoi(lab_env("SDFHIP_GEN_SEGS"))) : 4096u;
    const bool level_timing = lab_env("SDFHIP_GEN_LEVELS") != nullptr;      // debug aid: nodes, entries and time of every level on stderr
    const bool timing = lab_env("SDFHIP_GEN_TIMING") != nullptr;            // debug aid: phase times on stderr
    Build(const float *verts6, uint32_t n, int32_t depth, std::chrono::steady_clock::time_point t0) : verts6(verts6), n(n), depth(depth), t0(t0) {}

    void lap(const char *what) const
    {
        if (!timing) return;
        (void)hipDeviceSynchronize();
        fprintf(stderr, "sdfgen: %-28s at %.2f ms\n", what, std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count());
    }

    // the points on the device, GlobalScale and GlobalOffset from their bounds, the root and its candidate list (every point)
    int start()
    {
        P.max_depth = depth;
        d_verts = keep.alloc<float>(6 * (size_t)n);
        d_err = keep.alloc<uint32_t>(1);
        // (page-locked and mapped; one per host thread, kept for the life of the process: allocating one costs as much as a level)
        static thread_local Report *mine = nullptr;
        report = mine;
        if (!report) {
            //  COHERENT, said explicitly: the host spins on `seq` while the kernel is still running -- without fine-grained
            // coherence (HIP_HOST_COHERENT=0 makes that the default) every wait would burn its whole spin budget before the stream
            // synchronisation behind it; and the numbering starts from zeroed bytes, not from whatever the allocation held
            GEN_TRY(hipHostMalloc((void **)&report, sizeof(Report) + BOUNDS_WG * 6 * sizeof(float),
                                  hipHostMallocPortable | hipHostMallocMapped | hipHostMallocCoherent));
            memset(report, 0, sizeof(Report) + BOUNDS_WG * 6 * sizeof(float));
            mine = report;
        }
        float *bounds = reinterpret_cast<float *>(report + 1);
        report_seq = report->seq;                            // (the scans of this build are numbered on from the last build's)
        cand = lists[0].alloc<Cand>(n);
        if (!d_verts || !d_err || !cand) return GEN_NOMEM();
        GEN_TRY(hipMemcpy(d_verts, verts6, 6 * (size_t)n * sizeof(float), hipMemcpyHostToDevice));
        GEN_TRY(hipMemsetAsync(d_err, 0, sizeof(uint32_t), 0));
        hipLaunchKernelGGL(k_bounds, dim3(BOUNDS_WG), dim3(256), 0, 0, (const float *)d_verts, n, bounds);
        GEN_TRY(hipStreamSynchronize(0));
        {   // FindDimensions, dllmain.cpp:67-80 (the pass over the points ran on the device: 2 ms of a 15 ms build on the host)
            float lo[3] = { INFINITY, INFINITY, INFINITY }, hi[3] = { -INFINITY, -INFINITY, -INFINITY };
            for (uint32_t w = 0; w < BOUNDS_WG; w++)
                for (int k = 0; k < 3; k++) {
                    lo[k] = fminf(lo[k], ((volatile float *)bounds)[6 * w + k]);
                    hi[k] = fmaxf(hi[k], ((volatile float *)bounds)[6 * w + 3 + k]);
                }
            P.gox = (lo[0] + hi[0]) * 0.5f + 0.003f;
            P.goy = (lo[1] + hi[1]) * 0.5f + 0.003f;
            P.goz = (lo[2] + hi[2]) * 0.5f + 0.003f;
            const float lowest = fminf(lo[0], fminf(lo[1], lo[2])), highest = fmaxf(hi[0], fmaxf(hi[1], hi[2]));
            P.gs = (highest - lowest) * 1.1f;
        }
        P.verts = d_verts;
        hipLaunchKernelGGL(k_cand_init, dim3(1024), dim3(256), 0, 0, cand, (const float *)d_verts, n);
        if (!alloc_level(scratch[0], keep, L, 1)) return GEN_NOMEM();
        hipLaunchKernelGGL(k_root, dim3(1), dim3(1), 0, 0, L, n);
        return SDFHIP_OK;
    }

    // level `lvl`: centre search, the survivors' lists, corner search, the splits, the children.  more = false: nothing split
    int level(int lvl, bool &more)
    {
        auto tl = std::chrono::steady_clock::now();
        Arena &mine = scratch[lvl & 1], &other = scratch[(lvl + 1) & 1];
        P.depth = lvl;
        P.scale = ldexpf(1.0f, -lvl);                 // powf(0.5, depth)
        uint32_t *poff = mine.alloc<uint32_t>(n_nodes);
        if (!poff) return GEN_NOMEM();
        // which form: a wavefront per sibling block (k_center_sib / k_corners_sib) where that fills the chip -- 16 384 nodes = 2 048
        // wavefronts and more; below the root a level's nodes come in blocks of eight -- else a node's list over S workgroups of
        // 1 024 threads (k_center_seg_min, ...).  (1 M-point knot, depth 10: level 5, 10 776 nodes with lists of 50 000: 2.9 ms
        // in segments, 3.9 by sibling blocks; level 6, 37 896 nodes: 4.7 against 1.9)
        // ... and lists short enough that one wavefront per block is not the level's critical path (level 6 of the same knot:
        // 4 737 blocks with lists of 17 000 -- 1.6 ms by sibling blocks, 1.2 in segments; level 7, lists of 5 000: 1.1 against 2.2)
        const bool wide = n_nodes >= wide_level && lvl >= 1 && (n_nodes & 7u) == 0 &&
                          (wide_forced || list_entries / (n_nodes / 8) <= WIDE_MAX_LIST);
        SegArrays A{ nullptr, nullptr, nullptr, wide ? 0u : (seg_target + n_nodes - 1) / n_nodes };      // segments per node: ~4 096 workgroups per level
        // (the lists of a level are `list_entries` long together, one per block of eight siblings)
        const bool pipe = wide && list_entries / (n_nodes / 8) > 2u * (unsigned long long)SIB_CH;
        const bool fused = wide && !pipe && lvl >= depth;          // the last level: centre and corner searches in one kernel
        if (fused) ;
        else if (wide && pipe) hipLaunchKernelGGL(k_center_sib<true>, dim3(n_nodes / 8), dim3(64), 0, 0, P, L, cand, n_nodes, d_err);
        else if (wide) hipLaunchKernelGGL(k_center_sib<false>, dim3(n_nodes / 8), dim3(64), 0, 0, P, L, cand, n_nodes, d_err);
        else {
            A.best = mine.alloc<unsigned long long>(n_nodes); A.corner = mine.alloc<unsigned long long>(8 * (size_t)n_nodes);
            A.count = mine.alloc<uint32_t>((size_t)n_nodes * A.S);
            if (!A.best || !A.corner || !A.count) return GEN_NOMEM();
            GEN_TRY(hipMemsetAsync(A.best, 0xFF, (size_t)n_nodes * 8, 0));
            GEN_TRY(hipMemsetAsync(A.corner, 0xFF, (size_t)n_nodes * 64, 0));
            GEN_TRY(hipMemsetAsync(L.pcount, 0, (size_t)n_nodes * 4, 0));
            hipLaunchKernelGGL(k_center_seg_min, dim3((n_nodes * A.S + 7u) & ~7u), dim3(SEG_BT), 0, 0, P, L, A, cand, n_nodes);
            hipLaunchKernelGGL(k_center_seg_count, dim3((n_nodes * A.S + 7u) & ~7u), dim3(SEG_BT), 0, 0, P, L, A, cand, n_nodes, d_err);
        }
        // The survivors' lists of this level are the candidate lists of the next: their lengths are scanned into offsets and the
        // host allocates them -- except on the last level (lvl == MaxDepth), where no node splits: its survivors are looked at
        // for the corner values and written nowhere (1.9 GB of stores, a scan and a host round trip on the 1 M-point knot).
        const bool last_level = lvl >= depth;
        unsigned long long total = 0;
        Cand *possible = nullptr;
        if (!last_level) {
            if (!scan_u32(mine, L.pcount, poff, n_nodes, d_err, report, ++report_seq)) return GEN_NOMEM();
            GEN_TRY(wait_report(report, report_seq));
            total = ((volatile Report *)report)->total;
            if (total > 0xFFFFFFF0ull) return fail(SDFHIP_ERR_NOMEM, "sdfgen: candidate lists of level %d exceed 2^32 entries", lvl);
            lists[(lvl + 1) & 1].reset();             // the lists of level lvl-1: dead since k_children of lvl-1
            possible = lists[(lvl + 1) & 1].alloc<Cand>((size_t)total);
            if (!possible) return fail(SDFHIP_ERR_NOMEM, "sdfgen: out of device memory for %llu candidate entries", total);
        }
        cand_entries += total;
        list_entries = total;
        if (fused) hipLaunchKernelGGL((k_corners_sib<false, true>), dim3(n_nodes / 8), dim3(64), 0, 0, P, L, cand, poff, possible, n_nodes, d_err);
        else if (wide && pipe) hipLaunchKernelGGL(k_corners_sib<true>, dim3(n_nodes / 8), dim3(64), 0, 0, P, L, cand, poff, possible, n_nodes, d_err);
        else if (wide) hipLaunchKernelGGL(k_corners_sib<false>, dim3(n_nodes / 8), dim3(64), 0, 0, P, L, cand, poff, possible, n_nodes, d_err);
        else {
            hipLaunchKernelGGL(k_corners_seg, dim3((n_nodes * A.S + 7u) & ~7u), dim3(SEG_BT), 0, 0, P, L, A, cand, poff, possible, n_nodes);
            hipLaunchKernelGGL(k_corners_fin, dim3((8 * n_nodes + 255) / 256), dim3(256), 0, 0, P, L, A, cand, n_nodes, d_err);
        }
        if (!scan_u32(mine, L.split, L.block_of, n_nodes, d_err, report, ++report_seq)) return GEN_NOMEM();
        GEN_TRY(wait_report(report, report_seq));
        const unsigned long long n_split = ((volatile Report *)report)->total;
        if (((volatile Report *)report)->err)
            return fail(SDFHIP_ERR_ARG, "sdfgen: a cell at depth %d has no candidate point left (the reference throws \"Did not find\")", lvl);
        if (level_timing) {
            (void)hipDeviceSynchronize();
            fprintf(stderr, "sdfgen: level %2d: %9u nodes, %11llu entries kept for the next level, %8.3f ms\n", lvl, n_nodes, total,
                    std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - tl).count());
        }
        levels.push_back(KeptLevel{ L, n_nodes, nullptr, nullptr, nullptr });
        total_nodes += n_nodes;
        more = n_split != 0;
        if (!more) return SDFHIP_OK;
        if (total_nodes + 8 * n_split > 0x7FFFFFF0ull) return fail(SDFHIP_ERR_NOMEM, "sdfgen: more than 2^31 nodes");
        other.reset();                                // scratch of level lvl-1
        LevelArrays N;
        if (!alloc_level(other, keep, N, (size_t)(8 * n_split))) return GEN_NOMEM();
        hipLaunchKernelGGL(k_children, dim3((8 * n_nodes + 255) / 256), dim3(256), 0, 0, L, N, L.block_of, poff,
                           P.scale / 2, n_nodes);
        L = N;
        cand = possible;
        n_nodes = (uint32_t)(8 * n_split);
        return SDFHIP_OK;
    }

    // the reference's node order and bytes (k_subtree bottom-up, k_emit top-down)
    int order_and_bytes()
    {
        lap("levels done");
        d_S = keep.alloc<int32_t>(2 * total_nodes);
        d_V = keep.alloc<uint8_t>(8 * total_nodes);
        if (!d_S || !d_V) return GEN_NOMEM();
        for (auto &kl : levels) {
            kl.cnt = keep.alloc<uint32_t>(kl.n); kl.rank = keep.alloc<uint32_t>(kl.n); kl.index = keep.alloc<int32_t>(kl.n);
            if (!kl.cnt || !kl.rank || !kl.index) return GEN_NOMEM();
        }
        for (int l = (int)levels.size() - 1; l >= 0; l--) {
            KeptLevel &kl = levels[l];
            const uint32_t *next = l + 1 < (int)levels.size() ? levels[l + 1].cnt : nullptr;   // the last level splits nothing
            hipLaunchKernelGGL(k_subtree, dim3((kl.n + 255) / 256), dim3(256), 0, 0, kl.L.split, kl.L.block_of, next, kl.cnt, kl.n);
        }
        for (size_t l = 0; l < levels.size(); l++) {
            KeptLevel &kl = levels[l];
            hipLaunchKernelGGL(k_emit, dim3((kl.n + 255) / 256), dim3(256), 0, 0, kl.L.split, kl.L.parent, kl.L.vals, kl.cnt,
                               l ? levels[l - 1].rank : nullptr, l ? levels[l - 1].index : nullptr, kl.rank, kl.index,
                               ldexpf(1.0f, -(int)l), kl.n, d_S, d_V);
        }
        GEN_TRY(hipGetLastError());
        lap("order + bytes done");
        return SDFHIP_OK;
    }

    // the tree as a scene on `device`, as arrays on the host, or both; the statistics
    int results(int device, sdfhip_octdata *out, sdfhip_scene **scene_out, sdfhip_sdfgen_stats *stats)
    {
        if (scene_out) {
            // the viewer's generate -> upload flow (Program.cs:613-650 -> :147-152) without the round trip: the scene's records
            // and grids are made from the arrays the builder has just written (12 ms of copy to the host and 8 ms back, at depth 10)
            GEN_TRY(hipDeviceSynchronize());
            const int rc = sdfhip::scene_from_arrays(device, d_S, d_V, (uint32_t)total_nodes, true, nullptr, scene_out,
                                                     (int)levels.size() - 1);     // (the depth it built: levels 0 .. size - 1)
            if (rc != SDFHIP_OK) return rc;
            lap("scene made on the device");
        }
        if (out) {
            // the result arrays (the caller frees them with free()): large ones on 2 MB pages where the kernel offers them -- the
            // copy from the device writes every page for the first time, and 47 000 page faults of 4 KB take five times as long as
            // the 192 MB of a 12 M-node tree take over the link
            auto result_alloc = [](size_t bytes) -> void * {
                if (bytes < ((size_t)8 << 20)) return malloc(bytes);
                void *p = nullptr;
                if (posix_memalign(&p, (size_t)2 << 20, bytes) != 0) return malloc(bytes);
                (void)madvise(p, bytes, MADV_HUGEPAGE);
                return p;
            };
            const hipError_t e2 = tree_to_host(d_S, d_V, total_nodes, result_alloc, out);
            if (e2 != hipSuccess) {
                if (scene_out && *scene_out) { (void)sdfhip_scene_free(*scene_out); *scene_out = nullptr; }
                return fail(SDFHIP_ERR_DEVICE, "sdfgen: copying the tree back failed: %s", hipGetErrorString(e2));
            }
            lap("copied to the host");
        }
        if (stats) {
            stats->nodes = (uint32_t)total_nodes;
            stats->levels = (uint32_t)levels.size();
            stats->candidate_entries = cand_entries;
            stats->global_scale = P.gs;
            stats->global_offset[0] = P.gox; stats->global_offset[1] = P.goy; stats->global_offset[2] = P.goz;
            stats->total_ms = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
        }
        return SDFHIP_OK;
    }
};

// out: the tree on the host (may be null); scene_out: the tree as a scene handle on `device`, made from the builder's own device
// arrays (may be null)
int sdfgen_impl(int device, const float *verts6, uint32_t n, int32_t depth, sdfhip_octdata *out, sdfhip_scene **scene_out,
                sdfhip_sdfgen_stats *stats)
{
    if (!verts6 || (!out && !scene_out) || n == 0) return fail(SDFHIP_ERR_ARG, "sdfgen: null argument or empty point cloud");
    if (depth < 0 || depth > 12) return fail(SDFHIP_ERR_ARG, "sdfgen: depth %d outside 0..12", depth);
    if (out) { out->length = 0; out->structs = nullptr; out->values = nullptr; }
    if (scene_out) *scene_out = nullptr;
    const auto t0 = std::chrono::steady_clock::now();
    int ndev = 0;
    GEN_TRY(hipGetDeviceCount(&ndev));
    if (device < 0 || device >= ndev) return fail(SDFHIP_ERR_DEVICE, "sdfgen: device %d of %d does not exist", device, ndev);
    DeviceGuard g(device);
    if (!g.ok) GEN_TRY(hipSetDevice(device));                // (once more, for the runtime's word on it)
    try {
        Build b(verts6, n, depth, t0);
        int rc = b.start();
        bool more = true;
        for (int lvl = 0; rc == SDFHIP_OK && more; lvl++) rc = b.level(lvl, more);
        if (rc == SDFHIP_OK) rc = b.order_and_bytes();
        if (rc == SDFHIP_OK) rc = b.results(device, out, scene_out, stats);
        return rc;
    } catch (const std::bad_alloc &) {
        return fail(SDFHIP_ERR_NOMEM, "sdfgen: out of host memory");
    }
}

}  // namespace

extern "C" int sdfhip_sdfgen(int device, const float *verts6, uint32_t n, int32_t depth, sdfhip_octdata *out,
                             sdfhip_sdfgen_stats *stats)
try {
    if (!out) return fail(SDFHIP_ERR_ARG, "sdfgen: null argument or empty point cloud");
    return sdfgen_impl(device, verts6, n, depth, out, nullptr, stats);
}
SDFHIP_ABI_CATCH(sdfhip_sdfgen)

extern "C" int sdfhip_sdfgen_scene(int device, const float *verts6, uint32_t n, int32_t depth, sdfhip_scene **scene,
                                   sdfhip_octdata *out, sdfhip_sdfgen_stats *stats)
try {
    if (!scene) return fail(SDFHIP_ERR_ARG, "sdfgen_scene: null argument");
    return sdfgen_impl(device, verts6, n, depth, out, scene, stats);
}
SDFHIP_ABI_CATCH(sdfhip_sdfgen_scene)
