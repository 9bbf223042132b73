// libsdfhip.so, triangle mesh -> ASDF: sdfhip_trimesh_build -- the exact signed distance of a mesh (records from
// sdfhip_trimesh_prepare, trimesh.cpp) as a tree in HBM, level by level (kernels: trigen_kernels.h).
//
// Replaces: nothing in the live reference; the intent of its abandoned SdfBox/GpuGenerator.cs + Shaders/Distancer.hlsl, with the
// sign rule of the paper its README cites (include/sdfhip.h has the rule).
//
// Per level: k_tri_eval (every corner and centre of every block of siblings against the block's candidate list), and unless it
// is the last level k_tri_count, two scans, ONE host synchronisation for the two totals that size the next level (its blocks and
// its lists), k_tri_fill.  The levels' node arrays are joined at the end: breadth-first order is the order they were made in.
// Device memory: the builders' arenas over the chunk pool (host_support.h, device_memory.hip).
#include "trigen_kernels.h"
#include "host_support.h"
#include "abi_guard.h"

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdlib>
#include <vector>

using namespace sdfhip;

static_assert(sizeof(sdfhip_trimesh_stats) == 40 && sizeof(TriBlock) == 32, "the records of include/sdfhip.h and trigen_kernels.h");

namespace {

constexpr uint32_t TRI_WIDE_BLOCKS = 512;     // fewer blocks than this: 16 waves per block instead of 4 (the first levels' lists are long)

struct Level { int2 *S; uint2 *V; uint32_t n; };

// laboratory library: SDFHIP_TRI_PRUNE=0 -- every block keeps every record (the A/B, and the test that pruning changes no byte)
struct Knobs {
    bool prune = true;
    Knobs() { if (const char *e = lab_env("SDFHIP_TRI_PRUNE")) prune = atoi(e) != 0; }
};

// The build's arenas; laboratory library: SDFHIP_TRI_FAIL_ALLOC=k fails the build's k-th allocation (0 = the first)
struct Memory {
    Arena keep{ (size_t)32 << 20 }, scratch[2] = { Arena((size_t)32 << 20), Arena((size_t)32 << 20) };
    AllocFault fault{ "SDFHIP_TRI_FAIL_ALLOC" };
    template <class T> T *get(Arena &a, size_t n)
    {
        if (fault.next()) throw NoMem{};
        T *p = a.alloc<T>(n);
        if (!p) throw NoMem{};
        return p;
    }
};

#define TRI_TRY(expr) HIP_TRY_AS("trimesh_build: ", expr, #expr)

// out = exclusive scan of in[0 .. n), *d_total = its sum (device); sums: scratch of ceil(n / TRI_SCAN_CHUNK) entries
void scan(hipStream_t st, const uint32_t *in, uint32_t n, unsigned long long *sums, unsigned long long *out, unsigned long long *d_total)
{
    const uint32_t nchunk = (n + TRI_SCAN_CHUNK - 1) / TRI_SCAN_CHUNK;
    hipLaunchKernelGGL(k_tri_scan_sums, dim3(nchunk), dim3(TRI_SCAN_THREADS), 0, st, in, n, sums);
    hipLaunchKernelGGL(k_tri_scan_chunks, dim3(1), dim3(TRI_SCAN_THREADS), 0, st, sums, nchunk, d_total);
    hipLaunchKernelGGL(k_tri_scan_apply, dim3(nchunk), dim3(TRI_SCAN_THREADS), 0, st, in, n, sums, out);
}

}  // namespace

extern "C" int sdfhip_trimesh_build(int device, const sdfhip_trimesh *mesh, int32_t depth, sdfhip_scene **scene, sdfhip_octdata *host_out,
                                    sdfhip_trimesh_stats *stats)
try {
    const auto t0 = std::chrono::steady_clock::now();
    if (scene) *scene = nullptr;
    if (host_out) { host_out->length = 0; host_out->structs = nullptr; host_out->values = nullptr; }
    if (!mesh || !mesh->records || mesh->n_records == 0) return fail(SDFHIP_ERR_ARG, "trimesh_build: null mesh or no records");
    if (!scene && !host_out) return fail(SDFHIP_ERR_ARG, "trimesh_build: neither a scene nor host arrays asked for");
    if (depth < 0 || depth > TREE_MAX_DEPTH) return fail(SDFHIP_ERR_ARG, "trimesh_build: depth %d outside 0..%d", depth, TREE_MAX_DEPTH);
    const uint32_t nrec = mesh->n_records;
    // the pruning's absolute slack: 2^-14 of the largest coordinate in play, the cube's own 1 at least
    float bound = 1.0f;
    for (size_t r = 0; r < nrec; r++)
        for (int k = 0; k < 9; k++) bound = fmaxf(bound, fabsf(mesh->records[r * TRI_REC + k]));
    const float slack_abs = bound * 6.103515625e-5f;

    int ndev = 0;
    TRI_TRY(hipGetDeviceCount(&ndev));
    if (device < 0 || device >= ndev) return fail(SDFHIP_ERR_DEVICE, "trimesh_build: device %d of %d does not exist", device, ndev);
    DeviceGuard g(device);
    if (!g.ok) return fail(SDFHIP_ERR_DEVICE, "trimesh_build: hipSetDevice(%d) failed", device);
    const Knobs knobs;
    Memory mem;
    CallStream<2> cs;                       // (after `mem`: drained before the arenas give their chunks back)
    if (const int rc = cs.open("trimesh_build: ")) return rc;
    const hipStream_t st = cs.st;
    const hipEvent_t ev0 = cs.ev[0], ev1 = cs.ev[1];

    std::vector<Level> levels;
    uint64_t total_nodes = 0, cand_entries = 0;
    int2 *dS = nullptr; uint2 *dV = nullptr;
    try {
        float *d_rec = mem.get<float>(mem.keep, (size_t)nrec * TRI_REC);
        unsigned long long *d_totals = mem.get<unsigned long long>(mem.keep, 2);
        TRI_TRY(hipMemcpyAsync(d_rec, mesh->records, (size_t)nrec * TRI_REC * sizeof(float), hipMemcpyHostToDevice, st));
        TRI_TRY(hipEventRecord(ev0, st));
        // the root's block: the root alone, every record
        TriBlock *blocks = mem.get<TriBlock>(mem.scratch[0], 1);
        uint32_t *list = mem.get<uint32_t>(mem.scratch[0], nrec);
        const TriBlock root{ 0, 0, 0, 0, 0ull, nrec, 1 };
        TRI_TRY(hipMemcpyAsync(blocks, &root, sizeof root, hipMemcpyHostToDevice, st));
        hipLaunchKernelGGL(k_tri_iota, dim3(std::min<uint32_t>((nrec + 255) / 256, 1024)), dim3(256), 0, st, list, nrec);
        int2 *S_cur = mem.get<int2>(mem.keep, 1);
        const int2 root_links = make_int2(-1, -1);
        TRI_TRY(hipMemcpyAsync(S_cur, &root_links, sizeof root_links, hipMemcpyHostToDevice, st));
        TRI_TRY(hipStreamSynchronize(st));                     // (`root` and `root_links` are on the stack)
        uint32_t n_blocks = 1, n_nodes = 1;
        uint64_t list_entries = nrec;
        for (int lvl = 0;; lvl++) {
            Arena &mine = mem.scratch[lvl & 1], &other = mem.scratch[(lvl + 1) & 1];
            const float S = ldexpf(1.0f, -lvl);
            cand_entries += list_entries;
            uint2 *V = mem.get<uint2>(mem.keep, n_nodes);
            float *cdist = mem.get<float>(mine, n_nodes);
            uint32_t *split = mem.get<uint32_t>(mine, n_nodes);
            if (n_blocks < TRI_WIDE_BLOCKS)
                hipLaunchKernelGGL(k_tri_eval<16>, dim3(n_blocks), dim3(1024), 0, st, d_rec, list, blocks, S, lvl < depth ? 1 : 0, V, cdist, split);
            else
                hipLaunchKernelGGL(k_tri_eval<4>, dim3(n_blocks), dim3(256), 0, st, d_rec, list, blocks, S, lvl < depth ? 1 : 0, V, cdist, split);
            TRI_TRY(hipGetLastError());
            levels.push_back(Level{ S_cur, V, n_nodes });
            total_nodes += n_nodes;
            if (lvl >= depth) break;

            uint32_t *cnt = mem.get<uint32_t>(mine, n_nodes);
            uint8_t *mask = mem.get<uint8_t>(mine, (size_t)list_entries);
            const uint32_t nchunk = (n_nodes + TRI_SCAN_CHUNK - 1) / TRI_SCAN_CHUNK;
            unsigned long long *sums = mem.get<unsigned long long>(mine, nchunk);
            unsigned long long *rank = mem.get<unsigned long long>(mine, n_nodes), *coff = mem.get<unsigned long long>(mine, n_nodes);
            hipLaunchKernelGGL(k_tri_count, dim3(n_blocks), dim3(TRI_COUNT_THREADS), 0, st, d_rec, list, blocks, S, knobs.prune ? 1 : 0, slack_abs,
                               cdist, split, mask, cnt);
            scan(st, split, n_nodes, sums, rank, d_totals);
            scan(st, cnt, n_nodes, sums, coff, d_totals + 1);
            TRI_TRY(hipGetLastError());
            unsigned long long totals[2];
            TRI_TRY(hipMemcpyAsync(totals, d_totals, sizeof totals, hipMemcpyDeviceToHost, st));
            TRI_TRY(hipStreamSynchronize(st));
            const unsigned long long n_split = totals[0];
            if (!n_split) break;
            if (total_nodes + 8 * n_split > 0x7FFFFFFFull) return fail(SDFHIP_ERR_ARG, "trimesh_build: the tree would have more than 2^31 - 1 nodes");
            other.reset();                                     // the level before this one: its blocks and lists are read
            TriBlock *next_blocks = mem.get<TriBlock>(other, (size_t)n_split);
            uint32_t *next_list = mem.get<uint32_t>(other, (size_t)totals[1]);
            int2 *S_next = mem.get<int2>(mem.keep, (size_t)(8 * n_split));
            hipLaunchKernelGGL(k_tri_fill, dim3(n_blocks), dim3(64), 0, st, list, mask, blocks, split, cnt, rank, coff,
                               (uint32_t)(total_nodes - n_nodes), (uint32_t)total_nodes, S_cur, S_next, next_blocks, next_list);
            TRI_TRY(hipGetLastError());
            blocks = next_blocks; list = next_list; S_cur = S_next;
            n_blocks = (uint32_t)n_split; n_nodes = (uint32_t)(8 * n_split);
            list_entries = totals[1];
        }
        // breadth-first order: the levels, one behind the other
        dS = mem.get<int2>(mem.keep, (size_t)total_nodes);
        dV = mem.get<uint2>(mem.keep, (size_t)total_nodes);
        size_t at = 0;
        for (const Level &L : levels) {
            TRI_TRY(hipMemcpyAsync(dS + at, L.S, (size_t)L.n * sizeof(int2), hipMemcpyDeviceToDevice, st));
            TRI_TRY(hipMemcpyAsync(dV + at, L.V, (size_t)L.n * sizeof(uint2), hipMemcpyDeviceToDevice, st));
            at += L.n;
        }
        TRI_TRY(hipEventRecord(ev1, st));
        TRI_TRY(hipStreamSynchronize(st));
    } catch (const NoMem &) {
        return fail(SDFHIP_ERR_NOMEM, "trimesh_build: out of device memory");
    }
    float build_ms = 0.0f;
    TRI_TRY(hipEventElapsedTime(&build_ms, ev0, ev1));

    float scene_ms = 0.0f;
    if (const int rc = finish_tree("trimesh_build", device, dS, dV, (uint32_t)total_nodes, (int)levels.size() - 1, scene, host_out, &scene_ms)) return rc;
    if (stats) {
        stats->nodes = (uint32_t)total_nodes; stats->levels = (uint32_t)levels.size(); stats->records = nrec; stats->pad_ = 0;
        stats->candidate_entries = cand_entries;
        stats->build_ms = build_ms; stats->scene_ms = scene_ms; stats->pad1_ = 0;
        stats->total_ms = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
    }
    return SDFHIP_OK;
}
SDFHIP_ABI_CATCH(sdfhip_trimesh_build)
