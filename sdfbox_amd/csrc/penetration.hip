// libsdfhip.so, the penetration depth: sdfhip_instances_penetration -- how far each overlapping pair of an assembly's placed
// instances reaches into the other on a cubic lattice, at which point, and where each part's nearest surface lies (kernels:
// penetration_kernels.h).
//
// Replaces: nothing in the reference's code; its shader marches one immutable tree and knows no parts.
//
// The rule, pinned (include/sdfhip.h): the clash check's lattice and containment; r_k(p) = sqrtf(d2_k(q)) * s_k
// with q the placement's inverse map of p and d2_k sdfhip_scene_distance's on the source at level -1; per pair a < b the maximum of
// fminf(r_a, r_b) over the points both contain, the lowest index attaining it, and the search's answers there.
//
// Per call: the options and the list are checked as the clash check checks them (compose_host.h), each distinct source is read once
// under its own lock, and on a stream of the call's own (CallFrame): the table goes to device memory; the containment pass COUNTS
// the searches and names the instances that have any; the host refuses a count above 2^32 - 1 and a searched source that has no mesh,
// marks the "surface below" bitmap of each distinct searched source (k_dist_mark, this unit's own) and allocates 16 bytes per
// search; the containment pass EMITS the items; k_pen_search, k_pen_fold and k_pen_witness follow, and the records of the K (K - 1) / 2
// table entries come back in one copy.  The host keeps those with points > 0, which are in (a, b) order already.  No search at all
// (no point inside two parts): nothing is marked and nothing more allocated.  Nothing is built and nothing is kept on the handles.
#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Wunneeded-internal-declaration"
#include "penetration_kernels.h"
#include "compose_host.h"     // check_instance, read_instance (shared with compose.hip, instances.hip and clash.hip)
#include "distance_host.h"    // check_source, bitmap_words, launch_mark
#pragma clang diagnostic pop
#include "abi_guard.h"

#include <chrono>
#include <cmath>
#include <cstring>
#include <vector>

using namespace sdfhip;
using namespace sdfhip::levels;

static_assert(sizeof(sdfhip_penetration_options) == 28 && sizeof(sdfhip_penetration) == 64 && sizeof(sdfhip_penetration_stats) == 72,
              "the penetration records of include/sdfhip.h");
static_assert(sizeof(sdfhip_penetration) == sizeof(PenRecord) && offsetof(sdfhip_penetration, depth) == offsetof(PenRecord, depth) &&
              offsetof(sdfhip_penetration, node_a) == offsetof(PenRecord, node_a) && offsetof(sdfhip_penetration, nearest_b) == offsetof(PenRecord, nearest_b),
              "penetration_kernels.h restates the record");
static_assert(SDFHIP_CLASH_MAX_INSTANCES == PEN_MAX_INSTANCES, "penetration_kernels.h restates the header's limit");
static_assert(sizeof(sdfhip_penetration_options) == sizeof(sdfhip_clash_options) && SDFHIP_PENETRATION_NO_SKIP == SDFHIP_CLASH_NO_SKIP,
              "the options are the clash check's");

namespace {

constexpr uint32_t PEN_MAX_DEPTH = 10;
const char *const FAIL_ALLOC = "SDFHIP_PENETRATION_FAIL_ALLOC";      // laboratory library: AllocFault
enum { EV_BEGIN, EV_COUNTED, EV_MARK, EV_MARKED, EV_EMITTED, EV_SEARCHED, EV_FOLDED, EV_END, EV_COUNT };

// what the call took from its arguments before any device call
struct Request {
    std::vector<PenInstance> table;
    std::vector<Source> source;          // of each instance
    std::vector<uint32_t> distinct;      // of each instance: the first instance with the same handle
    int device = 0;
    PenLattice L{0.0f, 0.0f, 0.0f, 0x1p-6f, 6u, 4096u, 0u, 1u};
};

// sdfhip_instances_clash's checks, word for word (clash.hip's check_call)
int check_call(const char *name, const sdfhip_instance *instances, uint32_t n_instances, const sdfhip_penetration_options *opt,
               const sdfhip_penetration *out, uint32_t capacity, const uint32_t *n_pairs, Request &R)
{
    if (!instances) return fail(SDFHIP_ERR_ARG, "%s: null instance list", name);
    if (n_instances < 1 || n_instances > PEN_MAX_INSTANCES)
        return fail(SDFHIP_ERR_ARG, "%s: %u instances: 1..%u (SDFHIP_CLASH_MAX_INSTANCES: a containment mask is one 64-bit word)", name, n_instances,
                    PEN_MAX_INSTANCES);
    float side = 1.0f;
    if (opt) {
        if (const int rc = check_options_size(name, opt, sizeof(sdfhip_penetration_options), "sdfhip_penetration_options_default sets the size")) return rc;
        if (opt->flags & ~(uint32_t)SDFHIP_PENETRATION_NO_SKIP) return fail(SDFHIP_ERR_ARG, "%s: unknown flags %#x", name, opt->flags);
        if (opt->depth > PEN_MAX_DEPTH) return fail(SDFHIP_ERR_ARG, "%s: depth %u outside 0..%u", name, opt->depth, PEN_MAX_DEPTH);
        if (!std::isfinite(opt->origin[0]) || !std::isfinite(opt->origin[1]) || !std::isfinite(opt->origin[2]))
            return fail(SDFHIP_ERR_ARG, "%s: the origin (%g, %g, %g) is not finite", name, (double)opt->origin[0], (double)opt->origin[1], (double)opt->origin[2]);
        if (!std::isfinite(opt->side) || !(opt->side > 0.0f)) return fail(SDFHIP_ERR_ARG, "%s: the side %g is not finite and above 0", name, (double)opt->side);
        for (int a = 0; a < 3; a++)
            if (!std::isfinite(opt->origin[a] + opt->side))
                return fail(SDFHIP_ERR_ARG, "%s: the cube's far corner, origin + side = %g + %g, is not finite", name, (double)opt->origin[a], (double)opt->side);
        R.L.ox = opt->origin[0]; R.L.oy = opt->origin[1]; R.L.oz = opt->origin[2];
        R.L.depth = opt->depth;
        R.L.skip = (opt->flags & SDFHIP_PENETRATION_NO_SKIP) ? 0u : 1u;
        side = opt->side;
    }
    R.L.pitch = side * std::ldexp(1.0f, -(int)R.L.depth);
    R.L.n_blocks = 1u << (3u * (R.L.depth > 2u ? R.L.depth - 2u : 0u));
    R.L.n_instances = n_instances;
    if (!n_pairs) return fail(SDFHIP_ERR_ARG, "%s: null n_pairs", name);
    if (!out && capacity > 0) return fail(SDFHIP_ERR_ARG, "%s: null out with capacity %u", name, capacity);
    for (uint32_t k = 0; k < n_instances; k++)
        if (const int rc = check_instance(name, instances + k, k)) return rc;
    return SDFHIP_OK;
}

// The table, entry by entry as sdfhip_scene_compose reads it (read_instance); what was read of each instance's handle is kept by
// value, and the first instance of each handle stands for it
int read_table(const char *name, const sdfhip_instance *instances, uint32_t n_instances, Request &R)
{
    InstanceSources sources;
    R.table.resize(n_instances);
    R.source.resize(n_instances);
    R.distinct.resize(n_instances);
    for (uint32_t k = 0; k < n_instances; k++) {
        const Source *src = nullptr;
        bool fresh = false;
        if (const int rc = read_instance(name, sources, instances[k], k, R.table[k].I, &src, &fresh)) return rc;
        R.source[k] = *src;
        R.table[k].D = DistScene{src->Q.nodes, src->Q.n_nodes, nullptr, -1};
        R.distinct[k] = k;
        for (uint32_t j = 0; j < k; j++)
            if (instances[j].scene == instances[k].scene) { R.distinct[k] = j; break; }
    }
    R.device = sources.front().second.device;
    return SDFHIP_OK;
}

}  // namespace

extern "C" void sdfhip_penetration_options_default(sdfhip_penetration_options *opt)
try {
    if (!opt) { (void)fail(SDFHIP_ERR_ARG, "penetration_options_default: null argument"); return; }
    opt->size = (uint32_t)sizeof(sdfhip_penetration_options);
    opt->flags = 0u;
    opt->depth = 6u;
    opt->origin[0] = 0.0f; opt->origin[1] = 0.0f; opt->origin[2] = 0.0f;
    opt->side = 1.0f;
}
SDFHIP_ABI_CATCH_VOID(sdfhip_penetration_options_default)

extern "C" int sdfhip_instances_penetration(const sdfhip_instance *instances, uint32_t n_instances, const sdfhip_penetration_options *opt,
                                            sdfhip_penetration *out, uint32_t capacity, uint32_t *n_pairs, sdfhip_penetration_stats *stats)
try {
    const char *name = "instances_penetration";
    const auto t0 = std::chrono::steady_clock::now();
    Request R;
    if (const int rc = check_call(name, instances, n_instances, opt, out, capacity, n_pairs, R)) return rc;
    if (const int rc = read_table(name, instances, n_instances, R)) return rc;
    const uint32_t K = n_instances, n_table = K * (K - 1u) / 2u;
    std::vector<PenRecord> table(n_table);
    PenCounters counted, done;
    memset(&counted, 0, sizeof counted);
    memset(&done, 0, sizeof done);
    bool searched = false;
    CallFrame<EV_COUNT> call(name, R.device, FAIL_ALLOC, t0);
    const int rc = call.run("nothing was written", [&](hipStream_t st) -> int {
        const uint32_t per = PEN_THREADS / 64;
        const dim3 lattice_grid((R.L.n_blocks + per - 1) / per), wg(PEN_THREADS);
        PenInstance *d_table = call.bufs.get<PenInstance>(K);
        PenPair *d_pairs = call.bufs.get<PenPair>(n_table);
        PenCounters *d_counters = call.bufs.get<PenCounters>(1);
        HIP_TRY(hipMemcpyAsync(d_table, R.table.data(), K * sizeof(PenInstance), hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemsetAsync(d_pairs, 0, n_table ? (size_t)n_table * sizeof(PenPair) : 1, st));
        HIP_TRY(hipMemsetAsync(d_counters, 0, sizeof(PenCounters), st));
        // the count
        HIP_TRY(hipEventRecord(call.cs.ev[EV_BEGIN], st));
        hipLaunchKernelGGL(k_pen_contain<false>, lattice_grid, wg, 0, st, d_table, R.L, d_counters, (PenItem *)nullptr, 0ull);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipEventRecord(call.cs.ev[EV_COUNTED], st));
        HIP_TRY(hipMemcpyAsync(&counted, d_counters, sizeof counted, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        if (counted.searches == 0) return SDFHIP_OK;
        if (counted.searches > 0xFFFFFFFFull)
            return fail(SDFHIP_ERR_ARG, "%s: %llu searches (the points inside two or more parts, once per part), above 4294967295: narrow the box "
                        "(the clash record's clash_box) or lower the depth", name, counted.searches);
        for (uint32_t k = 0; k < K; k++)
            if ((counted.searched >> k) & 1ull) {
                char what[64];
                snprintf(what, sizeof what, "%s: instance %u", name, k);
                if (const int rc = check_source(what, R.source[k])) return rc;
            }
        // the bitmaps of the distinct searched sources, and the table again with them
        std::vector<uint32_t *> below(K, nullptr);
        for (uint32_t k = 0; k < K; k++)
            if ((counted.searched >> k) & 1ull) {
                const uint32_t first = R.distinct[k];
                if (!below[first]) below[first] = call.bufs.get<uint32_t>(bitmap_words(R.source[first].Q.n_nodes));
            }
        const unsigned long long n_items = counted.searches;
        PenItem *d_items = call.bufs.get<PenItem>((size_t)n_items);
        PenRecord *d_out = call.bufs.get<PenRecord>(n_table);
        for (uint32_t k = 0; k < K; k++) R.table[k].D.below = below[R.distinct[k]];     // (null: an instance nothing searches)
        HIP_TRY(hipMemcpyAsync(d_table, R.table.data(), K * sizeof(PenInstance), hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemsetAsync(d_out, 0, (size_t)n_table * sizeof(PenRecord), st));
        HIP_TRY(hipEventRecord(call.cs.ev[EV_MARK], st));
        for (uint32_t k = 0; k < K; k++)
            if (below[k])
                if (const int rc = launch_mark(R.source[k], -1, below[k], st)) return rc;
        HIP_TRY(hipEventRecord(call.cs.ev[EV_MARKED], st));
        // the emit, the searches, the fold, the records
        hipLaunchKernelGGL(k_pen_contain<true>, lattice_grid, wg, 0, st, d_table, R.L, d_counters, d_items, n_items);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipEventRecord(call.cs.ev[EV_EMITTED], st));
        const dim3 item_grid = grid_stride_blocks(n_items, LEVEL_MAX_WORKGROUPS);
        hipLaunchKernelGGL(k_pen_search, item_grid, wg, 0, st, d_table, R.L, d_items, n_items, d_counters);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipEventRecord(call.cs.ev[EV_SEARCHED], st));
        hipLaunchKernelGGL(k_pen_fold, item_grid, wg, 0, st, d_items, n_items, K, d_pairs);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipEventRecord(call.cs.ev[EV_FOLDED], st));
        hipLaunchKernelGGL(k_pen_witness, dim3((2u * n_table + PEN_THREADS - 1) / PEN_THREADS), wg, 0, st, d_table, R.L, d_pairs, n_table, d_out);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipEventRecord(call.cs.ev[EV_END], st));
        HIP_TRY(hipMemcpyAsync(table.data(), d_out, (size_t)n_table * sizeof(PenRecord), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(&done, d_counters, sizeof done, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        if (done.cursor != n_items)
            return fail(SDFHIP_ERR_DEVICE, "%s: the emit pass wrote %llu items where the count pass counted %llu", name, done.cursor, n_items);
        searched = true;
        return SDFHIP_OK;
    });
    if (rc != SDFHIP_OK) return rc;
    float pass_ms[6] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    if (const int rc = call.elapsed(&pass_ms[0], EV_BEGIN, EV_COUNTED)) return rc;
    if (searched) {
        const int from[5] = {EV_MARK, EV_MARKED, EV_EMITTED, EV_SEARCHED, EV_FOLDED};
        for (int k = 0; k < 5; k++)
            if (const int rc = call.elapsed(&pass_ms[k + 1], from[k], from[k] + 1)) return rc;
    }
    uint32_t total = 0;
    if (searched)
        for (const PenRecord &P : table) {
            if (!P.points) continue;
            if (total < capacity) memcpy(out + total, &P, sizeof P);
            total++;
        }
    *n_pairs = total;
    if (stats) {
        memset(stats, 0, sizeof *stats);
        stats->points = (uint64_t)1 << (3u * R.L.depth);
        stats->blocks = R.L.n_blocks;
        for (const PenStat &s : counted.slot) { stats->blocks_looked += s.blocks_looked; stats->lookups += s.lookups; }
        stats->searches = counted.searches;
        stats->visited = done.visited;
        for (int k = 0; k < 6; k++) { stats->pass_ms[k] = pass_ms[k]; stats->kernel_ms += pass_ms[k]; }
        stats->total_ms = call.total_ms();
    }
    return SDFHIP_OK;
}
SDFHIP_ABI_CATCH(sdfhip_instances_penetration)
