// libsdfhip.so, the clash check: sdfhip_instances_clash -- which pairs of an assembly's placed instances overlap on a cubic lattice,
// where, and in how many points (kernels: clash_kernels.h).
//
// Replaces: nothing in the reference's code; its shader marches one immutable tree and knows no parts.
//
// The rule, pinned (include/sdfhip.h): instance k contains the lattice point p iff compose_instance_value
// < 0 there; per pair a < b the count, the lowest index, the bounds and the coordinate sums of the points both contain, in integers.
//
// Per call: the options and the list are checked (the list as instances.hip checks it, by compose_host.h), each distinct source is
// read once under its own lock, and on a stream of the call's own (CallFrame) the instance table goes to device memory, k_clash_init
// empties the pair table of K (K - 1) / 2 entries and the counters, k_clash fills them, and both come back in one copy each.  The
// host keeps the entries with points > 0, which are in (a, b) order already.  Nothing is built and nothing is kept on the handles.
#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Wunneeded-internal-declaration"
#include "clash_kernels.h"
#include "compose_host.h"     // check_instance, read_instance (shared with compose.hip and instances.hip)
#pragma clang diagnostic pop
#include "abi_guard.h"

#include <chrono>
#include <cmath>
#include <cstring>
#include <vector>

using namespace sdfhip;
using namespace sdfhip::levels;

static_assert(sizeof(sdfhip_clash_options) == 28 && sizeof(sdfhip_clash) == 64 && sizeof(sdfhip_clash_stats) == 32,
              "the clash check's records of include/sdfhip.h");
static_assert(sizeof(sdfhip_clash) == sizeof(ClashPair) && offsetof(sdfhip_clash, lo) == offsetof(ClashPair, lo) &&
              offsetof(sdfhip_clash, sum) == offsetof(ClashPair, sum), "clash_kernels.h restates the record");
static_assert(SDFHIP_CLASH_MAX_INSTANCES == CLASH_MAX_INSTANCES, "clash_kernels.h restates the header's limit");

namespace {

constexpr uint32_t CLASH_MAX_DEPTH = 10;
const char *const FAIL_ALLOC = "SDFHIP_CLASH_FAIL_ALLOC";      // laboratory library: AllocFault

// what the call took from its arguments before any device call
struct Request {
    std::vector<ComposeInstance> table;
    int device = 0;
    ClashLattice L{0.0f, 0.0f, 0.0f, 0x1p-6f, 6u, 4096u, 0u, 1u};
};

int check_call(const char *name, const sdfhip_instance *instances, uint32_t n_instances, const sdfhip_clash_options *opt, const sdfhip_clash *out,
               uint32_t capacity, const uint32_t *n_pairs, Request &R)
{
    if (!instances) return fail(SDFHIP_ERR_ARG, "%s: null instance list", name);
    if (n_instances < 1 || n_instances > CLASH_MAX_INSTANCES)
        return fail(SDFHIP_ERR_ARG, "%s: %u instances: 1..%u (SDFHIP_CLASH_MAX_INSTANCES: a containment mask is one 64-bit word)", name, n_instances,
                    CLASH_MAX_INSTANCES);
    float side = 1.0f;
    if (opt) {
        if (const int rc = check_options_size(name, opt, sizeof(sdfhip_clash_options), "sdfhip_clash_options_default sets the size")) return rc;
        if (opt->flags & ~(uint32_t)SDFHIP_CLASH_NO_SKIP) return fail(SDFHIP_ERR_ARG, "%s: unknown flags %#x", name, opt->flags);
        if (opt->depth > CLASH_MAX_DEPTH) return fail(SDFHIP_ERR_ARG, "%s: depth %u outside 0..%u", name, opt->depth, CLASH_MAX_DEPTH);
        if (!std::isfinite(opt->origin[0]) || !std::isfinite(opt->origin[1]) || !std::isfinite(opt->origin[2]))
            return fail(SDFHIP_ERR_ARG, "%s: the origin (%g, %g, %g) is not finite", name, (double)opt->origin[0], (double)opt->origin[1], (double)opt->origin[2]);
        if (!std::isfinite(opt->side) || !(opt->side > 0.0f)) return fail(SDFHIP_ERR_ARG, "%s: the side %g is not finite and above 0", name, (double)opt->side);
        for (int a = 0; a < 3; a++)
            if (!std::isfinite(opt->origin[a] + opt->side))
                return fail(SDFHIP_ERR_ARG, "%s: the cube's far corner, origin + side = %g + %g, is not finite", name, (double)opt->origin[a], (double)opt->side);
        R.L.ox = opt->origin[0]; R.L.oy = opt->origin[1]; R.L.oz = opt->origin[2];
        R.L.depth = opt->depth;
        R.L.skip = (opt->flags & SDFHIP_CLASH_NO_SKIP) ? 0u : 1u;
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

// The table, entry by entry as sdfhip_scene_compose reads it (read_instance)
int read_table(const char *name, const sdfhip_instance *instances, uint32_t n_instances, Request &R)
{
    InstanceSources sources;
    R.table.resize(n_instances);
    for (uint32_t k = 0; k < n_instances; k++) {
        const Source *src = nullptr;
        bool fresh = false;
        if (const int rc = read_instance(name, sources, instances[k], k, R.table[k], &src, &fresh)) return rc;
    }
    R.device = sources.front().second.device;
    return SDFHIP_OK;
}

}  // namespace

extern "C" void sdfhip_clash_options_default(sdfhip_clash_options *opt)
try {
    if (!opt) { (void)fail(SDFHIP_ERR_ARG, "clash_options_default: null argument"); return; }
    opt->size = (uint32_t)sizeof(sdfhip_clash_options);
    opt->flags = 0u;
    opt->depth = 6u;
    opt->origin[0] = 0.0f; opt->origin[1] = 0.0f; opt->origin[2] = 0.0f;
    opt->side = 1.0f;
}
SDFHIP_ABI_CATCH_VOID(sdfhip_clash_options_default)

extern "C" int sdfhip_instances_clash(const sdfhip_instance *instances, uint32_t n_instances, const sdfhip_clash_options *opt, sdfhip_clash *out,
                                      uint32_t capacity, uint32_t *n_pairs, sdfhip_clash_stats *stats)
try {
    const char *name = "instances_clash";
    const auto t0 = std::chrono::steady_clock::now();
    Request R;
    if (const int rc = check_call(name, instances, n_instances, opt, out, capacity, n_pairs, R)) return rc;
    if (const int rc = read_table(name, instances, n_instances, R)) return rc;
    const uint32_t K = n_instances, n_table = K * (K - 1u) / 2u;
    std::vector<ClashPair> table(n_table);
    ClashStat slots[CLASH_STAT_SLOTS];
    float kernel_ms = 0.0f;
    CallFrame<2> call(name, R.device, FAIL_ALLOC, t0);
    const int rc = call.run("nothing was written", [&](hipStream_t st) -> int {
        ComposeInstance *d_table = call.bufs.get<ComposeInstance>(K);
        ClashPair *d_pairs = call.bufs.get<ClashPair>(n_table);
        ClashStat *d_stats = call.bufs.get<ClashStat>(CLASH_STAT_SLOTS);
        HIP_TRY(hipMemcpyAsync(d_table, R.table.data(), K * sizeof(ComposeInstance), hipMemcpyHostToDevice, st));
        HIP_TRY(hipEventRecord(call.cs.ev[0], st));
        const uint32_t init_threads = std::max(K * K, CLASH_STAT_SLOTS);
        hipLaunchKernelGGL(k_clash_init, dim3((init_threads + CLASH_THREADS - 1) / CLASH_THREADS), dim3(CLASH_THREADS), 0, st, d_pairs, K, d_stats);
        HIP_TRY(hipGetLastError());
        const uint32_t per = CLASH_THREADS / 64;
        hipLaunchKernelGGL(k_clash, dim3((R.L.n_blocks + per - 1) / per), dim3(CLASH_THREADS), 0, st, d_table, R.L, d_pairs, d_stats);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipEventRecord(call.cs.ev[1], st));
        if (n_table) HIP_TRY(hipMemcpyAsync(table.data(), d_pairs, (size_t)n_table * sizeof(ClashPair), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(slots, d_stats, sizeof slots, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        return call.elapsed(&kernel_ms, 0, 1);
    });
    if (rc != SDFHIP_OK) return rc;
    uint32_t total = 0;
    for (const ClashPair &P : table) {
        if (!P.points) continue;
        if (total < capacity) memcpy(out + total, &P, sizeof P);
        total++;
    }
    *n_pairs = total;
    if (stats) {
        memset(stats, 0, sizeof *stats);
        stats->points = (uint64_t)1 << (3u * R.L.depth);
        stats->blocks = R.L.n_blocks;
        for (const ClashStat &s : slots) { stats->blocks_looked += s.blocks_looked; stats->lookups += s.lookups; }
        stats->kernel_ms = kernel_ms;
        stats->total_ms = call.total_ms();
    }
    return SDFHIP_OK;
}
SDFHIP_ABI_CATCH(sdfhip_instances_clash)
