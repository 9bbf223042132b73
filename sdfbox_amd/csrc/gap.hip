// libsdfhip.so, the clearance of an assembly: sdfhip_instances_gap -- how far apart the surfaces of each pair of an assembly's placed
// instances lie, at which vertex, and where the other part's nearest surface point is (kernels: gap_kernels.h).
//
// Replaces: nothing in the reference's code; its shader marches one immutable tree and knows no parts.
//
// The rule, pinned (include/sdfhip.h): the vertices of each part's triangles (sdfhip_scene_mesh's at level
// -1) mapped forward, r_k of the penetration depth at them, per pair a < b the minimum over both directions, the lowest (direction,
// node, 3 k + v) attaining it, and the search's answer there.
//
// Per call: the options and the list are checked as the clash check checks them (compose_host.h), each distinct source is read once
// under its own lock, and on a stream of the call's own (CallFrame): per distinct source the cut cells are COUNTED (k_gap_cells<false>),
// the counts scanned (scan_device.h), and the cells EMITTED in node order together with their tight box; the host's broad phase, in
// double, maps each part's box forward to a bounding sphere and drops a pair only when the spheres are provably more than `limit`
// apart (a source without a mesh has no box to trust: its pairs are all kept); a source with a kept pair is refused if it has no
// mesh, and its "surface below" bitmap is marked (k_dist_mark, this unit's
// own); the work table -- one entry per (ordered pair, chunk of 256 cells) -- the keys and the instance table go to device memory;
// k_gap_search and k_gap_record follow, and the records of the K (K - 1) / 2 table entries come back in one copy.  The host keeps those
// whose key moved, which are in (a, b) order already.  Nothing is built and nothing is kept on the handles.
#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Wunneeded-internal-declaration"
#include "gap_kernels.h"
#include "compose_host.h"     // check_instance, read_instance (shared with compose.hip, instances.hip, clash.hip and penetration.hip)
#include "distance_host.h"    // check_source, bitmap_words, launch_mark
#pragma clang diagnostic pop
#include "abi_guard.h"

#include <chrono>
#include <cmath>
#include <cstring>
#include <vector>

using namespace sdfhip;
using namespace sdfhip::levels;

static_assert(sizeof(sdfhip_gap_options) == 12 && sizeof(sdfhip_gap) == 64 && sizeof(sdfhip_gap_stats) == 56, "the gap records of include/sdfhip.h");
static_assert(sizeof(sdfhip_gap) == sizeof(GapRecord) && offsetof(sdfhip_gap, gap) == offsetof(GapRecord, gap) &&
              offsetof(sdfhip_gap, corner) == offsetof(GapRecord, corner) && offsetof(sdfhip_gap, point_b) == offsetof(GapRecord, point_b),
              "gap_kernels.h restates the record");
static_assert(SDFHIP_CLASH_MAX_INSTANCES == GAP_MAX_INSTANCES && SDFHIP_GAP_NO_PRUNE == GAP_NO_PRUNE, "gap_kernels.h restates the header's constants");

namespace {

const char *const FAIL_ALLOC = "SDFHIP_GAP_FAIL_ALLOC";      // laboratory library: AllocFault
enum { EV_BEGIN, EV_LISTED, EV_MARK, EV_MARKED, EV_SEARCHED, EV_END, EV_COUNT };

// what the call took from its arguments before any device call
struct Request {
    std::vector<GapInstance> table;
    std::vector<Source> source;          // of each instance
    std::vector<uint32_t> distinct;      // of each instance: the first instance with the same handle
    int device = 0;
    uint32_t flags = 0u;
    float limit = INFINITY;
};

// per distinct source, in device memory: the scan's total (first, as k_scan_chunk_totals writes it) and the box
struct SourceHead {
    unsigned long long total;
    GapBox box;
};

int check_call(const char *name, const sdfhip_instance *instances, uint32_t n_instances, const sdfhip_gap_options *opt, const sdfhip_gap *out,
               uint32_t capacity, const uint32_t *n_pairs, Request &R)
{
    if (!instances) return fail(SDFHIP_ERR_ARG, "%s: null instance list", name);
    if (n_instances < 1 || n_instances > GAP_MAX_INSTANCES)
        return fail(SDFHIP_ERR_ARG, "%s: %u instances: 1..%u (SDFHIP_CLASH_MAX_INSTANCES: the list is the clash check's)", name, n_instances, GAP_MAX_INSTANCES);
    if (opt) {
        if (const int rc = check_options_size(name, opt, sizeof(sdfhip_gap_options), "sdfhip_gap_options_default sets the size")) return rc;
        if (opt->flags & ~(uint32_t)SDFHIP_GAP_NO_PRUNE) return fail(SDFHIP_ERR_ARG, "%s: unknown flags %#x", name, opt->flags);
        if (!(opt->limit >= 0.0f)) return fail(SDFHIP_ERR_ARG, "%s: the limit %g is not in [0, +inf]", name, (double)opt->limit);
        R.flags = opt->flags;
        R.limit = opt->limit;
    }
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
    R.source.resize(n_instances);
    R.distinct.resize(n_instances);
    for (uint32_t k = 0; k < n_instances; k++) {
        const Source *src = nullptr;
        bool fresh = false;
        if (const int rc = read_instance(name, sources, instances[k], k, R.table[k].I, &src, &fresh)) return rc;
        R.source[k] = *src;
        R.table[k].D = DistScene{src->Q.nodes, src->Q.n_nodes, nullptr, -1};
        R.table[k].cells = nullptr;
        R.table[k].n_cells = 0u; R.table[k].pad = 0u;
        R.distinct[k] = k;
        for (uint32_t j = 0; j < k; j++)
            if (instances[j].scene == instances[k].scene) { R.distinct[k] = j; break; }
    }
    R.device = sources.front().second.device;
    return SDFHIP_OK;
}

// The bounding sphere, in double, of a part whose source's cut cells lie in `box` (units of 2^-MESH_MAX_DEPTH): the box's centre mapped
// forward, and its half diagonal times s.  Every world vertex of the part and every point of its triangles lies within `radius` of
// `centre` up to the slack below: the rotation is orthogonal to 1e-4 (check_similarity), which the factor 1 + 1e-3 covers, and the
// fp32 roundings of the maps, which `slack` of keep() covers.
struct Sphere {
    double c[3], radius, reach;          // reach: |centre| + radius, what the roundings scale with
    bool known;                          // false: the box cannot be trusted, and no pair of this part is ever dropped
};
// trusted: the source is one sdfhip_scene_mesh takes (check_source's test).  On any other -- a bent link, a cell deeper than
// MESH_MAX_DEPTH, which k_gap_cells leaves out of the box -- the climb's coordinates mean nothing: such a part keeps its pairs, and
// check_source then refuses it by name instead of the broad phase dropping it silently.  Likewise a box that was never written
Sphere sphere_of(const GapInstance &G, const GapBox &box, bool trusted)
{
    const double unit = std::ldexp(1.0, -MESH_MAX_DEPTH);
    double mid[3], half2 = 0.0;
    for (int a = 0; a < 3; a++) {
        mid[a] = 0.5 * ((double)box.lo[a] + (double)box.hi[a]) * unit;
        const double h = 0.5 * ((double)box.hi[a] - (double)box.lo[a]) * unit;
        half2 += h * h;
    }
    const PlaceMap &M = G.I.M;
    const double t[3] = {M.tx, M.ty, M.tz};
    Sphere S;
    S.known = trusted && box.lo[0] <= box.hi[0] && box.lo[1] <= box.hi[1] && box.lo[2] <= box.hi[2];
    double norm2 = 0.0;
    for (int i = 0; i < 3; i++) {
        S.c[i] = ((double)M.r[i][0] * mid[0] + (double)M.r[i][1] * mid[1] + (double)M.r[i][2] * mid[2]) * (double)M.s + t[i];
        norm2 += S.c[i] * S.c[i];
    }
    S.radius = std::sqrt(half2) * (double)M.s * (1.0 + 1e-3);
    S.reach = std::sqrt(norm2) + S.radius;
    return S;
}
// is the pair kept: dropped only when centre distance - radii exceeds the limit by more than the slack.  r of the rule is an fp32
// value within a few 1e-7 relative of the exact distance between points whose coordinates carry a few 1e-7 of `reach` each; 1e-5 of
// everything involved is two orders above that
bool keep(const Sphere &A, const Sphere &B, float limit)
{
    if (!(limit < INFINITY) || !A.known || !B.known) return true;
    double d2 = 0.0;
    for (int i = 0; i < 3; i++) d2 += (A.c[i] - B.c[i]) * (A.c[i] - B.c[i]);
    const double apart = std::sqrt(d2) - A.radius - B.radius;
    const double slack = 1e-5 * (A.reach + B.reach + (double)limit + 1.0);
    return !(apart > (double)limit + slack);             // (a NaN keeps the pair)
}

}  // namespace

extern "C" void sdfhip_gap_options_default(sdfhip_gap_options *opt)
try {
    if (!opt) { (void)fail(SDFHIP_ERR_ARG, "gap_options_default: null argument"); return; }
    opt->size = (uint32_t)sizeof(sdfhip_gap_options);
    opt->flags = 0u;
    opt->limit = INFINITY;
}
SDFHIP_ABI_CATCH_VOID(sdfhip_gap_options_default)

extern "C" int sdfhip_instances_gap(const sdfhip_instance *instances, uint32_t n_instances, const sdfhip_gap_options *opt, sdfhip_gap *out,
                                    uint32_t capacity, uint32_t *n_pairs, sdfhip_gap_stats *stats)
try {
    const char *name = "instances_gap";
    const auto t0 = std::chrono::steady_clock::now();
    Request R;
    if (const int rc = check_call(name, instances, n_instances, opt, out, capacity, n_pairs, R)) return rc;
    if (const int rc = read_table(name, instances, n_instances, R)) return rc;
    const uint32_t K = n_instances, n_table = K * (K - 1u) / 2u;
    std::vector<GapRecord> table(n_table);
    std::vector<unsigned long long> keys(n_table);
    GapCounters done;
    memset(&done, 0, sizeof done);
    uint32_t pairs_searched = 0;
    uint64_t cells = 0;
    bool listed = false, searched = false;
    CallFrame<EV_COUNT> call(name, R.device, FAIL_ALLOC, t0);
    const int rc = n_table == 0 ? (int)SDFHIP_OK : call.run("nothing was written", [&](hipStream_t st) -> int {
        const dim3 wg(GAP_THREADS);
        GapInstance *d_table = call.bufs.get<GapInstance>(K);
        unsigned long long *d_keys = call.bufs.get<unsigned long long>(n_table);
        GapCounters *d_counters = call.bufs.get<GapCounters>(1);
        SourceHead *d_heads = call.bufs.get<SourceHead>(K);
        std::vector<SourceHead> heads(K);
        for (SourceHead &h : heads) { h.total = 0ull; for (int a = 0; a < 3; a++) { h.box.lo[a] = 0xFFFFFFFFu; h.box.hi[a] = 0u; } }
        HIP_TRY(hipMemcpyAsync(d_heads, heads.data(), K * sizeof(SourceHead), hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemsetAsync(d_counters, 0, sizeof(GapCounters), st));
        // the cut-cell lists of the distinct sources: count, scan; then the emit
        HIP_TRY(hipEventRecord(call.cs.ev[EV_BEGIN], st));
        std::vector<uint32_t *> chunk(K, nullptr);
        for (uint32_t k = 0; k < K; k++) {
            if (R.distinct[k] != k) continue;
            const uint32_t n = R.source[k].Q.n_nodes, nchunk = (n + GAP_THREADS - 1u) / GAP_THREADS;
            if (n == 0u) continue;
            chunk[k] = call.bufs.get<uint32_t>(nchunk);
            hipLaunchKernelGGL(k_gap_cells<false>, dim3(nchunk), wg, 0, st, R.source[k].Q.nodes, n, chunk[k], (GapCell *)nullptr, 0u, (GapBox *)nullptr);
            HIP_TRY(hipGetLastError());
            hipLaunchKernelGGL(k_scan_chunk_totals<unsigned long long>, dim3(1), dim3(1024), 0, st, chunk[k], nchunk, &d_heads[k].total);
            HIP_TRY(hipGetLastError());
        }
        HIP_TRY(hipMemcpyAsync(heads.data(), d_heads, K * sizeof(SourceHead), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        std::vector<GapCell *> list(K, nullptr);
        for (uint32_t k = 0; k < K; k++) {
            if (R.distinct[k] != k || !chunk[k] || heads[k].total == 0ull) continue;
            const uint32_t n = R.source[k].Q.n_nodes, nchunk = (n + GAP_THREADS - 1u) / GAP_THREADS;
            list[k] = call.bufs.get<GapCell>((size_t)heads[k].total);
            hipLaunchKernelGGL(k_gap_cells<true>, dim3(nchunk), wg, 0, st, R.source[k].Q.nodes, n, chunk[k], list[k], (uint32_t)heads[k].total, &d_heads[k].box);
            HIP_TRY(hipGetLastError());
        }
        HIP_TRY(hipEventRecord(call.cs.ev[EV_LISTED], st));
        HIP_TRY(hipMemcpyAsync(heads.data(), d_heads, K * sizeof(SourceHead), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        listed = true;
        for (uint32_t k = 0; k < K; k++) {
            R.table[k].cells = list[R.distinct[k]];
            R.table[k].n_cells = (uint32_t)heads[R.distinct[k]].total;
        }
        // the broad phase and the work table
        std::vector<Sphere> sphere(K);
        for (uint32_t k = 0; k < K; k++)
            if (R.table[k].n_cells)
                sphere[k] = sphere_of(R.table[k], heads[R.distinct[k]].box, R.source[k].stack_ok && R.source[k].depth <= (uint32_t)MESH_MAX_DEPTH);
        std::vector<GapOrdered> ordered;
        std::vector<GapWork> work;
        unsigned long long kept = 0ull, n_work = 0ull;
        for (uint32_t a = 0, e = 0; a < K; a++)
            for (uint32_t b = a + 1u; b < K; b++, e++) {
                if (!R.table[a].n_cells || !R.table[b].n_cells) continue;              // a part without a surface: no candidate either way
                if (!(R.flags & SDFHIP_GAP_NO_PRUNE) && !keep(sphere[a], sphere[b], R.limit)) continue;
                kept |= (1ull << a) | (1ull << b);
                pairs_searched++;
                for (uint32_t direction = 0; direction < 2u; direction++) {
                    const uint32_t from = direction ? b : a, to = direction ? a : b;
                    n_work += (R.table[from].n_cells + GAP_THREADS - 1u) / GAP_THREADS;
                    ordered.push_back(GapOrdered{from, to, e, direction});
                }
            }
        if (n_work > 0x7FFFFFFFull)
            return fail(SDFHIP_ERR_ARG, "%s: %llu workgroups (one per ordered pair and 256 cut cells), above 2147483647: shorten the list or set a limit", name, n_work);
        if (n_work == 0ull) return SDFHIP_OK;
        for (uint32_t k = 0; k < K; k++)
            if ((kept >> k) & 1ull) {
                char what[64];
                snprintf(what, sizeof what, "%s: instance %u", name, k);
                if (const int rc = check_source(what, R.source[k])) return rc;
            }
        work.reserve((size_t)n_work);
        for (uint32_t o = 0; o < (uint32_t)ordered.size(); o++) {
            const uint32_t chunks = (R.table[ordered[o].from].n_cells + GAP_THREADS - 1u) / GAP_THREADS;
            for (uint32_t c = 0; c < chunks; c++) work.push_back(GapWork{o, c});
            cells += R.table[ordered[o].from].n_cells;
        }
        // the bitmaps of the distinct searched sources, and the table with them
        std::vector<uint32_t *> below(K, nullptr);
        for (uint32_t k = 0; k < K; k++)
            if ((kept >> k) & 1ull) {
                const uint32_t first = R.distinct[k];
                if (!below[first]) below[first] = call.bufs.get<uint32_t>(bitmap_words(R.source[first].Q.n_nodes));
            }
        for (uint32_t k = 0; k < K; k++) R.table[k].D.below = below[R.distinct[k]];     // (null: an instance nothing searches)
        GapOrdered *d_ordered = call.bufs.get<GapOrdered>(ordered.size());
        GapWork *d_work = call.bufs.get<GapWork>(work.size());
        GapRecord *d_out = call.bufs.get<GapRecord>(n_table);
        const uint32_t limit_bits = [&] { uint32_t u; memcpy(&u, &R.limit, 4); return u; }();
        for (unsigned long long &key : keys) key = ((unsigned long long)limit_bits << 32) | 0xFFFFFFFFull;
        HIP_TRY(hipMemcpyAsync(d_table, R.table.data(), K * sizeof(GapInstance), hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(d_keys, keys.data(), (size_t)n_table * sizeof(unsigned long long), hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(d_ordered, ordered.data(), ordered.size() * sizeof(GapOrdered), hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(d_work, work.data(), work.size() * sizeof(GapWork), hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemsetAsync(d_out, 0, (size_t)n_table * sizeof(GapRecord), st));
        HIP_TRY(hipEventRecord(call.cs.ev[EV_MARK], st));
        for (uint32_t k = 0; k < K; k++)
            if (below[k])
                if (const int rc = launch_mark(R.source[k], -1, below[k], st)) return rc;
        HIP_TRY(hipEventRecord(call.cs.ev[EV_MARKED], st));
        hipLaunchKernelGGL(k_gap_search, dim3((uint32_t)n_work), wg, 0, st, d_table, d_ordered, d_work, (uint32_t)n_work, R.flags, d_keys, d_counters);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipEventRecord(call.cs.ev[EV_SEARCHED], st));
        hipLaunchKernelGGL(k_gap_record, dim3((n_table + GAP_THREADS - 1u) / GAP_THREADS), wg, 0, st, d_table, K, d_keys, n_table, d_out);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipEventRecord(call.cs.ev[EV_END], st));
        HIP_TRY(hipMemcpyAsync(table.data(), d_out, (size_t)n_table * sizeof(GapRecord), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(keys.data(), d_keys, (size_t)n_table * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(&done, d_counters, sizeof done, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        searched = true;
        return SDFHIP_OK;
    });
    if (rc != SDFHIP_OK) return rc;
    float pass_ms[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    if (listed)
        if (const int rc = call.elapsed(&pass_ms[0], EV_BEGIN, EV_LISTED)) return rc;
    if (searched) {
        const int from[3] = {EV_MARK, EV_MARKED, EV_SEARCHED};
        for (int k = 0; k < 3; k++)
            if (const int rc = call.elapsed(&pass_ms[k + 1], from[k], from[k] + 1)) return rc;
    }
    uint32_t total = 0;
    if (searched)
        for (uint32_t e = 0; e < n_table; e++) {
            if ((uint32_t)keys[e] == 0xFFFFFFFFu) continue;
            if (total < capacity) memcpy(out + total, &table[e], sizeof(GapRecord));
            total++;
        }
    *n_pairs = total;
    if (stats) {
        memset(stats, 0, sizeof *stats);
        stats->pairs = n_table;
        stats->pairs_searched = pairs_searched;
        stats->cells = cells;
        stats->searches = done.searches;
        stats->visited = done.visited;
        for (int k = 0; k < 4; k++) { stats->pass_ms[k] = pass_ms[k]; stats->kernel_ms += pass_ms[k]; }
        stats->total_ms = call.total_ms();
    }
    return SDFHIP_OK;
}
SDFHIP_ABI_CATCH(sdfhip_instances_gap)
