// libsdfhip.so, selection: sdfhip_scene_select -- the components of a resident scene kept, dropped or filled, the result a new
// handle (kernels: select_kernels.h).
//
// Replaces: nothing in the reference's code; a tree there is immutable, and nothing in it knows that a model has pieces.
//
// The rule, pinned (include/sdfhip.h; fp32, each operation rounded on its own in the order written):
//   labelling   sdfhip_scene_components', word for word (label_components, components_host.h); F[i]: point i's component flips
//               under the rule bits; T[i] = inside[i] XOR F[i]
//   value       v = sdfhip_scene_place's value at the identity; N(p) = the lattice points with non-zero trilinear weight at p;
//               v' = -fmaxf(fabsf(v), h) where some point of N(p) has F and all have T, fmaxf(fabsf(v), h) where some has F and none
//               has T, else v; h = 2^-8
//   tree        sdfhip_scene_place's construct rule and node order on v'
//
// Per call: the options and the list are checked, the list is sorted and deduplicated on the host, the scene is read under its lock
// (read_source), and on a stream of the call's own (CallFrame) the labelling runs as it does for sdfhip_scene_components;
// k_select_largest, k_select_decide and k_select_mark turn its records into the two bitmaps F and T; the host waits once, reads what
// the decision counted -- a listed label that is no component's, a void under KEEP_LISTED: the refusals that need the labelling --
// and frees the labelling's memory (4 bytes per point) before the tree takes its own; then level_build.h's build_levels runs
// k_select_level level by level, and the arrays go to scene_from_arrays as the placement's do.
#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Wunneeded-internal-declaration"
#include "select_kernels.h"
#include "level_build.h"      // host_support.h; Source, with_cursor, build_levels
#pragma clang diagnostic pop
#include "abi_guard.h"

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstring>
#include <vector>

using namespace sdfhip;
using namespace sdfhip::levels;

static_assert(sizeof(sdfhip_select_options) == 36 && sizeof(sdfhip_select_stats) == 64, "the selection's records of include/sdfhip.h");
static_assert(SDFHIP_SELECT_KEEP_LARGEST_SOLID == SELECT_KEEP_LARGEST && SDFHIP_SELECT_DROP_SMALL_SOLIDS == SELECT_DROP_SMALL &&
              SDFHIP_SELECT_FILL_ENCLOSED_VOIDS == SELECT_FILL_ENCLOSED && SDFHIP_SELECT_FLIP_LISTED == SELECT_FLIP_LISTED &&
              SDFHIP_SELECT_KEEP_LISTED == SELECT_KEEP_LISTED, "select_kernels.h restates the header's flags");

namespace {

constexpr uint32_t ALL_RULES = SELECT_KEEP_LARGEST | SELECT_DROP_SMALL | SELECT_FILL_ENCLOSED | SELECT_FLIP_LISTED | SELECT_KEEP_LISTED;
constexpr uint32_t LISTED_RULES = SELECT_FLIP_LISTED | SELECT_KEEP_LISTED;

// what the header refuses before any device call
int check_call(const sdfhip_scene *scene, const sdfhip_select_options *opt, const uint32_t *labels, uint32_t n_labels, sdfhip_scene **out,
               const sdfhip_octdata *host_out, sdfhip_select_options &O, CompLattice &L)
{
    const char *name = "scene_select";
    sdfhip_select_options_default(&O);
    if (opt) {
        if (const int rc = check_options_size(name, opt, sizeof(sdfhip_select_options), "sdfhip_select_options_default sets the size")) return rc;
        O = *opt;
    }
    if (!out && !host_out) return fail(SDFHIP_ERR_ARG, "%s: both outputs are null", name);
    if (O.flags & ~ALL_RULES) return fail(SDFHIP_ERR_ARG, "%s: unknown flags %#x", name, O.flags & ~ALL_RULES);
    if ((O.flags & LISTED_RULES) == LISTED_RULES) return fail(SDFHIP_ERR_ARG, "%s: both FLIP_LISTED and KEEP_LISTED: one list cannot be both", name);
    if ((O.flags & LISTED_RULES) && (!labels || !n_labels)) return fail(SDFHIP_ERR_ARG, "%s: a listed rule with no labels", name);
    if (!(O.flags & LISTED_RULES) && (labels || n_labels))
        return fail(SDFHIP_ERR_ARG, "%s: labels given without a listed rule (SDFHIP_SELECT_FLIP_LISTED or _KEEP_LISTED)", name);
    if (const int rc = check_comp_lattice(name, "lattice_depth", O.lattice_depth, O.origin, O.side, L)) return rc;
    if (O.depth < -1 || O.depth > TREE_MAX_DEPTH) return fail(SDFHIP_ERR_ARG, "%s: depth %d is neither -1 nor 0..%d", name, O.depth, TREE_MAX_DEPTH);
    if (!scene) return fail(SDFHIP_ERR_ARG, "%s: null scene", name);
    return SDFHIP_OK;
}

}  // namespace

extern "C" void sdfhip_select_options_default(sdfhip_select_options *opt)
try {
    if (!opt) { (void)fail(SDFHIP_ERR_ARG, "select_options_default: null argument"); return; }
    opt->size = (uint32_t)sizeof(sdfhip_select_options);
    opt->flags = 0u;
    opt->lattice_depth = 6u;
    opt->origin[0] = 0.0f; opt->origin[1] = 0.0f; opt->origin[2] = 0.0f;
    opt->side = 1.0f;
    opt->depth = -1;
    opt->min_points = 0u;
}
SDFHIP_ABI_CATCH_VOID(sdfhip_select_options_default)

extern "C" int sdfhip_scene_select(sdfhip_scene *scene, const sdfhip_select_options *opt, const uint32_t *labels, uint32_t n_labels,
                                   sdfhip_scene **out, sdfhip_octdata *host_out, sdfhip_select_stats *stats)
try {
    const auto t0 = std::chrono::steady_clock::now();
    sdfhip_select_options O;
    CompLattice L;
    if (const int rc = check_call(scene, opt, labels, n_labels, out, host_out, O, L)) return rc;
    std::vector<uint32_t> list(labels, labels + ((O.flags & LISTED_RULES) ? n_labels : 0u));
    std::sort(list.begin(), list.end());
    list.erase(std::unique(list.begin(), list.end()), list.end());
    const uint32_t n_list = (uint32_t)list.size();

    const Source src = read_source(scene);
    if (O.depth < 0 && src.depth > (uint32_t)TREE_MAX_DEPTH)
        return fail(SDFHIP_ERR_BAD_TREE, "scene_select: the source is not a consistent tree of at most %d levels, so it has no depth to take: give one",
                    TREE_MAX_DEPTH);
    const int depth = O.depth < 0 ? (int)src.depth : O.depth;

    CallFrame<4> call("scene_select", src.device, "SDFHIP_SELECT_FAIL_ALLOC", t0);
    CompLabels C;
    SelectHead head, empty;                 // (empty: the source of an asynchronous copy, alive until the call has waited)
    memset(&empty, 0, sizeof empty);
    empty.first_not_root = empty.first_void = 0xFFFFFFFFu;
    head = empty;
    LevelBuild R;
    if (const int rc = call.run("the source is untouched", [&](hipStream_t st) -> int {
        uint32_t *d_list = call.bufs.get<uint32_t>(n_list);
        if (n_list) HIP_TRY(hipMemcpyAsync(d_list, list.data(), (size_t)n_list * sizeof(uint32_t), hipMemcpyHostToDevice, st));
        if (const int rc = label_components(call.bufs, st, src, L, call.cs.ev[0], C)) return rc;
        const size_t words = std::max<size_t>(C.n >> 6, 1);
        uint8_t *d_decided = call.bufs.get<uint8_t>(C.total);
        SelectHead *d_head = call.bufs.get<SelectHead>(1);
        unsigned long long *d_F = call.bufs.get<unsigned long long>(words), *d_T = call.bufs.get<unsigned long long>(words);
        HIP_TRY(hipMemcpyAsync(d_head, &empty, sizeof empty, hipMemcpyHostToDevice, st));
        const uint32_t by_record = (std::max(C.total, n_list) + SELECT_THREADS - 1u) / SELECT_THREADS, by_point = (C.n + SELECT_THREADS - 1u) / SELECT_THREADS;
        if (O.flags & SELECT_KEEP_LARGEST)
            hipLaunchKernelGGL(k_select_largest, dim3((C.total + SELECT_THREADS - 1u) / SELECT_THREADS), dim3(SELECT_THREADS), 0, st, C.d_out, C.total, d_head);
        hipLaunchKernelGGL(k_select_decide, dim3(by_record), dim3(SELECT_THREADS), 0, st, C.d_out, C.total, O.flags, O.min_points, L.depth, d_list, n_list,
                           C.d_roots, C.n, d_decided, d_head);
        hipLaunchKernelGGL(k_select_mark, dim3(by_point), dim3(SELECT_THREADS), 0, st, C.d_parent, C.n, C.d_roots, C.d_pre, C.d_chunk, d_decided, d_F, d_T);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipEventRecord(call.cs.ev[1], st));
        // the call's one synchronisation of its own: what the decision counted, and with it the refusals that need the labelling
        HIP_TRY(hipMemcpyAsync(&head, d_head, sizeof head, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        if (head.not_roots)
            return fail(SDFHIP_ERR_ARG, "scene_select: label %u is not the label of a component on this lattice (%u of the %u listed are not): nothing was built",
                        head.first_not_root, head.not_roots, n_list);
        if (head.listed_voids)
            return fail(SDFHIP_ERR_ARG, "scene_select: label %u is a void, and KEEP_LISTED keeps solids (%u listed voids): nothing was built", head.first_void,
                        head.listed_voids);
        // the labelling's memory goes before the tree's comes: the bitmaps are all the levels read
        for (void *p : {(void *)C.d_parent, (void *)C.d_sign, (void *)C.d_roots, (void *)C.d_pre, (void *)C.d_chunk, (void *)C.d_stats, (void *)C.d_out,
                        (void *)d_decided, (void *)d_list})
            call.bufs.drop(p);
        const SelectLattice SL{L.ox, L.oy, L.oz, L.pitch, L.depth, d_F, d_T};
        const auto level = [&](const LevelBlock *blocks, uint32_t nblocks, uint32_t nchild, float S, int may_split, uint2 *V, uint8_t *split) {
            with_cursor(src.form, [&](auto c) {
                hipLaunchKernelGGL((k_select_level<typename decltype(c)::type>), grid_stride_blocks(64ull * nblocks, LEVEL_MAX_WORKGROUPS), dim3(LEVEL_THREADS), 0, st,
                                   src.Q, SL, blocks, nblocks, nchild, S, may_split, V, split);
            });
        };
        if (const int rc = build_levels(call.what, call.bufs, st, src.Q.n_nodes, depth, level, R, call.cs.ev[2])) return rc;
        HIP_TRY(hipEventRecord(call.cs.ev[3], st));
        HIP_TRY(hipStreamSynchronize(st));
        return SDFHIP_OK;
    })) return rc;

    float label_ms = 0.0f, kernel_ms = 0.0f, scene_ms = 0.0f;
    if (const int rc = call.elapsed(&label_ms, 0, 1)) return rc;
    if (const int rc = call.elapsed(&kernel_ms, 2, 3)) return rc;
    if (const int rc = call.finish(R.dS, R.dV, R.n_out, (int)R.depth_out, out, host_out, &scene_ms)) return rc;
    if (stats) {
        memset(stats, 0, sizeof *stats);
        stats->components = C.total; stats->solids = head.solids;
        stats->flipped_solids = head.flipped_solids; stats->flipped_voids = head.flipped_voids;
        stats->points_flipped = head.points_flipped;
        stats->nodes_in = src.Q.n_nodes; stats->nodes_out = R.n_out; stats->depth_out = R.depth_out; stats->levels = R.depth_out + 1;
        stats->samples = R.points;
        stats->label_ms = label_ms; stats->kernel_ms = kernel_ms; stats->scene_ms = scene_ms;
        stats->total_ms = call.total_ms();
    }
    return SDFHIP_OK;
}
SDFHIP_ABI_CATCH(sdfhip_scene_select)
