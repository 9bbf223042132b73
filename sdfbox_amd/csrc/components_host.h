// What the labelling of a scene's components shares between its two callers: components.hip (sdfhip_scene_components[_device], which
// returns the records and the labels) and select.hip (sdfhip_scene_select, which decides on the records and builds a tree).  The
// records' types, the lattice, value(p) -- a template, so any .hip may include it -- and the declarations of the two host functions
// that components.hip defines: the kernels of components_kernels.h are not templates and stay in that one translation unit.
//
// Replaces: nothing in the reference's code.
#pragma once
#include "query_kernels.h"   // QueryScene, grid_of; raymarch_device.h: the cursors, find_fresh, sample_after_find
#include "level_build.h"     // host_support.h: DeviceBuffers; Source

namespace sdfhip {

constexpr uint32_t COMP_STAT_SLOTS = 64, COMP_SOLID = 1u;

// sdfhip_component of include/sdfhip.h
struct Component {
    uint32_t label, flags, points, reserved;
    uint32_t lo[3], hi[3];
    unsigned long long sum[3];
};
static_assert(sizeof(Component) == 64, "sdfhip_component of include/sdfhip.h");

struct CompStat {
    unsigned long long inside;
    uint32_t solids, pad;
};

// the call's lattice as the kernels read it
struct CompLattice {
    float ox, oy, oz, pitch;
    uint32_t depth;         // 0..9
    uint32_t n_blocks;      // 8^max(depth - 2, 0)
};

// value(p) of the rule: k_volume_out's lines (volume_kernels.h), word for word -- the clamp to the cube, the scene's distance there
// (what sdfhip_scene_sample returns), continued outside at slope 1
template <class CursorT> __device__ __forceinline__ float components_value(const QueryScene &Q, float px, float py, float pz)
{
    const float cx = __builtin_fminf(__builtin_fmaxf(px, 0.0f), 1.0f);
    const float cy = __builtin_fminf(__builtin_fmaxf(py, 0.0f), 1.0f);
    const float cz = __builtin_fminf(__builtin_fmaxf(pz, 0.0f), 1.0f);
    const float ex = px - cx, ey = py - cy, ez = pz - cz;
    CursorT c;
    c.loads = 0;
    c.reset(Q.nodes[0]);
    typename CursorT::Pos u;
    find_fresh(c, Q.nodes, grid_of(Q), Q.n_nodes, nullptr, 0u, cx, cy, cz, u);
    const float D = sample_after_find(c, u, cx, cy, cz);
    return D + sqrtf((ex * ex + ey * ey) + ez * ez);
}

// What the labelling leaves in the caller's buffers (DeviceBuffers: freed with the call): every point's label, the blocks' sign words,
// the root bitmap, its ranks (pre, chunk: scan_device.h's rank_in_bitmap gives a label's slot), the counters and the record table,
// `total` records in ascending label order
struct CompLabels {
    uint32_t n = 0, m = 0, nchunk = 0, total = 0;        // points; words of the root bitmap; chunks of its scan; records
    uint32_t *d_parent = nullptr;
    unsigned long long *d_sign = nullptr;
    uint32_t *d_roots = nullptr, *d_pre = nullptr, *d_chunk = nullptr;
    CompStat *d_stats = nullptr;
    Component *d_out = nullptr;
};

// components.hip.  What both calls refuse of a lattice, before any device call: `field` names the depth in the message.  Fills L.
int check_comp_lattice(const char *name, const char *field, uint32_t depth, const float *origin, float side, CompLattice &L);
// The passes up to and including k_comp_records on `st`: allocates, in this order, the parents, the sign words, the root bitmap, its
// two scans, the counters and (after the one host synchronisation, whose count sizes it) the record table.  started: recorded once
// the buffers are there.  When it returns the last two kernels may still be in flight.  Throws NoMem (DeviceBuffers).
int label_components(DeviceBuffers &bufs, hipStream_t st, const levels::Source &src, const CompLattice &L, hipEvent_t started, CompLabels &C);

}  // namespace sdfhip
