// The host side that the calls on a list of placed instances share: compose.hip (sdfhip_scene_compose) and instances.hip
// (sdfhip_instances_*).  What the header refuses of the list and of an instance, and how an entry of the call's instance table is
// read from its handle: one definition, so that both families refuse the same things in the same words -- only the entry point's
// name in front of the message is the caller's.  Everything here is inline.
#pragma once
#include "compose_instance.h"   // ComposeInstance
#include "level_build.h"        // host_support.h; Source, read_source, check_similarity

#include <algorithm>
#include <cstdio>
#include <utility>
#include <vector>

namespace sdfhip {
namespace levels {

constexpr uint32_t MAX_INSTANCES = 4096;

// what the header refuses of instance k, before any device call: the op, the placement's checks (check_similarity), the handle.
// name: the entry point's, as its messages begin
inline int check_instance(const char *name, const sdfhip_instance *in, uint32_t k)
{
    if (in->op < SDFHIP_COMBINE_UNION || in->op > SDFHIP_COMBINE_SUBTRACT) return fail(SDFHIP_ERR_ARG, "%s: instance %u: unknown op %d", name, k, in->op);
    if (k == 0 && in->op != SDFHIP_COMBINE_UNION)
        return fail(SDFHIP_ERR_ARG, "%s: instance 0: op %d, but the first instance has nothing to join: SDFHIP_COMBINE_UNION", name, in->op);
    char what[64];
    snprintf(what, sizeof what, "%s: instance %u", name, k);
    if (const int rc = check_similarity(what, in->rotation, in->scale, in->translation)) return rc;
    if (!in->scene) return fail(SDFHIP_ERR_ARG, "%s: instance %u: null scene", name, k);
    return SDFHIP_OK;
}

// ... and of the list: a null list, a count outside 1..4096
inline int check_instance_count(const char *name, const sdfhip_instance *instances, uint32_t n_instances)
{
    if (!instances) return fail(SDFHIP_ERR_ARG, "%s: null instance list", name);
    if (n_instances < 1 || n_instances > MAX_INSTANCES) return fail(SDFHIP_ERR_ARG, "%s: %u instances: 1..%u", name, n_instances, MAX_INSTANCES);
    return SDFHIP_OK;
}

// The distinct handles of a list, each read once (read_source: under that handle's lock, one handle after the other and never two
// locks at once, the lock released before any work is issued: the records are only ever read)
typedef std::vector<std::pair<const sdfhip_scene *, Source>> InstanceSources;

// Entry k of the call's table from instance k: its source (read now if the list has not named it before; *fresh says so), the one-device
// rule, the map, the op and the cursor form.  *source: what was read of the handle
inline int read_instance(const char *name, InstanceSources &sources, const sdfhip_instance &in, uint32_t k, ComposeInstance &I, const Source **source,
                         bool *fresh)
{
    auto at = std::find_if(sources.begin(), sources.end(), [&](const auto &s) { return s.first == in.scene; });
    *fresh = at == sources.end();
    if (*fresh) {
        sources.emplace_back(in.scene, read_source(in.scene));
        at = sources.end() - 1;
    }
    const Source &src = at->second;
    *source = &src;
    if (src.device != sources.front().second.device)
        return fail(SDFHIP_ERR_ARG, "%s: instance %u lives on device %d, instance 0 on device %d: one device", name, k, src.device,
                    sources.front().second.device);
    I.Q = src.Q;
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) I.M.r[i][j] = in.rotation[i][j];
    I.M.s = in.scale; I.M.inv = 1.0f / in.scale;
    I.M.tx = in.translation[0]; I.M.ty = in.translation[1]; I.M.tz = in.translation[2];
    I.op = in.op; I.form = (int32_t)src.form;
    return SDFHIP_OK;
}

}  // namespace levels
}  // namespace sdfhip
