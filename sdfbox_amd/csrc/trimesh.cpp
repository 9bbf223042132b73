// Triangle mesh -> records for sdfhip_trimesh_build (trigen.hip): host code, no device.
//
//   sdfhip_trimesh_prepare   the optional fit, the weld, the dropped triangles, and per triangle its face normal and the
//                            angle-weighted pseudonormals of its three edges and three vertices (Baerentzen & Aanaes), in double
//                            from the fp32 positions, rounded once: the only transcendental arithmetic of the feature (atan2) is
//                            here, outside the part that is pinned bit for bit
//   sdfhip_trimesh_free      releases the records
//
// Replaces: nothing in the live reference (include/sdfhip.h has the rule and what it stands in for).
#include "abi_guard.h"
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <unordered_map>
#include <vector>

using namespace sdfhip;

static_assert(sizeof(sdfhip_trimesh_options) == 12, "the options record of include/sdfhip.h");

namespace {

struct V3 { double x, y, z; };
inline V3 sub(V3 a, V3 b) { return { a.x - b.x, a.y - b.y, a.z - b.z }; }
inline V3 cross(V3 a, V3 b) { return { a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x }; }
inline double dot(V3 a, V3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
inline double norm(V3 a) { return std::sqrt(dot(a, a)); }
inline void add_scaled(V3 &s, V3 a, double w) { s.x += a.x * w; s.y += a.y * w; s.z += a.z * w; }

struct Key3 {
    uint32_t b[3];
    bool operator==(const Key3 &o) const { return b[0] == o.b[0] && b[1] == o.b[1] && b[2] == o.b[2]; }
};
struct Key3Hash {
    size_t operator()(const Key3 &k) const
    {
        uint64_t h = k.b[0] * 0x9E3779B97F4A7C15ull;
        h = (h ^ k.b[1]) * 0xC2B2AE3D27D4EB4Full;
        h = (h ^ k.b[2]) * 0x165667B19E3779F9ull;
        return (size_t)(h ^ (h >> 29));
    }
};
struct EdgeSum { V3 n; uint32_t faces; };

int check_options(const sdfhip_trimesh_options *opt, int32_t *fit, float *fill)
{
    *fit = 0; *fill = 0.8f;
    if (!opt) return SDFHIP_OK;
    if (const int rc = check_options_size("trimesh_prepare", opt, sizeof(sdfhip_trimesh_options), "sdfhip_trimesh_options_default sets the size")) return rc;
    if (opt->fit < -1 || opt->fit > 1) return fail(SDFHIP_ERR_ARG, "trimesh_prepare: fit %d is none of -1, 0, 1", opt->fit);
    if (opt->fit == 1) *fit = 1;
    if (opt->fill != -1.0f) {
        if (!(opt->fill > 0.0f && opt->fill <= 1024.0f)) return fail(SDFHIP_ERR_ARG, "trimesh_prepare: fill must be in (0, 1024] (or -1)");
        *fill = opt->fill;
    }
    return SDFHIP_OK;
}

inline void put(float *dst, V3 v) { dst[0] = (float)v.x; dst[1] = (float)v.y; dst[2] = (float)v.z; }
// the sum normalised, or the triangle's own face normal where it is zero (or not finite)
inline V3 unit_or(V3 s, V3 face)
{
    const double l = norm(s);
    if (!(l > 0.0) || !std::isfinite(l)) return face;
    return { s.x / l, s.y / l, s.z / l };
}

}  // namespace

extern "C" void sdfhip_trimesh_options_default(sdfhip_trimesh_options *opt)
try {
    if (!opt) { (void)fail(SDFHIP_ERR_ARG, "trimesh_options_default: null argument"); return; }
    opt->size = (uint32_t)sizeof(sdfhip_trimesh_options);
    opt->fit = -1;
    opt->fill = -1.0f;
}
SDFHIP_ABI_CATCH_VOID(sdfhip_trimesh_options_default)

extern "C" void sdfhip_trimesh_free(sdfhip_trimesh *mesh)
try {
    if (!mesh) { (void)fail(SDFHIP_ERR_ARG, "trimesh_free: null argument"); return; }
    free(mesh->records);
    mesh->records = nullptr; mesh->n_records = 0;
}
SDFHIP_ABI_CATCH_VOID(sdfhip_trimesh_free)

extern "C" int sdfhip_trimesh_prepare(const float *verts, uint32_t n_triangles, uint32_t stride, const sdfhip_trimesh_options *opt,
                                      sdfhip_trimesh *out)
try {
    if (!verts || !out) return fail(SDFHIP_ERR_ARG, "trimesh_prepare: null argument");
    memset(out, 0, sizeof *out);
    out->scale = 1.0f;
    if (n_triangles == 0) return fail(SDFHIP_ERR_ARG, "trimesh_prepare: no triangles");
    if (stride != 3 && stride != 6) return fail(SDFHIP_ERR_ARG, "trimesh_prepare: a stride of %u floats is neither 3 nor 6", stride);
    int32_t fit; float fill;
    if (const int rc = check_options(opt, &fit, &fill)) return rc;

    const size_t nv = (size_t)n_triangles * 3;
    std::vector<float> P(nv * 3);
    float lo[3] = { INFINITY, INFINITY, INFINITY }, hi[3] = { -INFINITY, -INFINITY, -INFINITY };
    for (size_t v = 0; v < nv; v++)
        for (int k = 0; k < 3; k++) {
            const float x = verts[v * stride + k];
            if (!std::isfinite(x)) return fail(SDFHIP_ERR_ARG, "trimesh_prepare: vertex %zu has a coordinate that is not finite", v);
            P[v * 3 + k] = x;
            lo[k] = fminf(lo[k], x); hi[k] = fmaxf(hi[k], x);
        }
    if (fit) {
        // fp32, each operation rounded where it is written (-ffp-contract=off; float arithmetic is not widened on this target)
        float mid[3], ext = 0.0f;
        for (int k = 0; k < 3; k++) {
            mid[k] = (lo[k] + hi[k]) * 0.5f;
            ext = fmaxf(ext, hi[k] - lo[k]);
        }
        if (!(ext > 0.0f) || !std::isfinite(ext)) return fail(SDFHIP_ERR_ARG, "trimesh_prepare: the bounding box has no extent to fit");
        const float s = fill / ext;
        for (size_t v = 0; v < nv; v++)
            for (int k = 0; k < 3; k++) P[v * 3 + k] = (P[v * 3 + k] - mid[k]) * s + 0.5f;
        out->scale = s;
        for (int k = 0; k < 3; k++) out->offset[k] = mid[k];
    }
    for (size_t i = 0; i < nv * 3; i++) {
        if (!(fabsf(P[i]) <= 1024.0f)) return fail(SDFHIP_ERR_ARG, "trimesh_prepare: vertex %zu lies beyond |coordinate| <= 1024", i / 3);
        if (P[i] == 0.0f) P[i] = 0.0f;              // -0 -> +0
    }

    // the triangles kept, with their unit face normals
    std::vector<uint32_t> kept;
    std::vector<V3> face;
    const auto pos = [&](size_t v) { return V3{ (double)P[v * 3], (double)P[v * 3 + 1], (double)P[v * 3 + 2] }; };
    for (uint32_t t = 0; t < n_triangles; t++) {
        const V3 a = pos(3 * (size_t)t), b = pos(3 * (size_t)t + 1), c = pos(3 * (size_t)t + 2);
        const V3 ab = sub(b, a), ac = sub(c, a), bc = sub(c, b), n = cross(ab, ac);
        const double len = norm(n), area = 0.5 * len;
        const double longest = fmax(dot(ab, ab), fmax(dot(ac, ac), dot(bc, bc)));
        if (!(area > 0.0) || area < ldexp(1.0, -40) * longest) { out->n_dropped++; continue; }
        kept.push_back(t);
        face.push_back(V3{ n.x / len, n.y / len, n.z / len });
    }
    if (kept.empty()) return fail(SDFHIP_ERR_ARG, "trimesh_prepare: every one of the %u triangles is degenerate", n_triangles);

    // weld by bits; sum the edges' and the vertices' pseudonormals over the triangles kept, in their order
    std::unordered_map<Key3, uint32_t, Key3Hash> ids;
    ids.reserve(kept.size() * 2);
    std::vector<uint32_t> vid(kept.size() * 3);
    std::vector<V3> vsum;
    std::unordered_map<uint64_t, EdgeSum> edges;
    edges.reserve(kept.size() * 2);
    const auto edge_key = [](uint32_t u, uint32_t v) { return u < v ? ((uint64_t)u << 32 | v) : ((uint64_t)v << 32 | u); };
    for (size_t i = 0; i < kept.size(); i++) {
        const size_t v0 = 3 * (size_t)kept[i];
        for (int k = 0; k < 3; k++) {
            Key3 key;
            memcpy(key.b, &P[(v0 + k) * 3], 12);
            const auto it = ids.emplace(key, (uint32_t)ids.size()).first;
            vid[3 * i + k] = it->second;
            if (it->second == vsum.size()) vsum.push_back(V3{ 0, 0, 0 });
        }
        const V3 p[3] = { pos(v0), pos(v0 + 1), pos(v0 + 2) };
        for (int k = 0; k < 3; k++) {
            const V3 u = sub(p[(k + 1) % 3], p[k]), v = sub(p[(k + 2) % 3], p[k]);
            const double angle = std::atan2(norm(cross(u, v)), dot(u, v));
            add_scaled(vsum[vid[3 * i + k]], face[i], angle);
            EdgeSum &e = edges.emplace(edge_key(vid[3 * i + k], vid[3 * i + (k + 1) % 3]), EdgeSum{ { 0, 0, 0 }, 0 }).first->second;
            add_scaled(e.n, face[i], 1.0);
            e.faces++;
        }
    }
    out->n_vertices = (uint32_t)ids.size();
    out->n_edges = (uint32_t)edges.size();
    for (const auto &e : edges) out->open_edges += e.second.faces != 2;

    float *R = static_cast<float *>(malloc(kept.size() * 128));
    if (!R) return fail(SDFHIP_ERR_NOMEM, "trimesh_prepare: out of memory for %zu records", kept.size());
    for (size_t i = 0; i < kept.size(); i++) {
        float *r = R + 32 * i;
        memcpy(r, &P[9 * (size_t)kept[i]], 36);
        put(r + 9, face[i]);
        for (int k = 0; k < 3; k++) {                            // edges ab, bc, ca; vertices a, b, c
            put(r + 12 + 3 * k, unit_or(edges[edge_key(vid[3 * i + k], vid[3 * i + (k + 1) % 3])].n, face[i]));
            put(r + 21 + 3 * k, unit_or(vsum[vid[3 * i + k]], face[i]));
        }
        memcpy(r + 30, &kept[i], 4);
        r[31] = 0.0f;
    }
    out->n_records = (uint32_t)kept.size();
    out->records = R;
    return SDFHIP_OK;
}
SDFHIP_ABI_CATCH(sdfhip_trimesh_prepare)
