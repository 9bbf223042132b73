// The writers of a mesh from sdfhip_scene_mesh, and its release: host code, no device.
//
//   sdfhip_mesh_save_ply   binary little-endian PLY: the vertex element first, x y z nx ny nz as floats -- what sdfhip_load_ply
//                          (point_readers.cpp) and the reference's LoadPly read back as a point cloud -- then a face element of
//                          uchar / int lists (3i, 3i+1, 3i+2): the soup has no index buffer, every triangle owns its vertices
//   sdfhip_mesh_save_obj   `v` and `vn` lines printed with %.9g (nine significant digits carry every fp32 through the text), then
//                          `f a//a b//b c//c`: sdfhip_load_obj gives the same vertices back
//   sdfhip_mesh_free       releases verts6
//   sdfhip_load_ply_mesh / _obj_mesh   the way back in, WITH the faces (sdfhip_load_ply / _obj of point_readers.cpp read the vertices as a
//                          point cloud and drop them): the same format limits, polygons fanned from their first vertex, the result a
//                          soup like sdfhip_scene_mesh's -- what sdfhip_trimesh_prepare takes
//
// Replaces: nothing in the reference's code -- it reads meshes (ply_reader.cpp, obj_reader.cpp) and writes none.
#include "abi_guard.h"
#include <cctype>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <new>
#include <string>
#include <vector>

using namespace sdfhip;

namespace {

struct File {
    FILE *f = nullptr;
    ~File() { if (f) fclose(f); }
    // the buffered data reaches the file, or the call fails
    bool close() { const bool ok = f && fclose(f) == 0; f = nullptr; return ok; }
};

int check_mesh(const char *what, const sdfhip_mesh *mesh, const char *path)
{
    if (!mesh || !path) return fail(SDFHIP_ERR_ARG, "%s: null argument", what);
    if (mesh->n_triangles && !mesh->verts6) return fail(SDFHIP_ERR_ARG, "%s: %u triangles and no vertices", what, mesh->n_triangles);
    if (mesh->n_triangles > 0x7FFFFFFFu / 3u) return fail(SDFHIP_ERR_ARG, "%s: %u triangles: their vertices do not fit an int index", what, mesh->n_triangles);
    return SDFHIP_OK;
}

}  // namespace

extern "C" void sdfhip_mesh_free(sdfhip_mesh *mesh)
try {
    if (!mesh) { (void)fail(SDFHIP_ERR_ARG, "mesh_free: null argument"); return; }
    free(mesh->verts6);
    mesh->verts6 = nullptr; mesh->n_triangles = 0;
}
SDFHIP_ABI_CATCH_VOID(sdfhip_mesh_free)

extern "C" int sdfhip_mesh_save_ply(const sdfhip_mesh *mesh, const char *path)
try {
    if (const int rc = check_mesh("mesh_save_ply", mesh, path)) return rc;
    const size_t nt = mesh->n_triangles, nv = 3 * nt;
    File out;
    out.f = fopen(path, "wb");
    if (!out.f) return fail(SDFHIP_ERR_IO, "mesh_save_ply: could not open %s for writing", path);
    bool ok = fprintf(out.f, "ply\nformat binary_little_endian 1.0\ncomment sdfhip_mesh_save_ply\nelement vertex %zu\n"
                             "property float x\nproperty float y\nproperty float z\nproperty float nx\nproperty float ny\nproperty float nz\n"
                             "element face %zu\nproperty list uchar int vertex_indices\nend_header\n", nv, nt) > 0;
    ok = ok && (nv == 0 || fwrite(mesh->verts6, 24, nv, out.f) == nv);
    // faces: {uchar 3, int a, int b, int c}, 13 bytes each, a block at a time
    const size_t block = 1 << 16;
    std::vector<unsigned char> faces(13 * (nt < block ? nt : block));
    for (size_t first = 0; ok && first < nt; first += block) {
        const size_t m = nt - first < block ? nt - first : block;
        for (size_t k = 0; k < m; k++) {
            unsigned char *p = faces.data() + 13 * k;
            const int32_t idx[3] = { (int32_t)(3 * (first + k)), (int32_t)(3 * (first + k) + 1), (int32_t)(3 * (first + k) + 2) };
            p[0] = 3;
            memcpy(p + 1, idx, 12);
        }
        ok = fwrite(faces.data(), 13, m, out.f) == m;
    }
    if (!out.close() || !ok) return fail(SDFHIP_ERR_IO, "mesh_save_ply: writing %s failed", path);
    return SDFHIP_OK;
}
SDFHIP_ABI_CATCH(sdfhip_mesh_save_ply)

extern "C" int sdfhip_mesh_save_obj(const sdfhip_mesh *mesh, const char *path)
try {
    if (const int rc = check_mesh("mesh_save_obj", mesh, path)) return rc;
    const size_t nt = mesh->n_triangles, nv = 3 * nt;
    File out;
    out.f = fopen(path, "w");
    if (!out.f) return fail(SDFHIP_ERR_IO, "mesh_save_obj: could not open %s for writing", path);
    bool ok = fprintf(out.f, "# sdfhip_mesh_save_obj: %zu triangles\n", nt) > 0;
    const float *v = mesh->verts6;
    for (size_t k = 0; ok && k < nv; k++) ok = fprintf(out.f, "v %.9g %.9g %.9g\n", (double)v[6 * k], (double)v[6 * k + 1], (double)v[6 * k + 2]) > 0;
    for (size_t k = 0; ok && k < nv; k++) ok = fprintf(out.f, "vn %.9g %.9g %.9g\n", (double)v[6 * k + 3], (double)v[6 * k + 4], (double)v[6 * k + 5]) > 0;
    for (size_t k = 0; ok && k < nt; k++)
        ok = fprintf(out.f, "f %zu//%zu %zu//%zu %zu//%zu\n", 3 * k + 1, 3 * k + 1, 3 * k + 2, 3 * k + 2, 3 * k + 3, 3 * k + 3) > 0;
    if (!out.close() || !ok) return fail(SDFHIP_ERR_IO, "mesh_save_obj: writing %s failed", path);
    return SDFHIP_OK;
}
SDFHIP_ABI_CATCH(sdfhip_mesh_save_obj)

namespace {

// verts: 6 floats per indexed vertex; corners: the triangles' vertex indices (and with `normals`, a normal index per corner, -1 = none)
int hand_over_soup(const char *what, const std::vector<float> &verts, const std::vector<uint32_t> &corners, const std::vector<float> *normals,
                   const std::vector<int64_t> *corner_normals, sdfhip_mesh *out)
{
    const size_t nt = corners.size() / 3;
    if (nt > 0x7FFFFFFFu / 3u) return fail(SDFHIP_ERR_IO, "%s: more than 2^31 - 1 triangle corners", what);
    float *v = static_cast<float *>(malloc(nt ? nt * 18 * sizeof(float) : 4));
    if (!v) return fail(SDFHIP_ERR_NOMEM, "%s: out of memory for %zu triangles", what, nt);
    for (size_t k = 0; k < corners.size(); k++) {
        memcpy(v + 6 * k, &verts[(size_t)corners[k] * 6], 24);
        if (normals) {
            const int64_t ni = (*corner_normals)[k];
            if (ni >= 0) memcpy(v + 6 * k + 3, &(*normals)[(size_t)ni * 3], 12);
            else v[6 * k + 3] = v[6 * k + 4] = v[6 * k + 5] = 0.0f;
        }
    }
    out->n_triangles = (uint32_t)nt;
    out->verts6 = v;
    return SDFHIP_OK;
}

}  // namespace

extern "C" int sdfhip_load_ply_mesh(const char *path, sdfhip_mesh *out)
try {
    if (!path || !out) return fail(SDFHIP_ERR_ARG, "load_ply_mesh: null argument");
    out->n_triangles = 0; out->verts6 = nullptr;
    std::ifstream file(path, std::ios::binary);
    if (!file.is_open()) return fail(SDFHIP_ERR_IO, "load_ply_mesh: could not open %s", path);
    file.exceptions(std::ios::badbit);
    std::string word;
    auto bad = [&]() { return fail(SDFHIP_ERR_IO, "load_ply_mesh: %s: file format is unsupported or invalid", path); };
    if (!(file >> word) || word != "ply") return bad();
    if (!(file >> word) || word != "format") return bad();
    if (!(file >> word)) return bad();
    if (word == "ascii") return fail(SDFHIP_ERR_IO, "load_ply_mesh: %s: ASCII PLY is not supported (binary_little_endian only)", path);
    if (word == "binary_big_endian") return fail(SDFHIP_ERR_IO, "load_ply_mesh: %s: big-endian PLY is not supported", path);
    if (word != "binary_little_endian") return bad();
    // the header: `element vertex N` first (six floats per vertex, as sdfhip_load_ply takes them), then `element face M` whose one
    // property is `list uchar int`
    long long nv = -1, nf = -1;
    bool list_ok = false;
    while (file >> word) {
        if (word == "end_header") break;
        if (word == "element") {
            std::string name; long long count = -1;
            if (!(file >> name >> count) || count < 0) return bad();
            if (name == "vertex" && nv < 0 && nf < 0) nv = count;
            else if (name == "face" && nv >= 0 && nf < 0) nf = count;
            else return bad();
        } else if (word == "property" && nf >= 0) {
            std::string a, b, c, name;
            if (!(file >> a >> b >> c >> name) || list_ok) return bad();
            if (a != "list" || (b != "uchar" && b != "uint8") || (c != "int" && c != "int32" && c != "uint" && c != "uint32")) return bad();
            list_ok = true;
        }
    }
    if (word != "end_header" || nv < 0 || nf < 0 || (nf > 0 && !list_ok) || nv > 0x7FFFFFFFll / 24 || nf > 0x7FFFFFFFll) return bad();
    file.get();                                   // the newline that ends the header
    try {
        std::vector<float> verts((size_t)nv * 6);
        file.read((char *)verts.data(), (std::streamsize)(verts.size() * sizeof(float)));
        if ((size_t)file.gcount() != verts.size() * sizeof(float))
            return fail(SDFHIP_ERR_IO, "load_ply_mesh: %s holds fewer than %lld vertices of 6 floats", path, nv);
        std::vector<uint32_t> corners;
        corners.reserve((size_t)nf * 3);
        std::vector<int32_t> idx;
        for (long long f = 0; f < nf; f++) {
            const int k = file.get();
            if (k == std::char_traits<char>::eof() || k < 3) return fail(SDFHIP_ERR_IO, "load_ply_mesh: %s: face %lld is missing or has fewer than 3 vertices", path, f);
            idx.resize((size_t)k);
            file.read((char *)idx.data(), (std::streamsize)(4 * k));
            if (file.gcount() != (std::streamsize)(4 * k)) return fail(SDFHIP_ERR_IO, "load_ply_mesh: %s ends inside face %lld", path, f);
            for (int i = 0; i < k; i++)
                if (idx[(size_t)i] < 0 || idx[(size_t)i] >= nv) return fail(SDFHIP_ERR_IO, "load_ply_mesh: %s: face %lld: index out of range", path, f);
            for (int i = 1; i + 1 < k; i++) corners.insert(corners.end(), { (uint32_t)idx[0], (uint32_t)idx[(size_t)i], (uint32_t)idx[(size_t)i + 1] });
        }
        return hand_over_soup("load_ply_mesh", verts, corners, nullptr, nullptr, out);
    } catch (const std::bad_alloc &) {
        return fail(SDFHIP_ERR_NOMEM, "load_ply_mesh: out of memory");
    }
}
SDFHIP_ABI_CATCH(sdfhip_load_ply_mesh)

extern "C" int sdfhip_load_obj_mesh(const char *path, sdfhip_mesh *out)
try {
    if (!path || !out) return fail(SDFHIP_ERR_ARG, "load_obj_mesh: null argument");
    out->n_triangles = 0; out->verts6 = nullptr;
    std::ifstream file(path);
    if (!file.is_open()) return fail(SDFHIP_ERR_IO, "load_obj_mesh: could not open %s", path);
    file.exceptions(std::ios::badbit);            // (see sdfhip_load_obj: a failed extraction must not read as the end of the file)
    try {
        std::vector<float> verts, normals;        // 6 per vertex (normal 0), 3 per normal
        std::vector<uint32_t> corners;
        std::vector<int64_t> corner_normals;
        std::vector<uint32_t> fv;
        std::vector<int64_t> fn;
        std::string line;
        long lineno = 0;
        while (std::getline(file, line)) {
            lineno++;
            size_t i = 0;
            while (i < line.size() && isspace((unsigned char)line[i])) i++;
            if (i == line.size()) continue;
            const char *s = line.c_str() + i;
            auto bad = [&]() { return fail(SDFHIP_ERR_IO, "load_obj_mesh: %s:%ld: file format is unsupported or invalid", path, lineno); };
            if (s[0] == '#' || s[0] == 'o' || s[0] == 's') continue;
            if (s[0] == 'v' && s[1] == 't') continue;
            if (s[0] == 'v' && (s[1] == ' ' || s[1] == 'n')) {
                char *end = nullptr;
                const char *p = s + 2;
                float f[3];
                for (int k = 0; k < 3; k++) { f[k] = strtof(p, &end); if (end == p) return bad(); p = end; }
                if (s[1] == ' ') verts.insert(verts.end(), { f[0], f[1], f[2], 0.0f, 0.0f, 0.0f });
                else normals.insert(normals.end(), { f[0], f[1], f[2] });
                continue;
            }
            if (s[0] == 'f' && (s[1] == ' ' || s[1] == '\t')) {
                // a corner: a | a/b | a//c | a/b/c; a negative index counts back from the elements read so far
                fv.clear(); fn.clear();
                const char *p = s + 1;
                const auto resolve = [](long v, size_t count, int64_t *out_index) {
                    const int64_t k = v > 0 ? (int64_t)v - 1 : (int64_t)count + v;
                    *out_index = k;
                    return v != 0 && k >= 0 && (uint64_t)k < count;
                };
                for (;;) {
                    while (*p == ' ' || *p == '\t' || *p == '\r') p++;
                    if (!*p) break;
                    char *end = nullptr;
                    const long vi = strtol(p, &end, 10);
                    if (end == p) return bad();
                    p = end;
                    int64_t v_index, n_index = -1;
                    if (*p == '/') {
                        p++;
                        if (*p != '/' && *p != ' ' && *p != '\t' && *p != '\r' && *p) { (void)strtol(p, &end, 10); if (end == p) return bad(); p = end; }
                        if (*p == '/') {
                            p++;
                            const long ni = strtol(p, &end, 10);
                            if (end == p) return bad();
                            p = end;
                            if (!resolve(ni, normals.size() / 3, &n_index)) return fail(SDFHIP_ERR_IO, "load_obj_mesh: %s:%ld: face index out of range", path, lineno);
                        }
                    }
                    if (*p && *p != ' ' && *p != '\t' && *p != '\r') return bad();
                    if (!resolve(vi, verts.size() / 6, &v_index)) return fail(SDFHIP_ERR_IO, "load_obj_mesh: %s:%ld: face index out of range", path, lineno);
                    fv.push_back((uint32_t)v_index); fn.push_back(n_index);
                }
                if (fv.size() < 3) return bad();
                for (size_t k = 1; k + 1 < fv.size(); k++) {
                    corners.insert(corners.end(), { fv[0], fv[k], fv[k + 1] });
                    corner_normals.insert(corner_normals.end(), { fn[0], fn[k], fn[k + 1] });
                }
                continue;
            }
            return bad();
        }
        if (verts.size() / 6 > 0x7FFFFFFFu) return fail(SDFHIP_ERR_IO, "load_obj_mesh: %s: too many vertices", path);
        return hand_over_soup("load_obj_mesh", verts, corners, &normals, &corner_normals, out);
    } catch (const std::bad_alloc &) {
        return fail(SDFHIP_ERR_NOMEM, "load_obj_mesh: out of memory");
    } catch (const std::ios_base::failure &) {
        return fail(SDFHIP_ERR_IO, "load_obj_mesh: %s: read error", path);
    }
}
SDFHIP_ABI_CATCH(sdfhip_load_obj_mesh)
