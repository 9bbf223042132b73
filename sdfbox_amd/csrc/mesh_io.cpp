// The writers of a mesh from sdfhip_scene_mesh, and its release: host code, no device.
//
//   sdfhip_mesh_save_ply   binary little-endian PLY: the vertex element first, x y z nx ny nz as floats -- what sdfhip_load_ply
//                          (point_readers.cpp) and the reference's LoadPly read back as a point cloud -- then a face element of
//                          uchar / int lists (3i, 3i+1, 3i+2): the soup has no index buffer, every triangle owns its vertices
//   sdfhip_mesh_save_obj   `v` and `vn` lines printed with %.9g (nine significant digits carry every fp32 through the text), then
//                          `f a//a b//b c//c`: sdfhip_load_obj gives the same vertices back
//   sdfhip_mesh_free       releases verts6
//
// Replaces: nothing in the reference's code -- it reads meshes (ply_reader.cpp, obj_reader.cpp) and writes none.
#include "abi_guard.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>
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
