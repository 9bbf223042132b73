// sdfbox.hpp -- the host side of SdfBox's hot path, in C++, above the C ABI of sdfhip.h.
//
// The reference's host is C# (no .NET toolchain in the build image), so this header mirrors
// the classes a SdfBox maintainer knows -- same names, same argument meaning, same flow --
// as a header-only C++ layer; it is what tests/cpp_host.cpp drives.  Errors surface as
// SDFbox::Error (the reference lets native exceptions cross the FFI; here they are
// status codes below this layer and one C++ exception type above it).
//
//   SDFbox::OctLean, SDFbox::OctData      SdfBox/Program.cs:339-350, 503-667
//   SDFbox::OctData::NativeOctData        SdfBox/Program.cs:579-667 (Generate: .asdf, or
//                                         .ply/.obj -> SdfGen -> Save next to the mesh)
//   SDFbox::FileFormat, Logic::FormatOf, Logic::AutocompleteFile, Logic::MakeData
//                                         SdfBox/Logic.cs:87-151, 399-404
//   SDFbox::Logic::State/Heading/Position SdfBox/Logic.cs:30-78
//   SDFbox::Model::MaxDepth               SdfBox/Model.cs:18
//   SDFbox::Program::Load/Draw            SdfBox/Program.cs:79-110, 167-173 (compute pass only)
#pragma once
#include "sdfhip.h"

#include <cstring>
#include <fstream>
#include <stdexcept>
#include <string>
#include <vector>

namespace SDFbox {

struct Error : std::runtime_error {
    int code;
    Error(int c, const std::string &what) : std::runtime_error(what), code(c) {}
};
inline void Check(int rc)
{
    if (rc != SDFHIP_OK) throw Error(rc, std::string("sdfhip: ") + sdfhip_last_error());
}

enum class FileFormat { Invalid = -1, ASDF = 0, Stanford = 1, Wavefront = 2 };   // Logic.cs:399-404

struct OctLean {                     // Program.cs:339-350
    int32_t Parent, Children;
};
typedef sdfhip_info Info;            // Logic.cs:407-420, byte for byte

struct Model {
    static constexpr int MaxDepth = 10;   // Model.cs:18
};

class OctData {                      // Program.cs:503-577 (without the texture swizzle: not needed)
public:
    std::vector<OctLean> Structs;
    std::vector<uint8_t> Values;     // 8 per node, corner k = x + 2y + 4z
    int Length() const { return (int)Structs.size(); }

    // Program.cs:579-667
    struct NativeOctData {
        // Generate(path, type): load an .asdf, or import a mesh, build the ASDF on the GPU and
        // cache it as <mesh>.asdf next to the source (Program.cs:613-650)
        static OctData Generate(const std::string &path, FileFormat type, int device = 0)
        {
            sdfhip_octdata nod{};
            if (type == FileFormat::ASDF) {
                Check(sdfhip_asdf_load(path.c_str(), &nod));
            } else {
                sdfhip_points vertices{};
                if (type == FileFormat::Stanford) Check(sdfhip_load_ply(path.c_str(), &vertices));
                else if (type == FileFormat::Wavefront) Check(sdfhip_load_obj(path.c_str(), &vertices));
                else throw Error(SDFHIP_ERR_ARG, "NotImplemented: unknown file format");
                int rc = sdfhip_sdfgen(device, vertices.data, vertices.count, Model::MaxDepth, &nod, nullptr);
                sdfhip_points_free(&vertices);
                Check(rc);
                std::string saveto = path.substr(0, path.find_last_of('.')) + ".asdf";   // Path.ChangeExtension
                Check(sdfhip_asdf_save(&nod, saveto.c_str()));
            }
            OctData d = FromNative(nod);
            sdfhip_octdata_free(&nod);                                                  // NativeOctData.Free
            return d;
        }
    };

    void Save(const std::string &path) const
    {
        sdfhip_octdata raw{ (uint32_t)Length(), (int32_t *)Structs.data(), (uint8_t *)Values.data() };
        Check(sdfhip_asdf_save(&raw, path.c_str()));
    }

private:
    static OctData FromNative(const sdfhip_octdata &raw)            // ManagedStructs / ManagedValues
    {
        OctData d;
        d.Structs.resize(raw.length);
        d.Values.resize((size_t)raw.length * 8);
        memcpy(d.Structs.data(), raw.structs, (size_t)raw.length * 8);
        memcpy(d.Values.data(), raw.values, (size_t)raw.length * 8);
        return d;
    }
};

class Logic {                        // Logic.cs:15-355, the camera/model part
public:
    static constexpr int xSize = 720, ySize = 720;                   // Logic.cs:17-18
    Info State;

    Logic() { sdfhip_info_default(&State, (float)xSize, (float)ySize); }
    // Logic.Heading (X = pitch, Y = yaw), Logic.cs:46-55
    void SetHeading(float x, float y) { headingX = x; headingY = y; sdfhip_info_set_heading(&State, x, y); }
    float HeadingX() const { return headingX; }
    float HeadingY() const { return headingY; }
    // Logic.Position, Logic.cs:60-78 (also refreshes State.limit)
    void SetPosition(float x, float y, float z) { sdfhip_info_set_position(&State, x, y, z); }
    void Resize(int width, int height) { State.screen_size[0] = (float)width; State.screen_size[1] = (float)height; }
    // the camera part of Logic.Update (Logic.cs:239-272): keys is a mask of SDFHIP_KEY_*
    void Update(float seconds, uint32_t keys)
    {
        float h[2] = { headingX, headingY };
        sdfhip_camera_update(&State, h, mSpeed, keys, seconds);
        headingX = h[0]; headingY = h[1];
    }
    void MouseMove(float dx, float dy)                                // Logic.cs:290-293
    {
        float h[2] = { headingX, headingY };
        sdfhip_camera_mouse_move(&State, h, dx, dy);
        headingX = h[0]; headingY = h[1];
    }
    void MouseWheel(float delta) { mSpeed = sdfhip_camera_mouse_wheel(mSpeed, delta); }   // Logic.cs:202-205
    float mSpeed = 0.5f;                                              // Logic.cs:28

    static FileFormat FormatOf(const std::string &filename)          // Logic.cs:126-138
    {
        auto ends = [&](const char *e) { size_t n = strlen(e); return filename.size() >= n && filename.compare(filename.size() - n, n, e) == 0; };
        if (ends(".asdf")) return FileFormat::ASDF;
        if (ends(".ply")) return FileFormat::Stanford;
        if (ends(".obj")) return FileFormat::Wavefront;
        return FileFormat::Invalid;
    }
    static std::string AutocompleteFile(const std::string &filename)  // Logic.cs:139-151 ("" for null)
    {
        auto exists = [](const std::string &p) { return std::ifstream(p).good(); };
        for (const char *ext : { "", ".asdf", ".ply", ".obj" })
            if (exists(filename + ext)) return filename + ext;
        return std::string();
    }
    // Logic.MakeData, Logic.cs:87-105
    OctData MakeData(const std::string &name, int device = 0)
    {
        std::string filename = AutocompleteFile(name);
        if (filename.empty()) throw Error(SDFHIP_ERR_IO, "MakeData: no such model: " + name);
        OctData data = OctData::NativeOctData::Generate(filename, FormatOf(filename), device);
        State.buffer_size = (uint32_t)data.Length();
        return data;
    }

private:
    float headingX = 0, headingY = 0;
};

class Program {                      // Program.cs: the compute pass of Draw, and model (re)load
public:
    explicit Program(int device = 0) : device(device) {}
    ~Program() { if (scene) sdfhip_scene_free(scene); }
    Program(const Program &) = delete;
    Program &operator=(const Program &) = delete;

    // CreateResources' scene bindings / the reload swap of Program.cs:59-65: upload the new
    // model, then drop the old one
    void Load(const OctData &model)
    {
        sdfhip_scene *fresh = nullptr;
        Check(sdfhip_scene_upload(device, &model.Structs[0].Parent, model.Values.data(), (uint32_t)model.Length(), &fresh));
        Adopt(fresh);
    }
    // ... with the upload's choices taken by the host (sdfhip_upload_options: start from sdfhip_upload_options_default, -1 = choose):
    // e.g. top_grid_level = 0 for no lookup grid at all on a device short of memory
    void Load(const OctData &model, const sdfhip_upload_options &options)
    {
        sdfhip_scene *fresh = nullptr;
        Check(sdfhip_scene_upload_ex(device, &model.Structs[0].Parent, model.Values.data(), (uint32_t)model.Length(), &options, &fresh));
        Adopt(fresh);
    }
    // Space carving (sdfhip_scene_edit; the reference's README lists modeling under "Plans"): the brushes, in order, carve from or
    // add to the loaded model on its device, and the edited model replaces it as a reload does -- the old handle is freed once the
    // new one exists.  max_depth: -1 = the model's depth, else 0..12.  host_out (may be null): the edited tree's host arrays
    // (release with sdfhip_octdata_free), e.g. for sdfhip_asdf_save
    void Edit(const std::vector<sdfhip_edit> &edits, int max_depth = -1, sdfhip_edit_stats *stats = nullptr, sdfhip_octdata *host_out = nullptr)
    {
        if (!scene) throw Error(SDFHIP_ERR_ARG, "Edit: no model loaded");
        sdfhip_scene *fresh = nullptr;
        Check(sdfhip_scene_edit(scene, edits.data(), (uint32_t)edits.size(), max_depth, &fresh, host_out, stats));
        Adopt(fresh);
    }
    // Pruning (sdfhip_scene_prune): the blocks of eight that say nothing their parent does not already say -- within `tolerance` bytes
    // (0..255) of what the parent's bytes interpolate to, or below max_depth (-1 = no cut, else 0..12) -- are removed, and the
    // pruned model replaces the loaded one as Edit's result does.  host_out (may be null): the pruned tree's host arrays
    void Prune(int tolerance = 0, int max_depth = -1, sdfhip_prune_stats *stats = nullptr, sdfhip_octdata *host_out = nullptr)
    {
        if (!scene) throw Error(SDFHIP_ERR_ARG, "Prune: no model loaded");
        const sdfhip_prune_options opt = { (uint32_t)sizeof(sdfhip_prune_options), tolerance, max_depth };
        sdfhip_scene *fresh = nullptr;
        Check(sdfhip_scene_prune(scene, &opt, &fresh, host_out, stats));
        Adopt(fresh);
    }
    // Combination (sdfhip_scene_combine): the loaded model becomes its union (SDFHIP_COMBINE_UNION), intersection (_INTERSECT) or
    // difference (_SUBTRACT: this model without the other) with the model `other` has loaded on the same device (it may be this
    // Program); both live in the same unit cube (Place one first to move it), nothing is blended or pruned (chain Prune(0)).  The result replaces the
    // loaded model as Prune's does; `other` keeps its own.  max_depth: -1 = no cut, else 0..12.  host_out (may be null): the result's
    // host arrays
    void Combine(const Program &other, int op, int max_depth = -1, sdfhip_combine_stats *stats = nullptr, sdfhip_octdata *host_out = nullptr)
    {
        if (!scene || !other.scene) throw Error(SDFHIP_ERR_ARG, "Combine: no model loaded");
        const sdfhip_combine_options opt = { (uint32_t)sizeof(sdfhip_combine_options), max_depth };
        sdfhip_scene *fresh = nullptr;
        Check(sdfhip_scene_combine(scene, other.scene, op, &opt, &fresh, host_out, stats));
        Adopt(fresh);
    }
    // Placement (sdfhip_scene_place): the loaded model is rotated, scaled and moved -- a point x of it lands at scale * R x + t, R
    // row-major and orthogonal (a mirror is allowed), scale > 0 -- by resampling it into a new tree of at most `depth` levels (-1 = the
    // model's own depth, else 0..12), which replaces the loaded model as Prune's result does.  Nothing is pruned (chain Prune), and the
    // identity is a resampling, not a clone.  Place two Programs, then Combine them.  host_out (may be null): the result's host arrays
    void Place(const float (&rotation)[3][3], float scale, const float (&translation)[3], int depth = -1, sdfhip_place_stats *stats = nullptr,
               sdfhip_octdata *host_out = nullptr)
    {
        if (!scene) throw Error(SDFHIP_ERR_ARG, "Place: no model loaded");
        sdfhip_placement pl = {};
        pl.size = (uint32_t)sizeof(sdfhip_placement);
        for (int i = 0; i < 3; i++) {
            for (int j = 0; j < 3; j++) pl.rotation[i][j] = rotation[i][j];
            pl.translation[i] = translation[i];
        }
        pl.scale = scale;
        pl.depth = depth;
        sdfhip_scene *fresh = nullptr;
        Check(sdfhip_scene_place(scene, &pl, &fresh, host_out, stats));
        Adopt(fresh);
    }
    // Composition (sdfhip_scene_compose): the model becomes ONE tree made of many placed instances of the models that Programs on
    // this device have loaded (this one may be among them, and the same Program may appear in many parts), in a single pass: part
    // k's own field under its own placement -- a point x of it lands at scale * R x + t, as Place's -- folded in float in list order
    // (SDFHIP_COMBINE_UNION min, _INTERSECT max, _SUBTRACT max with the negated value; the first part is a union) and rounded to a
    // byte once.  One part is Place byte for byte; the result is not Combine of Places (one quantisation, not two).  depth: -1 = the
    // largest depth among the parts' models, else 0..12.  The result replaces the loaded model as Place's does; the other Programs
    // keep theirs.  Nothing is pruned (chain Prune).  host_out (may be null): the result's host arrays
    struct Part {
        const Program *program;
        float rotation[3][3];
        float scale;
        float translation[3];
        int op = SDFHIP_COMBINE_UNION;
    };
    void Compose(const std::vector<Part> &parts, int depth = -1, sdfhip_compose_stats *stats = nullptr, sdfhip_octdata *host_out = nullptr)
    {
        const std::vector<sdfhip_instance> list = InstanceList(parts, "Compose");
        const sdfhip_compose_options opt = { (uint32_t)sizeof(sdfhip_compose_options), depth };
        sdfhip_scene *fresh = nullptr;
        Check(sdfhip_scene_compose(list.data(), (uint32_t)list.size(), &opt, &fresh, host_out, stats));
        Adopt(fresh);
    }
    // The parts as the C list (Compose, DrawParts, PickParts, SampleParts)
    static std::vector<sdfhip_instance> InstanceList(const std::vector<Part> &parts, const char *what)
    {
        std::vector<sdfhip_instance> list(parts.size());
        for (size_t k = 0; k < parts.size(); k++) {
            if (!parts[k].program || !parts[k].program->scene) throw Error(SDFHIP_ERR_ARG, std::string(what) + ": a part has no model loaded");
            sdfhip_instance &in = list[k];
            in.scene = parts[k].program->scene;
            in.op = parts[k].op;
            for (int i = 0; i < 3; i++) {
                for (int j = 0; j < 3; j++) in.rotation[i][j] = parts[k].rotation[i][j];
                in.translation[i] = parts[k].translation[i];
            }
            in.scale = parts[k].scale;
        }
        return list;
    }
    // An assembly drawn, probed and picked without baking (sdfhip_instances_render / _pick / _sample; nothing in the reference
    // corresponds): the parts Compose takes, consumed as they are -- Compose's fold evaluated at every marched point, no tree built,
    // no Program's model replaced -- so a part can move from one frame to the next at no cost, and every answer names the part it
    // came from (sdfhip_part_hit.instance, sdfhip_part_probe.instance: the index in `parts`).  DrawParts: a width x height RGBA32F
    // frame, row 0 at the top; PickParts: the part under pixels {x, y} of the camera `state`; SampleParts: value, part and gradient
    // at points (xyz: 3 floats per point).  opt (may be null): max_steps, normal_step, SDFHIP_INSTANCES_NO_SKIP
    static std::vector<float> DrawParts(const std::vector<Part> &parts, const Info &state, uint32_t width, uint32_t height,
                                        const sdfhip_instances_options *opt = nullptr)
    {
        const std::vector<sdfhip_instance> list = InstanceList(parts, "DrawParts");
        std::vector<float> rgba((size_t)width * height * 4);
        Check(sdfhip_instances_render(list.data(), (uint32_t)list.size(), opt, &state, width, height, rgba.data()));
        return rgba;
    }
    static std::vector<sdfhip_part_hit> PickParts(const std::vector<Part> &parts, const Info &state, const std::vector<uint32_t> &pixels_xy,
                                                  const sdfhip_instances_options *opt = nullptr)
    {
        const std::vector<sdfhip_instance> list = InstanceList(parts, "PickParts");
        std::vector<sdfhip_part_hit> out(pixels_xy.size() / 2);
        Check(sdfhip_instances_pick(list.data(), (uint32_t)list.size(), opt, &state, pixels_xy.data(), (uint32_t)out.size(), out.data()));
        return out;
    }
    static std::vector<sdfhip_part_probe> SampleParts(const std::vector<Part> &parts, const std::vector<float> &xyz,
                                                      const sdfhip_instances_options *opt = nullptr)
    {
        const std::vector<sdfhip_instance> list = InstanceList(parts, "SampleParts");
        std::vector<sdfhip_part_probe> out(xyz.size() / 3);
        Check(sdfhip_instances_sample(list.data(), (uint32_t)list.size(), opt, xyz.data(), (uint32_t)out.size(), out.data()));
        return out;
    }
    // The clash check (sdfhip_instances_clash; nothing in the reference corresponds): which pairs of the parts share points of the
    // lattice of 8^depth cell centres of the cube (opt: depth, origin, side, SDFHIP_CLASH_NO_SKIP; null = depth 6 on the unit cube),
    // at most SDFHIP_CLASH_MAX_INSTANCES parts, the ops ignored.  One record per overlapping pair a < b, in (a, b) order: points,
    // first, lo / hi, sum -- integers, the same bytes on every call.  stats (may be null).  No Program's model is touched
    static std::vector<sdfhip_clash> ClashParts(const std::vector<Part> &parts, const sdfhip_clash_options *opt = nullptr,
                                                sdfhip_clash_stats *stats = nullptr)
    {
        const std::vector<sdfhip_instance> list = InstanceList(parts, "ClashParts");
        std::vector<sdfhip_clash> out(list.size() * (list.size() ? list.size() - 1 : 0) / 2);
        uint32_t n = 0;
        Check(sdfhip_instances_clash(list.data(), (uint32_t)list.size(), opt, out.empty() ? nullptr : out.data(), (uint32_t)out.size(), &n, stats));
        out.resize(n);
        return out;
    }
    // The penetration depth (sdfhip_instances_penetration; nothing in the reference corresponds): how far each overlapping pair of
    // the parts reaches into the other, on ClashParts' lattice (opt: depth, origin, side, SDFHIP_PENETRATION_NO_SKIP; null = depth 6
    // on the unit cube) and ClashParts' list.  One record per overlapping pair a < b, in (a, b) order: points, the witness, depth,
    // ra / rb, the nearest cells and the nearest surface points of both parts -- the same bytes on every call.  stats (may be null).
    // The workflow: ClashParts at a coarse depth, the cube round a record's lo..hi, this call on that cube.  No model is touched
    static std::vector<sdfhip_penetration> PenetrationParts(const std::vector<Part> &parts, const sdfhip_penetration_options *opt = nullptr,
                                                            sdfhip_penetration_stats *stats = nullptr)
    {
        const std::vector<sdfhip_instance> list = InstanceList(parts, "PenetrationParts");
        std::vector<sdfhip_penetration> out(list.size() * (list.size() ? list.size() - 1 : 0) / 2);
        uint32_t n = 0;
        Check(sdfhip_instances_penetration(list.data(), (uint32_t)list.size(), opt, out.empty() ? nullptr : out.data(), (uint32_t)out.size(), &n,
                                           stats));
        out.resize(n);
        return out;
    }
    // The clearance (sdfhip_instances_gap; nothing in the reference corresponds): how far apart the surfaces of each pair of the parts
    // lie and where they are nearest, on ClashParts' list (opt: limit, SDFHIP_GAP_NO_PRUNE; null = limit +inf).  One record per pair
    // a < b whose gap is <= limit, in (a, b) order: gap, flags, the cut cells and the two closest points in world coordinates
    // (point_b - point_a is the way across the gap) -- the same records on every call.  The vertex-to-surface distance both ways round:
    // never below the distance between the two meshes, above it by less than half an edge of the finer one.  stats (may be null).
    // No model is touched
    static std::vector<sdfhip_gap> GapParts(const std::vector<Part> &parts, const sdfhip_gap_options *opt = nullptr, sdfhip_gap_stats *stats = nullptr)
    {
        const std::vector<sdfhip_instance> list = InstanceList(parts, "GapParts");
        std::vector<sdfhip_gap> out(list.size() * (list.size() ? list.size() - 1 : 0) / 2);
        uint32_t n = 0;
        Check(sdfhip_instances_gap(list.data(), (uint32_t)list.size(), opt, out.empty() ? nullptr : out.data(), (uint32_t)out.size(), &n, stats));
        out.resize(n);
        return out;
    }
    // The components of the loaded model (sdfhip_scene_components; nothing in the reference corresponds): its face-connected solids
    // and voids on the lattice of 8^depth cell centres of the cube (opt: depth 0..9, origin, side; null = depth 6 on the unit cube).
    // One record per component in ascending label order -- label = its lowest linear index, flags = SDFHIP_COMPONENT_SOLID or 0 for a
    // void, points, lo / hi, sum: integers, the same bytes on every call.  labels (may be null): resized to 8^depth, every point's
    // label in linear-index order.  stats (may be null).  The model is untouched
    std::vector<sdfhip_component> Components(const sdfhip_components_options *opt = nullptr, std::vector<uint32_t> *labels = nullptr,
                                             sdfhip_components_stats *stats = nullptr) const
    {
        if (!scene) throw Error(SDFHIP_ERR_ARG, "Components: no model loaded");
        if (labels) labels->resize((size_t)1 << (3 * (opt && opt->depth <= SDFHIP_COMPONENTS_MAX_DEPTH ? opt->depth : 6u)));
        std::vector<sdfhip_component> out(64);
        for (;;) {
            uint32_t n = 0;
            Check(sdfhip_scene_components(scene, opt, out.data(), (uint32_t)out.size(), &n, labels ? labels->data() : nullptr, stats));
            const bool all = n <= out.size();
            out.resize(n);
            if (all) return out;
        }
    }
    // Selection (sdfhip_scene_select; nothing in the reference corresponds): the loaded model with some of its components' phases
    // flipped -- a solid becomes empty space, a void becomes solid -- resampled into a new tree, which replaces the loaded model as
    // Place's result does.  opt (null = the defaults: no rule, which is Place at the identity): the rule bits SDFHIP_SELECT_*, OR-ed,
    // the components' lattice (lattice_depth 0..9, origin, side), the result's depth (-1 = the model's own) and min_points.  labels: the
    // list of SDFHIP_SELECT_FLIP_LISTED or _KEEP_LISTED, labels as Components returns them on the same lattice, any order.  The removed
    // pieces' former surfaces stay as structure; nothing is pruned.  host_out (may be null): the result's host arrays
    void Select(const sdfhip_select_options *opt = nullptr, const std::vector<uint32_t> &labels = {}, sdfhip_select_stats *stats = nullptr,
                sdfhip_octdata *host_out = nullptr)
    {
        if (!scene) throw Error(SDFHIP_ERR_ARG, "Select: no model loaded");
        sdfhip_scene *fresh = nullptr;
        Check(sdfhip_scene_select(scene, opt, labels.empty() ? nullptr : labels.data(), (uint32_t)labels.size(), &fresh, host_out, stats));
        Adopt(fresh);
    }
    // Volumes in and out (sdfhip_volume_build / sdfhip_scene_volume; nothing in the reference corresponds).  LoadVolume: the model
    // becomes the tree of at most `depth` levels (0..12) of a dense lattice of distances -- n = {nx, ny, nz} floats, sample (i, j, k) at
    // index (k * ny + j) * nx + i and at origin + (i, j, k) * spacing in the unit cube's coordinates, stored value * value_scale =
    // distance -- the trilinear interpolant, continued outside the lattice's box at slope 1; it replaces the loaded model as a Load
    // does.  A non-finite sample is refused; nothing is pruned (chain Prune).  Volume: the loaded model's distances on such a lattice
    // (n_a >= 1), x fastest.  host_out (may be null): the result's host arrays
    void LoadVolume(const std::vector<float> &grid, const uint32_t (&n)[3], const float (&origin)[3], float spacing, int depth,
                    float value_scale = 1.0f, sdfhip_volume_stats *stats = nullptr, sdfhip_octdata *host_out = nullptr)
    {
        if ((uint64_t)n[0] * n[1] * n[2] != grid.size()) throw Error(SDFHIP_ERR_ARG, "LoadVolume: the grid's size is not nx * ny * nz");
        const sdfhip_volume vol = Lattice(n, origin, spacing, value_scale, depth);
        sdfhip_scene *fresh = nullptr;
        Check(sdfhip_volume_build(device, grid.data(), &vol, &fresh, host_out, stats));
        Adopt(fresh);
    }
    std::vector<float> Volume(const uint32_t (&n)[3], const float (&origin)[3], float spacing)
    {
        if (!scene) throw Error(SDFHIP_ERR_ARG, "Volume: no model loaded");
        const sdfhip_volume lattice = Lattice(n, origin, spacing, 0.0f, 0);
        std::vector<float> out((size_t)n[0] * n[1] * n[2]);
        Check(sdfhip_scene_volume(scene, &lattice, out.data()));
        return out;
    }
    // Exact distance (sdfhip_scene_distance / sdfhip_scene_offset; nothing in the reference corresponds).  Distance: how far points
    // (xyz: 3 floats per point) are from the loaded model's surface -- the triangles of its mesh at `level` -- at any range, where
    // Sample's distance saturates a leaf edge away; a bad element gets SDFHIP_QUERY_INVALID, not an exception.  Offset: the model grown
    // by delta (shrunk when it is negative); Shell: the wall of `thickness` > 0 centred on its surface -- each a new tree of at most
    // `depth` levels (-1 = the model's own depth, else 0..12), which replaces the loaded model as Place's result does.  Nothing is
    // pruned (chain Prune).  host_out (may be null): the result's host arrays
    std::vector<sdfhip_clearance> Distance(const std::vector<float> &xyz, int level = -1)
    {
        if (!scene) throw Error(SDFHIP_ERR_ARG, "Distance: no model loaded");
        std::vector<sdfhip_clearance> out(xyz.size() / 3);
        Check(sdfhip_scene_distance(scene, xyz.data(), (uint32_t)out.size(), level, out.data()));
        return out;
    }
    void Offset(float delta, int depth = -1, int level = -1, sdfhip_offset_stats *stats = nullptr, sdfhip_octdata *host_out = nullptr)
    {
        OffsetAs(SDFHIP_OFFSET_GROW, delta, depth, level, stats, host_out, "Offset: no model loaded");
    }
    void Shell(float thickness, int depth = -1, int level = -1, sdfhip_offset_stats *stats = nullptr, sdfhip_octdata *host_out = nullptr)
    {
        OffsetAs(SDFHIP_OFFSET_SHELL, thickness, depth, level, stats, host_out, "Shell: no model loaded");
    }
    // Smooth blends and morphs (sdfhip_scene_blend; nothing in the reference corresponds).  Blend: the loaded model becomes its smooth
    // union (SDFHIP_BLEND_UNION), intersection (_INTERSECT) or difference (_SUBTRACT: this model without the other) with the model
    // `other` has loaded on the same device (it may be this Program), on the two exact distances: a fillet of `radius` >= 0 where the
    // surfaces meet, the hard operation at 0.  Morph: the in-between a + (b - a) * t, 0 <= t <= 1; refused when either surface is
    // empty.  Each a new tree of at most `depth` levels (-1 = the deeper of the two models' depths, else 0..12), which replaces the
    // loaded model as Combine's result does; `other` keeps its own.  level, other_level: each surface's level.  Nothing is pruned
    // (chain Prune).  host_out (may be null): the result's host arrays
    void Blend(const Program &other, int op, float radius, int depth = -1, int level = -1, int other_level = -1, sdfhip_blend_stats *stats = nullptr,
               sdfhip_octdata *host_out = nullptr)
    {
        if (!scene || !other.scene) throw Error(SDFHIP_ERR_ARG, "Blend: no model loaded");
        sdfhip_blend_options opt = {};
        opt.size = (uint32_t)sizeof(sdfhip_blend_options);
        opt.op = op;
        opt.amount = radius;
        opt.depth = depth;
        opt.level_a = level;
        opt.level_b = other_level;
        sdfhip_scene *fresh = nullptr;
        Check(sdfhip_scene_blend(scene, other.scene, &opt, &fresh, host_out, stats));
        Adopt(fresh);
    }
    void Morph(const Program &other, float t, int depth = -1, int level = -1, int other_level = -1, sdfhip_blend_stats *stats = nullptr,
               sdfhip_octdata *host_out = nullptr)
    {
        Blend(other, SDFHIP_BLEND_MORPH, t, depth, level, other_level, stats, host_out);
    }
    // Point and ray queries (sdfhip_scene_sample / _raycast / _pick; nothing in the reference corresponds): what the loaded model
    // answers without drawing a frame, with the shader's own arithmetic.  Sample: distance, cell and gradient at points (xyz: 3 floats
    // per point); Raycast: the primary march of Compute.hlsl:194-203 for arbitrary rays; Pick: that march for pixels {x, y} of the
    // camera `state` -- Pick one pixel, put a brush at hit.position, Edit.  A bad element gets SDFHIP_QUERY_INVALID, not an exception.
    std::vector<sdfhip_probe> Sample(const std::vector<float> &xyz)
    {
        if (!scene) throw Error(SDFHIP_ERR_ARG, "Sample: no model loaded");
        std::vector<sdfhip_probe> out(xyz.size() / 3);
        Check(sdfhip_scene_sample(scene, xyz.data(), (uint32_t)out.size(), out.data()));
        return out;
    }
    std::vector<sdfhip_hit> Raycast(const std::vector<sdfhip_ray> &rays, float margin, float limit, uint32_t max_steps = 100)
    {
        if (!scene) throw Error(SDFHIP_ERR_ARG, "Raycast: no model loaded");
        std::vector<sdfhip_hit> out(rays.size());
        Check(sdfhip_scene_raycast(scene, rays.data(), (uint32_t)rays.size(), margin, limit, max_steps, out.data()));
        return out;
    }
    std::vector<sdfhip_hit> Pick(const Info &state, const std::vector<uint32_t> &pixels_xy, uint32_t max_steps = 100)
    {
        if (!scene) throw Error(SDFHIP_ERR_ARG, "Pick: no model loaded");
        std::vector<sdfhip_hit> out(pixels_xy.size() / 2);
        Check(sdfhip_scene_pick(scene, &state, pixels_xy.data(), (uint32_t)out.size(), max_steps, out.data()));
        return out;
    }
    // Surface extraction (sdfhip_scene_mesh; nothing in the reference corresponds -- its tree only ever becomes pixels): the loaded
    // model as a triangle soup, 3 vertices of six floats {position, normal} per triangle in a pinned order -- the layout of a point
    // cloud, so the result feeds sdfhip_sdfgen[_scene] as it is.  level: -1 = the leaves, 0..12 = the level-of-detail mesh of that
    // level.  Save it with sdfhip_mesh_save_ply / _obj on an sdfhip_mesh{n, data}
    std::vector<float> Mesh(int level = -1, sdfhip_mesh_stats *stats = nullptr)
    {
        if (!scene) throw Error(SDFHIP_ERR_ARG, "Mesh: no model loaded");
        sdfhip_mesh_options opt;
        sdfhip_mesh_options_default(&opt);
        opt.level = level;
        sdfhip_mesh mesh = { 0, nullptr };
        Check(sdfhip_scene_mesh(scene, &opt, &mesh, stats));
        struct Release { sdfhip_mesh &m; ~Release() { sdfhip_mesh_free(&m); } } release{ mesh };
        return mesh.n_triangles ? std::vector<float>(mesh.verts6, mesh.verts6 + (size_t)mesh.n_triangles * 18) : std::vector<float>();
    }
    // The measure (sdfhip_scene_measure; nothing in the reference corresponds -- no call there says anything quantitative about its
    // tree): volume, area, first and second moments about the origin, tight bounds and cell counts of the solid the loaded model
    // describes -- the one Mesh() bounds -- in double precision.  centroid = moment1 / volume.  level: as Mesh()
    sdfhip_measure Measure(int level = -1)
    {
        if (!scene) throw Error(SDFHIP_ERR_ARG, "Measure: no model loaded");
        sdfhip_measure_options opt;
        sdfhip_measure_options_default(&opt);
        opt.level = level;
        sdfhip_measure out;
        Check(sdfhip_scene_measure(scene, &opt, &out));
        return out;
    }
    // Cross-sections (sdfhip_scene_slice; nothing that runs in the reference corresponds -- its Layers.hlsl, a z-slice viewer, is dead
    // code): the contours of the loaded model in the planes dot(normal, p) = offset + k * pitch, k = 0 .. layers - 1, as directed
    // segments with the solid on the left seen from the tip of the normal, in the pinned node-major order (each record carries its
    // layer; std::stable_sort on it groups them).  layer_counts, when given, receives the records per layer.  level: as Mesh()
    std::vector<sdfhip_segment> Slice(const float (&normal)[3], float offset = 0.5f, float pitch = 0.0f, uint32_t layers = 1, int level = -1,
                                      std::vector<uint32_t> *layer_counts = nullptr, sdfhip_slice_stats *stats = nullptr)
    {
        if (!scene) throw Error(SDFHIP_ERR_ARG, "Slice: no model loaded");
        sdfhip_slice_options opt;
        sdfhip_slice_options_default(&opt);
        opt.level = level;
        opt.normal[0] = normal[0]; opt.normal[1] = normal[1]; opt.normal[2] = normal[2];
        opt.offset = offset; opt.pitch = pitch; opt.layers = layers;
        sdfhip_slice slice = { 0, nullptr, 0, nullptr };
        Check(sdfhip_scene_slice(scene, &opt, &slice, stats));
        struct Release { sdfhip_slice &s; ~Release() { sdfhip_slice_free(&s); } } release{ slice };
        if (layer_counts) layer_counts->assign(slice.layer_counts, slice.layer_counts + slice.layers);
        return slice.n_segments ? std::vector<sdfhip_segment>(slice.segments, slice.segments + slice.n_segments) : std::vector<sdfhip_segment>();
    }
    // Triangle mesh -> model (sdfhip_trimesh_prepare + sdfhip_trimesh_build; nothing in the live reference corresponds -- the intent of its
    // abandoned GpuGenerator.cs): verts6 = 3 * n vertices of six floats as Mesh() returns them (normals ignored), counter-clockwise seen
    // from outside; the exact signed distance field becomes the loaded model, placed where the coordinates say (fit = false) or fitted
    // into the cube.  The tree never leaves HBM.
    void LoadTriangles(const std::vector<float> &verts6, int depth, bool fit = false, sdfhip_trimesh_stats *stats = nullptr)
    {
        sdfhip_trimesh_options opt;
        sdfhip_trimesh_options_default(&opt);
        opt.fit = fit ? 1 : 0;
        sdfhip_trimesh mesh = {};
        Check(sdfhip_trimesh_prepare(verts6.data(), (uint32_t)(verts6.size() / 18), 6, &opt, &mesh));
        struct Release { sdfhip_trimesh &m; ~Release() { sdfhip_trimesh_free(&m); } } release{ mesh };
        sdfhip_scene *fresh = nullptr;
        Check(sdfhip_trimesh_build(device, &mesh, depth, &fresh, nullptr, stats));
        Adopt(fresh);
    }
    // Draw's UpdateBuffer(info) + DispatchSized(W, H, 1), Program.cs:81,94 -> RGBA32F frame
    void Draw(const Info &state, int width, int height, std::vector<float> &frame, uint32_t flags = 0)
    {
        if (!scene) throw Error(SDFHIP_ERR_ARG, "Draw: no model loaded");
        frame.resize((size_t)width * height * 4);
        Check(sdfhip_render(scene, &state, (uint32_t)width, (uint32_t)height, flags, frame.data(), nullptr));
    }
    // Draw including the display pass (DisplayFrag.hlsl via Program.cs:96-99) -> RGBA8 frame
    void DrawDisplay(const Info &state, int width, int height, bool debugGizmos, std::vector<uint8_t> &frame, uint32_t flags = 0)
    {
        if (!scene) throw Error(SDFHIP_ERR_ARG, "Draw: no model loaded");
        frame.resize((size_t)width * height * 4);
        Check(sdfhip_render_display(scene, &state, (uint32_t)width, (uint32_t)height, flags, debugGizmos ? 1 : 0, frame.data(), nullptr));
    }

private:
    // the reload swap: the new model exists, so drop the loaded one (if any) and take it
    void Adopt(sdfhip_scene *fresh)
    {
        if (scene) sdfhip_scene_free(scene);
        scene = fresh;
    }
    static sdfhip_volume Lattice(const uint32_t (&n)[3], const float (&origin)[3], float spacing, float value_scale, int depth)
    {
        sdfhip_volume v = {};
        v.size = (uint32_t)sizeof(sdfhip_volume);
        for (int a = 0; a < 3; a++) { v.n[a] = n[a]; v.origin[a] = origin[a]; }
        v.spacing = spacing;
        v.value_scale = value_scale;
        v.dtype = SDFHIP_VOLUME_F32;
        v.depth = depth;
        return v;
    }
    void OffsetAs(int32_t mode, float amount, int depth, int level, sdfhip_offset_stats *stats, sdfhip_octdata *host_out, const char *unloaded)
    {
        if (!scene) throw Error(SDFHIP_ERR_ARG, unloaded);
        sdfhip_offset_options opt = {};
        opt.size = (uint32_t)sizeof(sdfhip_offset_options);
        opt.mode = mode;
        opt.amount = amount;
        opt.depth = depth;
        opt.level = level;
        sdfhip_scene *fresh = nullptr;
        Check(sdfhip_scene_offset(scene, &opt, &fresh, host_out, stats));
        Adopt(fresh);
    }

    int device;
    sdfhip_scene *scene = nullptr;
};

// The same two calls with the frame rendered by several GPUs of the node (sdfhip_multi_*: the scene on every device, the frame's
// bands dealt to them, sparse shares gathered into devices[0], assembled there): Program.Draw stays ONE call.
class ProgramMulti {
public:
    explicit ProgramMulti(std::vector<int> devices) : devices(std::move(devices)) {}
    ~ProgramMulti() { if (multi) sdfhip_multi_free(multi); }
    ProgramMulti(const ProgramMulti &) = delete;
    ProgramMulti &operator=(const ProgramMulti &) = delete;

    void Load(const OctData &model)
    {
        sdfhip_multi *fresh = nullptr;
        Check(sdfhip_multi_create(devices.data(), (uint32_t)devices.size(), &model.Structs[0].Parent, model.Values.data(), (uint32_t)model.Length(), &fresh));
        if (multi) sdfhip_multi_free(multi);
        multi = fresh;
    }
    void Draw(const Info &state, int width, int height, std::vector<float> &frame, uint32_t flags = 0)
    {
        if (!multi) throw Error(SDFHIP_ERR_ARG, "Draw: no model loaded");
        frame.resize((size_t)width * height * 4);
        Check(sdfhip_multi_render(multi, &state, (uint32_t)width, (uint32_t)height, flags, frame.data(), nullptr));
    }

private:
    std::vector<int> devices;
    sdfhip_multi *multi = nullptr;
};

}  // namespace SDFbox
