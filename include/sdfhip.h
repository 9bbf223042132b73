/*
 * sdfhip.h -- C ABI of libsdfhip.so: MI355X (gfx950) sphere tracing of
 * adaptively sampled distance fields behind SdfBox's frame boundary.
 *
 * Plain C, cdecl, PODs and pointers only; every function returns an int
 * status (SDFHIP_OK == 0) and never throws or aborts across the boundary;
 * sdfhip_last_error() returns the calling thread's last message.
 *
 * Each entry point names the reference interface it replaces (paths are
 * relative to the tau-dev/SdfBox checkout).  INTEGRATION.md shows the C#
 * [DllImport] stub a maintainer would add.
 *
 * Loading the library has ONE side effect on its host: unless GPU_MAX_HW_QUEUES is already in the environment (any value: the
 * host's word stands) or SDFHIP_KEEP_ENV is set, it exports GPU_MAX_HW_QUEUES=8 -- the HIP runtime reads that variable when the
 * process makes its first HIP call, and a host that keeps four frames in flight on four streams renders 20 % slower on the
 * runtime's default of four hardware queues (0.1014 against 0.0841 ms per 1080p frame: INTEGRATION.md section 3).  A process
 * that has initialised HIP before it loads the library keeps what it had.  (The export is a setenv() in the library's
 * constructor: like every setenv it is not ordered against a getenv() that another thread of the host makes at that very moment.
 * A host that loads the library while other threads of it run either exports the variable itself at start-up -- the export then
 * never happens -- or sets SDFHIP_KEEP_ENV.)
 */
#ifndef SDFHIP_H
#define SDFHIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SDFHIP_API __attribute__((visibility("default")))

/* ---- status codes ------------------------------------------------------ */
enum {
    SDFHIP_OK = 0,
    SDFHIP_ERR_ARG = 1,       /* null pointer, zero size, bad enum            */
    SDFHIP_ERR_IO = 2,        /* file missing / short / not an .asdf          */
    SDFHIP_ERR_BAD_TREE = 3,  /* parent/children index out of range           */
    SDFHIP_ERR_DEVICE = 4,    /* HIP call failed or no gfx950 device          */
    SDFHIP_ERR_NOMEM = 5
};

/* ---- data contract ----------------------------------------------------- */

/* The `Info` cbuffer, passed verbatim (112 bytes).
 * Replaces: struct Info, SdfBox/Logic.cs:407-420 == Compute.hlsl:70-81;
 * heading rows are Float3x3, SdfBox/Logic.cs:427-463.
 * buffer_size is ignored by the renderer (the scene handle knows its length);
 * hidef is unused by the shader and by us. */
typedef struct sdfhip_info {
    float heading[3][4];   /*   0 */
    float position[3];     /*  48 */
    float margin;          /*  60 */
    float screen_size[2];  /*  64 */
    uint32_t buffer_size;  /*  72 */
    float limit;           /*  76 */
    float light[3];        /*  80 */
    float strength;        /*  92 */
    float fov;             /*  96 */
    int32_t hidef;         /* 100 */
    uint32_t pad_[2];      /* 104 -> 112 */
} sdfhip_info;

/* Flattened octree as the reference's native loader hands it over.
 * Replaces: struct OctData {Length, Structs, Values}, SdfGen/dllmain.cpp:36-41
 * == NativeOctData, SdfBox/Program.cs:579-583.  structs = N x {int32 parent,
 * int32 children} (OctS, dllmain.cpp:18-29), values = N x 8 bytes, corner
 * k = x + 2y + 4z, *before* the texture swizzle of Program.cs:514-538. */
typedef struct sdfhip_octdata {
    uint32_t length;
    int32_t *structs;
    uint8_t *values;
} sdfhip_octdata;

/* Opaque scene handle: the octree resident in one GPU's HBM. */
typedef struct sdfhip_scene sdfhip_scene;

/* Render flags.  (A scene handle keeps scratch memory per stream that renders on it, 16 at a time; a 17th stream takes over the
 * least recently used scratch whose work has drained.)  Any other bit is refused with SDFHIP_ERR_ARG: the A/B knobs of the
 * measured-and-dropped kernel forms exist in the experiments build only (include/sdfhip_experimental.h, libsdfhip_lab.so). */
enum {
    SDFHIP_KERNEL_AUTO = 0,       /* the default: a grid lookup per find() wherever the tree allows, else the shader's own traversal */
    SDFHIP_KERNEL_GENERIC = 1,    /* one thread per pixel, follows parent / children links through memory as Compute.hlsl does */
    SDFHIP_KERNEL_STACK = 2,      /* integer cell coordinates and the lookup grids (needs a consistent tree of depth <= 12)   */
    SDFHIP_KERNEL_MASK = 0xF,
    SDFHIP_FLAG_COMPACT = 0x10,   /* BASELINE cfg-3's wavefront ray compaction: after the shading step a wave that holds fewer than 32
                                     shadow rays hands them to a queue (slots by ballot + prefix count) that a second kernel marches
                                     64 to a wave; fuller waves march theirs in place.  On a tree without a full-depth grid:
                                     persistent waves with ballot/prefix refill of finished lanes.  Bit-identical; 2-3 % slower than
                                     the default on the frames measured -- coherent primary rays leave little to compact */
    SDFHIP_FLAG_COUNT = 0x20,     /* also count algorithmic node/sample reads (slower)     */
    SDFHIP_FLAG_DISPLAY = 0x40,   /* fused display pass: output is RGBA8, gamma 1/2.2 (DisplayFrag.hlsl:24) */
    SDFHIP_FLAG_DISPLAY_DEBUG = 0x80, /* fused display pass, debug heat map w/140 (DisplayFrag.hlsl:21-22) */
    SDFHIP_FLAG_TILE_ORDER = 0x100000 /* for a viewer that renders one frame at a time: launch this frame's 8x8 tiles in
                                     descending order of the march iterations they (or a tile within two of them) took in the
                                     last frame rendered with the same geometry on the same stream; the order is made on the
                                     device behind every such frame whose camera block differs from the one the order in use
                                     came from (two small kernels, 13 us; a camera at rest pays once).  The first frame of a
                                     geometry, frames of a batch, frames of more than 65 536 tiles and frames rendered with
                                     SDFHIP_FLAG_COMPACT or in path-traced mode take the default order.
                                     A frame alone ends when its longest wave does, so the tiles that were expensive a moment
                                     ago go first: 0.174 -> 0.133 ms per 1080p frame with the camera at rest, 0.188 -> 0.148
                                     with one degree between frames.  Not for frames in flight on several streams (the ordering
                                     kernels sit between a stream's frames).  Never changes a pixel. */
};

/* Per-call statistics (all optional: pass NULL). */
typedef struct sdfhip_stats {
    float kernel_ms;        /* HIP-event time of the ray-march kernel(s)      */
    float total_ms;         /* kernel + device->host copy, host clock         */
    uint64_t n_nodes;       /* with SDFHIP_FLAG_COUNT: node records find()    */
                            /* reads in the reference algorithm   */
    uint64_t n_samples;     /* interpol_world calls                           */
    uint64_t n_steps;       /* sum of the alpha channel (march steps)         */
    uint32_t kernel_used;   /* SDFHIP_KERNEL_GENERIC or _STACK (| COMPACT)    */
    uint32_t pad_;
    uint64_t n_shadow_rays; /* with SDFHIP_FLAG_COUNT: pixels (path vertices) */
                            /* that cast a shadow ray, Compute.hlsl:213       */
    uint64_t n_loads;       /* with SDFHIP_FLAG_COUNT: 16-byte node records / */
                            /* grid cells the kernels themselves loaded (one  */
                            /* per lane and load): their own algorithmic reads */
    uint64_t n_hits;        /* with SDFHIP_FLAG_COUNT: entries that travelled     */
                            /* through a queue between two kernels -- the path-   */
                            /* traced pipeline's hits, summed over its levels (48 */
                            /* bytes each, written once and read once); shadow    */
                            /* rays queued by SDFHIP_FLAG_COMPACT; else 0         */
} sdfhip_stats;

/* ---- errors ------------------------------------------------------------ */
/* Replaces: CheckError -> throw across the FFI, SdfGen/pch.h:20-26. */
SDFHIP_API const char *sdfhip_last_error(void);

/* ---- scene data on the host (.asdf) ------------------------------------ */

/* Replaces: LoadAsdf, SdfGen/dllmain.cpp:250-276 (P/Invoke Program.cs:658).
 * Allocates out->structs / out->values; release with sdfhip_octdata_free. */
SDFHIP_API int sdfhip_asdf_load(const char *path, sdfhip_octdata *out);

/* Replaces: Save, SdfGen/dllmain.cpp:278-292 (P/Invoke Program.cs:661). */
SDFHIP_API int sdfhip_asdf_save(const sdfhip_octdata *data, const char *path);

/* Replaces: Free, SdfGen/dllmain.cpp:346-351 (P/Invoke Program.cs:666). */
SDFHIP_API void sdfhip_octdata_free(sdfhip_octdata *data);

/* Analytic scene builder: the split rule and quantiser of SdfGen's
 * construct / FromFloat / WriteBytes (SdfGen/dllmain.cpp:163-207) applied to
 * a closed-form distance function instead of a point cloud, same node order.
 * Stands in for SdfGen (dllmain.cpp:295-319), which needs mesh files that do
 * not ship.  shape: SDFHIP_SHAPE_*; params: see each shape. */
enum {
    SDFHIP_SHAPE_SPHERE = 0,   /* params: cx, cy, cz, r                        */
    SDFHIP_SHAPE_TORUS = 1,    /* params: cx, cy, cz, R, r  (axis = y)         */
    SDFHIP_SHAPE_GYROID = 2    /* params: cx, cy, cz, clip_r, freq, thickness  */
};
SDFHIP_API int sdfhip_generate(int shape, const float *params, int nparams,
                               int max_depth, int nthreads, sdfhip_octdata *out);

/* ---- point cloud -> ASDF --------------------------------------------- */

/* A point cloud with normals: count x {position xyz, normal xyz} floats.
 * Replaces: gsl::span<Vertex>* / struct Vertex, SdfGen/math.h:47-51. */
typedef struct sdfhip_points {
    uint32_t count;
    float *data;
} sdfhip_points;

/* Replaces: LoadPly, SdfGen/dllmain.cpp:244-248 -> ply_reader.cpp:35-71 (binary
 * little-endian, vertex element first, 6 floats per vertex). */
SDFHIP_API int sdfhip_load_ply(const char *path, sdfhip_points *out);
/* Replaces: LoadObj, SdfGen/dllmain.cpp:237-242 -> obj_reader.cpp:45-96. */
SDFHIP_API int sdfhip_load_obj(const char *path, sdfhip_points *out);
SDFHIP_API void sdfhip_points_free(sdfhip_points *points);

typedef struct sdfhip_sdfgen_stats {
    uint32_t nodes, levels;
    uint64_t candidate_entries;   /* sum of all candidate-list lengths: the work measure */
    float global_scale;           /* GlobalScale / GlobalOffset of dllmain.cpp:67-80 */
    float global_offset[3];
    float total_ms;
} sdfhip_sdfgen_stats;

/* Replaces: SdfGen(vertices, depth), SdfGen/dllmain.cpp:295-319 (P/Invoke Program.cs:
 * 662-663): builds the flattened octree of a point cloud on GPU `device`, level by
 * level, one wavefront per node -- the same nodes, order and bytes as the reference's
 * recursive construct (:163-207), including its lossy candidate pruning, corner
 * inheritance and first-point tie-breaking.  out: release with sdfhip_octdata_free.
 * SDFHIP_ERR_ARG when no point can be the nearest one (NaN input: the reference throws
 * "Did not find" / "NaN distance"). */
SDFHIP_API int sdfhip_sdfgen(int device, const float *verts6, uint32_t n, int32_t depth,
                             sdfhip_octdata *out, sdfhip_sdfgen_stats *stats);

/* Replaces: the viewer's generate -> upload flow, NativeOctData.Generate (SdfBox/Program.cs:613-650: LoadPly / LoadObj -> SdfGen) followed
 * by OctData.StructBuffer() / ValueTexture() and their binding (:543-572, :147-152): the point cloud goes in, a scene handle on `device`
 * comes out, and the tree never leaves HBM -- sdfhip_sdfgen's copy of the result to the host (12 ms for the 192 MB of a 12 M-node tree)
 * and sdfhip_scene_upload's copy back (8 ms) do not happen.  out (may be NULL): also the host arrays, e.g. for the .asdf cache the
 * reference writes next to the mesh (Program.cs:638-641).  The handle's renders are those of sdfhip_sdfgen + sdfhip_scene_upload. */
SDFHIP_API int sdfhip_sdfgen_scene(int device, const float *verts6, uint32_t n, int32_t depth, sdfhip_scene **scene,
                                   sdfhip_octdata *out, sdfhip_sdfgen_stats *stats);

/* The builder keeps the device memory of its work arrays (up to 24 GB per device: what a depth-10 tree of a million points takes) for
 * the next build of the process -- on this stack the first allocation after gigabytes have been freed takes a third of a second.
 * This gives it back (Replaces: nothing -- the reference builds on the host; cf. Free, SdfGen/dllmain.cpp:349-358).  A build that
 * runs out of device memory trims the pool itself and tries again.  SDFHIP_GEN_POOL=0 in the environment turns the pool off. */
SDFHIP_API int sdfhip_sdfgen_trim(void);

/* Structural check used by upload: 0 = ok; SDFHIP_ERR_BAD_TREE for an index out of
 * range, a cycle in the parent links or a parent chain of more than 64 links (either
 * would keep the shader's ascend loop from terminating).  depth_out = deepest level,
 * consistent_out = 1 when every child's parent field points back at it. */
SDFHIP_API int sdfhip_octdata_validate(const int32_t *structs, uint32_t n,
                                       uint32_t *depth_out, int *consistent_out);

/* ---- camera block ------------------------------------------------------ */

/* Replaces: Logic.State initialiser, SdfBox/Logic.cs:30-38 + Program.cs:54
 * (heading = identity via Logic.Heading = Zero) + limit via Logic.Position. */
SDFHIP_API void sdfhip_info_default(sdfhip_info *info, float width, float height);

/* Replaces: Logic.Heading setter, SdfBox/Logic.cs:46-55:
 * heading = Float3x3(Matrix4x4.CreateFromYawPitchRoll(heading_y, heading_x, 0)). */
SDFHIP_API void sdfhip_info_set_heading(sdfhip_info *info, float heading_x, float heading_y);

/* Replaces: Logic.Position setter, SdfBox/Logic.cs:60-78 (position + limit). */
SDFHIP_API void sdfhip_info_set_position(sdfhip_info *info, float x, float y, float z);

/* Movement keys of Logic.Update (SdfBox/Logic.cs:252-271), as a bit mask. */
enum {
    SDFHIP_KEY_RIGHT = 1, SDFHIP_KEY_LEFT = 2, SDFHIP_KEY_UP = 4, SDFHIP_KEY_DOWN = 8,   /* arrow keys: turn   */
    SDFHIP_KEY_FORWARD = 16,        /* W / numpad 8 */
    SDFHIP_KEY_BACK = 32,           /* S / numpad 2 */
    SDFHIP_KEY_STRAFE_RIGHT = 64,   /* D / numpad 6 */
    SDFHIP_KEY_STRAFE_LEFT = 128,   /* A / numpad 4 */
    SDFHIP_KEY_SHIFT = 256,         /* left shift / numpad 9: position.y -= step */
    SDFHIP_KEY_CONTROL = 512        /* left control / numpad 3: position.y += step */
};

/* Replaces: the camera part of Logic.Update, SdfBox/Logic.cs:239-272, for one time step of
 * `seconds`: the arrow keys turn the heading by tSpeed * seconds, the movement keys move the
 * position by mSpeed^2 * seconds in the yaw plane (yawMat, Logic.cs:79-83) or along y, in the
 * reference's order; heading_xy (in/out: X = pitch, Y = yaw) and `info` (heading, position,
 * limit) are updated.  m_speed: Logic.mSpeed, 0.5 at start (Logic.cs:28). */
SDFHIP_API void sdfhip_camera_update(sdfhip_info *info, float *heading_xy, float m_speed, uint32_t keys, float seconds);

/* Replaces: Logic.MouseMove, SdfBox/Logic.cs:290-293: heading += (-dy, dx) / 512 * 4. */
SDFHIP_API void sdfhip_camera_mouse_move(sdfhip_info *info, float *heading_xy, float dx, float dy);

/* Replaces: the MouseWheel handler, SdfBox/Logic.cs:202-205: the new mSpeed. */
SDFHIP_API float sdfhip_camera_mouse_wheel(float m_speed, float wheel_delta);

/* ---- device ------------------------------------------------------------ */

SDFHIP_API int sdfhip_device_count(int *count);
/* The PCI bus id of a device ("0000:c1:00.0"; out holds at least 16 bytes): what tells two ranks of a multi-GPU run apart. */
SDFHIP_API int sdfhip_device_pci_bus_id(int device, char *out, uint32_t len);
/* What this device's memory delivers to a streaming kernel, in GB/s (1e9 bytes): a float4 copy (reads + writes 2 x bytes),
 * STREAM's triad a = b + s c (3 x bytes) and a read-only sum (1 x bytes) over arrays of `bytes` each (>= 1 MiB; use >= 1 GiB:
 * the Infinity Cache holds 256 MiB), `reps` launches timed with HIP events.  Any result pointer may be null (no triad: one
 * array less; read only: one array).  SURVEY.md 8d's "measured device bandwidth on the box": the denominator bench.py quotes HBM
 * fractions against, beside the 8 TB/s nameplate.  Nothing in the reference corresponds to it (it displays FPS only,
 * SdfBox/Logic.cs:298-301). */
SDFHIP_API int sdfhip_device_bandwidth(int device, uint64_t bytes, uint32_t reps, double *copy_gbs, double *triad_gbs, double *read_gbs);

/* Replaces: OctData.StructBuffer() + OctData.ValueTexture(),
 * SdfBox/Program.cs:543-572, bound at Program.cs:147-152: copies the scene to
 * device `device` once.  Host arrays may be freed after return. */
SDFHIP_API int sdfhip_scene_upload(int device, const int32_t *structs, const uint8_t *values,
                                   uint32_t n, sdfhip_scene **out);
/* The same with the choices the upload otherwise makes by itself (sdfhip_scene_top_grid below describes them).  Every field:
 * -1 = choose.  A host uses this to bound the accelerators' memory or to take a particular grid; the pixels never depend on it. */
typedef struct sdfhip_upload_options {
    uint32_t size;            /* sizeof(sdfhip_upload_options), set by sdfhip_upload_options_default: lets the struct grow -- a smaller
                                 (older) struct is accepted from version 1's 20 bytes on, its missing fields mean "choose"; a larger
                                 (newer) one is accepted when the fields this library does not know are all -1 */
    int32_t top_grid_level;   /* 0 = no grid; 1..10 = a plain grid of that level, as deep as the tree at most -- the tree's depth asks
                                 for the dense full-depth grid, taken if it fits 1/64 of the device's memory (2.1 GB at depth 9) */
    int32_t top_grid_split;   /* 0 = never a split grid; 1..8 = a split grid with that coarse level (needs depth - level <= 6) */
    int32_t scatter_grid;     /* the path-traced mode's second grid: 0 = none, 1..4 = the levels of its blocks (8^n cells each) */
    int32_t scatter_order;    /* ... 0 = its blocks in x-y-z order (default: 2x2x2 sub-cubes, one cache line each) */
} sdfhip_upload_options;
SDFHIP_API void sdfhip_upload_options_default(sdfhip_upload_options *opt);
SDFHIP_API int sdfhip_scene_upload_ex(int device, const int32_t *structs, const uint8_t *values, uint32_t n,
                                      const sdfhip_upload_options *opt, sdfhip_scene **out);
SDFHIP_API int sdfhip_scene_free(sdfhip_scene *scene);
SDFHIP_API int sdfhip_scene_info(const sdfhip_scene *scene, uint32_t *n, uint32_t *depth,
                                 int *stack_kernel_ok, int *device);

/* The top grid the upload built for the cursor-stack kernels: for every cell of octree level
 * `level`, the record of the deepest node of that level or above that contains it, so that a
 * find() that restarts near the root takes one load instead of `level` dependent ones (results
 * and algorithmic counts are unchanged).  level = 0, bytes = 0: none (inconsistent or deeper than
 * 12 levels: generic kernel).  The level is the tree's depth for trees of depth <= 8 (16 bytes per cell,
 * 8^level cells, <= 268 MB) -- every leaf is then in the grid and a find is one load.
 * Deeper trees (up to 12 levels) get a split grid: a coarse dense level (reported as `level`; as deep as 8,
 * no larger than the tree's own records) whose internal cells point at dense blocks of the remaining <= 4
 * levels, built only where the tree is deep (`bytes` counts both; a find is one or two loads), if the blocks
 * fit 1/16 of the memory; else a plain grid of at most level 8, no larger than the tree's own records.
 * sdfhip_scene_upload_ex takes other choices (sdfhip_upload_options: a plain grid of a given level, none at all,
 * a split grid with a given coarse level).  The grid shrinks by itself when memory is short.  (The laboratory
 * library also reads them from the environment: SDFHIP_TOP_GRID_LEVEL, SDFHIP_TOP_GRID_SPLIT.) */
SDFHIP_API int sdfhip_scene_top_grid(const sdfhip_scene *scene, int32_t *level, uint64_t *bytes);

/* Replaces: Program.Draw's UpdateBuffer(info) + DispatchSized(W, H, 1),
 * SdfBox/Program.cs:81,94 (kernel: Compute.hlsl:180-231).  Renders the whole
 * W x H frame and copies it to `rgba_out` (host, W*H*4 floats, row-major,
 * top-left origin, tightly packed: no 12-pixel padding, unlike Program.cs:
 * 311-314).  Synchronous. */
SDFHIP_API int sdfhip_render(sdfhip_scene *scene, const sdfhip_info *info,
                             uint32_t width, uint32_t height, uint32_t flags,
                             float *rgba_out, sdfhip_stats *stats);

/* Device-resident variant for callers that keep the frame in HBM (multi-GPU
 * tile sharding, timing with inputs resident).  Renders the rows
 *     y = (band_first + (k / band_rows)*band_stride)*band_rows + k % band_rows,
 * k = 0 .. nrows_out-1, i.e. every band_stride-th band of band_rows rows
 * starting at band `band_first`, into d_rgba_out (device pointer, nrows_out x
 * width x 4 floats, compact).  band_stride = 1, band_first = 0, nrows_out =
 * height renders the whole frame.  Asynchronous on `stream` (a hipStream_t;
 * NULL = the HIP default stream, as for any HIP call); no host
 * synchronisation unless `stats` is given. */
SDFHIP_API int sdfhip_render_device(sdfhip_scene *scene, const sdfhip_info *info,
                                    uint32_t width, uint32_t height,
                                    uint32_t band_rows, uint32_t band_first,
                                    uint32_t band_stride, uint32_t nrows_out,
                                    uint32_t flags, float *d_rgba_out, void *stream,
                                    sdfhip_stats *stats);

/* Path-traced mode (BASELINE config 5: 16 spp diffuse path trace).  NOT in the
 * reference -- its README lists path tracing under "plans" only -- so there is no
 * interface to replace; the mode is defined by o_pixel_pt in oracle/sdf_oracle.c
 * (DESIGN.md section 8): per pixel `spp` jittered camera rays, each followed by up to
 * `max_bounces` cosine-weighted diffuse bounces, every segment marched, shaded and
 * shadow-tested with the reference's own rules (Compute.hlsl:194-230); RNG = PCG hash
 * of (seed + pixel, sample, bounce, draw).  Output RGBA32F: mean radiance, alpha =
 * march steps of all segments.  Same buffer conventions as sdfhip_render[_device]. */
typedef struct sdfhip_pathtrace {
    uint32_t spp;           /* samples per pixel, 1..4096 (config 5: 16)            */
    uint32_t max_bounces;   /* diffuse bounces after the camera ray (config 5: 3)   */
    uint32_t seed;          /* config 5: 0x5DFB0C5                                  */
    float albedo;           /* diffuse reflectance of the surface (0.8)             */
} sdfhip_pathtrace;
/* The bounce levels of the path-traced pipeline read a second split grid of the scene's cells, with larger blocks (+0.83 GB for
 * the depth-9 bench scene).  sdfhip_scene_prepare_path builds it at load time (allocations, kernels and two
 * stream synchronisations on the scene's own stream); without the call the first path-traced render builds it before its clock
 * starts.  Its blocks hold 16^3 cells by default (8^3 for trees of depth < 6) in the order of 2x2x2 sub-cubes, one cache line each;
 * sdfhip_upload_options.scatter_grid / scatter_order choose otherwise (0 = no second grid).  sdfhip_scene_top_grid counts its
 * bytes once it exists.  sdfhip_render_path returns SDFHIP_ERR_NOMEM, not a wrong image, if a hit ever found no room in its queue
 * (their capacity is the worst case of every sub-queue, so this is a check, not a limit). */
SDFHIP_API int sdfhip_scene_prepare_path(sdfhip_scene *scene);
SDFHIP_API int sdfhip_render_path(sdfhip_scene *scene, const sdfhip_info *info,
                                  const sdfhip_pathtrace *pt, uint32_t width, uint32_t height,
                                  uint32_t flags, float *rgba_out, sdfhip_stats *stats);
SDFHIP_API int sdfhip_render_path_device(sdfhip_scene *scene, const sdfhip_info *info,
                                         const sdfhip_pathtrace *pt, uint32_t width, uint32_t height,
                                         uint32_t band_rows, uint32_t band_first,
                                         uint32_t band_stride, uint32_t nrows_out, uint32_t flags,
                                         float *d_rgba_out, void *stream, sdfhip_stats *stats);

/* Replaces: the display pass, SdfBox/Shaders/DisplayFrag.hlsl:16-24 drawn by
 * Program.cs:96-99, fused into the ray-march epilogue: the frame comes back as
 * R8G8B8A8_UNorm bytes (W*H*4, row-major), `pow(val, 1/2.2)` per channel, or with
 * debug != 0 the step-count heat map `(1,1,1,0) * val.w / 140`.  4x fewer bytes to
 * store, gather and copy to the host.  (The same output is selected on the
 * sdfhip_render / sdfhip_render_device calls by SDFHIP_FLAG_DISPLAY[_DEBUG]; their
 * output pointer then addresses W*H uint32 pixels.) */
SDFHIP_API int sdfhip_render_display(sdfhip_scene *scene, const sdfhip_info *info,
                                     uint32_t width, uint32_t height, uint32_t flags, int debug,
                                     uint8_t *rgba8_out, sdfhip_stats *stats);

/* The host's frame array, page-locked: sdfhip_render / sdfhip_render_display into such memory run the frame in
 * row bands whose copies to the host go beside the march (into pageable memory every copy is staged inside the copy call,
 * with the host waiting in it), and below 4 M pixels the march kernel stores its pixels into the array itself -- no device
 * frame, no copy: 1080p 0.735 -> 0.676 ms per call, RGBA8 0.296 -> 0.260.  Replaces nothing in the reference
 * -- Program.cs:94-99 leaves the frame in a GPU texture -- it is what a host that wants the pixels does once, beside
 * its one frame array:
 *   sdfhip_host_alloc(bytes, &p)   page-locked memory of the library's (any device may copy into it);
 *   sdfhip_host_register(p, bytes) page-locks the caller's own array where it lies: it must not move or be freed while
 *                                  registered (C#: a GCHandleType.Pinned handle kept for as long);
 *   sdfhip_host_release(p)         frees / unregisters (p = the start of the range; NULL is a no-op).
 * A destination that is neither is rendered as before: nothing here is required. */
SDFHIP_API int sdfhip_host_alloc(uint64_t bytes, void **out);
SDFHIP_API int sdfhip_host_register(void *p, uint64_t bytes);
SDFHIP_API int sdfhip_host_release(void *p);

/* Several frames in one launch: infos[0..n_frames-1] (n_frames <= 8) are rendered into
 * d_rgba_out[f * nrows_out * width ...], each with its own camera block; same band
 * arguments as sdfhip_render_device.  For sharded rendering, where one rank's share of a
 * frame is little work behind the serial tail of its longest pixels: the frames of a
 * gather group share that tail.  Plain kernel only (no COMPACT / COUNT flags). */
SDFHIP_API int sdfhip_render_batch_device(sdfhip_scene *scene, const sdfhip_info *infos,
                                          uint32_t n_frames, uint32_t width, uint32_t height,
                                          uint32_t band_rows, uint32_t band_first,
                                          uint32_t band_stride, uint32_t nrows_out,
                                          uint32_t flags, float *d_rgba_out, void *stream,
                                          sdfhip_stats *stats);

/* Rank-0 helper for the tile gather of DENSE bands (the path-traced mode; scenes without a full-depth grid): scatter `world`
 * compact band buffers back into row order.  One gather may carry several frames (fewer, larger messages):
 * d_gathered is [world][frames][rows_per_rank][width] pixels, d_frame is [frames][height][width].
 * pixel_bytes = 16 (RGBA32F) or 4 (RGBA8): both sides hold such pixels.  Asynchronous on `stream`. */
SDFHIP_API int sdfhip_deinterleave_device(int device, const void *d_gathered, void *d_frame,
                                          uint32_t width, uint32_t height,
                                          uint32_t band_rows, uint32_t world,
                                          uint32_t rows_per_rank, uint32_t pixel_bytes,
                                          uint32_t frames, void *stream);

/* Layouts that give the ranks unequal shares of the frame (rank 0 also assembles the frame, so it
 * should render less): the bands a rank renders come as an explicit list instead of "every
 * band_stride-th".  Local band i of the compact output (rows i*band_rows .. of nrows_out) is band
 * bands[i] of the frame; n_bands <= 512.  n_frames consecutive Info blocks render in one launch as
 * in sdfhip_render_batch_device; pt != NULL selects the path-traced mode (one frame). */
SDFHIP_API int sdfhip_render_bands_device(sdfhip_scene *scene, const sdfhip_info *infos, uint32_t n_frames,
                                          const sdfhip_pathtrace *pt, uint32_t width, uint32_t height,
                                          uint32_t band_rows, const uint16_t *bands, uint32_t n_bands,
                                          uint32_t nrows_out, uint32_t flags, float *d_rgba_out, void *stream,
                                          sdfhip_stats *stats);

/* sdfhip_deinterleave_device for such a layout: owner[b] = the rank that rendered band b of the frame
 * (ceil(height / band_rows) entries, at most 512; world <= 64); a rank's bands sit in its buffer in
 * increasing band order. */
SDFHIP_API int sdfhip_deinterleave_bands_device(int device, const void *d_gathered, void *d_frame,
                                                uint32_t width, uint32_t height, uint32_t band_rows,
                                                uint32_t world, uint32_t rows_per_rank, const uint8_t *owner,
                                                uint32_t pixel_bytes, uint32_t frames, void *stream);

/* ---- sparse wire shares written by the march kernel itself ------------------------------------------------------------
 * A wave of the default kernel renders one 8x8 tile, which is the unit of the sparse wire format: at its end it holds the tile's
 * 64 wire pixels in registers and writes the tile's mask (one ballot), its code bytes (one 64-byte store) and its non-zero floats
 * (slots from one atomic add) straight into the share -- no dense wire buffer and no sdfhip_wire_compact_device behind the render.
 * One share holds all `frames` frames of a launch: 64-byte header (word 0 = float slots handed out; beyond `capacity` they are
 * dropped, and the count says so) | masks | slot bases | codes (tile order) | floats, so a gather copies the fixed part and as many
 * floats as were used.  The order of the tiles' floats is whatever order the waves finished in; the expanded frame does not
 * depend on it (bit for bit the frame sdfhip_render_device writes).
 *   sdfhip_sparse2_bytes / _floats_offset   size of a share; offset of its float array (= bytes of the fixed part)
 *   sdfhip_render_sparse_device             like sdfhip_render_bands_device (explicit band list, n_frames <= 8 in one launch),
 *                                           output = one share at d_share.  The share's counter (header word 0) is never zeroed
 *                                           by the library: a launch counts on from `count_base`, which must be the counter's
 *                                           value before the launch (0 for a buffer the caller zeroed; after a launch that used n
 *                                           slots, count_base + n, modulo 2^32) -- no memset between the frames of a viewer
 *   sdfhip_deinterleave_sparse2_device      d_shares[r] = rank r's share (device pointers valid on `device`; world <= 16) ->
 *                                           d_frame [frames][height][width] RGBA32F, or with SDFHIP_FLAG_DISPLAY[_DEBUG] in
 *                                           `flags` RGBA8 through the display pass; only_rank >= 0: write that rank's rows only;
 *                                           counts_out (may be NULL; device-accessible, e.g. pinned host memory): receives the
 *                                           `world` counters of the shares as they arrived */
SDFHIP_API uint64_t sdfhip_sparse2_bytes(uint32_t width, uint32_t rows, uint32_t frames, uint32_t capacity);
SDFHIP_API uint64_t sdfhip_sparse2_floats_offset(uint32_t width, uint32_t rows, uint32_t frames);
SDFHIP_API int sdfhip_render_sparse_device(sdfhip_scene *scene, const sdfhip_info *infos, uint32_t n_frames, uint32_t width,
                                           uint32_t height, uint32_t band_rows, const uint16_t *bands, uint32_t n_bands,
                                           uint32_t nrows_out, uint32_t capacity, uint32_t count_base, uint32_t flags, void *d_share,
                                           void *stream);
SDFHIP_API int sdfhip_deinterleave_sparse2_device(int device, const void *const *d_shares, void *d_frame, uint32_t width,
                                                  uint32_t height, uint32_t band_rows, uint32_t world, uint32_t rows_per_rank,
                                                  const uint8_t *owner, uint32_t capacity, uint32_t frames, uint32_t flags,
                                                  int only_rank, uint32_t *counts_out, void *stream);

/* ---- space carving: brush edits of a resident scene -----------------------------------------------
 * Replaces: nothing in the reference's code -- its README lists "Add support for modeling, as efficient space carving is one of
 * the main benefits of distance fields" under "Plans", and a tree there is immutable once built.
 * sdfhip_scene_edit applies n_edits brushes, in order, to the tree of `scene` on its device and returns the result as a NEW handle
 * `*out` on the same device: the input is untouched (frames in flight on it included) and either handle may be freed first.  A list
 * gives byte for byte the tree that chained single calls give; n_edits = 0 is a clone.  The arithmetic is pinned (fp32, in the
 * order written):
 *   brush s(p): sphere sqrtf((dx*dx + dy*dy) + dz*dz) - r; box q = |p - c| - h, sqrtf(|max(q, 0)|^2) + fminf(fmaxf(qx, fmaxf(qy, qz)), 0);
 *               g = -s to carve (subtract), g = s to add (union)
 *   bytes:      q(f, S) = floorf(saturate(f/2/S + 0.25f) * 255) (SdfGen's FromFloat); a corner's byte becomes max(p, q(g, S))
 *               (carve) or min(p, q(g, S)) (add), p its byte before the edit
 *   refinement: a leaf above max_depth whose centre has |s| < 2 S (the builder's band, Model.cs:44) and where the brush wins over
 *               the trilinear value of its corners (carve: g > v, add: g < v) gets 8 children, whose values before the edit are
 *               the parent's, interpolated; they are edited by the same rules, recursively.  Nothing is pruned (sdfhip_scene_prune does).
 *   node order: original nodes keep their indices; new blocks of 8 are appended in the order (depth of the block, parent index).
 * max_depth: -1 = the input's depth, else 0..12 (deeper than the input lets brushes refine past it).  host_out (may be NULL): the
 * result's host arrays, as sdfhip_sdfgen_scene's `out` (release with sdfhip_octdata_free).  stats (may be NULL).
 * SDFHIP_ERR_ARG: a null pointer, an unknown op or brush, a non-finite parameter, r <= 0 or h <= 0, max_depth outside -1..12, a
 * result of more than 2^31 - 1 nodes; SDFHIP_ERR_BAD_TREE: the input is not consistent (stack_kernel_ok == 0 in
 * sdfhip_scene_info); SDFHIP_ERR_NOMEM: out of device memory (the input stays valid, nothing leaks).
 * Work is proportional to the nodes near and inside the brushes, not to the tree; the new handle builds its lookup grids anew. */
enum { SDFHIP_EDIT_CARVE = 0, SDFHIP_EDIT_ADD = 1 };          /* subtract / union */
enum { SDFHIP_BRUSH_SPHERE = 0, SDFHIP_BRUSH_BOX = 1 };
typedef struct sdfhip_edit {
    int32_t op, brush;
    float params[6];        /* sphere: cx cy cz r; box: cx cy cz hx hy hz (axis-aligned, half extents) */
} sdfhip_edit;
typedef struct sdfhip_edit_stats {
    uint32_t nodes_in, nodes_out;
    uint32_t nodes_visited;  /* nodes whose bytes the edits evaluated: original nodes the brushes reach, and every new node */
    uint32_t nodes_changed;  /* original nodes whose bytes changed (a node edited by several brushes counts once per brush) */
    uint32_t blocks_added, depth_out;
    float edit_ms;           /* HIP events around the edit's kernels */
    float scene_ms;          /* building the new handle (fused records, lookup grids), host clock */
    float total_ms;          /* host clock, the whole call */
} sdfhip_edit_stats;
SDFHIP_API int sdfhip_scene_edit(sdfhip_scene *scene, const sdfhip_edit *edits, uint32_t n_edits, int32_t max_depth, sdfhip_scene **out,
                                 sdfhip_octdata *host_out, sdfhip_edit_stats *stats);

/* ---- pruning: collapse the blocks of a resident scene that their parent already describes ------------
 * Replaces: nothing in the reference's code -- a tree there is immutable once built, and sdfhip_scene_edit only ever grows one.
 * sdfhip_scene_prune removes the redundant blocks of eight of the tree of `scene` on its device and returns the result as a NEW handle
 * `*out` on the same device: the input is untouched (frames in flight on it included) and either handle may be freed first.  The
 * tree leaves HBM only for host_out.  The rule, pinned (fp32, each operation rounded on its own in the order written, as the edit's):
 *   inherited byte   for an internal node P of depth d, S = 2^-d, bytes b[0..7]: f[j] = ((b[j] / 255.0f) - 0.25f) * S * 2.0f; child
 *                    i's corner k sits at t_a = ((i >> a & 1) + (k >> a & 1)) * 0.5f per axis a; v = trilerp(f, t_x, t_y, t_z) with
 *                    lerp(a, b, t) = a + (b - a) * t along x, then y, then z; q(i, k) = floorf(saturate(v / 2 / (S * 0.5f) + 0.25f) * 255)
 *                    -- exactly the byte sdfhip_scene_edit gives a new child before the brush touches it
 *   redundant block  the eight children of P are redundant iff (1) every child is a leaf, or has become one by this rule, and
 *                    (2) the children's depth d + 1 exceeds max_depth (when max_depth >= 0), or every one of the 64 bytes has
 *                    |byte(i, k) - q(i, k)| <= tolerance, compared as integers
 *   cascade          a redundant block is removed and P becomes a leaf (children -1) with its own bytes; decided from the deepest
 *                    level up, so one call collapses as many levels as collapse
 *   node order       survivors keep their relative order: a survivor's new index is the number of survivors with a lower old index;
 *                    parent and children are remapped, no surviving byte changes, blocks of eight stay contiguous (siblings live or
 *                    die together).  The result depends on the input arrays and the two options alone, never on which wave finished
 *                    first.
 * opt: NULL = defaults.  tolerance: 0..255, -1 = the default, 0.  max_depth: -1 = no cut, else 0..12.  The struct grows like
 * sdfhip_mesh_options: the caller sets size = sizeof(sdfhip_prune_options); a larger, newer struct is accepted when the fields this
 * library does not know are all -1.  Tolerance 0 without a cut on a tree with nothing redundant is a clone; tolerance 255, or
 * max_depth 0, gives the root alone.  host_out (may be NULL): the result's host arrays (release with sdfhip_octdata_free).  stats
 * (may be NULL).
 * SDFHIP_ERR_ARG: a null scene or output, tolerance outside -1..255, max_depth outside -1..12, an options struct the size rules
 * refuse; SDFHIP_ERR_BAD_TREE: the tree is not consistent (stack_kernel_ok == 0 in sdfhip_scene_info) or deeper than 12 levels, as
 * sdfhip_scene_edit refuses it; SDFHIP_ERR_NOMEM: out of device memory (the input stays valid, nothing leaks).
 * Work is proportional to the tree: every record is read, every survivor written; the new handle builds its lookup grids anew. */
typedef struct sdfhip_prune_options {
    uint32_t size;          /* sizeof(sdfhip_prune_options) of the caller's header */
    int32_t tolerance;      /* 0..255; -1 = default (0) */
    int32_t max_depth;      /* -1 = no cut; 0..12: every block whose children are deeper is removed */
} sdfhip_prune_options;
typedef struct sdfhip_prune_stats {
    uint32_t nodes_in, nodes_out;
    uint32_t blocks_removed, depth_out;
    float kernel_ms;         /* HIP events around the prune's kernels */
    float scene_ms;          /* building the new handle (fused records, lookup grids), host clock */
    float total_ms;          /* host clock, the whole call */
} sdfhip_prune_stats;
SDFHIP_API int sdfhip_scene_prune(sdfhip_scene *scene, const sdfhip_prune_options *opt, sdfhip_scene **out, sdfhip_octdata *host_out,
                                  sdfhip_prune_stats *stats);

/* ---- combination: the union, intersection or difference of two resident scenes -----------------------
 * Replaces: nothing in the reference's code -- a tree there is immutable once built and its only consumer draws one tree; two
 * models could meet only as triangles, before a rebuild.
 * sdfhip_scene_combine combines the trees of `a` and `b`, which live in the same unit cube on the same device, and returns the result
 * as a NEW handle `*out` on that device: both inputs are untouched (frames in flight on them included), any of the three handles may
 * be freed first, and a == b is allowed.  Calls on the operands from other threads (renders, queries) do not wait for the
 * combination: it holds the handles' locks only while it reads what they describe.  Every octree cell of one operand has the same address in the other, so nothing is
 * resampled: the trees leave HBM only for host_out.  An operand is placed beforehand (sdfhip_scene_place, below); there is no
 * blending, and nothing is pruned.  The rule, pinned (fp32, each operation rounded on its own in the order written, as the edit's and
 * the prune's; S = 2^-d the edge of a cell of depth d):
 *   cells            a cell of depth d is a node of the result iff it is a node of A or of B (the root always is).  A result node has
 *                    a block of eight children iff A's node there has children or B's has, and d < max_depth when a cut is given
 *   operand bytes    at a result cell, operand X's own eight bytes if X has this node.  Otherwise they are inherited: starting from
 *                    X's leaf that contains the cell, sdfhip_scene_prune's inherited byte q(i, k) is applied once per level down to
 *                    the cell, re-quantising at every level -- sdfhip_scene_edit's rule for new children, iterated
 *   negation         SUBTRACT only, applied to B's bytes at the result cell, after the inheritance:
 *                    neg(b) = floorf(saturate(-f / 2 / S + 0.25f) * 255), f = ((b / 255.0f) - 0.25f) * S * 2.0f; byte 63 becomes 64
 *                    and 64 becomes 63, so the sign flips exactly at the surface
 *   result byte      per corner: UNION min(a, b); INTERSECT max(a, b); SUBTRACT max(a, neg(b))
 *   node order       breadth first, as sdfhip_trimesh_build's: node 0 is the root (parent -1); a level's child blocks follow in
 *                    ascending result index of the parent; child i is at block + i; a leaf's children field is -1.  Bytes and links
 *                    depend on the operands' arrays, the op and the option alone, never on which wave finished first
 *   nothing is pruned  nodes_out <= nodes_a + nodes_b - 1.  Where one operand wins outright the other's structure stays in the
 *                    result with interpolated bytes; sdfhip_scene_prune at tolerance 0 on the result removes exactly those blocks
 * opt: NULL = defaults.  max_depth: -1 = no cut, else 0..12.  The struct grows like sdfhip_prune_options: the caller sets size =
 * sizeof(sdfhip_combine_options); a larger, newer struct is accepted when the fields this library does not know are all -1.
 * host_out (may be NULL): the result's host arrays (release with sdfhip_octdata_free).  stats (may be NULL).
 * SDFHIP_ERR_ARG: a null scene or output, an unknown op, max_depth outside -1..12, an options struct the size rules refuse, operands
 * on different devices, a result of more than 2^31 - 1 nodes; SDFHIP_ERR_BAD_TREE: either operand is not consistent
 * (stack_kernel_ok == 0 in sdfhip_scene_info) or deeper than 12 levels, as sdfhip_scene_prune refuses it; SDFHIP_ERR_NOMEM: out of
 * device memory (both inputs stay valid, nothing leaks).
 * Work is proportional to the result: every record of both operands is read once or twice, every result node written; the call's
 * device memory is sized for nodes_a + nodes_b - 1 nodes (or the full tree of max_depth, if smaller); the new handle builds its
 * lookup grids anew. */
enum { SDFHIP_COMBINE_UNION = 0, SDFHIP_COMBINE_INTERSECT = 1, SDFHIP_COMBINE_SUBTRACT = 2 };   /* A or B, A and B, A without B */
typedef struct sdfhip_combine_options {
    uint32_t size;          /* sizeof(sdfhip_combine_options) of the caller's header */
    int32_t max_depth;      /* -1 = no cut; 0..12: no result node is deeper */
} sdfhip_combine_options;
typedef struct sdfhip_combine_stats {
    uint32_t nodes_a, nodes_b, nodes_out, depth_out;
    uint32_t nodes_shared;   /* result cells that are nodes of both operands */
    float kernel_ms;         /* HIP events around the combination's kernels (the per-level host synchronisations included) */
    float scene_ms;          /* building the new handle (fused records, lookup grids), host clock */
    float total_ms;          /* host clock, the whole call */
} sdfhip_combine_stats;      /* 32 bytes */
SDFHIP_API int sdfhip_scene_combine(sdfhip_scene *a, sdfhip_scene *b, int32_t op, const sdfhip_combine_options *opt,
                                    sdfhip_scene **out, sdfhip_octdata *host_out, sdfhip_combine_stats *stats);

/* ---- placement: a resident scene rotated, scaled and moved by resampling ----------------------------
 * Replaces: nothing in the reference's code -- a tree there sits where its builder put it; a model that was loaded, built from
 * points or carved could be moved only as triangles, before a rebuild, losing everything below the mesh's resolution.
 * sdfhip_scene_place resamples the tree of `scene` under the similarity p = s * R x + t (a source point x lands at p) into a new tree
 * and returns it as a NEW handle `*out` on the same device: the input is untouched (frames in flight on it included) and either
 * handle may be freed first.  Calls on the source from other threads do not wait for the placement: it holds the handle's lock only
 * while it reads what the handle describes.  The tree leaves HBM only for host_out.  sdfhip_scene_combine, _prune, _edit, _mesh and
 * the renderers take the result as any other scene.  The rule, pinned (fp32, each operation rounded on its own in the order written;
 * S = 2^-d the edge of a cell of depth d):
 *   inverse map      for a destination point p: d = p - t per axis; inv = 1.0f / s;
 *                    q_a = ((R[0][a] * d_0 + R[1][a] * d_1) + R[2][a] * d_2) * inv -- the transpose of R applied to d
 *   value            qc = min(max(q, 0), 1) per axis (fmaxf / fminf); e = q - qc; D = the distance sdfhip_scene_sample returns at qc
 *                    (find from the root, interpol_world: the shader's arithmetic untouched);
 *                    value(p) = (D + sqrtf((e_0 * e_0 + e_1 * e_1) + e_2 * e_2)) * s.  Inside the source's cube e is 0 and the value is
 *                    D * s, with no branch; outside, the source's field continues at slope 1 from the nearest point of the cube's surface
 *   tree             sdfhip_trimesh_build's construct rule with this value: corner k of a node of depth d with integer coordinates c
 *                    sits at (c + split(k)) * S, its centre at (2 c + 1) * (S * 0.5f) (exact dyadics); byte = FromFloat(value, S); the
 *                    node splits iff fabsf(value(centre)) < 2 * S && d < depth.  Every point is evaluated as if alone: that siblings
 *                    share corners is an optimisation that cannot change a byte
 *   node order       breadth first, as sdfhip_trimesh_build's and sdfhip_scene_combine's: node 0 is the root (parent -1); a level's
 *                    blocks of eight follow in ascending index of their parents; child i is at block + i; a leaf's children field is
 *                    -1.  Bytes and links depend on the source's arrays and the placement alone, never on which wave finished first
 * What the rule implies.  A source's bytes saturate at -0.5 and 1.5 of its leaf's edge, so |D| stays small where the source's leaves
 * are small: inside a solid and in the band round it the result can be finer than the source, by up to two levels of the scaled
 * leaf.  Nothing is pruned: sdfhip_scene_prune removes what a tolerance allows.  The identity placement is a resampling, not a clone
 * (the depth-4 sphere of 3 465 nodes comes back with 4 681).  A source moved wholly out of the cube, or depth 0, gives the root alone.
 * placement: the caller sets size = sizeof(sdfhip_placement); the struct grows like sdfhip_prune_options (a larger, newer struct is
 * accepted when the fields this library does not know are all -1).  There is no _default helper.  rotation: R, row-major, orthogonal
 * (mirrors allowed); scale: s > 0; translation: t; depth: -1 = the source's depth, else 0..12 -- the deepest level of the result.
 * out, host_out: either may be NULL, not both; host_out: the result's host arrays (release with sdfhip_octdata_free).  stats (may be
 * NULL): samples counts the source look-ups, 9 for the root and 35 for every block of eight siblings (the 27 corners of its lattice and
 * its 8 centres).
 * SDFHIP_ERR_ARG: a null scene or placement, both outputs NULL, a size the growth rule refuses, a non-finite field, s <= 0, a rotation
 * with max |(R R^T - I)_ij| > 1e-4 (computed in double; the bound defines the interface), depth outside -1..12 -- each of these before
 * any device call -- and a result of more than 2^31 - 1 nodes; SDFHIP_ERR_BAD_TREE: depth -1 on a source that has no depth to give (not
 * consistent, or deeper than 12 levels; with a depth given the call accepts every scene sdfhip_scene_sample accepts); SDFHIP_ERR_NOMEM:
 * out of device memory (the input stays valid, nothing leaks).
 * A look-up is a grid lookup wherever the handle has a full-depth grid, as sdfhip_scene_raycast's, else the walk along the links;
 * both give the same bytes.  Work is proportional to the result; its device memory grows level by level; the host waits once per
 * level for the level's count; the new handle builds its lookup grids anew. */
typedef struct sdfhip_placement {
    uint32_t size;            /* sizeof(sdfhip_placement) of the caller's header */
    float rotation[3][3];     /* R, row-major, orthogonal */
    float scale;              /* s > 0 */
    float translation[3];     /* t */
    int32_t depth;            /* -1 = the source's depth; else 0..12 */
} sdfhip_placement;           /* 60 bytes */
typedef struct sdfhip_place_stats {
    uint32_t nodes_in, nodes_out, depth_out, levels;
    uint64_t samples;        /* source look-ups made */
    float kernel_ms;         /* HIP events around the placement's kernels (the per-level host synchronisations included) */
    float scene_ms;          /* building the new handle (fused records, lookup grids), host clock */
    float total_ms;          /* host clock, the whole call */
    uint32_t pad_;
} sdfhip_place_stats;        /* 40 bytes */
SDFHIP_API int sdfhip_scene_place(sdfhip_scene *scene, const sdfhip_placement *pl, sdfhip_scene **out, sdfhip_octdata *host_out,
                                  sdfhip_place_stats *stats);

/* ---- composition: one scene from many placed instances, in a single pass ------------------------------
 * Replaces: nothing in the reference's code -- a tree there is immutable once built and sits where its builder put it; an assembly of
 * parts could exist only as triangles, before a rebuild.
 * sdfhip_scene_compose builds ONE tree from `n_instances` instances, each a resident scene under a placement of its own and an op
 * that says how it joins what precedes it in the list, and returns it as a NEW handle `*out` on the sources' device.  The same
 * handle may appear in as many instances as the caller likes: sixteen copies of a part are sixteen entries of the list, not sixteen
 * trees.  Every source is untouched (frames in flight on it included) and any handle may be freed first.  Calls on a source from
 * other threads do not wait for the composition: each distinct source is read under its own lock, one after the other and never two
 * locks at once, and the lock is released before any work is issued.  The tree leaves HBM only for host_out.  The rule, pinned (fp32,
 * each operation rounded on its own in the order written; S = 2^-d the edge of a cell of depth d):
 *   value of k       u_k(p) = sdfhip_scene_place's value(p) of instances[k].scene under instances[k]'s rotation, scale and
 *                    translation, word for word: the inverse map, the clamp to the source's cube, the distance sdfhip_scene_sample
 *                    returns there, the continuation at slope 1 outside the cube, the multiplication by s
 *   fold             in list order: v = u_0 (instance 0's op must be SDFHIP_COMBINE_UNION: it has nothing to join); for k >= 1
 *                    SDFHIP_COMBINE_UNION v = fminf(v, u_k); _INTERSECT v = fmaxf(v, u_k); _SUBTRACT v = fmaxf(v, -u_k).  No NaN can
 *                    arise: the sources' fields are finite and every look-up is clamped
 *   tree             sdfhip_scene_place's tree, word for word, with this value: byte = FromFloat(v, S); a node splits iff
 *                    fabsf(v(centre)) < 2 * S && d < depth.  Every point is evaluated as if alone, against every instance
 *   node order       breadth first, as sdfhip_scene_place's.  Bytes and links depend on the sources' arrays and the list alone, never
 *                    on which wave finished first
 * What the rule implies.  One instance is sdfhip_scene_place byte for byte.  Nothing about an instance is special-cased: one placed
 * wholly outside the cube still has a value everywhere -- its field continued at slope 1 -- and leaves a union unchanged only where
 * that value exceeds the others'.  Nothing is pruned: chain sdfhip_scene_prune.  The result differs from sdfhip_scene_combine of sdfhip_scene_place's results, by design: that
 * route rounds every part to bytes and then takes min / max of bytes at the same cell, with bytes interpolated from a coarser leaf
 * where an operand has no node, and keeps every cell either operand had; here the parts' own fields are folded in float, rounded to a
 * byte once, and the split rule is applied to the folded value -- one quantisation instead of two, one tree instead of 2 K - 1.
 * instances: 1..4096 of them.  rotation, scale, translation: as sdfhip_placement's (R row-major and orthogonal, mirrors allowed; s > 0;
 * a source point x lands at s R x + t).  opt: NULL = defaults; the caller sets size = sizeof(sdfhip_compose_options), and the struct
 * grows like sdfhip_placement.  depth: -1 = the largest depth among the instances' sources, else 0..12 -- the deepest level of the
 * result.  out, host_out: either may be NULL, not both; host_out: the result's host arrays (release with sdfhip_octdata_free).  stats
 * (may be NULL): samples counts the look-ups the rule defines, instances * (9 for the root + 35 for every block of eight siblings).
 * SDFHIP_ERR_ARG: a null list, n_instances outside 1..4096, both outputs NULL, a size the growth rule refuses, depth outside -1..12,
 * and for an instance -- the message names its index -- a null scene, an unknown op, a first op other than SDFHIP_COMBINE_UNION, a
 * non-finite field, s <= 0, a rotation with max |(R R^T - I)_ij| > 1e-4 (in double, as the placement's), a source on another device than
 * instance 0's -- each of these before any device call -- and a result of more than 2^31 - 1 nodes; SDFHIP_ERR_BAD_TREE: depth -1 with
 * a source that has no depth to give (not consistent, or deeper than 12 levels), as the placement refuses it; SDFHIP_ERR_NOMEM: out of
 * device memory (every source stays valid, nothing leaks).
 * Each look-up takes its source's own cursor (a grid lookup wherever that handle has a full-depth grid, else the walk along the
 * links), so the instances of one call may mix the forms; all give the same bytes.  Work is proportional to the result times the
 * number of instances: every instance is looked up at every point, nothing is skipped.  Device memory grows level by level from the
 * distinct sources' sizes together; the host waits once per level; the new handle builds its lookup grids once.  Measured on an
 * MI355X to depth 9 on a 28 M-node scene and a 39 k-node torus (profiles/compose_bench.json): 2 instances 1.43 ms
 * against 3.05 ms for two placements and a combination, 8 instances 6.53 against 20.6 ms, 32 instances 11.8 against 59.0 ms. */
typedef struct sdfhip_instance {
    sdfhip_scene *scene;      /* resident source; the same handle may appear in several instances */
    int32_t op;               /* SDFHIP_COMBINE_UNION / _INTERSECT / _SUBTRACT: how this instance joins what precedes it */
    float rotation[3][3];     /* as sdfhip_placement: p = s R x + t */
    float scale;
    float translation[3];
} sdfhip_instance;            /* 64 bytes */
typedef struct sdfhip_compose_options {
    uint32_t size;            /* sizeof(sdfhip_compose_options) of the caller's header */
    int32_t depth;            /* -1 = the largest depth among the sources; else 0..12 */
} sdfhip_compose_options;     /* 8 bytes */
typedef struct sdfhip_compose_stats {
    uint32_t nodes_out, depth_out, levels, instances;
    uint64_t samples;        /* instances * (9 for the root + 35 per block of eight siblings): the look-ups the rule defines */
    float kernel_ms;         /* HIP events around the levels' kernels (the per-level host synchronisations included) */
    float scene_ms;          /* building the new handle (fused records, lookup grids), host clock */
    float total_ms;          /* host clock, the whole call */
    uint32_t pad_;
} sdfhip_compose_stats;      /* 40 bytes */
SDFHIP_API int sdfhip_scene_compose(const sdfhip_instance *instances, uint32_t n_instances, const sdfhip_compose_options *opt,
                                    sdfhip_scene **out, sdfhip_octdata *host_out, sdfhip_compose_stats *stats);

/* ---- volumes in and out: a dense lattice of distances as a scene, and a scene as one ------------------
 * Replaces: nothing in the reference's code -- its builder takes a point cloud and its tree only ever becomes pixels.  A field that
 * lives on a regular lattice -- a neural SDF evaluated on a grid, a TSDF from depth fusion, a level set, the distance transform of a
 * segmented scan -- had to be meshed elsewhere and rebuilt from triangles, losing the field; and a scene could be read as an array
 * only point by point, through sdfhip_probe records.
 * sdfhip_volume_build builds a NEW scene `*out` on `device` from the lattice `vol` of samples at `grid` (host memory, staged);
 * sdfhip_volume_build_device takes the samples from memory of `device`, which must be complete when the call is made and is only
 * read.  Both work on a stream of their own and return a finished handle, as sdfhip_scene_place does; the tree leaves HBM only for
 * host_out.  sdfhip_scene_volume fills the lattice `lattice` with the scene's distances (host memory, synchronous);
 * sdfhip_scene_volume_device fills device memory asynchronously on `stream` (NULL = the HIP default stream) with no host
 * synchronisation: sdfhip_scene_sample_device's convention.  The rules, pinned (fp32, each operation rounded on its own in the order
 * written; S = 2^-d the edge of a cell of depth d):
 *   build, per axis a  inv = 1.0f / spacing (one IEEE division, on the host).  For a destination point p: g = (p_a - origin_a) * inv;
 *                      gc = fminf(fmaxf(g, 0), (float)(n_a - 1)); e_a = (g - gc) * spacing; i = min((int)gc, n_a - 2); f = gc - (float)i
 *   build, value       the eight samples at i .. i + 1 per axis, converted to float (the F16 conversion is exact), under
 *                      lerp(u, v, f) = u * (1.0f - f) + v * f -- u at f = 0 and v at f = 1 exactly, so a point on a lattice vertex reads
 *                      that vertex's sample bit for bit, the last plane included (there i = n - 2 and f = 1) -- four times along x, then
 *                      two along y, then one along z: D.  value(p) = D * value_scale + sqrtf((e_0 * e_0 + e_1 * e_1) + e_2 * e_2).
 *                      Inside the lattice's box e is 0; outside, the field continues at slope 1 from the nearest point of the box, as the
 *                      placement's does outside the source's cube
 *   build, tree        sdfhip_scene_place's tree and node order, word for word, with this value: byte = FromFloat(value, S); a node
 *                      splits iff fabsf(value(centre)) < 2 * S && d < depth; breadth first
 *   out                element (i, j, k) is the placement's value at the identity: p_a = origin_a + (float)i_a * spacing;
 *                      qc = min(max(p, 0), 1) per axis (fmaxf / fminf); e = p - qc; D = the distance sdfhip_scene_sample returns at qc;
 *                      element = D + sqrtf((e_0 * e_0 + e_1 * e_1) + e_2 * e_2), stored as float or as its nearest half
 *                      (round to nearest even)
 * What the build's rule implies.  The split rule assumes a distance: |value| < 2 S only within two cells of the surface.  A field
 * truncated at +-tau satisfies it everywhere once 2 S >= tau, so every node of those levels splits: the 33^3 torus clipped at
 * +-1/16 has full levels 4 and 5 (4 096 and 32 768 nodes) at depth 6, and 75 657 nodes against 39 241 unclipped.  Nothing is pruned:
 * chain sdfhip_scene_prune.  A lattice wholly away from the cube, or depth 0, gives the root alone.  Before the first level one
 * pass counts the grid's non-finite samples; any refuses the call (the message names the count).
 * The round trip: every point a build to depth d evaluates is a vertex of the lattice {n = 2^d + 1 per axis, origin 0, spacing
 * 2^-d}, and vertices are exact, so sdfhip_volume_build of sdfhip_scene_volume's answer on that lattice is sdfhip_scene_place's
 * tree at the identity to depth d, byte for byte.
 * vol / lattice: the caller sets size = sizeof(sdfhip_volume); the struct grows like sdfhip_placement.  out, host_out, stats: as
 * sdfhip_scene_place's; samples counts 9 lattice reads for the root and 35 for every block of eight siblings.
 * SDFHIP_ERR_ARG: a null record, grid or output, both build outputs NULL, a size the growth rule refuses, n_a outside 2..4096 (build)
 * or 1..4096 (out), more than 2^31 samples, a spacing that is not finite and above 0, a non-finite origin, an unknown dtype; for the
 * build a value_scale that is not finite or is 0 (a negative one is allowed: fields positive inside) and a depth outside 0..12;
 * for the out direction a value_scale or a depth other than 0, and a null scene -- each of these before any device call -- then a
 * grid with a non-finite sample, and a result of more than 2^31 - 1 nodes; SDFHIP_ERR_NOMEM: out of device memory (nothing leaks). */
enum { SDFHIP_VOLUME_F32 = 0, SDFHIP_VOLUME_F16 = 1 };
typedef struct sdfhip_volume {
    uint32_t size;            /* sizeof(sdfhip_volume) of the caller's header */
    uint32_t n[3];            /* samples along x, y, z: element (i, j, k) at index (k * n[1] + j) * n[0] + i */
    float origin[3];          /* position of sample (0, 0, 0) in the scene's unit cube coordinates */
    float spacing;            /* above 0, uniform: sample (i, j, k) sits at origin + (i, j, k) * spacing */
    float value_scale;        /* build only: stored value * value_scale = distance in cube units (voxel units: = spacing) */
    int32_t dtype;            /* SDFHIP_VOLUME_F32 / SDFHIP_VOLUME_F16 */
    int32_t depth;            /* build only: 0..12, the deepest level of the result */
} sdfhip_volume;              /* 44 bytes */
typedef struct sdfhip_volume_stats {
    uint32_t nodes_out, depth_out, levels, pad_;
    uint64_t samples;        /* lattice reads made: 9 for the root, 35 per block of eight siblings */
    float check_ms;          /* HIP events around the pass that counts the non-finite samples */
    float kernel_ms;         /* HIP events around the levels' kernels (the per-level host synchronisations included) */
    float scene_ms;          /* building the new handle (fused records, lookup grids), host clock */
    float total_ms;          /* host clock, the whole call */
} sdfhip_volume_stats;       /* 40 bytes */
SDFHIP_API int sdfhip_volume_build(int device, const void *grid, const sdfhip_volume *vol, sdfhip_scene **out, sdfhip_octdata *host_out,
                                   sdfhip_volume_stats *stats);
SDFHIP_API int sdfhip_volume_build_device(int device, const void *d_grid, const sdfhip_volume *vol, sdfhip_scene **out,
                                          sdfhip_octdata *host_out, sdfhip_volume_stats *stats);
SDFHIP_API int sdfhip_scene_volume(sdfhip_scene *scene, const sdfhip_volume *lattice, void *out);
SDFHIP_API int sdfhip_scene_volume_device(sdfhip_scene *scene, const sdfhip_volume *lattice, void *d_out, void *stream);

/* ---- point and ray queries: what a resident scene answers without drawing a frame -------------------
 * Replaces: nothing in the reference's code -- its only consumer of the tree is Compute.hlsl; a host that wants the distance at a
 * point (collision, placement, snapping) or the surface point under the cursor (where to put a brush) has no call to make there.
 * Three questions, answered for a batch on the scene's device with the shader's own arithmetic (fp32, each operation rounded in the
 * order written, fused where the oracle fuses: DESIGN.md section 3), so an answer is bit for bit what a pixel of a frame would
 * have seen:
 *   sample    per point: interpol_world(find(p)) from the root (Compute.hlsl:54-58, 88-108; oracle_distance_at), the cell find()
 *             ended in, and gradient() (Compute.hlsl:112-130) in that cell at p
 *   raycast   per ray: the primary march of Compute.hlsl:194-203 and where it ended
 *   pick      per pixel of a camera block: the same march from info->position along the kernel's own ray() (Compute.hlsl:163-168)
 *             for pixel (x, y) -- the shader's direction bit for bit, not a host re-computation -- with info's margin and limit:
 *             "what is under the cursor"
 * The march, pinned (oracle/sdf_oracle.c o_pixel's first loop; nothing added but t):
 *     prox = 1; i = 0; t = 0; cursor at the root
 *     while ((prox > margin * 2.0f || prox < 0.0f) && i < max_steps) {
 *         if (dot(pos, pos) > limit) -> SDFHIP_QUERY_ESCAPED
 *         find(pos); prox = interpol_world(pos); pos = fma(dir, prox, pos); t = t + prox; i++ }
 *     -> SDFHIP_QUERY_HIT if !(prox > margin * 2.0f || prox < 0.0f), else SDFHIP_QUERY_EXHAUSTED
 * A NaN prox (degenerate data) ends the loop exactly as it ends the shader's and is reported SDFHIP_QUERY_HIT with prox NaN.  A ray
 * that starts inside the solid reads a negative prox and marches backwards, as the shader's rule has it.  The cursor is carried
 * from step to step as in the shader (a position on a cell face belongs to the cell the cursor came from); sample starts every
 * point at the root.  Points outside [0,1]^3 are answered the way find / interpol_world answer them (saturated), not refused.
 * max_steps: 1..4096 (the shader's value is 100).  n = 0 is a success that touches nothing.
 * SDFHIP_ERR_ARG: a null pointer, max_steps out of range, a non-finite margin or limit; SDFHIP_ERR_NOMEM / SDFHIP_ERR_DEVICE as
 * elsewhere.  A bad ELEMENT is not an error of the call: it gets SDFHIP_QUERY_INVALID and zeros, and the rest of the batch is answered.
 *   sdfhip_scene_sample / _raycast / _pick      host arrays, synchronous (staged through device memory on the scene's own stream)
 *   sdfhip_scene_sample_device / _raycast_device  device pointers on the scene's device, asynchronous on `stream` (NULL = the HIP
 *                                               default stream), no host synchronisation: sdfhip_render_device's convention
 * xyz: n x 3 floats, packed.  pixels_xy: n x {x, y}.  Queries on one handle may run beside frames on other streams. */
enum { SDFHIP_QUERY_HIT = 0,        /* the march ended by the shader's own test: !(prox > margin * 2 || prox < 0)
                                       (sample: the point was looked up) */
       SDFHIP_QUERY_ESCAPED = 1,    /* dot(pos, pos) > limit before a step (Compute.hlsl:195): the pixel would be sky */
       SDFHIP_QUERY_EXHAUSTED = 2,  /* max_steps steps taken and the test still asks for more (the shader shades such a pixel anyway) */
       SDFHIP_QUERY_INVALID = 3 };  /* a non-finite coordinate, or a direction that is not finite or is all zero: nothing was looked up */
typedef struct sdfhip_probe {       /* 32 bytes: the answer for one point */
    float distance;                 /* interpol_world(find(p)) from the root */
    uint32_t node;                  /* index of the cell find() ended in */
    float scale;                    /* its edge length */
    uint32_t status;                /* SDFHIP_QUERY_HIT or SDFHIP_QUERY_INVALID */
    float gradient[3];              /* gradient() in that cell at p: differences of the decoded corner values across the cell, not
                                       normalised (d distance / d world = 2 * gradient) */
    uint32_t pad_;
} sdfhip_probe;
typedef struct sdfhip_ray { float origin[3], pad0_, dir[3], pad1_; } sdfhip_ray;   /* 32 bytes; dir is used as given */
typedef struct sdfhip_hit {         /* 48 bytes: where one ray's march ended */
    float position[3];              /* pos when the loop ended (after the last step) */
    float t;                        /* the steps' distances summed in fp32 in march order: ((p1 + p2) + p3) ... */
    float normal[3];                /* HIT / EXHAUSTED: gradient() in the cursor's cell at `position`, times 1 / sqrt(dot(g, g)) as the
                                       shader normalises (Compute.hlsl:209; a flat cell's zero gradient gives NaN there too); else 0 */
    float prox;                     /* the last distance read (1.0f if no step was taken) */
    uint32_t status, steps, node;   /* steps == the i of Compute.hlsl:194; node = the cursor's cell */
    float scale;
} sdfhip_hit;
SDFHIP_API int sdfhip_scene_sample(sdfhip_scene *scene, const float *xyz, uint32_t n, sdfhip_probe *out);
SDFHIP_API int sdfhip_scene_sample_device(sdfhip_scene *scene, const float *d_xyz, uint32_t n, sdfhip_probe *d_out, void *stream);
SDFHIP_API int sdfhip_scene_raycast(sdfhip_scene *scene, const sdfhip_ray *rays, uint32_t n, float margin, float limit, uint32_t max_steps,
                                    sdfhip_hit *out);
SDFHIP_API int sdfhip_scene_raycast_device(sdfhip_scene *scene, const sdfhip_ray *d_rays, uint32_t n, float margin, float limit,
                                           uint32_t max_steps, sdfhip_hit *d_out, void *stream);
SDFHIP_API int sdfhip_scene_pick(sdfhip_scene *scene, const sdfhip_info *info, const uint32_t *pixels_xy, uint32_t n, uint32_t max_steps,
                                 sdfhip_hit *out);

/* ---- an assembly of placed instances, drawn, probed and picked without baking ---------------------------
 * Replaces: nothing in the reference's code -- its shader marches one immutable tree.  sdfhip_scene_compose bakes a list of placed
 * instances into one tree, which is right once an arrangement has settled and wrong while a part is still being moved: every change
 * of a placement costs the rebuild before the first frame, and the baked tree has forgotten which part a surface point came from.
 * The calls below take the SAME list sdfhip_scene_compose takes (1..4096 instances on one device, instance 0 a union; rotation,
 * scale, translation as sdfhip_placement's) and consume its field directly: nothing is built, nothing is kept on the handles, and
 * every answer names the instance it came from.  The rule, pinned (fp32, each operation rounded on its own in the order written, the
 * shader's fused operations fused as DESIGN.md section 3 has them):
 *   F(p)       sdfhip_scene_compose's fold, word for word: u_k(p) = sdfhip_scene_place's value of instances[k]; v = u_0; then in list
 *              order UNION v = fminf(v, u_k); INTERSECT v = fmaxf(v, u_k); SUBTRACT v = fmaxf(v, -u_k).  Every look-up starts at its
 *              source's root: no cursor is carried from step to step, F depends on the point alone.  Here the value leaves as a
 *              float, so the one case C leaves open is pinned: of two zeros of opposite sign fminf gives -0 and fmaxf +0, whichever
 *              operand comes first (-0 orders below +0: IEEE 754-2019's minimumNumber / maximumNumber, and what gfx950's
 *              v_min_f32 / v_max_f32 compute).  It is met: a source that reads +0 at p, joined and then subtracted, folds
 *              fmaxf(+0, -0), and F(p) = +0
 *   w(p)       the winner, tracked beside the fold: w = 0; UNION: w = k iff u_k < v before the fold; INTERSECT: iff u_k > v; SUBTRACT:
 *              iff -u_k > v.  Ties keep the earlier instance
 *   G(p)       with h = normal_step: (F(p + (h,0,0)) - F(p - (h,0,0)), F(p + (0,h,0)) - F(p - (0,h,0)), F(p + (0,0,h)) - F(p - (0,0,h))),
 *              the offsets added and subtracted as vectors.  One rule for every op and cursor form, used wherever the shader uses
 *              gradient(); not normalised (d F / d world = G / (2 h))
 *   sample     per point: F(p), w(p), G(p)
 *   raycast    per ray: sdfhip_scene_raycast's march with find + interpol_world replaced by F:
 *                  prox = 1; i = 0; t = 0; w = 0
 *                  while ((prox > margin * 2.0f || prox < 0.0f) && i < max_steps) {
 *                      if (dot(pos, pos) > limit) -> SDFHIP_QUERY_ESCAPED
 *                      prox = F(pos); w = w(pos); pos = fma(dir, prox, pos); t = t + prox; i++ }
 *                  -> SDFHIP_QUERY_HIT if !(prox > margin * 2.0f || prox < 0.0f), else SDFHIP_QUERY_EXHAUSTED
 *              normal = G(position) * (1 / sqrtf(dot(G, G))) for HIT and EXHAUSTED, else 0; instance = the winner of the last
 *              evaluation (0 when no step was taken): the part under the cursor
 *   pick       per pixel of a camera block: that march from info->position along the kernel's own ray() (Compute.hlsl:163-168), with
 *              info's margin and limit
 *   render     a width x height RGBA32F frame, tightly packed, row 0 at the top, alpha = the march's steps, as sdfhip_render has it:
 *              every pixel is main() of Compute.hlsl:180-231 line for line (oracle/sdf_oracle.c o_pixel) with find + interpol_world
 *              replaced by F, gradient() by G -- at the shading point and inside the shadow loop's prox < margin test -- and 100 by
 *              max_steps.  The sky colour, the black pixel, angle, dist, the 40-step shadow loop, its leave-the-unit-cube exit, the
 *              prox + margin step and the attenuation are the shader's
 * The exact skip (on by default).  u_k = (D + e) * s with e the distance from the inverse-mapped point to the source's cube, known
 * before any look-up, and D >= -0.5625 for every tree an upload accepts (csrc/instances_kernels.h has the argument).  b_k =
 * (-0.5625f + e) * s <= u_k by monotone rounding alone; for k >= 1 a UNION instance is not looked up when b_k > v, a SUBTRACT instance
 * when -b_k < v; an INTERSECT instance and instance 0 always are.  A skipped instance can neither change v nor win, so the skip
 * changes no bit of any output; SDFHIP_INSTANCES_NO_SKIP turns it off (tests, A/B).
 * opt: NULL = defaults; the caller sets size = sizeof(sdfhip_instances_options), and the struct grows like sdfhip_placement.
 * max_steps: 0 = 100 (the shader's), else 1..4096.  normal_step: 0 = 2^-10, else finite and above 0.  n = 0 and a 0 x 0 frame are
 * successes that touch nothing.  A bad ELEMENT -- a non-finite coordinate, a direction that is not finite or is all zero -- is not an
 * error of the call: it gets SDFHIP_QUERY_INVALID and zeros, and the rest of the batch is answered.
 *   sdfhip_instances_sample / _raycast / _pick / _render    host arrays, synchronous, on a stream of the call's own
 *   sdfhip_instances_sample_device / _raycast_device / _render_device
 *              device pointers on the instances' device; the kernel is enqueued on `stream` (NULL = the HIP default stream), so it
 *              orders after the caller's earlier work there, and the call synchronises `stream` before it returns and releases the
 *              per-call instance table.  A fully asynchronous form, and an assembly object that keeps its table resident, do not exist
 * Every source is untouched and may be freed as soon as the call returns.  Each distinct source is read once, under its own lock,
 * as sdfhip_scene_compose reads it; each look-up takes its source's own cursor form, and all forms give the same bytes.
 * SDFHIP_ERR_ARG: a null list, n_instances outside 1..4096, a size the growth rule refuses, unknown flags, max_steps above 4096, a
 * normal_step that is not finite or is below 0, a non-finite margin or limit, a null info, a frame side above 16384, a null array
 * with n > 0, and for an instance -- the message names its index -- what sdfhip_scene_compose refuses of it, word for word (a null
 * scene, an unknown op, a first op other than SDFHIP_COMBINE_UNION, a non-finite field, s <= 0, a rotation that is not orthogonal, a
 * source on another device than instance 0's); SDFHIP_ERR_NOMEM: out of device memory (nothing leaks); SDFHIP_ERR_DEVICE as elsewhere.
 * Work is proportional to points x steps x instances looked up.  Measured on an MI355X (profiles/instances_bench.json, DESIGN.md
 * N17), a 1920 x 1080 frame of 2 / 8 / 32 instances of a 28 M-node scene and a 39 k-node torus: 0.75 / 4.04 / 15.9 ms with the skip,
 * 0.71 / 4.21 / 21.1 ms without, against 2.80 / 8.03 / 13.6 ms for sdfhip_scene_compose to depth 9 plus one frame of the result (a
 * resident frame of which takes 0.14 .. 0.31 ms: bake once the arrangement has settled); a pick of one pixel 0.40 .. 0.70 ms. */
enum { SDFHIP_INSTANCES_NO_SKIP = 1 };   /* sdfhip_instances_options.flags: look every instance up at every point */
typedef struct sdfhip_instances_options {
    uint32_t size, flags;           /* sizeof(sdfhip_instances_options) of the caller's header; SDFHIP_INSTANCES_* */
    uint32_t max_steps;             /* 0 = 100, else 1..4096 */
    float normal_step;              /* h of G: 0 = 2^-10, else finite and above 0 */
} sdfhip_instances_options;         /* 16 bytes */
typedef struct sdfhip_part_probe {  /* 32 bytes: the answer for one point */
    float value;                    /* F(p) */
    uint32_t instance;              /* w(p) */
    uint32_t status;                /* SDFHIP_QUERY_HIT or SDFHIP_QUERY_INVALID */
    uint32_t pad0_;
    float gradient[3];              /* G(p), not normalised */
    uint32_t pad1_;
} sdfhip_part_probe;
typedef struct sdfhip_part_hit {    /* 48 bytes: where one ray's march through the assembly ended */
    float position[3];              /* pos when the loop ended (after the last step) */
    float t;                        /* the steps' distances summed in fp32 in march order */
    float normal[3];                /* HIT / EXHAUSTED: G(position) * (1 / sqrtf(dot(G, G))); else 0 */
    float prox;                     /* the last value read (1.0f if no step was taken) */
    uint32_t status, steps;
    uint32_t instance;              /* the winner of the last evaluation: the part under the cursor */
    uint32_t pad_;
} sdfhip_part_hit;
SDFHIP_API int sdfhip_instances_sample(const sdfhip_instance *instances, uint32_t n_instances, const sdfhip_instances_options *opt,
                                       const float *xyz, uint32_t n, sdfhip_part_probe *out);
SDFHIP_API int sdfhip_instances_sample_device(const sdfhip_instance *instances, uint32_t n_instances, const sdfhip_instances_options *opt,
                                              const float *d_xyz, uint32_t n, sdfhip_part_probe *d_out, void *stream);
SDFHIP_API int sdfhip_instances_raycast(const sdfhip_instance *instances, uint32_t n_instances, const sdfhip_instances_options *opt,
                                        const sdfhip_ray *rays, uint32_t n, float margin, float limit, sdfhip_part_hit *out);
SDFHIP_API int sdfhip_instances_raycast_device(const sdfhip_instance *instances, uint32_t n_instances, const sdfhip_instances_options *opt,
                                               const sdfhip_ray *d_rays, uint32_t n, float margin, float limit, sdfhip_part_hit *d_out,
                                               void *stream);
SDFHIP_API int sdfhip_instances_pick(const sdfhip_instance *instances, uint32_t n_instances, const sdfhip_instances_options *opt,
                                     const sdfhip_info *info, const uint32_t *pixels_xy, uint32_t n, sdfhip_part_hit *out);
SDFHIP_API int sdfhip_instances_render(const sdfhip_instance *instances, uint32_t n_instances, const sdfhip_instances_options *opt,
                                       const sdfhip_info *info, uint32_t width, uint32_t height, float *rgba);
SDFHIP_API int sdfhip_instances_render_device(const sdfhip_instance *instances, uint32_t n_instances, const sdfhip_instances_options *opt,
                                              const sdfhip_info *info, uint32_t width, uint32_t height, float *d_rgba, void *stream);

/* ---- clash check: the pairwise overlaps of an assembly of placed instances, in one pass ----------------
 * Replaces: nothing in the reference's code.  The question of whoever drags a part of an assembly: does it now collide with another
 * part, with which, where, and by how much?  sdfhip_instances_clash takes the list sdfhip_instances_sample takes and answers it on a
 * cubic lattice, for every pair at once; it builds no tree and keeps nothing on the handles.  The rule, pinned (fp32, each operation
 * rounded on its own in the order written):
 *   lattice    depth d in 0..10, origin[3] and side (> 0, finite) give a cube; pitch = side * 2^-d (an exact scaling).  Lattice point
 *              (x, y, z), 0 <= x, y, z < 2^d, is p_a = fmaf((float)i_a + 0.5f, pitch, origin_a): the centres of the cube's 8^d cells.
 *              Its linear index is (z << 2d) | (y << d) | x, which fits in 32 bits
 *   contains   instance k contains p iff u_k(p) < 0, u_k = sdfhip_scene_place's value of instances[k], word for word (as F's above).
 *              A NaN contains nothing
 *   ops        are ignored: every instance counts as a solid.  A cutter listed as SDFHIP_COMBINE_SUBTRACT overlaps its target by
 *              design; the caller filters the records by a and b.  The list is still validated as sdfhip_instances_sample validates
 *              it, so the same list is accepted -- up to this call's own limit
 *   limit      n_instances is 1..SDFHIP_CLASH_MAX_INSTANCES = 64: a point's containment mask is one 64-bit word and one wave ballot.
 *              The limit is this call's, not the record's: a and b are 32-bit
 *   record     one 64-byte sdfhip_clash for every pair a < b that shares at least one lattice point: points = how many they share,
 *              first = the lowest linear index among them (a witness inside both), lo[3] / hi[3] = their inclusive lattice bounds,
 *              sum[3] = the sums of their x, y and z.  So the overlap's centroid is origin + (sum / points + 0.5) * pitch and its
 *              volume points * pitch^3.  Records come in (a, b) order
 *   integers   everything in a record is an integer, accumulated with integer atomic add / min / max only; no float is ever summed:
 *              the bytes are the same on every call, whatever the waves' timing
 * No penetration depth.  The minimum over the overlap of max(u_a, u_b) saturates at the source's own band -- every pair of depth-4
 * spheres at half size gives -0.015625 -- because the stored field is a distance only near the surface.  The true depth is
 * sdfhip_instances_penetration's (below), on sdfhip_scene_distance's exact field: this call at a coarse depth, then that one on the
 * record's box at a finer pitch.
 * The exact skip (on by default).  b_k = (-0.5625f + e) * s <= u_k as above, so b_k >= 0 implies u_k >= 0: only the points with
 * !(b_k >= 0) look instance k up, and a 4 x 4 x 4 block of the lattice in which fewer than two instances have such a point looks
 * nothing up at all.  No margin is involved; SDFHIP_CLASH_NO_SKIP looks every instance up at every point and gives the same records.
 * opt: NULL = the defaults (depth 6, origin 0, side 1, the skip on); sdfhip_clash_options_default sets them and the size, and the
 * struct grows like sdfhip_instances_options.  out receives the first min(capacity, total) records and *n_pairs the total; out may be
 * NULL with capacity 0 (count first, then fetch).  One instance is a success with 0 pairs.  stats (may be NULL): points = 8^d, blocks
 * = the 4 x 4 x 4 blocks of the lattice, blocks_looked = those that looked anything up, lookups = the look-ups made (points *
 * n_instances under SDFHIP_CLASH_NO_SKIP), the kernels' time and the call's.
 * Synchronous, on a stream of the call's own.  Every source is untouched and may be freed as soon as the call returns.
 * SDFHIP_ERR_ARG: a null list, n_instances outside 1..64 (the message names the limit), a size the growth rule refuses, unknown flags,
 * depth above 10, a non-finite origin, a side that is not finite or is <= 0 (or overflows origin + side), a null n_pairs, a null out with capacity > 0, and for an
 * instance what sdfhip_instances_sample refuses of it, word for word; SDFHIP_ERR_NOMEM: out of device memory (nothing is written,
 * nothing leaks); SDFHIP_ERR_DEVICE as elsewhere.  Work is proportional to 8^d * n_instances bounds plus the look-ups the skip leaves;
 * device memory is 64 bytes per pair of the list.  Measured on an MI355X (profiles/clash_bench.json), 2 / 8 / 32
 * instances of a 28 M-node scene and a 39 k-node torus on 16.8 M points (depth 8): 0.92 / 1.39 / 1.38 ms, against 9.2 / 14.3 / 36.5 ms
 * for as many sdfhip_instances_sample_device calls and the pairing of their values; at K = 8 the skip loses 6 % of the kernels' time. */
enum { SDFHIP_CLASH_NO_SKIP = 1 };       /* sdfhip_clash_options.flags: look every instance up at every lattice point */
enum { SDFHIP_CLASH_MAX_INSTANCES = 64 };
typedef struct sdfhip_clash_options {
    uint32_t size, flags;           /* sizeof(sdfhip_clash_options) of the caller's header; SDFHIP_CLASH_* */
    uint32_t depth;                 /* 0..10: 2^depth lattice points along each axis */
    float origin[3];                /* the cube's corner */
    float side;                     /* the cube's side: finite and above 0 */
} sdfhip_clash_options;             /* 28 bytes */
typedef struct sdfhip_clash {       /* 64 bytes: one pair of instances that share lattice points */
    uint32_t a, b;                  /* a < b: indices in the list */
    uint32_t points;                /* >= 1: the lattice points inside both */
    uint32_t first;                 /* the lowest linear index among them */
    uint32_t lo[3], hi[3];          /* their inclusive lattice bounds, {x, y, z} */
    uint64_t sum[3];                /* the sums of their x, y and z */
} sdfhip_clash;
typedef struct sdfhip_clash_stats { /* 32 bytes */
    uint64_t points;                /* 8^depth */
    uint32_t blocks, blocks_looked; /* 4 x 4 x 4 blocks of the lattice; those that looked anything up */
    uint64_t lookups;               /* (point, instance) look-ups made */
    float kernel_ms, total_ms;      /* the two kernels on the device; the whole call on the host */
} sdfhip_clash_stats;
SDFHIP_API void sdfhip_clash_options_default(sdfhip_clash_options *opt);
SDFHIP_API int sdfhip_instances_clash(const sdfhip_instance *instances, uint32_t n_instances, const sdfhip_clash_options *opt,
                                      sdfhip_clash *out, uint32_t capacity, uint32_t *n_pairs, sdfhip_clash_stats *stats);

/* ---- penetration depth: how far the overlapping pairs of an assembly reach into each other -------------
 * Replaces: nothing in the reference's code.  sdfhip_instances_clash says THAT two parts collide, where, and in how many lattice
 * points; this call says BY HOW MUCH and WHICH WAY TO PUSH.  It takes the same list (1..SDFHIP_CLASH_MAX_INSTANCES instances) and the
 * same lattice, and runs one exact nearest-surface search per (point, containing part) at the points inside at least two parts.  The
 * workflow: sdfhip_instances_clash at a coarse depth, the cube round a record's lo..hi (the bindings' clash_box), then this call on
 * that cube at a finer pitch.  The rule, pinned (fp32, each operation rounded on its own in the order written):
 *   lattice    sdfhip_instances_clash's, word for word: depth d in 0..10, origin[3] and side, pitch = side * 2^-d, lattice point
 *              (x, y, z) is p_a = fmaf((float)i_a + 0.5f, pitch, origin_a), its linear index (z << 2d) | (y << d) | x
 *   contains   sdfhip_instances_clash's, word for word: instance k contains p iff u_k(p) < 0; the ops are ignored
 *   r_k(p)     q = the placement's inverse map of p -- the first three lines of sdfhip_scene_place's value: d = p - t,
 *              q_a = ((R[0][a] d_0 + R[1][a] d_1) + R[2][a] d_2) * inv, inv = 1 / s, with NO clamp -- and
 *              r_k(p) = sqrtf(d2_k(q)) * s_k, where d2_k is sdfhip_scene_distance's d2 on instance k's source at full detail
 *              (level -1): the minimum of tri_dist2 over sdfhip_scene_mesh's triangles, a NaN never wins, an empty surface gives
 *              +inf.  r_k is unsigned: no sign function is involved, containment is the clash rule's
 *   depth      depth(a, b) = the maximum of fminf(r_a(p), r_b(p)) over the lattice points both contain: the radius of the largest ball,
 *              centred on a shared lattice point, that stays inside both parts
 *   witness    the lowest linear index attaining depth(a, b)
 *   record     one 64-byte sdfhip_penetration for every pair a < b that shares at least one lattice point, in (a, b) order: points
 *              (equal to the clash record's), witness, depth, ra = r_a and rb = r_b at the witness (depth = fminf(ra, rb)), node_a /
 *              node_b = the cut cells holding the nearest triangles (as sdfhip_clearance.node), nearest_a / nearest_b = the nearest
 *              surface points of each part in world coordinates: the search's q - r (of the triangles that tie the lowest (node,
 *              tri) wins) mapped forward as ((R[i][0] x + R[i][1] y) + R[i][2] z) * s + t_i.  nearest_a - nearest_b is the translation
 *              of part b that separates the pair to first order, of length about ra + rb
 *   +inf       a depth (or ra, rb) of +inf means a part with no surface at all -- a full solid; that side's node and nearest are 0
 *   integers   the maximum with its lowest-index tie rule does not depend on order, and it is accumulated with integer atomics only:
 *              a 64-bit atomic max of the key (float bits << 32) | (0xFFFFFFFF - index) -- the values are >= 0 and never a NaN, so
 *              their bits are monotone -- and an integer atomic add for points.  Two calls give the same bytes
 * The exact skip (on by default) is sdfhip_instances_clash's; SDFHIP_PENETRATION_NO_SKIP looks every instance up at every point and
 * gives the same records.  opt: NULL = the defaults (depth 6, origin 0, side 1, the skip on); sdfhip_penetration_options_default sets
 * them and the size, and the struct has sdfhip_clash_options' layout and grows like it.  out receives the first min(capacity, total)
 * records and *n_pairs the total; out may be NULL with capacity 0 (count first, then fetch).  One instance is a success with 0 pairs.
 * stats (may be NULL): points, blocks, blocks_looked and lookups as sdfhip_clash_stats counts them; searches = the sum over the points
 * inside two or more parts of the number of parts containing them; visited = the node records those searches loaded (the searches
 * at the witnesses, two per record, are not counted) -- both are the same on every call; pass_ms = the device time of the count,
 * the bitmaps, the emit, the searches, the fold and the records, kernel_ms their sum, total_ms the whole call on the host.
 * Synchronous, on a stream of the call's own.  Every source is untouched and may be freed as soon as the call returns.
 * SDFHIP_ERR_ARG: what sdfhip_instances_clash refuses, word for word, and more than 2^32 - 1 searches (the message names the count and
 * says to narrow the box); SDFHIP_ERR_BAD_TREE: a source sdfhip_scene_mesh refuses, raised only when a search would run on it;
 * SDFHIP_ERR_NOMEM: out of device memory (nothing is written, nothing leaks); SDFHIP_ERR_DEVICE as elsewhere.  Device memory: 16 bytes
 * per search, 4 bytes per 32 nodes of each distinct searched source, 80 bytes per pair of the list.  Measured on an MI355X
 * (profiles/penetration_bench.json), 2 / 8 / 32 overlapping instances of a 28 M-node scene and a 39 k-node torus, on a
 * clash record's box at depths 5 and 6 (424 .. 10 306 searches): the call 3.9 .. 8.4 ms, of which the searches 1.6 .. 5.9 ms (the
 * latency of the slowest wave: eight times the searches cost 1.1 .. 1.4 x) and the large scene's bitmap 0.67 ms, against 22 .. 843 ms
 * for one sdfhip_scene_distance_device call per instance on all the box's points and the pairing of their values.
 * Out of scope: the gap between DISJOINT parts, which is sdfhip_instances_gap's (below), and lists of more than 64 instances
 * (DESIGN.md section 9). */
enum { SDFHIP_PENETRATION_NO_SKIP = 1 }; /* sdfhip_penetration_options.flags: look every instance up at every lattice point */
typedef struct sdfhip_penetration_options {
    uint32_t size, flags;           /* sizeof(sdfhip_penetration_options) of the caller's header; SDFHIP_PENETRATION_* */
    uint32_t depth;                 /* 0..10: 2^depth lattice points along each axis */
    float origin[3];                /* the cube's corner */
    float side;                     /* the cube's side: finite and above 0 */
} sdfhip_penetration_options;       /* 28 bytes */
typedef struct sdfhip_penetration { /* 64 bytes: one pair of instances that share lattice points */
    uint32_t a, b;                  /* a < b: indices in the list */
    uint32_t points;                /* >= 1: the lattice points inside both */
    uint32_t witness;               /* the lowest linear index attaining depth */
    float depth;                    /* the maximum over those points of fminf(r_a, r_b) */
    float ra, rb;                   /* r_a and r_b at the witness */
    uint32_t node_a, node_b;        /* the cut cells of the nearest triangles, in each part's source */
    float nearest_a[3];             /* part a's nearest surface point to the witness, world coordinates */
    float nearest_b[3];             /* part b's */
    uint32_t pad_;
} sdfhip_penetration;
typedef struct sdfhip_penetration_stats { /* 72 bytes */
    uint64_t points;                /* 8^depth */
    uint32_t blocks, blocks_looked; /* 4 x 4 x 4 blocks of the lattice; those that looked anything up */
    uint64_t lookups;               /* (point, instance) look-ups made, counted once */
    uint64_t searches;              /* (point, containing instance) searches at the points inside two or more parts */
    uint64_t visited;               /* node records those searches loaded */
    float kernel_ms, total_ms;      /* the kernels on the device; the whole call on the host */
    float pass_ms[6];               /* count, bitmaps, emit, searches, fold, records */
} sdfhip_penetration_stats;
SDFHIP_API void sdfhip_penetration_options_default(sdfhip_penetration_options *opt);
SDFHIP_API int sdfhip_instances_penetration(const sdfhip_instance *instances, uint32_t n_instances, const sdfhip_penetration_options *opt,
                                            sdfhip_penetration *out, uint32_t capacity, uint32_t *n_pairs, sdfhip_penetration_stats *stats);

/* ---- clearance: how far apart the parts of an assembly are that do not overlap, and where they are nearest --
 * Replaces: nothing in the reference's code.  sdfhip_instances_clash and sdfhip_instances_penetration answer for parts that overlap;
 * this call answers the question asked before two parts touch.  It takes the same list (1..SDFHIP_CLASH_MAX_INSTANCES instances, the
 * ops ignored) and returns one 64-byte record per pair a < b whose surfaces lie within `limit` of each other.  The rule, pinned (fp32,
 * each operation rounded on its own in the order written):
 *   surface    the surface of part k is the triangles sdfhip_scene_mesh emits for its source at full detail (level -1), in emitted
 *              order: node ascending, then triangle k of the cell, then vertex v of the triangle
 *   vertex     the world vertex of an emitted position (x, y, z) of part k is w_i = ((R[i][0] x + R[i][1] y) + R[i][2] z) * s + t_i, the
 *              forward map of sdfhip_penetration's nearest points
 *   r_k(w)     sdfhip_instances_penetration's r_k, word for word: q = the placement's inverse map of w with no clamp, and
 *              r_k(w) = sqrtf(d2_k(q)) * s_k with d2_k sdfhip_scene_distance's d2 on instance k's source at level -1
 *   candidates of pair (a, b): direction 0 is every vertex of a's triangles held against b, r_b(w); direction 1 every vertex of b's
 *              triangles held against a, r_a(w)
 *   gap        gap(a, b) = the minimum of r over all candidates.  A NaN never wins.  A pair whose minimum is +inf -- a part without
 *              a surface, values that overflow -- has no record.  A pair has a record iff gap <= limit
 *   witness    of the candidates attaining the minimum, the lowest (direction, node, 3 k + v)
 *   record     a, b, gap, flags; node_a / node_b = the cut cells that hold the two closest points: on the witness's side the vertex's
 *              cell, on the other side the cell of the nearest triangle (as sdfhip_clearance.node); corner = 3 k + v of the witness;
 *              point_a / point_b in world coordinates: on the witness's side the witness vertex w, on the other side the search's
 *              q - r (of the triangles that tie the lowest (node, tri) wins) mapped forward.  point_b - point_a is the bindings'
 *              gap_vector: the way from a to b across the gap.  Records come in (a, b) order
 *   flags      SDFHIP_GAP_WITNESS_OF_B (bit 0): the witness vertex belongs to b (direction 1).  SDFHIP_GAP_CONTAINED (bit 1): by
 *              sdfhip_instances_clash's `contains` rule the other part contains the witness vertex, or the witness's part contains
 *              the other side's point (two look-ups) -- the surfaces are nested or interpenetrating, and the gap is the distance
 *              between them INSIDE a part: run sdfhip_instances_clash
 *   integers   the minimum with its tie rule does not depend on order: a 64-bit integer atomic min of the key (float bits << 32) |
 *              (direction << 31 | node) -- the values are >= 0 and never a NaN, so their bits are monotone, and node indices fit 31
 *              bits because links are int32 -- from the start (bits(limit) << 32) | 0xFFFFFFFF; corner is resolved from the witness
 *              cell alone.  Two calls give the same records
 * What the value is.  This is the VERTEX-TO-SURFACE distance, both ways round: the closest approach of a vertex of one part's
 * triangles to the other part's triangles.  The edge-to-edge configuration -- two edges crossing at a distance with all four end
 * points farther away -- is not searched.  The value is therefore never below the distance between the two triangle sets, and it
 * exceeds that distance by at most half the shorter of the two edges involved, which is less than sqrt(3) / 2 * s * 2^-depth of the
 * finer cell (an edge of a cell's triangles lies inside the cell).
 * opt: NULL = the defaults (limit +inf, pruning on); sdfhip_gap_options_default sets them and the size, and the struct grows like
 * sdfhip_instances_options.  limit is in [0, +inf]; SDFHIP_GAP_NO_PRUNE runs every candidate of every pair with no bound and no broad
 * phase and gives the same records.  out receives the first min(capacity, total) records and *n_pairs the total; out may be NULL with
 * capacity 0 (count first, then fetch).  One instance is a success with 0 pairs.
 * How it runs.  Per distinct source the cut cells are listed once; the host drops a pair only when the parts' bounding spheres are
 * provably more than `limit` apart; one lane per (ordered pair, cut cell) searches from the cell's cut vertices into the other part,
 * each search starting from the pair's best gap so far (a box is pruned only when strictly farther, so ties at the bound are found).
 * stats (may be NULL): pairs = K (K - 1) / 2; pairs_searched = the pairs the broad phase kept, both of whose parts have a surface;
 * cells = the (ordered pair, cut cell) lanes; searches = the vertex searches those lanes ran and visited = the node records they
 * loaded -- BOTH DEPEND ON THE ORDER IN WHICH WAVES TIGHTEN THE BOUND AND DIFFER FROM CALL TO CALL (the records do not); under
 * SDFHIP_GAP_NO_PRUNE they are fixed, and searches is the sum over the ordered pairs with two non-empty surfaces of 3 x the triangles
 * of the first part.  The searches of the record pass are not counted.  pass_ms = the device time of the cell lists (the host's two
 * waits included), the bitmaps, the searches and the records; kernel_ms their sum; total_ms the whole call on the host.
 * Synchronous, on a stream of the call's own.  Every source is untouched and may be freed as soon as the call returns.
 * SDFHIP_ERR_ARG: what sdfhip_instances_clash refuses of the list and of an instance, word for word, a size the growth rule refuses,
 * unknown flags, a limit that is a NaN or negative, more than 2^31 - 1 workgroups; SDFHIP_ERR_BAD_TREE: a source sdfhip_scene_mesh
 * refuses, raised only when a search would run on it or from it (the message names the instance): such a source has no box the
 * broad phase could trust, so every pair of it with two surfaces is kept whatever the limit, and the call refuses it; SDFHIP_ERR_NOMEM: out of device
 * memory (nothing is written, nothing leaks); SDFHIP_ERR_DEVICE as elsewhere.  Device memory: per distinct source 16 bytes per cut
 * cell, 4 bytes per 256 nodes and 4 bytes per 32 nodes; 8 bytes per workgroup of the work table; 72 bytes per pair of the list.
 * Out of scope: edge-to-edge exactness, a `level` option (coarser surfaces), a reject of whole cells from
 * their centre, and lists of more than 64 instances. */
enum { SDFHIP_GAP_NO_PRUNE = 1 };        /* sdfhip_gap_options.flags: every candidate of every pair, no bound, no broad phase */
enum { SDFHIP_GAP_WITNESS_OF_B = 1, SDFHIP_GAP_CONTAINED = 2 };      /* sdfhip_gap.flags */
typedef struct sdfhip_gap_options {
    uint32_t size, flags;           /* sizeof(sdfhip_gap_options) of the caller's header; SDFHIP_GAP_NO_PRUNE or 0 */
    float limit;                    /* [0, +inf]: only pairs with gap <= limit have a record */
} sdfhip_gap_options;               /* 12 bytes */
typedef struct sdfhip_gap {         /* 64 bytes: one pair of instances whose surfaces lie within the limit */
    uint32_t a, b;                  /* a < b: indices in the list */
    float gap;                      /* the minimum of r over the pair's candidates */
    uint32_t flags;                 /* SDFHIP_GAP_WITNESS_OF_B, SDFHIP_GAP_CONTAINED */
    uint32_t node_a, node_b;        /* the cut cells that hold the two closest points, in each part's source */
    uint32_t corner;                /* 3 k + v: the witness vertex within its cell's triangles */
    float point_a[3];               /* the closest point on part a, world coordinates */
    float point_b[3];               /* ... and on part b */
    uint32_t pad_[3];
} sdfhip_gap;
typedef struct sdfhip_gap_stats {   /* 56 bytes */
    uint32_t pairs, pairs_searched; /* K (K - 1) / 2; those the broad phase kept, both parts with a surface */
    uint64_t cells;                 /* (ordered pair, cut cell) lanes */
    uint64_t searches;              /* vertex searches run: differs from call to call unless SDFHIP_GAP_NO_PRUNE */
    uint64_t visited;               /* node records those searches loaded: likewise */
    float kernel_ms, total_ms;      /* the passes on the device; the whole call on the host */
    float pass_ms[4];               /* cell lists, bitmaps, searches, records */
} sdfhip_gap_stats;
SDFHIP_API void sdfhip_gap_options_default(sdfhip_gap_options *opt);
SDFHIP_API int sdfhip_instances_gap(const sdfhip_instance *instances, uint32_t n_instances, const sdfhip_gap_options *opt, sdfhip_gap *out,
                                    uint32_t capacity, uint32_t *n_pairs, sdfhip_gap_stats *stats);

/* ---- components: the separate solids and enclosed voids of a scene, in one call ----------------------------
 * Replaces: nothing in the reference's code.  The questions of whoever has just carved, subtracted, offset, shelled or scanned: did
 * the part fall in two, are there floating crumbs, is the cavity sealed, how many bodies are there?  sdfhip_scene_components labels
 * the face-connected components of a resident scene on a cubic lattice, both phases at once; it builds no tree and keeps nothing on
 * the handle.  The rule, pinned (fp32, each operation rounded on its own in the order written):
 *   lattice    sdfhip_instances_clash's, word for word -- depth d, origin[3] and side (> 0, finite) give a cube, pitch = side * 2^-d,
 *              lattice point (x, y, z), 0 <= x, y, z < 2^d, is p_a = fmaf((float)i_a + 0.5f, pitch, origin_a), its linear index is
 *              (z << 2d) | (y << d) | x -- but d is 0..9, not 0..10: this call keeps 4 bytes per point, 512 MB at depth 9 and 4 GB at
 *              depth 10 (the refusal says so)
 *   inside     a point is inside iff value(p) < 0; a NaN is outside.  value is sdfhip_scene_place's at the identity, what
 *              sdfhip_scene_volume writes: qc_a = fminf(fmaxf(p_a, 0), 1), e = p - qc, D = the distance sdfhip_scene_sample returns
 *              at qc, value = D + sqrtf((e0 * e0 + e1 * e1) + e2 * e2)
 *   connected  two lattice points are connected iff they differ by 1 in exactly one coordinate (6-connectivity) and are both inside
 *              or both outside.  The components of the inside phase are solids, those of the outside phase voids
 *   label      the label of a point is the lowest linear index in its component: labels[label] == label, and the labels are the same
 *              on every call, whatever the waves' timing
 *   record     one 64-byte sdfhip_component per component, in ascending label order: flags = SDFHIP_COMPONENT_SOLID for a solid, 0 for
 *              a void; points; lo[3] / hi[3] the inclusive lattice bounds; sum[3] the sums of x, y and z.  So a component's volume is
 *              points * pitch^3, its centroid origin + (sum / points + 0.5) * pitch, and it is enclosed iff no lo[a] == 0 and no
 *              hi[a] == 2^d - 1: a sealed cavity is a void that is enclosed, a floating piece any solid beyond the first
 *   integers   everything in a record is an integer, accumulated with integer atomic add / min / max only: the bytes are the same on
 *              every call
 * Cell centres only: a wall or a gap thinner than the pitch may vanish, merge two pieces or open a cavity; ask again at a finer depth.
 * opt: NULL = the defaults (depth 6, origin 0, side 1); sdfhip_components_options_default sets them and the size, and the struct grows
 * like sdfhip_clash_options.  out receives the first min(capacity, total) records and *n_components the total (>= 1); out may be NULL
 * with capacity 0 (count first, then fetch).  labels (may be NULL): 8^d words in linear-index order, in host memory; the _device form
 * takes memory of the scene's device instead and is otherwise the same call (out and stats stay in host memory).  stats (may be
 * NULL): points = 8^d, inside = the points of the solids, components, solids, the kernels' time and the call's.
 * Both forms are synchronous, on a stream of the call's own.  The scene is read under its lock, is untouched and may be freed as
 * soon as the call returns.  SDFHIP_ERR_ARG, before any device call: a null scene, a null n_components, a null out with capacity > 0,
 * a size the growth rule refuses, non-zero flags, depth above 9, a non-finite origin, a side that is not finite or is <= 0 (or
 * overflows origin + side); SDFHIP_ERR_NOMEM: out of device memory (nothing is written, nothing leaks); SDFHIP_ERR_DEVICE as
 * elsewhere.  Device memory: 4 bytes per point, 8 bytes per 4 x 4 x 4 block, a quarter of a byte per point for the roots' ranks, and
 * 64 bytes per component.  Measured on an MI355X (profiles/components_bench.json), a 28 M-node scene on the unit cube
 * at depth 7 / 8 / 9 (2.1 M / 16.8 M / 134 M points): the call 1.46 / 2.80 / 7.05 ms, of which the kernels 0.56 / 1.37 / 5.40 ms; with
 * labels into device memory 1.20 / 2.90 / 7.47 ms, copied to pageable host memory 1.38 / 9.48 / 61.8 ms; against 4.97 / 53.9 / 737 ms
 * for sdfhip_scene_volume_device on the same centres plus min-label propagation in torch on the device. */
enum { SDFHIP_COMPONENT_SOLID = 1 };     /* sdfhip_component.flags: a component of the inside phase */
enum { SDFHIP_COMPONENTS_MAX_DEPTH = 9 };
typedef struct sdfhip_components_options {
    uint32_t size, flags;           /* sizeof(sdfhip_components_options) of the caller's header; must be 0 */
    uint32_t depth;                 /* 0..9: 2^depth lattice points along each axis */
    float origin[3];                /* the cube's corner */
    float side;                     /* the cube's side: finite and above 0 */
} sdfhip_components_options;        /* 28 bytes */
typedef struct sdfhip_component {   /* 64 bytes: one face-connected component */
    uint32_t label;                 /* the lowest linear index of the component: the value its points carry in labels[] */
    uint32_t flags;                 /* SDFHIP_COMPONENT_SOLID = 1: the inside phase; 0: a void */
    uint32_t points;                /* >= 1 */
    uint32_t reserved;              /* 0 */
    uint32_t lo[3], hi[3];          /* inclusive lattice bounds, {x, y, z} */
    uint64_t sum[3];                /* the sums of x, y and z */
} sdfhip_component;
typedef struct sdfhip_components_stats { /* 32 bytes */
    uint64_t points;                /* 8^depth */
    uint64_t inside;                /* the lattice points with value < 0 */
    uint32_t components, solids;    /* the records; those with SDFHIP_COMPONENT_SOLID */
    float kernel_ms, total_ms;      /* the kernels on the device; the whole call on the host */
} sdfhip_components_stats;
SDFHIP_API void sdfhip_components_options_default(sdfhip_components_options *opt);
SDFHIP_API int sdfhip_scene_components(sdfhip_scene *scene, const sdfhip_components_options *opt, sdfhip_component *out, uint32_t capacity,
                                       uint32_t *n_components, uint32_t *labels, sdfhip_components_stats *stats);
SDFHIP_API int sdfhip_scene_components_device(sdfhip_scene *scene, const sdfhip_components_options *opt, sdfhip_component *out,
                                              uint32_t capacity, uint32_t *n_components, uint32_t *d_labels,
                                              sdfhip_components_stats *stats);

/* ---- selection: keep, drop or fill a scene's components as a new scene --------------------------------------
 * Replaces: nothing in the reference's code.  What to do with sdfhip_scene_components' answer: remove the crumbs a carve or a negative
 * offset left behind, fill a sealed cavity before printing, keep the largest body of a scan, pull one body of a combination out as a
 * scene of its own.  sdfhip_scene_select labels the scene as sdfhip_scene_components does, decides for every component whether its
 * phase FLIPS (a solid becomes empty space, a void becomes solid), and resamples the scene into a NEW handle `*out` on the same
 * device in which the flipped components have the other phase.  The source is read under its lock, stays untouched and may be freed
 * as soon as the call returns.  The rule, pinned (fp32, each operation rounded on its own in the order written):
 *   labelling  the lattice of opt (lattice_depth d, origin, side: sdfhip_components_options' cube, pitch = side * 2^-d) is labelled
 *              exactly as sdfhip_scene_components labels it.  phase[i]: lattice point i is inside.  F[i]: i's component flips -- it
 *              does if ANY rule bit of opt->flags flips it:
 *                KEEP_LARGEST_SOLID   every solid but the one with most points (tie: the lowest label)
 *                DROP_SMALL_SOLIDS    every solid with points < min_points
 *                FILL_ENCLOSED_VOIDS  every void that is enclosed (no lo[a] == 0, no hi[a] == 2^d - 1)
 *                FLIP_LISTED          the listed components, solid or void
 *                KEEP_LISTED          every solid that is NOT listed
 *              T[i] = phase[i] XOR F[i] is i's target phase
 *   value      at a point p of the result's tree, v = sdfhip_scene_place's value at the identity (sdfhip_scene_components' value)
 *   N(p)       per axis a: g = (p_a - origin_a) / pitch - 0.5f; f = floorf(g); the candidates are {f} if g == f, else {f, f + 1},
 *              each clamped into 0 .. 2^d - 1 in float (fminf(fmaxf(., 0), 2^d - 1)) before it becomes an integer.  N(p) is the
 *              product of the three sets: the lattice points with non-zero trilinear weight at p, 1 to 8 of them
 *   classes    any: some point of N(p) has F; allin: every point of N(p) has T; allout: none has T
 *   result     v' = -fmaxf(fabsf(v), h) if any && allin; v' = fmaxf(fabsf(v), h) if any && allout; v' = v otherwise.  h = 2^-8, a
 *              constant: FromFloat(h, S) >= 64 for every S <= 1 while the surface sits at byte 63.75, so no corner of a zone that has
 *              become empty reads as inside (with plain |v| every corner within 0.002 S of the former surface would be a speck); a
 *              larger h would move kept surfaces that pass within a pitch of a removed piece
 *   tree       sdfhip_scene_place's construct rule and node order on v': byte = FromFloat(v', S), a node splits iff
 *              fabsf(v'(centre)) < 2 * S && d < depth; breadth first
 * What the rule implies.  With no rule bit, or none that flips anything, v' = v everywhere: the result is sdfhip_scene_place at the
 * identity, byte for byte.  At a result depth of at most 9 the links always equal the identity placement's: max(|v|, h) < 2 S iff
 * |v| < 2 S while h < 2 S, which holds on levels 0..8, so only the bytes of nodes with a corner in a changed zone differ -- the removed
 * piece's former surface stays resolved as ghost structure, and the distance bytes there are lower bounds, not distances:
 * sdfhip_scene_offset by 0 re-distances the result and rebuilds the tree round the surviving surface alone.  Near-contacts: where a
 * flipped piece lies within one pitch of a kept one of the same phase, N(p) is mixed and the point is left as it was; ask again on a
 * finer lattice.  Cell centres only: features thinner than the pitch are not seen, as in sdfhip_scene_components.
 * opt: NULL = the defaults (no rule); sdfhip_select_options_default sets them and the size, and the struct grows like
 * sdfhip_components_options.  depth: the result's deepest level, -1 = the source's, else 0..12, as sdfhip_placement.depth.  labels /
 * n_labels: the list of FLIP_LISTED or KEEP_LISTED -- component labels as sdfhip_scene_components returns them on the same lattice,
 * in host memory, in any order, repeats allowed.  out, host_out: either may be NULL, not both, as sdfhip_scene_place's; on any
 * failure *out is left as it was.  stats (may be NULL): the lattice's side -- components, solids, flipped_solids, flipped_voids,
 * points_flipped (the lattice points of the flipped components) -- the tree's side as sdfhip_place_stats has it, and the times.
 * SDFHIP_ERR_ARG before any device call: a null scene, both outputs NULL, a size the growth rule refuses, unknown flag bits, both
 * FLIP_LISTED and KEEP_LISTED, a listed rule with n_labels == 0 or labels NULL, labels given without a listed rule, lattice_depth above
 * 9, a non-finite origin, a side that is not finite or is <= 0 (or overflows origin + side), depth outside -1..12.  SDFHIP_ERR_ARG
 * after the labelling pass, with nothing built and the label named in the message: a listed label that is not the label of a
 * component (label >= 8^d or labels[label] != label), a void listed under KEEP_LISTED.  SDFHIP_ERR_BAD_TREE: depth -1 on a source that
 * has no depth to give, as sdfhip_scene_place; SDFHIP_ERR_NOMEM, SDFHIP_ERR_DEVICE as elsewhere.  Device memory: the labelling's (4
 * bytes per lattice point and the rest, freed before the tree is built), two bits per lattice point for F and T, then the
 * placement's. */
enum { SDFHIP_SELECT_KEEP_LARGEST_SOLID = 1,   /* flip every solid but the one with most points (tie: the lowest label) */
       SDFHIP_SELECT_DROP_SMALL_SOLIDS  = 2,   /* flip every solid with points < min_points */
       SDFHIP_SELECT_FILL_ENCLOSED_VOIDS = 4,  /* flip every void that is enclosed (no lo == 0, no hi == 2^d - 1) */
       SDFHIP_SELECT_FLIP_LISTED = 8,          /* flip the listed components, solid or void */
       SDFHIP_SELECT_KEEP_LISTED = 16 };       /* flip every solid that is NOT listed (a listed void: SDFHIP_ERR_ARG) */
typedef struct sdfhip_select_options {
    uint32_t size, flags;           /* sizeof(sdfhip_select_options) of the caller's header; rule bits, OR-ed: a component flips if any rule flips it */
    uint32_t lattice_depth;         /* 0..9, the components' lattice */
    float origin[3], side;          /* as sdfhip_components_options */
    int32_t depth;                  /* the result's depth: -1 = the source's, else 0..12 (as sdfhip_placement.depth) */
    uint32_t min_points;            /* DROP_SMALL_SOLIDS' threshold */
} sdfhip_select_options;            /* 36 bytes */
typedef struct sdfhip_select_stats { /* 64 bytes */
    uint32_t components, solids;    /* the lattice's records; the solids among them */
    uint32_t flipped_solids, flipped_voids;
    uint64_t points_flipped;        /* the lattice points of the flipped components */
    uint32_t nodes_in, nodes_out, depth_out, levels;    /* as sdfhip_place_stats */
    uint64_t samples;               /* source look-ups made by the tree's levels: 9 for the root, 35 for every block of eight siblings */
    float label_ms;                 /* HIP events around the labelling, the decision and the bitmaps */
    float kernel_ms;                /* HIP events around the levels' kernels (the per-level host synchronisations included) */
    float scene_ms, total_ms;       /* building the new handle; the whole call, host clock */
} sdfhip_select_stats;
SDFHIP_API void sdfhip_select_options_default(sdfhip_select_options *opt);   /* size, lattice depth 6, unit cube, depth -1, no rule */
SDFHIP_API int sdfhip_scene_select(sdfhip_scene *scene, const sdfhip_select_options *opt, const uint32_t *labels, uint32_t n_labels,
                                   sdfhip_scene **out, sdfhip_octdata *host_out, sdfhip_select_stats *stats);

/* ---- surface extraction: a resident scene as triangles ------------------------------------------------
 * Replaces: nothing in the reference's code -- its tree only ever becomes pixels.  A scene that was built, carved and picked here
 * leaves as geometry: a triangle soup of 3 * n_triangles vertices of six floats {position, normal}, the layout of sdfhip_points.data,
 * so a mesh goes straight back into sdfhip_sdfgen[_scene] and through sdfhip_load_ply / sdfhip_load_obj.  No index buffer.
 * The rule, pinned (fp32, each operation rounded in the order written; DESIGN.md section 8 has it in full):
 *   sign       a corner byte b decodes as (b/255 - 0.25) * 2S: the surface is at b = 63.75; inside <=> b <= 63
 *   cells      level -1: the leaves; level L = 0..12: the leaves of depth <= L and the internal nodes of depth exactly L with their own
 *              eight bytes (a level-of-detail mesh).  A cell emits triangles only if its bytes are mixed (min <= 63 < max).  Its integer
 *              coordinates c of its depth d (edge S = 2^-d) come from the links: octant within the parent = index - parent.children
 *   triangles  marching tetrahedra on the Kuhn decomposition: six tetrahedra {0, 1<<a0, 1<<a0 | 1<<a1, 7} round the diagonal 0-7, one
 *              per axis permutation (a0, a1, a2) in lexicographic order.  Cut edges are pairs of local corners (i, j), i < j.  One or
 *              three inside corners: one triangle of the three cut edges in ascending order; two inside i0 < i1 and two outside
 *              o0 < o1: the quad (i0,o0) (i0,o1) (i1,o1) (i1,o0) as triangles (q0,q1,q2) (q0,q2,q3).  Every triangle is counter-clockwise
 *              seen from outside (the last two vertices swapped where the unit tetrahedron with cuts at the edge midpoints asks for it)
 *   vertex     on the edge from cube corner lo to hi: t = (63.75f - (float)b_lo) / ((float)b_hi - (float)b_lo), and per axis a
 *              p_a = ((float)(c_a + bit_a(lo)) + (bit_a(hi) != bit_a(lo) ? t : 0.0f)) * S -- equal-depth neighbours with equal bytes
 *              on a shared edge produce the same bits
 *   normal     gradient() (Compute.hlsl:112-130) at that position with the cursor on the cell, times 1 / sqrt(dot(g, g)) as
 *              sdfhip_hit.normal; a zero gradient gives NaN, as there
 *   order      cells in ascending node index, tetrahedra and triangles as above: the bytes never depend on which wave finished first
 * Cells of different depth meet in T-junctions (no crack patching); nothing is welded, clipped or simplified.
 *   sdfhip_scene_mesh          the mesh in host memory (release with sdfhip_mesh_free), synchronous, on the scene's own stream
 *   sdfhip_scene_mesh_device   ALWAYS returns the count the scene needs in *n_triangles (one host synchronisation on `stream`); writes
 *                              the vertices to d_verts6 (device memory on the scene's device) only if the count fits
 *                              capacity_triangles -- capacity 0 with a null pointer asks for the count -- asynchronously on `stream`
 *                              (NULL = the HIP default stream): sdfhip_render_device's convention.  Runs beside frames that are
 *                              already enqueued on other streams; the call holds the handle's lock while it waits for the count, so
 *                              another host thread's call on the same scene (a render, a query, a mesh) waits for that round trip
 *   sdfhip_mesh_save_ply       binary little-endian, the vertex element first (x y z nx ny nz floats), then faces as uchar / int lists
 *                              (3i, 3i+1, 3i+2): sdfhip_load_ply reads the vertices back bit for bit
 *   sdfhip_mesh_save_obj       `v` / `vn` lines with %.9g, then `f a//a b//b c//c`: sdfhip_load_obj gives the same vertices back
 * opt: NULL = defaults (level -1); the struct grows like sdfhip_upload_options (size set by sdfhip_mesh_options_default; a larger,
 * newer struct is accepted when the fields this library does not know are all -1).
 * SDFHIP_ERR_ARG: a null scene or output, level outside -1..12, an options struct the size rules refuse, a capacity without a buffer, a
 * result of more than 2^31 - 1 triangles; SDFHIP_ERR_BAD_TREE: the tree is not consistent (stack_kernel_ok == 0 in sdfhip_scene_info), as
 * sdfhip_scene_edit refuses it; SDFHIP_ERR_NOMEM: out of device or host memory (nothing leaks, the scene is untouched).  A scene that
 * cuts nowhere is a success with zero triangles (verts6 NULL). */
typedef struct sdfhip_mesh_options { uint32_t size; int32_t level; } sdfhip_mesh_options;
typedef struct sdfhip_mesh { uint32_t n_triangles; float *verts6; } sdfhip_mesh;      /* 3 * n_triangles x 6 floats */
typedef struct sdfhip_mesh_stats {
    uint32_t nodes, cells, cells_cut, n_triangles;   /* cells: the cell set of the level; cells_cut: those with mixed bytes */
    float kernel_ms;                                 /* HIP events around the count, scan and emit kernels */
    float total_ms;                                  /* host clock, the whole call */
} sdfhip_mesh_stats;
SDFHIP_API void sdfhip_mesh_options_default(sdfhip_mesh_options *opt);
SDFHIP_API int sdfhip_scene_mesh(sdfhip_scene *scene, const sdfhip_mesh_options *opt, sdfhip_mesh *out, sdfhip_mesh_stats *stats);
SDFHIP_API int sdfhip_scene_mesh_device(sdfhip_scene *scene, const sdfhip_mesh_options *opt, float *d_verts6, uint32_t capacity_triangles,
                                        uint32_t *n_triangles, void *stream);
SDFHIP_API void sdfhip_mesh_free(sdfhip_mesh *mesh);
SDFHIP_API int sdfhip_mesh_save_ply(const sdfhip_mesh *mesh, const char *path);
SDFHIP_API int sdfhip_mesh_save_obj(const sdfhip_mesh *mesh, const char *path);

/* ---- the measure: volume, area, moments and bounds of a resident scene --------------------------------
 * Replaces: nothing in the reference's code -- its tree only ever becomes pixels, and no call there says anything quantitative about
 * the solid it describes.  sdfhip_scene_measure returns the volume, the surface area, the first and second moments about the origin
 * and the tight bounding box of the solid that N7's mesh bounds (marching tetrahedra on the Kuhn decomposition, the surface at byte
 * 63.75): what a placement fits from (sdfbox_amd.placement_fit), what an edit, a combination or a prune at a tolerance changed, and
 * the mass properties (centroid = moment1 / volume; inertia by the parallel-axis theorem) of a simulation's body at unit density.
 * It measures the solid the BYTES describe and the renderer draws, not the shape the builder was given: inside bytes saturate at -0.5
 * of a leaf's edge, which pulls the interpolated surface inward -- the depth-4 sphere of radius 0.3 (tests/golden/sphere_d4.asdf)
 * measures 0.10884054856 against the ball's 0.11309734, 3.76 % short, its mesh's vertices at radii 0.277 .. 0.3008.
 * The rule, pinned (fp64, each operation rounded on its own in the order written; DESIGN.md section 8 has it with the GPU path):
 *   cells      N7's: level -1 the leaves, level L the leaves of depth <= L and the internal nodes of depth exactly L; a corner is inside
 *              iff its byte <= 63; integer coordinates c of the cell's depth d from the links; S = 2^-d; cube corner k lies at
 *              ((double)c_a + bit_a(k)) * S.  A cell with no inside corner contributes +0.0 to every sum and nothing to the bounds
 *   cut point  on a tetrahedron's edge between local corners lo < hi (cube corners whose bits nest): t = (63.75 - b_lo) / (b_hi - b_lo),
 *              per axis ((double)(c_a + bit_a(lo)) + (bit_a(hi) != bit_a(lo) ? t : 0.0)) * S -- N7's vertex in fp64
 *   full cell  all eight bytes <= 63: the box lo = c * S, hi = (c + 1) * S: V = (S*S)*S, mid_a = (lo_a + hi_a) * 0.5, m1_a = V * mid_a,
 *              m2_aa = V * (((lo_a*lo_a + lo_a*hi_a) + hi_a*hi_a) / 3.0), m2_ab = V * (mid_a * mid_b), area 0
 *   cut cell   mixed bytes: cell-local sums from +0.0 over N7's six tetrahedra in order, each with corners (0, v1, v2, 7), inside
 *              corners i0 < i1 < .. and outside corners o0 < o1 < .., P(i, o) the cut point of that edge:
 *                four inside   the tetrahedron itself
 *                one           (i0, P(i0,o0), P(i0,o1), P(i0,o2))
 *                three         the whole tetrahedron added, then (o0, P(i0,o0), P(i1,o0), P(i2,o0)) subtracted
 *                two           q0 = P(i0,o0), q1 = P(i0,o1), q2 = P(i1,o1), q3 = P(i1,o0): (i0,q0,q1,q2), (i0,q0,q3,q2), (i0,i1,q3,q2) -- the
 *                              prism between the triangles (i0,q0,q1) and (i1,q3,q2)
 *   tetrahedron (a, b, c, d): e1 = b-a, e2 = c-a, e3 = d-a; det = (e1x*(e2y*e3z - e2z*e3y) - e1y*(e2x*e3z - e2z*e3x)) + e1z*(e2x*e3y - e2y*e3x);
 *              V = fabs(det) / 6.0; s = ((a+b)+c)+d; volume += V; m1_a += (V*0.25) * s_a;
 *              m2_ij += (V*0.05) * ((((a_i*a_j + b_i*b_j) + c_i*c_j) + d_i*d_j) + s_i*s_j)   (subtracted: -= each)
 *   area       N7's triangles (p0, p1, p2) of that tetrahedron and mask, vertices in fp64 in the table's order: u = p1-p0, v = p2-p0,
 *              n = (uy*vz - uz*vy, uz*vx - ux*vz, ux*vy - uy*vx), n2 = (nx*nx + ny*ny) + nz*nz, area += 0.5 * (double)sqrtf((float)n2) --
 *              the root in fp32 on purpose (the one root N11 already holds equal to numpy on the GPU; 6e-8 relative per triangle
 *              against a discretisation error of 1e-3).  Each cell's own triangles, as the mesh: no crack patching
 *   bounds     minimum and maximum per axis over the box corners of full cells, the inside cube corners of cut cells and their cut
 *              points: exact, whatever the order.  +inf / -inf when the solid is empty
 *   sums       each of the eleven (volume, area, moment1[3], moment2[6]) is the adjacent-pair tree over NODE INDEX: x[i] = node i's
 *              contribution (+0.0 for a node that is no cell), padded with +0.0 to a power of two, x = x[0::2] + x[1::2] until one value
 *              is left -- the bits never depend on which wave finished first, and no double is added atomically.  They do depend on
 *              the node order: the same tree in another order agrees to rounding (1e-12 relative), not bit for bit
 * The call is synchronous, on the scene's own stream, under the handle's lock as sdfhip_scene_mesh; the scene is untouched and frames
 * enqueued on other streams run beside it.  opt: NULL = level -1; the struct grows like sdfhip_mesh_options.
 * SDFHIP_ERR_ARG: a null scene or output, level outside -1..12, an options struct the size rules refuse (all before any device call);
 * SDFHIP_ERR_BAD_TREE: the tree is not consistent (stack_kernel_ok == 0) or deeper than 12 levels; SDFHIP_ERR_NOMEM: out of device
 * memory (136 bytes per 1024 nodes; nothing leaks).  *out is zeroed on every failure. */
typedef struct sdfhip_measure_options { uint32_t size; int32_t level; } sdfhip_measure_options;   /* level: as sdfhip_mesh_options */
typedef struct sdfhip_measure {
    double volume, area;
    double moment1[3];                      /* integral of x, y, z over the solid */
    double moment2[6];                      /* integral of xx, yy, zz, xy, xz, yz, about the origin */
    double bounds_min[3], bounds_max[3];    /* tight box of the solid; +inf / -inf when it is empty */
    uint32_t nodes, depth;                  /* the scene's */
    uint32_t cells, cells_cut, cells_inside;/* the level's cells; those with mixed bytes; those with all eight bytes <= 63 */
    uint32_t cells_at_depth[13];            /* the level's cells by depth */
    float kernel_ms;                        /* HIP events around the kernels */
    float total_ms;                         /* host clock, the whole call */
} sdfhip_measure;
SDFHIP_API void sdfhip_measure_options_default(sdfhip_measure_options *opt);
SDFHIP_API int sdfhip_scene_measure(sdfhip_scene *scene, const sdfhip_measure_options *opt, sdfhip_measure *out);

/* ---- cross-sections: the contours of a stack of planes ------------------------------------------------
 * Replaces: nothing that runs in the reference -- its tree only ever becomes pixels (its Layers.hlsl, a z-slice viewer, is dead code).
 * The outline of the solid in a plane, or in a stack of parallel planes: what a printer's slicer consumes after sdfhip_scene_offset, what
 * a section view draws and what a fit check between two parts looks at.  The slice is exactly plane x (the triangles of
 * sdfhip_scene_mesh), made on the device without a triangle ever being written: directed segments of 32 bytes, consistent with
 * sdfhip_scene_mesh and sdfhip_scene_measure by construction.
 * The rule, pinned (fp32, each operation rounded on its own in the order written; DESIGN.md section 8 has it with the GPU path):
 *   triangles  N7's, untouched: the cells of `level`, the six tetrahedra, the table's triangles (p0, p1, p2), counter-clockwise seen from
 *              outside, their vertices sdfhip_scene_mesh's positions
 *   height     d_i = ((nx * p_ix) + (ny * p_iy)) + (nz * p_iz) and h_k = offset + (float)k * pitch, k = 0 .. layers - 1 (layers = 1: h_0 =
 *              offset, whatever the pitch).  The normal is used as given, never normalised: h is in the units of dot(normal, p)
 *   side       vertex i is above plane k iff d_i >= h_k (these two floats compared, nothing subtracted).  A triangle gives one segment for
 *              plane k iff its three vertices are not all on one side; a triangle lying in the plane gives none
 *   point      on a triangle edge whose ends differ in side, ALWAYS from the below end a to the above end b, whichever way the triangle
 *              walks it: sa = d_a - h_k, sb = d_b - h_k, t = sa / (sa - sb), per axis q = a + (b - a) * t -- two triangles that share an
 *              edge with the same vertex bits produce the same three words, which is what closed contours rest on
 *   direction  of the triangle's edges 0->1, 1->2, 2->0 exactly one goes above->below and one below->above: segment.a is the point on the
 *              former, segment.b the point on the latter.  The solid lies on the left seen from the tip of the normal: outer loops are
 *              counter-clockwise and holes clockwise in any right-handed basis (u, v, normal)
 *   zero length  segments are emitted as they fall (a plane through a mesh vertex gives them); they disturb no point's balance
 *   order      ascending node index, then tetrahedron, then triangle, then layer k ascending; each record carries its layer and its node.
 *              layer_counts[k] is the number of records of layer k.  Grouping by layer is a stable sort on `layer`, left to the caller
 * Cells of different depth meet in T-junctions as in the mesh; nothing is welded, patched or chained into loops.
 *   sdfhip_scene_slice         the records (node-major) and the layers' counts in host memory (release with sdfhip_slice_free),
 *                              synchronous, on the scene's own stream, under the handle's lock.  layer_counts holds `layers` words on every
 *                              success; segments is NULL when there is no record
 *   sdfhip_scene_slice_device  ALWAYS returns the count in *n_segments (one host synchronisation on `stream`); writes the records to
 *                              d_segments (device memory on the scene's device, 16-byte aligned) only if the count fits
 *                              capacity_segments -- capacity 0 with a null pointer asks for the count -- asynchronously on `stream` (NULL =
 *                              the HIP default stream), node-major.  d_layer_counts (layers words of device memory, or NULL) is written
 *                              whether or not the records fit
 * opt: NULL = the defaults below; the struct grows like sdfhip_mesh_options.  stats may be NULL.
 * SDFHIP_ERR_ARG: a null scene, output or count; level outside -1..12; a normal that is not finite or all zero; an offset that is not
 * finite; layers 0 or above 65 536; a pitch that is not finite, or not > 0 when layers > 1; an options struct the size rules refuse; a
 * capacity without a buffer, a buffer that is not 16-byte aligned; a result of more than 2^31 - 1 segments.  SDFHIP_ERR_BAD_TREE and
 * SDFHIP_ERR_NOMEM as sdfhip_scene_mesh (nothing leaks, the scene is untouched).  *out is zeroed on every failure. */
typedef struct sdfhip_slice_options {
    uint32_t size; int32_t level;      /* size: set by sdfhip_slice_options_default; level: as sdfhip_mesh_options */
    float normal[3]; float offset;     /* plane k: dot(normal, p) = h_k */
    float pitch; uint32_t layers;      /* h_k = offset + (float)k * pitch, k = 0 .. layers-1 */
} sdfhip_slice_options;
typedef struct sdfhip_segment { float a[3]; uint32_t layer; float b[3]; uint32_t node; } sdfhip_segment;   /* 32 bytes */
typedef struct sdfhip_slice { uint32_t n_segments; sdfhip_segment *segments; uint32_t layers; uint32_t *layer_counts; } sdfhip_slice;
typedef struct sdfhip_slice_stats {
    uint32_t nodes, cells, cells_cut;  /* as sdfhip_mesh_stats */
    uint32_t cells_crossed;            /* the cut cells that emit at least one segment */
    uint32_t n_segments;
    float kernel_ms;                   /* HIP events around the count, scan and emit kernels */
    float total_ms;                    /* host clock, the whole call */
} sdfhip_slice_stats;
SDFHIP_API void sdfhip_slice_options_default(sdfhip_slice_options *opt);          /* level -1, normal (0,0,1), offset 0.5, pitch 0, layers 1 */
SDFHIP_API int sdfhip_scene_slice(sdfhip_scene *scene, const sdfhip_slice_options *opt, sdfhip_slice *out, sdfhip_slice_stats *stats);
SDFHIP_API int sdfhip_scene_slice_device(sdfhip_scene *scene, const sdfhip_slice_options *opt, sdfhip_segment *d_segments, uint32_t capacity_segments,
                                         uint32_t *d_layer_counts, uint32_t *n_segments, void *stream);
SDFHIP_API void sdfhip_slice_free(sdfhip_slice *slice);

/* ---- exact distance: clearance query, offset and shell ------------------------------------------------
 * Replaces: nothing in the reference's code -- its field is only ever read as stored, and the stored field is a distance only in a
 * thin band round the surface: a leaf of edge S holds values in [-0.5 S, 1.5 S] and every leaf away from the surface is saturated (the
 * notes at sdfhip_scene_place and sdfhip_scene_measure).  sdfhip_scene_sample therefore cannot say how far a point is from the model
 * beyond one leaf edge, and a scene could not be grown, shrunk or hollowed.  These calls compute the exact distance from a point to
 * the surface the scene describes, at any range, and build two modelling operations on it.  The rule, pinned (fp32, each operation
 * rounded on its own in the order written; S = 2^-d the edge of a cell of depth d):
 *   surface(scene, level)  the triangles sdfhip_scene_mesh emits for `level` (-1 = full detail, else as sdfhip_mesh_options): each the
 *                    three emitted positions a, b, c in emitted order.  Normals play no part
 *   d2(p)            best = +inf; for every triangle t = D(a, b, c, p), sdfhip_trimesh_build's squared distance below (it reads the
 *                    nine position floats only), then best = t < best ? t : best -- a NaN from a degenerate triangle never wins.  The
 *                    minimum of a set of floats does not depend on the order: d2 depends on the scene's arrays and p alone, never on
 *                    the traversal or on which wave finished first.  An empty surface gives +inf
 *   sign(p)          negative iff the distance sdfhip_scene_sample returns at pc = min(max(p, 0), 1) per axis (fmaxf / fminf, as the
 *                    placement clamps) is < 0.0f: find from the root and interpol_world, untouched.  The trilinear zero set of that
 *                    distance and the tetrahedra-linear surface the triangles bound differ by a sliver next to the surface; a point
 *                    inside the sliver gets the other sign, and since sqrtf(d2) there is no larger than the sliver is wide, dist is
 *                    off by at most twice that width (a fraction of the cell's edge), and only there
 *   dist(p)          sign(p) * sqrtf(d2(p))
 *   value(p)         SDFHIP_OFFSET_GROW: dist(p) - amount (amount > 0 grows the solid, < 0 shrinks it);
 *                    SDFHIP_OFFSET_SHELL: fabsf(dist(p)) - amount * 0.5f (amount > 0: the wall of that thickness centred on the surface)
 *   tree             sdfhip_scene_place's, word for word, with this value: byte = FromFloat(value, S); a node splits iff
 *                    fabsf(value(centre)) < 2 * S && d < depth; breadth-first node order; every point evaluated as if alone.  An empty
 *                    surface (value +-inf) gives the root alone.  Nothing is pruned: chain sdfhip_scene_prune
 * sdfhip_scene_distance answers n points (xyz: n x 3 floats, packed) with n sdfhip_clearance records; the _device form takes device
 * pointers, launches on the caller's stream and returns, as sdfhip_scene_sample_device.  A non-finite coordinate gets
 * SDFHIP_QUERY_INVALID and zeros, and the rest of the batch is answered.  Of the triangles that tie on d2 the one lowest in the mesh's
 * emitted order gives `node` and `nearest`; when d2 is +inf (an empty surface, or a point so far away that every squared distance
 * overflows) both are zero.  `visited` counts the records the search loaded: it depends on the point and the scene alone, and is the
 * same on every call.  level: -1, or 0..12.
 * sdfhip_scene_offset builds the tree of value(p) as a NEW handle `*out` on the same device: the input is untouched (frames in flight
 * on it included), either handle may be freed first, and the handle's lock is held only while its description is read.  opt: the
 * caller sets size = sizeof(sdfhip_offset_options); the struct grows like sdfhip_prune_options (a larger, newer struct is accepted when
 * the fields this library does not know are all -1).  depth: -1 = the source's depth, else 0..12; level: the source surface's level.
 * out, host_out: either may be NULL, not both; host_out: the result's host arrays (release with sdfhip_octdata_free).  stats (may be
 * NULL): points counts the evaluated points (9 for the root, 35 for every block of eight siblings), visited the records their
 * searches loaded.
 * SDFHIP_ERR_ARG: a null scene, options or point / record pointer (n > 0), both outputs NULL, a size the growth rule refuses, a
 * non-finite amount, a shell's thickness <= 0, an unknown mode, depth or level outside -1..12 -- each before any device call -- and a
 * result of more than 2^31 - 1 nodes; SDFHIP_ERR_BAD_TREE: a source sdfhip_scene_mesh refuses (not consistent, or deeper than 12
 * levels); SDFHIP_ERR_NOMEM: out of device memory (the input stays valid, nothing leaks).
 * The search (csrc/distance_kernels.h) is depth first from the root with the children of a node nearest first, skips a subtree that
 * holds no cut cell (a bitmap over the nodes, rebuilt per call: 4 bytes per 32 nodes) or whose box cannot hold anything nearer than the
 * best so far -- on a margin derived there for the rounding of the bound and of D, but for one case of D's face branch that DESIGN.md
 * N13 names -- and recomputes a cut cell's triangles with the mesh's own arithmetic.  Work per point grows with the number of
 * cells about as near as the nearest one. */
enum { SDFHIP_OFFSET_GROW = 0, SDFHIP_OFFSET_SHELL = 1 };
typedef struct sdfhip_clearance {   /* 32 bytes: the answer for one point */
    float distance;                 /* dist(p): signed, not saturated */
    uint32_t node;                  /* the cut cell that holds the nearest triangle */
    float nearest[3];               /* the closest point q on that triangle: p - r of D */
    uint32_t status;                /* SDFHIP_QUERY_HIT or SDFHIP_QUERY_INVALID; HIT with distance +-inf: an empty surface */
    uint32_t visited;               /* records the search loaded: the work measure */
    uint32_t pad_;
} sdfhip_clearance;
typedef struct sdfhip_offset_options {
    uint32_t size;            /* sizeof(sdfhip_offset_options) of the caller's header */
    int32_t mode;             /* SDFHIP_OFFSET_GROW or SDFHIP_OFFSET_SHELL */
    float amount;             /* GROW: delta; SHELL: the thickness, > 0 */
    int32_t depth;            /* -1 = the source's depth; else 0..12 */
    int32_t level;            /* the source surface's level: -1 = full detail; else 0..12 */
} sdfhip_offset_options;      /* 20 bytes */
typedef struct sdfhip_offset_stats {
    uint32_t nodes_in, nodes_out, depth_out, levels;
    uint64_t points;         /* points evaluated */
    uint64_t visited;        /* records their searches loaded */
    float kernel_ms;         /* HIP events around the call's kernels (the per-level host synchronisations included) */
    float scene_ms;          /* building the new handle (fused records, lookup grids), host clock */
    float total_ms;          /* host clock, the whole call */
    uint32_t pad_;
} sdfhip_offset_stats;       /* 48 bytes */
SDFHIP_API int sdfhip_scene_distance(sdfhip_scene *scene, const float *xyz, uint32_t n, int32_t level, sdfhip_clearance *out);
SDFHIP_API int sdfhip_scene_distance_device(sdfhip_scene *scene, const float *d_xyz, uint32_t n, int32_t level, sdfhip_clearance *d_out,
                                            void *stream);
SDFHIP_API int sdfhip_scene_offset(sdfhip_scene *scene, const sdfhip_offset_options *opt, sdfhip_scene **out, sdfhip_octdata *host_out,
                                   sdfhip_offset_stats *stats);

/* ---- smooth blends and morphs of two resident scenes on the exact distance ----------------------------
 * Replaces: nothing in the reference's code -- a tree there is immutable once built.  sdfhip_scene_combine takes min / max of stored
 * bytes, and a stored byte is a distance only in a thin band round the surface, so nothing could be blended there.  On the exact
 * distance above a fillet between two parts and an in-between of two shapes are one value each.  sdfhip_scene_blend builds the tree
 * of that value as a NEW handle.  The rule, pinned (fp32, each operation rounded on its own in the order written; S = 2^-d):
 *   a, b             a = dist_A(p), b = dist_B(p): dist(p) of sdfhip_scene_offset, word for word, on each operand -- the surface of
 *                    level_a / level_b, the sign from the operand's own sampled distance at the clamped point.  An empty surface
 *                    gives +inf or -inf
 *   smin(a, b, k)    h = k > 0.0f ? fmaxf(k - fabsf(a - b), 0.0f) / k : 0.0f;  smin = fminf(a, b) - ((h * h) * k) * 0.25f.
 *                    fmaxf / fminf return the operand that is not a NaN: inf - inf gives h = 0, and every case with an empty operand
 *                    is defined
 *   value(p)         SDFHIP_BLEND_UNION: smin(a, b, k); SDFHIP_BLEND_INTERSECT: -smin(-a, -b, k); SDFHIP_BLEND_SUBTRACT:
 *                    -smin(-a, b, k) (A without B); SDFHIP_BLEND_MORPH: a + (b - a) * t
 *   amount           k, the blend radius in units of the cube (finite, >= 0), for the three smooth ops; t (finite, 0 <= t <= 1) for
 *                    the morph
 *   tree             sdfhip_scene_place's / sdfhip_scene_offset's, word for word, with this value: byte = FromFloat(value, S); a
 *                    node splits iff fabsf(value(centre)) < 2 * S && d < depth; breadth-first node order; every point evaluated as if
 *                    alone.  Nothing is pruned: chain sdfhip_scene_prune
 * What follows from the rule: k = 0 gives the hard operation on exact distances (h = 0: fminf(a, b) and its mirror images), which is
 * not sdfhip_scene_combine's bytes.  t = 0 gives a exactly ((b - a) * 0 is a zero), so Morph(A, B, 0) is Offset(A, 0) byte for byte
 * when B's surface is not empty.  UNION with a B whose root is a leaf of bytes 255 (all outside, no surface: b = +inf, h = 0) is
 * Offset(A, 0) byte for byte, for any k.  smin >= fminf(a, b) - k / 4: two solids a gap g apart grow a bridge iff k > 2 g -- at the
 * midpoint a = b = g / 2 and the value is g / 2 - k / 4.
 * A morph with an empty surface: inf * 0 and inf - inf have no meaning worth pinning, so the call refuses with SDFHIP_ERR_ARG when
 * either operand's surface (at its level) is empty.
 * Both inputs are untouched (frames in flight on them included), a == b is allowed, the operands are on the same device, and each
 * handle's lock is held only while its description is read.  opt: the caller sets size = sizeof(sdfhip_blend_options); the struct
 * grows like sdfhip_prune_options.  depth: -1 = the deeper of the two operands' depths, else 0..12; level_a, level_b: -1 or 0..12,
 * each operand surface's level.  out, host_out: either may be NULL, not both.  stats (may be NULL): points counts the evaluated
 * points (9 for the root, 35 for every block of eight siblings), visited_a / visited_b the records the searches of A's and of B's
 * surface loaded: the same on every call.
 * SDFHIP_ERR_ARG: a null scene or options, both outputs NULL, a size the growth rule refuses, an unknown op, a non-finite amount,
 * k < 0, t outside [0, 1], depth or a level outside -1..12, operands on different devices -- each before any device call -- and a
 * result of more than 2^31 - 1 nodes, and the morph's refusal above; SDFHIP_ERR_BAD_TREE: an operand sdfhip_scene_mesh refuses;
 * SDFHIP_ERR_NOMEM: out of device memory (the inputs stay valid, nothing leaks).
 * The kernel (csrc/blend_kernels.h) is the offset's level pass with two searches per point, one after the other: every point of the
 * result searches both surfaces, the far one included, which is where the time goes (DESIGN.md N14 has the measurements). */
enum { SDFHIP_BLEND_UNION = 0, SDFHIP_BLEND_INTERSECT = 1, SDFHIP_BLEND_SUBTRACT = 2, SDFHIP_BLEND_MORPH = 3 };
typedef struct sdfhip_blend_options {
    uint32_t size;            /* sizeof(sdfhip_blend_options) of the caller's header */
    int32_t op;               /* SDFHIP_BLEND_* */
    float amount;             /* UNION, INTERSECT, SUBTRACT: the blend radius k >= 0; MORPH: t in [0, 1] */
    int32_t depth;            /* -1 = the deeper of the operands' depths; else 0..12 */
    int32_t level_a;          /* A's surface level: -1 = full detail; else 0..12 */
    int32_t level_b;          /* B's */
} sdfhip_blend_options;       /* 24 bytes */
typedef struct sdfhip_blend_stats {
    uint32_t nodes_a, nodes_b, nodes_out, depth_out, levels, pad0_;
    uint64_t points;         /* points evaluated */
    uint64_t visited_a;      /* records the searches of A's surface loaded */
    uint64_t visited_b;      /* ... of B's */
    float kernel_ms;         /* HIP events around the call's kernels (the per-level host synchronisations included) */
    float scene_ms;          /* building the new handle, host clock */
    float total_ms;          /* host clock, the whole call */
    uint32_t pad_;
} sdfhip_blend_stats;        /* 64 bytes */
SDFHIP_API int sdfhip_scene_blend(sdfhip_scene *a, sdfhip_scene *b, const sdfhip_blend_options *opt, sdfhip_scene **out,
                                  sdfhip_octdata *host_out, sdfhip_blend_stats *stats);

/* ---- triangle mesh -> ASDF: exact signed distance on the GPU ------------------------------------------
 * Replaces: nothing in the live reference -- SdfGen builds from the nearest POINT of a cloud (dllmain.cpp:117-161), which
 * sdfhip_sdfgen restates.  It is the intent of the reference's abandoned per-triangle GPU generator (SdfBox/GpuGenerator.cs +
 * Shaders/Distancer.hlsl, SURVEY C10, which never ran) with the sign rule of the paper its README names as a main reference:
 * Baerentzen & Aanaes, "Signed distance computation using the angle weighted pseudonormal".
 *   sdfhip_load_ply_mesh / _obj_mesh   a file WITH its faces into an sdfhip_mesh (release with sdfhip_mesh_free): the format limits of
 *                              sdfhip_load_ply / _obj (binary little-endian ply, vertex element first, six floats per vertex, then a
 *                              `property list uchar int` face element; obj: v / vn / f, `#`, o, s, vt skipped) with faces as
 *                              `a`, `a/b`, `a//c`, `a/b/c`, negative (relative) indices, polygons fanned from their first vertex
 *                              (0, i, i+1); a vertex's normal is the file's where it has one, else 0.  They read what
 *                              sdfhip_mesh_save_ply / _obj wrote bit for bit.  SDFHIP_ERR_IO: truncated or malformed.
 *   sdfhip_trimesh_prepare     host: n_triangles x 3 vertices of `stride` 3 or 6 floats (6 = sdfhip_mesh.verts6, normals ignored),
 *                              counter-clockwise seen from outside, into records (release with sdfhip_trimesh_free)
 *   sdfhip_trimesh_build       GPU: records -> a resident scene and / or host arrays; the tree leaves HBM only for host_out
 * prepare, pinned.  fit = 0 (default): coordinates as given, so the mesh of a scene lands where the scene was.  fit = 1: fp32, per
 * axis mid = (lo + hi) * 0.5f of the bounding box, ext = the largest hi - lo, s = fill / ext (fill default 0.8),
 * p' = (p - mid) * s + 0.5f; scale = s and offset = mid are reported (fit = 0: 1 and 0).  Then -0 becomes +0, and vertices are
 * welded when their fp32 bits are equal; an edge is the unordered pair of welded vertices.  A triangle whose area in double is 0 or
 * below 2^-40 of its longest edge squared is dropped and counted.  Normals, all in double from the fp32 positions, normalised, rounded
 * to fp32: face = cross(b - a, c - a); edge pseudonormal = the sum of the unit normals of the faces on that edge; vertex
 * pseudonormal = sum of angle * unit face normal, angle = atan2(|u x v|, u . v) of the triangle's two edges at the vertex; a zero
 * sum falls back to the triangle's own face normal.  A record is 32 floats (128 bytes): a b c | face normal | pseudonormals of edges
 * ab bc ca | of vertices a b c | index of the source triangle (uint32 bits) | 0.  An open or non-manifold mesh still builds (open_edges
 * counts the edges with other than two faces); the sign near such a defect is whatever the rule below gives with the one-sided sums.
 * SDFHIP_ERR_ARG: null pointer, n = 0, stride not 3 or 6, a non-finite coordinate, |coordinate| > 1024 after the fit, fill not in
 * (0, 1024], no triangle left, an options struct the size rules of sdfhip_mesh_options refuse.
 * build, pinned: fp32, each operation rounded in the order written, dot(x, y) = (x0*y0 + x1*y1) + x2*y2.
 *   distance of p to a record (Ericson's region test, in this order)
 *     ab = b-a, ac = c-a, ap = p-a, d1 = dot(ab,ap), d2 = dot(ac,ap);  d1 <= 0 && d2 <= 0: vertex a
 *     bp = p-b, d3 = dot(ab,bp), d4 = dot(ac,bp);                      d3 >= 0 && d4 <= d3: vertex b
 *     vc = d1*d4 - d3*d2;            vc <= 0 && d1 >= 0 && d3 <= 0: edge ab, q = a + ab*(d1/(d1-d3))
 *     cp = p-c, d5 = dot(ab,cp), d6 = dot(ac,cp);                      d6 >= 0 && d5 <= d6: vertex c
 *     vb = d5*d2 - d1*d6;            vb <= 0 && d2 >= 0 && d6 <= 0: edge ca, q = a + ac*(d2/(d2-d6))
 *     va = d3*d6 - d5*d4;            va <= 0 && (d4-d3) >= 0 && (d5-d6) >= 0: edge bc, q = b + (c-b)*((d4-d3)/((d4-d3)+(d5-d6)))
 *     else the face: den = 1/((va+vb)+vc), q = (a + ab*(vb*den)) + ac*(vc*den)
 *     r = p - q, D = dot(r, r)
 *   winner    the record with the smallest D by strict <, so a NaN never wins; ties go to the lowest record index; no winner: +inf
 *   value     s = dot(r, N), N the winner's face, edge or vertex pseudonormal by the region that returned; s < 0 ? -sqrtf(D) : sqrtf(D)
 *   tree      scene_gen's construct rule (SdfGen/dllmain.cpp:163-190) with this distance: corner k of a node of depth d at pos +
 *             split(k) * S, S = 2^-d (exact dyadics); byte = FromFloat(value, S) (dllmain.cpp:192-196); a node splits iff
 *             fabsf(value(centre)) < 2 * S && d < depth
 *   order     breadth first: node 0 the root (parent -1); a level's child blocks of eight follow in ascending parent index (the order
 *             sdfhip_scene_edit appends in); a leaf's children is -1
 * The GPU keeps a candidate list per block of eight siblings and prunes it conservatively (DESIGN.md N8 derives the slack): the bytes
 * are those of brute force over all records.  depth 0..12.  scene, host_out: either may be NULL, not both; stats may be NULL.
 * SDFHIP_ERR_ARG: a null mesh or records, n_records = 0, depth outside 0..12, both outputs NULL, more than 2^31 - 1 nodes;
 * SDFHIP_ERR_NOMEM: out of device memory (nothing leaks, no handle is returned).  Memory comes from the builder's chunk pool
 * (sdfhip_sdfgen_trim gives it back). */
typedef struct sdfhip_trimesh_options {
    uint32_t size;          /* set by sdfhip_trimesh_options_default; grows like sdfhip_mesh_options */
    int32_t fit;            /* -1 = default (0): coordinates as given; 1: centre the bounding box at 0.5, longest side = fill */
    float fill;             /* -1 = default (0.8f) */
} sdfhip_trimesh_options;
typedef struct sdfhip_trimesh {
    uint32_t n_records;
    float *records;         /* n_records x 32 floats */
    uint32_t n_vertices, n_edges;      /* welded vertices and edges of the triangles kept */
    uint32_t n_dropped, open_edges;    /* triangles dropped; edges with other than two faces */
    float scale, offset[3];            /* the fit's s and mid */
} sdfhip_trimesh;
typedef struct sdfhip_trimesh_stats {
    uint32_t nodes, levels, records, pad_;
    uint64_t candidate_entries;        /* sum of all candidate-list lengths: the work measure */
    float build_ms;                    /* HIP events around the build's kernels */
    float scene_ms;                    /* building the handle (fused records, lookup grids), host clock */
    float total_ms;                    /* host clock, the whole call */
    uint32_t pad1_;
} sdfhip_trimesh_stats;
SDFHIP_API int sdfhip_load_ply_mesh(const char *path, sdfhip_mesh *out);
SDFHIP_API int sdfhip_load_obj_mesh(const char *path, sdfhip_mesh *out);
SDFHIP_API void sdfhip_trimesh_options_default(sdfhip_trimesh_options *opt);
SDFHIP_API int sdfhip_trimesh_prepare(const float *verts, uint32_t n_triangles, uint32_t stride, const sdfhip_trimesh_options *opt,
                                      sdfhip_trimesh *out);
SDFHIP_API void sdfhip_trimesh_free(sdfhip_trimesh *mesh);
SDFHIP_API int sdfhip_trimesh_build(int device, const sdfhip_trimesh *mesh, int32_t depth, sdfhip_scene **scene, sdfhip_octdata *host_out,
                                    sdfhip_trimesh_stats *stats);

/* ---- one frame over several GPUs, behind one call -----------------------------------------------------------
 * Replaces: Program.Draw's UpdateBuffer(info) + DispatchSized(W, H, 1) (SdfBox/Program.cs:81,94) when the frame is rendered by
 * the GPUs of a node: the host still makes ONE call per frame.  One process; the scene is replicated on every device at
 * create; the frame's 16-row bands are dealt to the devices; every device renders its bands with the default kernel, which
 * writes the sparse wire share itself; ranks > 0 push their shares into device devices[0]'s memory over their own xGMI links
 * (peer copies on the rank's stream; SDFHIP_MULTI_TRANSPORT=rccl in the environment at create: ncclSend / ncclRecv inside
 * ncclGroupStart/End instead, RCCL loaded with dlopen); devices[0] expands them into the frame in row order.  Inside the
 * library: one host thread per device, the band layout, the gather, the float tail of a share that needed more than was
 * sent, no Python.  The same device may appear several times (a rehearsal of the pipeline on one GPU; not with RCCL).
 * Environment, read at create: SDFHIP_MULTI_TRANSPORT (above), SDFHIP_RCCL_LIB (the RCCL library to dlopen, if not the system's),
 * SDFHIP_MULTI_RCCL_SELF=1 (with ONE device and the RCCL transport: its share travels through ncclSend / ncclRecv to itself -- all
 * of that transport a single GPU can run).  With SDFHIP_GEN_POOL and SDFHIP_KEEP_ENV (the note at the top of this file) these are
 * the only variables the product library reads; every other choice is an argument (sdfhip_upload_options, sdfhip_multi_configure).
 *   sdfhip_multi_render        one frame to a host array: the viewer's call (latency: every device works on this frame)
 *   sdfhip_multi_submit/_wait  groups of n_frames <= 8 frames (one camera block each, one launch per device), up to 4 groups
 *                              in flight (slot 0..3): throughput.  d_frames_out: device memory on devices[0] for
 *                              [n_frames][height][width] pixels, or NULL for the slot's own buffer (returned by _wait, valid
 *                              until the slot's next submit).  _wait blocks until the slot's frames are complete.
 *   ..._path                   the path-traced mode (one frame; gathers dense RGBA32F bands)
 * Flags: 0, SDFHIP_FLAG_DISPLAY[_DEBUG] (RGBA8 frames: the display pass runs where the frame is assembled),
 * SDFHIP_FLAG_TILE_ORDER.  Pixels are bit for bit those of sdfhip_render on one device. */
typedef struct sdfhip_multi sdfhip_multi;
typedef struct sdfhip_multi_stats {
    float total_ms;             /* host clock: submit -> frames complete (sdfhip_multi_render: -> frame in the host array) */
    uint32_t n_devices;
    uint32_t resends;           /* shares whose float tail had to be sent again */
    uint32_t pad_;
    uint64_t gathered_bytes;    /* bytes that crossed into devices[0] */
    float rank_ms[16];          /* per device: first launch -> share sent (HIP events on its stream) */
    uint32_t floats_used[16];   /* per device: float slots of its share */
} sdfhip_multi_stats;
SDFHIP_API int sdfhip_multi_create(const int *devices, uint32_t n_devices, const int32_t *structs, const uint8_t *values,
                                   uint32_t n, sdfhip_multi **out);
/* First contact with the node's links.  Per device r > 0: can it reach devices[0]'s memory (hipDeviceCanAccessPeer), and does a
 * 1 MB pattern pushed the way the gather pushes shares -- hipMemcpyPeerAsync on r's stream, or ncclSend / ncclRecv in a group with
 * the RCCL transport -- arrive in devices[0]'s memory intact (read back and compared on the host)?  sdfhip_multi_create runs it and
 * fails with SDFHIP_ERR_DEVICE naming the pair, instead of leaving a link problem to surface as a wrong frame; callable again at
 * any time no slot is in flight.  links (may be NULL): n_devices entries. */
typedef struct sdfhip_multi_link {
    int32_t device;             /* devices[r]                                                        */
    int32_t peer_access;        /* 1: devices[r] writes devices[0]'s memory directly (xGMI / PCIe P2P); 0: the copy is staged; -1: same device */
    uint32_t ok;                /* the pattern arrived                                               */
    float push_ms;              /* HIP-event time of the 1 MB push on the sender's stream            */
    char pci_bus_id[16];        /* "0000:c1:00.0"                                                    */
} sdfhip_multi_link;
SDFHIP_API int sdfhip_multi_selftest(sdfhip_multi *m, sdfhip_multi_link *links);
SDFHIP_API int sdfhip_multi_free(sdfhip_multi *m);
/* band height (a multiple of 8; default 16) and the share of devices[0], which also assembles the frame, as a fraction of a
 * peer's (default 1); no slot may be in flight */
SDFHIP_API int sdfhip_multi_configure(sdfhip_multi *m, uint32_t band_rows, float rank0_weight);
SDFHIP_API int sdfhip_multi_info(const sdfhip_multi *m, uint32_t *n_devices, int *devices, uint32_t *band_rows,
                                 float *rank0_weight, int *transport /* 0 peer copies, 1 RCCL */);
SDFHIP_API int sdfhip_multi_render(sdfhip_multi *m, const sdfhip_info *info, uint32_t width, uint32_t height, uint32_t flags,
                                   float *rgba_out, sdfhip_multi_stats *stats);
SDFHIP_API int sdfhip_multi_render_path(sdfhip_multi *m, const sdfhip_info *info, const sdfhip_pathtrace *pt, uint32_t width,
                                        uint32_t height, uint32_t flags, float *rgba_out, sdfhip_multi_stats *stats);
SDFHIP_API int sdfhip_multi_submit(sdfhip_multi *m, uint32_t slot, const sdfhip_info *infos, uint32_t n_frames, uint32_t width,
                                   uint32_t height, uint32_t flags, void *d_frames_out);
SDFHIP_API int sdfhip_multi_submit_path(sdfhip_multi *m, uint32_t slot, const sdfhip_info *info, const sdfhip_pathtrace *pt,
                                        uint32_t width, uint32_t height, uint32_t flags, void *d_frame_out);
SDFHIP_API int sdfhip_multi_wait(sdfhip_multi *m, uint32_t slot, void **d_frames, sdfhip_multi_stats *stats);
#ifdef __cplusplus
}
#endif
#endif /* SDFHIP_H */
