"""ctypes binding of libsdfhip.so (include/sdfhip.h).

The library is the product; there is no Python or CPU fallback.  If it has not
been built (``python -c "import __graft_entry__ as g; g.build()"`` or
``make -C sdfbox_amd/csrc``) importing this module raises.
"""
import ctypes
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# SDFHIP_LIB: another build of the library -- sdfbox_amd/libsdfhip_lab.so is the experiments flavour (include/sdfhip_experimental.h:
# the A/B kernel forms, superseded gather formats and test hooks; sdfbox_amd.lab.load() imports this package a second time against it)
LIB_PATH = os.path.abspath(os.environ.get("SDFHIP_LIB") or os.path.join(_HERE, "libsdfhip.so"))
LAB_LIB_PATH = os.path.join(_HERE, "libsdfhip_lab.so")

# PyTorch bundles its own libamdhip64.so; load it first so that libsdfhip.so
# binds to the same HIP runtime instance torch uses (one runtime per process:
# device pointers and streams are then interchangeable).
try:  # pragma: no cover - depends on the environment
    import torch  # noqa: F401
except Exception:  # torch is plumbing, not a requirement of the C ABI
    torch = None

if not os.path.exists(LIB_PATH):
    raise ImportError(
        f"{LIB_PATH} is missing: build it with `make -C {os.path.join(_HERE, 'csrc')}` "
        "(hipcc --offload-arch=gfx950). sdfbox_amd has no CPU fallback.")

lib = ctypes.CDLL(LIB_PATH)

OK, ERR_ARG, ERR_IO, ERR_BAD_TREE, ERR_DEVICE, ERR_NOMEM = range(6)

KERNEL_AUTO, KERNEL_GENERIC, KERNEL_STACK = 0, 1, 2
FLAG_COMPACT, FLAG_COUNT, FLAG_DISPLAY, FLAG_DISPLAY_DEBUG = 0x10, 0x20, 0x40, 0x80
FLAG_TILE_ORDER = 0x100000    # launch the tiles in descending order of their cost in this stream's last frame (latency of one frame)
# include/sdfhip_experimental.h: the A/B knobs of the experiments build (libsdfhip.so refuses them)
FLAG_WIRE = 0x10000
TUNE_ORDER_SHIFT, TUNE_BLOCK_SHIFT = 8, 12
TUNE_ONE_KERNEL = 0x20000     # round 1's one-kernel lane state machine where the default is k_march
TUNE_LDS_TOP = 0x40000        # the one-kernel form with the top grid (level <= 3) staged in LDS per workgroup
TUNE_SHADOW_QUEUE = 0x80000   # FLAG_COMPACT's kernels with EVERY shadow ray queued for k_shadow (round 2's form; SDFHIP_SHADOW_MIN_LANES=T sets the threshold)
TUNE_PERSISTENT_WAVES = 0x400000   # with FLAG_COMPACT on a grid scene: the persistent-wave lane-refill kernel (k_compact), the flag's form until round 4
TUNE_BYTE_CELLS = 0x200000    # on a scene uploaded under SDFHIP_SAMPLE_RECORDS=1: back to the 16-byte cells every other scene reads
SHAPE_SPHERE, SHAPE_TORUS, SHAPE_GYROID = 0, 1, 2
EDIT_CARVE, EDIT_ADD = 0, 1          # sdfhip_scene_edit: subtract / union
BRUSH_SPHERE, BRUSH_BOX = 0, 1
COMBINE_UNION, COMBINE_INTERSECT, COMBINE_SUBTRACT = 0, 1, 2      # sdfhip_scene_combine: A or B, A and B, A without B
OFFSET_GROW, OFFSET_SHELL = 0, 1     # sdfhip_scene_offset: dist - amount / fabsf(dist) - amount / 2
BLEND_UNION, BLEND_INTERSECT, BLEND_SUBTRACT, BLEND_MORPH = 0, 1, 2, 3      # sdfhip_scene_blend: smooth A or B, A and B, A without B; the in-between
VOLUME_F32, VOLUME_F16 = 0, 1        # sdfhip_volume.dtype
QUERY_HIT, QUERY_ESCAPED, QUERY_EXHAUSTED, QUERY_INVALID = 0, 1, 2, 3      # sdfhip_probe.status / sdfhip_hit.status
INSTANCES_NO_SKIP = 1                # sdfhip_instances_options.flags: look every instance up at every point
CLASH_NO_SKIP = 1                    # sdfhip_clash_options.flags: look every instance up at every lattice point
CLASH_MAX_INSTANCES = 64             # sdfhip_instances_clash: a containment mask is one 64-bit word
PENETRATION_NO_SKIP = 1              # sdfhip_penetration_options.flags: look every instance up at every lattice point
GAP_NO_PRUNE = 1                     # sdfhip_gap_options.flags: every candidate of every pair, no bound, no broad phase
GAP_WITNESS_OF_B, GAP_CONTAINED = 1, 2   # sdfhip_gap.flags: the witness vertex is part b's; one closest point is inside the other part
COMPONENT_SOLID = 1                  # sdfhip_component.flags: a component of the inside phase (0: a void)
COMPONENTS_MAX_DEPTH = 9             # sdfhip_scene_components: 4 bytes per lattice point
# sdfhip_select_options.flags: the rule bits of sdfhip_scene_select, OR-ed
SELECT_KEEP_LARGEST_SOLID, SELECT_DROP_SMALL_SOLIDS, SELECT_FILL_ENCLOSED_VOIDS, SELECT_FLIP_LISTED, SELECT_KEEP_LISTED = 1, 2, 4, 8, 16


if __name__ != "sdfbox_amd._lib":
    # the package imported a second time against another flavour of the library (sdfbox_amd.lab.load()): both flavours share ONE
    # set of ctypes classes, so that a camera, a PathTrace or a Stats object made with either package is accepted by both
    from sdfbox_amd._lib import CMesh, COctData, CTriMesh, TriMeshOptions, TriMeshStats, CPoints, Edit, EditStats, PruneOptions, PruneStats, CombineOptions, CombineStats, Placement, PlaceStats, Instance, ComposeOptions, ComposeStats, InstancesOptions, PartProbe, PartHit, ClashOptions, Clash, ClashStats, PenetrationOptions, Penetration, PenetrationStats, GapOptions, Gap, GapStats, ComponentsOptions, Component, ComponentsStats, SelectOptions, SelectStats, Volume, VolumeStats, Clearance, OffsetOptions, OffsetStats, BlendOptions, BlendStats, Hit, Info, Measure, MeasureOptions, MeshOptions, MeshStats, SliceOptions, Segment, CSlice, SliceStats, MultiLink, MultiStats, PathTrace, Probe, Ray, SdfGenStats, SdfHipError, Stats, UploadOptions   # noqa: F401
else:
    class Info(ctypes.Structure):
        """The 112-byte `Info` cbuffer (Logic.cs:407-420)."""
        _fields_ = [
            ("heading", (ctypes.c_float * 4) * 3),
            ("position", ctypes.c_float * 3),
            ("margin", ctypes.c_float),
            ("screen_size", ctypes.c_float * 2),
            ("buffer_size", ctypes.c_uint32),
            ("limit", ctypes.c_float),
            ("light", ctypes.c_float * 3),
            ("strength", ctypes.c_float),
            ("fov", ctypes.c_float),
            ("hidef", ctypes.c_int32),
            ("pad_", ctypes.c_uint32 * 2),
        ]


    assert ctypes.sizeof(Info) == 112


    class COctData(ctypes.Structure):
        _fields_ = [
            ("length", ctypes.c_uint32),
            ("structs", ctypes.POINTER(ctypes.c_int32)),
            ("values", ctypes.POINTER(ctypes.c_uint8)),
        ]


    class Stats(ctypes.Structure):
        _fields_ = [
            ("kernel_ms", ctypes.c_float),
            ("total_ms", ctypes.c_float),
            ("n_nodes", ctypes.c_uint64),
            ("n_samples", ctypes.c_uint64),
            ("n_steps", ctypes.c_uint64),
            ("kernel_used", ctypes.c_uint32),
            ("pad_", ctypes.c_uint32),
            ("n_shadow_rays", ctypes.c_uint64),
            ("n_loads", ctypes.c_uint64),
            ("n_hits", ctypes.c_uint64),
        ]


    class PathTrace(ctypes.Structure):
        """sdfhip_pathtrace: parameters of the path-traced mode (BASELINE config 5 defaults)."""
        _fields_ = [
            ("spp", ctypes.c_uint32),
            ("max_bounces", ctypes.c_uint32),
            ("seed", ctypes.c_uint32),
            ("albedo", ctypes.c_float),
        ]

        def __init__(self, spp=16, max_bounces=3, seed=0x5DFB0C5, albedo=0.8):
            super().__init__(int(spp), int(max_bounces), int(seed), float(albedo))


    class UploadOptions(ctypes.Structure):
        """sdfhip_upload_options: the upload's own choices, overridden (None / -1 = choose)."""
        _fields_ = [("size", ctypes.c_uint32), ("top_grid_level", ctypes.c_int32), ("top_grid_split", ctypes.c_int32),
                    ("scatter_grid", ctypes.c_int32), ("scatter_order", ctypes.c_int32)]

        def __init__(self, top_grid_level=None, top_grid_split=None, scatter_grid=None, scatter_order=None):
            f = lambda v: -1 if v is None else int(v)
            super().__init__(ctypes.sizeof(type(self)), f(top_grid_level), f(top_grid_split), f(scatter_grid), f(scatter_order))


    class CPoints(ctypes.Structure):
        _fields_ = [("count", ctypes.c_uint32), ("data", ctypes.POINTER(ctypes.c_float))]


    class SdfGenStats(ctypes.Structure):
        _fields_ = [
            ("nodes", ctypes.c_uint32), ("levels", ctypes.c_uint32),
            ("candidate_entries", ctypes.c_uint64),
            ("global_scale", ctypes.c_float), ("global_offset", ctypes.c_float * 3),
            ("total_ms", ctypes.c_float),
        ]


    class MultiLink(ctypes.Structure):
        _fields_ = [("device", ctypes.c_int32), ("peer_access", ctypes.c_int32), ("ok", ctypes.c_uint32), ("push_ms", ctypes.c_float),
                    ("pci_bus_id", ctypes.c_char * 16)]


    class MultiStats(ctypes.Structure):
        _fields_ = [
            ("total_ms", ctypes.c_float), ("n_devices", ctypes.c_uint32), ("resends", ctypes.c_uint32), ("pad_", ctypes.c_uint32),
            ("gathered_bytes", ctypes.c_uint64), ("rank_ms", ctypes.c_float * 16), ("floats_used", ctypes.c_uint32 * 16),
        ]


    class Edit(ctypes.Structure):
        """sdfhip_edit: one brush.  params: sphere (cx, cy, cz, r); box (cx, cy, cz, hx, hy, hz), axis-aligned half extents."""
        _fields_ = [("op", ctypes.c_int32), ("brush", ctypes.c_int32), ("params", ctypes.c_float * 6)]

        def __init__(self, op, brush, params):
            p = [float(x) for x in params] + [0.0] * (6 - len(params))
            super().__init__(int(op), int(brush), (ctypes.c_float * 6)(*p[:6]))


    class EditStats(ctypes.Structure):
        _fields_ = [("nodes_in", ctypes.c_uint32), ("nodes_out", ctypes.c_uint32), ("nodes_visited", ctypes.c_uint32),
                    ("nodes_changed", ctypes.c_uint32), ("blocks_added", ctypes.c_uint32), ("depth_out", ctypes.c_uint32),
                    ("edit_ms", ctypes.c_float), ("scene_ms", ctypes.c_float), ("total_ms", ctypes.c_float)]


    class PruneOptions(ctypes.Structure):
        """sdfhip_prune_options: tolerance 0..255 (None = the default, 0); max_depth None = no cut, else 0..12."""
        _fields_ = [("size", ctypes.c_uint32), ("tolerance", ctypes.c_int32), ("max_depth", ctypes.c_int32)]

        def __init__(self, tolerance=None, max_depth=None):
            super().__init__(ctypes.sizeof(type(self)), -1 if tolerance is None else int(tolerance), -1 if max_depth is None else int(max_depth))


    class PruneStats(ctypes.Structure):
        _fields_ = [("nodes_in", ctypes.c_uint32), ("nodes_out", ctypes.c_uint32), ("blocks_removed", ctypes.c_uint32),
                    ("depth_out", ctypes.c_uint32), ("kernel_ms", ctypes.c_float), ("scene_ms", ctypes.c_float), ("total_ms", ctypes.c_float)]


    assert (ctypes.sizeof(PruneOptions), ctypes.sizeof(PruneStats)) == (12, 28)


    class CombineOptions(ctypes.Structure):
        """sdfhip_combine_options: max_depth None = no cut, else 0..12."""
        _fields_ = [("size", ctypes.c_uint32), ("max_depth", ctypes.c_int32)]

        def __init__(self, max_depth=None):
            super().__init__(ctypes.sizeof(type(self)), -1 if max_depth is None else int(max_depth))


    class CombineStats(ctypes.Structure):
        _fields_ = [("nodes_a", ctypes.c_uint32), ("nodes_b", ctypes.c_uint32), ("nodes_out", ctypes.c_uint32), ("depth_out", ctypes.c_uint32),
                    ("nodes_shared", ctypes.c_uint32), ("kernel_ms", ctypes.c_float), ("scene_ms", ctypes.c_float), ("total_ms", ctypes.c_float)]


    assert (ctypes.sizeof(CombineOptions), ctypes.sizeof(CombineStats)) == (8, 32)


    class Placement(ctypes.Structure):
        """sdfhip_placement: a source point x lands at scale * rotation @ x + translation.  rotation (3, 3) row-major, orthogonal;
        scale > 0; depth None = the source's depth, else 0..12."""
        _fields_ = [("size", ctypes.c_uint32), ("rotation", (ctypes.c_float * 3) * 3), ("scale", ctypes.c_float),
                    ("translation", ctypes.c_float * 3), ("depth", ctypes.c_int32)]

        def __init__(self, rotation=((1, 0, 0), (0, 1, 0), (0, 0, 1)), scale=1.0, translation=(0, 0, 0), depth=None):
            rows = [[float(x) for x in row] for row in rotation]
            if len(rows) != 3 or any(len(row) != 3 for row in rows):
                raise ValueError("rotation must be 3 x 3")
            t = [float(x) for x in translation]
            if len(t) != 3:
                raise ValueError("translation must have three components")
            super().__init__(ctypes.sizeof(type(self)), ((ctypes.c_float * 3) * 3)(*[(ctypes.c_float * 3)(*row) for row in rows]), float(scale),
                             (ctypes.c_float * 3)(*t), -1 if depth is None else int(depth))


    class PlaceStats(ctypes.Structure):
        _fields_ = [("nodes_in", ctypes.c_uint32), ("nodes_out", ctypes.c_uint32), ("depth_out", ctypes.c_uint32), ("levels", ctypes.c_uint32),
                    ("samples", ctypes.c_uint64), ("kernel_ms", ctypes.c_float), ("scene_ms", ctypes.c_float), ("total_ms", ctypes.c_float),
                    ("pad_", ctypes.c_uint32)]


    assert (ctypes.sizeof(Placement), ctypes.sizeof(PlaceStats)) == (60, 40)


    class Instance(ctypes.Structure):
        """sdfhip_instance: one placed instance of a resident scene for sdfhip_scene_compose.  scene: the handle (a c_void_p or its
        value); op: COMBINE_UNION / _INTERSECT / _SUBTRACT, how the instance joins what precedes it; rotation, scale, translation:
        as Placement's."""
        _fields_ = [("scene", ctypes.c_void_p), ("op", ctypes.c_int32), ("rotation", (ctypes.c_float * 3) * 3), ("scale", ctypes.c_float),
                    ("translation", ctypes.c_float * 3)]

        def __init__(self, scene=None, op=0, rotation=((1, 0, 0), (0, 1, 0), (0, 0, 1)), scale=1.0, translation=(0, 0, 0)):
            rows = [[float(x) for x in row] for row in rotation]
            if len(rows) != 3 or any(len(row) != 3 for row in rows):
                raise ValueError("rotation must be 3 x 3")
            t = [float(x) for x in translation]
            if len(t) != 3:
                raise ValueError("translation must have three components")
            super().__init__(getattr(scene, "value", scene), int(op), ((ctypes.c_float * 3) * 3)(*[(ctypes.c_float * 3)(*row) for row in rows]),
                             float(scale), (ctypes.c_float * 3)(*t))


    class ComposeOptions(ctypes.Structure):
        """sdfhip_compose_options: depth None = the largest depth among the sources, else 0..12."""
        _fields_ = [("size", ctypes.c_uint32), ("depth", ctypes.c_int32)]

        def __init__(self, depth=None):
            super().__init__(ctypes.sizeof(type(self)), -1 if depth is None else int(depth))


    class ComposeStats(ctypes.Structure):
        _fields_ = [("nodes_out", ctypes.c_uint32), ("depth_out", ctypes.c_uint32), ("levels", ctypes.c_uint32), ("instances", ctypes.c_uint32),
                    ("samples", ctypes.c_uint64), ("kernel_ms", ctypes.c_float), ("scene_ms", ctypes.c_float), ("total_ms", ctypes.c_float),
                    ("pad_", ctypes.c_uint32)]


    assert (ctypes.sizeof(Instance), ctypes.sizeof(ComposeOptions), ctypes.sizeof(ComposeStats)) == (64, 8, 40)


    class Volume(ctypes.Structure):
        """sdfhip_volume: a regular lattice of n = (nx, ny, nz) samples, sample (i, j, k) at origin + (i, j, k) * spacing and at index
        (k * ny + j) * nx + i.  value_scale and depth describe a build (stored value * value_scale = distance in cube units; depth
        0..12) and are 0 for a lattice to fill; dtype VOLUME_F32 / VOLUME_F16."""
        _fields_ = [("size", ctypes.c_uint32), ("n", ctypes.c_uint32 * 3), ("origin", ctypes.c_float * 3), ("spacing", ctypes.c_float),
                    ("value_scale", ctypes.c_float), ("dtype", ctypes.c_int32), ("depth", ctypes.c_int32)]

        def __init__(self, n=(2, 2, 2), origin=(0, 0, 0), spacing=1.0, value_scale=0.0, dtype=0, depth=0):
            n = [int(x) for x in n]
            o = [float(x) for x in origin]
            if len(n) != 3 or len(o) != 3:
                raise ValueError("n and origin must have three components")
            if any(x < 0 or x > 0xFFFFFFFF for x in n):
                raise ValueError("n must be three counts")
            super().__init__(ctypes.sizeof(type(self)), (ctypes.c_uint32 * 3)(*n), (ctypes.c_float * 3)(*o), float(spacing), float(value_scale),
                             int(dtype), int(depth))


    class VolumeStats(ctypes.Structure):
        _fields_ = [("nodes_out", ctypes.c_uint32), ("depth_out", ctypes.c_uint32), ("levels", ctypes.c_uint32), ("pad_", ctypes.c_uint32),
                    ("samples", ctypes.c_uint64), ("check_ms", ctypes.c_float), ("kernel_ms", ctypes.c_float), ("scene_ms", ctypes.c_float),
                    ("total_ms", ctypes.c_float)]


    assert (ctypes.sizeof(Volume), ctypes.sizeof(VolumeStats)) == (44, 40)


    class Clearance(ctypes.Structure):
        """sdfhip_clearance: the answer for one point of sdfhip_scene_distance."""
        _fields_ = [("distance", ctypes.c_float), ("node", ctypes.c_uint32), ("nearest", ctypes.c_float * 3), ("status", ctypes.c_uint32),
                    ("visited", ctypes.c_uint32), ("pad_", ctypes.c_uint32)]


    class OffsetOptions(ctypes.Structure):
        """sdfhip_offset_options: mode OFFSET_GROW (amount = delta) or OFFSET_SHELL (amount = the thickness, > 0); depth None = the
        source's depth, else 0..12; level: the source surface's level, -1 = full detail."""
        _fields_ = [("size", ctypes.c_uint32), ("mode", ctypes.c_int32), ("amount", ctypes.c_float), ("depth", ctypes.c_int32),
                    ("level", ctypes.c_int32)]

        def __init__(self, mode=0, amount=0.0, depth=None, level=-1):
            super().__init__(ctypes.sizeof(type(self)), int(mode), float(amount), -1 if depth is None else int(depth), int(level))


    class OffsetStats(ctypes.Structure):
        _fields_ = [("nodes_in", ctypes.c_uint32), ("nodes_out", ctypes.c_uint32), ("depth_out", ctypes.c_uint32), ("levels", ctypes.c_uint32),
                    ("points", ctypes.c_uint64), ("visited", ctypes.c_uint64), ("kernel_ms", ctypes.c_float), ("scene_ms", ctypes.c_float),
                    ("total_ms", ctypes.c_float), ("pad_", ctypes.c_uint32)]


    assert (ctypes.sizeof(Clearance), ctypes.sizeof(OffsetOptions), ctypes.sizeof(OffsetStats)) == (32, 20, 48)


    class BlendOptions(ctypes.Structure):
        """sdfhip_blend_options: op BLEND_UNION / _INTERSECT / _SUBTRACT (amount = the blend radius k >= 0) or BLEND_MORPH (amount = t in
        [0, 1]); depth None = the deeper of the operands' depths, else 0..12; level_a, level_b: each operand surface's level, -1 = full
        detail."""
        _fields_ = [("size", ctypes.c_uint32), ("op", ctypes.c_int32), ("amount", ctypes.c_float), ("depth", ctypes.c_int32),
                    ("level_a", ctypes.c_int32), ("level_b", ctypes.c_int32)]

        def __init__(self, op=0, amount=0.0, depth=None, level_a=-1, level_b=-1):
            super().__init__(ctypes.sizeof(type(self)), int(op), float(amount), -1 if depth is None else int(depth), int(level_a), int(level_b))


    class BlendStats(ctypes.Structure):
        _fields_ = [("nodes_a", ctypes.c_uint32), ("nodes_b", ctypes.c_uint32), ("nodes_out", ctypes.c_uint32), ("depth_out", ctypes.c_uint32),
                    ("levels", ctypes.c_uint32), ("pad0_", ctypes.c_uint32), ("points", ctypes.c_uint64), ("visited_a", ctypes.c_uint64),
                    ("visited_b", ctypes.c_uint64), ("kernel_ms", ctypes.c_float), ("scene_ms", ctypes.c_float), ("total_ms", ctypes.c_float),
                    ("pad_", ctypes.c_uint32)]


    assert (ctypes.sizeof(BlendOptions), ctypes.sizeof(BlendStats)) == (24, 64)


    class Probe(ctypes.Structure):
        """sdfhip_probe: the answer for one point of sdfhip_scene_sample."""
        _fields_ = [("distance", ctypes.c_float), ("node", ctypes.c_uint32), ("scale", ctypes.c_float), ("status", ctypes.c_uint32),
                    ("gradient", ctypes.c_float * 3), ("pad_", ctypes.c_uint32)]


    class Ray(ctypes.Structure):
        """sdfhip_ray: origin and direction (used as given) of one ray of sdfhip_scene_raycast."""
        _fields_ = [("origin", ctypes.c_float * 3), ("pad0_", ctypes.c_float), ("dir", ctypes.c_float * 3), ("pad1_", ctypes.c_float)]


    class Hit(ctypes.Structure):
        """sdfhip_hit: where one ray's march ended (sdfhip_scene_raycast, sdfhip_scene_pick)."""
        _fields_ = [("position", ctypes.c_float * 3), ("t", ctypes.c_float), ("normal", ctypes.c_float * 3), ("prox", ctypes.c_float),
                    ("status", ctypes.c_uint32), ("steps", ctypes.c_uint32), ("node", ctypes.c_uint32), ("scale", ctypes.c_float)]


    assert (ctypes.sizeof(Probe), ctypes.sizeof(Ray), ctypes.sizeof(Hit)) == (32, 32, 48)


    class InstancesOptions(ctypes.Structure):
        """sdfhip_instances_options: flags INSTANCES_NO_SKIP or 0; max_steps None = 100 (the shader's), else 1..4096; normal_step None =
        2^-10, else finite and above 0."""
        _fields_ = [("size", ctypes.c_uint32), ("flags", ctypes.c_uint32), ("max_steps", ctypes.c_uint32), ("normal_step", ctypes.c_float)]

        def __init__(self, flags=0, max_steps=None, normal_step=None):
            super().__init__(ctypes.sizeof(type(self)), int(flags), 0 if max_steps is None else int(max_steps),
                             0.0 if normal_step is None else float(normal_step))


    class PartProbe(ctypes.Structure):
        """sdfhip_part_probe: the answer for one point of sdfhip_instances_sample."""
        _fields_ = [("value", ctypes.c_float), ("instance", ctypes.c_uint32), ("status", ctypes.c_uint32), ("pad0_", ctypes.c_uint32),
                    ("gradient", ctypes.c_float * 3), ("pad1_", ctypes.c_uint32)]


    class PartHit(ctypes.Structure):
        """sdfhip_part_hit: where one ray's march through an assembly ended (sdfhip_instances_raycast, sdfhip_instances_pick)."""
        _fields_ = [("position", ctypes.c_float * 3), ("t", ctypes.c_float), ("normal", ctypes.c_float * 3), ("prox", ctypes.c_float),
                    ("status", ctypes.c_uint32), ("steps", ctypes.c_uint32), ("instance", ctypes.c_uint32), ("pad_", ctypes.c_uint32)]


    assert (ctypes.sizeof(InstancesOptions), ctypes.sizeof(PartProbe), ctypes.sizeof(PartHit)) == (16, 32, 48)


    class ClashOptions(ctypes.Structure):
        """sdfhip_clash_options: flags CLASH_NO_SKIP or 0; depth 0..10 (2^depth lattice points along each axis); the cube's origin and
        side (finite, above 0)."""
        _fields_ = [("size", ctypes.c_uint32), ("flags", ctypes.c_uint32), ("depth", ctypes.c_uint32), ("origin", ctypes.c_float * 3),
                    ("side", ctypes.c_float)]

        def __init__(self, flags=0, depth=6, origin=(0.0, 0.0, 0.0), side=1.0):
            super().__init__(ctypes.sizeof(type(self)), int(flags), int(depth), (ctypes.c_float * 3)(*[float(x) for x in origin]), float(side))


    class Clash(ctypes.Structure):
        """sdfhip_clash: one pair a < b of instances that share lattice points (sdfhip_instances_clash)."""
        _fields_ = [("a", ctypes.c_uint32), ("b", ctypes.c_uint32), ("points", ctypes.c_uint32), ("first", ctypes.c_uint32),
                    ("lo", ctypes.c_uint32 * 3), ("hi", ctypes.c_uint32 * 3), ("sum", ctypes.c_uint64 * 3)]


    class ClashStats(ctypes.Structure):
        """sdfhip_clash_stats: points = 8^depth, the lattice's 4 x 4 x 4 blocks, those that looked anything up, the look-ups made."""
        _fields_ = [("points", ctypes.c_uint64), ("blocks", ctypes.c_uint32), ("blocks_looked", ctypes.c_uint32), ("lookups", ctypes.c_uint64),
                    ("kernel_ms", ctypes.c_float), ("total_ms", ctypes.c_float)]


    assert (ctypes.sizeof(ClashOptions), ctypes.sizeof(Clash), ctypes.sizeof(ClashStats)) == (28, 64, 32)


    class PenetrationOptions(ctypes.Structure):
        """sdfhip_penetration_options: flags PENETRATION_NO_SKIP or 0; depth 0..10 (2^depth lattice points along each axis); the cube's
        origin and side (finite, above 0).  sdfhip_clash_options' layout."""
        _fields_ = [("size", ctypes.c_uint32), ("flags", ctypes.c_uint32), ("depth", ctypes.c_uint32), ("origin", ctypes.c_float * 3),
                    ("side", ctypes.c_float)]

        def __init__(self, flags=0, depth=6, origin=(0.0, 0.0, 0.0), side=1.0):
            super().__init__(ctypes.sizeof(type(self)), int(flags), int(depth), (ctypes.c_float * 3)(*[float(x) for x in origin]), float(side))


    class Penetration(ctypes.Structure):
        """sdfhip_penetration: one pair a < b of instances that share lattice points, how far they reach into each other and where
        each part's nearest surface lies (sdfhip_instances_penetration)."""
        _fields_ = [("a", ctypes.c_uint32), ("b", ctypes.c_uint32), ("points", ctypes.c_uint32), ("witness", ctypes.c_uint32),
                    ("depth", ctypes.c_float), ("ra", ctypes.c_float), ("rb", ctypes.c_float), ("node_a", ctypes.c_uint32),
                    ("node_b", ctypes.c_uint32), ("nearest_a", ctypes.c_float * 3), ("nearest_b", ctypes.c_float * 3), ("pad_", ctypes.c_uint32)]


    class PenetrationStats(ctypes.Structure):
        """sdfhip_penetration_stats: the clash check's counts, the searches run and the node records they loaded; pass_ms = the count,
        the bitmaps, the emit, the searches, the fold, the records."""
        _fields_ = [("points", ctypes.c_uint64), ("blocks", ctypes.c_uint32), ("blocks_looked", ctypes.c_uint32), ("lookups", ctypes.c_uint64),
                    ("searches", ctypes.c_uint64), ("visited", ctypes.c_uint64), ("kernel_ms", ctypes.c_float), ("total_ms", ctypes.c_float),
                    ("pass_ms", ctypes.c_float * 6)]


    assert (ctypes.sizeof(PenetrationOptions), ctypes.sizeof(Penetration), ctypes.sizeof(PenetrationStats)) == (28, 64, 72)


    class GapOptions(ctypes.Structure):
        """sdfhip_gap_options: flags GAP_NO_PRUNE or 0; limit in [0, +inf]: only the pairs whose gap is <= limit have a record."""
        _fields_ = [("size", ctypes.c_uint32), ("flags", ctypes.c_uint32), ("limit", ctypes.c_float)]

        def __init__(self, flags=0, limit=float("inf")):
            super().__init__(ctypes.sizeof(type(self)), int(flags), float(limit))


    class Gap(ctypes.Structure):
        """sdfhip_gap: one pair a < b of instances whose surfaces lie within the limit, how far apart they are and the two closest
        points (sdfhip_instances_gap)."""
        _fields_ = [("a", ctypes.c_uint32), ("b", ctypes.c_uint32), ("gap", ctypes.c_float), ("flags", ctypes.c_uint32),
                    ("node_a", ctypes.c_uint32), ("node_b", ctypes.c_uint32), ("corner", ctypes.c_uint32), ("point_a", ctypes.c_float * 3),
                    ("point_b", ctypes.c_float * 3), ("pad_", ctypes.c_uint32 * 3)]


    class GapStats(ctypes.Structure):
        """sdfhip_gap_stats: the pairs of the list and those searched, the (ordered pair, cut cell) lanes, the vertex searches run and
        the node records they loaded (both differ from call to call unless GAP_NO_PRUNE); pass_ms = the cell lists, the bitmaps, the
        searches, the records."""
        _fields_ = [("pairs", ctypes.c_uint32), ("pairs_searched", ctypes.c_uint32), ("cells", ctypes.c_uint64), ("searches", ctypes.c_uint64),
                    ("visited", ctypes.c_uint64), ("kernel_ms", ctypes.c_float), ("total_ms", ctypes.c_float), ("pass_ms", ctypes.c_float * 4)]


    assert (ctypes.sizeof(GapOptions), ctypes.sizeof(Gap), ctypes.sizeof(GapStats)) == (12, 64, 56)


    class ComponentsOptions(ctypes.Structure):
        """sdfhip_components_options: flags 0; depth 0..9 (2^depth lattice points along each axis); the cube's origin and side
        (finite, above 0)."""
        _fields_ = [("size", ctypes.c_uint32), ("flags", ctypes.c_uint32), ("depth", ctypes.c_uint32), ("origin", ctypes.c_float * 3),
                    ("side", ctypes.c_float)]

        def __init__(self, flags=0, depth=6, origin=(0.0, 0.0, 0.0), side=1.0):
            super().__init__(ctypes.sizeof(type(self)), int(flags), int(depth), (ctypes.c_float * 3)(*[float(x) for x in origin]), float(side))


    class Component(ctypes.Structure):
        """sdfhip_component: one face-connected component of a scene on a lattice (sdfhip_scene_components); flags COMPONENT_SOLID for
        the inside phase, 0 for a void."""
        _fields_ = [("label", ctypes.c_uint32), ("flags", ctypes.c_uint32), ("points", ctypes.c_uint32), ("reserved", ctypes.c_uint32),
                    ("lo", ctypes.c_uint32 * 3), ("hi", ctypes.c_uint32 * 3), ("sum", ctypes.c_uint64 * 3)]


    class ComponentsStats(ctypes.Structure):
        """sdfhip_components_stats: points = 8^depth, inside = those with value < 0, the records and the solids among them."""
        _fields_ = [("points", ctypes.c_uint64), ("inside", ctypes.c_uint64), ("components", ctypes.c_uint32), ("solids", ctypes.c_uint32),
                    ("kernel_ms", ctypes.c_float), ("total_ms", ctypes.c_float)]


    assert (ctypes.sizeof(ComponentsOptions), ctypes.sizeof(Component), ctypes.sizeof(ComponentsStats)) == (28, 64, 32)


    class SelectOptions(ctypes.Structure):
        """sdfhip_select_options: flags = SELECT_* rule bits, OR-ed; lattice_depth 0..9 and the cube's origin and side, as
        ComponentsOptions; depth None = the source's depth, else 0..12; min_points: SELECT_DROP_SMALL_SOLIDS' threshold."""
        _fields_ = [("size", ctypes.c_uint32), ("flags", ctypes.c_uint32), ("lattice_depth", ctypes.c_uint32), ("origin", ctypes.c_float * 3),
                    ("side", ctypes.c_float), ("depth", ctypes.c_int32), ("min_points", ctypes.c_uint32)]

        def __init__(self, flags=0, lattice_depth=6, origin=(0.0, 0.0, 0.0), side=1.0, depth=None, min_points=0):
            super().__init__(ctypes.sizeof(type(self)), int(flags), int(lattice_depth), (ctypes.c_float * 3)(*[float(x) for x in origin]), float(side),
                             -1 if depth is None else int(depth), int(min_points))


    class SelectStats(ctypes.Structure):
        """sdfhip_select_stats: the lattice's records and which of them flipped; the result's tree as PlaceStats has it; the times."""
        _fields_ = [("components", ctypes.c_uint32), ("solids", ctypes.c_uint32), ("flipped_solids", ctypes.c_uint32),
                    ("flipped_voids", ctypes.c_uint32), ("points_flipped", ctypes.c_uint64), ("nodes_in", ctypes.c_uint32),
                    ("nodes_out", ctypes.c_uint32), ("depth_out", ctypes.c_uint32), ("levels", ctypes.c_uint32), ("samples", ctypes.c_uint64),
                    ("label_ms", ctypes.c_float), ("kernel_ms", ctypes.c_float), ("scene_ms", ctypes.c_float), ("total_ms", ctypes.c_float)]


    assert (ctypes.sizeof(SelectOptions), ctypes.sizeof(SelectStats)) == (36, 64)


    class MeshOptions(ctypes.Structure):
        """sdfhip_mesh_options: level -1 = the leaves (full detail), 0..12 = the level-of-detail mesh of that level."""
        _fields_ = [("size", ctypes.c_uint32), ("level", ctypes.c_int32)]

        def __init__(self, level=-1):
            super().__init__(ctypes.sizeof(type(self)), int(level))


    class CMesh(ctypes.Structure):
        _fields_ = [("n_triangles", ctypes.c_uint32), ("verts6", ctypes.POINTER(ctypes.c_float))]


    class MeshStats(ctypes.Structure):
        _fields_ = [("nodes", ctypes.c_uint32), ("cells", ctypes.c_uint32), ("cells_cut", ctypes.c_uint32), ("n_triangles", ctypes.c_uint32),
                    ("kernel_ms", ctypes.c_float), ("total_ms", ctypes.c_float)]


    class MeasureOptions(ctypes.Structure):
        """sdfhip_measure_options: level as MeshOptions"""
        _fields_ = [("size", ctypes.c_uint32), ("level", ctypes.c_int32)]

        def __init__(self, level=-1):
            super().__init__(ctypes.sizeof(type(self)), int(level))


    class Measure(ctypes.Structure):
        """sdfhip_measure: volume, area, first and second moments about the origin, the tight bounds and the cell counts of the solid a
        scene describes (Scene.Measure) -- the solid the bytes describe and the renderer draws."""
        _fields_ = [("volume", ctypes.c_double), ("area", ctypes.c_double), ("moment1", ctypes.c_double * 3), ("moment2", ctypes.c_double * 6),
                    ("bounds_min", ctypes.c_double * 3), ("bounds_max", ctypes.c_double * 3), ("nodes", ctypes.c_uint32), ("depth", ctypes.c_uint32),
                    ("cells", ctypes.c_uint32), ("cells_cut", ctypes.c_uint32), ("cells_inside", ctypes.c_uint32),
                    ("cells_at_depth", ctypes.c_uint32 * 13), ("kernel_ms", ctypes.c_float), ("total_ms", ctypes.c_float)]

        @property
        def empty(self):
            return not self.volume > 0.0

        @property
        def centroid(self):
            """moment1 / volume as three floats, or None for an empty solid"""
            if self.empty:
                return None
            return tuple(m / self.volume for m in self.moment1)

        def inertia(self):
            """The 3 x 3 inertia tensor about the centroid at unit density (nested tuples, rows x y z): the second moments about the
            origin moved to the centroid by the parallel-axis theorem, then I_aa = the other two central moments' sum, I_ab = -the
            central product.  None for an empty solid."""
            if self.empty:
                return None
            V = self.volume
            c = self.centroid
            xx, yy, zz, xy, xz, yz = self.moment2
            cxx, cyy, czz = xx - V * c[0] * c[0], yy - V * c[1] * c[1], zz - V * c[2] * c[2]
            cxy, cxz, cyz = xy - V * c[0] * c[1], xz - V * c[0] * c[2], yz - V * c[1] * c[2]
            return ((cyy + czz, -cxy, -cxz), (-cxy, cxx + czz, -cyz), (-cxz, -cyz, cxx + cyy))


    assert (ctypes.sizeof(MeasureOptions), ctypes.sizeof(Measure)) == (8, 216)


    class SliceOptions(ctypes.Structure):
        """sdfhip_slice_options: plane k is dot(normal, p) = offset + k * pitch, k = 0 .. layers - 1 (the normal as given, never
        normalised); level as MeshOptions."""
        _fields_ = [("size", ctypes.c_uint32), ("level", ctypes.c_int32), ("normal", ctypes.c_float * 3), ("offset", ctypes.c_float),
                    ("pitch", ctypes.c_float), ("layers", ctypes.c_uint32)]

        def __init__(self, normal=(0.0, 0.0, 1.0), offset=0.5, pitch=0.0, layers=1, level=-1):
            super().__init__(ctypes.sizeof(type(self)), int(level), (ctypes.c_float * 3)(*[float(x) for x in normal]), float(offset), float(pitch),
                             int(layers))


    class Segment(ctypes.Structure):
        """sdfhip_segment: from a to b the solid lies on the left, seen from the tip of the normal"""
        _fields_ = [("a", ctypes.c_float * 3), ("layer", ctypes.c_uint32), ("b", ctypes.c_float * 3), ("node", ctypes.c_uint32)]


    class CSlice(ctypes.Structure):
        _fields_ = [("n_segments", ctypes.c_uint32), ("segments", ctypes.POINTER(Segment)), ("layers", ctypes.c_uint32),
                    ("layer_counts", ctypes.POINTER(ctypes.c_uint32))]


    class SliceStats(ctypes.Structure):
        _fields_ = [("nodes", ctypes.c_uint32), ("cells", ctypes.c_uint32), ("cells_cut", ctypes.c_uint32), ("cells_crossed", ctypes.c_uint32),
                    ("n_segments", ctypes.c_uint32), ("kernel_ms", ctypes.c_float), ("total_ms", ctypes.c_float)]


    assert (ctypes.sizeof(SliceOptions), ctypes.sizeof(Segment), ctypes.sizeof(CSlice), ctypes.sizeof(SliceStats)) == (32, 32, 32, 28)


    class TriMeshOptions(ctypes.Structure):
        """sdfhip_trimesh_options: fit 0 = coordinates as given, 1 = bounding box centred at 0.5 with its longest side `fill` (None = default)."""
        _fields_ = [("size", ctypes.c_uint32), ("fit", ctypes.c_int32), ("fill", ctypes.c_float)]

        def __init__(self, fit=None, fill=None):
            super().__init__(ctypes.sizeof(type(self)), -1 if fit is None else int(fit), -1.0 if fill is None else float(fill))


    class CTriMesh(ctypes.Structure):
        _fields_ = [("n_records", ctypes.c_uint32), ("records", ctypes.POINTER(ctypes.c_float)), ("n_vertices", ctypes.c_uint32),
                    ("n_edges", ctypes.c_uint32), ("n_dropped", ctypes.c_uint32), ("open_edges", ctypes.c_uint32), ("scale", ctypes.c_float),
                    ("offset", ctypes.c_float * 3)]


    class TriMeshStats(ctypes.Structure):
        _fields_ = [("nodes", ctypes.c_uint32), ("levels", ctypes.c_uint32), ("records", ctypes.c_uint32), ("pad_", ctypes.c_uint32),
                    ("candidate_entries", ctypes.c_uint64), ("build_ms", ctypes.c_float), ("scene_ms", ctypes.c_float),
                    ("total_ms", ctypes.c_float), ("pad1_", ctypes.c_uint32)]


    assert (ctypes.sizeof(TriMeshOptions), ctypes.sizeof(TriMeshStats)) == (12, 40)


    class SdfHipError(RuntimeError):
        def __init__(self, code, message):
            super().__init__(f"sdfhip error {code}: {message}")
            self.code = code


_c = ctypes
_vp = ctypes.c_void_p
_SIG = {
    "sdfhip_last_error": (_c.c_char_p, []),
    "sdfhip_asdf_load": (_c.c_int, [_c.c_char_p, _c.POINTER(COctData)]),
    "sdfhip_asdf_save": (_c.c_int, [_c.POINTER(COctData), _c.c_char_p]),
    "sdfhip_octdata_free": (None, [_c.POINTER(COctData)]),
    "sdfhip_generate": (_c.c_int, [_c.c_int, _c.POINTER(_c.c_float), _c.c_int, _c.c_int, _c.c_int,
                                   _c.POINTER(COctData)]),
    "sdfhip_load_ply": (_c.c_int, [_c.c_char_p, _c.POINTER(CPoints)]),
    "sdfhip_load_obj": (_c.c_int, [_c.c_char_p, _c.POINTER(CPoints)]),
    "sdfhip_points_free": (None, [_c.POINTER(CPoints)]),
    "sdfhip_sdfgen": (_c.c_int, [_c.c_int, _vp, _c.c_uint32, _c.c_int32, _c.POINTER(COctData),
                                 _c.POINTER(SdfGenStats)]),
    "sdfhip_sdfgen_scene": (_c.c_int, [_c.c_int, _vp, _c.c_uint32, _c.c_int32, _c.POINTER(_vp), _c.POINTER(COctData),
                                       _c.POINTER(SdfGenStats)]),
    "sdfhip_sdfgen_trim": (_c.c_int, []),
    "sdfhip_octdata_validate": (_c.c_int, [_vp, _c.c_uint32, _c.POINTER(_c.c_uint32),
                                           _c.POINTER(_c.c_int)]),
    "sdfhip_info_default": (None, [_c.POINTER(Info), _c.c_float, _c.c_float]),
    "sdfhip_info_set_heading": (None, [_c.POINTER(Info), _c.c_float, _c.c_float]),
    "sdfhip_info_set_position": (None, [_c.POINTER(Info), _c.c_float, _c.c_float, _c.c_float]),
    "sdfhip_device_count": (_c.c_int, [_c.POINTER(_c.c_int)]),
    "sdfhip_device_pci_bus_id": (_c.c_int, [_c.c_int, _c.c_char_p, _c.c_uint32]),
    "sdfhip_device_bandwidth": (_c.c_int, [_c.c_int, _c.c_uint64, _c.c_uint32, _c.POINTER(_c.c_double), _c.POINTER(_c.c_double), _c.POINTER(_c.c_double)]),
    "sdfhip_multi_selftest": (_c.c_int, [_vp, _c.POINTER(MultiLink)]),
    "sdfhip_scene_upload": (_c.c_int, [_c.c_int, _vp, _vp, _c.c_uint32, _c.POINTER(_vp)]),
    "sdfhip_upload_options_default": (None, [_c.POINTER(UploadOptions)]),
    "sdfhip_scene_upload_ex": (_c.c_int, [_c.c_int, _vp, _vp, _c.c_uint32, _c.POINTER(UploadOptions), _c.POINTER(_vp)]),
    "sdfhip_scene_free": (_c.c_int, [_vp]),
    "sdfhip_scene_info": (_c.c_int, [_vp, _c.POINTER(_c.c_uint32), _c.POINTER(_c.c_uint32),
                                     _c.POINTER(_c.c_int), _c.POINTER(_c.c_int)]),
    "sdfhip_render": (_c.c_int, [_vp, _c.POINTER(Info), _c.c_uint32, _c.c_uint32, _c.c_uint32, _vp,
                                 _c.POINTER(Stats)]),
    "sdfhip_render_device": (_c.c_int, [_vp, _c.POINTER(Info), _c.c_uint32, _c.c_uint32,
                                        _c.c_uint32, _c.c_uint32, _c.c_uint32, _c.c_uint32,
                                        _c.c_uint32, _vp, _vp, _c.POINTER(Stats)]),
    "sdfhip_render_batch_device": (_c.c_int, [_vp, _c.POINTER(Info), _c.c_uint32, _c.c_uint32, _c.c_uint32,
                                              _c.c_uint32, _c.c_uint32, _c.c_uint32, _c.c_uint32,
                                              _c.c_uint32, _vp, _vp, _c.POINTER(Stats)]),
    "sdfhip_scene_prepare_path": (_c.c_int, [_vp]),
    "sdfhip_render_path": (_c.c_int, [_vp, _c.POINTER(Info), _c.POINTER(PathTrace), _c.c_uint32, _c.c_uint32,
                                      _c.c_uint32, _vp, _c.POINTER(Stats)]),
    "sdfhip_render_path_device": (_c.c_int, [_vp, _c.POINTER(Info), _c.POINTER(PathTrace), _c.c_uint32,
                                             _c.c_uint32, _c.c_uint32, _c.c_uint32, _c.c_uint32,
                                             _c.c_uint32, _c.c_uint32, _vp, _vp, _c.POINTER(Stats)]),
    "sdfhip_render_display": (_c.c_int, [_vp, _c.POINTER(Info), _c.c_uint32, _c.c_uint32, _c.c_uint32,
                                         _c.c_int, _vp, _c.POINTER(Stats)]),
    "sdfhip_host_alloc": (_c.c_int, [_c.c_uint64, _c.POINTER(_vp)]),
    "sdfhip_host_register": (_c.c_int, [_vp, _c.c_uint64]),
    "sdfhip_host_release": (_c.c_int, [_vp]),
    "sdfhip_deinterleave_device": (_c.c_int, [_c.c_int, _vp, _vp, _c.c_uint32, _c.c_uint32,
                                              _c.c_uint32, _c.c_uint32, _c.c_uint32, _c.c_uint32, _c.c_uint32, _vp]),
    "sdfhip_camera_update": (None, [_c.POINTER(Info), _c.POINTER(_c.c_float), _c.c_float, _c.c_uint32, _c.c_float]),
    "sdfhip_camera_mouse_move": (None, [_c.POINTER(Info), _c.POINTER(_c.c_float), _c.c_float, _c.c_float]),
    "sdfhip_camera_mouse_wheel": (_c.c_float, [_c.c_float, _c.c_float]),
    "sdfhip_scene_edit": (_c.c_int, [_vp, _c.POINTER(Edit), _c.c_uint32, _c.c_int32, _c.POINTER(_vp), _c.POINTER(COctData),
                                     _c.POINTER(EditStats)]),
    "sdfhip_scene_prune": (_c.c_int, [_vp, _c.POINTER(PruneOptions), _c.POINTER(_vp), _c.POINTER(COctData), _c.POINTER(PruneStats)]),
    "sdfhip_scene_combine": (_c.c_int, [_vp, _vp, _c.c_int32, _c.POINTER(CombineOptions), _c.POINTER(_vp), _c.POINTER(COctData), _c.POINTER(CombineStats)]),
    "sdfhip_scene_place": (_c.c_int, [_vp, _c.POINTER(Placement), _c.POINTER(_vp), _c.POINTER(COctData), _c.POINTER(PlaceStats)]),
    "sdfhip_scene_compose": (_c.c_int, [_c.POINTER(Instance), _c.c_uint32, _c.POINTER(ComposeOptions), _c.POINTER(_vp), _c.POINTER(COctData), _c.POINTER(ComposeStats)]),
    "sdfhip_volume_build": (_c.c_int, [_c.c_int, _vp, _c.POINTER(Volume), _c.POINTER(_vp), _c.POINTER(COctData), _c.POINTER(VolumeStats)]),
    "sdfhip_volume_build_device": (_c.c_int, [_c.c_int, _vp, _c.POINTER(Volume), _c.POINTER(_vp), _c.POINTER(COctData), _c.POINTER(VolumeStats)]),
    "sdfhip_scene_volume": (_c.c_int, [_vp, _c.POINTER(Volume), _vp]),
    "sdfhip_scene_volume_device": (_c.c_int, [_vp, _c.POINTER(Volume), _vp, _vp]),
    "sdfhip_scene_distance": (_c.c_int, [_vp, _vp, _c.c_uint32, _c.c_int32, _vp]),
    "sdfhip_scene_distance_device": (_c.c_int, [_vp, _vp, _c.c_uint32, _c.c_int32, _vp, _vp]),
    "sdfhip_scene_offset": (_c.c_int, [_vp, _c.POINTER(OffsetOptions), _c.POINTER(_vp), _c.POINTER(COctData), _c.POINTER(OffsetStats)]),
    "sdfhip_scene_blend": (_c.c_int, [_vp, _vp, _c.POINTER(BlendOptions), _c.POINTER(_vp), _c.POINTER(COctData), _c.POINTER(BlendStats)]),
    "sdfhip_scene_sample": (_c.c_int, [_vp, _vp, _c.c_uint32, _vp]),
    "sdfhip_scene_sample_device": (_c.c_int, [_vp, _vp, _c.c_uint32, _vp, _vp]),
    "sdfhip_scene_raycast": (_c.c_int, [_vp, _vp, _c.c_uint32, _c.c_float, _c.c_float, _c.c_uint32, _vp]),
    "sdfhip_scene_raycast_device": (_c.c_int, [_vp, _vp, _c.c_uint32, _c.c_float, _c.c_float, _c.c_uint32, _vp, _vp]),
    "sdfhip_scene_pick": (_c.c_int, [_vp, _c.POINTER(Info), _vp, _c.c_uint32, _c.c_uint32, _vp]),
    "sdfhip_instances_sample": (_c.c_int, [_c.POINTER(Instance), _c.c_uint32, _c.POINTER(InstancesOptions), _vp, _c.c_uint32, _vp]),
    "sdfhip_instances_sample_device": (_c.c_int, [_c.POINTER(Instance), _c.c_uint32, _c.POINTER(InstancesOptions), _vp, _c.c_uint32, _vp, _vp]),
    "sdfhip_instances_raycast": (_c.c_int, [_c.POINTER(Instance), _c.c_uint32, _c.POINTER(InstancesOptions), _vp, _c.c_uint32, _c.c_float, _c.c_float, _vp]),
    "sdfhip_instances_raycast_device": (_c.c_int, [_c.POINTER(Instance), _c.c_uint32, _c.POINTER(InstancesOptions), _vp, _c.c_uint32, _c.c_float, _c.c_float,
                                                   _vp, _vp]),
    "sdfhip_instances_pick": (_c.c_int, [_c.POINTER(Instance), _c.c_uint32, _c.POINTER(InstancesOptions), _c.POINTER(Info), _vp, _c.c_uint32, _vp]),
    "sdfhip_instances_render": (_c.c_int, [_c.POINTER(Instance), _c.c_uint32, _c.POINTER(InstancesOptions), _c.POINTER(Info), _c.c_uint32, _c.c_uint32, _vp]),
    "sdfhip_instances_render_device": (_c.c_int, [_c.POINTER(Instance), _c.c_uint32, _c.POINTER(InstancesOptions), _c.POINTER(Info), _c.c_uint32, _c.c_uint32,
                                                  _vp, _vp]),
    "sdfhip_clash_options_default": (None, [_c.POINTER(ClashOptions)]),
    "sdfhip_instances_clash": (_c.c_int, [_c.POINTER(Instance), _c.c_uint32, _c.POINTER(ClashOptions), _vp, _c.c_uint32, _c.POINTER(_c.c_uint32),
                                          _c.POINTER(ClashStats)]),
    "sdfhip_penetration_options_default": (None, [_c.POINTER(PenetrationOptions)]),
    "sdfhip_instances_penetration": (_c.c_int, [_c.POINTER(Instance), _c.c_uint32, _c.POINTER(PenetrationOptions), _vp, _c.c_uint32,
                                                _c.POINTER(_c.c_uint32), _c.POINTER(PenetrationStats)]),
    "sdfhip_gap_options_default": (None, [_c.POINTER(GapOptions)]),
    "sdfhip_instances_gap": (_c.c_int, [_c.POINTER(Instance), _c.c_uint32, _c.POINTER(GapOptions), _vp, _c.c_uint32, _c.POINTER(_c.c_uint32),
                                        _c.POINTER(GapStats)]),
    "sdfhip_components_options_default": (None, [_c.POINTER(ComponentsOptions)]),
    "sdfhip_scene_components": (_c.c_int, [_vp, _c.POINTER(ComponentsOptions), _vp, _c.c_uint32, _c.POINTER(_c.c_uint32), _vp,
                                           _c.POINTER(ComponentsStats)]),
    "sdfhip_scene_components_device": (_c.c_int, [_vp, _c.POINTER(ComponentsOptions), _vp, _c.c_uint32, _c.POINTER(_c.c_uint32), _vp,
                                                  _c.POINTER(ComponentsStats)]),
    "sdfhip_select_options_default": (None, [_c.POINTER(SelectOptions)]),
    "sdfhip_scene_select": (_c.c_int, [_vp, _c.POINTER(SelectOptions), _vp, _c.c_uint32, _c.POINTER(_vp), _c.POINTER(COctData), _c.POINTER(SelectStats)]),
    "sdfhip_mesh_options_default": (None, [_c.POINTER(MeshOptions)]),
    "sdfhip_scene_mesh": (_c.c_int, [_vp, _c.POINTER(MeshOptions), _c.POINTER(CMesh), _c.POINTER(MeshStats)]),
    "sdfhip_scene_mesh_device": (_c.c_int, [_vp, _c.POINTER(MeshOptions), _vp, _c.c_uint32, _c.POINTER(_c.c_uint32), _vp]),
    "sdfhip_mesh_free": (None, [_c.POINTER(CMesh)]),
    "sdfhip_measure_options_default": (None, [_c.POINTER(MeasureOptions)]),
    "sdfhip_scene_measure": (_c.c_int, [_vp, _c.POINTER(MeasureOptions), _c.POINTER(Measure)]),
    "sdfhip_slice_options_default": (None, [_c.POINTER(SliceOptions)]),
    "sdfhip_scene_slice": (_c.c_int, [_vp, _c.POINTER(SliceOptions), _c.POINTER(CSlice), _c.POINTER(SliceStats)]),
    "sdfhip_scene_slice_device": (_c.c_int, [_vp, _c.POINTER(SliceOptions), _vp, _c.c_uint32, _vp, _c.POINTER(_c.c_uint32), _vp]),
    "sdfhip_slice_free": (None, [_c.POINTER(CSlice)]),
    "sdfhip_mesh_save_ply": (_c.c_int, [_c.POINTER(CMesh), _c.c_char_p]),
    "sdfhip_mesh_save_obj": (_c.c_int, [_c.POINTER(CMesh), _c.c_char_p]),
    "sdfhip_load_ply_mesh": (_c.c_int, [_c.c_char_p, _c.POINTER(CMesh)]),
    "sdfhip_load_obj_mesh": (_c.c_int, [_c.c_char_p, _c.POINTER(CMesh)]),
    "sdfhip_trimesh_options_default": (None, [_c.POINTER(TriMeshOptions)]),
    "sdfhip_trimesh_prepare": (_c.c_int, [_vp, _c.c_uint32, _c.c_uint32, _c.POINTER(TriMeshOptions), _c.POINTER(CTriMesh)]),
    "sdfhip_trimesh_free": (None, [_c.POINTER(CTriMesh)]),
    "sdfhip_trimesh_build": (_c.c_int, [_c.c_int, _c.POINTER(CTriMesh), _c.c_int32, _c.POINTER(_vp), _c.POINTER(COctData),
                                        _c.POINTER(TriMeshStats)]),
    "sdfhip_scene_top_grid": (_c.c_int, [_vp, _c.POINTER(_c.c_int32), _c.POINTER(_c.c_uint64)]),
    "sdfhip_render_bands_device": (_c.c_int, [_vp, _c.POINTER(Info), _c.c_uint32, _c.POINTER(PathTrace), _c.c_uint32,
                                              _c.c_uint32, _c.c_uint32, _c.POINTER(_c.c_uint16), _c.c_uint32,
                                              _c.c_uint32, _c.c_uint32, _vp, _vp, _c.POINTER(Stats)]),
    "sdfhip_deinterleave_bands_device": (_c.c_int, [_c.c_int, _vp, _vp, _c.c_uint32, _c.c_uint32, _c.c_uint32,
                                                    _c.c_uint32, _c.c_uint32, _c.POINTER(_c.c_uint8), _c.c_uint32,
                                                    _c.c_uint32, _vp]),
    "sdfhip_sparse2_bytes": (_c.c_uint64, [_c.c_uint32, _c.c_uint32, _c.c_uint32, _c.c_uint32]),
    "sdfhip_sparse2_floats_offset": (_c.c_uint64, [_c.c_uint32, _c.c_uint32, _c.c_uint32]),
    "sdfhip_render_sparse_device": (_c.c_int, [_vp, _c.POINTER(Info), _c.c_uint32, _c.c_uint32, _c.c_uint32, _c.c_uint32,
                                               _c.POINTER(_c.c_uint16), _c.c_uint32, _c.c_uint32, _c.c_uint32, _c.c_uint32, _c.c_uint32, _vp, _vp]),
    "sdfhip_deinterleave_sparse2_device": (_c.c_int, [_c.c_int, _c.POINTER(_vp), _vp, _c.c_uint32, _c.c_uint32, _c.c_uint32,
                                                      _c.c_uint32, _c.c_uint32, _c.POINTER(_c.c_uint8), _c.c_uint32, _c.c_uint32,
                                                      _c.c_uint32, _c.c_int, _vp, _vp]),
    "sdfhip_multi_create": (_c.c_int, [_c.POINTER(_c.c_int), _c.c_uint32, _vp, _vp, _c.c_uint32, _c.POINTER(_vp)]),
    "sdfhip_multi_free": (_c.c_int, [_vp]),
    "sdfhip_multi_configure": (_c.c_int, [_vp, _c.c_uint32, _c.c_float]),
    "sdfhip_multi_info": (_c.c_int, [_vp, _c.POINTER(_c.c_uint32), _c.POINTER(_c.c_int), _c.POINTER(_c.c_uint32),
                                     _c.POINTER(_c.c_float), _c.POINTER(_c.c_int)]),
    "sdfhip_multi_render": (_c.c_int, [_vp, _c.POINTER(Info), _c.c_uint32, _c.c_uint32, _c.c_uint32, _vp, _c.POINTER(MultiStats)]),
    "sdfhip_multi_render_path": (_c.c_int, [_vp, _c.POINTER(Info), _c.POINTER(PathTrace), _c.c_uint32, _c.c_uint32, _c.c_uint32,
                                            _vp, _c.POINTER(MultiStats)]),
    "sdfhip_multi_submit": (_c.c_int, [_vp, _c.c_uint32, _c.POINTER(Info), _c.c_uint32, _c.c_uint32, _c.c_uint32, _c.c_uint32, _vp]),
    "sdfhip_multi_submit_path": (_c.c_int, [_vp, _c.c_uint32, _c.POINTER(Info), _c.POINTER(PathTrace), _c.c_uint32, _c.c_uint32,
                                            _c.c_uint32, _vp]),
    "sdfhip_multi_wait": (_c.c_int, [_vp, _c.c_uint32, _c.POINTER(_vp), _c.POINTER(MultiStats)]),
}
# include/sdfhip_experimental.h: exported by the experiments flavour only
_SIG_LAB = {
    "sdfhip_debug_tile_order": (_c.c_int, [_vp, _vp, _vp]),
    "sdfhip_debug_unorm_table": (_c.c_int, [_c.c_int, _vp]),
    "sdfhip_debug_step_classes": (_c.c_int, [_vp, _vp, _c.POINTER(_c.c_uint64)]),
    "sdfhip_multi_debug_floats_sent": (_c.c_int, [_vp, _c.c_uint32]),
    "sdfhip_debug_fail_host_allocations": (_c.c_int, [_c.c_int64, _c.POINTER(_c.c_uint64)]),
    "sdfhip_debug_touch_begin": (_c.c_int, [_vp]),
    "sdfhip_debug_touch_end": (_c.c_int, [_vp, _c.POINTER(_c.c_uint64), _c.c_uint32, _c.POINTER(_c.c_uint32), _c.POINTER(_c.c_uint64)]),
}
# every symbol include/sdfhip.h declares must be exported: fail at import otherwise
for _name, (_res, _args) in _SIG.items():
    _fn = getattr(lib, _name)
    _fn.restype = _res
    _fn.argtypes = _args
EXPERIMENTS = hasattr(lib, "sdfhip_debug_unorm_table")       # libsdfhip_lab.so: then every symbol of sdfhip_experimental.h must be there
if EXPERIMENTS:
    for _name, (_res, _args) in _SIG_LAB.items():
        _fn = getattr(lib, _name)
        _fn.restype = _res
        _fn.argtypes = _args

EXPORTED_SYMBOLS = tuple(_SIG)
EXPERIMENTAL_SYMBOLS = tuple(_SIG_LAB)


def need_lab(what):
    if not EXPERIMENTS:
        raise RuntimeError(f"{what} is part of the experiments build (include/sdfhip_experimental.h): load libsdfhip_lab.so "
                           "(sdfbox_amd.lab.load(), or SDFHIP_LIB=sdfbox_amd/libsdfhip_lab.so)")



def check(code):
    if code != OK:
        raise SdfHipError(code, lib.sdfhip_last_error().decode("utf-8", "replace"))
