"""sdfbox_amd -- MI355X (gfx950) sphere tracing of adaptively sampled distance
fields behind SdfBox's frame boundary.  The compute lives in libsdfhip.so
(hand-written HIP, C ABI in include/sdfhip.h); this package is the host-side
mirror of the reference's interface for that path: OctData (.asdf), Logic
(camera -> Info), Scene.Draw (Program.Draw's compute pass).
"""
from . import _lib, tiles
from ._lib import (VOLUME_F16, VOLUME_F32, Volume, VolumeStats, BRUSH_BOX, BRUSH_SPHERE, COMBINE_INTERSECT, COMBINE_SUBTRACT, COMBINE_UNION, CombineOptions, CombineStats, EDIT_ADD, EDIT_CARVE, FLAG_COMPACT, FLAG_COUNT, FLAG_DISPLAY, FLAG_DISPLAY_DEBUG, FLAG_TILE_ORDER, FLAG_WIRE, KERNEL_AUTO, KERNEL_GENERIC, KERNEL_STACK, QUERY_ESCAPED, QUERY_EXHAUSTED, QUERY_HIT, QUERY_INVALID, TUNE_ONE_KERNEL, TUNE_SHADOW_QUEUE, Edit, EditStats, PruneOptions, PruneStats, Placement, PlaceStats, Instance, ComposeOptions, ComposeStats, INSTANCES_NO_SKIP, InstancesOptions, PartProbe, PartHit, CLASH_NO_SKIP, CLASH_MAX_INSTANCES, ClashOptions, Clash, ClashStats, PENETRATION_NO_SKIP, GAP_NO_PRUNE, GAP_WITNESS_OF_B, GAP_CONTAINED, GapOptions, Gap, GapStats, PenetrationOptions, Penetration, PenetrationStats, COMPONENT_SOLID, COMPONENTS_MAX_DEPTH, ComponentsOptions, Component, ComponentsStats, SELECT_KEEP_LARGEST_SOLID, SELECT_DROP_SMALL_SOLIDS, SELECT_FILL_ENCLOSED_VOIDS, SELECT_FLIP_LISTED, SELECT_KEEP_LISTED, SelectOptions, SelectStats, OFFSET_GROW, OFFSET_SHELL, Clearance, OffsetOptions, OffsetStats, BLEND_UNION, BLEND_INTERSECT, BLEND_SUBTRACT, BLEND_MORPH, BlendOptions, BlendStats,
                   Hit, Info, Measure, MeasureOptions, MeshOptions, MeshStats, SliceOptions, SliceStats, Segment, MultiStats, TriMeshOptions, TriMeshStats, PathTrace, Probe, Ray, SdfHipError, Stats)
from .logic import Logic
from .octdata import OctData, dragon_standin, knot_point_cloud, sphere_d4, torus_d6, write_ply
from .slices import slice_areas, slice_basis, slice_loops
from .renderer import HostFrame, LoadMeshObj, LoadMeshPly, MultiScene, SaveMeshObj, SaveMeshPly, Scene, TriMesh, lattice_of_depth, clash_volume, clash_centroid, clash_box, penetration_push, gap_vector, component_volume, component_centroid, component_box, component_enclosed, placement, placement_fit, linear_array, circular_array, device_bandwidth, device_count, device_pci_bus_id, sdfgen_trim, unorm_table

__all__ = [
    "BRUSH_BOX", "BRUSH_SPHERE", "EDIT_ADD", "EDIT_CARVE", "Edit", "EditStats", "PruneOptions", "PruneStats",
    "COMBINE_UNION", "COMBINE_INTERSECT", "COMBINE_SUBTRACT", "CombineOptions", "CombineStats", "Placement", "PlaceStats", "placement", "placement_fit", "Instance", "ComposeOptions", "ComposeStats", "linear_array", "circular_array", "VOLUME_F32", "VOLUME_F16", "Volume", "VolumeStats", "lattice_of_depth", "Measure", "MeasureOptions",
    "OFFSET_GROW", "OFFSET_SHELL", "Clearance", "OffsetOptions", "OffsetStats",
    "BLEND_UNION", "BLEND_INTERSECT", "BLEND_SUBTRACT", "BLEND_MORPH", "BlendOptions", "BlendStats",
    "QUERY_HIT", "QUERY_ESCAPED", "QUERY_EXHAUSTED", "QUERY_INVALID", "Probe", "Ray", "Hit",
    "INSTANCES_NO_SKIP", "InstancesOptions", "PartProbe", "PartHit",
    "CLASH_NO_SKIP", "CLASH_MAX_INSTANCES", "ClashOptions", "Clash", "ClashStats", "clash_volume", "clash_centroid", "clash_box",
    "PENETRATION_NO_SKIP", "PenetrationOptions", "Penetration", "PenetrationStats", "penetration_push",
    "GAP_NO_PRUNE", "GAP_WITNESS_OF_B", "GAP_CONTAINED", "GapOptions", "Gap", "GapStats", "gap_vector",
    "COMPONENT_SOLID", "COMPONENTS_MAX_DEPTH", "ComponentsOptions", "Component", "ComponentsStats", "component_volume", "component_centroid", "component_box", "component_enclosed",
    "SELECT_KEEP_LARGEST_SOLID", "SELECT_DROP_SMALL_SOLIDS", "SELECT_FILL_ENCLOSED_VOIDS", "SELECT_FLIP_LISTED", "SELECT_KEEP_LISTED", "SelectOptions", "SelectStats",
    "SliceOptions", "SliceStats", "Segment", "slice_basis", "slice_areas", "slice_loops",
    "MeshOptions", "MeshStats", "SaveMeshPly", "SaveMeshObj", "LoadMeshPly", "LoadMeshObj", "TriMesh", "TriMeshOptions", "TriMeshStats",
    "FLAG_COMPACT", "FLAG_COUNT", "FLAG_DISPLAY", "FLAG_DISPLAY_DEBUG", "FLAG_TILE_ORDER", "FLAG_WIRE", "KERNEL_AUTO", "KERNEL_GENERIC", "KERNEL_STACK", "TUNE_ONE_KERNEL", "TUNE_SHADOW_QUEUE", "Info",
    "PathTrace", "SdfHipError", "Stats", "Logic", "OctData", "dragon_standin", "knot_point_cloud", "write_ply", "sphere_d4", "torus_d6",
    "Scene", "HostFrame", "MultiScene", "MultiStats", "device_bandwidth", "device_count", "device_pci_bus_id", "sdfgen_trim", "unorm_table",
]
