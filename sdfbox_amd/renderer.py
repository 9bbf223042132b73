"""Frame driver: what `Program.Draw` does for the compute pass
(SdfBox/Program.cs:79-110: UpdateBuffer(info) + DispatchSized(W, H, 1)),
on an MI355X through libsdfhip.so.
"""
import ctypes
import os

import numpy as np

from . import _lib
from ._lib import Info, MultiStats, PathTrace, Stats, check, lib


class HostFrame:
    """A frame array in page-locked host memory (sdfhip_host_alloc), or the caller's own array page-locked where it lies
    (sdfhip_host_register): Scene.Draw / DrawDisplay into `.array` run the frame's copy to the host beside its march.
    Keep the object for as long as the array is in use; close() (or the end of a `with`) gives the memory back."""

    def __init__(self, height=None, width=None, dtype=np.float32, array=None):
        self._p = None
        self._owned = array is None
        if array is None:
            shape = (int(height), int(width), 4)
            nbytes = int(np.prod(shape)) * np.dtype(dtype).itemsize
            p = ctypes.c_void_p()
            check(lib.sdfhip_host_alloc(nbytes, ctypes.byref(p)))
            self._p = p.value
            buf = (ctypes.c_uint8 * nbytes).from_address(self._p)
            self.array = np.frombuffer(buf, dtype=dtype).reshape(shape)
        else:
            if not array.flags.c_contiguous or not array.flags.writeable:
                raise ValueError("HostFrame: the array must be C-contiguous and writeable")
            check(lib.sdfhip_host_register(array.ctypes.data, array.nbytes))
            self._p = array.ctypes.data
            self.array = array

    def close(self):
        if self._p is not None:
            p, self._p = self._p, None
            self.array = None
            check(lib.sdfhip_host_release(ctypes.c_void_p(p)))

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _rays(origins, dirs):
    """(n, 3) origins and directions -> n sdfhip_ray records"""
    o = np.asarray(origins, dtype=np.float32).reshape(-1, 3)
    d = np.asarray(dirs, dtype=np.float32).reshape(-1, 3)
    if len(o) != len(d):
        raise ValueError("Raycast: as many directions as origins")
    rays = np.zeros(len(o), dtype=np.dtype(_lib.Ray))
    rays["origin"] = o
    rays["dir"] = d
    return rays


def placement(yaw, pitch, roll, scale=1.0, about=(0.5, 0.5, 0.5), to=(0.5, 0.5, 0.5)):
    """(R, s, t) for Scene.Place from angles in degrees: R = Ry(yaw) @ Rx(pitch) @ Rz(roll) (right-handed, each about the named
    axis), s = scale, and t such that the source point `about` lands at `to`: t = to - s R about.  Computed in double from the
    arguments and rounded to float32 once, at the end."""
    y, p, r = (np.deg2rad(float(a)) for a in (yaw, pitch, roll))
    Ry = np.array([[np.cos(y), 0.0, np.sin(y)], [0.0, 1.0, 0.0], [-np.sin(y), 0.0, np.cos(y)]])
    Rx = np.array([[1.0, 0.0, 0.0], [0.0, np.cos(p), -np.sin(p)], [0.0, np.sin(p), np.cos(p)]])
    Rz = np.array([[np.cos(r), -np.sin(r), 0.0], [np.sin(r), np.cos(r), 0.0], [0.0, 0.0, 1.0]])
    R = Ry @ Rx @ Rz
    s = float(scale)
    t = np.asarray(to, dtype=np.float64).reshape(3) - s * (R @ np.asarray(about, dtype=np.float64).reshape(3))
    return R.astype(np.float32), np.float32(s), t.astype(np.float32)


def placement_fit(measure, yaw=0, pitch=0, roll=0, size=0.8, to=(0.5, 0.5, 0.5)):
    """(R, s, t) for Scene.Place that fits a measured solid: the centre of `measure`'s bounds (a Scene.Measure result, or anything
    with bounds_min and bounds_max) lands at `to`, and the longest side of those bounds becomes `size`; the angles are placement()'s.
    The bounds are the source's own, axis-aligned before the rotation: a rotated box's own bounds are larger.  Raises ValueError on
    an empty solid (bounds +inf / -inf) and on one without extent."""
    lo = np.array([float(x) for x in measure.bounds_min], dtype=np.float64)
    hi = np.array([float(x) for x in measure.bounds_max], dtype=np.float64)
    if lo.shape != (3,) or hi.shape != (3,) or not (np.isfinite(lo).all() and np.isfinite(hi).all()) or (hi < lo).any():
        raise ValueError("placement_fit: the measured solid is empty")
    side = float((hi - lo).max())
    if not side > 0.0:
        raise ValueError("placement_fit: the measured solid has no extent")
    return placement(yaw, pitch, roll, float(size) / side, about=(lo + hi) * 0.5, to=to)


def linear_array(placement, step, count):
    """`count` placements (R, s, t) for Scene.Compose in a row: copy i is `placement` = (R, s, t) translated by i * step.  Computed
    in double from the arguments and rounded to float32 once, at the end; copy 0 is the input."""
    R, s, t = placement
    count = int(count)
    if count < 1:
        raise ValueError("linear_array: count must be at least 1")
    R = np.asarray(R, dtype=np.float64).reshape(3, 3)
    t = np.asarray(t, dtype=np.float64).reshape(3)
    step = np.asarray(step, dtype=np.float64).reshape(3)
    return [(R.astype(np.float32), np.float32(float(s)), (t + float(i) * step).astype(np.float32)) for i in range(count)]


def _axis_rotation(axis, angle):
    """the rotation by `angle` (radians, right-handed) about the unit vector `axis`, in double (Rodrigues); the identity exactly at 0"""
    K = np.array([[0.0, -axis[2], axis[1]], [axis[2], 0.0, -axis[0]], [-axis[1], axis[0], 0.0]])
    return np.eye(3) + np.sin(angle) * K + (1.0 - np.cos(angle)) * (K @ K)


def circular_array(placement, centre, axis, count):
    """`count` placements (R, s, t) for Scene.Compose round a circle: copy i is `placement` = (R, s, t) turned by 360 * i / count
    degrees (right-handed) about the line through `centre` along the unit vector `axis`: with Q that rotation, (Q R, s, Q t +
    (centre - Q centre)).  Q is a proper rotation, so a mirror stays a mirror.  Computed in double from the arguments and rounded to
    float32 once, at the end; copy 0 is the input.  Raises ValueError on an axis that is not of length 1 (to 1e-6)."""
    R, s, t = placement
    count = int(count)
    if count < 1:
        raise ValueError("circular_array: count must be at least 1")
    R = np.asarray(R, dtype=np.float64).reshape(3, 3)
    t = np.asarray(t, dtype=np.float64).reshape(3)
    c = np.asarray(centre, dtype=np.float64).reshape(3)
    a = np.asarray(axis, dtype=np.float64).reshape(3)
    length = float(np.sqrt((a * a).sum()))
    if not abs(length - 1.0) <= 1e-6:
        raise ValueError("circular_array: the axis must be a unit vector")
    a = a / length
    out = []
    for i in range(count):
        Q = _axis_rotation(a, 2.0 * np.pi * i / count)
        out.append(((Q @ R).astype(np.float32), np.float32(float(s)), (Q @ t + (c - Q @ c)).astype(np.float32)))
    return out


def lattice_of_depth(d):
    """(shape, origin, spacing) for Scene.Volume / Scene.FromVolume: the lattice whose vertices are every corner and every inner
    centre of a tree of depth d -- 2^d + 1 samples along each axis, from the origin, 2^-d apart (every point a build to depth d
    evaluates is a vertex of it, and vertices are exact)."""
    d = int(d)
    if not 0 <= d <= 11:
        raise ValueError("lattice_of_depth: depth outside 0..11 (a lattice has at most 4096 samples along an axis)")
    return ((2 ** d + 1,) * 3, (0, 0, 0), 2.0 ** -d)


def clash_volume(rec, depth, side=1.0):
    """The volume of a clash record's overlap on the lattice of Scene.ClashParts(depth=depth, side=side): points * pitch^3."""
    return int(rec["points"]) * (float(side) * 2.0 ** -int(depth)) ** 3


def clash_centroid(rec, depth, origin=(0.0, 0.0, 0.0), side=1.0):
    """The centroid (3,) of a clash record's shared lattice points: origin + (sum / points + 0.5) * pitch."""
    pitch = float(side) * 2.0 ** -int(depth)
    return np.asarray(origin, dtype=np.float64) + (np.asarray(rec["sum"], dtype=np.float64) / float(rec["points"]) + 0.5) * pitch


def clash_box(rec, depth, origin=(0.0, 0.0, 0.0), side=1.0):
    """(origin, side) of the smallest cube round the cells lo..hi of a clash record, centred on them: the arguments of a second
    Scene.ClashParts that looks at this clash again at a finer pitch."""
    pitch = float(side) * 2.0 ** -int(depth)
    lo, hi = np.asarray(rec["lo"], dtype=np.float64), np.asarray(rec["hi"], dtype=np.float64) + 1.0
    cube = float((hi - lo).max()) * pitch
    centre = np.asarray(origin, dtype=np.float64) + (lo + hi) * 0.5 * pitch
    return tuple(float(c) for c in centre - cube * 0.5), cube


def penetration_push(rec):
    """nearest_a - nearest_b (3,) of a penetration record (Scene.PenetrationParts): the translation of part b that separates the pair
    to first order, of length about ra + rb.  For two overlapping balls it is the axis of their centres, from a to b."""
    return np.asarray(rec["nearest_a"], dtype=np.float64) - np.asarray(rec["nearest_b"], dtype=np.float64)


def gap_vector(rec):
    """point_b - point_a (3,) of a gap record (Scene.GapParts): the way from part a's closest point to part b's, of length about
    gap.  Moving part b by it, reversed, closes the gap to first order."""
    return np.asarray(rec["point_b"], dtype=np.float64) - np.asarray(rec["point_a"], dtype=np.float64)


def component_volume(rec, depth, side=1.0):
    """The volume of a component record on the lattice of Scene.Components(depth=depth, side=side): points * pitch^3."""
    return int(rec["points"]) * (float(side) * 2.0 ** -int(depth)) ** 3


def component_centroid(rec, depth, origin=(0.0, 0.0, 0.0), side=1.0):
    """The centroid (3,) of a component's lattice points: origin + (sum / points + 0.5) * pitch."""
    pitch = float(side) * 2.0 ** -int(depth)
    return np.asarray(origin, dtype=np.float64) + (np.asarray(rec["sum"], dtype=np.float64) / float(rec["points"]) + 0.5) * pitch


def component_box(rec, depth, origin=(0.0, 0.0, 0.0), side=1.0):
    """(origin, side) of the smallest cube round the cells lo..hi of a component record, centred on them: the arguments of a second
    Scene.Components that looks at this piece again at a finer pitch."""
    return clash_box(rec, depth, origin, side)


def component_enclosed(rec, depth):
    """Does the component stay clear of the lattice's six faces (no lo == 0, no hi == 2^depth - 1)?  An enclosed void is a sealed
    cavity."""
    last = (1 << int(depth)) - 1
    return bool(all(int(v) > 0 for v in rec["lo"]) and all(int(v) < last for v in rec["hi"]))


class Scene:
    """A scene resident in one GPU's HBM (replaces the `data` / `values`
    bindings of Program.cs:147-152)."""

    def __init__(self, octdata, device=0, top_grid_level=None, top_grid_split=None, scatter_grid=None, scatter_order=None):
        """top_grid_level / top_grid_split / scatter_grid / scatter_order: sdfhip_upload_options (None = the upload chooses):
        a plain lookup grid of that level (0 = none), a split grid with that coarse level (0 = never), the levels of the
        path-traced mode's second grid's blocks (0 = none) and 0 for its blocks in x-y-z order.  Pixels never depend on them."""
        self._h = ctypes.c_void_p()
        self.device = int(device)
        if (top_grid_level, top_grid_split, scatter_grid, scatter_order) == (None, None, None, None):
            check(lib.sdfhip_scene_upload(self.device, octdata.Structs.ctypes.data,
                                          octdata.Values.ctypes.data, octdata.Length,
                                          ctypes.byref(self._h)))
        else:
            opt = _lib.UploadOptions(top_grid_level, top_grid_split, scatter_grid, scatter_order)
            check(lib.sdfhip_scene_upload_ex(self.device, octdata.Structs.ctypes.data, octdata.Values.ctypes.data, octdata.Length,
                                             ctypes.byref(opt), ctypes.byref(self._h)))
        self._describe()

    def _describe(self):
        n = ctypes.c_uint32(); d = ctypes.c_uint32(); ok = ctypes.c_int(); dev = ctypes.c_int()
        check(lib.sdfhip_scene_info(self._h, ctypes.byref(n), ctypes.byref(d), ctypes.byref(ok),
                                    ctypes.byref(dev)))
        self.Length, self.depth, self.stack_kernel_ok = n.value, d.value, bool(ok.value)
        lvl = ctypes.c_int32(); nb = ctypes.c_uint64()
        check(lib.sdfhip_scene_top_grid(self._h, ctypes.byref(lvl), ctypes.byref(nb)))
        self.top_grid_level, self.top_grid_bytes = lvl.value, nb.value

    @classmethod
    def _built(cls, device, st, call, want_octdata, want_stats, want_scene=True):
        """The frame of every call that returns a new tree.  call(handle, octdata, stats): a lambda round the library's entry point,
        which gets the three byref()s: the new handle (None with want_scene False: TriMesh.Build), the host arrays (None unless
        wanted) and the stats record `st`.  Returns the new Scene, or (scene[, octdata][, stats])."""
        from .octdata import OctData
        self = cls.__new__(cls)
        self._h = ctypes.c_void_p()
        self.device = int(device)
        raw = _lib.COctData()
        check(call(ctypes.byref(self._h) if want_scene else None, ctypes.byref(raw) if want_octdata else None, ctypes.byref(st)))
        out = []
        if want_scene:
            self._describe()
            out.append(self)
        if want_octdata:
            out.append(OctData._from_native(raw))
        if want_stats:
            out.append(st)
        return out[0] if len(out) == 1 else tuple(out)

    @classmethod
    def FromPoints(cls, vertices, depth, device=0, want_octdata=False, want_stats=False):
        """The viewer's generate -> upload flow in one call (sdfhip_sdfgen_scene; Program.cs:613-650 + :147-152): point
        cloud (n, 6) float32 {position, normal} -> scene handle, the tree never leaving HBM.  want_octdata: also the host
        arrays (for the .asdf cache)."""
        v = np.ascontiguousarray(vertices, dtype=np.float32).reshape(-1, 6)
        return cls._built(device, _lib.SdfGenStats(), lambda h, raw, st: lib.sdfhip_sdfgen_scene(int(device), v.ctypes.data, len(v), int(depth), h, raw, st),
                          want_octdata, want_stats)

    def Edit(self, edits, max_depth=None, want_octdata=False, want_stats=False):
        """Space carving (sdfhip_scene_edit): the brushes `edits` -- Edit objects, or (op, brush, params) tuples, applied in order --
        carve from (EDIT_CARVE) or add to (EDIT_ADD) this scene's tree on its device; the result is a NEW Scene, this one is left as
        it was.  max_depth: None = this tree's depth, else 0..12 (deeper lets the brushes refine past it).  want_octdata: also the
        result's host arrays (e.g. for OctData.Save); want_stats: an EditStats."""
        items = [e if isinstance(e, _lib.Edit) else _lib.Edit(*e) for e in edits]
        arr = (_lib.Edit * max(1, len(items)))(*items)
        maxd = -1 if max_depth is None else int(max_depth)
        return Scene._built(self.device, _lib.EditStats(), lambda h, raw, st: lib.sdfhip_scene_edit(self._h, arr, len(items), maxd, h, raw, st),
                            want_octdata, want_stats)

    def Prune(self, tolerance=0, max_depth=None, want_octdata=False, want_stats=False):
        """Pruning (sdfhip_scene_prune): the blocks of eight whose bytes are, within `tolerance` (0..255), what their parent's bytes
        interpolate to -- what Edit gave them before a brush touched them -- are removed, bottom-up, and with max_depth (None = no
        cut, else 0..12) every block below that depth; the result is a NEW Scene, this one is left as it was.  want_octdata: also
        the result's host arrays; want_stats: a PruneStats."""
        opt = _lib.PruneOptions(tolerance, max_depth)
        return Scene._built(self.device, _lib.PruneStats(), lambda h, raw, st: lib.sdfhip_scene_prune(self._h, ctypes.byref(opt), h, raw, st),
                            want_octdata, want_stats)

    def Combine(self, other, op, max_depth=None, want_octdata=False, want_stats=False):
        """Combination (sdfhip_scene_combine): the union (COMBINE_UNION), intersection (COMBINE_INTERSECT) or difference
        (COMBINE_SUBTRACT: this scene without `other`) of this scene and `other`, a Scene on the same device (it may be this one); both
        live in the same unit cube, nothing is placed, blended or pruned (chain Prune(0)).  max_depth: None = no cut, else 0..12.
        The result is a NEW Scene in breadth-first order, both inputs are left as they were.  want_octdata: also the result's host
        arrays; want_stats: a CombineStats."""
        opt = _lib.CombineOptions(max_depth)
        return Scene._built(self.device, _lib.CombineStats(),
                            lambda h, raw, st: lib.sdfhip_scene_combine(self._h, other._h, int(op), ctypes.byref(opt), h, raw, st), want_octdata, want_stats)

    def Place(self, rotation, scale, translation, depth=None, want_octdata=False, want_stats=False):
        """Placement (sdfhip_scene_place): this scene resampled under p = scale * rotation @ x + translation -- rotation (3, 3)
        row-major and orthogonal (a mirror is allowed), scale > 0; placement() makes the three from angles -- into a NEW Scene in
        breadth-first order on the same device; this one is left as it was.  depth: None = this tree's depth, else 0..12.  Nothing is
        pruned (chain Prune), and the identity is a resampling, not a clone.  want_octdata: also the result's host arrays;
        want_stats: a PlaceStats."""
        pl = _lib.Placement(np.asarray(rotation, dtype=np.float32).reshape(3, 3).tolist(), scale, np.asarray(translation, dtype=np.float32).reshape(3).tolist(), depth)
        return Scene._built(self.device, _lib.PlaceStats(), lambda h, raw, st: lib.sdfhip_scene_place(self._h, ctypes.byref(pl), h, raw, st),
                            want_octdata, want_stats)

    @staticmethod
    def Compose(parts, depth=None, want_octdata=False, want_stats=False):
        """Composition (sdfhip_scene_compose): ONE new Scene from many placed instances, in a single pass.  parts: a list of
        (scene, (R, s, t)) or (scene, (R, s, t), op) -- a Scene, its placement as Place takes it, and how the instance joins what
        precedes it in the list: COMBINE_UNION (the default), COMBINE_INTERSECT or COMBINE_SUBTRACT; the first is a union.  The same
        Scene may appear in as many parts as wanted (linear_array() and circular_array() make the placements of a pattern).  Every
        instance's own field is evaluated at every point of the result's lattice, folded in float in list order and rounded to a byte
        once: one instance is Place byte for byte, and the result is NOT Combine of Places (one quantisation, not two).  depth: None =
        the largest depth among the parts' scenes, else 0..12.  Nothing is pruned (chain Prune); every source is left as it was.
        Returns what Place returns; want_stats: a ComposeStats.  Raises ValueError on an empty list and on a part that is not such a
        tuple."""
        parts, arr = Scene._instances("Compose", parts)
        opt = _lib.ComposeOptions(depth)
        return Scene._built(parts[0][0].device, _lib.ComposeStats(),
                            lambda h, raw, st: lib.sdfhip_scene_compose(arr, len(arr), ctypes.byref(opt), h, raw, st), want_octdata, want_stats)

    @staticmethod
    def _instances(what, parts):
        """(the parts as a list, the sdfhip_instance array) of a list of (scene, (R, s, t)) or (scene, (R, s, t), op); ValueError on an
        empty list and on a part that is not such a tuple.  what: the method's name for the messages."""
        parts = list(parts)
        if not parts:
            raise ValueError(f"{what}: no parts")
        items = []
        for k, part in enumerate(parts):
            if not isinstance(part, (tuple, list)) or len(part) not in (2, 3):
                raise ValueError(f"{what}: part {k} is neither (scene, (R, s, t)) nor (scene, (R, s, t), op)")
            scene, pl = part[0], part[1]
            if not isinstance(scene, Scene):
                raise ValueError(f"{what}: part {k}: not a Scene")
            if not isinstance(pl, (tuple, list)) or len(pl) != 3:
                raise ValueError(f"{what}: part {k}: the placement is not (R, s, t)")
            R, sc, t = pl
            op = _lib.COMBINE_UNION if len(part) == 2 else int(part[2])
            items.append(_lib.Instance(scene._h, op, np.asarray(R, dtype=np.float32).reshape(3, 3).tolist(), sc,
                                       np.asarray(t, dtype=np.float32).reshape(3).tolist()))
        return parts, (_lib.Instance * len(items))(*items)

    # -- an assembly of placed instances, drawn, probed and picked without baking (sdfhip_instances_*) -----------------------------------
    # parts: what Compose takes.  skip=False looks every instance up at every point (INSTANCES_NO_SKIP: the same bytes, for tests and
    # the A/B); max_steps None = 100; normal_step None = 2^-10, the h of the six-tap gradient G.
    @staticmethod
    def _instances_options(skip, max_steps, normal_step):
        return _lib.InstancesOptions(0 if skip else _lib.INSTANCES_NO_SKIP, max_steps, normal_step)

    @staticmethod
    def SampleParts(parts, points, skip=True, normal_step=None):
        """The assembly's field at points (n, 3) float32 (sdfhip_instances_sample): n sdfhip_part_probe records -- value = Compose's
        fold F(p) evaluated there, instance = the part that decided it, status, gradient = G(p), not normalised.  A non-finite point
        gets QUERY_INVALID and zeros.  Nothing is built and nothing is kept."""
        _, arr = Scene._instances("SampleParts", parts)
        opt = Scene._instances_options(skip, None, normal_step)
        p = np.ascontiguousarray(points, dtype=np.float32).reshape(-1, 3)
        out = np.zeros(len(p), dtype=np.dtype(_lib.PartProbe))
        check(lib.sdfhip_instances_sample(arr, len(arr), ctypes.byref(opt), p.ctypes.data, len(p), out.ctypes.data))
        return out

    @staticmethod
    def RaycastParts(parts, origins, dirs, margin, limit, max_steps=None, skip=True, normal_step=None):
        """Raycast's march through the assembly's field (sdfhip_instances_raycast): n sdfhip_part_hit records (position, t, normal,
        prox, status, steps, instance = the part the march ended on)."""
        _, arr = Scene._instances("RaycastParts", parts)
        opt = Scene._instances_options(skip, max_steps, normal_step)
        rays = _rays(origins, dirs)
        out = np.zeros(len(rays), dtype=np.dtype(_lib.PartHit))
        check(lib.sdfhip_instances_raycast(arr, len(arr), ctypes.byref(opt), rays.ctypes.data, len(rays), float(margin), float(limit), out.ctypes.data))
        return out

    @staticmethod
    def PickParts(parts, state, pixels, max_steps=None, skip=True, normal_step=None):
        """Which part is under the pixels (n, 2) {x, y} of the camera `state` (a Logic or an Info): RaycastParts from the camera's
        position along the kernel's own ray() for each pixel, margin and limit the camera's (sdfhip_instances_pick)."""
        _, arr = Scene._instances("PickParts", parts)
        opt = Scene._instances_options(skip, max_steps, normal_step)
        px = np.ascontiguousarray(pixels, dtype=np.uint32).reshape(-1, 2)
        out = np.zeros(len(px), dtype=np.dtype(_lib.PartHit))
        info = state if isinstance(state, Info) else state.State
        check(lib.sdfhip_instances_pick(arr, len(arr), ctypes.byref(opt), ctypes.byref(info), px.ctypes.data, len(px), out.ctypes.data))
        return out

    @staticmethod
    def DrawParts(parts, state, width, height, max_steps=None, skip=True, normal_step=None):
        """A (height, width, 4) float32 frame of the assembly, row 0 at the top, alpha = the march's steps (sdfhip_instances_render):
        the shader's pixel with Compose's fold in the place of the tree's distance and G in the place of gradient().  No tree is
        built: a placement may change from one frame to the next at no cost."""
        _, arr = Scene._instances("DrawParts", parts)
        opt = Scene._instances_options(skip, max_steps, normal_step)
        width, height = int(width), int(height)
        if width < 0 or height < 0:
            raise ValueError("DrawParts: width and height must not be negative")
        out = np.zeros((height, width, 4), dtype=np.float32)
        info = state if isinstance(state, Info) else state.State
        check(lib.sdfhip_instances_render(arr, len(arr), ctypes.byref(opt), ctypes.byref(info), width, height, out.ctypes.data))
        return out

    @staticmethod
    def SamplePartsDevice(parts, xyz_ptr, n, out_ptr, stream=None, skip=True, normal_step=None):
        """SampleParts for n points (n x 3 floats) in device memory at `xyz_ptr` into n sdfhip_part_probe records at `out_ptr`: enqueued
        on `stream` (a raw hipStream_t value or None) after the caller's earlier work there; the call waits for that stream."""
        _, arr = Scene._instances("SamplePartsDevice", parts)
        opt = Scene._instances_options(skip, None, normal_step)
        if int(n) < 0:
            raise ValueError("SamplePartsDevice: n must not be negative")
        check(lib.sdfhip_instances_sample_device(arr, len(arr), ctypes.byref(opt), ctypes.c_void_p(int(xyz_ptr)), int(n), ctypes.c_void_p(int(out_ptr)),
                                                 ctypes.c_void_p(int(stream)) if stream else None))

    @staticmethod
    def RaycastPartsDevice(parts, rays_ptr, n, margin, limit, out_ptr, max_steps=None, stream=None, skip=True, normal_step=None):
        """RaycastParts for n sdfhip_ray records in device memory into n sdfhip_part_hit records at `out_ptr`, as SamplePartsDevice."""
        _, arr = Scene._instances("RaycastPartsDevice", parts)
        opt = Scene._instances_options(skip, max_steps, normal_step)
        if int(n) < 0:
            raise ValueError("RaycastPartsDevice: n must not be negative")
        check(lib.sdfhip_instances_raycast_device(arr, len(arr), ctypes.byref(opt), ctypes.c_void_p(int(rays_ptr)), int(n), float(margin), float(limit),
                                                  ctypes.c_void_p(int(out_ptr)), ctypes.c_void_p(int(stream)) if stream else None))

    @staticmethod
    def DrawPartsDevice(parts, state, width, height, out_ptr, max_steps=None, stream=None, skip=True, normal_step=None):
        """DrawParts into width x height float4 pixels of device memory at `out_ptr`, as SamplePartsDevice."""
        _, arr = Scene._instances("DrawPartsDevice", parts)
        opt = Scene._instances_options(skip, max_steps, normal_step)
        if int(width) < 0 or int(height) < 0:
            raise ValueError("DrawPartsDevice: width and height must not be negative")
        info = state if isinstance(state, Info) else state.State
        check(lib.sdfhip_instances_render_device(arr, len(arr), ctypes.byref(opt), ctypes.byref(info), int(width), int(height),
                                                 ctypes.c_void_p(int(out_ptr)), ctypes.c_void_p(int(stream)) if stream else None))

    # -- volumes in and out (sdfhip_volume_build / sdfhip_scene_volume): a dense lattice of distances as a scene and back -------------
    @staticmethod
    def ClashParts(parts, depth=6, origin=(0.0, 0.0, 0.0), side=1.0, skip=True):
        """The clash check (sdfhip_instances_clash): which pairs of the parts overlap on the lattice of the 8^depth cell centres of the
        cube (origin, side), depth 0..10.  parts: what Compose takes, at most CLASH_MAX_INSTANCES of them; the ops are ignored, every
        part counts as a solid.  Returns (records, stats): a structured array of sdfhip_clash records in (a, b) order -- a < b, points =
        the lattice points inside both, first = the lowest linear index (z << 2 depth | y << depth | x) among them, lo / hi their
        inclusive lattice bounds, sum the sums of their x, y and z -- and a ClashStats.  Everything is an integer: two calls give the
        same bytes.  clash_volume(), clash_centroid() and clash_box() read a record.  Nothing is built and nothing is kept."""
        _, arr = Scene._instances("ClashParts", parts)
        opt = _lib.ClashOptions(0 if skip else _lib.CLASH_NO_SKIP, depth, np.asarray(origin, dtype=np.float32).reshape(3).tolist(), side)
        st = _lib.ClashStats()
        n = ctypes.c_uint32()
        out = np.zeros(len(arr) * (len(arr) - 1) // 2, dtype=np.dtype(_lib.Clash))
        check(lib.sdfhip_instances_clash(arr, len(arr), ctypes.byref(opt), out.ctypes.data if len(out) else None, len(out), ctypes.byref(n), ctypes.byref(st)))
        return out[:n.value].copy(), st

    @staticmethod
    def PenetrationParts(parts, depth=6, origin=(0.0, 0.0, 0.0), side=1.0, skip=True):
        """The penetration depth (sdfhip_instances_penetration): how far each overlapping pair of the parts reaches into the other, on
        ClashParts' lattice -- the 8^depth cell centres of the cube (origin, side), depth 0..10 -- and ClashParts' list.  At every
        lattice point inside two or more parts one exact nearest-surface search runs per containing part: r_k = the distance from
        the point to part k's surface.  Returns (records, stats): a structured array of sdfhip_penetration records in (a, b) order --
        points as ClashParts counts them, depth = the largest fminf(r_a, r_b) over the shared points (the radius of the largest ball
        round a shared lattice point inside both), witness = the lowest linear index attaining it, ra / rb there, node_a / node_b the
        cut cells of the nearest triangles and nearest_a / nearest_b each part's nearest surface point in world coordinates -- and a
        PenetrationStats.  penetration_push() reads the way to push part b.  Two calls give the same bytes.  The workflow: ClashParts
        at a coarse depth, clash_box(record, ...) for the cube round one overlap, then PenetrationParts(parts, depth, *box) on that
        cube at a finer pitch.  Nothing is built and nothing is kept."""
        _, arr = Scene._instances("PenetrationParts", parts)
        opt = _lib.PenetrationOptions(0 if skip else _lib.PENETRATION_NO_SKIP, depth, np.asarray(origin, dtype=np.float32).reshape(3).tolist(), side)
        st = _lib.PenetrationStats()
        n = ctypes.c_uint32()
        out = np.zeros(len(arr) * (len(arr) - 1) // 2, dtype=np.dtype(_lib.Penetration))
        check(lib.sdfhip_instances_penetration(arr, len(arr), ctypes.byref(opt), out.ctypes.data if len(out) else None, len(out), ctypes.byref(n),
                                               ctypes.byref(st)))
        return out[:n.value].copy(), st

    @staticmethod
    def GapParts(parts, limit=float("inf"), prune=True):
        """The clearance (sdfhip_instances_gap): how far apart the surfaces of each pair of the parts lie and where they are nearest,
        on ClashParts' list.  Every vertex of each part's triangles (the mesh of its source at full detail, placed) is held against
        the other part's surface by an exact nearest-surface search that starts from the pair's best gap so far.  Returns (records,
        stats): a structured array of sdfhip_gap records in (a, b) order, one per pair whose gap is <= limit -- gap, flags
        (GAP_WITNESS_OF_B: the closest vertex is part b's; GAP_CONTAINED: one of the two closest points lies inside the other part, the surfaces are nested or
        interpenetrating: run ClashParts), node_a / node_b the cut cells of the two closest points, corner = 3 k + v of the witness
        vertex in its cell, point_a / point_b the closest points in world coordinates -- and a GapStats.  gap_vector() reads the way
        across the gap.  This is the vertex-to-surface distance both ways round: never below the distance between the two triangle
        sets, above it by less than half an edge of the finer mesh.  prune=False runs every candidate with no bound and gives the same
        records.  Two calls give the same records; stats.searches and stats.visited differ from call to call unless prune=False.
        Nothing is built and nothing is kept."""
        _, arr = Scene._instances("GapParts", parts)
        opt = _lib.GapOptions(0 if prune else _lib.GAP_NO_PRUNE, limit)
        st = _lib.GapStats()
        n = ctypes.c_uint32()
        out = np.zeros(len(arr) * (len(arr) - 1) // 2, dtype=np.dtype(_lib.Gap))
        check(lib.sdfhip_instances_gap(arr, len(arr), ctypes.byref(opt), out.ctypes.data if len(out) else None, len(out), ctypes.byref(n), ctypes.byref(st)))
        return out[:n.value].copy(), st

    @classmethod
    def FromVolume(cls, grid, origin=(0, 0, 0), spacing=None, depth=None, value_scale=1.0, device=0, want_octdata=False, want_stats=False):
        """A scene from a regular lattice of distances (sdfhip_volume_build[_device]): `grid` is a C-contiguous (nz, ny, nx) numpy
        array, or a contiguous torch tensor on cuda:`device` (read where it lies, through data_ptr(), after the device's current
        torch stream has been waited for), float32 or float16, at least two samples along each axis.  Sample (k, j, i) sits at origin
        + (i, j, k) * spacing in the unit cube's coordinates; spacing None = the grid spans the cube along x, 1 / (nx - 1).
        stored value * value_scale = distance in cube units (a field in voxel units: value_scale = spacing; positive inside: a
        negative scale).  depth: 0..12, the deepest level of the tree; None = the first level whose cells are no larger than the
        spacing.  The value is the trilinear interpolant, continued outside the grid's box at slope 1; the split rule assumes a
        distance, so a truncated field splits everywhere below its truncation: chain Prune.  A non-finite sample is refused
        (ERR_ARG).  want_octdata: also the result's host arrays; want_stats: a VolumeStats."""
        dtypes = {"float32": _lib.VOLUME_F32, "float16": _lib.VOLUME_F16}
        on_device = hasattr(grid, "data_ptr") and hasattr(grid, "is_cuda")
        if on_device:
            import torch
            name = str(grid.dtype).replace("torch.", "")
            if not grid.is_cuda:
                raise TypeError("FromVolume: a torch tensor must live on the device (a host tensor: pass tensor.numpy())")
            if name not in dtypes:
                raise TypeError(f"FromVolume: dtype {grid.dtype} is neither float32 nor float16")
            if grid.dim() != 3 or not grid.is_contiguous():
                raise ValueError("FromVolume: the grid must be a contiguous (nz, ny, nx) tensor")
            if grid.device.index != int(device):
                raise ValueError(f"FromVolume: the tensor is on {grid.device}, the scene is asked for on device {int(device)}")
            shape = tuple(int(x) for x in grid.shape)
        elif isinstance(grid, np.ndarray):
            name = grid.dtype.name
            if name not in dtypes:
                raise TypeError(f"FromVolume: dtype {grid.dtype} is neither float32 nor float16")
            if grid.ndim != 3 or not grid.flags.c_contiguous:
                raise ValueError("FromVolume: the grid must be a C-contiguous (nz, ny, nx) array")
            shape = grid.shape
        else:
            raise TypeError("FromVolume: the grid must be a numpy array or a torch tensor on the device")
        nz, ny, nx = shape
        if min(shape) < 2 or max(shape) > 4096 or nx * ny * nz > 2 ** 31:
            raise ValueError(f"FromVolume: a grid of {nx} x {ny} x {nz} samples (2..4096 along each axis, at most 2^31 in all)")
        spacing = 1.0 / (nx - 1) if spacing is None else float(spacing)
        if not (np.isfinite(spacing) and spacing > 0):
            raise ValueError("FromVolume: spacing must be a finite number above 0")
        if depth is None:
            depth = min(max(int(np.ceil(-np.log2(spacing))), 0), 12)
        if not 0 <= int(depth) <= 12:
            raise ValueError("FromVolume: depth outside 0..12")
        vol = _lib.Volume((nx, ny, nz), origin, spacing, value_scale, dtypes[name], depth)
        if on_device:
            torch.cuda.current_stream(int(device)).synchronize()
            build, where = lib.sdfhip_volume_build_device, ctypes.c_void_p(grid.data_ptr())
        else:
            build, where = lib.sdfhip_volume_build, grid.ctypes.data
        return cls._built(device, _lib.VolumeStats(), lambda h, raw, st: build(int(device), where, ctypes.byref(vol), h, raw, st),
                          want_octdata, want_stats)

    def Volume(self, shape, origin=(0, 0, 0), spacing=None, dtype=np.float32, out=None):
        """This scene's distances on a regular lattice (sdfhip_scene_volume[_device]): element (k, j, i) of the (nz, ny, nx) = `shape`
        result is what Sample returns at origin + (i, j, k) * spacing clamped to the cube, plus the distance from there to the point:
        the field continued outside the cube at slope 1.  spacing None = the lattice spans the cube along x, 1 / (nx - 1).  Returns
        a numpy array of `dtype` (float32 or float16); or, with `out` a contiguous torch tensor of that shape on this scene's device,
        fills it asynchronously on the device's current torch stream and returns it.  lattice_of_depth(d) gives the three arguments
        of the lattice a depth-d tree is built on."""
        dtypes = {"float32": _lib.VOLUME_F32, "float16": _lib.VOLUME_F16}
        shape = tuple(int(x) for x in shape)
        if len(shape) != 3 or min(shape) < 1 or max(shape) > 4096 or shape[0] * shape[1] * shape[2] > 2 ** 31:
            raise ValueError(f"Volume: shape {shape} is not (nz, ny, nx) with 1..4096 along each axis and at most 2^31 elements")
        nz, ny, nx = shape
        if spacing is None:
            if nx < 2:
                raise ValueError("Volume: a lattice of one sample along x needs a spacing")
            spacing = 1.0 / (nx - 1)
        if not (np.isfinite(float(spacing)) and float(spacing) > 0):
            raise ValueError("Volume: spacing must be a finite number above 0")
        if out is None:
            name = np.dtype(dtype).name
            if name not in dtypes:
                raise TypeError(f"Volume: dtype {dtype} is neither float32 nor float16")
            lattice = _lib.Volume((nx, ny, nz), origin, spacing, 0.0, dtypes[name], 0)
            res = np.empty(shape, dtype=np.dtype(dtype))
            check(lib.sdfhip_scene_volume(self._h, ctypes.byref(lattice), res.ctypes.data))
            return res
        if not (hasattr(out, "data_ptr") and hasattr(out, "is_cuda")):
            raise TypeError("Volume: out must be a torch tensor on the scene's device")
        import torch
        name = str(out.dtype).replace("torch.", "")
        if not out.is_cuda or name not in dtypes:
            raise TypeError("Volume: out must be a float32 or float16 tensor on the scene's device")
        if tuple(out.shape) != shape or not out.is_contiguous() or out.device.index != self.device:
            raise ValueError(f"Volume: out must be a contiguous tensor of shape {shape} on device {self.device}")
        lattice = _lib.Volume((nx, ny, nz), origin, spacing, 0.0, dtypes[name], 0)
        stream = torch.cuda.current_stream(self.device).cuda_stream
        check(lib.sdfhip_scene_volume_device(self._h, ctypes.byref(lattice), ctypes.c_void_p(out.data_ptr()),
                                             ctypes.c_void_p(int(stream)) if stream else None))
        return out

    # -- components (sdfhip_scene_components[_device]): the separate solids and enclosed voids on a cubic lattice ------------------------
    def _components(self, what, call, depth, origin, side, labels):
        opt = _lib.ComponentsOptions(0, depth, np.asarray(origin, dtype=np.float32).reshape(3).tolist(), side)
        st = _lib.ComponentsStats()
        n = ctypes.c_uint32()
        out = np.zeros(1024, dtype=np.dtype(_lib.Component))
        # (a table of 1024 records holds all but a hostile scene's components; a longer one takes the call a second time)
        for _ in range(2):
            check(call(self._h, ctypes.byref(opt), out.ctypes.data, len(out), ctypes.byref(n), labels, ctypes.byref(st)))
            if n.value <= len(out):
                return out[:n.value].copy(), st
            out = np.zeros(n.value, dtype=out.dtype)
        raise RuntimeError(f"{what}: the number of components changed between two calls")

    def Components(self, depth=6, origin=(0.0, 0.0, 0.0), side=1.0, labels=False):
        """The face-connected components of this scene (sdfhip_scene_components) on the lattice of the 8^depth cell centres of the cube
        (origin, side), depth 0..9: a point is inside iff the value Volume writes there is < 0, two points that differ by 1 in one
        coordinate and are both inside or both outside are connected.  Returns (records, stats): a structured array of
        sdfhip_component records in ascending label order -- label = the lowest linear index (z << 2 depth | y << depth | x) of the
        component, flags = COMPONENT_SOLID for a solid and 0 for a void, points, lo / hi the inclusive lattice bounds, sum the sums
        of x, y and z -- and a ComponentsStats.  labels=True: also every point's label, a uint32 array of shape (n, n, n), n = 2^depth,
        indexed [z, y, x].  Everything is an integer: two calls give the same bytes.  component_volume(), component_centroid(),
        component_box() and component_enclosed() read a record.  Nothing is built and nothing is kept."""
        n = 1 << int(depth) if 0 <= int(depth) <= _lib.COMPONENTS_MAX_DEPTH else 1
        lab = np.empty((n, n, n), dtype=np.uint32) if labels else None
        rec, st = self._components("Components", lib.sdfhip_scene_components, depth, origin, side, lab.ctypes.data if labels else None)
        return (rec, st, lab) if labels else (rec, st)

    def ComponentsDevice(self, depth=6, origin=(0.0, 0.0, 0.0), side=1.0, labels_ptr=None):
        """Components with the labels written to 8^depth uint32 words of device memory at `labels_ptr` on this scene's device (a torch
        tensor's data_ptr(); None: no labels).  Synchronous, on a stream of the call's own: work enqueued on `labels_ptr` by other
        streams must have been waited for.  Returns (records, stats), both in host memory."""
        return self._components("ComponentsDevice", lib.sdfhip_scene_components_device, depth, origin, side,
                                ctypes.c_void_p(int(labels_ptr)) if labels_ptr else None)

    # -- selection (sdfhip_scene_select): keep, drop or fill this scene's components as a new scene ------------------------------------
    def Select(self, keep_largest=False, drop_below=0, fill_enclosed=False, flip=None, keep=None, lattice_depth=6, origin=(0.0, 0.0, 0.0),
               side=1.0, depth=None, want_octdata=False, want_stats=False):
        """Selection (sdfhip_scene_select): this scene with some of its components' phases flipped -- a solid becomes empty space, a
        void becomes solid -- as a NEW Scene in breadth-first order on the same device; this one is left as it was.  The components
        are those Components(lattice_depth, origin, side) reports.  A component flips if any rule flips it: keep_largest, every solid
        but the one with most points (tie: the lowest label); drop_below=k > 0, every solid with fewer than k points; fill_enclosed,
        every void that touches no face of the lattice; flip=[labels], the listed components, solid or void; keep=[labels], every
        solid that is not listed (flip and keep exclude each other; a listed label must be a component's, and under keep a solid's).
        With no rule the result is Place at the identity, byte for byte.  depth: None = this tree's depth, else 0..12.  The tree keeps
        the removed pieces' former surfaces as structure (the bytes there are lower bounds): Offset(0) re-distances it; nothing is
        pruned (chain Prune).  want_octdata: also the result's host arrays; want_stats: a SelectStats."""
        if flip is not None and keep is not None:
            raise ValueError("Select: flip and keep exclude each other")
        flags = ((_lib.SELECT_KEEP_LARGEST_SOLID if keep_largest else 0) | (_lib.SELECT_DROP_SMALL_SOLIDS if int(drop_below) > 0 else 0)
                 | (_lib.SELECT_FILL_ENCLOSED_VOIDS if fill_enclosed else 0) | (_lib.SELECT_FLIP_LISTED if flip is not None else 0)
                 | (_lib.SELECT_KEEP_LISTED if keep is not None else 0))
        listed = None if flip is None and keep is None else np.ascontiguousarray(flip if keep is None else keep, dtype=np.uint32).reshape(-1)
        opt = _lib.SelectOptions(flags, lattice_depth, np.asarray(origin, dtype=np.float32).reshape(3).tolist(), side, depth, max(int(drop_below), 0))
        where, count = (listed.ctypes.data if listed is not None and len(listed) else None), (0 if listed is None else len(listed))
        return Scene._built(self.device, _lib.SelectStats(),
                            lambda h, raw, st: lib.sdfhip_scene_select(self._h, ctypes.byref(opt), where, count, h, raw, st), want_octdata, want_stats)

    def KeepLargest(self, lattice_depth=6, origin=(0.0, 0.0, 0.0), side=1.0, depth=None, want_octdata=False, want_stats=False):
        """Select(keep_largest=True): this scene without its floating pieces."""
        return self.Select(keep_largest=True, lattice_depth=lattice_depth, origin=origin, side=side, depth=depth, want_octdata=want_octdata,
                           want_stats=want_stats)

    def FillCavities(self, lattice_depth=6, origin=(0.0, 0.0, 0.0), side=1.0, depth=None, want_octdata=False, want_stats=False):
        """Select(fill_enclosed=True): this scene with its sealed cavities filled."""
        return self.Select(fill_enclosed=True, lattice_depth=lattice_depth, origin=origin, side=side, depth=depth, want_octdata=want_octdata,
                           want_stats=want_stats)

    def Split(self, lattice_depth=6, origin=(0.0, 0.0, 0.0), side=1.0, depth=None, max_parts=64):
        """This scene's solids as scenes of their own: one Components call, then one Select(keep=[label]) per solid, in label order.
        Returns the list of new Scenes (the caller closes them).  Raises ValueError when there are more solids than max_parts."""
        rec, _ = self.Components(depth=lattice_depth, origin=origin, side=side)
        solids = [int(r["label"]) for r in rec if r["flags"] & _lib.COMPONENT_SOLID]
        if len(solids) > int(max_parts):
            raise ValueError(f"Split: {len(solids)} solids, more than max_parts = {int(max_parts)}")
        parts = []
        try:
            for label in solids:
                parts.append(self.Select(keep=[label], lattice_depth=lattice_depth, origin=origin, side=side, depth=depth))
        except Exception:
            for p in parts:
                p.close()
            raise
        return parts

    # -- exact distance (sdfhip_scene_distance / _offset): clearance, offset and shell ------------------------------------------------
    def Distance(self, points, level=-1):
        """The exact signed distance from points (n, 3) float32 to this scene's surface -- the triangles Mesh(level) emits -- at any
        range, where Sample's distance saturates one leaf edge away: a structured array of n records (fields of sdfhip_clearance:
        distance, node, nearest, status, visited).  A non-finite point gets QUERY_INVALID and zeros; an empty surface gives +-inf."""
        p = np.ascontiguousarray(points, dtype=np.float32).reshape(-1, 3)
        out = np.zeros(len(p), dtype=np.dtype(_lib.Clearance))
        check(lib.sdfhip_scene_distance(self._h, p.ctypes.data, len(p), int(level), out.ctypes.data))
        return out

    def DistanceDevice(self, xyz_ptr, n, out_ptr, level=-1, stream=None):
        """Distance for n points (n x 3 floats) in device memory at `xyz_ptr` into n sdfhip_clearance records at `out_ptr`,
        asynchronously on `stream` (a raw hipStream_t value or None), as SampleDevice."""
        check(lib.sdfhip_scene_distance_device(self._h, ctypes.c_void_p(int(xyz_ptr)), int(n), int(level), ctypes.c_void_p(int(out_ptr)),
                                               ctypes.c_void_p(int(stream)) if stream else None))

    def _offset(self, mode, amount, depth, level, want_octdata, want_stats):
        opt = _lib.OffsetOptions(mode, amount, depth, level)
        return Scene._built(self.device, _lib.OffsetStats(), lambda h, raw, st: lib.sdfhip_scene_offset(self._h, ctypes.byref(opt), h, raw, st),
                            want_octdata, want_stats)

    def Offset(self, delta, depth=None, level=-1, want_octdata=False, want_stats=False):
        """Offset (sdfhip_scene_offset, OFFSET_GROW): this scene's solid grown by `delta` (shrunk when it is negative) -- the tree of
        Distance(p) - delta -- as a NEW Scene in breadth-first order on the same device; this one is left as it was.  depth: None =
        this tree's depth, else 0..12; level: the source surface's level, as Mesh.  Nothing is pruned (chain Prune).  want_octdata:
        also the result's host arrays; want_stats: an OffsetStats."""
        return self._offset(_lib.OFFSET_GROW, delta, depth, level, want_octdata, want_stats)

    def Shell(self, thickness, depth=None, level=-1, want_octdata=False, want_stats=False):
        """Shell (sdfhip_scene_offset, OFFSET_SHELL): the wall of `thickness` > 0 centred on this scene's surface -- the tree of
        abs(Distance(p)) - thickness / 2 -- as a NEW Scene; the arguments are Offset's."""
        return self._offset(_lib.OFFSET_SHELL, thickness, depth, level, want_octdata, want_stats)

    # -- smooth blends and morphs on the exact distance (sdfhip_scene_blend) ------------------------------------------------------------
    def Blend(self, other, op, radius, depth=None, level=-1, other_level=-1, want_octdata=False, want_stats=False):
        """Smooth blend (sdfhip_scene_blend): the smooth union (BLEND_UNION), intersection (BLEND_INTERSECT) or difference
        (BLEND_SUBTRACT: this scene without `other`) of this scene and `other`, a Scene on the same device (it may be this one), on
        their exact distances a = Distance_A(p), b = Distance_B(p): the tree of smin(a, b, radius) and its mirror images, smin = min(a,
        b) - h * h * radius / 4 with h = max(radius - |a - b|, 0) / radius -- a fillet of radius `radius` >= 0 where the two surfaces
        meet, the hard operation at 0 -- as a NEW Scene in breadth-first order; both inputs are left as they were.  BLEND_MORPH takes
        `radius` as t (Morph).  depth: None = the deeper of the two trees' depths, else 0..12; level, other_level: each surface's
        level, as Mesh.  Nothing is pruned (chain Prune).  want_octdata: also the result's host arrays; want_stats: a BlendStats."""
        opt = _lib.BlendOptions(op, radius, depth, level, other_level)
        return Scene._built(self.device, _lib.BlendStats(), lambda h, raw, st: lib.sdfhip_scene_blend(self._h, other._h, ctypes.byref(opt), h, raw, st),
                            want_octdata, want_stats)

    def Morph(self, other, t, depth=None, level=-1, other_level=-1, want_octdata=False, want_stats=False):
        """Morph (sdfhip_scene_blend, BLEND_MORPH): the in-between of this scene and `other` -- the tree of a + (b - a) * t, 0 <= t <= 1:
        this scene's exact field at 0, the other's at 1 -- as a NEW Scene; the other arguments are Blend's.  Refused (ERR_ARG) when
        either surface is empty."""
        return self.Blend(other, _lib.BLEND_MORPH, t, depth, level, other_level, want_octdata, want_stats)

    # -- point and ray queries (sdfhip_scene_sample / _raycast / _pick): answers without a frame ---------------------------------
    def Sample(self, points):
        """Distance, cell and gradient at points (n, 3) float32, with the shader's own arithmetic: a structured array of n records
        (fields of sdfhip_probe: distance, node, scale, status, gradient).  A non-finite point gets QUERY_INVALID and zeros."""
        p = np.ascontiguousarray(points, dtype=np.float32).reshape(-1, 3)
        out = np.zeros(len(p), dtype=np.dtype(_lib.Probe))
        check(lib.sdfhip_scene_sample(self._h, p.ctypes.data, len(p), out.ctypes.data))
        return out

    def Raycast(self, origins, dirs, margin, limit, max_steps=100):
        """The shader's primary march (Compute.hlsl:194-203) for n arbitrary rays -- origins, dirs (n, 3) float32, dirs used as given:
        a structured array of n sdfhip_hit records (position, t, normal, prox, status, steps, node, scale)."""
        rays = _rays(origins, dirs)
        out = np.zeros(len(rays), dtype=np.dtype(_lib.Hit))
        check(lib.sdfhip_scene_raycast(self._h, rays.ctypes.data, len(rays), float(margin), float(limit), int(max_steps), out.ctypes.data))
        return out

    def Pick(self, state, pixels, max_steps=100):
        """What is under the pixels (n, 2) {x, y} of the camera `state` (a Logic or an Info): the march of Raycast from the camera's
        position along the kernel's own ray() for each pixel, margin and limit the camera's."""
        px = np.ascontiguousarray(pixels, dtype=np.uint32).reshape(-1, 2)
        out = np.zeros(len(px), dtype=np.dtype(_lib.Hit))
        info = state if isinstance(state, Info) else state.State
        check(lib.sdfhip_scene_pick(self._h, ctypes.byref(info), px.ctypes.data, len(px), int(max_steps), out.ctypes.data))
        return out

    def SampleDevice(self, xyz_ptr, n, out_ptr, stream=None):
        """Sample for n points (n x 3 floats) in device memory at `xyz_ptr` into n sdfhip_probe records at `out_ptr`, asynchronously
        on `stream` (a raw hipStream_t value or None), as DrawDevice."""
        check(lib.sdfhip_scene_sample_device(self._h, ctypes.c_void_p(int(xyz_ptr)), int(n), ctypes.c_void_p(int(out_ptr)),
                                             ctypes.c_void_p(int(stream)) if stream else None))

    def RaycastDevice(self, rays_ptr, n, margin, limit, out_ptr, max_steps=100, stream=None):
        """Raycast for n sdfhip_ray records in device memory into n sdfhip_hit records at `out_ptr`, asynchronously on `stream`."""
        check(lib.sdfhip_scene_raycast_device(self._h, ctypes.c_void_p(int(rays_ptr)), int(n), float(margin), float(limit), int(max_steps),
                                              ctypes.c_void_p(int(out_ptr)), ctypes.c_void_p(int(stream)) if stream else None))

    # -- surface extraction (sdfhip_scene_mesh): the scene as triangles ----------------------------------------------------------
    def Mesh(self, level=-1, want_stats=True):
        """The surface as a triangle soup: an (n, 3, 6) float32 array {position, normal} per vertex -- reshape(-1, 6) is a point cloud
        for FromPoints / OctData.SdfGen -- in the pinned order (cells by node index).  level: -1 = the leaves, 0..12 = the
        level-of-detail mesh of that level.  Returns (triangles, MeshStats), or the array alone with want_stats=False."""
        opt = _lib.MeshOptions(level)
        raw = _lib.CMesh()
        st = _lib.MeshStats()
        check(lib.sdfhip_scene_mesh(self._h, ctypes.byref(opt), ctypes.byref(raw), ctypes.byref(st) if want_stats else None))
        try:
            n = raw.n_triangles
            tris = np.ctypeslib.as_array(raw.verts6, shape=(n, 3, 6)).copy() if n else np.zeros((0, 3, 6), np.float32)
        finally:
            lib.sdfhip_mesh_free(ctypes.byref(raw))
        return (tris, st) if want_stats else tris

    def MeshDevice(self, out_ptr=None, capacity=0, level=-1, stream=None):
        """The triangle count the scene needs at `level` -- always -- and, if it fits `capacity` triangles, the vertices into device
        memory at `out_ptr` (capacity x 3 x 6 floats), asynchronously on `stream` (a raw hipStream_t value or None), as DrawDevice.
        MeshDevice() asks for the count alone."""
        opt = _lib.MeshOptions(level)
        n = ctypes.c_uint32()
        check(lib.sdfhip_scene_mesh_device(self._h, ctypes.byref(opt), ctypes.c_void_p(int(out_ptr)) if out_ptr else None, int(capacity),
                                           ctypes.byref(n), ctypes.c_void_p(int(stream)) if stream else None))
        return n.value

    # -- the measure (sdfhip_scene_measure): what the solid amounts to -----------------------------------------------------------
    def Measure(self, level=-1):
        """Volume, area, first and second moments about the origin, the tight bounds and the cell counts of the solid this scene
        describes -- the one Mesh bounds and the renderer draws, in double precision: a _lib.Measure with the raw fields of
        sdfhip_measure, `centroid` (None for an empty solid) and `inertia()`.  level: as Mesh.  The sums are the same bits on every
        call; placement_fit() makes a placement from the bounds."""
        opt = _lib.MeasureOptions(level)
        out = _lib.Measure()
        check(lib.sdfhip_scene_measure(self._h, ctypes.byref(opt), ctypes.byref(out)))
        return out

    # -- cross-sections (sdfhip_scene_slice): the contours of a stack of planes ---------------------------------------------------
    def Slice(self, normal=(0.0, 0.0, 1.0), offset=0.5, pitch=0.0, layers=1, level=-1, want_stats=True):
        """The contours of the solid in the planes dot(normal, p) = offset + k * pitch, k = 0 .. layers - 1 (the normal as given, never
        normalised), as directed segments: the solid lies on the left of a -> b seen from the tip of the normal.  Returns
        (segments, layer_starts, SliceStats), or without the statistics with want_stats=False: `segments` a structured array
        {a: 3f4, layer: u4, b: 3f4, node: u4} stably sorted by layer (node-major within a layer), `layer_starts` the layers + 1
        offsets of the layers in it.  level: as Mesh.  slices.slice_loops chains a layer into closed polylines."""
        from .slices import SEGMENT
        opt = _lib.SliceOptions(normal, offset, pitch, layers, level)
        raw = _lib.CSlice()
        st = _lib.SliceStats()
        check(lib.sdfhip_scene_slice(self._h, ctypes.byref(opt), ctypes.byref(raw), ctypes.byref(st) if want_stats else None))
        try:
            n = raw.n_segments
            segs = np.ctypeslib.as_array(ctypes.cast(raw.segments, ctypes.POINTER(ctypes.c_uint32)), shape=(n, 8)).copy().view(SEGMENT).reshape(n) \
                if n else np.zeros(0, SEGMENT)
            counts = np.ctypeslib.as_array(raw.layer_counts, shape=(raw.layers,)).copy()
        finally:
            lib.sdfhip_slice_free(ctypes.byref(raw))
        starts = np.concatenate([[0], np.cumsum(counts, dtype=np.int64)])
        segs = segs[np.argsort(segs["layer"], kind="stable")]
        return (segs, starts, st) if want_stats else (segs, starts)

    def SliceDevice(self, out_ptr=None, capacity=0, counts_ptr=None, normal=(0.0, 0.0, 1.0), offset=0.5, pitch=0.0, layers=1, level=-1, stream=None):
        """The record count of Slice -- always -- and, if it fits `capacity` records, the 32-byte records into device memory at
        `out_ptr`, asynchronously on `stream` (a raw hipStream_t value or None), as MeshDevice; in node-major order, NOT sorted by
        layer.  counts_ptr: `layers` words of device memory for the records per layer, written whether or not the records fit."""
        opt = _lib.SliceOptions(normal, offset, pitch, layers, level)
        n = ctypes.c_uint32()
        check(lib.sdfhip_scene_slice_device(self._h, ctypes.byref(opt), ctypes.c_void_p(int(out_ptr)) if out_ptr else None, int(capacity),
                                            ctypes.c_void_p(int(counts_ptr)) if counts_ptr else None, ctypes.byref(n),
                                            ctypes.c_void_p(int(stream)) if stream else None))
        return n.value

    def close(self):
        if self._h:
            lib.sdfhip_scene_free(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    # -- Program.Draw ----------------------------------------------------
    def Draw(self, state, width, height, flags=_lib.KERNEL_AUTO, want_stats=False, out=None):
        """Render one frame to a host array (H, W, 4) float32; alpha = step count.  out: reuse this
        array (a renderer does: a fresh 4K array per frame costs 5 ms of first-touch page faults in the copy)."""
        if out is None:
            out = np.empty((int(height), int(width), 4), dtype=np.float32)
        elif out.shape != (int(height), int(width), 4) or out.dtype != np.float32 or not out.flags.c_contiguous:
            raise ValueError("Draw: out must be a C-contiguous float32 array of shape (height, width, 4)")
        st = Stats()
        info = state if isinstance(state, Info) else state.State
        check(lib.sdfhip_render(self._h, ctypes.byref(info), int(width), int(height), int(flags),
                                out.ctypes.data, ctypes.byref(st) if want_stats else None))
        return (out, st) if want_stats else out

    def DrawBatchDevice(self, states, width, height, out_ptr, nrows_out=None, band_rows=None,
                        band_first=0, band_stride=1, flags=_lib.KERNEL_AUTO, stream=None, stats=None):
        """Several frames (<= 8 cameras) in one launch into out_ptr[f][nrows_out][width] pixels."""
        infos = (Info * len(states))(*[s if isinstance(s, Info) else s.State for s in states])
        if nrows_out is None:
            nrows_out = height
        if band_rows is None:
            band_rows = height
        check(lib.sdfhip_render_batch_device(self._h, infos, len(states), int(width), int(height),
                                             int(band_rows), int(band_first), int(band_stride),
                                             int(nrows_out), int(flags), ctypes.c_void_p(int(out_ptr)),
                                             ctypes.c_void_p(int(stream)) if stream else None,
                                             ctypes.byref(stats) if stats is not None else None))

    def DrawBandsDevice(self, states, width, height, out_ptr, band_rows, bands, nrows_out=None, pt=None,
                        flags=_lib.KERNEL_AUTO, stream=None, stats=None):
        """The listed bands (band indices of the frame, `band_rows` rows each) of one or several
        frames into out_ptr[f][nrows_out][width] pixels: local band i = bands[i].  pt: path-traced
        mode (one frame)."""
        if not isinstance(states, (list, tuple)):
            states = [states]
        infos = (Info * len(states))(*[s if isinstance(s, Info) else s.State for s in states])
        blist = (ctypes.c_uint16 * len(bands))(*[int(b) for b in bands])
        if nrows_out is None:
            nrows_out = len(bands) * int(band_rows)
        check(lib.sdfhip_render_bands_device(self._h, infos, len(states), ctypes.byref(pt) if pt is not None else None,
                                             int(width), int(height), int(band_rows), blist, len(bands),
                                             int(nrows_out), int(flags), ctypes.c_void_p(int(out_ptr)),
                                             ctypes.c_void_p(int(stream)) if stream else None,
                                             ctypes.byref(stats) if stats is not None else None))

    def DrawPath(self, state, width, height, pt=None, flags=_lib.KERNEL_AUTO, want_stats=False):
        """Path-traced frame (BASELINE config 5; defined by the oracle's o_pixel_pt): host array
        (H, W, 4) float32, mean radiance + step count."""
        pt = pt if pt is not None else PathTrace()
        out = np.empty((int(height), int(width), 4), dtype=np.float32)
        st = Stats()
        info = state if isinstance(state, Info) else state.State
        check(lib.sdfhip_render_path(self._h, ctypes.byref(info), ctypes.byref(pt), int(width), int(height),
                                     int(flags), out.ctypes.data, ctypes.byref(st) if want_stats else None))
        return (out, st) if want_stats else out

    def DrawPathDevice(self, state, width, height, out_ptr, pt=None, nrows_out=None, band_rows=None,
                       band_first=0, band_stride=1, flags=_lib.KERNEL_AUTO, stream=None, stats=None):
        pt = pt if pt is not None else PathTrace()
        info = state if isinstance(state, Info) else state.State
        if nrows_out is None:
            nrows_out = height
        if band_rows is None:
            band_rows = height
        check(lib.sdfhip_render_path_device(self._h, ctypes.byref(info), ctypes.byref(pt), int(width),
                                            int(height), int(band_rows), int(band_first), int(band_stride),
                                            int(nrows_out), int(flags), ctypes.c_void_p(int(out_ptr)),
                                            ctypes.c_void_p(int(stream)) if stream else None,
                                            ctypes.byref(stats) if stats is not None else None))

    def DrawDisplay(self, state, width, height, debug=False, flags=_lib.KERNEL_AUTO, want_stats=False, out=None):
        """Render + display pass (DisplayFrag.hlsl) fused: host array (H, W, 4) uint8, R,G,B,A.
        debug=True gives the step-count heat map of DisplayFrag.hlsl:21-22.  out: reuse this array."""
        if out is None:
            out = np.empty((int(height), int(width), 4), dtype=np.uint8)
        elif out.shape != (int(height), int(width), 4) or out.dtype != np.uint8 or not out.flags.c_contiguous:
            raise ValueError("DrawDisplay: out must be a C-contiguous uint8 array of shape (height, width, 4)")
        st = Stats()
        info = state if isinstance(state, Info) else state.State
        check(lib.sdfhip_render_display(self._h, ctypes.byref(info), int(width), int(height), int(flags),
                                        1 if debug else 0, out.ctypes.data,
                                        ctypes.byref(st) if want_stats else None))
        return (out, st) if want_stats else out

    def DrawDevice(self, state, width, height, out_ptr, nrows_out=None, band_rows=None,
                   band_first=0, band_stride=1, flags=_lib.KERNEL_AUTO, stream=None, stats=None):
        """Render into device memory at `out_ptr` (nrows_out x width x 4 floats),
        asynchronously on `stream` (a raw hipStream_t value or None)."""
        info = state if isinstance(state, Info) else state.State
        if nrows_out is None:
            nrows_out = height
        if band_rows is None:
            band_rows = height
        check(lib.sdfhip_render_device(self._h, ctypes.byref(info), int(width), int(height),
                                       int(band_rows), int(band_first), int(band_stride),
                                       int(nrows_out), int(flags), ctypes.c_void_p(int(out_ptr)),
                                       ctypes.c_void_p(int(stream)) if stream else None,
                                       ctypes.byref(stats) if stats is not None else None))

    def step_classes(self, stream=None):
        """After a FLAG_COUNT DrawDevice on `stream`: lane-steps by the kind of cell they sampled
        (sdfhip_debug_step_classes)."""
        _lib.need_lab("Scene.step_classes")
        out = (ctypes.c_uint64 * 6)()
        check(lib.sdfhip_debug_step_classes(self._h, ctypes.c_void_p(int(stream)) if stream else None, out))
        return dict(zip(("flat_coarse", "flat_fine", "nonflat_coarse", "nonflat_full_depth", "nonflat_between", "nonflat_outside"),
                        (int(v) for v in out)))

    def touch_begin(self):
        """From here to touch_end() every FLAG_COUNT render marks the 128-byte lines of the lookup grid its find() touches, per XCD
        (sdfhip_debug_touch_begin; laboratory library)."""
        _lib.need_lab("Scene.touch_begin")
        check(lib.sdfhip_debug_touch_begin(self._h))

    def touch_end(self):
        """-> {"phases": [{"grid": "own" | "bounce", "coarse_lines", "fine_lines", "coarse_lines_xcd_sum", "fine_lines_xcd_sum"}, ...],
        "array_bytes": {"coarse", "fine", "coarse2", "fine2"}}: the distinct lines each counted launch touched (a frame of the
        default kernel is one phase; a path-traced frame is its camera segments and then one phase per bounce level), chip-wide and
        summed over the XCDs (sdfhip_debug_touch_end)."""
        _lib.need_lab("Scene.touch_end")
        out = (ctypes.c_uint64 * (16 * 8))()
        n = ctypes.c_uint32(0)
        ab = (ctypes.c_uint64 * 4)()
        check(lib.sdfhip_debug_touch_end(self._h, out, 16, ctypes.byref(n), ab))
        phases = [{"grid": "own" if int(out[8 * i + 4]) == 0 else "bounce", "coarse_lines": int(out[8 * i]), "fine_lines": int(out[8 * i + 1]),
                   "coarse_lines_xcd_sum": int(out[8 * i + 2]), "fine_lines_xcd_sum": int(out[8 * i + 3])} for i in range(n.value)]
        return {"phases": phases, "array_bytes": dict(zip(("coarse", "fine", "coarse2", "fine2"), (int(v) for v in ab)))}


class MultiScene:
    """A scene replicated on several GPUs of one node; a frame is ONE call (sdfhip_multi_*: bands dealt to the devices,
    sparse wire shares gathered into devices[0] over xGMI, assembled there).  `devices` may repeat a device
    (rehearsal of the pipeline on one GPU)."""

    def __init__(self, octdata, devices):
        self._h = ctypes.c_void_p()
        self.devices = [int(d) for d in devices]
        arr = (ctypes.c_int * len(self.devices))(*self.devices)
        check(lib.sdfhip_multi_create(arr, len(self.devices), octdata.Structs.ctypes.data, octdata.Values.ctypes.data,
                                      octdata.Length, ctypes.byref(self._h)))

    def close(self):
        if self._h:
            lib.sdfhip_multi_free(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def configure(self, band_rows=16, rank0_weight=1.0):
        check(lib.sdfhip_multi_configure(self._h, int(band_rows), float(rank0_weight)))

    def selftest(self):
        """First contact with the node's links (sdfhip_multi_selftest; create runs it too): per device its PCI bus id, whether it
        reaches devices[0]'s memory directly, and whether a 1 MB pattern pushed the gather's way arrived intact.  Raises
        SdfHipError naming the pair when one did not."""
        links = (_lib.MultiLink * len(self.devices))()
        check(lib.sdfhip_multi_selftest(self._h, links))
        return [{"device": l.device, "pci_bus_id": l.pci_bus_id.decode(), "peer_access": l.peer_access, "ok": bool(l.ok), "push_ms": l.push_ms}
                for l in links]

    @property
    def transport(self):
        t = ctypes.c_int()
        check(lib.sdfhip_multi_info(self._h, None, None, None, None, ctypes.byref(t)))
        return "rccl" if t.value else "peer"

    def Draw(self, state, width, height, flags=0, pt=None, want_stats=False, out=None):
        """One frame across the devices to a host array: (H, W, 4) float32, or uint8 with FLAG_DISPLAY[_DEBUG]."""
        display = bool(flags & (_lib.FLAG_DISPLAY | _lib.FLAG_DISPLAY_DEBUG))
        want = np.uint8 if display else np.float32
        if out is None:
            out = np.empty((int(height), int(width), 4), dtype=want)
        elif not isinstance(out, np.ndarray) or out.shape != (int(height), int(width), 4) or out.dtype != want or \
                not out.flags.c_contiguous or not out.flags.writeable:
            raise ValueError(f"MultiScene.Draw: out must be a writeable C-contiguous {np.dtype(want).name} array of shape (height, width, 4)")
        st = MultiStats()
        stp = ctypes.byref(st) if want_stats else None             # (statistics cost an event per rank: only when asked for)
        info = state if isinstance(state, Info) else state.State
        if pt is not None:
            check(lib.sdfhip_multi_render_path(self._h, ctypes.byref(info), ctypes.byref(pt), int(width), int(height), int(flags),
                                               out.ctypes.data, stp))
        else:
            check(lib.sdfhip_multi_render(self._h, ctypes.byref(info), int(width), int(height), int(flags), out.ctypes.data, stp))
        return (out, st) if want_stats else out

    def Submit(self, slot, states, width, height, flags=0, out_ptr=None, pt=None):
        """A group of frames (one camera block each) into slot 0..3; frames land in device memory of devices[0]."""
        if not isinstance(states, (list, tuple)):
            states = [states]
        infos = (Info * len(states))(*[s if isinstance(s, Info) else s.State for s in states])
        dst = ctypes.c_void_p(int(out_ptr)) if out_ptr else None
        if pt is not None:
            check(lib.sdfhip_multi_submit_path(self._h, int(slot), infos, ctypes.byref(pt), int(width), int(height), int(flags), dst))
        else:
            check(lib.sdfhip_multi_submit(self._h, int(slot), infos, len(states), int(width), int(height), int(flags), dst))

    def Wait(self, slot, want_stats=False):
        """Block until the slot's frames are complete; returns the device pointer of its frames (and the stats)."""
        p = ctypes.c_void_p()
        st = MultiStats()
        check(lib.sdfhip_multi_wait(self._h, int(slot), ctypes.byref(p), ctypes.byref(st)))
        return (p.value, st) if want_stats else p.value

    def debug_floats_sent(self, floats):
        _lib.need_lab("MultiScene.debug_floats_sent")
        check(lib.sdfhip_multi_debug_floats_sent(self._h, int(floats)))


class TriMesh:
    """A triangle mesh prepared for the exact signed-distance builder (sdfhip_trimesh_prepare / sdfhip_trimesh_build): per triangle
    kept a 32-float record -- a b c, face normal, angle-weighted pseudonormals of its edges and vertices, source index."""

    def __init__(self, vertices, stride, fit=None, fill=None):
        v = np.ascontiguousarray(vertices, dtype=np.float32).reshape(-1, 3 * stride)
        opt = _lib.TriMeshOptions(fit, fill)
        self._raw = _lib.CTriMesh()
        check(lib.sdfhip_trimesh_prepare(v.ctypes.data, len(v), int(stride), ctypes.byref(opt), ctypes.byref(self._raw)))
        r = self._raw
        self.n_vertices, self.n_edges, self.n_dropped, self.open_edges = r.n_vertices, r.n_edges, r.n_dropped, r.open_edges
        self.scale, self.offset = r.scale, tuple(r.offset)

    @classmethod
    def FromSoup(cls, triangles, fit=None, fill=None):
        """triangles: (n, 3, 3) float32 positions, counter-clockwise seen from outside."""
        return cls(np.ascontiguousarray(triangles, dtype=np.float32).reshape(-1, 3, 3), 3, fit, fill)

    @classmethod
    def FromMesh(cls, triangles, fit=None, fill=None):
        """triangles: (n, 3, 6) float32 {position, normal} as Scene.Mesh returns them; the normals are ignored."""
        return cls(np.ascontiguousarray(triangles, dtype=np.float32).reshape(-1, 3, 6), 6, fit, fill)

    @classmethod
    def LoadPly(cls, path, fit=None, fill=None):
        return cls.FromMesh(LoadMeshPly(path), fit, fill)

    @classmethod
    def LoadObj(cls, path, fit=None, fill=None):
        return cls.FromMesh(LoadMeshObj(path), fit, fill)

    @property
    def n_records(self):
        return self._raw.n_records

    @property
    def records(self):
        """(n_records, 32) float32: a view of the library's memory, valid until close()."""
        n = self._raw.n_records
        return np.ctypeslib.as_array(self._raw.records, shape=(n, 32)) if n else np.zeros((0, 32), np.float32)

    def Build(self, depth, device=0, want_octdata=False, want_scene=True, want_stats=False):
        """The mesh's exact signed distance field as a Scene on `device` (the tree never leaves HBM), and / or its host arrays."""
        return Scene._built(device, _lib.TriMeshStats(), lambda h, raw, st: lib.sdfhip_trimesh_build(int(device), ctypes.byref(self._raw), int(depth), h, raw, st),
                            want_octdata, want_stats, want_scene)

    def close(self):
        if self._raw.records:
            lib.sdfhip_trimesh_free(ctypes.byref(self._raw))

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def _load_mesh(fn, path):
    raw = _lib.CMesh()
    check(fn(os.fsencode(str(path)), ctypes.byref(raw)))
    try:
        n = raw.n_triangles
        return np.ctypeslib.as_array(raw.verts6, shape=(n, 3, 6)).copy() if n else np.zeros((0, 3, 6), np.float32)
    finally:
        lib.sdfhip_mesh_free(ctypes.byref(raw))


def LoadMeshPly(path):
    """sdfhip_load_ply_mesh: a binary little-endian .ply WITH its faces as an (n, 3, 6) float32 soup (polygons fanned)."""
    return _load_mesh(lib.sdfhip_load_ply_mesh, path)


def LoadMeshObj(path):
    """sdfhip_load_obj_mesh: an .obj WITH its faces as an (n, 3, 6) float32 soup (polygons fanned; normals from the file, else 0)."""
    return _load_mesh(lib.sdfhip_load_obj_mesh, path)


def _as_mesh(triangles):
    t = np.ascontiguousarray(triangles, dtype=np.float32).reshape(-1, 3, 6)
    raw = _lib.CMesh(len(t), t.ctypes.data_as(ctypes.POINTER(ctypes.c_float)))
    return t, raw


def SaveMeshPly(path, triangles):
    """(n, 3, 6) float32 triangles -> binary little-endian .ply, vertices {x y z nx ny nz} then faces (sdfhip_mesh_save_ply):
    OctData.LoadPly reads the vertices back."""
    import os
    keep, raw = _as_mesh(triangles)
    check(lib.sdfhip_mesh_save_ply(ctypes.byref(raw), os.fsencode(path)))


def SaveMeshObj(path, triangles):
    """(n, 3, 6) float32 triangles -> .obj with `v`, `vn` (%.9g) and `f a//a b//b c//c` lines (sdfhip_mesh_save_obj)."""
    import os
    keep, raw = _as_mesh(triangles)
    check(lib.sdfhip_mesh_save_obj(ctypes.byref(raw), os.fsencode(path)))


def device_pci_bus_id(device=0):
    out = ctypes.create_string_buffer(32)
    check(lib.sdfhip_device_pci_bus_id(int(device), out, 32))
    return out.value.decode()


def device_bandwidth(device=0, nbytes=2 << 30, reps=10):
    """(copy, triad, read) GB/s of the device's memory for a streaming kernel (sdfhip_device_bandwidth): arrays of nbytes each."""
    c, t, r = ctypes.c_double(), ctypes.c_double(), ctypes.c_double()
    check(lib.sdfhip_device_bandwidth(int(device), int(nbytes), int(reps), ctypes.byref(c), ctypes.byref(t), ctypes.byref(r)))
    return c.value, t.value, r.value


def sdfgen_trim():
    """Give back the device memory the point-cloud builder keeps between builds (sdfhip_sdfgen_trim)."""
    check(lib.sdfhip_sdfgen_trim())


def device_count():
    n = ctypes.c_int()
    check(lib.sdfhip_device_count(ctypes.byref(n)))
    return n.value


def unorm_table(device=0):
    _lib.need_lab("unorm_table")
    out = np.empty(256, dtype=np.float32)
    check(lib.sdfhip_debug_unorm_table(int(device), out.ctypes.data))
    return out
