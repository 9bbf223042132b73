"""Cross-sections (sdfhip_scene_slice) without a GPU.  The numpy restatement of the rule (tests/slice_restatement.py; DESIGN.md section 8,
N18) is held here to things it did not make -- the record counts a prototype of the rule gave on the golden trees, contours that close
point for point, the orientation and size of the sphere's sections, a float64 slice of the same triangles written another way -- so that
tests/test_gpu_slice.py, which holds the GPU to the restatement byte for byte, is not the author's code compared with the author's
code.  And the ABI as far as it goes without a device: names, record sizes, the defaults, the host-only argument errors, the helpers."""
import ctypes

import numpy as np
import pytest

import mesh_restatement as mr
import slice_restatement as sr

f32 = np.float32
SLICE_SYMBOLS = ("sdfhip_slice_options_default", "sdfhip_scene_slice", "sdfhip_scene_slice_device", "sdfhip_slice_free")

AXIS = ((0.0, 0.0, 1.0), 0.21, 0.0625, 10)
FACES = ((0.0, 1.0, 0.0), 0.25, 0.03125, 17)               # dyadic: the planes lie on cell faces
OBLIQUE = ((0.6, 0.0, 0.8), 0.3, 0.05, 12)

_meshed = {}


def meshed(scenes, name, level):
    """the mesh restatement's triangles, nodes and cell counts, made once"""
    if (name, level) not in _meshed:
        od = scenes[name]
        _meshed[name, level] = mr.mesh(od.Structs, od.Values, level, want_cells=True)
    return _meshed[name, level]


def sliced(scenes, name, level, plane):
    od = scenes[name]
    return sr.slice_scene(od.Structs, od.Values, *plane, level, meshed=meshed(scenes, name, level))


# the counts of a prototype of the rule (the issue that asked for the feature): segments and, where it gave them, zero-length segments
@pytest.mark.parametrize("name, level, plane, segments, zero_length",
                         [("sphere_d4", -1, AXIS, 1040, 0), ("sphere_d4", -1, FACES, 1986, 532), ("sphere_d4", 3, AXIS, 526, None),
                          ("torus_d6", -1, AXIS, 3430, None), ("torus_d6", -1, OBLIQUE, 4102, 219)])
def test_the_prototypes_counts(scenes, name, level, plane, segments, zero_length):
    rec, counts, (cells, cut, crossed) = sliced(scenes, name, level, plane)
    assert len(rec) == segments and int(counts.sum()) == segments
    if zero_length is not None:
        assert sr.zero_length(rec) == zero_length
    assert (np.diff(rec["node"].astype(np.int64)) >= 0).all()                # node-major
    same_node = np.diff(rec["node"].astype(np.int64)) == 0
    assert 0 < crossed <= cut and crossed == len(np.unique(rec["node"]))
    # every record's node is a cut cell of the mesh
    assert np.isin(rec["node"], meshed(scenes, name, level)[1]).all()
    assert same_node.any()


@pytest.mark.parametrize("name", ["sphere_d4", "torus_d6"])
@pytest.mark.parametrize("level", [-1, 3])
@pytest.mark.parametrize("plane", [AXIS, FACES, OBLIQUE], ids=["axis", "faces", "oblique"])
def test_every_layer_is_closed_point_for_point(sb, scenes, name, level, plane):
    rec, counts, _ = sliced(scenes, name, level, plane)
    seg, starts = sr.by_layer(rec, plane[3])
    assert len(seg) > 100 and starts[-1] == len(seg)
    for k in range(plane[3]):
        layer = seg[starts[k]:starts[k + 1]]
        assert (layer["layer"] == k).all()
        assert sr.balance(layer) == 0, (name, level, k)
        loops = sb.slice_loops(layer)
        assert sum(len(l) - 1 for l in loops) == len(layer) - sr.zero_length(layer)
        for l in loops:
            assert len(l) >= 4 and l[0].tobytes() == l[-1].tobytes()
        assert (len(loops) > 0) == (len(layer) > sr.zero_length(layer))


def test_the_spheres_sections_are_counter_clockwise_discs_inside_the_meshs_radius(sb, scenes):
    # the mesh's vertices lie within radius 0.3008 of the centre (include/sdfhip.h, N12) and a contour lies in their hull
    normal, offset, pitch, layers = AXIS
    rec, counts, _ = sliced(scenes, "sphere_d4", -1, AXIS)
    seg, starts = sr.by_layer(rec, layers)
    areas = sb.slice_areas(seg, starts, normal)
    assert areas.dtype == np.float64 and len(areas) == layers and (counts > 0).sum() == layers
    for k in range(layers):
        h = offset + k * pitch
        disc = np.pi * (0.3008 ** 2 - (h - 0.5) ** 2)
        print(f"layer {k}: h = {h:.4f}, {counts[k]} records, area {areas[k]:.6f}, disc {disc:.6f}")
        assert 0 < areas[k] <= disc, k
    assert abs(areas[5] - 0.2725) < 5e-4                       # the prototype's mid layer, against the disc's 0.2827
    # one loop per layer, counter-clockwise seen from +z
    for k in range(layers):
        loops = sb.slice_loops(seg[starts[k]:starts[k + 1]])
        assert len(loops) == 1
        p = loops[0].astype(np.float64)
        assert 0.5 * (p[:-1, 0] * p[1:, 1] - p[1:, 0] * p[:-1, 1]).sum() > 0


def test_the_torus_has_a_hole_and_its_loops_run_the_other_way(sb, scenes):
    # a plane square to the torus' axis (y), just off its middle: an annulus -- an outer counter-clockwise loop and a clockwise inner one
    normal = (0.0, 1.0, 0.0)
    rec, counts, _ = sliced(scenes, "torus_d6", -1, (normal, 0.51, 0.0, 1))
    loops = sb.slice_loops(rec)
    u, v = sb.slice_basis(normal)
    signed = sorted(0.5 * ((p[:-1] @ u) * (p[1:] @ v) - (p[1:] @ u) * (p[:-1] @ v)).sum() for p in (l.astype(np.float64) for l in loops))
    assert len(loops) == 2 and signed[0] < 0 < signed[1] and signed[1] > -signed[0], signed
    assert abs(sb.slice_areas(rec, [0, len(rec)], normal)[0] - (signed[0] + signed[1])) < 1e-12
    # and through the tube, along the axis: two discs, both counter-clockwise
    rec, counts, _ = sliced(scenes, "torus_d6", -1, ((0.0, 0.0, 1.0), 0.51, 0.0, 1))
    loops = sb.slice_loops(rec)
    assert len(loops) == 2
    for p in (l.astype(np.float64) for l in loops):
        assert 0.5 * (p[:-1, 0] * p[1:, 1] - p[1:, 0] * p[:-1, 1]).sum() > 0


def test_a_negated_normal_with_negated_offsets_gives_the_same_points_exchanged(scenes):
    tris = meshed(scenes, "sphere_d4", -1)[0][:, :, :3]
    for normal, offset, pitch, layers in (AXIS, OFF_LATTICE):
        h = sr.heights(offset, pitch, layers)
        hit = np.unique(sr.slice_triangles(tris, normal, offset, pitch, layers)["layer"])
        for k in (hit[0], hit[len(hit) // 2], hit[-1]):
            fwd = sr.slice_triangles(tris, normal, float(h[k]), 0.0, 1)
            rev = sr.slice_triangles(tris, tuple(-x for x in normal), -float(h[k]), 0.0, 1)
            # d and h change sign together, so `above` becomes `not above` except where d == h exactly, which these stacks avoid
            on_plane = (sr.vertex_heights(tris, normal) == h[k]).any()
            assert len(fwd) > 0 and not on_plane
            # The heights negate exactly (d, h, sa and sb change sign bit for bit), so the same triangles cross, in the same order.  But
            # the rule walks every edge from its below end, which is now the other end: t' = sb / (sb - sa) and q' = b + (a - b) * t'
            # where it was t = sa / (sa - sb) and q = a + (b - a) * t.  t + t' = 1 within 2u (u = 2^-24), and each point rounds a
            # product and a sum of terms below 1: the two agree within 8u = 2^-21 per coordinate, not bit for bit.
            assert len(fwd) == len(rev) and (fwd["node"] == rev["node"]).all()
            worst = max(float(np.abs(fwd["a"].astype(np.float64) - rev["b"]).max()), float(np.abs(fwd["b"].astype(np.float64) - rev["a"]).max()))
            print(f"normal {normal}, h = {float(h[k]):.4f}: {len(fwd)} records, a and b exchanged within {worst:.3e}")
            assert worst <= 2.0 ** -21


# OBLIQUE's planes pass through lattice points by design: a vertex on a y-edge has x = i / 64 and z = j / 64, and 0.6 x + 0.8 z = (3 i + 4 j) / 320
# takes the values 0.3 + 0.05 k exactly.  For the comparison of counts the stack is moved off them: (0.3013 + 0.05 k) * 320 is 0.416 away from
# an integer, 1.3e-3 in height
OFF_LATTICE = ((0.6, 0.0, 0.8), 0.3013, 0.05, 12)


# ---- an independent route: the same triangles sliced in float64, written another way -------------------------------------------------
def slice64(tris, normal, h):
    """per triangle and plane: the two points where the plane meets the triangle's outline, by clipping each edge p + s (q - p) at
    s = (h - n.p) / (n.q - n.p) -- not the restatement's below-to-above form.  -> (mask of crossed triangles, (m, 2, 3) points, margin),
    margin = the smallest |n.p - h| over all vertices"""
    P = tris.astype(np.float64)
    n = np.asarray(normal, np.float64)
    d = P @ n
    side = d >= h
    crossed = side.any(1) & ~side.all(1)
    pts = np.zeros((int(crossed.sum()), 2, 3))
    filled = np.zeros(len(pts), dtype=np.int64)
    Pc, dc, sc = P[crossed], d[crossed], side[crossed]
    for e in range(3):
        f = (e + 1) % 3
        w = np.nonzero(sc[:, e] != sc[:, f])[0]
        s = (h - dc[w, e]) / (dc[w, f] - dc[w, e])
        pts[w, filled[w]] = Pc[w, e] + s[:, None] * (Pc[w, f] - Pc[w, e])
        filled[w] += 1
    assert (filled == 2).all()
    return crossed, pts, float(np.abs(d - h).min())


def distance_to_line(q, p0, p1):
    u = p1 - p0
    length = np.linalg.norm(u, axis=1)
    w = q - p0
    along = np.where(length > 0, np.einsum("ij,ij->i", w, u) / np.where(length > 0, length, 1.0), 0.0)
    return np.sqrt(np.maximum(np.einsum("ij,ij->i", w, w) - along ** 2, 0.0))


@pytest.mark.parametrize("name", ["sphere_d4", "torus_d6"])
def test_agreement_with_a_float64_slice_of_the_same_triangles(scenes, name):
    """Offsets 0.21 + k / 16 along z and 0.3013 + 0.05 k along the unit normal (0.6, 0, 0.8).  A float32 endpoint is a dozen roundings at
    magnitudes <= 2 away from its plane and from its edge's line: 2^-20.  The counts are compared on the layers where no vertex is
    within 2^-20 of the plane (there float32 and float64 may put a vertex on different sides); at most a tenth of the layers may be
    excluded that way."""
    BOUND = 2.0 ** -20
    tris = meshed(scenes, name, -1)[0][:, :, :3]
    excluded = total = 0
    worst_plane = worst_line = worst_point = 0.0
    for normal, offset, pitch, layers in (AXIS, OFF_LATTICE):
        assert abs(np.linalg.norm(normal) - 1.0) < 1e-12
        rec = sr.slice_triangles(tris, normal, offset, pitch, layers, nodes=np.arange(len(tris)))       # `node`: the triangle's index
        h = sr.heights(offset, pitch, layers).astype(np.float64)
        n64 = np.asarray(normal, np.float64)
        for k in range(layers):
            layer = rec[rec["layer"] == k]
            crossed, pts, margin = slice64(tris, normal, h[k])
            total += 1
            # every endpoint against its plane, and against the line of the triangle edge it sits on: the nearest of its own
            # triangle's three edge lines
            own = tris[layer["node"]].astype(np.float64)
            for end in ("a", "b"):
                q = layer[end].astype(np.float64)
                worst_plane = max(worst_plane, float(np.abs(q @ n64 - h[k]).max(initial=0.0)))
                line = np.min([distance_to_line(q, own[:, e], own[:, (e + 1) % 3]) for e in range(3)], axis=0)
                worst_line = max(worst_line, float(line.max(initial=0.0)))
            if margin < BOUND:
                excluded += 1
                continue
            assert len(layer) == int(crossed.sum()), (name, normal, k)
            assert (layer["node"] == np.nonzero(crossed)[0]).all()
            # each float32 endpoint against the float64 points of its own triangle (either order): reported, not bounded -- along an
            # edge that is nearly parallel to the plane the point moves by the heights' rounding over the edge's slope
            for end in ("a", "b"):
                q = layer[end].astype(np.float64)
                near = np.minimum(np.linalg.norm(q - pts[:, 0], axis=1), np.linalg.norm(q - pts[:, 1], axis=1))
                worst_point = max(worst_point, float(near.max(initial=0.0)))
    share = excluded / total
    print(f"{name}: {excluded} of {total} layers excluded ({share:.3f}); worst |dot(n, q) - h| {worst_plane:.3e}, worst distance to the edge's line {worst_line:.3e}, to the float64 point {worst_point:.3e}")
    assert worst_plane <= BOUND and worst_line <= BOUND
    assert share <= 0.10


# ---- corner cases -----------------------------------------------------------------------------------------------------------------

def test_layers_outside_the_cube_one_layer_and_an_unnormalised_normal(scenes):
    od = scenes["sphere_d4"]
    m = meshed(scenes, "sphere_d4", -1)
    for offset in (1.5, -4.0):
        rec, counts, (cells, cut, crossed) = sr.slice_scene(od.Structs, od.Values, (0, 0, 1), offset, 0.25, 8, meshed=m)
        assert len(rec) == 0 and counts.tolist() == [0] * 8 and crossed == 0 and cut == 416
        assert sr.by_layer(rec, 8)[1].tolist() == [0] * 9
    # part of the stack inside: the layers outside stay flat
    rec, counts, _ = sr.slice_scene(od.Structs, od.Values, (0, 0, 1), -0.5, 0.25, 8, meshed=m)
    assert counts[:3].tolist() == [0, 0, 0] and counts[3] > 0 and counts[6:].tolist() == [0, 0]
    # layers = 1 ignores the pitch
    one = sr.slice_scene(od.Structs, od.Values, (0, 0, 1), 0.4, 0.0, 1, meshed=m)[0]
    assert len(one) > 0
    for pitch in (0.3, -2.0, 1e30):
        assert sr.slice_scene(od.Structs, od.Values, (0, 0, 1), 0.4, pitch, 1, meshed=m)[0].tobytes() == one.tobytes()
    # (0, 0, 2) with doubled offsets: scaling by two is exact, the same bits
    a = sr.slice_scene(od.Structs, od.Values, *AXIS, meshed=m)
    b = sr.slice_scene(od.Structs, od.Values, (0.0, 0.0, 2.0), 2 * AXIS[1], 2 * AXIS[2], AXIS[3], meshed=m)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tolist() == b[1].tolist()


def test_the_helpers(sb):
    for normal in ((0, 0, 1), (0, 0, -3), (0.6, 0, 0.8), (1, 1, 1), (0, 2, 0), (-1, 0.5, 0.25)):
        u, v = sb.slice_basis(normal)
        n = np.asarray(normal, np.float64) / np.linalg.norm(normal)
        assert u.dtype == v.dtype == np.float64
        assert np.allclose([u @ u, v @ v, u @ v, u @ n, v @ n], [1, 1, 0, 0, 0], atol=1e-15)
        assert np.allclose(np.cross(u, v), n, atol=1e-15)          # right-handed with the normal
    assert [x.tolist() for x in sb.slice_basis((0, 0, 1))] == [[1, 0, 0], [0, 1, 0]]
    with pytest.raises(ValueError):
        sb.slice_basis((0, 0, 0))
    # a unit square walked counter-clockwise in the plane z = 2, a zero-length record among its sides, and a clockwise hole
    sq = np.array([[0, 0, 2], [1, 0, 2], [1, 1, 2], [0, 1, 2]], f32)
    hole = np.array([[0.25, 0.25, 2], [0.25, 0.75, 2], [0.75, 0.75, 2], [0.75, 0.25, 2]], f32)
    seg = np.zeros(9, sr.SEGMENT)
    assert sb.slices.SEGMENT == sr.SEGMENT
    seg["a"][:4], seg["b"][:4] = sq, np.roll(sq, -1, 0)
    seg["a"][4] = seg["b"][4] = sq[2]
    seg["a"][5:], seg["b"][5:] = hole, np.roll(hole, -1, 0)
    seg = seg[[3, 5, 0, 4, 8, 2, 6, 1, 7]]                         # in no order
    assert sb.slice_areas(seg, [0, 9], (0, 0, 5)).tolist() == [0.75]
    assert sb.slice_areas(seg, [0, 0, 9, 9], (0, 0, 1)).tolist() == [0.0, 0.75, 0.0]
    loops = sb.slice_loops(seg)
    assert sorted(len(l) for l in loops) == [5, 5] and all(l[0].tobytes() == l[-1].tobytes() for l in loops)
    assert sb.slice_loops(seg[:0]) == []
    with pytest.raises(ValueError):
        sb.slice_loops(seg[seg["a"][:, 0] > 0])                    # the square and the hole without some of their sides


# ---- the ABI without a device ----------------------------------------------------------------------------------------------

def test_the_library_exports_the_slice_entry_points_and_record_sizes(sb):
    import sdfbox_amd.lab
    for pkg in (sb, sdfbox_amd.lab.load()):
        L = pkg._lib
        for name in SLICE_SYMBOLS:
            assert hasattr(L.lib, name) and name in L.EXPORTED_SYMBOLS
        assert (ctypes.sizeof(L.Segment), ctypes.sizeof(L.SliceOptions), ctypes.sizeof(L.CSlice), ctypes.sizeof(L.SliceStats)) == (32, 32, 32, 28)
        assert sr.SEGMENT.itemsize == 32 and [sr.SEGMENT.fields[f][1] for f in ("a", "layer", "b", "node")] == [0, 12, 16, 28]
        assert [getattr(L.Segment, f).offset for f in ("a", "layer", "b", "node")] == [0, 12, 16, 28]
        opt = L.SliceOptions((1, 2, 3), 9.0, 9.0, 9, 9)
        opt.size = 0
        L.lib.sdfhip_slice_options_default(ctypes.byref(opt))
        assert (opt.size, opt.level, list(opt.normal), opt.offset, opt.pitch, opt.layers) == (32, -1, [0.0, 0.0, 1.0], 0.5, 0.0, 1)
        L.lib.sdfhip_slice_options_default(None)                   # a null pointer is not a crash
        py = L.SliceOptions()
        assert bytes(py) == bytes(opt)                             # the binding's defaults are the library's


def test_null_arguments_are_status_codes_and_free_twice_is_safe(sb):
    L = sb._lib
    out, st, n = L.CSlice(), L.SliceStats(), ctypes.c_uint32(7)
    out.n_segments, out.layers = 3, 4
    assert L.lib.sdfhip_scene_slice(None, None, ctypes.byref(out), ctypes.byref(st)) == L.ERR_ARG and L.lib.sdfhip_last_error()
    assert (out.n_segments, out.layers) == (0, 0) and not out.segments and not out.layer_counts      # zeroed on failure
    assert L.lib.sdfhip_scene_slice(None, None, None, None) == L.ERR_ARG
    assert L.lib.sdfhip_scene_slice_device(None, None, None, 0, None, ctypes.byref(n), None) == L.ERR_ARG
    assert L.lib.sdfhip_scene_slice_device(None, None, None, 0, None, None, None) == L.ERR_ARG
    # sdfhip_slice_free: what malloc made, twice, and on null
    libc = ctypes.CDLL(None)
    libc.malloc.restype = ctypes.c_void_p
    owned = L.CSlice(2, ctypes.cast(libc.malloc(64), ctypes.POINTER(L.Segment)), 3, ctypes.cast(libc.malloc(12), ctypes.POINTER(ctypes.c_uint32)))
    L.lib.sdfhip_slice_free(ctypes.byref(owned))
    assert (owned.n_segments, owned.layers) == (0, 0) and not owned.segments and not owned.layer_counts
    L.lib.sdfhip_slice_free(ctypes.byref(owned))
    L.lib.sdfhip_slice_free(None)
