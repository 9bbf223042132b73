"""Volumes in and out (sdfhip_volume_build, sdfhip_scene_volume) without a GPU: the CPU restatement (tests/volume_restatement.py) is
held to things it did not come from -- the analytic builder's sphere, cell for cell; the exactness of a lattice's vertices; the
continuation outside the lattice's box; the structure of a breadth-first tree; what a truncated field does to the split rule -- the
entry points refuse what they must refuse before they touch a device, and the Python mirror's records are the header's.
tests/test_gpu_volume.py holds the GPU to the restatement byte for byte."""
import ctypes
import os
import re

import numpy as np
import pytest

import volume_cases as vc
import volume_restatement as vr
from conftest import REPO
from test_combine import assert_breadth_first

f32 = np.float32
EPS = 2.0 ** -24                               # half an ulp of 1: the relative error of one fp32 operation


def test_the_analytic_sphere_cell_for_cell(sb):
    # the 17^3 grid of |p - 0.5| - 0.3 holds the analytic field at every point a depth-4 build evaluates, and vertices are exact: the
    # tree is sphere_d4's, whatever order its builder numbers the nodes in
    S, V, _ = vc.restated("sphere17_d4")
    od = sb.sphere_d4()
    want, got = vc.cells(od.Structs, od.Values), vc.cells(S, V)
    assert len(S) == od.Length == 3465 and len(want) == 3465
    differing = [k for k in want if got.get(k) != want[k]]
    assert set(got) == set(want) and not differing, (len(set(got) ^ set(want)), differing[:5])


@pytest.mark.parametrize("name", ["two_d3", "sphere17_d4", "aniso_inset_d5", "voxel_units_d5", "torus33_f16_d6", "tsdf_d6"])
def test_a_vertex_reads_its_sample_bit_for_bit(name):
    c = vc.case(name)
    grid = c["grid"]
    p = vr.lattice_points(grid.shape, c["origin"], c["spacing"])
    got = vr.value(grid, p, c["origin"], c["spacing"], c["value_scale"])
    want = grid.reshape(-1).astype(f32) * f32(c["value_scale"])
    # (u * 1 + v * 0 turns a sample of -0 into +0: none of these grids holds one)
    assert not (grid == 0).any() or not np.signbit(grid[grid == 0]).any()
    if name != "aniso_inset_d5":
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), name
        # the last planes are read through i = n - 2, f = 1
        nz, ny, nx = grid.shape
        i, f, e = vr.axis(p[:, 0], f32(c["origin"][0]), f32(1) / f32(c["spacing"]), f32(c["spacing"]), nx)
        last = p[:, 0] == p[:, 0].max()
        assert (i[last] == nx - 2).all() and (f[last] == 1).all() and (e == 0).all()
    else:
        # origin + (float)i * spacing is rounded where the spacing is no dyadic: the point is the vertex to within an ulp, and the
        # value is the sample to within the field's slope (1) times that, plus the interpolation's own roundings
        assert np.abs(got.astype(np.float64) - want).max() <= 8 * EPS, name
    # ... and with a negative scale, for a field that is positive inside
    neg = vr.value(grid, p[:500], c["origin"], c["spacing"], -c["value_scale"])
    assert np.array_equal(neg, -got[:500])


@pytest.mark.parametrize("name", ["sphere17_d4", "aniso_inset_d5", "torus33_f16_d6"])
def test_the_field_continues_at_slope_one_outside_the_box(name):
    # a point at distance r from the box along an axis reads the value on the box's face plus r.  `on` lies on the face -- at the
    # origin's coordinate, where g = 0 and e = 0 exactly, or at the last plane's where that is a float (the dyadic lattices), else
    # 1e-3 past it -- and `out` lies r further along the axis: both clamp to the same point of the face, so they read the same D
    c = vc.case(name)
    grid, h = c["grid"], float(f32(c["spacing"]))
    o = np.array(c["origin"], dtype=f32).astype(np.float64)
    n = np.array(grid.shape[::-1])
    hi = o + (n - 1) * h
    rng = np.random.default_rng(7)
    for a in range(3):
        for side in (0, 1):
            on = (o + rng.uniform(0.05, 0.95, size=(200, 3)) * (hi - o)).astype(f32)
            on[:, a] = f32(o[a]) if side == 0 else f32(hi[a]) if float(f32(hi[a])) == hi[a] else f32(hi[a] + 1e-3)
            assert side == 0 or (on[:, a] >= hi[a]).all()
            r = rng.uniform(0.01, 0.7, size=200).astype(f32)
            out = on.copy()
            out[:, a] = on[:, a] - r if side == 0 else on[:, a] + r
            far = np.abs(out[:, a].astype(np.float64) - on[:, a].astype(np.float64))
            base = vr.value(grid, on, c["origin"], h, c["value_scale"])
            got = vr.value(grid, out, c["origin"], h, c["value_scale"])
            assert (got > base).all()
            # three roundings on the way to the lattice coordinate g (the subtraction, 1 / spacing, the product), each relative to
            # |p - origin|, for either point; then the product with the spacing, the square, the root and the final sum, each relative
            # to the distance or to the value
            bound = EPS * (3 * (np.abs(out[:, a] - o[a]) + np.abs(on[:, a] - o[a])) + 4 * (far + np.abs(got) + np.abs(base)))
            err = np.abs(got.astype(np.float64) - (base.astype(np.float64) + far))
            print(f"{name} axis {a} side {side}: max error {err.max():.3e}, bound there {bound[err.argmax()]:.3e}")
            assert (err <= bound).all(), (name, a, side)


@pytest.mark.parametrize("name", vc.NAMES)
def test_structure(sb, name):
    S, V, counts = vc.restated(name)
    assert len(S) == vc.NODES[name]
    assert assert_breadth_first(sb, S, V) == counts["depth_out"] == counts["levels"] - 1
    assert counts["samples"] == 9 + 35 * ((len(S) - 1) // 8)
    if name == "outside":
        assert len(S) == 1 and tuple(S[0]) == (-1, -1) and (V == 255).all(), "far outside: the root alone, every byte saturated"
    else:
        # (the 2^3 grid's field is flat, 0.566 everywhere: no centre is within 2 S of it below level 2)
        assert len(S) > 1 and counts["depth_out"] == (2 if name == "two_d3" else vc.case(name)["depth"])


def test_depth_zero_is_the_root_alone():
    c = vc.case("sphere17_d4")
    S, V = vr.build(c["grid"], c["origin"], c["spacing"], 0)
    assert len(S) == 1 and np.array_equal(V, vc.restated("sphere17_d4")[1][:1])


def test_the_cases_are_what_they_are_for():
    # a level that ends inside a workgroup of four blocks; a level past one chunk of the scan (1024 words of 32 nodes)
    blocks = [m // 8 for m in vc.level_sizes(vc.restated("aniso_inset_d5")[0])]
    assert blocks[4] == 262 and blocks[4] % 4
    assert vc.level_sizes(vc.restated("sphere17_d7")[0])[6] == 38016 > 32768
    # the anisotropic grid's box leaves part of the cube to the continuation, and its strides differ
    c = vc.case("aniso_inset_d5")
    assert c["grid"].shape == (21, 13, 9) and c["origin"][0] + 8 * c["spacing"] < 1 and c["origin"][2] > 0
    # the voxel-unit grid stores 32 times the distance
    assert np.abs(vc.case("voxel_units_d5")["grid"]).max() > 10 and vc.case("voxel_units_d5")["value_scale"] == 1 / 32
    assert vc.case("torus33_f16_d6")["grid"].dtype == np.float16


def test_the_second_rounds_cases_are_what_they_are_for():
    # depth 12 in the far corner: 12 levels, and blocks of the last level with all three coordinates above 2^10 -- bit 10 of the
    # packed y and of x set, the emit's doubling past 2^11
    for name in ("corner_d12", "corner_d12_f16"):
        S, _, counts = vc.restated(name)
        assert counts["depth_out"] == 12 and len(S) == vc.NODES[name] == 12433, name
        assert vc.level_sizes(S) == [1, 8, 32, 32, 32, 32, 56, 64, 160, 336, 936, 2488, 8256], name
        blocks = vc.last_blocks(S)
        assert len(blocks) == 8256 // 8 and (blocks > 2 ** 10).all(1).any() and blocks.max() < 2 ** 11, name
    c = vc.case("corner_d12")
    assert c["grid"].shape == (17, 17, 17) and c["spacing"] == 2.0 ** -11 and c["origin"][0] + 16 * c["spacing"] < 1
    assert vc.case("corner_d12_f16")["grid"].dtype == np.float16
    assert not np.array_equal(vc.restated("corner_d12")[1], vc.restated("corner_d12_f16")[1]), "the rounding to half moves bytes"
    # the cube strictly inside the grid's box, off its lattice
    c = vc.case("wraps_d5")
    nz, ny, nx = c["grid"].shape
    assert (nx, ny, nz) == (36, 37, 33) and max(c["origin"]) < 0 and all(o + (n - 1) * c["spacing"] > 1 for o, n in zip(c["origin"], (nx, ny, nz)))
    assert all((0 - o) / c["spacing"] % 1 > 0.01 for o in c["origin"])
    assert len(vc.restated("wraps_d5")[0]) == len(vc.restated("voxel_units_d5")[0]) == 13385
    # the middle of the cube along x, out of it on the negative side along y, with the surface inside the grid's box there
    c, was = vc.case("inset_negative_d5"), vc.case("aniso_inset_d5")
    assert c["grid"].shape == was["grid"].shape and c["spacing"] == was["spacing"]
    assert 0.25 < c["origin"][0] and c["origin"][0] + 8 * c["spacing"] < 0.75 and c["origin"][1] < -0.1 < 0.25 < c["origin"][1] + 12 * c["spacing"] < 1
    assert (c["grid"][:, :5, :] > 0).all() and (c["grid"] < 0).any(), "five planes lie below y = 0, outside the solid; the surface crosses the box"
    assert len(vc.restated("inset_negative_d5")[0]) == 4809
    # a negative scale: the negated grid's tree is sphere17_d4's, array for array
    c = vc.case("negative_scale_d4")
    assert c["value_scale"] == -1.0 and np.array_equal(c["grid"], -vc.case("sphere17_d4")["grid"])
    for a, b in zip(vc.restated("negative_scale_d4")[:2], vc.restated("sphere17_d4")[:2]):
        assert np.array_equal(a, b)
    # more samples than k_volume_check's 2048 workgroups of 256 threads; the same tree as the 17^3 grid's
    c = vc.case("sphere81_d4")
    assert c["grid"].size == 531441 > 2048 * 256
    for a, b in zip(vc.restated("sphere81_d4")[:2], vc.restated("sphere17_d4")[:2]):
        assert np.array_equal(a, b)
    # the edges of float16 are among the samples, the large ones do not overflow under either scale, and they move bytes
    edges = np.array(vc.HALF_EDGES, dtype=np.float16).view(np.uint16)
    assert sorted(edges.tolist()) == [0x0001, 0x0300, 0x0400, 0x7BFF, 0x8000, 0x8001, 0x8400, 0xFBFF]
    for name, scale in (("half_edges_d3", 1.0), ("half_edges_scaled_d3", 2.0 ** -16)):
        c = vc.case(name)
        bits = c["grid"].reshape(-1).view(np.uint16)
        assert c["grid"].dtype == np.float16 and c["grid"].shape == (9, 9, 9) and c["value_scale"] == scale, name
        assert all(int((bits == e).sum()) >= 3 for e in edges), name
        assert np.isfinite(c["grid"]).all() and len(vc.restated(name)[0]) == 585, name
        plain = vc._case(vc.sphere, (9, 9, 9), (0, 0, 0), 1.0 / 8, 3, dtype=np.float16, stored=1.0 / scale)
        assert (vr.build(plain["grid"], plain["origin"], plain["spacing"], 3, scale)[1] != vc.restated(name)[1]).sum() > 100, name
    assert np.abs(vc.case("half_edges_scaled_d3")["grid"].astype(np.float64)).max() == 65504.0


def test_a_truncated_field_splits_every_node_below_its_truncation():
    # include/sdfhip.h says so: the split rule assumes a distance.  |value| <= tau = 1/16 everywhere, so fabsf(value(centre)) < 2 S
    # holds for every node of depths 0..4 (2 S >= 1/8 > tau): levels up to 5 are full
    clipped, plain = vc.restated("tsdf_d6")[0], vr.build(vc.torus(vc.lattice64((33, 33, 33), (0, 0, 0), 1 / 32)).astype(f32), (0, 0, 0), 1 / 32, 6)[0]
    sizes = vc.level_sizes(clipped)
    assert sizes[:6] == [8 ** d for d in range(6)] and (sizes[4], sizes[5]) == (4096, 32768)
    assert (len(clipped), len(plain)) == (75657, 39241)
    text = open(os.path.join(REPO, "include", "sdfhip.h")).read()
    assert "75 657 nodes against 39 241 unclipped" in text


def test_records_match_the_header(sb):
    text = open(os.path.join(REPO, "include", "sdfhip.h")).read()
    record = lambda name: re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), text, re.S).group(1)
    fields = lambda body: [re.sub(r"\[.*", "", f.strip()) for decl in re.findall(r"(?:uint32_t|int32_t|uint64_t|float)\s+([^;]+);", body)
                           for f in decl.split(",")]
    assert fields(record("sdfhip_volume")) == [f for f, _ in sb.Volume._fields_]
    assert fields(record("sdfhip_volume_stats")) == [f for f, _ in sb.VolumeStats._fields_]
    P, T = sb.Volume, sb.VolumeStats
    assert ctypes.sizeof(P) == 44 and (P.n.offset, P.origin.offset, P.spacing.offset, P.value_scale.offset, P.dtype.offset, P.depth.offset) == (4, 16, 28, 32, 36, 40)
    assert ctypes.sizeof(T) == 40 and (T.samples.offset, T.check_ms.offset, T.kernel_ms.offset, T.total_ms.offset) == (16, 24, 28, 36)
    assert (sb.VOLUME_F32, sb.VOLUME_F16) == (0, 1) and re.search(r"SDFHIP_VOLUME_F32 = 0, SDFHIP_VOLUME_F16 = 1", text)
    for name in ("sdfhip_volume_build", "sdfhip_volume_build_device", "sdfhip_scene_volume", "sdfhip_scene_volume_device"):
        assert name in sb._lib.EXPORTED_SYMBOLS
    assert hasattr(sb.Scene, "FromVolume") and hasattr(sb.Scene, "Volume")
    assert sb.lattice_of_depth(3) == ((9, 9, 9), (0, 0, 0), 0.125) and sb.lattice_of_depth(0) == ((2, 2, 2), (0, 0, 0), 1.0)


def test_the_entry_points_refuse_bad_arguments_without_a_gpu(sb):
    L = sb._lib
    grid = np.zeros((2, 2, 2), dtype=np.float32)

    def build(vol, entry="sdfhip_volume_build", data=grid, want_out=True, host=None):
        out = ctypes.c_void_p(1)
        rc = getattr(L.lib, entry)(0, data.ctypes.data if data is not None else None, ctypes.byref(vol) if vol is not None else None,
                                   ctypes.byref(out) if want_out else None, ctypes.byref(host) if host is not None else None, None)
        assert not want_out or out.value is None, "*out is not null after a failure"
        return rc, L.lib.sdfhip_last_error()

    def fill(lattice, entry="sdfhip_scene_volume", scene=None, want_out=True):
        out = np.zeros(8, dtype=np.float32)
        args = [scene, ctypes.byref(lattice) if lattice is not None else None, out.ctypes.data if want_out else None]
        rc = getattr(L.lib, entry)(*(args + [None] if entry.endswith("_device") else args))
        return rc, L.lib.sdfhip_last_error()

    good = lambda **kw: sb.Volume(**dict(dict(n=(2, 2, 2), spacing=1.0, value_scale=1.0, dtype=0, depth=3), **kw))
    lattice = lambda **kw: sb.Volume(**dict(dict(n=(2, 2, 2), spacing=1.0), **kw))
    for entry in ("sdfhip_volume_build", "sdfhip_volume_build_device"):
        what = entry[len("sdfhip_"):].encode()
        assert build(None, entry) == (L.ERR_ARG, what + b": null volume record")
        assert build(good(), entry, data=None) == (L.ERR_ARG, what + b": null grid")
        rc, msg = build(good(), entry, want_out=False)
        assert rc == L.ERR_ARG and b"both outputs" in msg
        for size in (4, 40, 45, 4100):                     # the size rules of sdfhip_placement
            vol = good()
            vol.size = size
            rc, msg = build(vol, entry)
            assert rc == L.ERR_ARG and b"bytes" in msg, size

        class Newer(ctypes.Structure):
            _fields_ = sb.Volume._fields_ + [("unknown", ctypes.c_int32)]
        newer = Newer()
        ctypes.memmove(ctypes.byref(newer), ctypes.byref(good(depth=13)), 44)
        newer.size, newer.unknown = 48, 5
        as_volume = ctypes.cast(ctypes.pointer(newer), ctypes.POINTER(sb.Volume)).contents
        rc, msg = build(as_volume, entry)
        assert rc == L.ERR_ARG and b"does not know" in msg
        newer.unknown = -1                                 # a newer struct whose new field says "default" reaches the record's own checks
        rc, msg = build(as_volume, entry)
        assert rc == L.ERR_ARG and b"depth" in msg
        for n in ((1, 2, 2), (2, 0, 2), (2, 2, 4097), (0xFFFFFFFF, 2, 2)):
            rc, msg = build(good(n=n), entry)
            assert rc == L.ERR_ARG and b"outside 2..4096" in msg, n
        rc, msg = build(good(n=(2048, 2048, 513)), entry)
        assert rc == L.ERR_ARG and b"more than 2^31" in msg
        for spacing in (0.0, -0.0, -1.0, float("nan"), float("inf")):
            rc, msg = build(good(spacing=spacing), entry)
            assert rc == L.ERR_ARG and b"spacing" in msg, spacing
        for bad in (float("nan"), float("inf"), -float("inf")):
            rc, msg = build(good(origin=(0, bad, 0)), entry)
            assert rc == L.ERR_ARG and b"origin" in msg, bad
        for scale in (0.0, -0.0, float("nan"), float("inf")):
            rc, msg = build(good(value_scale=scale), entry)
            assert rc == L.ERR_ARG and b"value_scale" in msg, scale
        for dtype in (-1, 2, 7):
            rc, msg = build(good(dtype=dtype), entry)
            assert rc == L.ERR_ARG and b"dtype" in msg, dtype
        for depth in (-1, 13, 100):
            rc, msg = build(good(depth=depth), entry)
            assert rc == L.ERR_ARG and b"depth" in msg, depth
    for entry in ("sdfhip_scene_volume", "sdfhip_scene_volume_device"):
        what = entry[len("sdfhip_"):].encode()
        assert fill(None, entry) == (L.ERR_ARG, what + b": null lattice record")
        assert fill(lattice(), entry, want_out=False) == (L.ERR_ARG, what + b": null output")
        assert fill(lattice(), entry) == (L.ERR_ARG, what + b": null scene")          # a valid lattice reaches the scene check
        assert fill(lattice(n=(1, 1, 1)), entry) == (L.ERR_ARG, what + b": null scene")
        assert fill(lattice(n=(4096, 1, 5), dtype=1), entry) == (L.ERR_ARG, what + b": null scene")
        for n in ((0, 2, 2), (2, 2, 4097)):
            rc, msg = fill(lattice(n=n), entry)
            assert rc == L.ERR_ARG and b"outside 1..4096" in msg, n
        rc, msg = fill(lattice(n=(2048, 2048, 513)), entry)
        assert rc == L.ERR_ARG and b"more than 2^31" in msg
        for bad in (lattice(value_scale=1.0), lattice(depth=3), lattice(depth=-1)):
            rc, msg = fill(bad, entry)
            assert rc == L.ERR_ARG and b"both must be 0" in msg
        for bad, word in ((lattice(spacing=0.0), b"spacing"), (lattice(spacing=float("nan")), b"spacing"), (lattice(origin=(float("inf"), 0, 0)), b"origin"),
                          (lattice(dtype=2), b"dtype")):
            rc, msg = fill(bad, entry)
            assert rc == L.ERR_ARG and word in msg, word
        small = lattice()
        small.size = 40
        rc, msg = fill(small, entry)
        assert rc == L.ERR_ARG and b"bytes" in msg


def test_a_valid_build_needs_a_gpu_and_says_so(sb):
    # the product has no CPU path: with valid arguments the call runs on the device, or there is none
    import torch
    c = vc.case("two_d3")
    if torch.cuda.is_available():
        with sb.Scene.FromVolume(c["grid"], c["origin"], c["spacing"], c["depth"]) as scene:
            assert scene.Length == vc.NODES["two_d3"]
    else:
        with pytest.raises(sb.SdfHipError) as e:
            sb.Scene.FromVolume(c["grid"], c["origin"], c["spacing"], c["depth"])
        assert e.value.code == sb._lib.ERR_DEVICE
        host = sb._lib.COctData()
        vol = sb.Volume((2, 2, 2), c["origin"], c["spacing"], 1.0, 0, 3)
        assert sb._lib.lib.sdfhip_volume_build(0, c["grid"].ctypes.data, ctypes.byref(vol), None, ctypes.byref(host), None) == sb._lib.ERR_DEVICE
        assert host.length == 0 and not host.structs


def test_the_python_wrappers_refuse_before_the_library_is_called(sb, monkeypatch):
    called = []
    for name in ("sdfhip_volume_build", "sdfhip_volume_build_device", "sdfhip_scene_volume", "sdfhip_scene_volume_device"):
        monkeypatch.setattr(sb.renderer.lib, name, lambda *a, _n=name: called.append(_n) or sb._lib.ERR_DEVICE, raising=False)
    ok = np.zeros((3, 3, 3), dtype=np.float32)
    for bad in ([[[0.0, 1.0], [0.0, 1.0]], [[0.0, 1.0], [0.0, 1.0]]], ok.astype(np.float64), ok.astype(np.int32), None, "grid"):
        with pytest.raises(TypeError):
            sb.Scene.FromVolume(bad, depth=2)
    for bad in (ok[:, :, ::2], ok[0], np.zeros((3, 3, 1), dtype=np.float32), ok.transpose(2, 1, 0)):
        with pytest.raises(ValueError):
            sb.Scene.FromVolume(bad, depth=2)
    for kw in (dict(depth=13), dict(depth=-1), dict(spacing=0.0), dict(spacing=float("nan")), dict(origin=(0, 0))):
        with pytest.raises(ValueError):
            sb.Scene.FromVolume(ok, **dict(dict(depth=2), **kw))
    import torch
    with pytest.raises(TypeError):
        sb.Scene.FromVolume(torch.zeros((3, 3, 3)), depth=2)          # a host tensor
    scene = sb.Scene.__new__(sb.Scene)
    scene._h, scene.device = ctypes.c_void_p(), 0
    for shape in ((3, 3), (0, 3, 3), (3, 3, 4097), (2048, 2048, 513)):
        with pytest.raises(ValueError):
            scene.Volume(shape)
    with pytest.raises(ValueError):
        scene.Volume((3, 3, 1))                                      # one sample along x: no spacing to derive
    with pytest.raises(ValueError):
        scene.Volume((3, 3, 3), spacing=-1.0)
    with pytest.raises(TypeError):
        scene.Volume((3, 3, 3), dtype=np.float64)
    with pytest.raises(TypeError):
        scene.Volume((3, 3, 3), out=np.zeros((3, 3, 3), dtype=np.float32))
    with pytest.raises(TypeError):
        scene.Volume((3, 3, 3), out=torch.zeros((3, 3, 3)))
    assert not called
    # the default depth: the first level whose cells are no larger than the spacing
    with pytest.raises(sb.SdfHipError):
        sb.Scene.FromVolume(ok)
    assert called == ["sdfhip_volume_build"]
