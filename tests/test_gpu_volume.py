"""Volumes in and out on the GPU (sdfhip_volume_build[_device], sdfhip_scene_volume[_device]), both flavours of the library: the
built tree is the CPU restatement's (tests/volume_restatement.py) byte for byte -- every grid of tests/volume_cases.py, through the
host entry and from a torch tensor -- its statistics are the restatement's counts; a scene read on a lattice is what the sampler
answers at the same points, bit for bit, with every cursor form; the two directions compose into the placement's identity; the
result renders, prunes, combines and measures as any other scene; and the errors are status codes.  The second round (the cases of
volume_cases.py from corner_d12 on): depth 12 in the far corner, grids on the negative side and of the other sign, the edges of
float16 in both directions, and more samples than k_volume_check strides with.  Zoo trees as sources, and the lattice past
k_volume_out's stride: tests/test_gpu_zoo_volumes.py."""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import combine_restatement as cr
import edit_restatement as er
import prune_restatement as pr
import volume_cases as vc
import volume_restatement as vr
from conftest import REPO, assert_frames_identical, make_camera
from test_gpu_combine import tree
from test_gpu_prune import assert_same_tree

pytestmark = pytest.mark.gpu

DEVICE_ENTRY = ("sphere17_d4", "aniso_inset_d5", "torus33_f16_d6", "corner_d12", "corner_d12_f16", "negative_scale_d4",
                "half_edges_scaled_d3")                                   # also built from a torch tensor
OUT_SOURCES = ["leaf", "nine", "sphere_d4", "torus_edited", "off_d7"]
# (shape (nz, ny, nx), origin, spacing): a 5 x 1 x 7 lattice that sticks out of the cube on every side, and one element
STICKS_OUT, ONE = vc.STICKS_OUT, vc.ONE


@pytest.fixture(scope="module", params=["product", "lab"])
def sb(request):
    import sdfbox_amd
    if request.param == "product":
        return sdfbox_amd
    import sdfbox_amd.lab
    return sdfbox_amd.lab.load()


def build(sb, name, grid=None, **kw):
    c = vc.case(name)
    return sb.Scene.FromVolume(c["grid"] if grid is None else grid, c["origin"], c["spacing"], c["depth"], c["value_scale"], **kw)


def check_build(sb, name, grid=None):
    S, V, counts = vc.restated(name)
    res, got, st = build(sb, name, grid, want_octdata=True, want_stats=True)
    with res:
        what = f"volume {name}" + ("" if grid is None else " from a device tensor")
        assert_same_tree(got, S, V, what)
        assert (st.nodes_out, st.depth_out, st.levels, st.samples) == (len(S), counts["depth_out"], counts["levels"], counts["samples"]), what
        assert st.depth_out == er.tree_depth(S) and st.check_ms >= 0 and st.kernel_ms > 0, what
        assert res.Length == len(S) and res.depth == st.depth_out and res.stack_kernel_ok, what


@pytest.mark.parametrize("name", vc.NAMES)
def test_built_bytes_are_the_restatements(sb, name):
    import torch
    assert len(vc.restated(name)[0]) == vc.NODES[name]
    check_build(sb, name)
    if name in DEVICE_ENTRY:
        host = vc.case(name)["grid"]
        t = torch.from_numpy(host.copy()).cuda()
        check_build(sb, name, t)
        assert np.array_equal(t.cpu().numpy().view(np.uint8), host.view(np.uint8)), "the input tensor after the build"


def upload(sb, name, **kw):
    return sb.Scene(sb.OctData(*tree(name)), **kw)


_outs = {}


def restated_out(src, lattice, dtype=np.float32):
    key = (src, lattice, np.dtype(dtype).name)
    if key not in _outs:
        _outs[key] = vr.volume_out(tree(src), *lattice, dtype=dtype)
    return _outs[key]


def check_out(sb, scene, src):
    import torch
    bits = lambda a: a.view(np.uint32 if a.dtype == np.float32 else np.uint16)
    for lattice in (sb.lattice_of_depth(3), STICKS_OUT, ONE):
        shape, origin, spacing = lattice
        got = scene.Volume(*lattice)
        assert got.shape == tuple(shape) and got.dtype == np.float32
        # the sampler at the same float32 coordinates: where the point lies in the cube the element IS the sample
        p = vr.lattice_points(shape, origin, spacing)
        inside = ((p >= 0) & (p <= 1)).all(1)
        sampled = scene.Sample(p)["distance"]
        assert np.array_equal(bits(got.reshape(-1)[inside]), bits(sampled[inside])), (src, lattice)
        # ... and everywhere, out of the cube included, the restatement's; the float16 form is its rounding
        want = restated_out(src, lattice)
        assert np.array_equal(bits(got), bits(want)), (src, lattice)
        half = scene.Volume(*lattice, dtype=np.float16)
        assert half.dtype == np.float16 and np.array_equal(bits(half), bits(restated_out(src, lattice, np.float16))), (src, lattice)
        # the device form, on the current torch stream
        for dtype, host in ((torch.float32, got), (torch.float16, half)):
            out = torch.full(tuple(shape), 7.0, dtype=dtype, device="cuda")
            assert scene.Volume(shape, origin, spacing, out=out) is out
            torch.cuda.current_stream().synchronize()
            assert np.array_equal(bits(out.cpu().numpy()), bits(host)), (src, lattice, dtype)


@pytest.mark.parametrize("src", OUT_SOURCES)
def test_a_scene_on_a_lattice_is_what_the_sampler_answers(sb, src):
    lattices = (sb.lattice_of_depth(3), STICKS_OUT, ONE)
    p = vr.lattice_points(*STICKS_OUT)
    outside = ~((p >= 0) & (p <= 1)).all(1)
    assert outside.any() and not outside.all() and lattices[0][0] == (9, 9, 9)
    with upload(sb, src) as scene:
        check_out(sb, scene, src)
    # the walk along the links gives the same elements as the grids
    with upload(sb, src, top_grid_level=0) as scene:
        assert scene.top_grid_level == 0
        check_out(sb, scene, src)


@pytest.mark.parametrize("src, D", [("sphere_d4", 4), ("torus_d6", 5), ("torus_d6", 6)])
def test_out_then_in_is_the_placement_at_the_identity(sb, src, D):
    # independent of the restatement: every point a build to depth D evaluates is a vertex of lattice_of_depth(D), vertices are
    # exact, and an element of Volume is the placement's value at the identity
    import torch
    with upload(sb, src) as scene:
        placed, want = scene.Place(np.eye(3, dtype=np.float32), 1.0, (0, 0, 0), D, want_octdata=True)
        placed.close()
        lattice = sb.lattice_of_depth(D)
        res, got = sb.Scene.FromVolume(scene.Volume(*lattice), lattice[1], lattice[2], depth=D, want_octdata=True)
        with res:
            assert_same_tree(got, want.Structs, want.Values, f"FromVolume(Volume({src})) to depth {D}")
        # ... and without the field leaving the device
        out = torch.empty(lattice[0], dtype=torch.float32, device="cuda")
        res, got = sb.Scene.FromVolume(scene.Volume(*lattice, out=out), lattice[1], lattice[2], depth=D, want_octdata=True)
        with res:
            assert_same_tree(got, want.Structs, want.Values, f"FromVolume(Volume({src})) on the device to depth {D}")
    assert want.Length > 1000


def test_the_result_renders_and_chains(sb, oracle_mod):
    W, H = 64, 64
    S, V, _ = vc.restated("sphere17_d4")
    cam = make_camera("rotated", W, H)
    od = sb.sphere_d4()
    with build(sb, "sphere17_d4") as scene, sb.Scene(od) as analytic, sb.Scene(sb.OctData(S, V)) as same_arrays:
        ref, _ = oracle_mod.render(S, V, cam.State, W, H)
        for flags in (sb.KERNEL_AUTO, sb.KERNEL_GENERIC):
            assert_frames_identical(scene.Draw(cam, W, H, flags), ref, f"a scene from a volume, flags {flags}")
        # the measure: the same arrays measure the same, bit for bit; the analytic builder's tree has the same cells in another
        # order, which include/sdfhip.h says agrees to rounding, 1e-12 relative
        m, m_same, m_analytic = scene.Measure(), same_arrays.Measure(), analytic.Measure()
        assert (m.volume, m.area, tuple(m.moment1), tuple(m.moment2)) == (m_same.volume, m_same.area, tuple(m_same.moment1), tuple(m_same.moment2))
        assert (m.cells, m.cells_cut, m.cells_inside, m.nodes) == (m_analytic.cells, m_analytic.cells_cut, m_analytic.cells_inside, m_analytic.nodes)
        assert m.volume > 0.1 and abs(m.volume - m_analytic.volume) <= 1e-12 * m_analytic.volume
        assert abs(m.area - m_analytic.area) <= 1e-12 * m_analytic.area
        # after a tolerance-0 prune of both the cells are still the same
        with scene.Prune(0) as a, analytic.Prune(0) as b:
            ma, mb = a.Measure(), b.Measure()
            assert a.Length == b.Length and (ma.cells, ma.cells_cut) == (mb.cells, mb.cells_cut)
            assert abs(ma.volume - mb.volume) <= 1e-12 * mb.volume
        # prune and combine take it, and give what the restatements give from the restated arrays
        res, got = scene.Prune(2, None, want_octdata=True)
        with res:
            assert_same_tree(got, *pr.prune(S, V, 2), "prune of a scene from a volume")
        with upload(sb, "off_d7") as other:
            res, got = scene.Combine(other, cr.COMBINE_UNION, want_octdata=True)
            with res:
                assert_same_tree(got, *cr.combine((S, V), tree("off_d7"), cr.COMBINE_UNION), "combine of a scene from a volume")


def test_volume_leaves_the_source_as_it_was(sb):
    W, H = 64, 48
    cam = make_camera("rotated", W, H)
    with upload(sb, "torus_edited") as scene:
        before = scene.Draw(cam, W, H)
        first = scene.Volume(*sb.lattice_of_depth(4))
        assert_frames_identical(scene.Draw(cam, W, H), before, "the source after Volume")
        assert np.array_equal(first.view(np.uint32), scene.Volume(*sb.lattice_of_depth(4)).view(np.uint32))


def test_non_finite_samples_and_bad_arguments_are_status_codes(sb):
    import torch
    L = sb._lib
    c = vc.case("sphere17_d4")
    for bad, count in ((np.nan, 1), (np.inf, 1), (-np.inf, 3)):
        for dtype in (np.float32, np.float16):
            grid = c["grid"].astype(dtype)
            grid.reshape(-1)[[5, 2000, 4912][:count]] = bad
            for g in (grid, torch.from_numpy(grid).cuda()):
                with pytest.raises(sb.SdfHipError) as e:
                    sb.Scene.FromVolume(g, c["origin"], c["spacing"], c["depth"])
                assert e.value.code == L.ERR_ARG and f"{count} of the grid's 4913 samples are not finite" in str(e.value), (bad, dtype)
    # the library works afterwards, and host_out alone is an output
    raw = L.COctData()
    vol = sb.Volume((17, 17, 17), c["origin"], c["spacing"], 1.0, L.VOLUME_F32, 4)
    assert L.lib.sdfhip_volume_build(0, c["grid"].ctypes.data, ctypes.byref(vol), None, ctypes.byref(raw), None) == L.OK
    assert raw.length == vc.NODES["sphere17_d4"]
    L.lib.sdfhip_octdata_free(ctypes.byref(raw))
    h = ctypes.c_void_p()
    assert L.lib.sdfhip_volume_build(64, c["grid"].ctypes.data, ctypes.byref(vol), ctypes.byref(h), None, None) == L.ERR_DEVICE and not h.value
    with build(sb, "sphere17_d4") as scene:
        out = np.zeros(8, dtype=np.float32)
        assert L.lib.sdfhip_scene_volume(scene._h, ctypes.byref(sb.Volume((2, 2, 2), (0, 0, 0), 1.0, 0.0, 0, 3)), out.ctypes.data) == L.ERR_ARG
        assert L.lib.sdfhip_scene_volume(scene._h, ctypes.byref(sb.Volume((2, 2, 2), (0, 0, 0), 1.0)), out.ctypes.data) == L.OK
        assert np.array_equal(out.reshape(2, 2, 2), scene.Volume((2, 2, 2)))


def test_non_finite_samples_past_the_first_stride_are_counted(sb):
    # 81^3 = 531 441 samples against the 524 288 threads k_volume_check strides with: the last 7 153 are a thread's second trip.  One
    # bad sample alone at the first and the last index of either trip; then every 97th sample, NaN and both infinities in turn -- a
    # count that every lane, wave and workgroup contributes to.  The message's count is exactly what was planted
    import torch
    c = vc.case("sphere81_d4")
    total, stride = c["grid"].size, 2048 * 256
    assert total == 531441 > stride
    every = np.arange(0, total, 97)
    assert len(every) == 5479 and every[-1] > stride
    plantings = [(np.array([i]), [np.nan]) for i in (0, stride - 1, stride, total - 1)] + [(every, [np.nan, np.inf, -np.inf])]
    for dtype in (np.float32, np.float16):
        clean = c["grid"].astype(dtype)
        for at, bad in plantings:
            grid = clean.copy()
            grid.reshape(-1)[at] = np.resize(np.array(bad, dtype=dtype), len(at))
            assert int((~np.isfinite(grid)).sum()) == len(at)
            for g in (grid, torch.from_numpy(grid).cuda()):
                with pytest.raises(sb.SdfHipError) as e:
                    sb.Scene.FromVolume(g, c["origin"], c["spacing"], c["depth"])
                assert e.value.code == sb._lib.ERR_ARG, (dtype, at[:3])
                assert f" {len(at)} of the grid's {total} samples are not finite" in str(e.value), (dtype, at[:3], str(e.value))
    # the clean grid builds afterwards to the restatement's tree, from the host and from the device
    check_build(sb, "sphere81_d4")
    check_build(sb, "sphere81_d4", torch.from_numpy(c["grid"].copy()).cuda())


def test_half_precision_out_beyond_its_precision_and_below_its_normals(sb):
    # far outside the cube: elements 0.013 apart at distance 300, where a half's ulp is 0.25 -- neighbours differ in float32 and round
    # to the same half, some of them across a tie's neighbourhood; nothing overflows (the header leaves an overflow undefined)
    far = ((2, 3, 40), (-300.0, 0.3, 0.4), 0.013)
    bits = lambda a: a.view(np.uint32 if a.dtype == np.float32 else np.uint16)
    with upload(sb, "torus_edited") as scene:
        want = restated_out("torus_edited", far)
        half = restated_out("torus_edited", far, np.float16)
        assert np.abs(want).max() < 65504 and np.isfinite(half).all()
        assert len(np.unique(bits(want))) > 4 * len(np.unique(bits(half))) > 4
        assert np.array_equal(bits(scene.Volume(*far)), bits(want))
        assert np.array_equal(bits(scene.Volume(*far, dtype=np.float16)), bits(half))
    # near the surface of the depth-12 sphere after a prune that removes nothing it should not: distances of a few 2^-12 / 255, which
    # round to subnormal halves (below 2^-14)
    S, V, _ = vc.restated("corner_d12")
    PS, PV = pr.prune(S, V, 0)
    centre, r = np.array(vc.CORNER_D12[:3]), vc.CORNER_D12[3]
    near = ((9, 9, 9), tuple(float(x) for x in np.floor((centre + r / np.sqrt(3.0)) * 4096) / 4096 - 4 * 2.0 ** -12), 2.0 ** -12)
    want = vr.volume_out((PS, PV), *near, dtype=np.float16)
    subnormal = (bits(want) & 0x7C00 == 0) & (bits(want) & 0x03FF != 0)
    assert subnormal.sum() > 20 and (want[subnormal] < 0).any() and (want[subnormal] > 0).any()
    with build(sb, "corner_d12") as scene, scene.Prune(0) as pruned:
        assert pruned.Length == len(PS) <= len(S)
        assert np.array_equal(bits(pruned.Volume(*near, dtype=np.float16)), bits(want))
        assert np.array_equal(bits(pruned.Volume(*near)), bits(vr.volume_out((PS, PV), *near)))


def test_an_allocation_that_fails_is_nomem_and_leaves_the_library_working():
    # in a fresh process of its own, so that neither the variable nor a failed call can reach the tests beside this one: every
    # allocation the build reaches fails once (k = 0, 1, ... until a call gets through), each is SDFHIP_ERR_NOMEM with no handle; the
    # out direction's one allocation likewise; afterwards a plain build gives the restatement's tree (tests/volume_fault_child.py).
    # The variable refuses an allocation on the host side: no device fault is involved.
    S, V, _ = vc.restated("tsdf_d6")
    child = os.path.join(REPO, "tests", "volume_fault_child.py")
    out = subprocess.run([sys.executable, child], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, (out.returncode, out.stdout[-2000:], out.stderr[-2000:])
    report = json.loads(out.stdout.strip().splitlines()[-1])
    # the staged grid, the counter, the two arrays, the blocks, the bitmap, its two scan buffers and the next level's blocks are
    # nine; this result outgrows the arrays' start, so the two larger arrays are among them as well
    assert report["codes_ok"] and 11 <= report["failed"] < 64, report
    assert report["out_is_nomem"] and report["out_works_afterwards"], report
    assert report["nodes_after"] == len(S) and report["structs_sha"] == sha(S) and report["values_sha"] == sha(V), report
    assert report["product_reads_no_variable"], report


def sha(a):
    import hashlib
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()
