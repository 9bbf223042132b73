"""Cross-sections on the GPU (sdfhip_scene_slice / sdfhip_scene_slice_device), both flavours of the library: every word of every
record, the per-layer counts and the statistics are the numpy restatement's (tests/slice_restatement.py, which tests every triangle of
the mesh restatement against every layer and is held to things it did not make by tests/test_slice.py) -- on the golden trees, a carved
tree with cells of mixed depth and the zoo's trees round the 1024-node workgroup, for an axis stack, a stack on cell faces, an oblique
stack, 257 layers that ALL lie on cell faces (the reject margin's worst case), 4096 layers over the 12-deep chain and 65 536 over one cell, and on a
1.4 M-node tree with more chunks than the chunk scan has threads; the
_device form counts, fills, refuses a short buffer, writes the layer counts either way and leaves frames in flight alone; the errors
are status codes; the records are the slice of Scene.Mesh's own triangles."""
import ctypes

import numpy as np
import pytest

import big_cell_tree
import edit_restatement as er
import mesh_restatement as mr
import slice_restatement as sr
import tree_zoo
from conftest import assert_frames_identical, make_camera

pytestmark = pytest.mark.gpu
f32 = np.float32

# (normal, offset, pitch, layers)
AXIS = ((0.0, 0.0, 1.0), 0.21, 0.0625, 10)
FACES = ((0.0, 1.0, 0.0), 0.25, 0.03125, 17)              # every plane on a face of the depth-5 cells
OBLIQUE = ((0.6, 0.0, 0.8), 0.3, 0.05, 12)
FACES_257 = ((1.0, 0.0, 0.0), 0.0, 2.0 ** -8, 257)        # every plane on a cell face of every depth up to 8, the cube's two faces included
FINE_4096 = ((0.0, 0.0, 1.0), 0.0, 2.0 ** -12, 4096)      # past the LDS histogram's 1024 layers: the counts go straight to global memory
PLANES = {"axis": AXIS, "faces": FACES, "oblique": OBLIQUE, "faces_257": FACES_257, "fine_4096": FINE_4096}
FOUR = ("axis", "faces", "oblique", "faces_257")


@pytest.fixture(scope="module", params=["product", "lab"])
def sb(request):
    import sdfbox_amd
    if request.param == "product":
        return sdfbox_amd
    import sdfbox_amd.lab
    return sdfbox_amd.lab.load()


_trees, _want = {}, {}


def tree(name):
    """host arrays of the test scenes (the same for both flavours)"""
    if name not in _trees:
        import sdfbox_amd as base
        if name == "sphere_d4":
            _trees[name] = base.sphere_d4()
        elif name == "torus_d6":
            _trees[name] = base.torus_d6()
        elif name == "carved_d7":
            # a carve through the torus' surface that refines one level deeper: cells of depth 6 and 7 side by side
            with base.Scene(base.torus_d6()) as scene:
                res, out = scene.Edit([(er.EDIT_CARVE, er.BRUSH_SPHERE, (0.75, 0.5, 0.5, 0.07))], max_depth=7, want_octdata=True)
                res.close()
            _trees[name] = out
        else:
            _trees[name] = base.OctData(*tree_zoo.zoo()[name])
    return _trees[name]


def want(key, make):
    """the restatement's answer, computed once for both flavours"""
    if key not in _want:
        _want[key] = make()
    return _want[key]


def meshed(name, level):
    od = tree(name)
    walked = want(("walk", name), lambda: mr.walk(od.Structs))
    return want(("mesh", name, level), lambda: mr.mesh(od.Structs, od.Values, level, want_cells=True, walked=walked))


def restated(name, level, plane):
    od = tree(name)
    return want(("slice", name, level, plane), lambda: sr.slice_scene(od.Structs, od.Values, *PLANES[plane], level, meshed=meshed(name, level)))


def assert_records(got, ref, what):
    assert got.dtype == sr.SEGMENT and got.shape == ref.shape, (what, got.shape, ref.shape)
    a, b = got.view(np.uint32).reshape(-1, 8), ref.view(np.uint32).reshape(-1, 8)
    if not (a == b).all():
        w = np.nonzero((a != b).any(1))[0]
        raise AssertionError(f"{what}: {len(w)} of {len(a)} records differ; first: record {int(w[0])} {got[w[0]]} against {ref[w[0]]}")


CASES = [("sphere_d4", (-1, 0, 3, 12), FOUR), ("torus_d6", (-1, 3, 9), FOUR), ("carved_d7", (-1, 6), FOUR),
         ("leaf", (-1, 0), FOUR), ("chain12", (-1, 6), FOUR + ("fine_4096",)), ("blocks_1017", (-1, 3), FOUR), ("blocks_1025", (-1, 3), FOUR),
         ("blocks_4097", (-1, 3), FOUR), ("dfs_d6_a", (-1, 3), FOUR)]


@pytest.mark.parametrize("name, levels, planes", CASES, ids=[c[0] for c in CASES])
def test_slice_is_the_restatements(sb, name, levels, planes):
    od = tree(name)
    total = 0
    with sb.Scene(od) as scene:
        assert scene.stack_kernel_ok
        for level in levels:
            for plane in planes:
                normal, offset, pitch, layers = PLANES[plane]
                rec, counts, (cells, cut, crossed) = restated(name, level, plane)
                ref, ref_starts = sr.by_layer(rec, layers)
                got, starts, st = scene.Slice(normal, offset, pitch, layers, level)
                what = (name, level, plane)
                assert (st.nodes, st.cells, st.cells_cut, st.cells_crossed, st.n_segments) == (od.Length, cells, cut, crossed, len(rec)), what
                assert st.total_ms >= st.kernel_ms > 0
                assert starts.tolist() == ref_starts.tolist() and np.diff(starts).tolist() == counts.tolist(), what
                assert_records(got, ref, what)
                assert scene.SliceDevice(normal=normal, offset=offset, pitch=pitch, layers=layers, level=level) == len(rec), what
                total += len(rec)
        got, starts = scene.Slice(*PLANES[planes[0]], levels[0], want_stats=False)              # no statistics: the other count kernel
        assert_records(got, sr.by_layer(restated(name, levels[0], planes[0])[0], PLANES[planes[0]][3])[0], (name, "no statistics"))
    assert total > 0


def test_more_chunks_than_the_scan_has_threads(sb):
    """each of the 1024 threads of the chunk scan (scan_device.h, the mesh's too) owns more than one chunk's total; the tree and its
    restated triangles are big_cell_tree.py's, made once for both modules"""
    od, triple = big_cell_tree.tree(), big_cell_tree.meshed()
    assert len(od.Structs) > 1024 * 1024
    plane = ((0.0, 0.0, 1.0), 0.1, 0.1, 9)
    rec, counts, (cells, cut, crossed) = want(("slice", "big"), lambda: sr.slice_scene(od.Structs, od.Values, *plane, -1, meshed=triple))
    assert (len(rec), crossed) == (9376, 2570)
    ref, ref_starts = sr.by_layer(rec, plane[3])
    with sb.Scene(od) as scene:
        got, starts, st = scene.Slice(*plane, -1)
        assert (st.nodes, st.cells, st.cells_cut, st.cells_crossed, st.n_segments) == (od.Length, cells, cut, crossed, len(rec))
        assert starts.tolist() == ref_starts.tolist() and np.diff(starts).tolist() == counts.tolist()
        assert_records(got, ref, "more chunks than scan threads")
        assert scene.SliceDevice(normal=plane[0], offset=plane[1], pitch=plane[2], layers=plane[3], level=-1) == len(rec)


def test_the_most_layers_there_may_be(sb):
    # 65 536 planes 2^-16 apart through the one-node tree: most layers of the stack hold a record of every triangle
    od = tree("leaf")
    plane = ((0.0, 0.0, 1.0), 0.0, 2.0 ** -16, 65536)
    rec, counts, (cells, cut, crossed) = want(("slice", "leaf", -1, "65536"), lambda: sr.slice_scene(od.Structs, od.Values, *plane, -1, meshed=meshed("leaf", -1)))
    assert (cells, cut, crossed) == (1, 1, 1) and len(rec) > 65536 and (counts == 0).any()
    with sb.Scene(od) as scene:
        got, starts, st = scene.Slice(*plane)
        assert st.n_segments == len(rec) and np.diff(starts).tolist() == counts.tolist()
        assert_records(got, sr.by_layer(rec, 65536)[0], "65 536 layers")


@pytest.mark.parametrize("name", ["torus_d6", "carved_d7"])
def test_the_device_form_counts_fills_and_refuses_a_short_buffer_beside_frames_in_flight(sb, name):
    import torch
    od = tree(name)
    W = H = 256
    cam = make_camera("rotated", W, H)
    normal, offset, pitch, layers = OBLIQUE
    kw = dict(normal=normal, offset=offset, pitch=pitch, layers=layers)
    host, counts, _ = restated(name, -1, "oblique")                # node-major, as the device form writes
    low, low_counts, _ = restated(name, 4, "oblique")
    n = len(host)
    assert n > 1000 and len(low) > 100
    with sb.Scene(od) as scene:
        alone = scene.Draw(cam, W, H)
        assert scene.SliceDevice(**kw) == n                        # capacity 0 and a null pointer: the count
        buf = torch.full((n + 1, 8), -7.0, dtype=torch.float32, device="cuda")
        cnt = torch.full((layers + 1,), 77, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        assert scene.SliceDevice(buf.data_ptr(), n, cnt.data_ptr(), **kw) == n
        torch.cuda.synchronize()
        assert buf[:n].cpu().numpy().tobytes() == host.tobytes(), name
        assert (buf[n].cpu().numpy() == -7.0).all()                # nothing past the last record
        assert cnt.cpu().numpy().tolist() == counts.tolist() + [77]
        # one short: the count comes back, no record is written, the layer counts are
        buf.fill_(-7.0); cnt.fill_(77)
        torch.cuda.synchronize()
        assert scene.SliceDevice(buf.data_ptr(), n - 1, cnt.data_ptr(), **kw) == n
        torch.cuda.synchronize()
        assert (buf.cpu().numpy() == -7.0).all()
        assert cnt.cpu().numpy().tolist() == counts.tolist() + [77]
        # the counts alone
        cnt.fill_(77)
        torch.cuda.synchronize()
        assert scene.SliceDevice(counts_ptr=cnt.data_ptr(), **kw) == n
        torch.cuda.synchronize()
        assert cnt.cpu().numpy().tolist() == counts.tolist() + [77]
        # beside frames in flight on another stream, at two levels
        frames = [torch.zeros((H, W, 4), dtype=torch.float32, device="cuda") for _ in range(8)]
        d_low = torch.zeros((len(low) + 1, 8), dtype=torch.float32, device="cuda")
        c_low = torch.zeros((layers,), dtype=torch.int32, device="cuda")
        buf.fill_(0.0)
        torch.cuda.synchronize()
        s_frames, s_slice = torch.cuda.Stream(), torch.cuda.Stream()
        for k, b in enumerate(frames):
            scene.DrawDevice(cam, W, H, b.data_ptr(), stream=s_frames.cuda_stream)
            if k % 2 == 0:
                assert scene.SliceDevice(buf.data_ptr(), n, cnt.data_ptr(), stream=s_slice.cuda_stream, **kw) == n
            else:
                assert scene.SliceDevice(d_low.data_ptr(), len(low), c_low.data_ptr(), level=4, stream=s_slice.cuda_stream, **kw) == len(low)
        torch.cuda.synchronize()
        assert buf[:n].cpu().numpy().tobytes() == host.tobytes(), name
        assert d_low[:len(low)].cpu().numpy().tobytes() == low.tobytes(), name
        assert cnt.cpu().numpy().tolist() == counts.tolist() + [77] and c_low.cpu().numpy().tolist() == low_counts.tolist()
        for k, b in enumerate(frames):
            assert_frames_identical(b.cpu().numpy(), alone, f"{name}: frame {k} beside the slice")


def test_errors_are_status_codes(sb):
    L = sb._lib
    od = tree("torus_d6")
    inf, nan = float("inf"), float("nan")
    bad = [dict(level=-2), dict(level=13), dict(level=1 << 20),
           dict(normal=(0.0, 0.0, 0.0)), dict(normal=(-0.0, 0.0, 0.0)), dict(normal=(nan, 0.0, 1.0)), dict(normal=(0.0, inf, 1.0)), dict(normal=(0.0, 1.0, -inf)),
           dict(offset=nan), dict(offset=inf),
           dict(layers=0), dict(layers=65537, pitch=0.001), dict(layers=0xFFFFFFFF, pitch=0.001),
           dict(pitch=nan), dict(pitch=inf), dict(pitch=-inf), dict(layers=2, pitch=0.0), dict(layers=2, pitch=-0.01), dict(layers=2, pitch=nan)]
    out, n = L.CSlice(), ctypes.c_uint32(7)
    with sb.Scene(od) as scene:
        h = scene._h
        for kw in bad:
            opt = L.SliceOptions(**kw)
            out.n_segments = 5; n.value = 7
            assert L.lib.sdfhip_scene_slice(h, ctypes.byref(opt), ctypes.byref(out), None) == L.ERR_ARG, kw
            assert out.n_segments == 0 and not out.segments and not out.layer_counts
            assert L.lib.sdfhip_scene_slice_device(h, ctypes.byref(opt), None, 0, None, ctypes.byref(n), None) == L.ERR_ARG, kw
            assert n.value == 0 and L.lib.sdfhip_last_error()
        assert L.lib.sdfhip_scene_slice(h, None, None, None) == L.ERR_ARG
        assert L.lib.sdfhip_scene_slice_device(h, None, None, 0, None, None, None) == L.ERR_ARG
        assert L.lib.sdfhip_scene_slice_device(h, None, None, 5, None, ctypes.byref(n), None) == L.ERR_ARG      # a capacity and no buffer
        # the options struct's size rules: too small, not a multiple of four; a larger one with unknown fields all -1 is accepted
        for size in (0, 28, 34):
            opt = L.SliceOptions(); opt.size = size
            assert L.lib.sdfhip_scene_slice_device(h, ctypes.byref(opt), None, 0, None, ctypes.byref(n), None) == L.ERR_ARG, size
        big = (ctypes.c_int32 * 10)()
        ctypes.memmove(big, ctypes.byref(L.SliceOptions(*OBLIQUE, 3)), 32)
        big[0], big[8], big[9] = 40, -1, -1
        assert L.lib.sdfhip_scene_slice_device(h, ctypes.cast(big, ctypes.POINTER(L.SliceOptions)), None, 0, None, ctypes.byref(n), None) == L.OK
        assert n.value == len(restated("torus_d6", 3, "oblique")[0])
        big[9] = 0
        assert L.lib.sdfhip_scene_slice_device(h, ctypes.cast(big, ctypes.POINTER(L.SliceOptions)), None, 0, None, ctypes.byref(n), None) == L.ERR_ARG
        # NULL options = the defaults: one plane z = 0.5; and layers = 1 ignores the pitch
        default = sr.slice_scene(od.Structs, od.Values, meshed=meshed("torus_d6", -1))[0]
        assert L.lib.sdfhip_scene_slice_device(h, None, None, 0, None, ctypes.byref(n), None) == L.OK and n.value == len(default) > 0
        got, starts = scene.Slice(pitch=123.0, want_stats=False)
        assert_records(got, default, "one layer, a pitch given")
        assert starts.tolist() == [0, len(default)]
    # a child whose parent field points elsewhere: the tree uploads, the walk up the links cannot be trusted
    S = od.Structs.copy()
    S[int(S[0, 1]) + 3, 0] = int(S[0, 1])
    with sb.Scene(sb.OctData(S, od.Values)) as scene:
        assert not scene.stack_kernel_ok
        out.n_segments = 5
        assert L.lib.sdfhip_scene_slice(scene._h, None, ctypes.byref(out), None) == L.ERR_BAD_TREE
        assert L.lib.sdfhip_scene_slice_device(scene._h, None, None, 0, None, ctypes.byref(n), None) == L.ERR_BAD_TREE
        assert out.n_segments == 0 and not out.segments and not out.layer_counts and n.value == 0


def test_a_scene_with_no_surface_and_layers_outside_the_cube_give_zero_records(sb):
    od = sb.OctData.Generate(sb._lib.SHAPE_SPHERE, [3.0, 3.0, 3.0, 0.3], 4)          # the ball lies outside the cube
    assert mr.count(od.Structs, od.Values, -1)[2] == 0
    with sb.Scene(od) as scene:
        segs, starts, st = scene.Slice(*AXIS)
        assert segs.shape == (0,) and segs.dtype == sr.SEGMENT and starts.tolist() == [0] * 11
        assert (st.n_segments, st.cells_cut, st.cells_crossed) == (0, 0, 0) and st.nodes == od.Length
        assert scene.SliceDevice() == 0
    with sb.Scene(tree("sphere_d4")) as scene:
        for offset, pitch in ((1.5, 0.25), (-3.0, 0.25)):
            segs, starts, st = scene.Slice((0.0, 0.0, 1.0), offset, pitch, 8)
            assert len(segs) == 0 and starts.tolist() == [0] * 9 and (st.cells_cut, st.cells_crossed) == (416, 0)


def test_a_failed_allocation_is_nomem_and_leaves_the_scene_alone(sb, monkeypatch):
    od = tree("sphere_d4")
    ref = sr.by_layer(restated("sphere_d4", -1, "axis")[0], AXIS[3])[0]
    with sb.Scene(od) as scene:
        if not sb._lib.EXPERIMENTS:
            monkeypatch.setenv("SDFHIP_SLICE_FAIL_ALLOC", "0")        # the product reads no such variable
            assert_records(scene.Slice(*AXIS, want_stats=False)[0], ref, "the product ignores the laboratory's knob")
            return
        for k in (0, 1, 2, 3):                                  # the chunk totals, the host counts, the device records, the host records
            monkeypatch.setenv("SDFHIP_SLICE_FAIL_ALLOC", str(k))
            with pytest.raises(sb.SdfHipError) as e:
                scene.Slice(*AXIS)
            assert e.value.code == sb._lib.ERR_NOMEM, k
        monkeypatch.setenv("SDFHIP_SLICE_FAIL_ALLOC", "4")         # the call allocates four times
        assert_records(scene.Slice(*AXIS, want_stats=False)[0], ref, "no fifth allocation")
        monkeypatch.delenv("SDFHIP_SLICE_FAIL_ALLOC")
        assert_records(scene.Slice(*AXIS, want_stats=False)[0], ref, "after the failed calls")


def test_the_slice_is_the_slice_of_the_scenes_own_mesh(sb):
    od = tree("torus_d6")
    cut_cells = np.unique(meshed("torus_d6", -1)[1])
    with sb.Scene(od) as scene:
        tris = scene.Mesh(want_stats=False)
        for plane in ("axis", "oblique", "faces"):
            normal, offset, pitch, layers = PLANES[plane]
            n = scene.SliceDevice(normal=normal, offset=offset, pitch=pitch, layers=layers)
            got, starts = scene.Slice(normal, offset, pitch, layers, want_stats=False)
            assert n == len(got) > 0
            assert np.isin(got["node"], cut_cells).all()
            own, _ = sr.by_layer(sr.slice_triangles(tris[:, :, :3], normal, offset, pitch, layers), layers)
            for field in ("a", "layer", "b"):
                assert got[field].tobytes() == own[field].tobytes(), (plane, field)
