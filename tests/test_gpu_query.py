"""Point and ray queries on the GPU (sdfhip_scene_sample / _raycast / _pick and the _device forms), both flavours of the library:
every field of every record is the numpy restatement's (tests/query_restatement.py, held to the frozen oracle by
tests/test_query.py) bit for bit, on trees behind a dense grid, a split grid and no grid at all (the generic form); picks agree
with the GPU's own frames; the _device forms give the host forms' bytes and leave frames in flight alone; a pick places a brush;
the errors are status codes."""
import ctypes

import numpy as np
import pytest

import edit_restatement as er
import query_restatement as qr
from conftest import CAMERAS, assert_frames_identical, make_camera
from test_query import lattice_points, outside_points

pytestmark = pytest.mark.gpu
f32 = np.float32
SKY = np.array([0.005, 0.01, 0.2], dtype=np.float32)
SCENES = ["sphere_d4", "torus_d6", "gyroid_d8", "builder_d10", "builder_d10_nogrid", "inconsistent"]


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
        elif name == "gyroid_d8":
            _trees[name] = base.dragon_standin(8, nthreads=16)
        elif name == "builder_d10":
            _trees[name] = base.OctData.SdfGen(base.knot_point_cloud(100_000, seed=3), 10)
        elif name == "builder_d10_nogrid":
            _trees[name] = tree("builder_d10")
        elif name == "dragon_d9":
            _trees[name] = base.dragon_standin(9, nthreads=16)
        elif name == "inconsistent":
            # a child whose parent field points elsewhere: it uploads, but only the shader's own walk through the links may read it
            od = base.torus_d6()
            S = od.Structs.copy()
            S[int(S[0, 1]) + 3, 0] = int(S[0, 1])
            _trees[name] = base.OctData(S, od.Values)
    return _trees[name]


def upload(sb, name):
    """the scene, and the form its queries must take: a dense full-depth grid, a split grid, or none (the generic form)"""
    od = tree(name)
    scene = sb.Scene(od, top_grid_level=0) if name == "builder_d10_nogrid" else sb.Scene(od)
    if name in ("builder_d10_nogrid", "inconsistent"):
        assert scene.top_grid_level == 0 or not scene.stack_kernel_ok, name
    elif name == "builder_d10":
        assert scene.stack_kernel_ok and 0 < scene.top_grid_level < scene.depth, (name, scene.top_grid_level)      # split
    else:
        assert scene.stack_kernel_ok and scene.top_grid_level >= scene.depth, (name, scene.top_grid_level)           # dense
    return scene


def want(key, make):
    """the restatement's answer, computed once for both flavours"""
    if key not in _want:
        _want[key] = make()
    return _want[key]


def assert_records(got, ref, what):
    bad = qr.records_differ(got, ref)
    assert not bad, (what, bad)


def frame_pixels(W, H):
    ys, xs = np.mgrid[0:H, 0:W]
    return np.stack([xs.ravel(), ys.ravel()], 1).astype(np.uint32)


def random_rays(seed, n):
    """origins inside and around the box, directions of any length towards anywhere"""
    rng = np.random.default_rng(seed)
    o = rng.uniform(-0.6, 1.6, size=(n, 3))
    o[: n // 2] = rng.random((n // 2, 3))
    d = rng.normal(size=(n, 3)) * rng.uniform(0.2, 2.0, size=(n, 1))
    aim = rng.random(n) < 0.5                                   # half of them aimed at the box's middle region
    d[aim] = (rng.uniform(0.25, 0.75, size=(n, 3)) - o)[aim]
    return o.astype(f32), d.astype(f32)


@pytest.mark.parametrize("name", SCENES)
def test_sample_is_the_restatements(sb, name, monkeypatch):
    od = tree(name)
    rng = np.random.default_rng(101)
    depth = er.tree_depth(od.Structs)
    sets = {"uniform": rng.random((200_000, 3)).astype(f32), "lattice": lattice_points(rng, depth), "outside": outside_points(rng)}
    with upload(sb, name) as scene:
        for what, pts in sets.items():
            ref = want(("sample", name, what), lambda: qr.sample(od.Structs, od.Values, pts))
            got = scene.Sample(pts)
            assert (got["status"] == qr.HIT).all()
            assert_records(got, ref, (name, what))
        if sb._lib.EXPERIMENTS:
            # sample walks the links by default and the march looks the grid up; the laboratory library can force either form
            for form in ("grid", "generic"):
                monkeypatch.setenv("SDFHIP_QUERY_FORM", form)
                for what, pts in sets.items():
                    assert_records(scene.Sample(pts), want(("sample", name, what), None), (name, what, form))
            monkeypatch.delenv("SDFHIP_QUERY_FORM")
        # NaN / inf sprinkled in: those, and only those, INVALID and zero; the neighbours unaffected
        pts = sets["uniform"][:5000].copy()
        bad = np.array([0, 63, 64, 65, 255, 256, 1000, 4999])
        pts[bad, [0, 1, 2, 0, 1, 2, 0, 1]] = [np.nan, np.inf, -np.inf, np.nan, np.inf, np.nan, -np.inf, np.nan]
        got = scene.Sample(pts)
        assert (np.nonzero(got["status"] == qr.INVALID)[0] == bad).all()
        assert_records(got, qr.sample(od.Structs, od.Values, pts), (name, "non-finite"))
        zero = np.zeros(1, qr.PROBE); zero["status"] = qr.INVALID
        assert all(got[k].tobytes() == zero.tobytes() for k in bad)
        # batch sizes around a wavefront and a workgroup
        whole = want(("sample", name, "uniform"), None)
        for n in (0, 1, 63, 64, 65, 1000):
            got = scene.Sample(sets["uniform"][:n])
            assert len(got) == n
            assert_records(got, whole[:n], (name, f"n = {n}"))


@pytest.mark.parametrize("name", SCENES)
def test_raycast_and_pick_are_the_restatements_and_agree_with_the_frame(sb, name):
    od = tree(name)
    W = H = 256
    pixels = frame_pixels(W, H)
    n_sky = 0
    with upload(sb, name) as scene:
        for cam_name in CAMERAS:
            cam = make_camera(cam_name, W, H)
            # (the restatement's raycast along these rays IS its pick, the same loop on the same arrays:
            # tests/test_query.py::test_raycast_along_the_cameras_rays_is_pick)
            ref = want(("pick", name, cam_name), lambda: qr.pick(od.Structs, od.Values, cam.State, pixels))
            o, d = want(("rays", name, cam_name), lambda: qr.camera_rays(od.Structs, od.Values, cam.State, pixels))
            picked = scene.Pick(cam, pixels)
            assert_records(picked, ref, (name, cam_name, "pick"))
            assert_records(scene.Raycast(o, d, cam.State.margin, cam.State.limit), ref, (name, cam_name, "raycast along the camera's rays"))
            # against the GPU's own frame of the same camera: sky <=> ESCAPED, with steps == alpha there; elsewhere steps <= alpha
            frame = scene.Draw(cam, W, H).reshape(-1, 4)
            sky = (frame[:, :3].view(np.uint32) == SKY.view(np.uint32)).all(1)
            assert ((picked["status"] == qr.ESCAPED) == sky).all(), (name, cam_name)
            assert (picked["steps"][sky] == frame[sky, 3]).all() and (picked["steps"][~sky] <= frame[~sky, 3]).all(), (name, cam_name)
            n_sky += int(sky.sum())
    assert 0 < n_sky < 3 * W * H                                # both classes occur among the three cameras


@pytest.mark.parametrize("name", SCENES)
def test_random_rays_and_step_limits(sb, name, monkeypatch):
    od = tree(name)
    o, d = random_rays(7, 100_000)
    with upload(sb, name) as scene:
        ref = want(("random rays", name), lambda: qr.raycast(od.Structs, od.Values, o, d, 0.001, 4.0, 100))
        got = scene.Raycast(o, d, 0.001, 4.0, 100)
        assert_records(got, ref, (name, "random rays"))
        if sb._lib.EXPERIMENTS:                                 # the march's other form on the same tree
            monkeypatch.setenv("SDFHIP_QUERY_FORM", "generic")
            assert_records(scene.Raycast(o, d, 0.001, 4.0, 100), ref, (name, "random rays, links walked"))
            monkeypatch.delenv("SDFHIP_QUERY_FORM")
        assert all((got["status"] == s).sum() > 100 for s in (qr.HIT, qr.ESCAPED)), np.bincount(got["status"])
        # max_steps 1 and 4096 (fewer rays: the restatement steps while any lane does); a margin nothing meets exhausts the steps
        for steps, margin, n in ((1, 0.001, 20_000), (4096, 0.001, 3000), (4096, 0.0, 300)):
            ref = want(("random rays", name, steps, margin), lambda: qr.raycast(od.Structs, od.Values, o[:n], d[:n], margin, 4.0, steps))
            got = scene.Raycast(o[:n], d[:n], margin, 4.0, steps)
            assert_records(got, ref, (name, f"max_steps {steps}, margin {margin}"))
            assert got["steps"].max() <= steps
        # rays that start inside the solid: the first distance is negative and the shader's rule marches backwards
        s = scene.Sample(o[:50_000])
        inside = np.nonzero(s["distance"] < 0)[0][:2000]
        assert len(inside) > 50, len(inside)
        ref = qr.raycast(od.Structs, od.Values, o[inside], d[inside], 0.001, 4.0, 100)
        got = scene.Raycast(o[inside], d[inside], 0.001, 4.0, 100)
        assert_records(got, ref, (name, "from inside the solid"))
        # zero and non-finite directions and origins: INVALID and zeros, the neighbours unaffected
        o2, d2 = o[:1000].copy(), d[:1000].copy()
        bad = np.array([0, 63, 64, 65, 500, 999])
        d2[0] = 0.0; d2[63, 1] = np.nan; d2[64, 2] = np.inf; o2[65, 0] = -np.inf; d2[500] = (0.0, -0.0, 0.0); o2[999, 2] = np.nan
        got = scene.Raycast(o2, d2, 0.001, 4.0, 100)
        assert (np.nonzero(got["status"] == qr.INVALID)[0] == bad).all()
        assert_records(got, qr.raycast(od.Structs, od.Values, o2, d2, 0.001, 4.0, 100), (name, "bad rays"))
        zero = np.zeros(1, qr.HIT_REC); zero["status"] = qr.INVALID
        assert all(got[k].tobytes() == zero.tobytes() for k in bad)
        assert len(scene.Raycast(o[:0], d[:0], 0.001, 4.0)) == 0 and len(scene.Pick(make_camera("default", 64, 64), np.zeros((0, 2)))) == 0


@pytest.mark.parametrize("name", ["torus_d6", "builder_d10", "inconsistent"])
def test_device_forms_give_the_host_forms_bytes_beside_frames_in_flight(sb, name):
    import torch
    od = tree(name)
    W = H = 256
    cam = make_camera("rotated", W, H)
    rng = np.random.default_rng(31)
    pts = rng.random((70_001, 3)).astype(f32)
    o, d = random_rays(9, 30_000)
    with upload(sb, name) as scene:
        host_probe, host_hit = scene.Sample(pts), scene.Raycast(o, d, 0.001, 4.0, 100)
        alone = scene.Draw(cam, W, H)
        rays = np.zeros(len(o), np.dtype(sb.Ray)); rays["origin"] = o; rays["dir"] = d
        d_pts = torch.from_numpy(pts).cuda()
        d_rays = torch.from_numpy(rays.view(np.uint8).reshape(-1, 32)).cuda()
        d_probe = torch.zeros((len(pts), 32), dtype=torch.uint8, device="cuda")
        d_hit = torch.zeros((len(o), 48), dtype=torch.uint8, device="cuda")
        frames = [torch.zeros((H, W, 4), dtype=torch.float32, device="cuda") for _ in range(8)]
        torch.cuda.synchronize()
        s_frames, s_query = torch.cuda.Stream(), torch.cuda.Stream()
        for k, b in enumerate(frames):                      # frames in flight on one stream, queries on another, interleaved
            scene.DrawDevice(cam, W, H, b.data_ptr(), stream=s_frames.cuda_stream)
            if k % 2 == 0:
                scene.SampleDevice(d_pts.data_ptr(), len(pts), d_probe.data_ptr(), stream=s_query.cuda_stream)
            else:
                scene.RaycastDevice(d_rays.data_ptr(), len(o), 0.001, 4.0, d_hit.data_ptr(), stream=s_query.cuda_stream)
        torch.cuda.synchronize()
        assert d_probe.cpu().numpy().tobytes() == host_probe.tobytes(), name
        assert d_hit.cpu().numpy().tobytes() == host_hit.tobytes(), name
        for k, b in enumerate(frames):
            assert_frames_identical(b.cpu().numpy(), alone, f"{name}: frame {k} beside the queries")
        scene.SampleDevice(0, 0, 0); scene.RaycastDevice(0, 0, 0.001, 4.0, 0)        # n = 0 touches nothing


def test_a_pick_places_the_brush(sb):
    """The reason the feature exists: the pixel under the cursor -> a surface point -> a carve there."""
    od = tree("torus_d6")
    W = H = 256
    cam = make_camera("default", W, H)
    centre = np.array([[W // 2, H // 2]], dtype=np.uint32)
    with sb.Scene(od) as scene:
        hit = scene.Pick(cam, centre)[0]
        assert hit["status"] == qr.HIT
        p = hit["position"]
        with scene.Edit([(sb.EDIT_CARVE, sb.BRUSH_SPHERE, (*[float(v) for v in p], 0.05))]) as carved:
            a, b = scene.Draw(cam, W, H), carved.Draw(cam, W, H)
            assert not np.array_equal(a[H // 2, W // 2], b[H // 2, W // 2])
            before, after = scene.Sample([p])[0], carved.Sample([p])[0]
            assert after["distance"] > before["distance"] and after["distance"] > 0, (before["distance"], after["distance"])
            again = carved.Pick(cam, centre)[0]
            assert again["status"] != qr.HIT or again["t"] > hit["t"]               # the surface under the cursor moved away


def test_the_28m_node_scene_on_a_sampled_subset(sb):
    """cfg-2's scene: one sample batch of 1 M points and the 1080p camera's 2 073 600 picks.  The restatement is numpy, so it is
    held to every 997th element: 1004 of the points and 2080 of the pixels; the status counts are taken over all of them."""
    od = tree("dragon_d9")
    W, H = 1920, 1080
    cam = sb.Logic(W, H)
    cam.Position = (0.5, 0.5, -0.35); cam.Heading = (-0.2, 0.35)        # cfg-2's camera
    pts = np.random.default_rng(77).random((1_000_000, 3)).astype(f32)
    pixels = frame_pixels(W, H)
    with sb.Scene(od) as scene:
        probes, hits = scene.Sample(pts), scene.Pick(cam, pixels)
    assert (probes["status"] == qr.HIT).all() and len(hits) == W * H
    sub = slice(0, None, 997)
    assert len(pts[sub]) == 1004 and len(pixels[sub]) == 2080
    assert_records(probes[sub], want(("28m", "sample"), lambda: qr.sample(od.Structs, od.Values, pts[sub])), "28 M nodes, sample")
    assert_records(hits[sub], want(("28m", "pick"), lambda: qr.pick(od.Structs, od.Values, cam.State, pixels[sub])), "28 M nodes, pick")
    counts = np.bincount(hits["status"], minlength=4)
    assert counts[qr.HIT] > W * H // 10 and counts[qr.ESCAPED] > W * H // 10 and counts[qr.INVALID] == 0, counts


def test_errors_are_status_codes(sb):
    L = sb._lib
    od = tree("sphere_d4")
    info = sb.Logic(64, 64).State
    pts = np.zeros((4, 3), f32); rays = np.zeros(4, np.dtype(sb.Ray)); px = np.zeros((4, 2), np.uint32)
    probes = np.zeros(4, np.dtype(sb.Probe)); hits = np.zeros(4, np.dtype(sb.Hit))
    P = lambda a: a.ctypes.data
    with sb.Scene(od) as scene:
        h = scene._h
        refused = [
            lambda: L.lib.sdfhip_scene_sample(None, P(pts), 4, P(probes)),
            lambda: L.lib.sdfhip_scene_sample(h, None, 4, P(probes)),
            lambda: L.lib.sdfhip_scene_sample(h, P(pts), 4, None),
            lambda: L.lib.sdfhip_scene_sample_device(h, None, 4, None, None),
            lambda: L.lib.sdfhip_scene_raycast(h, None, 4, 0.001, 4.0, 100, P(hits)),
            lambda: L.lib.sdfhip_scene_raycast(h, P(rays), 4, 0.001, 4.0, 100, None),
            lambda: L.lib.sdfhip_scene_raycast(h, P(rays), 4, 0.001, 4.0, 0, P(hits)),
            lambda: L.lib.sdfhip_scene_raycast(h, P(rays), 4, 0.001, 4.0, 4097, P(hits)),
            lambda: L.lib.sdfhip_scene_raycast(h, P(rays), 4, float("nan"), 4.0, 100, P(hits)),
            lambda: L.lib.sdfhip_scene_raycast(h, P(rays), 4, 0.001, float("inf"), 100, P(hits)),
            lambda: L.lib.sdfhip_scene_raycast_device(h, None, 4, 0.001, 4.0, 100, None, None),
            lambda: L.lib.sdfhip_scene_raycast_device(h, P(rays), 4, 0.001, 4.0, 5000, P(hits), None),
            lambda: L.lib.sdfhip_scene_pick(h, None, P(px), 4, 100, P(hits)),
            lambda: L.lib.sdfhip_scene_pick(h, ctypes.byref(info), None, 4, 100, P(hits)),
            lambda: L.lib.sdfhip_scene_pick(h, ctypes.byref(info), P(px), 4, 100, None),
            lambda: L.lib.sdfhip_scene_pick(h, ctypes.byref(info), P(px), 4, 0, P(hits)),
        ]
        for k, call in enumerate(refused):
            assert call() == L.ERR_ARG, k
            assert L.lib.sdfhip_last_error(), k
        bad_info = sb.Info.from_buffer_copy(bytes(info)); bad_info.limit = float("nan")
        assert L.lib.sdfhip_scene_pick(h, ctypes.byref(bad_info), P(px), 4, 100, P(hits)) == L.ERR_ARG
        assert not probes.view(np.uint8).any() and not hits.view(np.uint8).any()      # a refused call wrote nothing
        # n = 0 is a success that touches nothing, null arrays included
        assert L.lib.sdfhip_scene_sample(h, None, 0, None) == L.OK and L.lib.sdfhip_scene_raycast(h, None, 0, 0.001, 4.0, 100, None) == L.OK
        assert L.lib.sdfhip_scene_pick(h, ctypes.byref(info), None, 0, 100, None) == L.OK
        assert L.lib.sdfhip_scene_pick(h, ctypes.byref(info), P(px), 4, 4096, P(hits)) == L.OK
