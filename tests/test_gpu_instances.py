"""An assembly of placed instances on the GPU (sdfhip_instances_*), both flavours of the library: every case of
tests/instances_cases.py through sample, raycast, pick and render is the CPU restatement's (tests/instances_restatement.py) bit for
bit -- floats as their uint32 views; a NaN equals a NaN whatever its sign and payload, the project's convention (conftest.bits_equal,
query_restatement.records_differ): numpy on the host and the GPU need not agree on the sign of a default NaN, and the only NaNs
in this file are normals of a zero gradient, 0 * inf (tests/test_gpu_instances_zoo.py meets others: gradients of far points, inf - inf)
-- the host and the _device forms give the same bytes, so do the exact skip on and off
and the sources' three cursor forms in every pairing; the sources are untouched and may be freed; the errors are status codes that
name the instance; an allocation that fails is SDFHIP_ERR_NOMEM; the C++ mirror's methods give the same bytes."""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import compose_cases as cc
import compose_restatement as cr
import edit_restatement as er
import instances_cases as ic
import instances_restatement as ir
import query_restatement as qr
from conftest import REPO, assert_frames_identical, make_camera
from test_gpu_compose import Uploaded

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", params=["product", "lab"])
def sb(request):
    import sdfbox_amd
    if request.param == "product":
        return sdfbox_amd
    import sdfbox_amd.lab
    return sdfbox_amd.lab.load()


def host_answers(sb, handles, name, skip=True):
    """(sample, raycast, pick, frame) of the case through the host forms"""
    cam, (W, H), steps = ic.camera(name), ic.size(name), ic.max_steps(name)
    o, d = ic.rays(name)
    return (sb.Scene.SampleParts(handles, ic.points(name), skip=skip),
            sb.Scene.RaycastParts(handles, o, d, cam.State.margin, cam.State.limit, max_steps=steps, skip=skip),
            sb.Scene.PickParts(handles, cam, ic.pixels(name), max_steps=steps, skip=skip),
            sb.Scene.DrawParts(handles, cam, W, H, max_steps=steps, skip=skip))


def device_answers(sb, handles, name, skip=True):
    """(sample, raycast, frame) of the case through the _device forms, on a stream of the test's own"""
    import torch
    from sdfbox_amd.renderer import _rays
    cam, (W, H), steps = ic.camera(name), ic.size(name), ic.max_steps(name)
    pts, rays = ic.points(name), _rays(*ic.rays(name))
    d_pts = torch.from_numpy(pts).cuda()
    d_rays = torch.from_numpy(rays.view(np.uint8).reshape(-1, 32)).cuda()
    d_probe = torch.full((len(pts), 32), 0xEE, dtype=torch.uint8, device="cuda")
    d_hit = torch.full((len(rays), 48), 0xEE, dtype=torch.uint8, device="cuda")
    d_frame = torch.full((H, W, 4), -1.0, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    st = torch.cuda.Stream()
    sb.Scene.SamplePartsDevice(handles, d_pts.data_ptr(), len(pts), d_probe.data_ptr(), stream=st.cuda_stream, skip=skip)
    sb.Scene.RaycastPartsDevice(handles, d_rays.data_ptr(), len(rays), cam.State.margin, cam.State.limit, d_hit.data_ptr(), max_steps=steps,
                                stream=st.cuda_stream, skip=skip)
    sb.Scene.DrawPartsDevice(handles, cam, W, H, d_frame.data_ptr(), max_steps=steps, stream=st.cuda_stream, skip=skip)
    # (each call has waited for the stream: nothing is in flight)
    return (d_probe.cpu().numpy().view(np.dtype(sb.PartProbe)).reshape(-1), d_hit.cpu().numpy().view(np.dtype(sb.PartHit)).reshape(-1),
            d_frame.cpu().numpy())


def assert_restated(got, name, what):
    sample, raycast, pick, frame = got
    for records, kind in ((sample, "sample"), (raycast, "raycast"), (pick, "pick")):
        if records is not None:
            bad = qr.records_differ(records, ic.restated(name, kind))
            assert not bad, (what, kind, bad)
            assert not any(records[f].any() for f in records.dtype.names if f.startswith("pad")), (what, kind, "padding is zero")
    assert_frames_identical(frame, ic.restated(name, "frame"), f"{what}: frame")


@pytest.mark.parametrize("name", ic.NAMES)
def test_every_case_is_the_restatements(sb, name):
    parts = ic.parts(name)
    with Uploaded(sb, parts) as up:
        handles = up.parts(parts)
        for skip in (True, False):
            assert_restated(host_answers(sb, handles, name, skip), name, f"{name}, host forms, skip {skip}")
            s, r, f = device_answers(sb, handles, name, skip)
            assert_restated((s, r, None, f), name, f"{name}, device forms, skip {skip}")


def test_the_sources_three_cursor_forms_give_the_same_bytes(sb):
    name = "deepest"
    parts = ic.parts(name)                                   # sphere_d4 and torus_d6, both unions
    names = [src for src, _, _ in parts]
    split_level = {src: max(er.tree_depth(cc.tree(src)[0]) // 2, er.tree_depth(cc.tree(src)[0]) - 6) for src in names}
    with Uploaded(sb, parts) as grid, Uploaded(sb, parts, **{src: dict(top_grid_level=0) for src in names}) as none, \
            Uploaded(sb, parts, **{src: dict(top_grid_split=split_level[src]) for src in names}) as split:
        for src in names:
            g, n, s = grid.scenes[src], none.scenes[src], split.scenes[src]
            assert g.stack_kernel_ok and g.top_grid_level >= g.depth and n.top_grid_level == 0
            assert s.top_grid_level == split_level[src] < s.depth
        for first in (grid, none, split):
            for second in (grid, none, split):
                handles = [(first.scenes[names[0]], parts[0][1], parts[0][2]), (second.scenes[names[1]], parts[1][1], parts[1][2])]
                for skip in (True, False):
                    assert_restated(host_answers(sb, handles, name, skip), name, f"forms {first is grid, first is split} x {second is grid, second is split}")
        # all three forms of ONE source in one list
        three = ic.parts("three_forms")
        assert {src for src, _, _ in three} == {"sphere_d4"} and len(three) == 3
        handles = [(up.scenes["sphere_d4"], pl, op) for up, (_, pl, op) in zip((grid, split, none), three)]
        assert_restated(host_answers(sb, handles, "three_forms"), "three_forms", "three forms of one source in one call")


def test_the_sources_are_untouched_and_nothing_is_kept(sb):
    W, H = 64, 48
    name = "csg"
    parts = ic.parts(name)
    cams = [make_camera(cam, W, H) for cam in ("default", "rotated")]
    up = Uploaded(sb, parts)
    before = {src: [scene.Draw(cam, W, H) for cam in cams] for src, scene in up.scenes.items()}
    got = host_answers(sb, up.parts(parts), name)
    dev = device_answers(sb, up.parts(parts), name)
    for src, scene in up.scenes.items():
        for cam, frame in zip(cams, before[src]):
            assert_frames_identical(scene.Draw(cam, W, H), frame, f"{src} after the calls")
    up.__exit__()
    # the sources are freed: the answers stand alone, and a fresh upload answers the same
    assert_restated(got, name, "answers read after the sources were freed")
    assert_restated((dev[0], dev[1], None, dev[2]), name, "device answers read after the sources were freed")
    with Uploaded(sb, parts) as again:
        assert_restated(host_answers(sb, again.parts(parts), name), name, "a fresh upload")


def test_errors_are_status_codes_and_nothing_is_touched_at_zero(sb):
    L = sb._lib
    R, s, t = cc.ONE_PLACEMENTS["generic_half"]()
    cam = sb.Logic(16, 16).State
    with sb.Scene(sb.OctData(*cc.tree("sphere_d4"))) as scene, sb.Scene(sb.OctData(*cc.tree("nine"))) as nine:
        good = lambda **kw: sb.Instance(**dict(dict(scene=scene._h, op=0, rotation=R.tolist(), scale=s, translation=t.tolist()), **kw))
        pts = np.zeros((4, 3), np.float32)
        out = np.zeros(4, np.dtype(sb.PartProbe))
        hits = np.zeros(4, np.dtype(sb.PartHit))
        px = np.zeros((4, 2), np.uint32)
        rays = np.zeros(4, np.dtype(sb.Ray))
        rays["dir"] = 1.0
        frame = np.zeros((2, 2, 4), np.float32)

        def every(items, n_items=None, n=4, side=2, opt=None):
            arr = (sb.Instance * len(items))(*items)
            k = len(items) if n_items is None else n_items
            o = ctypes.byref(opt) if opt is not None else None
            info = ctypes.byref(cam)
            return {"sample": lambda: L.lib.sdfhip_instances_sample(arr, k, o, pts.ctypes.data, n, out.ctypes.data),
                    "raycast": lambda: L.lib.sdfhip_instances_raycast(arr, k, o, rays.ctypes.data, n, 0.001, 3.0, hits.ctypes.data),
                    "pick": lambda: L.lib.sdfhip_instances_pick(arr, k, o, info, px.ctypes.data, n, hits.ctypes.data),
                    "render": lambda: L.lib.sdfhip_instances_render(arr, k, o, info, side, side, frame.ctypes.data)}

        for name, call in every([good(), good(op=2), good(scene=nine._h, op=1)]).items():
            assert call() == L.OK, (name, L.lib.sdfhip_last_error())
        # further down the list than a test without handles can reach: the index in the message is the instance's
        long = [good() for _ in range(70)]
        for at, bad, word in ((66, good(op=7), b"unknown op"), (69, good(scene=None), b"null scene"), (65, good(scale=-2.0), b"scale"),
                              (67, good(rotation=((1, 0, 0), (0, 1, 0), (0, 0, 1.01))), b"orthogonal")):
            items = list(long)
            items[at] = bad
            for name, call in every(items).items():
                rc, msg = call(), L.lib.sdfhip_last_error()
                assert rc == L.ERR_ARG and b"instance %d" % at in msg and word in msg and b"instances_" + name.encode() in msg, (name, msg)
        # n = 0 and a 0 x 0 frame: successes that touch nothing -- null arrays are not even looked at
        for name, call in every([good(), good()], n=0, side=0).items():
            assert call() == L.OK, name
        arr = (sb.Instance * 1)(good())
        assert L.lib.sdfhip_instances_sample(arr, 1, None, None, 0, None) == L.OK
        assert L.lib.sdfhip_instances_sample_device(arr, 1, None, None, 0, None, None) == L.OK
        assert L.lib.sdfhip_instances_raycast_device(arr, 1, None, None, 0, 0.001, 3.0, None, None) == L.OK
        assert L.lib.sdfhip_instances_render_device(arr, 1, None, ctypes.byref(cam), 0, 0, None, None) == L.OK
        assert L.lib.sdfhip_instances_render(arr, 1, None, ctypes.byref(cam), 5, 0, None) == L.OK
        # ... but a null array with something to answer is refused
        assert L.lib.sdfhip_instances_sample(arr, 1, None, None, 3, None) == L.ERR_ARG
        assert L.lib.sdfhip_instances_render(arr, 1, None, ctypes.byref(cam), 2, 2, None) == L.ERR_ARG
        # the options: the defaults are max_steps 100 and normal_step 2^-10, given or not
        handles = [(scene, (R, s, t)), (nine, cc.ONE_PLACEMENTS["mirror"](), cr.COMBINE_UNION)]
        a = sb.Scene.RaycastParts(handles, [[0.5, 0.5, -0.5]], [[0, 0, 1]], 0.001, 3.0)
        b = sb.Scene.RaycastParts(handles, [[0.5, 0.5, -0.5]], [[0, 0, 1]], 0.001, 3.0, max_steps=100, normal_step=2.0 ** -10)
        assert not qr.records_differ(a, b)
        c = sb.Scene.RaycastParts(handles, [[0.5, 0.5, -0.5]], [[0, 0, 1]], 0.001, 3.0, normal_step=2.0 ** -7)
        inst = cr.as_instances([(cc.tree("sphere_d4"), (R, s, t)), (cc.tree("nine"), cc.ONE_PLACEMENTS["mirror"](), cr.COMBINE_UNION)])
        assert not qr.records_differ(c, ir.raycast(inst, [[0.5, 0.5, -0.5]], [[0, 0, 1]], 0.001, 3.0, h=np.float32(2.0 ** -7)))
        assert not qr.records_differ(a, ir.raycast(inst, [[0.5, 0.5, -0.5]], [[0, 0, 1]], 0.001, 3.0))


def test_an_allocation_that_fails_is_nomem_and_a_plain_call_follows():
    # in a fresh process of its own, so that neither the variable nor a failed call can reach the tests beside this one: every
    # allocation each call reaches fails once through the library's own host-side allocation hook (nothing on the device is
    # provoked), each is SDFHIP_ERR_NOMEM, and afterwards a plain call gives the restatement's bytes (tests/instances_fault_child.py)
    child = os.path.join(REPO, "tests", "instances_fault_child.py")
    out = subprocess.run([sys.executable, child], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, (out.returncode, out.stdout[-2000:], out.stderr[-2000:])
    report = json.loads(out.stdout.strip().splitlines()[-1])
    # the table, the records in and the records out of a host form; the table alone of a _device form; a frame has no records in
    assert report["failed"] == {"sample": 3, "raycast": 3, "pick": 3, "render": 2, "sample_device": 1, "raycast_device": 1, "render_device": 1}, report
    assert report["codes_ok"] and report["outputs_untouched"] and report["source_frames_unchanged"], report
    assert report["plain_calls_are_the_restatements"] and report["product_reads_no_variable"], report


def test_the_cpp_mirror_draws_picks_and_samples_the_parts(tmp_path):
    # Program::DrawParts / PickParts / SampleParts (include/sdfbox.hpp) on "two_spheres": the restatement's bytes (tests/cpp_parts.cpp)
    import shutil
    import sdfbox_amd as product
    from conftest import GOLDEN
    name = "two_spheres"
    W, H = ic.size(name)
    exe, libdir = str(tmp_path / "cpp_parts"), os.path.join(REPO, "sdfbox_amd")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-I", os.path.join(REPO, "include"), os.path.join(REPO, "tests", "cpp_parts.cpp"),
                           "-o", exe, "-L", libdir, "-lsdfhip", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    shutil.copy(os.path.join(GOLDEN, "sphere_d4.asdf"), tmp_path / "sphere.asdf")
    golden = product.OctData.LoadAsdf(str(tmp_path / "sphere.asdf"))
    assert np.array_equal(golden.Structs, cc.tree("sphere_d4")[0]) and np.array_equal(golden.Values, cc.tree("sphere_d4")[1])
    ic.pixels(name).tofile(tmp_path / "pixels.bin")
    ic.points(name).tofile(tmp_path / "points.bin")
    out = subprocess.run([exe, str(tmp_path / "sphere.asdf"), str(W), str(H), str(tmp_path / "pixels.bin"), str(tmp_path / "points.bin"),
                          str(tmp_path / "out")], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, (out.returncode, out.stderr)
    assert_frames_identical(np.fromfile(tmp_path / "out.frame", dtype=np.float32).reshape(H, W, 4), ic.restated(name, "frame"), "Program::DrawParts")
    assert not qr.records_differ(np.fromfile(tmp_path / "out.hits", dtype=ir.PART_HIT), ic.restated(name, "pick"))
    assert not qr.records_differ(np.fromfile(tmp_path / "out.probes", dtype=ir.PART_PROBE), ic.restated(name, "sample"))
