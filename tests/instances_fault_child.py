"""The child process of tests/test_gpu_instances.py::test_an_allocation_that_fails_is_nomem_and_a_plain_call_follows: on the laboratory
library, SDFHIP_INSTANCES_FAIL_ALLOC=k for k = 0, 1, ... until the call gets through, for each of the seven entry points; prints one
JSON line.  The hook fails a host-side allocation call with a status code; nothing on the device is provoked.  Not a test module."""
import ctypes
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), HERE]

import numpy as np  # noqa: E402


def main():
    import torch
    import sdfbox_amd as product
    import sdfbox_amd.lab
    import instances_cases as ic
    import query_restatement as qr
    from conftest import bits_equal
    from sdfbox_amd.renderer import _rays
    sb = sdfbox_amd.lab.load()
    L = sb._lib
    assert L.EXPERIMENTS
    name = "two_spheres"
    parts = ic.parts(name)
    cam, (W, H) = ic.camera(name), ic.size(name)
    pts, px, rays = ic.points(name), ic.pixels(name), _rays(*ic.rays(name))
    report = {"codes_ok": True, "outputs_untouched": True, "failed": {}}
    with sb.Scene(product.sphere_d4()) as sphere:
        assert {src for src, _, _ in parts} == {"sphere_d4"}
        before = sphere.Draw(cam, W, H)
        handles = [(sphere, pl, op) for _, pl, op in parts]
        _, arr = sb.Scene._instances("child", handles)
        info = ctypes.byref(cam.State)
        probes = np.zeros(len(pts), np.dtype(sb.PartProbe))
        hits_r = np.zeros(len(rays), np.dtype(sb.PartHit))
        hits_p = np.zeros(len(px), np.dtype(sb.PartHit))
        frame = np.zeros((H, W, 4), np.float32)
        d_pts = torch.from_numpy(pts).cuda()
        d_rays = torch.from_numpy(rays.view(np.uint8).reshape(-1, 32)).cuda()
        d_probe = torch.zeros((len(pts), 32), dtype=torch.uint8, device="cuda")
        d_hit = torch.zeros((len(rays), 48), dtype=torch.uint8, device="cuda")
        d_frame = torch.zeros((H, W, 4), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        m, lim = cam.State.margin, cam.State.limit
        vp = ctypes.c_void_p
        calls = {
            "sample": (lambda: L.lib.sdfhip_instances_sample(arr, len(arr), None, pts.ctypes.data, len(pts), probes.ctypes.data), lambda: probes),
            "raycast": (lambda: L.lib.sdfhip_instances_raycast(arr, len(arr), None, rays.ctypes.data, len(rays), m, lim, hits_r.ctypes.data), lambda: hits_r),
            "pick": (lambda: L.lib.sdfhip_instances_pick(arr, len(arr), None, info, px.ctypes.data, len(px), hits_p.ctypes.data), lambda: hits_p),
            "render": (lambda: L.lib.sdfhip_instances_render(arr, len(arr), None, info, W, H, frame.ctypes.data), lambda: frame),
            "sample_device": (lambda: L.lib.sdfhip_instances_sample_device(arr, len(arr), None, vp(d_pts.data_ptr()), len(pts), vp(d_probe.data_ptr()), None),
                              lambda: d_probe.cpu().numpy()),
            "raycast_device": (lambda: L.lib.sdfhip_instances_raycast_device(arr, len(arr), None, vp(d_rays.data_ptr()), len(rays), m, lim,
                                                                             vp(d_hit.data_ptr()), None), lambda: d_hit.cpu().numpy()),
            "render_device": (lambda: L.lib.sdfhip_instances_render_device(arr, len(arr), None, info, W, H, vp(d_frame.data_ptr()), None),
                              lambda: d_frame.cpu().numpy()),
        }
        for what, (call, output) in calls.items():
            failed = 0
            for k in range(16):
                os.environ["SDFHIP_INSTANCES_FAIL_ALLOC"] = str(k)
                rc = call()
                if rc == L.OK:
                    break
                ok = rc == L.ERR_NOMEM and b"out of device memory" in L.lib.sdfhip_last_error() and b"instances_" + what.encode() in L.lib.sdfhip_last_error()
                report["codes_ok"] = report["codes_ok"] and bool(ok)
                report["outputs_untouched"] = report["outputs_untouched"] and not np.ascontiguousarray(output()).view(np.uint8).any()
                failed += 1
            report["failed"][what] = failed
        del os.environ["SDFHIP_INSTANCES_FAIL_ALLOC"]
        report["source_frames_unchanged"] = bool(bits_equal(sphere.Draw(cam, W, H), before).all())
        # plain calls: the restatement's bytes (the last call of each loop above got through: its output is one of them)
        same = not qr.records_differ(probes, ic.restated(name, "sample")) and not qr.records_differ(hits_r, ic.restated(name, "raycast"))
        same = same and not qr.records_differ(hits_p, ic.restated(name, "pick")) and bool(bits_equal(frame, ic.restated(name, "frame")).all())
        same = same and not qr.records_differ(d_probe.cpu().numpy().view(np.dtype(sb.PartProbe)).reshape(-1), ic.restated(name, "sample"))
        same = same and not qr.records_differ(d_hit.cpu().numpy().view(np.dtype(sb.PartHit)).reshape(-1), ic.restated(name, "raycast"))
        same = same and bool(bits_equal(d_frame.cpu().numpy(), ic.restated(name, "frame")).all())
        again = sb.Scene.DrawParts(handles, cam, W, H)
        report["plain_calls_are_the_restatements"] = bool(same and bits_equal(again, ic.restated(name, "frame")).all())
    # the product flavour reads no such variable
    os.environ["SDFHIP_INSTANCES_FAIL_ALLOC"] = "0"
    with product.Scene(product.sphere_d4()) as sphere:
        got = product.Scene.DrawParts([(sphere, pl, op) for _, pl, op in parts], cam, W, H)
        report["product_reads_no_variable"] = bool(bits_equal(got, ic.restated(name, "frame")).all())
    print(json.dumps(report))


if __name__ == "__main__":
    main()
