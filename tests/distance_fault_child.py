"""The child process of tests/test_gpu_distance.py::test_an_allocation_that_fails_is_nomem_and_leaves_the_source: on the laboratory
library, SDFHIP_OFFSET_FAIL_ALLOC=k and SDFHIP_DISTANCE_FAIL_ALLOC=k for k = 0, 1, ... until a call gets through; prints one JSON
line.  Not a test module."""
import ctypes
import hashlib
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), HERE]

import numpy as np  # noqa: E402


def main():
    import sdfbox_amd as product
    import sdfbox_amd.lab
    sb = sdfbox_amd.lab.load()
    L = sb._lib
    assert L.EXPERIMENTS
    W, H = 64, 48
    cam = sb.Logic(W, H)
    od = product.sphere_d4()
    opt = sb.OffsetOptions(L.OFFSET_GROW, 0.03, 3)
    pts = (np.random.default_rng(3).random((64, 3)) * 1.2 - 0.1).astype(np.float32)
    sha = lambda a: hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()
    report = {"codes_ok": True, "offset_failed": 0, "distance_failed": 0}
    with sb.Scene(od) as scene:
        before = scene.Draw(cam, W, H)
        for k in range(64):
            os.environ["SDFHIP_OFFSET_FAIL_ALLOC"] = str(k)
            h = ctypes.c_void_p()
            raw = L.COctData()
            rc = L.lib.sdfhip_scene_offset(scene._h, ctypes.byref(opt), ctypes.byref(h), ctypes.byref(raw), None)
            if rc == L.OK:
                L.lib.sdfhip_scene_free(h)
                L.lib.sdfhip_octdata_free(ctypes.byref(raw))
                break
            ok = rc == L.ERR_NOMEM and not h.value and raw.length == 0 and not raw.structs and b"out of device memory" in L.lib.sdfhip_last_error()
            report["codes_ok"] = report["codes_ok"] and bool(ok)
            report["offset_failed"] += 1
        del os.environ["SDFHIP_OFFSET_FAIL_ALLOC"]
        out = np.zeros(len(pts), np.dtype(sb.Clearance))
        for k in range(16):
            os.environ["SDFHIP_DISTANCE_FAIL_ALLOC"] = str(k)
            rc = L.lib.sdfhip_scene_distance(scene._h, pts.ctypes.data, len(pts), -1, out.ctypes.data)
            if rc == L.OK:
                break
            ok = rc == L.ERR_NOMEM and b"out of device memory" in L.lib.sdfhip_last_error()
            report["codes_ok"] = report["codes_ok"] and bool(ok)
            report["distance_failed"] += 1
        del os.environ["SDFHIP_DISTANCE_FAIL_ALLOC"]
        after = scene.Draw(cam, W, H)
        report["source_frame_unchanged"] = bool(np.array_equal(before.view(np.uint32), after.view(np.uint32)))
        res, got = scene.Offset(0.03, 3, want_octdata=True)
        with res:
            report.update(nodes_after=int(got.Length), structs_sha=sha(got.Structs), values_sha=sha(got.Values))
        report["distance_sha"] = sha(scene.Distance(pts)["distance"])
    # the product flavour reads no such variable
    os.environ["SDFHIP_OFFSET_FAIL_ALLOC"] = "0"
    os.environ["SDFHIP_DISTANCE_FAIL_ALLOC"] = "0"
    with product.Scene(od) as scene, scene.Offset(0.03, 3) as res:
        report["product_reads_no_variable"] = res.Length == report["nodes_after"] and sha(scene.Distance(pts)["distance"]) == report["distance_sha"]
    print(json.dumps(report))


if __name__ == "__main__":
    main()
