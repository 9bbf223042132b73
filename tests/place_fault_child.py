"""The child process of tests/test_gpu_place.py::test_an_allocation_that_fails_is_nomem_and_leaves_the_source: on the laboratory
library, SDFHIP_PLACE_FAIL_ALLOC=k for k = 0, 1, ... until a call gets through; prints one JSON line.  Not a test module."""
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
    od = product.torus_d6()
    R, s, t = product.placement(30, 20, 0, 0.62)
    pl = sb.Placement(R.tolist(), s, t.tolist(), 7)
    sha = lambda a: hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()
    report = {"codes_ok": True, "failed": 0}
    with sb.Scene(od) as scene:
        before = scene.Draw(cam, W, H)
        for k in range(64):
            os.environ["SDFHIP_PLACE_FAIL_ALLOC"] = str(k)
            h = ctypes.c_void_p()
            raw = L.COctData()
            rc = L.lib.sdfhip_scene_place(scene._h, ctypes.byref(pl), ctypes.byref(h), ctypes.byref(raw), None)
            if rc == L.OK:
                L.lib.sdfhip_scene_free(h)
                L.lib.sdfhip_octdata_free(ctypes.byref(raw))
                break
            ok = rc == L.ERR_NOMEM and not h.value and raw.length == 0 and not raw.structs and b"out of device memory" in L.lib.sdfhip_last_error()
            report["codes_ok"] = report["codes_ok"] and bool(ok)
            report["failed"] += 1
        del os.environ["SDFHIP_PLACE_FAIL_ALLOC"]
        after = scene.Draw(cam, W, H)
        report["source_frame_unchanged"] = bool(np.array_equal(before.view(np.uint32), after.view(np.uint32)))
        res, got = scene.Place(R, s, t, 7, want_octdata=True)
        with res:
            report.update(nodes_after=int(got.Length), structs_sha=sha(got.Structs), values_sha=sha(got.Values))
    # the product flavour reads no such variable
    os.environ["SDFHIP_PLACE_FAIL_ALLOC"] = "0"
    with product.Scene(od) as scene, scene.Place(R, s, t, 7) as res:
        report["product_reads_no_variable"] = res.Length == report["nodes_after"]
    print(json.dumps(report))


if __name__ == "__main__":
    main()
