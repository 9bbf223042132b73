"""The child process of tests/test_gpu_blend.py::test_an_allocation_that_fails_is_nomem_and_leaves_the_operands: on the laboratory
library, SDFHIP_BLEND_FAIL_ALLOC=k for k = 0, 1, ... until a call gets through; prints one JSON line.  Not a test module."""
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
    od_a = product.sphere_d4()
    od_b = product.OctData.Generate(L.SHAPE_TORUS, [0.5, 0.5, 0.5, 0.25, 0.1], 4)          # tests/test_gpu_distance.py's torus_d4
    opt = sb.BlendOptions(L.BLEND_UNION, 0.03, 3)
    sha = lambda a: hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()
    same = lambda x, y: bool(np.array_equal(x.view(np.uint32), y.view(np.uint32)))
    report = {"codes_ok": True, "blend_failed": 0}
    with sb.Scene(od_a) as A, sb.Scene(od_b) as B:
        before = A.Draw(cam, W, H), B.Draw(cam, W, H)
        for k in range(64):
            os.environ["SDFHIP_BLEND_FAIL_ALLOC"] = str(k)
            h = ctypes.c_void_p()
            raw = L.COctData()
            rc = L.lib.sdfhip_scene_blend(A._h, B._h, ctypes.byref(opt), ctypes.byref(h), ctypes.byref(raw), None)
            if rc == L.OK:
                L.lib.sdfhip_scene_free(h)
                L.lib.sdfhip_octdata_free(ctypes.byref(raw))
                break
            ok = rc == L.ERR_NOMEM and not h.value and raw.length == 0 and not raw.structs and b"out of device memory" in L.lib.sdfhip_last_error()
            report["codes_ok"] = report["codes_ok"] and bool(ok)
            report["blend_failed"] += 1
        del os.environ["SDFHIP_BLEND_FAIL_ALLOC"]
        report["frames_unchanged"] = same(before[0], A.Draw(cam, W, H)) and same(before[1], B.Draw(cam, W, H))
        res, got = A.Blend(B, L.BLEND_UNION, 0.03, 3, want_octdata=True)
        with res:
            report.update(nodes_after=int(got.Length), structs_sha=sha(got.Structs), values_sha=sha(got.Values))
    # the product flavour reads no such variable
    os.environ["SDFHIP_BLEND_FAIL_ALLOC"] = "0"
    with product.Scene(od_a) as A, product.Scene(od_b) as B, A.Blend(B, L.BLEND_UNION, 0.03, 3) as res:
        report["product_reads_no_variable"] = res.Length == report["nodes_after"]
    print(json.dumps(report))


if __name__ == "__main__":
    main()
