"""The child process of tests/test_gpu_measure.py::test_an_allocation_that_fails_is_nomem_and_leaks_nothing: on the laboratory
library, SDFHIP_MEASURE_FAIL_ALLOC=k for k = 0, 1, ... until a call gets through; prints one JSON line.  Not a test module."""
import ctypes
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
    doubles = lambda m: np.array([m.volume, m.area, *m.moment1, *m.moment2, *m.bounds_min, *m.bounds_max], dtype=np.float64)
    report = {"codes_ok": True, "failed": 0}
    with sb.Scene(od) as scene:
        before = scene.Draw(cam, W, H)
        opt = sb.MeasureOptions()
        for k in range(8):
            os.environ["SDFHIP_MEASURE_FAIL_ALLOC"] = str(k)
            out = L.Measure()
            ctypes.memset(ctypes.byref(out), 0xFF, ctypes.sizeof(out))
            rc = L.lib.sdfhip_scene_measure(scene._h, ctypes.byref(opt), ctypes.byref(out))
            if rc == L.OK:
                break
            ok = rc == L.ERR_NOMEM and bytes(out) == bytes(ctypes.sizeof(out)) and b"out of device memory" in L.lib.sdfhip_last_error()
            report["codes_ok"] = report["codes_ok"] and bool(ok)
            report["failed"] += 1
        del os.environ["SDFHIP_MEASURE_FAIL_ALLOC"]
        after = scene.Draw(cam, W, H)
        report["frame_unchanged"] = bool(np.array_equal(before.view(np.uint32), after.view(np.uint32)))
        m = scene.Measure()
        report.update(doubles=doubles(m).tobytes().hex(), counts=[m.cells, m.cells_cut, m.cells_inside, *m.cells_at_depth])
    # the product flavour reads no such variable
    os.environ["SDFHIP_MEASURE_FAIL_ALLOC"] = "0"
    with product.Scene(od) as scene:
        report["product_reads_no_variable"] = doubles(scene.Measure()).tobytes().hex() == report["doubles"]
    print(json.dumps(report))


if __name__ == "__main__":
    main()
