"""The child process of tests/test_gpu_gap.py::test_an_allocation_that_fails_is_nomem_and_a_plain_call_follows: on the
laboratory library, SDFHIP_GAP_FAIL_ALLOC=k for k = 0, 1, ... until sdfhip_instances_gap gets through; prints one JSON
line.  The hook fails a host-side allocation call with a status code; nothing on the device is provoked.  Not a test module."""
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
    import gap_cases as gc
    from conftest import bits_equal
    sb = sdfbox_amd.lab.load()
    L = sb._lib
    assert L.EXPERIMENTS
    name = "apart"
    parts = gc.parts(name)
    want = gc.restated(name)[0]
    cam, W, H = sb.Logic(64, 48), 64, 48
    report = {"codes_ok": True, "outputs_untouched": True, "failed": 0}
    with sb.Scene(product.sphere_d4()) as sphere:
        assert {src for src, _, _ in parts} == {"sphere_d4"}
        before = sphere.Draw(cam, W, H)
        handles = [(sphere, pl, op) for _, pl, op in parts]
        _, arr = sb.Scene._instances("child", handles)
        opt = sb.GapOptions()
        out = np.zeros(1, np.dtype(sb.Gap))
        n = ctypes.c_uint32(77)
        for k in range(16):
            os.environ["SDFHIP_GAP_FAIL_ALLOC"] = str(k)
            rc = L.lib.sdfhip_instances_gap(arr, len(arr), ctypes.byref(opt), out.ctypes.data, 1, ctypes.byref(n), None)
            if rc == L.OK:
                break
            said = L.lib.sdfhip_last_error()
            report["codes_ok"] = report["codes_ok"] and bool(rc == L.ERR_NOMEM and b"out of device memory" in said and b"instances_gap" in said)
            report["outputs_untouched"] = report["outputs_untouched"] and n.value == 77 and not out.view(np.uint8).any()
            report["failed"] += 1
        del os.environ["SDFHIP_GAP_FAIL_ALLOC"]
        report["source_frame_unchanged"] = bool(bits_equal(sphere.Draw(cam, W, H), before).all())
        # the call that got through, and a plain call after it: the restatement's bytes
        same = n.value == 1 and out.tobytes() == want.tobytes()
        again, _ = sb.Scene.GapParts(handles)
        report["plain_call_is_the_restatement"] = bool(same and again.tobytes() == want.tobytes())
    # the product flavour reads no such variable
    os.environ["SDFHIP_GAP_FAIL_ALLOC"] = "0"
    with product.Scene(product.sphere_d4()) as sphere:
        got, _ = product.Scene.GapParts([(sphere, pl, op) for _, pl, op in parts])
        report["product_reads_no_variable"] = bool(got.tobytes() == want.tobytes())
    print(json.dumps(report))


if __name__ == "__main__":
    main()
