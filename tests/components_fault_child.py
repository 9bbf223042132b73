"""The child process of tests/test_gpu_components.py::test_an_allocation_that_fails_is_nomem_and_a_plain_call_follows: on the
laboratory library, SDFHIP_COMPONENTS_FAIL_ALLOC=k for k = 0, 1, ... until sdfhip_scene_components gets through; prints one JSON
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
    import components_cases as cs
    from conftest import bits_equal
    sb = sdfbox_amd.lab.load()
    L = sb._lib
    assert L.EXPERIMENTS
    name, depth = "hollow", 5
    want, want_labels = cs.restated(name, depth)
    cam, W, H = sb.Logic(64, 48), 64, 48
    report = {"codes_ok": True, "outputs_untouched": True, "failed": 0}
    with sb.Scene(sb.OctData(*cs.tree(name))) as scene:
        before = scene.Draw(cam, W, H)
        opt = sb.ComponentsOptions(depth=depth)
        out = np.zeros(len(want), np.dtype(sb.Component))
        labels = np.zeros(8 ** depth, np.uint32)
        n = ctypes.c_uint32(77)
        for k in range(16):
            os.environ["SDFHIP_COMPONENTS_FAIL_ALLOC"] = str(k)
            rc = L.lib.sdfhip_scene_components(scene._h, ctypes.byref(opt), out.ctypes.data, len(out), ctypes.byref(n), labels.ctypes.data, None)
            if rc == L.OK:
                break
            said = L.lib.sdfhip_last_error()
            report["codes_ok"] = report["codes_ok"] and bool(rc == L.ERR_NOMEM and b"out of device memory" in said and b"scene_components" in said)
            report["outputs_untouched"] = report["outputs_untouched"] and n.value == 77 and not out.view(np.uint8).any() and not labels.any()
            report["failed"] += 1
        del os.environ["SDFHIP_COMPONENTS_FAIL_ALLOC"]
        report["source_frame_unchanged"] = bool(bits_equal(scene.Draw(cam, W, H), before).all())
        # the call that got through, and a plain call after it: the restatement's bytes
        same = n.value == len(want) and out.tobytes() == want.tobytes() and labels.tobytes() == want_labels.tobytes()
        again, _, again_labels = scene.Components(depth=depth, labels=True)
        report["plain_call_is_the_restatement"] = bool(same and again.tobytes() == want.tobytes() and again_labels.tobytes() == want_labels.tobytes())
    # the product flavour reads no such variable
    os.environ["SDFHIP_COMPONENTS_FAIL_ALLOC"] = "0"
    with product.Scene(product.OctData(*cs.tree(name))) as scene:
        got, _ = scene.Components(depth=depth)
        report["product_reads_no_variable"] = bool(got.tobytes() == want.tobytes())
    print(json.dumps(report))


if __name__ == "__main__":
    main()
