"""The child process of tests/test_gpu_volume.py::test_an_allocation_that_fails_is_nomem_and_leaves_the_library_working: on the
laboratory library, SDFHIP_VOLUME_FAIL_ALLOC=k for k = 0, 1, ... until a build gets through; prints one JSON line.  Not a test
module."""
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
    import volume_cases as vc
    sb = sdfbox_amd.lab.load()
    L = sb._lib
    assert L.EXPERIMENTS
    c = vc.case("tsdf_d6")
    grid = c["grid"]
    nz, ny, nx = grid.shape
    vol = sb.Volume((nx, ny, nz), c["origin"], c["spacing"], c["value_scale"], L.VOLUME_F32, c["depth"])
    sha = lambda a: hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()
    report = {"codes_ok": True, "failed": 0}
    for k in range(64):
        os.environ["SDFHIP_VOLUME_FAIL_ALLOC"] = str(k)
        h = ctypes.c_void_p()
        raw = L.COctData()
        rc = L.lib.sdfhip_volume_build(0, grid.ctypes.data, ctypes.byref(vol), ctypes.byref(h), ctypes.byref(raw), None)
        if rc == L.OK:
            L.lib.sdfhip_scene_free(h)
            L.lib.sdfhip_octdata_free(ctypes.byref(raw))
            break
        ok = rc == L.ERR_NOMEM and not h.value and raw.length == 0 and not raw.structs and b"out of device memory" in L.lib.sdfhip_last_error()
        report["codes_ok"] = report["codes_ok"] and bool(ok)
        report["failed"] += 1
    del os.environ["SDFHIP_VOLUME_FAIL_ALLOC"]
    res, got = sb.Scene.FromVolume(grid, c["origin"], c["spacing"], c["depth"], c["value_scale"], want_octdata=True)
    with res:
        report.update(nodes_after=int(got.Length), structs_sha=sha(got.Structs), values_sha=sha(got.Values))
        # the out direction's host form has one allocation
        lattice = sb.Volume((9, 9, 9), (0, 0, 0), 0.125)
        out = np.zeros((9, 9, 9), dtype=np.float32)
        os.environ["SDFHIP_VOLUME_FAIL_ALLOC"] = "0"
        rc = L.lib.sdfhip_scene_volume(res._h, ctypes.byref(lattice), out.ctypes.data)
        report["out_is_nomem"] = bool(rc == L.ERR_NOMEM and b"out of device memory" in L.lib.sdfhip_last_error() and not out.any())
        del os.environ["SDFHIP_VOLUME_FAIL_ALLOC"]
        again = res.Volume((9, 9, 9))
        report["out_works_afterwards"] = bool(np.isfinite(again).all() and again.any())
    # the product flavour reads no such variable
    os.environ["SDFHIP_VOLUME_FAIL_ALLOC"] = "0"
    with product.Scene.FromVolume(grid, c["origin"], c["spacing"], c["depth"], c["value_scale"]) as res:
        report["product_reads_no_variable"] = res.Length == report["nodes_after"]
    print(json.dumps(report))


if __name__ == "__main__":
    main()
