"""The child process of tests/test_gpu_compose.py::test_an_allocation_that_fails_is_nomem_and_leaves_the_sources: on the laboratory
library, SDFHIP_COMPOSE_FAIL_ALLOC=k for k = 0, 1, ... until a call gets through; prints one JSON line.  Not a test module."""
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
    # compose_cases' "far": the torus as the placement's own child places it, and a sphere three cubes away, to depth 7
    sources = [product.torus_d6(), product.sphere_d4()]
    placements = [product.placement(30, 20, 0, 0.62), (np.eye(3, dtype=np.float32), 1.0, (3.0, 0.0, 0.0))]
    depth = 7
    sha = lambda a: hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()
    report = {"codes_ok": True, "failed": 0}
    with sb.Scene(sources[0]) as torus, sb.Scene(sources[1]) as sphere:
        scenes = (torus, sphere)
        before = [s.Draw(cam, W, H) for s in scenes]
        items = [sb.Instance(s._h, 0, np.asarray(R, dtype=np.float32).tolist(), sc, np.asarray(t, dtype=np.float32).tolist())
                 for s, (R, sc, t) in zip(scenes, placements)]
        arr = (sb.Instance * 2)(*items)
        opt = sb.ComposeOptions(depth)
        for k in range(64):
            os.environ["SDFHIP_COMPOSE_FAIL_ALLOC"] = str(k)
            h = ctypes.c_void_p()
            raw = L.COctData()
            rc = L.lib.sdfhip_scene_compose(arr, 2, ctypes.byref(opt), ctypes.byref(h), ctypes.byref(raw), None)
            if rc == L.OK:
                L.lib.sdfhip_scene_free(h)
                L.lib.sdfhip_octdata_free(ctypes.byref(raw))
                break
            ok = rc == L.ERR_NOMEM and not h.value and raw.length == 0 and not raw.structs and b"out of device memory" in L.lib.sdfhip_last_error()
            report["codes_ok"] = report["codes_ok"] and bool(ok)
            report["failed"] += 1
        del os.environ["SDFHIP_COMPOSE_FAIL_ALLOC"]
        after = [s.Draw(cam, W, H) for s in scenes]
        report["source_frames_unchanged"] = all(bool(np.array_equal(b.view(np.uint32), a.view(np.uint32))) for b, a in zip(before, after))
        res, got = sb.Scene.Compose(list(zip(scenes, placements)), depth, want_octdata=True)
        with res:
            report.update(nodes_after=int(got.Length), structs_sha=sha(got.Structs), values_sha=sha(got.Values))
    # the product flavour reads no such variable
    os.environ["SDFHIP_COMPOSE_FAIL_ALLOC"] = "0"
    with product.Scene(sources[0]) as torus, product.Scene(sources[1]) as sphere:
        with product.Scene.Compose(list(zip((torus, sphere), placements)), depth) as res:
            report["product_reads_no_variable"] = res.Length == report["nodes_after"]
    print(json.dumps(report))


if __name__ == "__main__":
    main()
