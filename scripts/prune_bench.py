"""The prune's cost (sdfhip_scene_prune) on cfg-2's 28 M-node scene (dragon_standin(9)): the scene as
uploaded at tolerance 0 (a prune that finds little), and the scene after the r = 0.05 sphere carve profiles/edit_bench.json times
(centred on the surface point under the cfg-2 camera's central ray) at tolerance 0 and 1.  Per case, median, minimum and maximum of
20 calls after 3 warm-ups: kernel_ms (HIP events around the prune's kernels), scene_ms (the new handle: fused records, lookup
grids), total_ms (host clock, the whole call); nodes in and out; the bytes the kernels must move (one read of the 16-byte records
plus one write of the survivors' 16 bytes); kernel_ms as a multiple of ONE read of the records at the device's measured streaming
read rate (sdfhip_device_bandwidth), as the mesh count is reported.  Beside them the alternative a host has without the call:
sdfhip_scene_upload of the pruned tree from the host (median, minimum and maximum of 5).

    python scripts/prune_bench.py [--out FILE]          # prints one JSON line (and writes it to FILE)"""
import argparse
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import edit_restatement as er  # noqa: E402
import sdfbox_amd as sb  # noqa: E402

W, H = 1920, 1080
CALLS, WARMUP, UPLOADS = 20, 3, 5
RECORD_BYTES = 16


def spread(values, digits=3):
    a = np.asarray(values, dtype=np.float64)
    return {"median": round(float(np.median(a)), digits), "min": round(float(a.min()), digits), "max": round(float(a.max()), digits)}


def upload_ms(od):
    t = []
    for _ in range(1 + UPLOADS):                           # (the first: a warm-up)
        t0 = time.perf_counter()
        s = sb.Scene(od)
        t.append((time.perf_counter() - t0) * 1e3)
        s.close()
    return spread(t[1:])


def bench_case(name, scene, tolerance, read_gbs):
    rows = []
    for i in range(WARMUP + CALLS):
        res, st = scene.Prune(tolerance, want_stats=True)
        res.close()
        if i >= WARMUP:
            rows.append((st.kernel_ms, st.scene_ms, st.total_ms))
    res, od, st = scene.Prune(tolerance, want_octdata=True, want_stats=True)
    res.close()
    a = np.array(rows, dtype=np.float64)
    one_read_ms = st.nodes_in * RECORD_BYTES / (read_gbs * 1e9) * 1e3
    rec = {"case": name, "tolerance": tolerance, "nodes_in": int(st.nodes_in), "nodes_out": int(st.nodes_out),
           "blocks_removed": int(st.blocks_removed), "depth_out": int(st.depth_out),
           "kernel_ms": spread(a[:, 0], 4), "scene_ms": spread(a[:, 1]), "total_ms": spread(a[:, 2]),
           "bytes_min": int((st.nodes_in + st.nodes_out) * RECORD_BYTES),
           "one_read_of_the_records_ms": round(one_read_ms, 4),
           "kernel_ms_over_one_read": round(float(np.median(a[:, 0])) / one_read_ms, 2),
           "upload_of_the_result_ms": upload_ms(od)}
    print(json.dumps(rec), file=sys.stderr, flush=True)
    return rec


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    cam = sb.Logic(W, H)
    cam.Position = (0.5, 0.5, -0.35); cam.Heading = (-0.2, 0.35)        # cfg-2's camera
    _, _, read_gbs = sb.device_bandwidth(0)
    line = {"what": "sdfhip_scene_prune", "device": torch.cuda.get_device_name(0), "calls": CALLS, "warmup": WARMUP, "uploads": UPLOADS,
            "scene": "dragon_standin_d9", "read_GBps": round(read_gbs, 1), "cases": []}
    od = sb.dragon_standin(9, nthreads=16)
    c = er.surface_point_under(od.Structs, cam.Position, [list(r) for r in cam.State.heading])
    line["brush_centre"] = [round(v, 6) for v in c]
    with sb.Scene(od) as scene:
        del od
        line["cases"].append(bench_case("as_uploaded", scene, 0, read_gbs))
        with scene.Edit([(sb.EDIT_CARVE, sb.BRUSH_SPHERE, (*c, 0.05))]) as carved:
            for tolerance in (0, 1):
                line["cases"].append(bench_case("after_r0.05_carve", carved, tolerance, read_gbs))
    text = json.dumps(line)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
