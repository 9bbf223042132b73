"""The placement's cost (sdfhip_scene_place) on cfg-2's 28 M-node scene (dragon_standin(9)): placed at half
size (a generic two-axis rotation about the cube's centre) and at identity (a resampling to the source's own depth, which refines
wherever the source's saturated bytes keep |value| small).  Per placement, median, minimum and maximum of 10 calls after 2 warm-ups:
kernel_ms (HIP events around the call's kernels, the per-level host synchronisations included), scene_ms (the new handle: fused
records, lookup grids), total_ms (host clock, the whole call); the nodes of source and result, the levels, the source look-ups made
and their rate.  Beside them the alternative a host has once it holds the result's arrays: sdfhip_scene_upload of the same result
from the host (median, minimum and maximum of 3).

    python scripts/place_bench.py [--out FILE]          # prints one JSON line (and writes it to FILE)"""
import argparse
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import sdfbox_amd as sb  # noqa: E402

CALLS, WARMUP, UPLOADS = 10, 2, 3
PLACEMENTS = (("half size, yaw 30 pitch 20", lambda: sb.placement(30, 20, 0, 0.5)),
              ("identity", lambda: sb.placement(0, 0, 0)))


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


def bench_case(scene, name, pl):
    rows, st = [], None
    for i in range(WARMUP + CALLS):
        res, st = scene.Place(*pl, want_stats=True)
        res.close()
        if i >= WARMUP:
            rows.append((st.kernel_ms, st.scene_ms, st.total_ms))
    t = np.array(rows, dtype=np.float64)
    # (st: the last call's; the counts below are the same in every call)
    rec = {"placement": name, "nodes_in": int(st.nodes_in), "nodes_out": int(st.nodes_out), "depth_out": int(st.depth_out),
           "levels": int(st.levels), "samples": int(st.samples),
           "kernel_ms": spread(t[:, 0], 4), "scene_ms": spread(t[:, 1]), "total_ms": spread(t[:, 2]),
           "Gsamples_per_s": round(int(st.samples) / float(np.median(t[:, 0])) / 1e6, 2)}
    res, od = scene.Place(*pl, want_octdata=True)
    res.close()
    rec["upload_of_the_result_ms"] = upload_ms(od)
    print(json.dumps(rec), file=sys.stderr, flush=True)
    return rec


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    line = {"what": "sdfhip_scene_place", "device": torch.cuda.get_device_name(0), "calls": CALLS, "warmup": WARMUP, "uploads": UPLOADS,
            "scene": "dragon_standin_d9", "cases": []}
    od = sb.dragon_standin(9, nthreads=16)
    with sb.Scene(od) as big:
        del od
        line["top_grid_level"] = int(big.top_grid_level)
        for name, make in PLACEMENTS:
            line["cases"].append(bench_case(big, name, make()))
    text = json.dumps(line)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
