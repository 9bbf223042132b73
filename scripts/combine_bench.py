"""The combination's cost (sdfhip_scene_combine) on cfg-2's 28 M-node scene (dragon_standin(9)), combined
with torus_d6 (a small second operand: the result is the big scene re-ordered breadth first, plus the torus's cells) and with itself
(a == b: every cell shared, the most the call reads).  Per pair and op, median, minimum and maximum of 10 calls after 2 warm-ups:
kernel_ms (HIP events around the call's kernels, the per-level host synchronisations included), scene_ms (the new handle: fused
records, lookup grids), total_ms (host clock, the whole call); the nodes of both operands and of the result; the bytes the kernels
must move at least (one read of both operands' 16-byte records plus one write of the result's 16 bytes per node); kernel_ms as a
multiple of the time that traffic takes at the device's measured streaming copy rate (sdfhip_device_bandwidth: bytes read plus
bytes written per second).  Beside them the alternative a host has once it holds the result's arrays: sdfhip_scene_upload of the
same result from the host (median, minimum and maximum of 3).

    python scripts/combine_bench.py [--out FILE]          # prints one JSON line (and writes it to FILE)"""
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
RECORD_BYTES = 16
OPS = (("union", sb.COMBINE_UNION), ("intersect", sb.COMBINE_INTERSECT), ("subtract", sb.COMBINE_SUBTRACT))


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


def bench_case(pair, a, b, name, op, copy_gbs, want_upload):
    rows, st = [], None
    for i in range(WARMUP + CALLS):
        res, st = a.Combine(b, op, want_stats=True)
        res.close()
        if i >= WARMUP:
            rows.append((st.kernel_ms, st.scene_ms, st.total_ms))
    t = np.array(rows, dtype=np.float64)
    # (st: the last call's; the node counts below are the same in every call)
    read_bytes, write_bytes = (st.nodes_a + st.nodes_b) * RECORD_BYTES, st.nodes_out * RECORD_BYTES
    traffic_ms = (read_bytes + write_bytes) / (copy_gbs * 1e9) * 1e3
    rec = {"pair": pair, "op": name, "nodes_a": int(st.nodes_a), "nodes_b": int(st.nodes_b), "nodes_out": int(st.nodes_out),
           "nodes_shared": int(st.nodes_shared), "depth_out": int(st.depth_out),
           "kernel_ms": spread(t[:, 0], 4), "scene_ms": spread(t[:, 1]), "total_ms": spread(t[:, 2]),
           "bytes_min": int(read_bytes + write_bytes), "one_read_of_both_and_one_write_ms": round(traffic_ms, 4),
           "kernel_ms_over_that_traffic": round(float(np.median(t[:, 0])) / traffic_ms, 2)}
    if want_upload:                                        # (the result's size does not depend on the op: timed once per pair)
        res, od = a.Combine(b, op, want_octdata=True)
        res.close()
        rec["upload_of_the_result_ms"] = upload_ms(od)
    print(json.dumps(rec), file=sys.stderr, flush=True)
    return rec


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    copy_gbs, _, _ = sb.device_bandwidth(0)
    line = {"what": "sdfhip_scene_combine", "device": torch.cuda.get_device_name(0), "calls": CALLS, "warmup": WARMUP, "uploads": UPLOADS,
            "scene": "dragon_standin_d9", "copy_GBps": round(copy_gbs, 1), "cases": []}
    od = sb.dragon_standin(9, nthreads=16)
    with sb.Scene(od) as big, sb.Scene(sb.torus_d6()) as torus:
        del od
        for pair, other in (("dragon_standin_d9 x torus_d6", torus), ("dragon_standin_d9 x itself", big)):
            for k, (name, op) in enumerate(OPS):
                line["cases"].append(bench_case(pair, big, other, name, op, copy_gbs, k == 0))
    text = json.dumps(line)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
