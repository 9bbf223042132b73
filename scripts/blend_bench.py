"""What a smooth blend costs (sdfhip_scene_blend), on cfg-2's 28 M-node scene (dragon_standin(9)) as A and
torus_d6 placed beside it (scaled by 0.4, its centre on the face of A's measured bounds) as B:

  blend     UNION at k = 0.02 to depth 9, and the morph at t = 0.5: kernel_ms (HIP events round the call's kernels, the per-level host
            synchronisations included), scene_ms, total_ms, the result's nodes, the points evaluated, the records the searches of each
            operand's surface loaded per point
  against   Offset(A, 0) and Offset(B, 0) to the same depth, timed in the same run: one search per point each.  A blend is two
            searches per point, so the expectation is about the sum of the two; `over_the_two_offsets` is the blend's kernel time over
            that sum (recorded, not gated)

Median, minimum and maximum of 5 calls after 1 warm-up (fewer where a case's calls would pass CASE_BUDGET_MS: each record says).

    python scripts/blend_bench.py [--out FILE] [--quick]       # prints one JSON line (and writes it to FILE)"""
import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import sdfbox_amd as sb  # noqa: E402

DEPTH, RADIUS, T, B_SCALE = 9, 0.02, 0.5, 0.4
CASE_BUDGET_MS = 40_000.0      # a case's timed calls, together: fewer than CALLS where one call is long


def spread(values, digits=3):
    a = np.asarray(values, dtype=np.float64)
    return {"median": round(float(np.median(a)), digits), "min": round(float(a.min()), digits), "max": round(float(a.max()), digits)}


def bench(what, call, calls, warmup, blend):
    rows, st, i = [], None, 0
    while i < warmup + calls:
        res, st = call()
        res.close()
        if i >= warmup:
            rows.append((st.kernel_ms, st.scene_ms, st.total_ms))
        elif i == warmup - 1:
            calls = max(1, min(calls, int(CASE_BUDGET_MS / max(st.total_ms, 1.0))))      # a case stays within its budget
        print(f"{what}: call {i} kernel {st.kernel_ms:.1f} ms", file=sys.stderr, flush=True)
        i += 1
    t = np.array(rows, dtype=np.float64)
    points = int(st.points)
    rec = {"what": what, "calls": len(rows), "nodes_out": int(st.nodes_out), "depth_out": int(st.depth_out), "points": points}
    if blend:
        rec.update(nodes_a=int(st.nodes_a), nodes_b=int(st.nodes_b), visited_a_per_point=round(int(st.visited_a) / max(1, points), 2),
                   visited_b_per_point=round(int(st.visited_b) / max(1, points), 2))
    else:
        rec.update(nodes_in=int(st.nodes_in), visited_per_point=round(int(st.visited) / max(1, points), 2))
    rec.update(kernel_ms=spread(t[:, 0]), scene_ms=spread(t[:, 1]), total_ms=spread(t[:, 2]),
               mpoints_per_s=round(points / float(np.median(t[:, 0])) / 1e3, 2))
    print(json.dumps(rec), file=sys.stderr, flush=True)
    return rec


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--out", default=None)
    ap.add_argument("--quick", action="store_true", help="one call of each after one warm-up")
    args = ap.parse_args()
    calls, warmup = (1, 1) if args.quick else (5, 1)
    line = {"what": "sdfhip_scene_blend", "device": torch.cuda.get_device_name(0), "calls": calls, "warmup": warmup, "scene": "dragon_standin_d9",
            "depth": DEPTH, "k": RADIUS, "t": T}
    od = sb.dragon_standin(9, nthreads=16)
    with sb.Scene(od) as A, sb.Scene(sb.torus_d6()) as torus:
        line["nodes"] = od.Length
        del od
        m = A.Measure()
        centre = [float(m.bounds_max[0]), 0.5 * float(m.bounds_min[1] + m.bounds_max[1]), 0.5 * float(m.bounds_min[2] + m.bounds_max[2])]
        centre = [min(max(c, 0.5 * B_SCALE), 1.0 - 0.5 * B_SCALE) for c in centre]           # the placed torus stays inside the cube
        move = [c - B_SCALE * 0.5 for c in centre]                                           # the source's centre (0.5, 0.5, 0.5) lands at `centre`
        with torus.Place(np.eye(3), B_SCALE, move, 8) as B:
            line["b"] = {"what": f"torus_d6 scaled by {B_SCALE}, its centre at {[round(c, 4) for c in centre]}, depth 8", "nodes": B.Length}
            union = bench(f"Blend(UNION, k = {RADIUS}, depth {DEPTH})", lambda: A.Blend(B, sb.BLEND_UNION, RADIUS, DEPTH, want_stats=True), calls, warmup, True)
            morph = bench(f"Morph(t = {T}, depth {DEPTH})", lambda: A.Morph(B, T, DEPTH, want_stats=True), calls, warmup, True)
            off_a = bench(f"Offset(A, 0, depth {DEPTH})", lambda: A.Offset(0.0, DEPTH, want_stats=True), calls, warmup, False)
            off_b = bench(f"Offset(B, 0, depth {DEPTH})", lambda: B.Offset(0.0, DEPTH, want_stats=True), calls, warmup, False)
    both = off_a["kernel_ms"]["median"] + off_b["kernel_ms"]["median"]
    for rec in (union, morph):
        rec["over_the_two_offsets"] = round(rec["kernel_ms"]["median"] / both, 3)
    line["blend"] = [union, morph]
    line["offsets"] = [off_a, off_b]
    text = json.dumps(line)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
