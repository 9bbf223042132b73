"""The penetration depth (sdfhip_instances_penetration) in the flow it is for, against the route the library
offered before it, on cfg-2's 28 M-node scene (dragon_standin(9)) and torus_d6 in turn, K = 2, 8 and 32 instances.  The arrangement is
"crowded": compose_bench.py's grid of cells with every instance at 1.6 of its cell where the clash bench has 0.9 -- neighbours DO
overlap (the clash bench's arrangements have no pair at all).  The flow: one Scene.ClashParts at depth 6 on the unit cube; then, for
the RECORDS records with the most shared points, clash_box(record) and on that cube, at lattice depths 5 and 6, in the same process
and alternating inside every one of CALLS rounds after WARMUP:
  call    one Scene.PenetrationParts of the whole list on the box: call_ms = host clock round the synchronous call; kernel_ms and
          pass_ms (count, bitmaps, emit, searches, fold, records) = the call's own device events; searches, visited per search
  route   what a user had: the box's lattice points made and inverse-mapped in torch, one Scene.DistanceDevice per instance on ALL of
          them (the exact signed distance; it knows no containment mask to skip by), then the pairing in torch: inside = distance < 0,
          r = |distance| * s, and per pair with a shared point the maximum of min(r_a, r_b).  Neither the witness nor the nearest
          points are computed.  Host clock to the last synchronise.  Its depths are compared with the call's once and the largest
          difference recorded (its sign is sdfhip_scene_sample's at the clamped point, not the clash rule's: they may part outside
          a source's cube)
Every figure is the median, minimum and maximum over the rounds.  These figures are recorded, not gated.

    python scripts/penetration_bench.py [--out FILE]          # prints one JSON line (and writes it to FILE)"""
import argparse
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.dirname(os.path.abspath(__file__))]

import numpy as np  # noqa: E402
import torch  # noqa: E402

import sdfbox_amd as sb  # noqa: E402
from compose_bench import COUNTS, spread  # noqa: E402

CALLS, WARMUP, RECORDS = 5, 1, 2
CLASH_DEPTH, DEPTHS = 6, (5, 6)
PASSES = ("count", "bitmaps", "emit", "searches", "fold", "records")


def placements(k):
    """compose_bench.placements with 1.6 of a cell instead of 0.9: instance i round the centre of cell i, turned by its index"""
    n = 2 if k <= 8 else 4
    out = []
    for i in range(k):
        cell = (i % n, i // n % n, i // (n * n) % n)
        out.append(sb.placement(37.0 * i, 11.0 * i - 40.0, 5.0 * i, 1.6 / n, to=tuple((c + 0.5) / n for c in cell)))
    return out


def route_depths(parts, depth, origin, side, clear):
    """{(a, b): depth} by the route; clear: room for 8^depth sdfhip_clearance records on the device"""
    n, st = 1 << depth, torch.cuda.current_stream().cuda_stream
    pitch = np.float32(side) * np.float32(2.0 ** -depth)
    axis = [(torch.arange(n, dtype=torch.float32, device="cuda") + 0.5) * float(pitch) + float(np.float32(o)) for o in origin]
    z, y, x = torch.meshgrid(axis[2], axis[1], axis[0], indexing="ij")
    p = torch.stack([x.reshape(-1), y.reshape(-1), z.reshape(-1)], 1)
    inside, r = [], []
    for scene, (R, s, t) in parts:
        q = (((p - torch.from_numpy(np.asarray(t, np.float32)).cuda()) @ torch.from_numpy(np.asarray(R, np.float32)).cuda()) * (1.0 / float(s))).contiguous()
        scene.DistanceDevice(q.data_ptr(), len(q), clear.data_ptr(), stream=st)
        dist = clear.view(torch.float32)[:len(q), 0].clone()
        inside.append(dist < 0)
        r.append(dist.abs() * float(s))
    inside, r = torch.stack(inside), torch.stack(r)
    c = inside.float()
    counts = (c @ c.T).cpu().numpy()                 # (exact: at most 2^18 points)
    out = {}
    for a in range(len(parts)):
        for b in range(a + 1, len(parts)):
            if counts[a, b] > 0:
                both = inside[a] & inside[b]
                out[(a, b)] = float(torch.minimum(r[a], r[b])[both].max())
    torch.cuda.synchronize()
    return out


def bench_box(parts, record, depth, clear):
    origin, side = sb.clash_box(record, CLASH_DEPTH)
    rec, st = sb.Scene.PenetrationParts(parts, depth=depth, origin=origin, side=side)
    again, _ = sb.Scene.PenetrationParts(parts, depth=depth, origin=origin, side=side, skip=False)
    assert rec.tobytes() == again.tobytes(), "the records with and without the skip differ"
    by_route = route_depths(parts, depth, origin, side, clear)
    by_call = {(int(x["a"]), int(x["b"])): float(x["depth"]) for x in rec}
    shared = sorted(set(by_route) & set(by_call))
    diff = max([abs(by_route[k] - by_call[k]) for k in shared], default=0.0)
    t = {"call": [], "route": []}
    kernel, passes = [], []
    for i in range(WARMUP + CALLS):
        for what in t:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            if what == "call":
                s = sb.Scene.PenetrationParts(parts, depth=depth, origin=origin, side=side)[1]
            else:
                route_depths(parts, depth, origin, side, clear)
            torch.cuda.synchronize()
            if i >= WARMUP:
                t[what].append((time.perf_counter() - t0) * 1e3)
                if what == "call":
                    kernel.append(s.kernel_ms)
                    passes.append(list(s.pass_ms))
    passes = np.asarray(passes, dtype=np.float64)
    out = {"pair": [int(record["a"]), int(record["b"])], "box_side": round(float(side), 6), "depth": depth, "points": int(st.points),
           "pairs_in_box": int(len(rec)), "deepest": round(float(rec["depth"].max()), 6) if len(rec) else None,
           "searches": int(st.searches), "visited_per_search": round(st.visited / max(1, st.searches), 2),
           "lookups_per_point": round(st.lookups / st.points, 4),
           "call_ms": spread(t["call"]), "kernel_ms": spread(kernel),
           "pass_ms_median": {name: round(float(np.median(passes[:, k])), 4) for k, name in enumerate(PASSES)},
           "route_ms": spread(t["route"]), "route_pairs": len(by_route), "pairs_in_both": len(shared), "route_depth_max_abs_diff": diff,
           "route_over_call": round(float(np.median(t["route"]) / np.median(t["call"])), 2)}
    print(json.dumps(out), file=sys.stderr, flush=True)
    return out


def bench_case(parts, clear):
    K = len(parts)
    clash_ms = []
    for i in range(WARMUP + CALLS):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        records, _ = sb.Scene.ClashParts(parts, depth=CLASH_DEPTH)
        if i >= WARMUP:
            clash_ms.append((time.perf_counter() - t0) * 1e3)
    assert len(records) >= 1, f"K = {K}: the crowded arrangement has no overlapping pair"
    order = np.argsort(-records["points"].astype(np.int64), kind="stable")[:RECORDS]
    return {"arrangement": "crowded", "instances": K, "clash_depth": CLASH_DEPTH, "clash_pairs": int(len(records)), "clash_ms": spread(clash_ms),
            "boxes": [bench_box(parts, records[i], depth, clear) for i in order for depth in DEPTHS]}


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    line = {"what": "sdfhip_instances_penetration", "device": torch.cuda.get_device_name(0), "calls": CALLS, "warmup": WARMUP, "depths": list(DEPTHS),
            "records_per_case": RECORDS, "scenes": ["dragon_standin_d9", "torus_d6"], "passes": list(PASSES),
            "clock": "host, round a synchronous call; kernel_ms, pass_ms: the call's device events",
            "spread": "median, minimum, maximum over the rounds; call and route alternate inside a round", "cases": []}
    od = sb.dragon_standin(9, nthreads=16)
    with sb.Scene(od) as big, sb.Scene(sb.torus_d6()) as torus:
        del od
        line["nodes_in"] = [int(big.Length), int(torus.Length)]
        clear = torch.empty((8 ** max(DEPTHS), 32), dtype=torch.uint8, device="cuda")
        for k in COUNTS:
            line["cases"].append(bench_case([((big, torus)[i & 1], pl) for i, pl in enumerate(placements(k))], clear))
    text = json.dumps(line)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
