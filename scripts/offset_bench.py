"""What the exact distance costs (sdfhip_scene_distance / sdfhip_scene_offset), on cfg-2's 28 M-node scene
(dragon_standin(9)):

  distance_device  1 M points, uniform in the cube, in random order and sorted in Morton order: ms per launch (HIP events round the
                   launch, the bitmap's rebuild included), Mpoints/s, and the mean and maximum of `visited` (records a search loaded)
  offset           delta = +0.01 and -0.01 to depth 9, and the shell of thickness 0.02: kernel_ms (HIP events round the call's
                   kernels, the per-level host synchronisations included), scene_ms, total_ms, the result's nodes, the points
                   evaluated, the records their searches loaded
  against          the only route there was: Mesh(level 6) -> sdfhip_trimesh_prepare -> sdfhip_trimesh_build to depth 9 (the field
                   of the level-6 surface, rebuilt; an offset of it would still need its bytes shifted on the host), host clock

Median, minimum and maximum of 5 calls after 1 warm-up (fewer where a case's calls would pass CASE_BUDGET_MS: each record says).

    python scripts/offset_bench.py [--out FILE] [--quick]       # prints one JSON line (and writes it to FILE)"""
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

POINTS = 1_000_000
DEPTH, DELTA, THICKNESS, LOD = 9, 0.01, 0.02, 6
CASE_BUDGET_MS = 40_000.0      # an offset's timed calls, together: fewer than CALLS where one call is long


def spread(values, digits=3):
    a = np.asarray(values, dtype=np.float64)
    return {"median": round(float(np.median(a)), digits), "min": round(float(a.min()), digits), "max": round(float(a.max()), digits)}


def morton_order(p):
    q = np.clip((p * 1024.0).astype(np.int64), 0, 1023)
    code = np.zeros(len(p), np.int64)
    for b in range(10):
        for a in range(3):
            code |= ((q[:, a] >> b) & 1) << (3 * b + a)
    return np.argsort(code, kind="stable")


def bench_distance(scene, calls, warmup):
    rng = np.random.default_rng(1)
    pts = rng.random((POINTS, 3)).astype(np.float32)
    st = torch.cuda.Stream()
    d_out = torch.zeros((POINTS, 8), dtype=torch.int32, device="cuda")
    out = []
    for order, p in (("random", pts), ("morton", pts[morton_order(pts)])):
        d_in = torch.from_numpy(np.ascontiguousarray(p)).cuda()
        ms = []
        for i in range(warmup + calls):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(st)
            scene.DistanceDevice(d_in.data_ptr(), POINTS, d_out.data_ptr(), stream=st.cuda_stream)
            e1.record(st)
            e1.synchronize()
            if i >= warmup:
                ms.append(e0.elapsed_time(e1))
        rec = d_out.cpu().numpy().view(np.dtype(sb.Clearance)).reshape(-1)
        row = {"points": POINTS, "order": order, "ms": spread(ms, 4), "mpoints_per_s": round(POINTS / float(np.median(ms)) / 1e3, 2),
               "visited_mean": round(float(rec["visited"].mean()), 2), "visited_max": int(rec["visited"].max()),
               "abs_distance_mean": round(float(np.abs(rec["distance"]).mean()), 5)}
        print(json.dumps(row), file=sys.stderr, flush=True)
        out.append(row)
        del d_in
    return out


def bench_offset(scene, what, call, calls, warmup):
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
    rec = {"what": what, "calls": len(rows), "nodes_in": int(st.nodes_in), "nodes_out": int(st.nodes_out), "depth_out": int(st.depth_out), "points": int(st.points),
           "visited": int(st.visited), "visited_per_point": round(int(st.visited) / max(1, int(st.points)), 2),
           "kernel_ms": spread(t[:, 0]), "scene_ms": spread(t[:, 1]), "total_ms": spread(t[:, 2]),
           "mpoints_per_s": round(int(st.points) / float(np.median(t[:, 0])) / 1e3, 2)}
    print(json.dumps(rec), file=sys.stderr, flush=True)
    return rec


def bench_rebuild(scene, calls, warmup):
    """Mesh(level 6) -> prepare -> build to depth 9, each step on the host clock"""
    rows, n_tri, nodes = [], 0, 0
    for i in range(warmup + calls):
        t0 = time.perf_counter()
        tris = scene.Mesh(LOD, want_stats=False)
        t1 = time.perf_counter()
        tm = sb.TriMesh.FromMesh(tris)
        t2 = time.perf_counter()
        res = tm.Build(DEPTH)
        t3 = time.perf_counter()
        n_tri, nodes = len(tris), res.Length
        res.close()
        tm.close()
        if i >= warmup:
            rows.append(((t1 - t0) * 1e3, (t2 - t1) * 1e3, (t3 - t2) * 1e3, (t3 - t0) * 1e3))
    t = np.array(rows, dtype=np.float64)
    rec = {"what": f"Mesh(level {LOD}) -> trimesh_prepare -> trimesh_build(depth {DEPTH})", "triangles": n_tri, "nodes_out": nodes,
           "mesh_ms": spread(t[:, 0]), "prepare_ms": spread(t[:, 1]), "build_ms": spread(t[:, 2]), "total_ms": spread(t[:, 3])}
    print(json.dumps(rec), file=sys.stderr, flush=True)
    return rec


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--out", default=None)
    ap.add_argument("--quick", action="store_true", help="one call of each after one warm-up")
    args = ap.parse_args()
    calls, warmup = (1, 1) if args.quick else (5, 1)
    line = {"what": "sdfhip_scene_distance / sdfhip_scene_offset", "device": torch.cuda.get_device_name(0), "calls": calls, "warmup": warmup,
            "scene": "dragon_standin_d9"}
    od = sb.dragon_standin(9, nthreads=16)
    with sb.Scene(od) as big:
        line["nodes"] = od.Length
        del od
        line["distance_device"] = bench_distance(big, calls, warmup)
        line["offset"] = [bench_offset(big, f"Offset({DELTA:+}, depth {DEPTH})", lambda: big.Offset(DELTA, DEPTH, want_stats=True), calls, warmup),
                          bench_offset(big, f"Offset({-DELTA:+}, depth {DEPTH})", lambda: big.Offset(-DELTA, DEPTH, want_stats=True), calls, warmup),
                          bench_offset(big, f"Shell({THICKNESS}, depth {DEPTH})", lambda: big.Shell(THICKNESS, DEPTH, want_stats=True), calls, warmup)]
        line["rebuild_from_the_mesh"] = bench_rebuild(big, calls, warmup)
    text = json.dumps(line)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
