"""The clearance (sdfhip_instances_gap) against the route the library offered before it, on cfg-2's 28 M-node
scene (dragon_standin(9)) and torus_d6 in turn, K = 2, 8 and 32 instances in compose_bench.py's arrangement (instance i at 0.9 of
cell i of a grid, turned by its index; that no two parts overlap is asserted from the records: no GAP_CONTAINED, no gap of 0).  Per arrangement, in the same process:
  call      Scene.GapParts of the whole list at limit = +inf, at a small limit (SMALL_LIMIT) and, where the estimate of its searches
            allows (NO_PRUNE_MAX_SEARCHES), with no pruning: call_ms = host clock round the synchronous call; kernel_ms and pass_ms
            (cell lists, bitmaps, searches, records) = the call's own device events; the counters.  CALLS rounds after WARMUP
  route     what a user had: Scene.MeshDevice of part a's source, its vertices mapped forward and into part b's source in torch, one
            Scene.DistanceDevice per ORDERED pair on all of them, and a torch minimum of |distance| * s_b.  Neither the witness nor
            the other side's point are computed.  Host clock to the last synchronise.  Ordered pairs are timed one by one until
            half of ROUTE_BUDGET_S is spent on their kind (the large scene or the torus as the first part); if some are left, the
            total is EXTRAPOLATED from the mean of those timed of the same kind and the line says so.  Its gaps are compared with the call's on the pairs timed
Every figure is the median, minimum and maximum over the rounds.  These figures are recorded, not gated.

    python scripts/gap_bench.py [--out FILE] [--counts 2,8,32]          # prints one JSON line (and writes it to FILE)"""
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
from compose_bench import placements, spread  # noqa: E402

CALLS, WARMUP = 3, 1
SMALL_LIMIT = 0.01
NO_PRUNE_MAX_SEARCHES = 4e8
ROUTE_BUDGET_S = 40.0
PASSES = ("cell_lists", "bitmaps", "searches", "records")


def timed_call(parts, **kw):
    t, kernel, passes, st = [], [], [], None
    rec = None
    for i in range(WARMUP + CALLS):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        rec, st = sb.Scene.GapParts(parts, **kw)
        if i >= WARMUP:
            t.append((time.perf_counter() - t0) * 1e3)
            kernel.append(st.kernel_ms)
            passes.append(list(st.pass_ms))
    passes = np.asarray(passes, dtype=np.float64)
    out = {"records": int(len(rec)), "least_gap": round(float(rec["gap"].min()), 6) if len(rec) else None, "pairs": int(st.pairs),
           "contained_records": int((rec["flags"] & sb.GAP_CONTAINED != 0).sum()), "zero_gaps": int((rec["gap"] == 0).sum()),
           "pairs_searched": int(st.pairs_searched), "cells": int(st.cells), "searches_last_call": int(st.searches),
           "visited_per_search_last_call": round(st.visited / max(1, st.searches), 2), "call_ms": spread(t), "kernel_ms": spread(kernel),
           "pass_ms_median": {name: round(float(np.median(passes[:, k])), 4) for k, name in enumerate(PASSES)}}
    return rec, out


class Meshes:
    """the vertices of each distinct source, meshed once per route run as the route would"""

    def __init__(self):
        self.buf = {}

    def of(self, scene):
        if scene not in self.buf:
            n = scene.MeshDevice()
            v = torch.empty((n, 3, 6), dtype=torch.float32, device="cuda")
            got = scene.MeshDevice(v.data_ptr(), n, stream=torch.cuda.current_stream().cuda_stream)
            assert got == n
            self.buf[scene] = v[:, :, :3].reshape(-1, 3)
        return self.buf[scene]


def route_pair(meshes, a, b):
    """min over a's vertices of |Distance_b| * s_b"""
    (sa, (Ra, s_a, ta)), (sb_, (Rb, s_b, tb)) = a, b
    x = meshes.of(sa)
    Ra_, Rb_ = torch.from_numpy(np.asarray(Ra, np.float32)).cuda(), torch.from_numpy(np.asarray(Rb, np.float32)).cuda()
    w = (x @ Ra_.T) * float(s_a) + torch.from_numpy(np.asarray(ta, np.float32)).cuda()
    q = (((w - torch.from_numpy(np.asarray(tb, np.float32)).cuda()) @ Rb_) * (1.0 / float(s_b))).contiguous()
    clear = torch.empty((len(q), 32), dtype=torch.uint8, device="cuda")
    sb_.DistanceDevice(q.data_ptr(), len(q), clear.data_ptr(), stream=torch.cuda.current_stream().cuda_stream)
    return float(clear.view(torch.float32)[:, 0].abs().min()) * float(s_b)


def timed_route(parts, big, by_call):
    K = len(parts)
    # the cheap kind first (a torus's 96 k vertices into anything), so that both kinds are timed before either budget is spent
    ordered = sorted([(a, b) for a in range(K) for b in range(K) if a != b], key=lambda ab: parts[ab[0]][0] is big)
    spent, by_kind, gaps, done = {True: 0.0, False: 0.0}, {True: [], False: []}, {}, set()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    meshes = Meshes()
    for s in {p[0] for p in parts}:
        meshes.of(s)
    torch.cuda.synchronize()
    mesh_ms = (time.perf_counter() - t0) * 1e3
    for a, b in ordered:
        kind = parts[a][0] is big
        if spent[kind] > ROUTE_BUDGET_S / 2:
            continue
        t0 = time.perf_counter()
        g = route_pair(meshes, parts[a], parts[b])
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        spent[kind] += dt
        done.add((a, b))
        by_kind[kind].append(dt * 1e3)
        key = (min(a, b), max(a, b))
        gaps[key] = min(g, gaps.get(key, np.inf))
    total = mesh_ms + sum(float(np.mean(by_kind[parts[a][0] is big])) for a, b in ordered)
    both = [k for k in gaps if k in by_call and k in done and k[::-1] in done]
    return {"mesh_ms": round(mesh_ms, 3), "ordered_pairs": len(ordered), "ordered_pairs_timed": len(done), "extrapolated": len(done) < len(ordered),
            "pair_ms_large_first": spread(by_kind[True]) if by_kind[True] else None, "pair_ms_torus_first": spread(by_kind[False]) if by_kind[False] else None,
            "route_ms": round(total, 3), "pairs_compared": len(both),
            "gap_max_abs_diff": max([abs(gaps[k] - by_call[k]) for k in both], default=None)}


def bench_case(parts, big, big_triangles, torus_triangles):
    K = len(parts)
    out = {"arrangement": "disjoint", "instances": K}
    rec, out["limit_inf"] = timed_call(parts)
    # the arrangement is meant to be disjoint: no record says that a closest point lies inside the other part, and no gap is 0
    assert len(rec) == K * (K - 1) // 2 and not (rec["flags"] & sb.GAP_CONTAINED).any() and (rec["gap"] > 0).all(), "the arrangement is not disjoint"
    print(json.dumps({"instances": K, "limit_inf": out["limit_inf"]}), file=sys.stderr, flush=True)
    _, out["limit_small"] = timed_call(parts, limit=SMALL_LIMIT)
    out["limit_small"]["limit"] = SMALL_LIMIT
    tri = [big_triangles if p[0] is big else torus_triangles for p in parts]
    closed = 3 * sum(tri) * (K - 1)
    if closed <= NO_PRUNE_MAX_SEARCHES:
        full, out["no_prune"] = timed_call(parts, prune=False)
        assert full.tobytes() == rec.tobytes(), "the records with and without pruning differ"
        assert out["no_prune"]["searches_last_call"] == closed
    else:
        out["no_prune"] = {"not_run": f"{closed} searches, above {int(NO_PRUNE_MAX_SEARCHES)}"}
    by_call = {(int(r["a"]), int(r["b"])): float(r["gap"]) for r in rec}
    out["route"] = timed_route(parts, big, by_call)
    out["route_over_call"] = round(out["route"]["route_ms"] / out["limit_inf"]["call_ms"]["median"], 2)
    print(json.dumps(out), file=sys.stderr, flush=True)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--out", default=None)
    ap.add_argument("--counts", default="2,8,32")
    args = ap.parse_args()
    counts = [int(c) for c in args.counts.split(",")]
    line = {"what": "sdfhip_instances_gap", "device": torch.cuda.get_device_name(0), "calls": CALLS, "warmup": WARMUP, "small_limit": SMALL_LIMIT,
            "scenes": ["dragon_standin_d9", "torus_d6"], "passes": list(PASSES), "route_budget_s": ROUTE_BUDGET_S,
            "clock": "host, round a synchronous call; kernel_ms, pass_ms: the call's device events",
            "spread": "median, minimum, maximum over the rounds", "cases": []}
    od = sb.dragon_standin(9, nthreads=16)
    with sb.Scene(od) as big, sb.Scene(sb.torus_d6()) as torus:
        del od
        line["nodes_in"] = [int(big.Length), int(torus.Length)]
        line["triangles"] = [int(big.MeshDevice()), int(torus.MeshDevice())]
        for k in counts:
            line["cases"].append(bench_case([((big, torus)[i & 1], pl) for i, pl in enumerate(placements(k))], big, *line["triangles"]))
            if args.out:                      # (kept as the cases come in: a later case may be cut short)
                with open(args.out, "w") as f:
                    f.write(json.dumps(line) + "\n")
    print(json.dumps(line))


if __name__ == "__main__":
    main()
