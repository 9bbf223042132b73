"""The composition's cost (sdfhip_scene_compose) against the route the library offered before it, on cfg-2's
28 M-node scene (dragon_standin(9)) and torus_d6, to depth 9.  K = 2, 8 and 32 instances on a grid of cells in the cube (2 x 2 x 2
cells for K <= 8, 4 x 4 x 4 for K = 32; each instance at 0.9 of its cell, turned differently), in two arrangements: "mixed" (the big
scene and the torus in turn, two handles) and "repeats" (K times the ONE handle of the big scene).  In the same process, per case:
  compose   one Scene.Compose: median, minimum and maximum of CALLS calls after WARMUP of total_ms (host clock, the whole call),
            kernel_ms (HIP events round the levels) and scene_ms; the result's nodes; kernel ms per million samples (samples counts by
            the rule: instances * look-up points)
  chain     K x Scene.Place to depth 9, then K - 1 x Scene.Combine (union) folding them in list order: the sum of the calls'
            total_ms, median, minimum and maximum of CHAIN_CALLS runs after one warm-up, and of the last run the placements' and the
            combinations' shares and the slowest single call of each; the final result's nodes (the trees differ by design: one
            quantisation against two, and the combination keeps every cell either operand had)
and the ratio chain / compose of the medians.

    python scripts/compose_bench.py [--out FILE]          # prints one JSON line (and writes it to FILE)"""
import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import sdfbox_amd as sb  # noqa: E402

CALLS, WARMUP, CHAIN_CALLS, DEPTH = 5, 1, 3, 9
COUNTS = (2, 8, 32)


def spread(values, digits=3):
    a = np.asarray(values, dtype=np.float64)
    return {"median": round(float(np.median(a)), digits), "min": round(float(a.min()), digits), "max": round(float(a.max()), digits)}


def placements(k):
    """k placements on a grid of n^3 cells, n = 2 for k <= 8 and 4 above: instance i at 0.9 of cell i, turned by its index"""
    n = 2 if k <= 8 else 4
    out = []
    for i in range(k):
        cell = (i % n, i // n % n, i // (n * n) % n)
        to = tuple((c + 0.5) / n for c in cell)
        out.append(sb.placement(37.0 * i, 11.0 * i - 40.0, 5.0 * i, 0.9 / n, to=to))
    return out


def compose_once(parts):
    res, st = sb.Scene.Compose(parts, DEPTH, want_stats=True)
    res.close()
    return st


def chain_once(parts):
    """the same assembly by K placements and K - 1 unions; -> (the placements' total_ms, the combinations' total_ms, nodes of the final
    result)"""
    place_ms, combine_ms, acc = [], [], None
    for scene, pl in parts:
        placed, st = scene.Place(*pl, DEPTH, want_stats=True)
        place_ms.append(st.total_ms)
        if acc is None:
            acc = placed
            continue
        joined, cst = acc.Combine(placed, sb.COMBINE_UNION, want_stats=True)
        combine_ms.append(cst.total_ms)
        acc.close()
        placed.close()
        acc = joined
    nodes = int(acc.Length)
    acc.close()
    return place_ms, combine_ms, nodes


def bench_case(name, parts):
    rows, st = [], None
    for i in range(WARMUP + CALLS):
        st = compose_once(parts)
        if i >= WARMUP:
            rows.append((st.total_ms, st.kernel_ms, st.scene_ms))
    t = np.array(rows, dtype=np.float64)
    chain, chain_nodes, parts_of_it = [], 0, None
    for i in range(1 + CHAIN_CALLS):
        place_ms, combine_ms, chain_nodes = chain_once(parts)
        if i >= 1:
            chain.append(sum(place_ms) + sum(combine_ms))
            # (the last run's: where the chain's time goes, and its slowest single call)
            parts_of_it = {"place_ms_sum": round(sum(place_ms), 3), "combine_ms_sum": round(sum(combine_ms), 3),
                           "slowest_place_ms": round(max(place_ms), 3), "slowest_combine_ms": round(max(combine_ms), 3)}
    rec = {"arrangement": name, "instances": len(parts), "distinct_handles": len({id(s) for s, _ in parts}),
           "compose": {"total_ms": spread(t[:, 0]), "kernel_ms": spread(t[:, 1]), "scene_ms": spread(t[:, 2]), "nodes_out": int(st.nodes_out),
                       "depth_out": int(st.depth_out), "samples": int(st.samples),
                       "kernel_ms_per_Msample": round(float(np.median(t[:, 1])) / (int(st.samples) / 1e6), 5)},
           "chain": {"total_ms": spread(chain), "nodes_out": chain_nodes, "calls": 2 * len(parts) - 1, "last_run": parts_of_it},
           "chain_over_compose": round(float(np.median(chain)) / float(np.median(t[:, 0])), 3)}
    print(json.dumps(rec), file=sys.stderr, flush=True)
    return rec


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    line = {"what": "sdfhip_scene_compose", "device": torch.cuda.get_device_name(0), "calls": CALLS, "warmup": WARMUP, "chain_calls": CHAIN_CALLS,
            "depth": DEPTH, "scenes": ["dragon_standin_d9", "torus_d6"], "cases": []}
    od = sb.dragon_standin(9, nthreads=16)
    with sb.Scene(od) as big, sb.Scene(sb.torus_d6()) as torus:
        del od
        line["nodes_in"] = [int(big.Length), int(torus.Length)]
        for k in COUNTS:
            pls = placements(k)
            line["cases"].append(bench_case("mixed", [((big, torus)[i & 1], pl) for i, pl in enumerate(pls)]))
            line["cases"].append(bench_case("repeats", [(big, pl) for pl in pls]))
    text = json.dumps(line)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
