"""The clash check (sdfhip_instances_clash) against the route the library offered before it, on the assemblies
of instances_bench.py: cfg-2's 28 M-node scene (dragon_standin(9)) and torus_d6 in turn, compose_bench.py's "mixed" arrangements of
K = 2, 8 and 32 instances, on the unit cube's lattice at depth 7 and 8 (2 M and 16.8 M points).  In the same process, per K and depth,
the variants alternate inside every one of CALLS rounds after WARMUP; each figure is the median, minimum and maximum over the rounds:
  clash / clash_no_skip   one Scene.ClashParts with the exact skip on / with every instance looked up at every point (the same bytes,
                          asserted here once): call_ms = host clock round the synchronous call, kernel_ms = the call's own device
                          events round its two kernels (sdfhip_clash_stats.kernel_ms), lookups_per_point from its stats
  route                   what a user had: K single-instance Scene.SamplePartsDevice calls on the same lattice (each writes a 32-byte
                          probe per point and takes the six taps of a gradient nobody asked for), then the pairing in torch on the
                          device -- only the K x K matrix of shared-point COUNTS, by exact fp32 products over chunks of 2^20 points;
                          the witness, the bounds and the sums the call returns are not computed.  Host clock to the last synchronise;
                          the counts are asserted equal to the call's once
These figures are recorded, not gated.

    python scripts/clash_bench.py [--out FILE]          # prints one JSON line (and writes it to FILE)"""
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
from compose_bench import COUNTS, placements, spread  # noqa: E402

CALLS, WARMUP = 5, 1
DEPTHS = (7, 8)
CHUNK = 1 << 20


def lattice_points(depth):
    """(8^d, 3) float32 on the device, in linear-index order: (i + 0.5) * 2^-d, exact -- the call's points on the unit cube"""
    n = 1 << depth
    c = (torch.arange(n, dtype=torch.float32, device="cuda") + 0.5) * (2.0 ** -depth)
    z, y, x = torch.meshgrid(c, c, c, indexing="ij")
    return torch.stack([x.reshape(-1), y.reshape(-1), z.reshape(-1)], 1).contiguous()


def route_counts(parts, pts, probes):
    """K x K int64 matrix of shared-point counts by the route: one SamplePartsDevice per part, then the pairing in torch"""
    n, st = len(pts), torch.cuda.current_stream().cuda_stream
    inside = torch.empty((len(parts), n), dtype=torch.bool, device="cuda")
    for k, part in enumerate(parts):
        sb.Scene.SamplePartsDevice([(part[0], part[1])], pts.data_ptr(), n, probes.data_ptr(), stream=st)
        inside[k] = probes.view(torch.float32)[:, 0] < 0
    counts = torch.zeros((len(parts), len(parts)), dtype=torch.int64, device="cuda")
    for at in range(0, n, CHUNK):
        c = inside[:, at:at + CHUNK].float()
        counts += (c @ c.T).long()
    torch.cuda.synchronize()
    return counts


def bench_case(parts, depth, pts, probes):
    K = len(parts)
    on, st_on = sb.Scene.ClashParts(parts, depth=depth)
    off, st_off = sb.Scene.ClashParts(parts, depth=depth, skip=False)
    same = on.tobytes() == off.tobytes()
    assert same, f"K = {K}, depth {depth}: the records with and without the skip differ"
    counts = route_counts(parts, pts, probes).cpu().numpy()
    want = np.zeros((K, K), np.int64)
    want[on["a"], on["b"]] = on["points"]
    agrees = bool((np.triu(counts, 1) == want).all())
    assert agrees, f"K = {K}, depth {depth}: the route counts other points than the call"
    t = {"clash": ([], []), "clash_no_skip": ([], []), "route": ([], [])}
    for i in range(WARMUP + CALLS):
        for what in t:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            if what == "route":
                route_counts(parts, pts, probes)
                kernel = float("nan")
            else:
                kernel = sb.Scene.ClashParts(parts, depth=depth, skip=what == "clash")[1].kernel_ms
            torch.cuda.synchronize()
            if i >= WARMUP:
                t[what][0].append((time.perf_counter() - t0) * 1e3)
                t[what][1].append(kernel)
    med = {what: float(np.median(v[0])) for what, v in t.items()}
    rec = {"arrangement": "mixed", "instances": K, "depth": depth, "points": int(st_on.points), "pairs": int(len(on)),
           "shared_points": int(on["points"].sum()), "skip_on_and_off_same_bytes": same, "route_counts_agree": agrees,
           "clash_call_ms": spread(t["clash"][0]), "clash_kernel_ms": spread(t["clash"][1]),
           "clash_no_skip_call_ms": spread(t["clash_no_skip"][0]), "clash_no_skip_kernel_ms": spread(t["clash_no_skip"][1]),
           "route_ms": spread(t["route"][0]),
           "lookups_per_point": round(st_on.lookups / st_on.points, 4), "lookups_per_point_no_skip": round(st_off.lookups / st_off.points, 4),
           "blocks_looked_fraction": round(st_on.blocks_looked / st_on.blocks, 4),
           "no_skip_over_skip": round(med["clash_no_skip"] / med["clash"], 3), "route_over_clash": round(med["route"] / med["clash"], 2)}
    print(json.dumps(rec), file=sys.stderr, flush=True)
    return rec


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    line = {"what": "sdfhip_instances_clash", "device": torch.cuda.get_device_name(0), "calls": CALLS, "warmup": WARMUP, "depths": list(DEPTHS),
            "scenes": ["dragon_standin_d9", "torus_d6"], "clock": "host, round a synchronous call; kernel_ms: the call's device events",
            "spread": "median, minimum, maximum over the rounds; the variants alternate inside a round", "cases": []}
    od = sb.dragon_standin(9, nthreads=16)
    with sb.Scene(od) as big, sb.Scene(sb.torus_d6()) as torus:
        del od
        line["nodes_in"] = [int(big.Length), int(torus.Length)]
        for depth in DEPTHS:
            pts = lattice_points(depth)
            probes = torch.empty((len(pts), 32), dtype=torch.uint8, device="cuda")
            for k in COUNTS:
                line["cases"].append(bench_case([((big, torus)[i & 1], pl) for i, pl in enumerate(placements(k))], depth, pts, probes))
            del pts, probes
    text = json.dumps(line)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
