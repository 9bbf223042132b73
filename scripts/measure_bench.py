"""What the measure costs (sdfhip_scene_measure), on cfg-2's 28 M-node scene (dragon_standin(9)), at level -1
(the leaves) and level 6:

  kernel_ms    HIP events around k_measure_cells and the k_measure_fold rounds (sdfhip_measure.kernel_ms)
  total_ms     the host's clock over the whole call: the memset, the kernels, the 200-byte copy of the result, the wait
  against      the time sdfhip_device_bandwidth's read_gbs gives for ONE read of the scene's records (16 bytes per node), and the
               mesh's figures on the same scene from profiles/mesh_bench.json: its count pass is the floor (one read of the records),
               count + emit followed by a reduction on the host is what a caller without this call would do
  bytes        what the pass moves by construction: one read of the records, the partials written and read (136 bytes per 1024 nodes,
               and 1/1024 of that per further round), and the parent links the climb touches -- counted as the distinct internal
               nodes' 8 bytes once (siblings share every ancestor, so a wave's climb loads one line per level, not one per lane)

Median (minimum .. maximum) of REPS calls after WARMUP.  Recorded, not gated.

    python scripts/measure_bench.py [--out FILE]        # prints one JSON line (and writes it to FILE)"""
import argparse
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import torch  # noqa: E402

import sdfbox_amd as sb  # noqa: E402

REPS, WARMUP = 10, 2
LEVELS = (-1, 6)


def spread(values):
    return [round(statistics.median(values), 4), round(min(values), 4), round(max(values), 4)]


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    _, _, read_gbs = sb.device_bandwidth(0, 2 << 30, 10)
    od = sb.dragon_standin(9, nthreads=16)
    one_read_ms = od.Length * 16 / (read_gbs * 1e6)
    internal = int((od.Structs[:, 1] >= 0).sum())
    partial_bytes = 2 * 136 * ((od.Length + 1023) // 1024) * (1 + 1 / 1024)
    line = {"what": "sdfhip_scene_measure", "device": torch.cuda.get_device_name(0), "reps": REPS, "warmup": WARMUP, "read_gbs": round(read_gbs, 1),
            "scene": "dragon_standin_d9", "nodes": od.Length, "record_bytes": od.Length * 16, "one_read_ms": round(one_read_ms, 4),
            "bytes_moved_over_one_read": round((od.Length * 16 + partial_bytes + internal * 8) / (od.Length * 16), 3),
            "mesh_bench_parent_commit_ms": {"count": 0.14, "count_emit": 2.2}, "levels": []}
    try:
        with open(os.path.join(REPO, "profiles", "mesh_bench.json")) as f:
            mesh = json.loads(f.readline())["scenes"][0]["levels"][0]
        line["mesh_bench_parent_commit_ms"] = {"count": mesh["count_ms"][0], "count_emit": mesh["count_emit_ms"][0]}
    except (OSError, KeyError, IndexError, ValueError):
        pass
    with sb.Scene(od) as scene:
        for level in LEVELS:
            for _ in range(WARMUP):
                scene.Measure(level)
            runs = [scene.Measure(level) for _ in range(REPS)]
            m = runs[-1]
            rec = {"level": level, "kernel_ms": spread([r.kernel_ms for r in runs]), "total_ms": spread([r.total_ms for r in runs]),
                   "cells": m.cells, "cells_cut": m.cells_cut, "cells_inside": m.cells_inside, "volume": m.volume, "area": m.area,
                   "same_bits_every_call": len({(r.volume, r.area, tuple(r.moment1), tuple(r.moment2)) for r in runs}) == 1}
            rec["kernel_over_one_read"] = round(rec["kernel_ms"][0] / one_read_ms, 2)
            rec["kernel_over_mesh_count"] = round(rec["kernel_ms"][0] / line["mesh_bench_parent_commit_ms"]["count"], 2)
            line["levels"].append(rec)
            print(json.dumps(rec), file=sys.stderr, flush=True)
    text = json.dumps(line)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
