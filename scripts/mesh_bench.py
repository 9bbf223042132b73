"""What surface extraction costs (sdfhip_scene_mesh_device), on cfg-2's 28 M-node scene (dragon_standin(9))
and on the depth-10 knot scene (OctData.SdfGen(knot_point_cloud(), 10)), at level -1 (the leaves) and level 6:

  count        the count pass alone (k_mesh_count + the chunk scan and the 16-byte copy of the total): MeshDevice() with no buffer
  count_emit   count, the host's wait for the total, and k_mesh_emit into a device buffer that fits: MeshDevice(buffer, capacity)
  per second   triangles per second of count_emit; output bytes (72 per triangle)
  against      the time sdfhip_device_bandwidth's read_gbs gives for ONE read of the scene's records (16 bytes per node); the pass reads
               them twice, so 2.0 is the floor of count_emit's ratio and 1.0 of count's
  A/B          (laboratory library) non-temporal instead of plain stores (SDFHIP_MESH_STORE=nt), 8-byte stores only (SDFHIP_MESH_VEC=8)

HIP events on the call's stream around each single call, median (and minimum) of REPS calls after WARMUP.  The call waits on the host
for the total between count and emit, so count_emit includes that round trip.

    python scripts/mesh_bench.py [--out FILE] [--quick]        # prints one JSON line (and writes it to FILE)"""
import argparse
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import torch  # noqa: E402

import sdfbox_amd as sb  # noqa: E402
import sdfbox_amd.lab  # noqa: E402

REPS, WARMUP = 20, 3
LEVELS = (-1, 6)


def timed(call, stream, reps=REPS, warmup=WARMUP):
    """[median, minimum] ms of single calls on `stream`, each between its own pair of HIP events"""
    for _ in range(warmup):
        call()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        call()
        e1.record(stream)
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return [round(statistics.median(ms), 4), round(min(ms), 4)]


def bench_scene(scene, st, one_read_ms, levels=LEVELS):
    out = []
    for level in levels:
        n = scene.MeshDevice(level=level)
        buf = torch.empty((max(n, 1), 3, 6), dtype=torch.float32, device="cuda")
        rec = {"level": level, "triangles": n, "output_bytes": n * 72,
               "count_ms": timed(lambda: scene.MeshDevice(level=level, stream=st.cuda_stream), st),
               "count_emit_ms": timed(lambda: scene.MeshDevice(buf.data_ptr(), n, level=level, stream=st.cuda_stream), st)}
        rec["mtriangles_per_s"] = round(n / rec["count_emit_ms"][0] / 1e3, 1)
        rec["count_over_one_read"] = round(rec["count_ms"][0] / one_read_ms, 2)
        rec["count_emit_over_one_read"] = round(rec["count_emit_ms"][0] / one_read_ms, 2)
        out.append(rec)
        print(json.dumps(rec), file=sys.stderr, flush=True)
        del buf
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--out", default=None)
    ap.add_argument("--quick", action="store_true", help="cfg-2's scene only, no A/B")
    args = ap.parse_args()
    st = torch.cuda.Stream()
    _, _, read_gbs = sb.device_bandwidth(0, 2 << 30, 10)
    line = {"what": "sdfhip_scene_mesh_device", "device": torch.cuda.get_device_name(0), "reps": REPS, "warmup": WARMUP,
            "read_gbs": round(read_gbs, 1), "scenes": []}
    makers = [("dragon_standin_d9", lambda: sb.dragon_standin(9, nthreads=16))]
    if not args.quick:
        makers.append(("knot_d10", lambda: sb.OctData.SdfGen(sb.knot_point_cloud(), 10)))
    for name, make in makers:
        od = make()
        one_read_ms = od.Length * 16 / (read_gbs * 1e6)
        rec = {"scene": name, "nodes": od.Length, "record_bytes": od.Length * 16, "one_read_ms": round(one_read_ms, 4)}
        with sb.Scene(od) as scene:
            rec["depth"] = scene.depth
            rec["levels"] = bench_scene(scene, st, one_read_ms)
            tris, stats = scene.Mesh(6)
            rec["host_form_level_6"] = {"triangles": len(tris), "cells": stats.cells, "cells_cut": stats.cells_cut,
                                        "kernel_ms": round(stats.kernel_ms, 4), "total_ms": round(stats.total_ms, 4)}
        if not args.quick:
            lab = sdfbox_amd.lab.load()
            ab = {}
            with lab.Scene(od) as scene:
                for label, env in (("default", {}), ("non_temporal_stores", {"SDFHIP_MESH_STORE": "nt"}), ("stores_of_8_bytes", {"SDFHIP_MESH_VEC": "8"})):
                    os.environ.update(env)
                    try:
                        ab[label] = bench_scene(scene, st, one_read_ms, levels=(-1,))[0]["count_emit_ms"]
                    finally:
                        for k in env:
                            del os.environ[k]
            rec["ab_laboratory_library_level_-1_count_emit_ms"] = ab
        line["scenes"].append(rec)
        del od
    text = json.dumps(line)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
