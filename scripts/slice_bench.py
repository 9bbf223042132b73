"""What a cross-section costs (sdfhip_scene_slice / sdfhip_scene_slice_device), on cfg-2's 28 M-node scene
(dragon_standin(9)) at level -1: one plane, 100 layers and 1000 layers through the whole cube, along z and along the oblique unit
normal (0.6, 0, 0.8), beside the route it replaces, Scene.Mesh's count + emit of the same scene and level.

  count        the count pass alone (k_slice_count + the chunk scan and the copy of the total): SliceDevice() with no buffer
  count_emit   count, the host's wait for the total, and k_slice_emit into a device buffer that fits: SliceDevice(buffer, capacity, counts)
  host form    Scene.Slice once: its statistics (kernel_ms; total_ms, the whole C call with the copy to the host -- the binding's sort
               by layer is not in it; cells_cut, cells_crossed, the fullest layer)
  mesh         MeshDevice(buffer, capacity) of the same scene: count + emit, 72 bytes per triangle
  bytes        32 per record, against the mesh's

HIP events on the call's stream around each single call, median (and minimum) of REPS calls after WARMUP.  The call waits on the host
for the total between count and emit, so count_emit includes that round trip, as the mesh's does.

    python scripts/slice_bench.py [--out FILE] [--quick]       # prints one JSON line (and writes it to FILE)"""
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
# name -> (normal, [(offset, pitch, layers)]): each stack spans the cube's whole height range along its normal (1 along z, 1.4 oblique)
STACKS = {
    "z": ((0.0, 0.0, 1.0), [(0.5, 0.0, 1), (0.005, 0.01, 100), (0.0005, 0.001, 1000)]),
    "oblique": ((0.6, 0.0, 0.8), [(0.7, 0.0, 1), (0.007, 0.014, 100), (0.0007, 0.0014, 1000)]),
}


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


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--out", default=None)
    ap.add_argument("--quick", action="store_true", help="the z stacks only, no host form")
    args = ap.parse_args()
    st = torch.cuda.Stream()
    od = sb.dragon_standin(9, nthreads=16)
    line = {"what": "sdfhip_scene_slice_device", "device": torch.cuda.get_device_name(0), "reps": REPS, "warmup": WARMUP,
            "scene": "dragon_standin_d9", "nodes": od.Length, "record_bytes": od.Length * 16, "level": -1, "stacks": []}
    with sb.Scene(od) as scene:
        n_tri = scene.MeshDevice()
        buf = torch.empty((max(n_tri, 1), 3, 6), dtype=torch.float32, device="cuda")
        line["mesh"] = {"triangles": n_tri, "output_bytes": n_tri * 72,
                        "count_ms": timed(lambda: scene.MeshDevice(stream=st.cuda_stream), st),
                        "count_emit_ms": timed(lambda: scene.MeshDevice(buf.data_ptr(), n_tri, stream=st.cuda_stream), st)}
        print(json.dumps(line["mesh"]), file=sys.stderr, flush=True)
        del buf
        torch.cuda.empty_cache()
        for name, (normal, stacks) in STACKS.items():
            if args.quick and name != "z":
                continue
            for offset, pitch, layers in stacks:
                kw = dict(normal=normal, offset=offset, pitch=pitch, layers=layers)
                n = scene.SliceDevice(**kw)
                out = torch.empty((max(n, 1), 8), dtype=torch.float32, device="cuda")
                cnt = torch.empty((layers,), dtype=torch.int32, device="cuda")
                rec = {"stack": name, "normal": list(normal), "offset": offset, "pitch": pitch, "layers": layers, "records": n, "output_bytes": n * 32,
                       "count_ms": timed(lambda: scene.SliceDevice(stream=st.cuda_stream, **kw), st),
                       "count_emit_ms": timed(lambda: scene.SliceDevice(out.data_ptr(), n, cnt.data_ptr(), stream=st.cuda_stream, **kw), st)}
                rec["count_emit_over_mesh_count_emit"] = round(rec["count_emit_ms"][0] / line["mesh"]["count_emit_ms"][0], 3)
                rec["mesh_bytes_over_slice_bytes"] = round(n_tri * 72 / max(n * 32, 1), 1)
                del out, cnt
                if not args.quick:
                    segs, starts, stats = scene.Slice(level=-1, **kw)
                    assert len(segs) == n
                    rec["host_form"] = {"kernel_ms": round(stats.kernel_ms, 4), "total_ms": round(stats.total_ms, 4), "cells": stats.cells,
                                        "cells_cut": stats.cells_cut, "cells_crossed": stats.cells_crossed,
                                        "fullest_layer": int((starts[1:] - starts[:-1]).max())}
                    del segs
                line["stacks"].append(rec)
                print(json.dumps(rec), file=sys.stderr, flush=True)
    one = [r for r in line["stacks"] if r["layers"] == 1]
    line["single_plane_faster_than_mesh_count_emit"] = all(r["count_emit_ms"][0] < line["mesh"]["count_emit_ms"][0] for r in one)
    text = json.dumps(line)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
