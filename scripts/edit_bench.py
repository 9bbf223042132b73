"""Space carving's cost (sdfhip_scene_edit): one brush on cfg-2's 28 M-node scene (dragon_standin(9)) and on
the builder's depth-10 knot scene, centred on the surface point under the cfg-2 camera's central ray; radius (sphere) or half
extent (box) 0.01, 0.05 and 0.2; carve and add.  Per case, the median and minimum of 20 calls after 3 warm-ups: edit_ms (HIP events
around the edit's kernels), scene_ms (the new handle: fused records, lookup grids), total_ms (host clock, the whole call), nodes
visited, blocks added.  Beside them: sdfhip_scene_upload of the same tree from the host (median of 5), and one cfg-2 frame of the
edited and of the original handle -- 20-frame bursts on one stream, alternated, 5 of each, median per frame.

    python scripts/edit_bench.py [--out FILE]          # prints one JSON line (and writes it to FILE)"""
import argparse
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import edit_restatement as er  # noqa: E402
import sdfbox_amd as sb  # noqa: E402

W, H = 1920, 1080
CALLS, WARMUP = 20, 3


def camera():
    cam = sb.Logic(W, H)
    cam.Position = (0.5, 0.5, -0.35); cam.Heading = (-0.2, 0.35)        # cfg-2's camera
    return cam


def frame_ms(scenes, cam, bursts=5, frames=20):
    """per scene: median over `bursts` alternated bursts of `frames` back-to-back frames on one stream (HIP events), per frame"""
    buf = torch.empty((H, W, 4), dtype=torch.float32, device="cuda:0")
    st = torch.cuda.Stream()
    out = {k: [] for k in scenes}
    for _ in range(2):                                                   # warm-up of both
        for s in scenes.values():
            s.DrawDevice(cam, W, H, buf.data_ptr(), stream=st.cuda_stream)
    torch.cuda.synchronize()
    for _ in range(bursts):
        for k, s in scenes.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(st)
            for _ in range(frames):
                s.DrawDevice(cam, W, H, buf.data_ptr(), stream=st.cuda_stream)
            e1.record(st)
            e1.synchronize()
            out[k].append(e0.elapsed_time(e1) / frames)
    return {k: round(statistics.median(v), 4) for k, v in out.items()}


def upload_ms(od, n=5):
    t = []
    for _ in range(n):
        t0 = time.perf_counter()
        s = sb.Scene(od)
        t.append((time.perf_counter() - t0) * 1e3)
        s.close()
    return round(statistics.median(t), 3)


def bench_scene(name, od, scene, cam):
    c = er.surface_point_under(od.Structs, cam.Position, [list(r) for r in cam.State.heading])
    rec = {"scene": name, "nodes": od.Length, "depth": scene.depth, "brush_centre": [round(v, 6) for v in c],
           "upload_ms": upload_ms(od), "cases": []}
    for size in (0.01, 0.05, 0.2):
        for op_name, op in (("carve", sb.EDIT_CARVE), ("add", sb.EDIT_ADD)):
            for brush_name, brush in (("sphere", sb.BRUSH_SPHERE), ("box", sb.BRUSH_BOX)):
                params = (*c, size) if brush == sb.BRUSH_SPHERE else (*c, size, size, size)
                rows = []
                for i in range(WARMUP + CALLS):
                    res, st = scene.Edit([(op, brush, params)], want_stats=True)
                    res.close()
                    if i >= WARMUP:
                        rows.append((st.edit_ms, st.scene_ms, st.total_ms, st.nodes_visited, st.blocks_added))
                a = np.array(rows, dtype=np.float64)
                med, mn = np.median(a, 0), a.min(0)
                rec["cases"].append({"size": size, "op": op_name, "brush": brush_name,
                                     "edit_ms": [round(med[0], 4), round(mn[0], 4)], "scene_ms": [round(med[1], 3), round(mn[1], 3)],
                                     "total_ms": [round(med[2], 3), round(mn[2], 3)], "nodes_visited": int(med[3]),
                                     "blocks_added": int(med[4]), "nodes_out": int(st.nodes_out)})
                print(json.dumps({"scene": name, **rec["cases"][-1]}), file=sys.stderr, flush=True)
    # one cfg-2 frame of the r = 0.05 carve against the original handle
    edited = scene.Edit([(sb.EDIT_CARVE, sb.BRUSH_SPHERE, (*c, 0.05))])
    ms = frame_ms({"original": scene, "edited_r0.05_carve": edited}, cam)
    edited.close()
    rec["frame_ms"] = ms
    return rec


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    cam = camera()
    line = {"what": "sdfhip_scene_edit", "device": torch.cuda.get_device_name(0), "calls": CALLS, "warmup": WARMUP, "scenes": []}
    od = sb.dragon_standin(9, nthreads=16)
    with sb.Scene(od) as scene:
        line["scenes"].append(bench_scene("dragon_standin_d9", od, scene, cam))
    del od
    scene, od = sb.Scene.FromPoints(sb.knot_point_cloud(), 10, want_octdata=True)
    with scene:
        line["scenes"].append(bench_scene("knot_builder_d10", od, scene, cam))
    text = json.dumps(line)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
