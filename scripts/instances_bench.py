"""An assembly drawn without baking (sdfhip_instances_*) against the route the library offered before it, on
cfg-2's 28 M-node scene (dragon_standin(9)) and torus_d6: compose_bench.py's "mixed" arrangements of K = 2, 8 and 32 instances (the
big scene and the torus in turn, on a grid of cells, each turned differently), a 1920 x 1080 frame from the default camera.  In the
same process, per K, each the median, minimum and maximum of CALLS calls after WARMUP, host clock round a call that has waited for
its stream:
  draw_parts           one Scene.DrawPartsDevice, the exact skip on
  draw_parts_no_skip   the same with every instance looked up at every point (INSTANCES_NO_SKIP): the same bytes (asserted here once)
  compose_then_draw    the route that existed: one Scene.Compose to depth 9, then one DrawDevice frame of the result, until that frame
                       is complete (freeing the composed scene afterwards is outside the clock); and the two parts' medians;
                       `resident_frame` is that frame alone, once the composition exists
  pick_one_pixel       Scene.PickParts of the frame's centre pixel
These figures are recorded, not gated.

    python scripts/instances_bench.py [--out FILE]          # prints one JSON line (and writes it to FILE)"""
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
from compose_bench import COUNTS, DEPTH, placements, spread  # noqa: E402

CALLS, WARMUP = 5, 1
W, H = 1920, 1080


def timed(call, after=None):
    """host milliseconds of CALLS calls after WARMUP; each call returns with nothing in flight.  after: what tidies up behind a call,
    outside the clock"""
    out = []
    for i in range(WARMUP + CALLS):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        call()
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        if after:
            after()
        if i >= WARMUP:
            out.append((t1 - t0) * 1e3)
    return out


def bench_case(parts, cam, buf, other):
    ptr, st = buf.data_ptr(), torch.cuda.current_stream().cuda_stream
    sb.Scene.DrawPartsDevice(parts, cam, W, H, ptr, stream=st)
    sb.Scene.DrawPartsDevice(parts, cam, W, H, other.data_ptr(), stream=st, skip=False)
    same = bool(torch.equal(buf.view(torch.int32), other.view(torch.int32)))
    assert same, f"K = {len(parts)}: the frames with and without the skip differ"
    steps = float(buf[..., 3].mean())
    sky = float((buf[..., 2] == 0.2).float().mean())
    on = timed(lambda: sb.Scene.DrawPartsDevice(parts, cam, W, H, ptr, stream=st))
    off = timed(lambda: sb.Scene.DrawPartsDevice(parts, cam, W, H, ptr, stream=st, skip=False))
    compose_ms, frame_ms, made = [], [], []

    def route():
        t0 = time.perf_counter()
        res = sb.Scene.Compose(parts, DEPTH)
        t1 = time.perf_counter()
        res.DrawDevice(cam, W, H, ptr, stream=st)
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        made.append(res)
        compose_ms.append((t1 - t0) * 1e3)
        frame_ms.append((t2 - t1) * 1e3)
    both = timed(route, after=lambda: made.pop().close())       # (freeing the composed scene is not part of the time to the screen)
    with sb.Scene.Compose(parts, DEPTH) as res:
        resident = timed(lambda: res.DrawDevice(cam, W, H, ptr, stream=st))
        nodes = int(res.Length)
    pick = timed(lambda: sb.Scene.PickParts(parts, cam, [[W // 2, H // 2]]))
    hit = sb.Scene.PickParts(parts, cam, [[W // 2, H // 2]])[0]
    rec = {"arrangement": "mixed", "instances": len(parts), "skip_on_and_off_same_bytes": same, "mean_steps_per_pixel": round(steps, 2),
           "sky_fraction": round(sky, 4),
           "draw_parts_ms": spread(on), "draw_parts_no_skip_ms": spread(off), "no_skip_over_skip": round(float(np.median(off) / np.median(on)), 3),
           "compose_then_draw_ms": spread(both), "of_it_compose_ms": spread(compose_ms[WARMUP:]), "of_it_first_frame_ms": spread(frame_ms[WARMUP:]),
           "composed_nodes": nodes, "resident_frame_ms": spread(resident),
           "compose_then_draw_over_draw_parts": round(float(np.median(both) / np.median(on)), 3),
           "draw_parts_over_resident_frame": round(float(np.median(on) / np.median(resident)), 2),
           "pick_one_pixel_ms": spread(pick), "picked": {"status": int(hit["status"]), "instance": int(hit["instance"]), "steps": int(hit["steps"])}}
    print(json.dumps(rec), file=sys.stderr, flush=True)
    return rec


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    line = {"what": "sdfhip_instances_render_device / sdfhip_instances_pick", "device": torch.cuda.get_device_name(0), "calls": CALLS, "warmup": WARMUP,
            "frame": [W, H], "compose_depth": DEPTH, "scenes": ["dragon_standin_d9", "torus_d6"], "clock": "host, round a synchronous call", "cases": []}
    cam = sb.Logic(W, H)
    buf = torch.zeros((H, W, 4), dtype=torch.float32, device="cuda")
    other = torch.zeros_like(buf)
    od = sb.dragon_standin(9, nthreads=16)
    with sb.Scene(od) as big, sb.Scene(sb.torus_d6()) as torus:
        del od
        line["nodes_in"] = [int(big.Length), int(torus.Length)]
        for k in COUNTS:
            line["cases"].append(bench_case([((big, torus)[i & 1], pl) for i, pl in enumerate(placements(k))], cam, buf, other))
    text = json.dumps(line)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
