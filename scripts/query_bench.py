"""What point and ray queries cost (sdfhip_scene_sample / _raycast / _pick), on cfg-2's 28 M-node scene
(dragon_standin(9)):

  sample_device   1 M and 16 M points in three input orders -- uniform random, random within two leaf scales of the surface, the
                  latter sorted in Morton order -- in Mpoints/s and GB/s of records moved (12 B in, 32 B out per point)
  raycast_device  the 2 073 600 camera rays of cfg-2's 1080p frame, against sdfhip_render_device of that frame measured in the same
                  run, one launch at a time; the ratio
  pick            one pixel through the host call: what a viewer pays per mouse move (host clock)
  A/B             (laboratory library) the same sample and raycast launches with both kernels walking the links
                  (SDFHIP_QUERY_FORM=generic), both looking the grid up (=grid; the default is sample walking, the march on the
                  grid), and with plain instead of non-temporal stores (SDFHIP_QUERY_STORE=plain)

_device calls: HIP events around each single launch, median (and minimum) of REPS launches after WARMUP; host calls: the host clock.

    python scripts/query_bench.py [--out FILE] [--quick]        # prints one JSON line (and writes it to FILE)"""
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
import query_restatement as qr  # noqa: E402
import sdfbox_amd as sb  # noqa: E402
import sdfbox_amd.lab  # noqa: E402

W, H = 1920, 1080
REPS, WARMUP = 20, 3


def camera():
    cam = sb.Logic(W, H)
    cam.Position = (0.5, 0.5, -0.35); cam.Heading = (-0.2, 0.35)        # cfg-2's camera
    return cam


def timed(launch, stream, reps=REPS, warmup=WARMUP):
    """[median, minimum] ms of single launches on `stream`, each between its own pair of HIP events"""
    for _ in range(warmup):
        launch()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        launch()
        e1.record(stream)
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return [round(statistics.median(ms), 4), round(min(ms), 4)]


def morton_order(p):
    q = np.clip((p * 1024.0).astype(np.int64), 0, 1023)
    code = np.zeros(len(p), np.int64)
    for b in range(10):
        for a in range(3):
            code |= ((q[:, a] >> b) & 1) << (3 * b + a)
    return np.argsort(code, kind="stable")


def point_orders(od, n, rng):
    centres, scale = er.deepest_leaf_centres(od.Structs)
    near = (centres[rng.integers(0, len(centres), n)] + rng.uniform(-2 * scale, 2 * scale, size=(n, 3))).astype(np.float32)
    return {"uniform": rng.random((n, 3)).astype(np.float32), "near_surface": near, "near_surface_morton": near[morton_order(near)]}


def bench_sample(scene, od, sizes, st):
    rng = np.random.default_rng(1)
    out = []
    for n in sizes:
        d_out = torch.empty((n, 32), dtype=torch.uint8, device="cuda")
        for order, pts in point_orders(od, n, rng).items():
            d_in = torch.from_numpy(pts).cuda()
            ms = timed(lambda: scene.SampleDevice(d_in.data_ptr(), n, d_out.data_ptr(), stream=st.cuda_stream), st)
            out.append({"points": n, "order": order, "ms": ms, "mpoints_per_s": round(n / ms[0] / 1e3, 1), "gb_per_s": round(n * 44 / ms[0] / 1e6, 1)})
            print(json.dumps(out[-1]), file=sys.stderr, flush=True)
            del d_in
        del d_out
    return out


def camera_ray_records(od, cam):
    ys, xs = np.mgrid[0:H, 0:W]
    pixels = np.stack([xs.ravel(), ys.ravel()], 1)
    o, d = qr.camera_rays(od.Structs[:1], od.Values[:1], cam.State, pixels)
    rays = np.zeros(len(o), np.dtype(sb.Ray)); rays["origin"] = o; rays["dir"] = d
    return rays


def bench_rays(scene, rays, cam, st):
    n = len(rays)
    d_rays = torch.from_numpy(rays.view(np.uint8).reshape(-1, 32)).cuda()
    d_hits = torch.empty((n, 48), dtype=torch.uint8, device="cuda")
    frame = torch.empty((H, W, 4), dtype=torch.float32, device="cuda")
    m, lim = cam.State.margin, cam.State.limit
    rec = {"rays": n,
           "frame_ms": timed(lambda: scene.DrawDevice(cam, W, H, frame.data_ptr(), stream=st.cuda_stream), st),
           "raycast_ms": timed(lambda: scene.RaycastDevice(d_rays.data_ptr(), n, m, lim, d_hits.data_ptr(), stream=st.cuda_stream), st)}
    rec["frame_ms_again"] = timed(lambda: scene.DrawDevice(cam, W, H, frame.data_ptr(), stream=st.cuda_stream), st)
    rec["raycast_over_frame"] = round(rec["raycast_ms"][0] / rec["frame_ms"][0], 3)
    rec["mrays_per_s"] = round(n / rec["raycast_ms"][0] / 1e3, 1)
    rec["bytes_moved"] = {"raycast": n * 80, "frame": n * 16}
    return rec


def bench_pick(scene, cam, calls=200):
    px = np.array([[W // 2, H // 2]], dtype=np.uint32)
    for _ in range(10):
        hit = scene.Pick(cam, px)
    us = []
    for _ in range(calls):
        t0 = time.perf_counter()
        scene.Pick(cam, px)
        us.append((time.perf_counter() - t0) * 1e6)
    return {"pixels": 1, "host_us": [round(statistics.median(us), 1), round(min(us), 1)], "status": int(hit["status"][0]), "steps": int(hit["steps"][0])}


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--out", default=None)
    ap.add_argument("--quick", action="store_true", help="1 M points only, no A/B")
    args = ap.parse_args()
    cam = camera()
    st = torch.cuda.Stream()
    od = sb.dragon_standin(9, nthreads=16)
    line = {"what": "sdfhip_scene_sample / _raycast / _pick", "device": torch.cuda.get_device_name(0), "scene": "dragon_standin_d9",
            "nodes": od.Length, "reps": REPS, "warmup": WARMUP}
    rays = camera_ray_records(od, cam)
    with sb.Scene(od) as scene:
        line["grid"] = {"coarse_level": scene.top_grid_level, "depth": scene.depth}
        line["sample_device"] = bench_sample(scene, od, (1_000_000,) if args.quick else (1_000_000, 16_000_000), st)
        line["raycast_device"] = bench_rays(scene, rays, cam, st)
        line["pick_one_pixel"] = bench_pick(scene, cam)
    if not args.quick:
        lab = sdfbox_amd.lab.load()
        ab = {}
        with lab.Scene(od) as scene:
            for label, env in (("default", {}), ("both_walk_links", {"SDFHIP_QUERY_FORM": "generic"}), ("both_grid", {"SDFHIP_QUERY_FORM": "grid"}),
                               ("default_plain_stores", {"SDFHIP_QUERY_STORE": "plain"})):
                os.environ.update(env)
                try:
                    ab[label] = {"sample_device": bench_sample(scene, od, (1_000_000,), st), "raycast_ms": bench_rays(scene, rays, cam, st)["raycast_ms"]}
                finally:
                    for k in env:
                        del os.environ[k]
        line["ab_laboratory_library"] = ab
    line["scatter_grid_ab"] = "not run"
    text = json.dumps(line)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
