"""What the mesh builder costs (sdfhip_trimesh_build), on the level-6 mesh of cfg-2's 28 M-node scene
(dragon_standin(9): 299 256 triangles) and on the torus mesh (torus_d6 at its leaves: 31 880 triangles), at depths 8, 9 and 10:

  per run      build_ms (HIP events round the build's kernels), scene_ms (the handle: fused records, grids), total_ms (host clock, the
               whole call), nodes, candidate entries
  against      sdfhip_sdfgen_scene on the same mesh's vertices at the same depth, in the same run: the ratio of the total times.  It
               answers a different question (nearest point of a cloud, scaled to fill the cube), so the ratio is reported, not held
  pruning A/B  (laboratory library) the same build with SDFHIP_TRI_PRUNE=0 -- every block keeps every record -- on the torus mesh at
               depth 6, where brute force still ends in seconds; alternating with the pruned build of the same library
  headline     cfg-2's frame time (1080p, the default kernel) in the same run: the builder must not move it

Median (and minimum) of REPS calls after WARMUP; every call ends in the library's own stream synchronisation.

    python scripts/trimesh_bench.py [--out FILE] [--quick]      # prints one JSON line (and writes it to FILE)"""
import argparse
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import sdfbox_amd as sb  # noqa: E402
import sdfbox_amd.lab  # noqa: E402

REPS, WARMUP = 20, 3
DEPTHS = (8, 9, 10)


def med(xs):
    return [round(statistics.median(xs), 4), round(min(xs), 4)]


def bench_build(lib, mesh, depth, reps=REPS, warmup=WARMUP):
    rows = []
    for i in range(warmup + reps):
        scene, st = mesh.Build(depth, want_stats=True)
        scene.close()
        if i >= warmup:
            rows.append(st)
    return {"depth": depth, "nodes": rows[0].nodes, "levels": rows[0].levels, "records": rows[0].records,
            "candidate_entries": rows[0].candidate_entries, "build_ms": med([r.build_ms for r in rows]),
            "scene_ms": med([r.scene_ms for r in rows]), "total_ms": med([r.total_ms for r in rows])}


def bench_points(verts6, depth, reps=REPS, warmup=WARMUP):
    ms = []
    for i in range(warmup + reps):
        scene, st = sb.Scene.FromPoints(verts6, depth, want_stats=True)
        scene.close()
        if i >= warmup:
            ms.append(st.total_ms)
    return {"nodes": st.nodes, "total_ms": med(ms)}


def frame_ms(scene, reps=200):
    cam = sb.Logic(1920, 1080)
    cam.Position = (0.5, 0.5, 0.1)
    out = torch.empty((1080, 1920, 4), dtype=torch.float32, device="cuda")
    for _ in range(20):
        scene.DrawDevice(cam, 1920, 1080, out.data_ptr())
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        scene.DrawDevice(cam, 1920, 1080, out.data_ptr())
    e1.record()
    e1.synchronize()
    return round(e0.elapsed_time(e1) / reps, 4)


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--out", default=None)
    ap.add_argument("--quick", action="store_true", help="5 calls after 1, depth 8 only")
    args = ap.parse_args()
    reps, warmup = (5, 1) if args.quick else (REPS, WARMUP)
    depths = (8,) if args.quick else DEPTHS
    line = {"what": "sdfhip_trimesh_build", "device": torch.cuda.get_device_name(0), "reps": reps, "warmup": warmup, "meshes": []}
    dragon = sb.dragon_standin(9, nthreads=16)
    with sb.Scene(dragon) as scene:
        line["cfg2_frame_ms_before"] = frame_ms(scene)
        soups = [("dragon_standin_d9_level6", scene.Mesh(6, want_stats=False))]
    with sb.Scene(sb.torus_d6()) as scene:
        soups.append(("torus_d6_leaves", scene.Mesh(-1, want_stats=False)))
    for name, soup in soups:
        rec = {"mesh": name, "triangles": len(soup), "runs": []}
        with sb.TriMesh.FromMesh(soup) as mesh:
            rec.update(records=mesh.n_records, dropped=mesh.n_dropped, open_edges=mesh.open_edges)
            for depth in depths:
                run = bench_build(sb, mesh, depth, reps, warmup)
                pts = bench_points(soup.reshape(-1, 6), depth, reps, warmup)
                run["sdfgen_scene_total_ms"] = pts["total_ms"]
                run["sdfgen_scene_nodes"] = pts["nodes"]
                run["total_over_sdfgen_scene"] = round(run["total_ms"][0] / pts["total_ms"][0], 2)
                rec["runs"].append(run)
                print(json.dumps(run), file=sys.stderr, flush=True)
        line["meshes"].append(rec)
    # the pruning A/B: the laboratory library against itself, alternating
    lab = sdfbox_amd.lab.load()
    ab_depth = 6
    with lab.TriMesh.FromMesh(soups[1][1]) as mesh:
        rows = {"pruned": [], "brute": []}
        for i in range(warmup + reps):
            for what in ("pruned", "brute"):
                if what == "brute":
                    os.environ["SDFHIP_TRI_PRUNE"] = "0"
                try:
                    scene, st = mesh.Build(ab_depth, want_stats=True)
                finally:
                    os.environ.pop("SDFHIP_TRI_PRUNE", None)
                scene.close()
                if i >= warmup:
                    rows[what].append(st)
        line["prune_ab"] = {"mesh": soups[1][0], "depth": ab_depth, "nodes": rows["pruned"][0].nodes,
                            **{k: {"build_ms": med([r.build_ms for r in v]), "candidate_entries": v[0].candidate_entries} for k, v in rows.items()}}
        line["prune_ab"]["brute_over_pruned"] = round(line["prune_ab"]["brute"]["build_ms"][0] / line["prune_ab"]["pruned"]["build_ms"][0], 2)
    with sb.Scene(dragon) as scene:
        line["cfg2_frame_ms_after"] = frame_ms(scene)
    text = json.dumps(line)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
