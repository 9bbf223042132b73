"""The cost of volumes in and out (sdfhip_volume_build_device, sdfhip_scene_volume_device) on cfg-2's
28 M-node scene (dragon_standin(9)), each beside its peer:
  out    Scene.Volume into a device tensor -- the depth-9 lattice (513^3) as float32 and as float16, and the 257^3 lattice -- against
         Scene.SampleDevice on the same number of points in the same order (torch events round the launch, the stream waited for)
  in     Scene.FromVolume of each of those tensors to depth 9, 8 and 7 (the last small enough that no build's arrays grow) --
         check_ms (the finite check on its own), kernel_ms, scene_ms, total_ms -- against Scene.Place at the identity to the same depth: the same level passes, with a tree look-up per
         point where the volume has eight loads; compared per node of result
Median, minimum and maximum of CALLS calls after WARMUP warm-ups (three: on a machine that has not run the library before, the first
calls' large allocations take a hundred milliseconds and more); every ratio is volume over peer, with both raw times beside it.

    python scripts/volume_bench.py [--out FILE]          # prints one JSON line (and writes it to FILE)"""
import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import sdfbox_amd as sb  # noqa: E402

CALLS, WARMUP = 5, 3
LATTICES = (("513^3 float32", 9, torch.float32), ("513^3 float16", 9, torch.float16), ("257^3 float32", 8, torch.float32))
BUILD_DEPTHS = (9, 8, 7)


def spread(values, digits=4):
    a = np.asarray(values, dtype=np.float64)
    return {"median": round(float(np.median(a)), digits), "min": round(float(a.min()), digits), "max": round(float(a.max()), digits)}


def timed(launch):
    """milliseconds of launch() on the current torch stream, CALLS times after WARMUP"""
    t = []
    for i in range(WARMUP + CALLS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        launch()
        b.record()
        b.synchronize()
        if i >= WARMUP:
            t.append(a.elapsed_time(b))
    return t


def lattice_xyz(shape, origin, spacing):
    """the lattice's positions (n, 3) float32 on the device, x fastest: the order Volume's threads take them in"""
    nz, ny, nx = shape
    ax = [origin[a] + torch.arange(n, dtype=torch.float32, device="cuda") * np.float32(spacing) for a, n in ((0, nx), (1, ny), (2, nz))]
    p = torch.empty((nz, ny, nx, 3), dtype=torch.float32, device="cuda")
    p[..., 0] = ax[0][None, None, :]
    p[..., 1] = ax[1][None, :, None]
    p[..., 2] = ax[2][:, None, None]
    return p.reshape(-1, 3)


def bench_out(scene, name, depth, dtype):
    lattice = sb.lattice_of_depth(depth)
    out = torch.empty(lattice[0], dtype=dtype, device="cuda")
    t_volume = timed(lambda: scene.Volume(*lattice, out=out))
    n = out.numel()
    xyz = lattice_xyz(*lattice)
    probes = torch.empty((n, 8), dtype=torch.float32, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    t_sample = timed(lambda: scene.SampleDevice(xyz.data_ptr(), n, probes.data_ptr(), stream=stream))
    same = bool(torch.equal(probes[:, 0].reshape(lattice[0]).to(dtype), out))
    del xyz, probes
    v, s = float(np.median(t_volume)), float(np.median(t_sample))
    rec = {"lattice": name, "elements": n, "volume_ms": spread(t_volume), "sample_device_ms": spread(t_sample),
           "volume_over_sample": round(v / s, 3), "Gelements_per_s": round(n / v / 1e6, 2), "equals_the_samples": same}
    print(json.dumps(rec), file=sys.stderr, flush=True)
    return rec, out


def bench_place(scene, depth):
    rows, st = [], None
    for i in range(WARMUP + CALLS):
        res, st = scene.Place(np.eye(3, dtype=np.float32), 1.0, (0, 0, 0), depth, want_stats=True)
        res.close()
        if i >= WARMUP:
            rows.append((st.kernel_ms, st.scene_ms, st.total_ms))
    t = np.array(rows, dtype=np.float64)
    rec = {"depth": depth, "nodes_out": int(st.nodes_out), "samples": int(st.samples), "kernel_ms": spread(t[:, 0]), "scene_ms": spread(t[:, 1]),
           "total_ms": spread(t[:, 2])}
    print(json.dumps({"place_identity": rec}), file=sys.stderr, flush=True)
    return rec


def bench_in(name, grid, lattice, depth, place):
    rows, st = [], None
    for i in range(WARMUP + CALLS):
        res, st = sb.Scene.FromVolume(grid, lattice[1], lattice[2], depth=depth, want_stats=True)
        res.close()
        if i >= WARMUP:
            rows.append((st.check_ms, st.kernel_ms, st.scene_ms, st.total_ms))
    t = np.array(rows, dtype=np.float64)
    k, pk = float(np.median(t[:, 1])), place["kernel_ms"]["median"]
    rec = {"grid": name, "depth": depth, "nodes_out": int(st.nodes_out), "samples": int(st.samples), "check_ms": spread(t[:, 0]),
           "kernel_ms": spread(t[:, 1]), "scene_ms": spread(t[:, 2]), "total_ms": spread(t[:, 3]),
           "place_nodes_out": place["nodes_out"], "place_kernel_ms": pk,
           "ns_per_node": round(k * 1e6 / int(st.nodes_out), 4), "place_ns_per_node": round(pk * 1e6 / place["nodes_out"], 4),
           "kernel_per_node_over_place": round((k / int(st.nodes_out)) / (pk / place["nodes_out"]), 3)}
    print(json.dumps(rec), file=sys.stderr, flush=True)
    return rec


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    line = {"what": "sdfhip_volume_build_device / sdfhip_scene_volume_device", "device": torch.cuda.get_device_name(0), "calls": CALLS,
            "warmup": WARMUP, "scene": "dragon_standin_d9", "out": [], "in": []}
    od = sb.dragon_standin(9, nthreads=16)
    with sb.Scene(od) as big:
        del od
        line["nodes"], line["top_grid_level"] = int(big.Length), int(big.top_grid_level)
        places = {d: bench_place(big, d) for d in BUILD_DEPTHS}
        line["place_identity"] = [places[d] for d in BUILD_DEPTHS]
        for name, depth, dtype in LATTICES:
            rec, grid = bench_out(big, name, depth, dtype)
            line["out"].append(rec)
            for d in BUILD_DEPTHS:
                line["in"].append(bench_in(name, grid, sb.lattice_of_depth(depth), d, places[d]))
            del grid
    text = json.dumps(line)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
