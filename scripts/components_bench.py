"""The components of a scene (sdfhip_scene_components) against the only route the library offered before it,
on cfg-2's 28 M-node scene (dragon_standin(9)) and on that scene after a carve (a ball of radius 0.2 round the cube's centre taken
out with Scene.Edit), on the unit cube's lattice at depth 7, 8 and 9 (2 M, 16.8 M and 134 M points).  In the same process, per scene
and depth, CALLS rounds after WARMUP; each figure is the median, minimum and maximum over the rounds:
  components / components_labels   one Scene.Components without / with the labels copied to the host: call_ms = host clock round the
                                   synchronous call, kernel_ms = the call's own device events round its kernels
                                   (sdfhip_components_stats.kernel_ms)
  components_device                Scene.ComponentsDevice with the labels left in a torch tensor
  route_torch                      what a user had: Scene.Volume into a torch tensor on the same centres (the values the call's
                                   "inside" reads), then min-label propagation over the six shifts with pointer jumping in torch on the
                                   device until nothing changes, then the components counted (torch.unique of the labels); no record is
                                   computed.  Host clock to the last synchronise; the count is asserted equal to the call's once
  route_host                       Scene.Volume to the host, then scipy.ndimage.label of both phases (where scipy imports; once per
                                   scene and depth, not CALLS times: it takes seconds); the count is asserted equal to the call's
These figures are recorded, not gated.

    python scripts/components_bench.py [--out FILE]          # prints one JSON line (and writes it to FILE)
    python scripts/components_bench.py --profile DEPTH       # ten calls with labels on the carved scene and nothing else: the run
                                                             # a kernel trace is taken round (the per-kernel split)"""
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
from compose_bench import spread  # noqa: E402

CALLS, WARMUP = 5, 1
DEPTHS = (7, 8, 9)
CARVE = [(sb.EDIT_CARVE, sb.BRUSH_SPHERE, (0.5, 0.5, 0.5, 0.2))]


def centres(depth):
    """Scene.Volume's arguments for the call's points on the unit cube: (i + 0.5) * 2^-d along each axis, exact"""
    n, pitch = 1 << depth, 2.0 ** -depth
    return (n, n, n), (pitch / 2,) * 3, pitch


def route_torch(scene, depth, values):
    """the number of components by the route on the device"""
    shape, origin, spacing = centres(depth)
    n = shape[0]
    scene.Volume(shape, origin, spacing, out=values)
    ins = values < 0
    lab = torch.arange(n ** 3, dtype=torch.int64, device=values.device).reshape(n, n, n)
    while True:
        new = lab.clone()
        for axis in range(3):
            a, b = [slice(None)] * 3, [slice(None)] * 3
            a[axis], b[axis] = slice(0, n - 1), slice(1, n)
            a, b = tuple(a), tuple(b)
            same = ins[a] == ins[b]
            new[a] = torch.where(same, torch.minimum(new[a], lab[b]), new[a])
            new[b] = torch.where(same, torch.minimum(new[b], lab[a]), new[b])
        new = new.reshape(-1)[new]
        if bool((new == lab).all()):
            break
        lab = new
    count = int(torch.unique(lab).numel())
    torch.cuda.synchronize()
    return count


def route_host(scene, depth):
    """(the number of components, milliseconds) by the route on the host, or None without scipy"""
    try:
        import scipy.ndimage as ndi
    except ImportError:
        return None
    t0 = time.perf_counter()
    ins = scene.Volume(*centres(depth)) < 0
    count = ndi.label(ins)[1] + ndi.label(~ins)[1]
    return count, (time.perf_counter() - t0) * 1e3


def bench_case(what, scene, depth):
    rec, st = scene.Components(depth=depth)
    values = torch.empty((1 << depth,) * 3, dtype=torch.float32, device="cuda")
    labels = torch.empty(8 ** depth, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    agrees = route_torch(scene, depth, values) == len(rec)
    assert agrees, f"{what}, depth {depth}: the torch route counts other components than the call"
    host = route_host(scene, depth)
    assert host is None or host[0] == len(rec), f"{what}, depth {depth}: scipy counts other components than the call"
    calls = {"components": lambda: scene.Components(depth=depth)[1].kernel_ms,
             "components_labels": lambda: scene.Components(depth=depth, labels=True)[1].kernel_ms,
             "components_device": lambda: scene.ComponentsDevice(depth=depth, labels_ptr=labels.data_ptr())[1].kernel_ms,
             "route_torch": lambda: float("nan") * route_torch(scene, depth, values)}
    t = {name: ([], []) for name in calls}
    for i in range(WARMUP + CALLS):
        for name, call in calls.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            kernel = call()
            torch.cuda.synchronize()
            if i >= WARMUP:
                t[name][0].append((time.perf_counter() - t0) * 1e3)
                t[name][1].append(kernel)
    solid = rec["flags"] == sb.COMPONENT_SOLID
    out = {"scene": what, "depth": depth, "points": int(st.points), "inside": int(st.inside), "components": int(len(rec)), "solids": int(solid.sum()),
           "largest_solid_points": int(rec["points"][solid].max()) if solid.any() else 0,
           "enclosed_voids": int(sum(sb.component_enclosed(r, depth) for r in rec[~solid])),
           "route_torch_count_agrees": agrees, "route_host_count_agrees": None if host is None else True,
           "route_host_ms_once": None if host is None else round(host[1], 1)}
    for name in calls:
        out[name + "_call_ms"] = spread(t[name][0])
        if name != "route_torch":
            out[name + "_kernel_ms"] = spread(t[name][1])
    out["route_torch_over_components_device"] = round(out["route_torch_call_ms"]["median"] / out["components_device_call_ms"]["median"], 2)
    print(json.dumps(out), file=sys.stderr, flush=True)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--out", default=None)
    ap.add_argument("--profile", type=int, default=None)
    args = ap.parse_args()
    od = sb.dragon_standin(9, nthreads=16)
    with sb.Scene(od) as big:
        del od
        with big.Edit(CARVE) as carved:
            if args.profile is not None:
                for _ in range(10):
                    rec, st, _ = carved.Components(depth=args.profile, labels=True)
                print(json.dumps({"depth": args.profile, "components": len(rec), "kernel_ms": round(st.kernel_ms, 4)}))
                return
            line = {"what": "sdfhip_scene_components", "device": torch.cuda.get_device_name(0), "calls": CALLS, "warmup": WARMUP, "depths": list(DEPTHS),
                    "scenes": ["dragon_standin_d9", "dragon_standin_d9 carved (sphere 0.5 0.5 0.5 r 0.2)"], "nodes_in": [int(big.Length), int(carved.Length)],
                    "clock": "host, round a synchronous call; kernel_ms: the call's device events",
                    "spread": "median, minimum, maximum over the rounds; the variants alternate inside a round", "cases": []}
            for what, scene in (("dragon", big), ("carved", carved)):
                for depth in DEPTHS:
                    line["cases"].append(bench_case(what, scene, depth))
    text = json.dumps(line)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
