"""Selection (sdfhip_scene_select) against the route the library offered before it, on cfg-2's 28 M-node
scene (dragon_standin(9)) after edit_bench's r = 0.05 carve at the cube's centre, on the unit cube's lattice at depth 7, 8 and 9 and
to a result of depth 9.  In the same process, per lattice depth, CALLS rounds after WARMUP; each figure is the median, minimum and
maximum over the rounds:
  keep_largest / fill_enclosed   one Scene.Select with that rule: call_ms = host clock round the synchronous call; label_ms, kernel_ms
                                 and scene_ms = the call's own figures (sdfhip_select_stats)
  route                          what a user had: Scene.ComponentsDevice with the labels in a torch tensor, Scene.Volume on the same
                                 centres, the mask in torch (the points whose label is not the largest solid's get |value|), and
                                 Scene.FromVolume of the masked lattice to depth 9.  Host clock to the last synchronise.  It resamples
                                 the field twice and its tree is another tree: the figure is a time, not an equivalence
  place                          Scene.Place at the identity to depth 9: the same look-ups as the selection's levels without the bit
                                 tests.  kernel_ms per node of the selection over the placement's says what the tests cost
These figures are recorded, not gated.

    python scripts/select_bench.py [--out FILE]          # prints one JSON line (and writes it to FILE)"""
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
RESULT_DEPTH = 9
CARVE = [(sb.EDIT_CARVE, sb.BRUSH_SPHERE, (0.5, 0.5, 0.5, 0.05))]


def route(scene, depth, keep_label, labels, values):
    """the largest solid alone by the old route; returns the result's node count"""
    n, pitch = 1 << depth, 2.0 ** -depth
    scene.ComponentsDevice(depth=depth, labels_ptr=labels.data_ptr())
    scene.Volume((n, n, n), (pitch / 2,) * 3, pitch, out=values)
    masked = torch.where((values < 0) & (labels.view(n, n, n) != keep_label), values.abs(), values)
    with sb.Scene.FromVolume(masked, (pitch / 2,) * 3, pitch, RESULT_DEPTH) as res:
        torch.cuda.synchronize()
        return int(res.Length)


def timed(call):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = call()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def select_stats(scene, depth, **rule):
    res, st = scene.Select(lattice_depth=depth, depth=RESULT_DEPTH, want_stats=True, **rule)
    res.close()
    return st


def bench_case(scene, depth, place_ms_per_node):
    rec, _ = scene.Components(depth=depth)
    solid = rec["flags"] == sb.COMPONENT_SOLID
    largest = rec[solid][np.argmax(rec["points"][solid])]
    labels = torch.empty(8 ** depth, dtype=torch.int32, device="cuda")
    values = torch.empty((1 << depth,) * 3, dtype=torch.float32, device="cuda")
    rules = {"keep_largest": dict(keep_largest=True), "fill_enclosed": dict(fill_enclosed=True)}
    t = {name: {k: [] for k in ("call_ms", "label_ms", "kernel_ms", "scene_ms")} for name in rules}
    route_ms, last = [], {}
    route_nodes = 0
    for i in range(WARMUP + CALLS):
        for name, rule in rules.items():
            ms, st = timed(lambda: select_stats(scene, depth, **rule))
            last[name] = st
            if i >= WARMUP:
                t[name]["call_ms"].append(ms)
                for k in ("label_ms", "kernel_ms", "scene_ms"):
                    t[name][k].append(getattr(st, k))
        ms, route_nodes = timed(lambda: route(scene, depth, int(largest["label"]), labels, values))
        if i >= WARMUP:
            route_ms.append(ms)
    out = {"lattice_depth": depth, "points": 8 ** depth, "components": int(len(rec)), "solids": int(solid.sum()),
           "largest_solid_points": int(largest["points"]), "route_call_ms": spread(route_ms), "route_nodes_out": route_nodes}
    for name in rules:
        st = last[name]
        out[name] = {k: spread(v) for k, v in t[name].items()}
        out[name].update({"flipped_solids": int(st.flipped_solids), "flipped_voids": int(st.flipped_voids), "points_flipped": int(st.points_flipped),
                          "nodes_out": int(st.nodes_out), "samples": int(st.samples)})
        per_node = out[name]["kernel_ms"]["median"] / st.nodes_out
        out[name]["kernel_ms_per_node_over_place"] = round(per_node / place_ms_per_node, 3)
    out["route_over_keep_largest"] = round(out["route_call_ms"]["median"] / out["keep_largest"]["call_ms"]["median"], 2)
    print(json.dumps(out), file=sys.stderr, flush=True)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    od = sb.dragon_standin(9, nthreads=16)
    with sb.Scene(od) as big:
        del od
        with big.Edit(CARVE) as carved:
            place = {k: [] for k in ("call_ms", "kernel_ms", "scene_ms")}
            nodes = 0
            for i in range(WARMUP + CALLS):
                def placed():
                    res, st = carved.Place(np.eye(3, dtype=np.float32), 1.0, (0.0, 0.0, 0.0), RESULT_DEPTH, want_stats=True)
                    res.close()
                    return st
                ms, st = timed(placed)
                nodes = int(st.nodes_out)
                if i >= WARMUP:
                    place["call_ms"].append(ms)
                    place["kernel_ms"].append(st.kernel_ms)
                    place["scene_ms"].append(st.scene_ms)
            line = {"what": "sdfhip_scene_select", "device": torch.cuda.get_device_name(0), "calls": CALLS, "warmup": WARMUP,
                    "lattice_depths": list(DEPTHS), "result_depth": RESULT_DEPTH, "scene": "dragon_standin_d9 carved (sphere 0.5 0.5 0.5 r 0.05)",
                    "nodes_in": int(carved.Length), "clock": "host, round a synchronous call; label_ms, kernel_ms: the call's device events",
                    "spread": "median, minimum, maximum over the rounds; the variants alternate inside a round",
                    "place_identity": dict({k: spread(v) for k, v in place.items()}, nodes_out=nodes), "cases": []}
            per_node = line["place_identity"]["kernel_ms"]["median"] / nodes
            for depth in DEPTHS:
                line["cases"].append(bench_case(carved, depth, per_node))
    text = json.dumps(line)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
