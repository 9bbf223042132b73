"""The workload and the summary of scripts/volume_pmc.sh: --lattice D --depth d --builds N reads the 28 M-node scene (dragon_standin(9))
on lattice_of_depth(D) into a device tensor and builds it N times to depth d (Scene.FromVolume); --summarise DIR adds up, per counter,
the values of every k_volume_level dispatch in DIR's rocprofv3 CSV files and divides by the builds: one JSON line, per lattice."""
import argparse
import collections
import csv
import glob
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def workload(lattice_depth, depth, builds):
    import torch

    import sdfbox_amd as sb
    with sb.Scene(sb.dragon_standin(9, nthreads=16)) as big:
        lattice = sb.lattice_of_depth(lattice_depth)
        grid = torch.empty(lattice[0], dtype=torch.float32, device="cuda")
        big.Volume(*lattice, out=grid)
        for _ in range(builds):
            res, st = sb.Scene.FromVolume(grid, lattice[1], lattice[2], depth=depth, want_stats=True)
            res.close()
        print(json.dumps({"lattice": lattice[0][0], "depth": depth, "nodes_out": int(st.nodes_out), "kernel_ms_under_the_profiler": round(st.kernel_ms, 3)}))


def summarise(root, builds, out):
    line = {"what": "rocprofv3 --pmc over scripts/volume_pmc.py, a few counters per pass and nothing traced beside them; k_volume_level<float> "
                    "building the 28 M-node scene's field to depth 8 from its 257^3 (lattice 8) and its 513^3 (lattice 9) grid; per counter "
                    "the sum over one build's level dispatches (mean of the builds); chip-wide sums", "builds": builds, "lattices": {}}
    for lattice in (8, 9):
        agg, launches = collections.defaultdict(float), collections.Counter()
        for f in glob.glob(os.path.join(root, f"p*_l{lattice}", "*", "*_counter_collection.csv")):
            for r in csv.DictReader(open(f)):
                if "k_volume_level" in r["Kernel_Name"]:
                    agg[r["Counter_Name"]] += float(r["Counter_Value"])
                    launches[r["Counter_Name"]] += 1
        rec = {k: round(v / builds) for k, v in sorted(agg.items())}
        rec["level_dispatches_per_build"] = (max(launches.values()) // builds) if launches else 0
        if rec.get("TCC_REQ_sum"):
            rec["l2_hit_rate"] = round(rec.get("TCC_HIT_sum", 0) / max(rec.get("TCC_HIT_sum", 0) + rec.get("TCC_MISS_sum", 0), 1), 4)
        line["lattices"][str(2 ** lattice + 1)] = rec
    text = json.dumps(line)
    print(text)
    if out:
        with open(out, "w") as f:
            f.write(text + "\n")


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--lattice", type=int, default=8)
    ap.add_argument("--depth", type=int, default=8)
    ap.add_argument("--builds", type=int, default=3)
    ap.add_argument("--summarise", default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.summarise:
        summarise(args.summarise, args.builds, args.out)
    else:
        workload(args.lattice, args.depth, args.builds)


if __name__ == "__main__":
    main()
