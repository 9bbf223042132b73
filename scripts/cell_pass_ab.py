"""A/B of two builds of the library on the three passes over a scene's cells (DESIGN.md section 8, N7 "The cell pass"): scripts/mesh_bench.py,
scripts/slice_bench.py and scripts/measure_bench.py, each in a fresh process per run with SDFHIP_LIB set, alternating parent, head,
parent, head in one session.  Every timed figure of the benches' lines (a [median, ...] list under a key that ends in `_ms`) becomes one
row: the parent's two medians, their mean (the reference) and their spread (the margin: |run 1 - run 2|), the head's two medians and
their mean, whether the head's mean lies within the spread of the reference, and the same verdict for each of the head's runs on its
own (the mean can average one run back in).  A commit cannot name its own hash: the record holds the sha256 of both libraries as
they were benchmarked.  A run that fails ends the session: nothing more is started.

    python scripts/cell_pass_ab.py --parent PARENT.so --head HEAD.so --parent-commit HASH --head-commit HASH --out profiles/cell_pass_ab.json"""
import argparse
import hashlib
import json
import os
import subprocess
import sys
import tempfile

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCHES = (("mesh", ["scripts/mesh_bench.py"]), ("slice", ["scripts/slice_bench.py"]), ("measure", ["scripts/measure_bench.py"]))
RUN_SECONDS = 240


def timed_rows(node, path=""):
    """(path, median) of every `*_ms: [median, ...]` list below `node`, in the line's order"""
    if isinstance(node, dict):
        for k, v in node.items():
            if k.endswith("_ms") and isinstance(v, list) and v and all(isinstance(x, (int, float)) for x in v):
                yield f"{path}/{k}", v[0]
            else:
                yield from timed_rows(v, f"{path}/{k}")
    elif isinstance(node, list):
        for v in node:
            tag = ",".join(str(v[k]) for k in ("scene", "stack", "layers", "level") if isinstance(v, dict) and k in v)
            yield from timed_rows(v, f"{path}[{tag}]")


def sha256_of(path):
    with open(path, "rb") as f:
        return hashlib.sha256(f.read()).hexdigest()


def run(bench, lib, tmp, name):
    out = os.path.join(tmp, name + ".json")
    env = dict(os.environ, SDFHIP_LIB=os.path.abspath(lib))
    subprocess.run([sys.executable] + bench + ["--out", out], cwd=REPO, env=env, check=True, timeout=RUN_SECONDS, stdout=subprocess.DEVNULL)
    with open(out) as f:
        return json.loads(f.readline())


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    for a in ("--parent", "--head", "--parent-commit", "--head-commit", "--out"):
        ap.add_argument(a, required=True)
    args = ap.parse_args()
    lines = {}
    with tempfile.TemporaryDirectory() as tmp:
        for rnd in (1, 2):
            for side, lib in (("parent", args.parent), ("head", args.head)):
                for name, bench in BENCHES:
                    lines[(name, side, rnd)] = run(bench, lib, tmp, f"{name}_{side}_{rnd}")
                    print(f"{name} {side} run {rnd} done", file=sys.stderr, flush=True)
    rows = []
    for name, _ in BENCHES:
        cols = {(side, rnd): dict(timed_rows(lines[(name, side, rnd)])) for side in ("parent", "head") for rnd in (1, 2)}
        for key in cols[("parent", 1)]:
            p, h = [cols[("parent", r)][key] for r in (1, 2)], [cols[("head", r)][key] for r in (1, 2)]
            ref, spread, head = (p[0] + p[1]) / 2, abs(p[0] - p[1]), (h[0] + h[1]) / 2
            rows.append({"bench": name, "line": key, "parent_ms": p, "parent_reference_ms": round(ref, 4), "parent_spread_ms": round(spread, 4),
                         "head_ms": h, "head_mean_ms": round(head, 4), "head_minus_reference_ms": round(head - ref, 4),
                         "within_parent_spread": abs(head - ref) <= spread, "head_runs_within_parent_spread": [abs(x - ref) <= spread for x in h]})
    rec = {"what": "parent against head on the cell passes: mesh_bench, slice_bench, measure_bench; parent, head, parent, head in one session",
           "device": lines[("mesh", "head", 1)]["device"], "parent_commit": args.parent_commit, "head_commit": args.head_commit,
           "parent_library_sha256": sha256_of(args.parent), "head_library_sha256": sha256_of(args.head),
           "rows": rows, "rows_within_parent_spread": sum(r["within_parent_spread"] for r in rows),
           "rows_with_both_head_runs_within": sum(all(r["head_runs_within_parent_spread"]) for r in rows), "rows_total": len(rows)}
    with open(args.out, "w") as f:
        f.write(json.dumps(rec, indent=1) + "\n")
    print(json.dumps({k: rec[k] for k in ("rows_within_parent_spread", "rows_with_both_head_runs_within", "rows_total")}))


if __name__ == "__main__":
    main()
