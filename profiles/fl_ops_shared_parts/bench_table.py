"""The speed check of this folder's README from the JSON lines of three parent runs and three child runs
of a benchmark (benchmarks/bench_robust_agg.py, benchmarks/bench_clipped_gossip.py), which alternated
P C P C P C in one job:

    python bench_table.py DIR NAME      reads DIR/NAME_P{1,2,3}.jsonl and DIR/NAME_C{1,2,3}.jsonl

A kernel-time figure is a "ms" leaf under "kernels" (bench_robust_agg.py) or a top-level "*_ms" field
(bench_clipped_gossip.py: the median of its windows). For each, the parent's three-run range is widened by its own width on either
side, and the child's three values must lie inside. Prints a markdown table; exit status 1 if one is outside.
"""

import json
import sys


def figures(path):
    out = {}
    for line in open(path):
        if not line.startswith("{"):
            continue
        rec = json.loads(line)
        case = "/".join(str(rec[k]) for k in ("model", "aggregator", "op", "honest_rows", "size", "name", "peers") if k in rec)
        for name, val in rec.get("kernels", {}).items():
            if isinstance(val, dict) and "ms" in val:
                out[f"{case}: {name}"] = val["ms"]
        for name, val in rec.items():
            if name.endswith("_ms") and "kernels" not in rec:  # a number, or {"median", "min", "max"} over the windows
                out[f"{case}: {name}"] = val["median"] if isinstance(val, dict) else val
    return out


def main(d, name):
    runs = {s: [figures(f"{d}/{name}_{s}{i}.jsonl") for i in (1, 2, 3)] for s in "PC"}
    bad = 0
    print("| figure (ms) | parent 1 | parent 2 | parent 3 | child 1 | child 2 | child 3 | allowed | |")
    print("|---|---|---|---|---|---|---|---|---|")
    for key in runs["P"][0]:
        if not all(key in r for side in runs.values() for r in side):
            print(f"| {key} | missing from a run | | | | | | | OUTSIDE |")
            bad += 1
            continue
        p = [r[key] for r in runs["P"]]
        c = [r[key] for r in runs["C"]]
        lo, hi = min(p), max(p)
        lo, hi = lo - (hi - lo), hi + (hi - lo)
        ok = all(lo <= v <= hi for v in c)
        bad += not ok
        print(f"| {key} | " + " | ".join(f"{v:.4f}" for v in p + c) + f" | {lo:.4f} .. {hi:.4f} | {'inside' if ok else 'OUTSIDE'} |")
    print(f"\n{len(runs['P'][0])} figures, {bad} outside")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1], sys.argv[2]))
