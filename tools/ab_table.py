#!/usr/bin/env python3
"""Table of a tools/ab_bench.sh run: per variant the headline (M pairs/s), the mean
k_accumulate<1> ms of the timed batch (legs.ches_h2d.kernel_ms) and ms per MSM --
median, min, max and every round -- then each variant against `prev` with prev's own
max - min beside it (the adoption rule of DESIGN 22).
usage: python tools/ab_table.py <output directory of the run> [variant ...]   (default: every variant found, prev first)"""
import glob
import json
import os
import re
import statistics
import sys


def load(d, names):
    runs = {}
    for f in glob.glob(os.path.join(d, "*.json")):
        base = os.path.basename(f)
        # (a variant's name may end in a digit: match the names asked for first)
        m = next((m for m in (re.match(rf"({re.escape(v)})(\d+)\.json$", base) for v in names) if m), None)
        if not m and not names:
            m = re.match(r"([a-z0-9_]*[a-z_])(\d+)\.json$", base)
        if not m:
            continue
        lines = open(f).read().strip().splitlines()
        if not lines:
            continue
        j = json.loads(lines[-1])
        assert j["parity_vs_reference"] is not False, f  # (None: a run without --full checks nothing)
        runs.setdefault(m.group(1), {})[int(m.group(2))] = {
            "value": j["value"] / 1e6, "kernel_ms": j["legs"]["ches_h2d"]["kernel_ms"], "ms_per_step": j["ms_per_step"]}
    return runs


def main(d, names):
    runs = load(d, names)
    names = names or sorted(runs, key=lambda v: (v != "prev", v))
    metrics = ("value", "kernel_ms", "ms_per_step")
    print("  variant  metric        median      min       max     n   per round")
    col = {}
    for v in names:
        for k in metrics:
            xs = [runs[v][i][k] for i in sorted(runs[v])]
            col[v, k] = xs
            print(f"  {v:8s} {k:12s} {statistics.median(xs):9.4f} {min(xs):9.4f} {max(xs):9.4f} {len(xs):4d}   "
                  + " ".join(f"{x:.4f}" if k != "value" else f"{x:.1f}" for x in xs))
    for v in names:
        if v == "prev" or "prev" not in runs:
            continue
        for k in metrics:
            a, b = col[v, k], col["prev", k]
            dm = statistics.median(a) - statistics.median(b)
            print(f"  {v} - prev: {k} median {dm:+.4f} ({100 * dm / statistics.median(b):+.2f} %), "
                  f"prev's max-min {max(b) - min(b):.4f}; per round " + " ".join(f"{x - y:+.4f}" for x, y in zip(a, b)))


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2:])
