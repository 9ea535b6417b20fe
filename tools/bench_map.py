#!/usr/bin/env python
"""What a MAP rule costs a batch against the table circuit of the life-like kernels.

For n boards of H x W cells and T turns, in one process on one GPU, the variants alternating:

  table_step    step(T) of a batch under set_rule("B36/S23"): the one-rule TABLE kernel (not the 7-gate one).
  map_step      step(T) of the same boards under set_map(map_from_rule("B36/S23")): the map kernel, one map.
  table_cycles  step_cycles(T) under the rule.
  map_cycles    step_cycles(T) under the map.

The two batches hold the same boards and stay in step, so every call works on the same states; before the timing
the tool checks that they agree after T turns.  Host clock around the blocking calls, --settle-s seconds of batch
steps first, one warm-up of every variant, --reps repetitions, medians with minimum and maximum.  The ratio map /
table is reported, not gated.  Prints one JSON line per point (--out: also appended to that file).
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "gol-distributed-final_amd")]

POINTS = [(64, 65536), (512, 4096)]
RULE = "B36/S23"


def timed(fn):
    t0 = time.perf_counter()
    fn()
    return time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--points", default=",".join(f"{s}x{n}" for s, n in POINTS), help="side x boards, comma-separated")
    ap.add_argument("--turns", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--settle-s", type=float, default=0.5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "batch", "bench_map.jsonl"))
    a = ap.parse_args()
    import numpy as np

    import golhip
    T = a.turns
    for point in a.points.split(","):
        side, n = (int(v) for v in point.split("x"))
        with golhip.Batch(n, side, side, rule=RULE, device=0) as table, golhip.Batch(n, side, side, device=0) as mapped:
            mapped.set_map(golhip.map_from_rule(RULE))
            table.load_random(side + n)
            mapped.load_words(table.store_words())
            t_end = time.perf_counter() + a.settle_s
            while time.perf_counter() < t_end:
                table.step(100)
                mapped.step(100)
            table.step(T)
            mapped.step(T)
            same = bool(np.array_equal(table.hashes(), mapped.hashes()))
            variants = [("table_step", lambda: table.step(T)), ("map_step", lambda: mapped.step(T)),
                        ("table_cycles", lambda: table.step_cycles(T)), ("map_cycles", lambda: mapped.step_cycles(T))]
            secs = {name: [] for name, _ in variants}
            for rep in range(1 + a.reps):
                for name, fn in variants:
                    t = timed(fn)
                    if rep >= 1:
                        secs[name].append(t)
            same = same and bool(np.array_equal(table.hashes(), mapped.hashes()))
            med = {name: statistics.median(v) for name, v in secs.items()}
            out = {"tool": "bench_map", "side": side, "boards": n, "turns": T, "reps": a.reps, "rule": RULE, "kernels_agree": same,
                   "info": mapped.info(),
                   "median_s": {k: round(v, 6) for k, v in med.items()},
                   "min_s": {k: round(min(v), 6) for k, v in secs.items()},
                   "max_s": {k: round(max(v), 6) for k, v in secs.items()},
                   "cell_updates_per_s": {k: float(f"{n * side * side * T / v:.4g}") for k, v in med.items()},
                   "map_over_table_step": round(med["map_step"] / med["table_step"], 3),
                   "map_over_table_step_min_max": [round(min(secs["map_step"]) / max(secs["table_step"]), 3),
                                                   round(max(secs["map_step"]) / min(secs["table_step"]), 3)],
                   "map_over_table_cycles": round(med["map_cycles"] / med["table_cycles"], 3),
                   "map_over_table_cycles_min_max": [round(min(secs["map_cycles"]) / max(secs["table_cycles"]), 3),
                                                     round(max(secs["map_cycles"]) / min(secs["table_cycles"]), 3)]}
            line = json.dumps(out)
            print(line, flush=True)
            if a.out:
                os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
                with open(a.out, "a") as f:
                    f.write(line + "\n")


if __name__ == "__main__":
    main()
