#!/usr/bin/env python
"""The soup search against the only other route to the same census, on a batch of small boards.

For n slots of H x W cells, a horizon and a supply of `total` soups, in one process on one GPU, the
variants alternating:

  search  search(seed, total, horizon): soups streamed through the slots, a census per soup.
  loop    for k in range(total / n): load_soups(seed, k n), run_cycles(horizon), alive_counts(), hashes()
          -- a pass per n soups, each paying run_cycles' tail of mostly empty launches.

Before the timing the tool checks on soups [0, n) that both return equal found and period.  Host clock
around the blocking calls, --settle-s seconds of batch steps first, one warm-up of every variant, --reps
repetitions, medians with minimum and maximum.  Per point: soups per second of both, their ratio, and
the search's occupancy from its stats (board-turns computed over the board-turns of a full grid).
Prints one JSON line per point (--out: also appended to that file).
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "gol-distributed-final_amd")]

POINTS = [(64, 65536, 1 << 20), (512, 4096, 16384)]


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--points", default=",".join(f"{s}x{n}x{t}" for s, n, t in POINTS), help="side x slots x soups, comma-separated")
    ap.add_argument("--horizon", type=int, default=10000)
    ap.add_argument("--rule", default="B3/S23")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--settle-s", type=float, default=0.5)
    ap.add_argument("--turns-per-launch", type=int, default=0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "batch", "bench_search.jsonl"))
    a = ap.parse_args()
    import numpy as np

    import golhip
    for point in a.points.split(","):
        side, n, total = (int(v) for v in point.split("x"))
        seed = side + n
        with golhip.Batch(n, side, side, rule=a.rule, device=0, turns_per_launch=a.turns_per_launch) as b:
            b.load_random(seed)
            t_end = time.perf_counter() + a.settle_s
            while time.perf_counter() < t_end:
                b.step(100)

            def search():
                t0 = time.perf_counter()
                res = b.search(seed, total, a.horizon, stats=True)
                return time.perf_counter() - t0, res

            def loop():
                t0 = time.perf_counter()
                found = []
                for k in range(0, total, n):
                    b.load_soups(seed, k)
                    f, _ = b.run_cycles(a.horizon)
                    b.alive_counts()
                    b.hashes()
                    found.append(f)
                return time.perf_counter() - t0, np.concatenate(found)[:total]

            f0, p0, _, _ = b.search(seed, n, a.horizon)
            b.load_soups(seed, 0)
            f1, p1 = b.run_cycles(a.horizon)
            same = bool(np.array_equal(f0, f1) and np.array_equal(p0, p1))
            secs = {"search": [], "loop": []}
            stats = found = None
            for rep in range(1 + a.reps):
                t, res = search()
                stats, found = res[4], res[0]
                ts, fl = loop()
                same = same and bool(np.array_equal(found, fl))
                if rep >= 1:
                    secs["search"].append(t)
                    secs["loop"].append(ts)
            med = {k: statistics.median(v) for k, v in secs.items()}
            out = {"tool": "bench_search", "side": side, "slots": n, "soups": total, "rule": a.rule, "horizon": a.horizon,
                   "reps": a.reps, "calls_agree": same, "info": b.info(), "found": int(np.count_nonzero(found >= 0)),
                   "found_median": int(np.median(found[found >= 0])) if np.any(found >= 0) else -1, "stats": stats,
                   "median_s": {k: round(v, 6) for k, v in med.items()},
                   "min_s": {k: round(min(v), 6) for k, v in secs.items()},
                   "max_s": {k: round(max(v), 6) for k, v in secs.items()},
                   "soups_per_s": {k: round(total / v, 1) for k, v in med.items()},
                   "search_over_loop_time": round(med["search"] / med["loop"], 4),
                   "search_over_loop_time_min_max": [round(min(secs["search"]) / max(secs["loop"]), 4),
                                                     round(max(secs["search"]) / min(secs["loop"]), 4)]}
            line = json.dumps(out)
            print(line, flush=True)
            if a.out:
                os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
                with open(a.out, "a") as f:
                    f.write(line + "\n")
            if not same:
                sys.exit("search and the run_cycles loop disagree")


if __name__ == "__main__":
    main()
