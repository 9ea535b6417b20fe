#!/usr/bin/env python
"""Retirement of found boards against the plain cycle scan on a batch of small boards.

For n boards of H x W cells from load_random, a rule and T turns, in one process on one GPU, the
variants alternating, each on a freshly loaded batch (the load is not timed):

  step_cycles  step_cycles(T): every board makes all T turns.
  run_cycles   run_cycles(T): a board leaves the launches once it is found and makes only its remainder.

The points: B3/S23 at every T of --turns, and B2/S (nothing is ever found: the list mode, the retire
pass and the readbacks are pure overhead there) at the first T.  Before the timing the tool checks
that the two calls return equal found and period and leave equal hashes().  Host clock around the
blocking calls, --settle-s seconds of batch steps first, one warm-up of every variant, --reps
repetitions, medians with minimum and maximum.  Per point: the two times, their ratio, and the work
fraction sum(made) / (n T).  Prints one JSON line per point (--out: also appended to that file).
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


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--points", default=",".join(f"{s}x{n}" for s, n in POINTS), help="side x boards, comma-separated")
    ap.add_argument("--turns", default="1000,10000")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--settle-s", type=float, default=0.5)
    ap.add_argument("--turns-per-launch", type=int, default=0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "batch", "bench_retire.jsonl"))
    a = ap.parse_args()
    import numpy as np

    import golhip
    turns = [int(t) for t in a.turns.split(",")]
    for point in a.points.split(","):
        side, n = (int(v) for v in point.split("x"))
        seed = side + n
        with golhip.Batch(n, side, side, device=0, turns_per_launch=a.turns_per_launch) as b:
            b.load_random(seed)
            t_end = time.perf_counter() + a.settle_s
            while time.perf_counter() < t_end:
                b.step(100)
            for rule, T in [("B3/S23", t) for t in turns] + [("B2/S", turns[0])]:
                b.set_rule(rule)

                def timed(call):
                    b.load_random(seed)
                    t0 = time.perf_counter()
                    res = call(T)
                    return time.perf_counter() - t0, res

                _, (f0, p0) = timed(b.step_cycles)
                h0 = b.hashes()
                _, (f1, p1, made) = timed(lambda t: b.run_cycles(t, made=True))
                same = bool(np.array_equal(f0, f1) and np.array_equal(p0, p1) and np.array_equal(h0, b.hashes()))
                variants = [("step_cycles", b.step_cycles), ("run_cycles", b.run_cycles)]
                secs = {name: [] for name, _ in variants}
                for rep in range(1 + a.reps):
                    for name, call in variants:
                        t = timed(call)[0]
                        if rep >= 1:
                            secs[name].append(t)
                med = {name: statistics.median(v) for name, v in secs.items()}
                out = {"tool": "bench_retire", "side": side, "boards": n, "rule": rule, "turns": T, "reps": a.reps,
                       "calls_agree": same, "info": b.info(), "found": int(np.count_nonzero(f0 >= 0)),
                       "found_median": int(np.median(f0[f0 >= 0])) if np.any(f0 >= 0) else -1,
                       "found_max": int(f0.max()),
                       "work_fraction": round(float(made.sum()) / (n * T), 4),
                       "median_s": {k: round(v, 6) for k, v in med.items()},
                       "min_s": {k: round(min(v), 6) for k, v in secs.items()},
                       "max_s": {k: round(max(v), 6) for k, v in secs.items()},
                       "run_over_step": round(med["run_cycles"] / med["step_cycles"], 4),
                       "run_over_step_min_max": [round(min(secs["run_cycles"]) / max(secs["step_cycles"]), 4),
                                                 round(max(secs["run_cycles"]) / min(secs["step_cycles"]), 4)]}
                line = json.dumps(out)
                print(line, flush=True)
                if a.out:
                    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
                    with open(a.out, "a") as f:
                        f.write(line + "\n")
                if not same:
                    sys.exit("run_cycles and step_cycles disagree")


if __name__ == "__main__":
    main()
