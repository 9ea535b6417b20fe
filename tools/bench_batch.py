#!/usr/bin/env python
"""A batch of small boards against the only other way to step them.

For n boards of H x W cells and T turns, in one process on one GPU, the variants alternating:

  loop          the route without the batch: one Engine(H, W), and per board load_words + step(T).
                The boards of a loop run one after the other, so the time per board does not depend
                on n: the loop is timed over the first --loop-boards boards of the batch (all of
                them when n is smaller) and reported per board.
  batch         one Batch of the n boards: load_words of all of them + step(T).
  batch_step    the step(T) alone, on boards already loaded.
  batch_settle  step(T, settled=True) alone: the settle scan's cost is batch_settle / batch_step.

Host clock around the blocking calls, --settle-s seconds of batch steps first, one warm-up of every
variant, --reps repetitions, medians.  Before the timing the tool checks that the loop's boards after
T turns equal the batch's.  Prints one JSON line per point (--out: also appended to that file):
boards/s and cell-updates/s of every variant and ratio = loop seconds per board / batch seconds per
board.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "gol-distributed-final_amd")]

POINTS = [(64, 256), (64, 4096), (64, 65536), (512, 256), (512, 4096)]


def timed(fn):
    t0 = time.perf_counter()
    fn()
    return time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--points", default=",".join(f"{s}x{n}" for s, n in POINTS), help="side x boards, comma-separated")
    ap.add_argument("--turns", default="100,1000")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--loop-boards", type=int, default=64)
    ap.add_argument("--settle-s", type=float, default=0.5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import numpy as np

    import golhip
    for point in a.points.split(","):
        side, n = (int(v) for v in point.split("x"))
        with golhip.Batch(n, side, side, device=0) as b, golhip.Engine(side, side, device=0) as e:
            b.load_random(side + n)
            words = b.store_words()
            m = min(n, a.loop_boards)
            t_end = time.perf_counter() + a.settle_s
            while time.perf_counter() < t_end:
                b.step(100)
            for T in (int(t) for t in a.turns.split(",")):
                def loop():
                    for i in range(m):
                        e.load_words(0, words[i])
                        e.step(T)

                def batch():
                    b.load_words(words)
                    b.step(T)
                # the two routes agree on the loop's boards
                batch()
                got = b.store_words(0, m)
                same = True
                for i in range(m):
                    e.load_words(0, words[i])
                    e.step(T)
                    same = same and bool(np.array_equal(e.store_words(0, side), got[i]))
                variants = [("loop", loop), ("batch", batch), ("batch_step", lambda: b.step(T)),
                            ("batch_settle", lambda: b.step(T, settled=True))]
                secs = {name: [] for name, _ in variants}
                for rep in range(1 + a.reps):
                    for name, fn in variants:
                        t = timed(fn)
                        if rep >= 1:
                            secs[name].append(t)
                med = {name: statistics.median(v) for name, v in secs.items()}
                per_board = {name: med[name] / (m if name == "loop" else n) for name in med}
                out = {"tool": "bench_batch", "side": side, "boards": n, "turns": T, "reps": a.reps, "loop_boards": m,
                       "routes_agree": same, "info": b.info(), "engine": e.info(),
                       "median_s": {k: round(v, 6) for k, v in med.items()},
                       "min_s": {k: round(min(v), 6) for k, v in secs.items()},
                       "max_s": {k: round(max(v), 6) for k, v in secs.items()},
                       "boards_per_s": {k: round(1.0 / v, 1) for k, v in per_board.items()},
                       "cell_updates_per_s": {k: float(f"{side * side * T / v:.4g}") for k, v in per_board.items()},
                       "ratio_loop_over_batch": round(per_board["loop"] / per_board["batch"], 1),
                       "settle_over_step": round(med["batch_settle"] / med["batch_step"], 3)}
                line = json.dumps(out)
                print(line, flush=True)
                if a.out:
                    with open(a.out, "a") as f:
                        f.write(line + "\n")


if __name__ == "__main__":
    main()
