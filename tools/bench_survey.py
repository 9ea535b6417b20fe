#!/usr/bin/env python
"""A rule survey and a cycle census on a batch of small boards.

For n boards of H x W cells and T turns, in one process on one GPU, the variants alternating:

  uniform_step  step(T) of a batch under one table rule (B36/S23): the one-rule kernel.
  mixed_step    step(T) of the same boards with board i under rule i mod 2^18 (birth = the low 9 bits,
                survive = the next 9): the kernel that reads a rule per board.
  each_step     step(T) of the per-board kernel on the uniform batch itself, the same device buffers and
                boards: every board under B36/S23 but the last one (B3/S23), set before the clock starts
                (with one untimed turn, which uploads the rules) and undone after it stops.  each_step /
                uniform_step is what the kernel itself costs.
  busy_step     step(T) of the one-rule kernel under B0246/S1357, a rule that flips most cells every
                turn as half the rules of the mixed batch do (every rule with B0): busy_step /
                uniform_step is what such boards cost the unchanged kernel.
  loop          the only other route to a rule survey: per rule one set_rule + load_words + step(T) on
                a batch of one board.  The rules of a loop run one after the other, so the time per
                rule does not depend on n: the loop is timed over the first --loop-rules rules and
                reported per rule, against the mixed batch's load_words + step(T) per board.
  mixed         load_words of all n boards + step(T) of the mixed batch.
  step          step(T) of a B3/S23 batch.
  settle        step(T, settled=True) of it: the scan for periods 1 and 2.
  cycles        step_cycles(T) of it: the scan for any period.
  mixed_cycles  step_cycles(T) of the mixed batch.

Host clock around the blocking calls, --settle-s seconds of batch steps first, one warm-up of every
variant, --reps repetitions, medians with minimum and maximum.  Before the timing the tool checks that
the loop's boards after T turns equal the mixed batch's.  Prints one JSON line per point and T
(--out: also appended to that file).
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


def timed(fn):
    t0 = time.perf_counter()
    fn()
    return time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--points", default=",".join(f"{s}x{n}" for s, n in POINTS), help="side x boards, comma-separated")
    ap.add_argument("--turns", default="100,1000")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--loop-rules", type=int, default=64)
    ap.add_argument("--settle-s", type=float, default=0.5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "batch", "bench_survey.jsonl"))
    a = ap.parse_args()
    import numpy as np

    import golhip
    for point in a.points.split(","):
        side, n = (int(v) for v in point.split("x"))
        index = np.arange(n, dtype=np.uint32) % np.uint32(1 << 18)
        rules = np.stack([index & np.uint32(511), index >> np.uint32(9)], axis=1)
        with golhip.Batch(n, side, side, device=0) as conway, golhip.Batch(n, side, side, rule="B36/S23", device=0) as uniform, \
                golhip.Batch(n, side, side, device=0) as mixed, golhip.Batch(1, side, side, device=0) as one, \
                golhip.Batch(n, side, side, rule="B0246/S1357", device=0) as busy:
            mixed.set_rules(rules)
            conway.load_random(side + n)
            words = conway.store_words()
            uniform.load_words(words)
            mixed.load_words(words)
            busy.load_words(words)
            m = min(n, a.loop_rules)
            t_end = time.perf_counter() + a.settle_s
            while time.perf_counter() < t_end:
                conway.step(100)
            for T in (int(t) for t in a.turns.split(",")):
                def loop():
                    for i in range(m):
                        one.set_rule((int(rules[i, 0]), int(rules[i, 1])))
                        one.load_words(words[i:i + 1])
                        one.step(T)

                def each_step():
                    uniform.set_rules(["B3/S23"], first=n - 1)
                    uniform.step(1)
                    t = timed(lambda: uniform.step(T))
                    uniform.set_rule("B36/S23")
                    return t

                def mixed_all():
                    mixed.load_words(words)
                    mixed.step(T)
                # the two routes agree on the loop's rules
                mixed_all()
                got = mixed.store_words(0, m)
                same = True
                for i in range(m):
                    one.set_rule((int(rules[i, 0]), int(rules[i, 1])))
                    one.load_words(words[i:i + 1])
                    one.step(T)
                    same = same and bool(np.array_equal(one.store_words()[0], got[i]))
                variants = [("uniform_step", lambda: uniform.step(T)), ("mixed_step", lambda: mixed.step(T)),
                            ("each_step", None), ("busy_step", lambda: busy.step(T)), ("loop", loop),
                            ("mixed", mixed_all), ("step", lambda: conway.step(T)),
                            ("settle", lambda: conway.step(T, settled=True)), ("cycles", lambda: conway.step_cycles(T)),
                            ("mixed_cycles", lambda: mixed.step_cycles(T))]
                secs = {name: [] for name, _ in variants}
                for rep in range(1 + a.reps):
                    for name, fn in variants:
                        t = each_step() if fn is None else timed(fn)
                        if rep >= 1:
                            secs[name].append(t)
                med = {name: statistics.median(v) for name, v in secs.items()}
                per_board = {name: med[name] / (m if name == "loop" else n) for name in med}
                out = {"tool": "bench_survey", "side": side, "boards": n, "turns": T, "reps": a.reps, "loop_rules": m,
                       "routes_agree": same, "info": mixed.info(),
                       "median_s": {k: round(v, 6) for k, v in med.items()},
                       "min_s": {k: round(min(v), 6) for k, v in secs.items()},
                       "max_s": {k: round(max(v), 6) for k, v in secs.items()},
                       "cell_updates_per_s": {k: float(f"{side * side * T / v:.4g}") for k, v in per_board.items()},
                       "mixed_over_uniform": round(med["mixed_step"] / med["uniform_step"], 3),
                       "mixed_over_uniform_min_max": [round(min(secs["mixed_step"]) / max(secs["uniform_step"]), 3),
                                                      round(max(secs["mixed_step"]) / min(secs["uniform_step"]), 3)],
                       "each_over_uniform": round(med["each_step"] / med["uniform_step"], 3),
                       "each_over_uniform_min_max": [round(min(secs["each_step"]) / max(secs["uniform_step"]), 3),
                                                     round(max(secs["each_step"]) / min(secs["uniform_step"]), 3)],
                       "busy_over_uniform": round(med["busy_step"] / med["uniform_step"], 3),
                       "ratio_loop_over_mixed": round(per_board["loop"] / per_board["mixed"], 1),
                       "cycles_over_settle": round(med["cycles"] / med["settle"], 3),
                       "cycles_over_step": round(med["cycles"] / med["step"], 3),
                       "mixed_cycles_over_mixed_step": round(med["mixed_cycles"] / med["mixed_step"], 3)}
                line = json.dumps(out)
                print(line, flush=True)
                if a.out:
                    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
                    with open(a.out, "a") as f:
                        f.write(line + "\n")


if __name__ == "__main__":
    main()
