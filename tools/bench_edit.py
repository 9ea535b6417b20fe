#!/usr/bin/env python
"""Board edits in place against the only other route to the same cells ("Board edits").

On a band-layout N x N board (default 65536), after load_random and ~0.6 s of settle steps, times
with a host clock around the blocking calls, 3 warm-ups and then --reps repetitions with the
variants alternating, for a 36 x 9 pattern (the Gosper gun) and a 4096 x 4096 random pattern ORed
into the board at a column that is a multiple of 64 (the cheapest case for the host edit of b):

  paste_<name>   (a) Engine.paste(pattern, x0, y0, "or") followed by step(12): the board stays in the
                 band layout and keeps its turn counter; the 2-D array is bit-packed inside the call
  words_<name>   (a) with the pattern packed beforehand (Engine.paste_words), as the old route has it
  old_<name>     (b) store_words of the covered rows (the board is converted to the standard layout),
                 the pattern ORed into them on the host, load_words (the turn counter restarts at 0),
                 then step(12) (the board is converted back)
  step12         a plain step(12)

Prints one JSON line; <route>_minus_step_ms is what the edit costs beyond the step.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "gol-distributed-final_amd")]

GOSPER_GUN = ("x = 36, y = 9, rule = B3/S23\n24bo$22bobo$12b2o6b2o12b2o$11bo3bo4b2o12b2o$2o8bo5bo3b2o$2o8bo3bob2o4bobo$"
              "10bo5bo7bo$11bo3bo$12b2o!\n")


def summary(ms):
    s = sorted(ms)
    return {"median_ms": round(statistics.median(s), 4), "min_ms": round(s[0], 4), "max_ms": round(s[-1], 4),
            "p25_ms": round(s[len(s) // 4], 4), "p75_ms": round(s[(3 * len(s)) // 4], 4), "n": len(s)}


def timed(fn):
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e3


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--board", type=int, default=65536)
    ap.add_argument("--big", type=int, default=4096, help="side of the large pattern")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--settle-s", type=float, default=0.6)
    a = ap.parse_args()
    import numpy as np

    import golhip
    from golhip._lib import pack_pattern
    n = a.board
    x0, y0 = (n // 3) // 64 * 64, n // 2 + 3
    patterns = {"gun": golhip.parse_rle(GOSPER_GUN)[0],
                "big": np.random.default_rng(1).random((a.big, a.big)) < 0.3}
    out = {"tool": "bench_edit", "board": n, "at": [x0, y0], "reps": a.reps,
           "patterns": {k: list(v.shape[::-1]) for k, v in patterns.items()}}
    with golhip.Engine(n, n, layout="band", device=0) as e:
        e.load_random(1)
        out["settle_steps"] = max(1, round(a.settle_s * 145e12 / (n * n * 12.0)))
        e.step(12 * out["settle_steps"])
        layouts, turns = {}, {}

        def paste(name):
            def f():
                _, layouts[name] = e.paste(patterns[name], x0, y0, "or", return_layout=True)
                e.step(12)
                turns["paste"] = e.turn
            return f

        def paste_words(name):
            words = pack_pattern(patterns[name])
            w = patterns[name].shape[1]

            def f():
                e.paste_words(words, w, x0, y0, "or")
                e.step(12)
            return f

        def old(name):
            words = pack_pattern(patterns[name])  # (packed beforehand, as for words_<name>)
            h, pw = words.shape

            def f():
                rows = e.store_words(y0, y0 + h)
                rows[:, x0 // 64:x0 // 64 + pw] |= words
                e.load_words(y0, rows)
                e.step(12)
                turns["old"] = e.turn
            return f
        variants = []
        for name in patterns:
            variants += [("paste_" + name, paste(name)), ("words_" + name, paste_words(name)), ("old_" + name, old(name))]
        variants.append(("step12", lambda: e.step(12)))
        ms = {name: [] for name, _ in variants}
        for rep in range(3 + a.reps):
            for name, fn in variants:
                t = timed(fn)
                if rep >= 3:
                    ms[name].append(t)
        out["ms"] = {name: summary(v) for name, v in ms.items()}
        step = out["ms"]["step12"]["median_ms"]
        out["minus_step_ms"] = {name: round(v["median_ms"] - step, 4) for name, v in out["ms"].items() if name != "step12"}
        out["paste_layouts"] = layouts
        out["turn_after"] = turns  # the old route restarts the counter: 12 after its step
    print(json.dumps(out))


if __name__ == "__main__":
    main()
