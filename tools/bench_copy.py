#!/usr/bin/env python
"""Region reads in place against the only other route to the same cells ("Region reads").

On a band-layout N x N board (default 65536), after load_random and ~0.6 s of settle steps, times
with a host clock around the blocking calls, 3 warm-ups and then --reps repetitions with the
variants alternating, for a 36 x 9 rectangle (the Gosper gun's box) and a 4096 x 4096 one at the
board position of tools/bench_edit.py (a column that is a multiple of 64: the cheapest case for the
host slice of b):

  copy_<name>    (a) Engine.copy_words of the rectangle followed by step(12): the board stays in the
                 band layout
  old_<name>     (b) store_words of the covered rows (the board is converted to the standard layout),
                 the rectangle's words sliced out on the host, then step(12) (the board is converted
                 back)
  step12         a plain step(12)
  bounds_board   Engine.bounds() of the whole board
  alive_count    Engine.alive_count(), which reads the same bytes once

Prints one JSON line; <route>_minus_step_ms is what the read costs beyond the step.  The two routes'
cells are compared once before the timing (same board, same turn).
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "gol-distributed-final_amd")]


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
    ap.add_argument("--big", type=int, default=4096, help="side of the large rectangle")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--settle-s", type=float, default=0.6)
    a = ap.parse_args()
    import numpy as np

    import golhip
    n = a.board
    x0, y0 = (n // 3) // 64 * 64, n // 2 + 3
    rects = {"gun": (36, 9), "big": (a.big, a.big)}
    out = {"tool": "bench_copy", "board": n, "at": [x0, y0], "reps": a.reps, "rects": {k: list(v) for k, v in rects.items()}}
    with golhip.Engine(n, n, layout="band", device=0) as e:
        e.load_random(1)
        out["settle_steps"] = max(1, round(a.settle_s * 145e12 / (n * n * 12.0)))
        e.step(12 * out["settle_steps"])
        layouts, got = {}, {}

        def copy(name):
            w, h = rects[name]

            def f():
                got[name], _, layouts[name] = e.copy_words(x0, y0, w, h, return_layout=True)
                e.step(12)
            return f

        def old(name):
            w, h = rects[name]
            pw = (w + 63) // 64

            def f():
                got[name] = np.ascontiguousarray(e.store_words(y0, y0 + h)[:, x0 // 64:x0 // 64 + pw])
                e.step(12)
            return f
        same = {}
        for name, (w, h) in rects.items():  # the two routes agree (the old one keeps the bits past w of its last word)
            new, _ = e.copy_words(x0, y0, w, h)
            ref = e.store_words(y0, y0 + h)[:, x0 // 64:x0 // 64 + (w + 63) // 64].copy()
            if w % 64:
                ref[:, -1] &= np.uint64((1 << (w % 64)) - 1)
            same[name] = bool(np.array_equal(new, ref))
        out["routes_agree"] = same
        variants = []
        for name in rects:
            variants += [("copy_" + name, copy(name)), ("old_" + name, old(name))]
        variants += [("step12", lambda: e.step(12)), ("bounds_board", lambda: got.update(box=e.bounds())),
                     ("alive_count", lambda: got.update(alive=e.alive_count()))]
        ms = {name: [] for name, _ in variants}
        for rep in range(3 + a.reps):
            for name, fn in variants:
                t = timed(fn)
                if rep >= 3:
                    ms[name].append(t)
        out["ms"] = {name: summary(v) for name, v in ms.items()}
        step = out["ms"]["step12"]["median_ms"]
        out["minus_step_ms"] = {name: round(v["median_ms"] - step, 4) for name, v in out["ms"].items()
                                if name.startswith(("copy_", "old_"))}
        out["copy_layouts"] = layouts
        out["bounds_alive_equals_alive_count"] = got["box"][4] == got["alive"]
        out["box"] = list(got["box"])
    print(json.dumps(out))


if __name__ == "__main__":
    main()
