#!/usr/bin/env python
"""Viewport frames against the only other route to the same cells ("Viewport frames").

On a band-layout N x N board (default 65536), after load_random and ~0.6 s of settle steps
(DESIGN.md §6), times with a host clock around the blocking calls, 3 warm-ups and then --reps
repetitions with the variants alternating:

  view_s<k>   Engine.view(x0, y0, k, 1920, 1080) for k = 1, 8, 32 (the board stays in the band layout);
              view_s1_again is the scale-1 view repeated at once
  step12      a plain step(12)
  old_s<k>    store_rows(y0, y0 + 1080 k) followed by step(12): the store converts the whole board
              to the standard layout and the step converts it back; its cost for the picture is
              old_s<k> - step12 (--old-scales, default 1 and 8: at 32 the rows are 2.2 GB of bytes)

and then the scale-1 view (alternating with step12) on a --small board (default 16384^2): if the
work follows the viewport and not the board, the two scale-1 times agree within their spread.
Prints one JSON line.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "gol-distributed-final_amd")]

OUT_W, OUT_H = 1920, 1080


def summary(ms):
    s = sorted(ms)
    return {"median_ms": round(statistics.median(s), 4), "min_ms": round(s[0], 4), "max_ms": round(s[-1], 4),
            "p25_ms": round(s[len(s) // 4], 4), "p75_ms": round(s[(3 * len(s)) // 4], 4), "n": len(s)}


def timed(fn):
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e3


def settle(e, n, seconds):
    steps = max(1, round(seconds * 145e12 / (n * n * 12.0)))
    e.step(12 * steps)
    return steps


def run_board(golhip, n, scales, old_scales, reps, settle_s):
    x0, y0 = n // 3 + 5, n // 2 + 3  # no multiple of a word or a band
    res = {"board": n}
    with golhip.Engine(n, n, layout="band", device=0) as e:
        e.load_random(1)
        res["settle_steps"] = settle(e, n, settle_s)
        layouts = {}

        def view(k):
            def f():
                _, layouts[k] = e.view(x0, y0, k, OUT_W, OUT_H, return_layout=True)
            return f

        def old(k):
            def f():
                e.store_rows(y0, y0 + OUT_H * k)
                e.step(12)
            return f
        # every round: the old routes, a plain step, then the views -- on both boards the scale-1 view
        # follows a plain step (right after the 566 MB store of old_s8 it measured 0.06 ms slower: the
        # host's caches and allocator, not the GPU)
        variants = [("old_s%d" % k, old(k)) for k in old_scales]
        variants.append(("step12", lambda: e.step(12)))
        for k in scales:
            variants.append(("view_s%d" % k, view(k)))
            if k == 1:  # the same view again at once: what the first view after a step pays for coming first
                variants.append(("view_s1_again", view(1)))
        ms = {name: [] for name, _ in variants}
        for rep in range(3 + reps):
            for name, fn in variants:
                t = timed(fn)
                if rep >= 3:
                    ms[name].append(t)
        res["ms"] = {name: summary(v) for name, v in ms.items()}
        res["view_layouts"] = {str(k): v for k, v in layouts.items()}
        step = res["ms"]["step12"]["median_ms"]
        res["old_route_minus_step_ms"] = {str(k): round(res["ms"]["old_s%d" % k]["median_ms"] - step, 4)
                                          for k in old_scales}
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--board", type=int, default=65536)
    ap.add_argument("--small", type=int, default=16384)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--settle-s", type=float, default=0.6)
    ap.add_argument("--old-scales", type=int, nargs="*", default=[1, 8])
    a = ap.parse_args()
    import golhip
    out = {"tool": "bench_view", "viewport": [OUT_W, OUT_H], "reps": a.reps,
           "big": run_board(golhip, a.board, [1, 8, 32], a.old_scales, a.reps, a.settle_s),
           "small": run_board(golhip, a.small, [1], [], a.reps, a.settle_s)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
