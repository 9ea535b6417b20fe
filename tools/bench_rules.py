#!/usr/bin/env python
"""Life-like rules on the rule kernels against the B3/S23 kernels.

On one GPU, after load_random and ~0.6 s of settle steps per engine, times
step(--turns) with a host clock around the blocking call, 3 warm-ups and then --reps repetitions
with the variants alternating:

  band_default       16384^2, band layout, B3/S23 on the default path (the k = 12 pipeline)
  band_generic       the same board, B3/S23 with GOL_RULE_GENERIC (the rule kernels, k = 8)
  band_b36s23        the same board, B36/S23
  standard_generic   16384 x 16320 (W % 1024 != 0: standard layout), B3/S23 with GOL_RULE_GENERIC
  standard_b36s23    the same board, B36/S23

and reports T cell-updates/s from the median.  Prints one JSON line.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "gol-distributed-final_amd")]

VARIANTS = [
    ("band_default", 16384, 16384, "B3/S23", False),
    ("band_generic", 16384, 16384, "B3/S23", True),
    ("band_b36s23", 16384, 16384, "B36/S23", False),
    ("standard_generic", 16384, 16320, "B3/S23", True),
    ("standard_b36s23", 16384, 16320, "B36/S23", False),
]


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--turns", type=int, default=240, help="turns per timed call (a multiple of 24: whole k = 12 and k = 8 launches)")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--settle-s", type=float, default=0.6)
    a = ap.parse_args()
    import golhip
    engines, info = [], {}
    for name, H, W, rule, generic in VARIANTS:
        e = golhip.Engine(H, W, device=0)
        e.load_random(1)
        e.set_rule(rule, generic=generic)
        assert e.rule_generic == (generic or rule != "B3/S23")
        i = e.info()
        info[name] = {"board": [H, W], "rule": e.rule, "generic": e.rule_generic, "layout": i["layout"],
                      "turns_per_launch": i["turns_per_launch"], "cells_per_lane": i["cells_per_lane"]}
        # settle: ~settle_s of stepping (a first guess of the rate from a short run)
        t0 = time.perf_counter()
        e.step(a.turns)
        per_turn = (time.perf_counter() - t0) / a.turns
        e.step(max(a.turns, int(a.settle_s / per_turn) // 24 * 24))
        engines.append((name, e, H * W))
    ms = {name: [] for name, _, _ in engines}
    for rep in range(3 + a.reps):
        for name, e, _ in engines:
            t0 = time.perf_counter()
            e.step(a.turns)
            t = (time.perf_counter() - t0) * 1e3
            if rep >= 3:
                ms[name].append(t)
    out = {"tool": "bench_rules", "turns": a.turns, "reps": a.reps, "variants": {}}
    for name, e, cells in engines:
        s = sorted(ms[name])
        rate = lambda x: round(cells * a.turns / (x * 1e-3) / 1e12, 3)  # noqa: E731
        out["variants"][name] = dict(info[name], median_ms=round(statistics.median(s), 4), min_ms=round(s[0], 4),
                                     max_ms=round(s[-1], 4), T_cell_updates_per_s=rate(statistics.median(s)),
                                     T_best=rate(s[0]), T_worst=rate(s[-1]))
        e.close()
    base = out["variants"]["band_default"]["T_cell_updates_per_s"]
    out["relative_to_band_default"] = {n: round(v["T_cell_updates_per_s"] / base, 4) for n, v in out["variants"].items()}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
