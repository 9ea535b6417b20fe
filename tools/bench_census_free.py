#!/usr/bin/env python
"""What the free hash costs: the census and the standing tally with symmetry ISLAND_FIXED and ISLAND_FREE in turn
(DESIGN.md §4.25), written to profiles/batch/bench_census_free.jsonl (one JSON line per board shape and reach).

The shapes and the method are those of tools/bench_census.py (§4.24): 65536 slots of 64 x 64 over 2^20 soups and
4096 slots of 512 x 512 over 16384 soups, horizon 10000, in one process on one GPU, --settle-s seconds of batch
steps first, one warm-up of every variant, then --reps repetitions with the variants alternating, host clock
round the blocking calls, medians with minimum and maximum.

  census_fixed / census_free   Batch.census of the same soups with either symmetry.
  tally_fixed / tally_free     Batch.islands_tally on the boards run_cycles(horizon) leaves.

Before the timing the tool checks that the two censuses agree on found, period, alive, hash and the island counts,
that both tallies hold every island, and that the free tally is the fixed one with lines merged (no more kinds, the
same islands).  It reports the kinds FIXED and FREE, the block's share of all islands, and FREE / FIXED per call.

--fixed-only times the FIXED calls alone, through the entries without _sym: with --library it measures another
build of libgolhip.so (one that may lack the _sym entries) for a comparison of what both builds have.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "gol-distributed-final_amd"), os.path.join(ROOT, "tools")]

from bench_census import SHAPES, SMALL, alternate, ratio, summary  # noqa: E402

BLOCK = "x = 2, y = 2\n2o$2o!"
FIXED, FREE = 0, 1


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--horizon", type=int, default=10000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--kinds", type=int, default=1 << 16)
    ap.add_argument("--settle-s", type=float, default=0.5)
    ap.add_argument("--small", action="store_true", help="a quick pass over small batches")
    ap.add_argument("--fixed-only", action="store_true", help="the FIXED calls alone (a build without the _sym entries)")
    ap.add_argument("--library", default="", help="another build of libgolhip.so (with --fixed-only)")
    ap.add_argument("--label", default="", help="a name for the build, copied into every line")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "batch", "bench_census_free.jsonl"))
    a = ap.parse_args()
    import time

    import numpy as np

    import golhip
    if a.library:
        if not a.fixed_only:
            sys.exit("--library goes with --fixed-only")
        golhip._lib._lib = golhip._lib.load(os.path.abspath(a.library), strict=False)
    syms = (FIXED,) if a.fixed_only else (FIXED, FREE)
    name = {FIXED: "fixed", FREE: "free"}
    for side, n, total in SMALL if a.small else SHAPES:
        with golhip.Batch(n, side, side, device=0) as b:
            b.load_random(a.seed)
            t_end = time.perf_counter() + a.settle_s
            while time.perf_counter() < t_end:
                b.step(100)
            for reach in (1, 2):
                kinds = a.kinds
                while True:  # a table that holds the kinds (the fixed tally has the most)
                    try:
                        got = {s: b.census(a.seed, total, a.horizon, reach=reach, kinds=kinds, symmetry=s) for s in syms}
                        break
                    except golhip.GolError as e:
                        if "ENOMEM" not in str(e) or kinds >= 1 << 23:
                            raise
                        kinds *= 2
                islands = int(got[FIXED]["islands"].sum())
                same = all(int(g["kinds"]["count"].sum()) == islands for g in got.values())
                out = {"tool": "bench_census_free", "build": a.label, "side": side, "slots": n, "soups": total, "horizon": a.horizon,
                       "reach": reach, "reps": a.reps, "kinds_cap": kinds, "found": int((got[FIXED]["found"] >= 0).sum()),
                       "islands": islands, "n_kinds": {name[s]: got[s]["n_kinds"] for s in syms}}
                if not a.fixed_only:
                    same = same and all(np.array_equal(got[FIXED][k], got[FREE][k]) for k in ("found", "period", "alive", "hash", "islands"))
                    same = same and got[FREE]["n_kinds"] <= got[FIXED]["n_kinds"]
                    block = int(golhip.island(BLOCK, reach, symmetry=FREE)["hash"])
                    at = np.nonzero(got[FREE]["kinds"]["hash"] == np.uint64(block))[0]
                    out["block_share"] = round(int(got[FREE]["kinds"]["count"][at[0]]) / islands, 4) if len(at) and islands else 0.0
                    out["top_kinds_free"] = [{k: int(r[k]) for k in ("hash", "count", "first", "cells", "rows", "cols")}
                                             for r in got[FREE]["kinds"][:8]]
                secs = alternate([(f"census_{name[s]}", lambda s=s: b.census(a.seed, total, a.horizon, reach=reach, kinds=kinds, symmetry=s))
                                  for s in syms], a.reps)
                out["search"] = summary(secs)
                if not a.fixed_only:
                    out["search"]["free_over_fixed"] = ratio(secs, "census_free", "census_fixed")
                # the boards as they stand after run_cycles
                b.load_soups(a.seed)
                b.run_cycles(a.horizon)
                tal = {s: b.islands_tally(reach=reach, kinds=kinds, symmetry=s) for s in syms}
                standing = int(tal[FIXED][0].sum())
                agree = all(int(t[2]["count"].sum()) == standing for t in tal.values())
                if not a.fixed_only:
                    agree = agree and np.array_equal(tal[FIXED][0], tal[FREE][0]) and len(tal[FREE][2]) <= len(tal[FIXED][2])
                secs = alternate([(f"tally_{name[s]}", lambda s=s: b.islands_tally(reach=reach, kinds=kinds, symmetry=s)) for s in syms],
                                 a.reps)
                out["standing"] = dict(summary(secs), islands=standing, n_kinds={name[s]: len(tal[s][2]) for s in syms})
                if not a.fixed_only:
                    out["standing"]["free_over_fixed"] = ratio(secs, "tally_free", "tally_fixed")
                out["calls_agree"] = bool(same and agree)
                line = json.dumps(out)
                print(line, flush=True)
                if a.out:
                    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
                    with open(a.out, "a") as f:
                        f.write(line + "\n")
                if not (same and agree):
                    sys.exit("the calls disagree")


if __name__ == "__main__":
    main()
