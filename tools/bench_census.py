#!/usr/bin/env python
"""The tally of island kinds against the calls it extends, written to
profiles/batch/bench_census.jsonl (one JSON line per board shape and reach).

Per shape -- 65536 slots of 64 x 64 over 2^20 soups and 4096 slots of 512 x 512 over 16384 soups by default,
horizon 10000 -- in one process on one GPU, by the method of tools/bench_retire.py: --settle-s seconds of batch
steps first, one warm-up of every variant, then --reps repetitions with the variants alternating, host clock
round the blocking calls, medians with minimum and maximum.

  search / census          Batch.search and Batch.census of the same soups: what the census inside the harvest adds.
  islands0 / islands64 / islands_tally
                           on the boards run_cycles(horizon) leaves: Batch.islands with cap 0 (counts and
                           fingerprints alone) and cap 64 (64 records per board brought back), and
                           Batch.islands_tally (the kinds instead of the records).

Before the timing the tool checks that census returns search's four outputs, and that islands_tally returns the
counts and fingerprints of islands and the tally of its records where no board holds more than the cap.  It
reports the distinct kinds, the share of the commonest kind among all islands, and `dropped` (0: the call would
have raised otherwise; the table is sized by --kinds, doubled when it is full).
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "gol-distributed-final_amd")]

SHAPES = [(64, 65536, 1 << 20), (512, 4096, 16384)]  # side, slots, soups
SMALL = [(64, 512, 4096), (512, 16, 32)]


def timed(call):
    t0 = time.perf_counter()
    res = call()
    return time.perf_counter() - t0, res


def alternate(variants, reps):
    """{name: seconds[reps]} of the variants run in turn, after one warm-up round."""
    secs = {name: [] for name, _ in variants}
    for rep in range(1 + reps):
        for name, call in variants:
            t = timed(call)[0]
            if rep >= 1:
                secs[name].append(t)
    return secs


def summary(secs):
    return {"median_s": {k: round(statistics.median(v), 6) for k, v in secs.items()},
            "min_s": {k: round(min(v), 6) for k, v in secs.items()}, "max_s": {k: round(max(v), 6) for k, v in secs.items()}}


def ratio(secs, a, b):
    return {"median": round(statistics.median(secs[a]) / statistics.median(secs[b]), 4),
            "min_max": [round(min(secs[a]) / max(secs[b]), 4), round(max(secs[a]) / min(secs[b]), 4)]}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--horizon", type=int, default=10000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--kinds", type=int, default=1 << 16)
    ap.add_argument("--settle-s", type=float, default=0.5)
    ap.add_argument("--small", action="store_true", help="a quick pass over small batches")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "batch", "bench_census.jsonl"))
    a = ap.parse_args()
    import numpy as np

    import golhip
    for side, n, total in SMALL if a.small else SHAPES:
        with golhip.Batch(n, side, side, device=0) as b:
            b.load_random(a.seed)
            t_end = time.perf_counter() + a.settle_s
            while time.perf_counter() < t_end:
                b.step(100)
            for reach in (1, 2):
                kinds = a.kinds
                while True:  # a table that holds the kinds
                    try:
                        got = b.census(a.seed, total, a.horizon, reach=reach, kinds=kinds)
                        break
                    except golhip.GolError as e:
                        if "ENOMEM" not in str(e) or kinds >= 1 << 23:
                            raise
                        kinds *= 2
                ref = b.search(a.seed, total, a.horizon)
                same = all(np.array_equal(got[k], r) for k, r in zip(("found", "period", "alive", "hash"), ref))
                secs = alternate([("search", lambda: b.search(a.seed, total, a.horizon)),
                                  ("census", lambda: b.census(a.seed, total, a.horizon, reach=reach, kinds=kinds))], a.reps)
                islands = int(got["islands"].sum())
                out = {"tool": "bench_census", "side": side, "slots": n, "soups": total, "horizon": a.horizon, "reach": reach,
                       "reps": a.reps, "kinds_cap": kinds, "calls_agree": bool(same), "found": int((got["found"] >= 0).sum()),
                       "islands": islands, "n_kinds": got["n_kinds"], "dropped": 0,
                       "top_kind": {k: int(got["kinds"][0][k]) for k in ("hash", "count", "first", "cells", "rows", "cols")} if islands else None,
                       "top_share": round(int(got["kinds"][0]["count"]) / islands, 4) if islands else 0.0,
                       "search": dict(summary(secs), census_over_search=ratio(secs, "census", "search"))}
                # the boards as they stand after run_cycles
                b.load_soups(a.seed)
                b.run_cycles(a.horizon)
                counts, fps, tk = b.islands_tally(reach=reach, kinds=kinds)
                c64, recs, f64 = b.islands(reach=reach, cap=64, fingerprints=True)
                agree = bool(np.array_equal(counts, c64) and np.array_equal(fps, f64))
                if c64.max() <= 64:  # the records are all there: their tally
                    hs, cs = np.unique(recs["hash"][np.arange(64)[None, :] < c64[:, None]], return_counts=True)
                    order = np.argsort(tk["hash"])
                    agree = agree and np.array_equal(hs, tk["hash"][order]) and np.array_equal(cs, tk["count"][order])
                secs = alternate([("islands0", lambda: b.islands(reach=reach, cap=0, fingerprints=True)),
                                  ("islands64", lambda: b.islands(reach=reach, cap=64, fingerprints=True)),
                                  ("islands_tally", lambda: b.islands_tally(reach=reach, kinds=kinds))], a.reps)
                out["standing"] = dict(summary(secs), calls_agree=agree, islands=int(counts.sum()), n_kinds=len(tk),
                                       top_share=round(int(tk[0]["count"]) / max(int(counts.sum()), 1), 4) if len(tk) else 0.0,
                                       tally_over_islands0=ratio(secs, "islands_tally", "islands0"),
                                       tally_over_islands64=ratio(secs, "islands_tally", "islands64"))
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
