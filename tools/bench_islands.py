#!/usr/bin/env python3
"""Time the island census of a batch (Batch.islands) against the two things it can be weighed by, and write
profiles/batch/bench_islands.jsonl (one JSON line per board shape and reach).

Per shape -- 65536 boards of 64 x 64 and 4096 boards of 512 x 512 by default -- the boards are soups run for
`--turns` turns with run_cycles (timed: the search that produced them).  Then, at reach 1 and 2:
  islands_s       the median of `--reps` calls of Batch.islands with `cap` records per board (after one warm-up
                  call, which allocates the handle's scratch);
  counts_only_s   the same with cap = 0: counts and fingerprints alone, no record leaves the device;
  host_s          the only other route: store_words of every board (timed whole) plus a loop of the host twin
                  (gol_batch_islands_host) over the first `host_boards` boards, scaled to all n boards -- the
                  loop is single-threaded and the sample keeps the tool short; host_sample_s is what was timed;
  vs_host, vs_search   host_s / islands_s and islands_s / search_s.
The host twin's counts and fingerprints of the sample are compared with the GPU's before anything is written.
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gol-distributed-final_amd"))

import numpy as np  # noqa: E402


def timed(f):
    t = time.perf_counter()
    r = f()
    return time.perf_counter() - t, r


def bench(G, n, side, turns, cap, host_boards, reps, seed):
    L = G.lib()
    with G.Batch(n, side, side, device=0) as b:
        b.load_soups(seed)
        search_s, (found, _) = timed(lambda: b.run_cycles(turns))
        store_s, words = timed(b.store_words)
        for reach in (1, 2):
            b.islands(reach=reach, cap=cap)  # warm-up: the scratch
            ts, t0s = [], []
            for _ in range(reps):
                t, (counts, recs, fps) = timed(lambda: b.islands(reach=reach, cap=cap, fingerprints=True))
                ts.append(t)
                t0s.append(timed(lambda: b.islands(reach=reach, cap=0, fingerprints=True))[0])
            m = min(host_boards, n)
            out = np.zeros(cap, dtype=G.ISLAND_DTYPE)
            hc, hf = np.zeros(m, dtype=np.int64), np.zeros(m, dtype=np.uint64)

            def host_loop():
                for i in range(m):
                    c, f = ctypes.c_int64(), ctypes.c_uint64()
                    rc = L.gol_batch_islands_host(side, side, reach, words[i].ctypes.data, words.shape[2], cap, ctypes.byref(c),
                                                  out.ctypes.data, ctypes.byref(f))
                    assert rc == 0
                    hc[i], hf[i] = c.value, f.value

            sample_s, _ = timed(host_loop)
            assert np.array_equal(hc, counts[:m]) and np.array_equal(hf, fps[:m]), "the host twin and the GPU differ"
            islands_s = statistics.median(ts)
            host_s = store_s + sample_s * n / m
            yield {"boards": n, "side": side, "turns": turns, "reach": reach, "cap": cap, "found": int((found >= 0).sum()),
                   "islands_mean": float(counts.mean()), "islands_max": int(counts.max()), "search_s": search_s,
                   "islands_s": islands_s, "counts_only_s": statistics.median(t0s), "store_words_s": store_s,
                   "host_boards": m, "host_sample_s": sample_s, "host_s": host_s, "vs_host": host_s / islands_s,
                   "vs_search": islands_s / search_s}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--turns", type=int, default=10000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--small", action="store_true", help="a quick pass over small batches (nothing is written)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "batch", "bench_islands.jsonl"))
    a = ap.parse_args()
    import golhip as G
    # (boards, side, cap, boards of the host sample)
    shapes = [(512, 64, 64, 64), (16, 512, 4096, 2)] if a.small else [(65536, 64, 64, 2048), (4096, 512, 4096, 16)]
    lines = []
    for n, side, cap, hb in shapes:
        for rec in bench(G, n, side, a.turns, cap, hb, a.reps, a.seed):
            print(json.dumps(rec), flush=True)
            lines.append(rec)
    if not a.small:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            for rec in lines:
                f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
