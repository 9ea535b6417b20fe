"""Histogram of the 4 x 3 neighbourhoods of a settled soup (CPU only; measurement data).

    python tools/nbhd_hist.py [--seed 1] [--size 1024] [--turns 700] [--out tests/golden/nbhd_hist_4x3.json]

Steps a seeded random soup on a size x size torus with the CPU oracle (oracle.bits_run) and counts,
over every cell position (y, x), the 12 cells of rows y-1 .. y+2 and columns x-1 .. x+1 (the
input of one column of the band pipeline's pair step, gol_pipe.h pstage: it emits rows y and y+1).
Index of a neighbourhood: bit 3 r + c is the cell of row y-1+r, column x-1+c.  The counts weight
the gate outputs of the rule circuits (tests/test_tail_polarity_cpu.py; tools/rule_search_pair.c
--hist ranks the truth tables of the pair tail by them): the timed steps of bench.py run on such
a board (4-5 % alive), so a gate's share of ones there is what the datapath carries.
The 3 x 3 neighbourhoods of the one-row rule are the margin over row y+2.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def histogram(cells):
    """(H, W) 0/1 cells of a torus -> 4096 counts, index bit 3 r + c = cell (y-1+r, x-1+c)."""
    idx = np.zeros(cells.shape, dtype=np.int64)
    for r in range(4):
        for c in range(3):
            idx |= np.roll(np.roll(cells, 1 - r, axis=0), 1 - c, axis=1).astype(np.int64) << (3 * r + c)
    return np.bincount(idx.ravel(), minlength=4096)


def main():
    from oracle import oracle as O
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--turns", type=int, default=700)
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "nbhd_hist_4x3.json"))
    a = ap.parse_args()
    words = O.bits_run(O.random_words(a.seed, 0, a.size, a.size // 64), a.turns)
    cells = (O.unpack(words) != 0).astype(np.uint8)
    counts = histogram(cells)
    doc = {"what": "counts of the 4 x 3 neighbourhoods (rows y-1..y+2, columns x-1..x+1) over every cell of a "
                   "settled random soup on a torus; index bit 3 r + c = cell (y-1+r, x-1+c)",
           "tool": "tools/nbhd_hist.py", "seed": a.seed, "height": a.size, "width": a.size, "turns": a.turns,
           "cells": int(cells.size), "alive": int(cells.sum()), "density": round(float(cells.mean()), 6),
           "counts": [int(x) for x in counts]}
    with open(a.out, "w") as f:
        json.dump(doc, f, separators=(",", ":"))
        f.write("\n")
    print("%s: %d cells, density %.4f, %d of 4096 neighbourhoods occur" %
          (os.path.relpath(a.out, ROOT), doc["cells"], doc["density"], int((counts > 0).sum())))


if __name__ == "__main__":
    main()
