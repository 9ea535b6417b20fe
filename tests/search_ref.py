"""Reference for the soup search (helper of the search tests, not a test).  The definition of
include/golhip.h, gol_batch_search, from parts that are not the code under test:

  soup g of (seed, H, W) = the oracle's random_words(seed, g*H, H, Ww) with the padding cleared;
  found and period = cycle_ref.scan of the soup over `horizon` turns from t0 = 0;
  alive and hash = the oracle's popcount and hash of s(found), the state the numpy stepper of
  rule_ref.py reaches after `found` turns; -1, -1, 0, 0 for a soup the scan does not find.

A result is computed once per (seed, first, total, H, W, rule, horizon) and shared; the arrays are
read-only."""
import functools

import numpy as np

import cycle_ref as C
import rule_ref as R
from batch_ref import from_words, tail_mask, to_words
from oracle import oracle as O


def soup_words(seed: int, g: int, H: int, W: int) -> np.ndarray:
    """uint64[H, ceil(W / 64)]: the words of soup g."""
    Ww = (W + 63) // 64
    w = O.random_words(seed, g * H, H, Ww)
    w[:, Ww - 1] &= tail_mask(W)
    return w


def soup_cells(seed: int, g: int, H: int, W: int) -> np.ndarray:
    """uint8[H, W] of 0 / 1."""
    return from_words(soup_words(seed, g, H, W), W)


@functools.lru_cache(maxsize=None)
def one(seed: int, g: int, H: int, W: int, rule: str, horizon: int):
    """(found, period, alive, hash) of soup g."""
    cells = soup_cells(seed, g, H, W)
    found, period, _ = C.scan(cells, rule, horizon)
    if found < 0:
        return -1, -1, 0, 0
    words = to_words(R.run(cells, rule, found)[0])
    return found, period, O.popcount_words(words), O.hash_words(words)


@functools.lru_cache(maxsize=None)
def search(seed: int, first: int, total: int, H: int, W: int, rule: str, horizon: int):
    """(found int64[total], period int64[total], alive uint64[total], hash uint64[total]), read-only."""
    res = [one(seed, first + i, H, W, rule, horizon) for i in range(total)]
    out = (np.array([r[0] for r in res], np.int64), np.array([r[1] for r in res], np.int64),
           np.array([r[2] for r in res], np.uint64), np.array([r[3] for r in res], np.uint64))
    for a in out:
        a.setflags(write=False)
    return out
