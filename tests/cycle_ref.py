"""Reference for the batch's cycle scan (helper of the survey tests, not a test).  The definition of
include/golhip.h, gol_batch_step_cycles, written out with the numpy stepper of rule_ref.py and a
brute-force list of the marks:

  t0 is the turn before the call, s(t) the state of a board at turn t.  The marks are m_j = t0 + 2^j - 1
  (t0, t0 + 1, t0 + 3, t0 + 7, ...).  For t = t0 + 1 .. t0 + turns, m(t) is the largest mark < t.  The
  board is found at the smallest t with s(t) == s(m(t)): found = t, period = t - m(t); a board never
  found has -1 in both.  (At a turn that is itself a mark the comparison uses the older mark.)
"""
import numpy as np

import rule_ref as R

# the rules of the survey tests: board i of a mixed batch runs under RULES[i % 18]
RULES = ["B3/S23", "B36/S23", "B3678/S34678", "B2/S", "B0/S8", "B1357/S1357", "B3/S012345678", "B/S", "B012345678/S012345678",
         "B34/S34", "B368/S245", "B2/S0", "B3/S", "B1/S1", "B45678/S2345", "B0/S", "B01/S01", "B35678/S5678"]

MARKS = [2 ** j - 1 for j in range(40)]  # relative to t0


def last_mark(d: int) -> int:
    """The largest mark < d (d >= 1, relative to t0), by search in the list."""
    return max(m for m in MARKS if m < d)


def scan(board, rule, turns: int, t0: int = 0):
    """(found, period, s(t0 + turns)) of one board of 0 / 1 under `rule` (text or mask pair)."""
    birth, survive = R.masks(rule) if isinstance(rule, str) else rule
    states = [(np.asarray(board) != 0).astype(np.uint8)]
    found = period = -1
    for d in range(1, turns + 1):
        states.append(R.step(states[-1], birth, survive))
        m = last_mark(d)
        if found < 0 and np.array_equal(states[d], states[m]):
            found, period = t0 + d, d - m
    return found, period, states[-1]


def scan_all(boards, rules, turns: int, t0: int = 0):
    """scan of every board; `rules` is one rule or one per board.  (found[n], period[n], final[n, H, W])."""
    if isinstance(rules, str) or (len(rules) == 2 and isinstance(rules[0], int)):
        rules = [rules] * len(boards)
    res = [scan(b, r, turns, t0) for b, r in zip(boards, rules)]
    return (np.array([f for f, _, _ in res], np.int64), np.array([p for _, p, _ in res], np.int64),
            np.stack([s for _, _, s in res]))


def place(H: int, W: int, rows, y: int = 0, x: int = 0) -> np.ndarray:
    """An H x W board of 0 / 1 with the pattern `rows` ("O" = alive) at (y, x), wrapping round the torus."""
    b = np.zeros((H, W), np.uint8)
    for dy, row in enumerate(rows):
        for dx, c in enumerate(row):
            if c == "O":
                b[(y + dy) % H, (x + dx) % W] = 1
    return b


GLIDER = [".O.", "..O", "OOO"]
R_PENTOMINO = [".OO", "OO.", ".O."]
BLOCK = ["OO", "OO"]
BLINKER = ["OOO"]
ROW10 = ["O" * 10]
PULSAR = ["..OOO...OOO..", ".............", "O....O.O....O", "O....O.O....O", "O....O.O....O", "..OOO...OOO..",
          ".............", "..OOO...OOO..", "O....O.O....O", "O....O.O....O", "O....O.O....O", ".............",
          "..OOO...OOO.."]
