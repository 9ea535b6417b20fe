"""The cycle scan of the batch, the part that needs no GPU: gol_batch_cycles_host (the kernel's turn
and the mark arithmetic of csrc/gol_batch.h on host memory) against tests/cycle_ref.py, which holds
the definition, on patterns of known period and on soups, out of place and in place, with a row
stride above ceil(W / 64) and the padding bits of the input set; the marks at every turn up to 1100;
the refusals; and the same code in the stand-alone program under AddressSanitizer +
UndefinedBehaviorSanitizer (build/asan/batch_check cycles, a plain child process; nothing loaded into
Python is sanitized).  All comparisons are exact, and every expectation is the reference's."""
import ctypes
import subprocess

import numpy as np
import pytest

import cycle_ref as C
import rule_ref as R
from batch_ref import GAP, PATTERNS, tail_mask, to_words
from testlib import check_program, cpu_lib as G  # noqa: F401 (the fixture)


def cycles_host(G, cells, rule, turns, pad=0, in_place=False, want_period=True):
    """gol_batch_cycles_host on rows Ww + pad words apart, every padding bit of the input set.
    Returns (rc, found, period, the buffer written)."""
    H, W = cells.shape
    Ww = (W + 63) // 64
    b, s = R.masks(rule) if isinstance(rule, str) else rule
    buf = np.full((H, Ww + pad), GAP, np.uint64)
    buf[:, :Ww] = to_words(cells)
    buf[:, Ww - 1] |= ~tail_mask(W)
    out = buf if in_place else np.full((H, Ww + pad), GAP, np.uint64)
    found, period = ctypes.c_int64(77), ctypes.c_int64(77)
    rc = G.lib().gol_batch_cycles_host(H, W, b, s, buf.ctypes.data, out.ctypes.data, Ww + pad, turns, ctypes.byref(found),
                                       ctypes.byref(period) if want_period else None)
    return rc, found.value, period.value, out


def check(G, cells, rule, turns, want, pad, in_place):
    H, W = cells.shape
    Ww = (W + 63) // 64
    rc, found, period, out = cycles_host(G, cells, rule, turns, pad, in_place)
    assert rc == 0, G.lib().gol_last_error()
    assert (found, period) == want[:2], (H, W, rule, turns, pad, in_place)
    assert np.array_equal(out[:, :Ww], to_words(want[2])), (H, W, rule, turns, pad, in_place)
    assert np.all(out[:, Ww:] == GAP)


@pytest.mark.parametrize("k", range(len(PATTERNS)))
def test_cycles_host_known_patterns(G, k):
    cells, turns, stated = PATTERNS[k]
    want = C.scan(cells, R.CONWAY, turns)
    assert want[:2] == stated  # (the reference alone: the pattern has the period it is here for)
    check(G, cells, R.CONWAY, turns, want, 0, False)
    check(G, cells, R.CONWAY, turns, want, 2, True)


def test_cycles_host_soups(G):
    """24 soups of 16 x 16, 600 turns: all found, the latest at 512, as still lifes or period 2."""
    soups = [R.random_board(1000 + i, 16, 16, 0.35) for i in range(24)]
    want = [C.scan(b, R.CONWAY, 600) for b in soups]
    assert all(f >= 0 for f, _, _ in want) and max(f for f, _, _ in want) == 512 and {p for _, p, _ in want} == {1, 2}
    for i, (b, w) in enumerate(zip(soups, want)):
        check(G, b, R.CONWAY, 600, w, 2 * (i % 2), i % 3 == 0)


def test_cycles_host_other_rules(G):
    """One 5 x 33 soup under 18 rules: periods 1, 2, 4 and 28, and five boards never found."""
    b = R.random_board(4243, 5, 33, 0.4)
    want = [C.scan(b, r, 300) for r in C.RULES]
    assert {p for _, p, _ in want} == {-1, 1, 2, 4, 28} and sum(f < 0 for f, _, _ in want) == 5
    for i, (r, w) in enumerate(zip(C.RULES, want)):
        check(G, b, r, 300, w, 1, i % 2 == 0)


def test_marks_up_to_1100(G):
    """The marks against a brute-force list: the reference's own list first, then the library through
    boards found at many different turns -- an empty board (found 1, period 1 whatever the turns),
    gliders whose period 4 lcm(H, W) puts found = the first mark >= the period + the period -- and a board
    never found, whose snapshot changes at every mark up to 1100."""
    marks = [d for d in range(1101) if bin(d + 1).count("1") == 1]
    assert marks == [0, 1, 3, 7, 15, 31, 63, 127, 255, 511, 1023] == [m for m in C.MARKS if m <= 1100]
    for d in range(1, 1101):
        assert C.last_mark(d) == max(m for m in marks if m < d)
    for turns in (1, 2, 1100):
        assert cycles_host(G, np.zeros((3, 3), np.uint8), R.CONWAY, turns)[:3] == (0, 1, 1)
    seen = set()
    for H, W in [(5, 5), (5, 6), (6, 7), (5, 7), (7, 8), (8, 9), (9, 10), (10, 11)]:
        cells = C.place(H, W, C.GLIDER)
        want = C.scan(cells, R.CONWAY, 1100)
        period = 4 * np.lcm(H, W)
        assert want[:2] == (min(m for m in marks if m + 1 >= period) + period, period)
        seen.add(want[0])
        check(G, cells, R.CONWAY, 1100, want, 0, False)
    assert len(seen) == 8 and max(seen) == 951
    # every turn of a call is compared: a glider found at 507 is not found in 506 turns
    cells = C.place(7, 9, C.GLIDER)
    check(G, cells, R.CONWAY, 506, C.scan(cells, R.CONWAY, 506), 0, False)
    assert C.scan(cells, R.CONWAY, 506)[:2] == (-1, -1)
    chaos = R.random_board(4242, 16, 16, 0.35)  # B2/S: never repeats within 1100 turns
    want = C.scan(chaos, "B2/S", 1100)
    assert want[:2] == (-1, -1)
    check(G, chaos, "B2/S", 1100, want, 0, True)


def test_cycles_host_zero_turns_and_null_period(G):
    cells = R.random_board(9, 5, 70, 0.5)
    rc, found, period, out = cycles_host(G, cells, R.CONWAY, 0, pad=1)
    assert (rc, found, period) == (0, -1, -1)
    assert np.array_equal(out[:, :2], to_words(cells)) and np.all(out[:, 2:] == GAP)  # the board, its padding cleared
    rc, found, period, _ = cycles_host(G, C.place(5, 5, C.BLINKER, 2, 1), R.CONWAY, 10, want_period=False)
    assert (rc, found, period) == (0, 3, 77)


def test_cycles_host_einval(G):
    L = G.lib()
    buf = np.zeros((8, 9), np.uint64)
    out = np.full((8, 9), GAP, np.uint64)
    found, period = ctypes.c_int64(77), ctypes.c_int64(77)
    f, p = ctypes.byref(found), ctypes.byref(period)
    i, o = buf.ctypes.data, out.ctypes.data
    bad = [L.gol_batch_cycles_host(0, 8, 8, 12, i, o, 1, 1, f, p), L.gol_batch_cycles_host(8, 0, 8, 12, i, o, 1, 1, f, p),
           L.gol_batch_cycles_host(513, 8, 8, 12, i, o, 1, 1, f, p), L.gol_batch_cycles_host(8, 513, 8, 12, i, o, 9, 1, f, p),
           L.gol_batch_cycles_host(-1, 8, 8, 12, i, o, 1, 1, f, p), L.gol_batch_cycles_host(8, 8, 512, 12, i, o, 1, 1, f, p),
           L.gol_batch_cycles_host(8, 8, 8, 512, i, o, 1, 1, f, p), L.gol_batch_cycles_host(8, 65, 8, 12, i, o, 1, 1, f, p),
           L.gol_batch_cycles_host(8, 512, 8, 12, i, o, 7, 1, f, p), L.gol_batch_cycles_host(8, 8, 8, 12, i, o, 0, 1, f, p),
           L.gol_batch_cycles_host(8, 8, 8, 12, None, o, 1, 1, f, p), L.gol_batch_cycles_host(8, 8, 8, 12, i, None, 1, 1, f, p),
           L.gol_batch_cycles_host(8, 8, 8, 12, i, o, 1, -1, f, p), L.gol_batch_cycles_host(8, 8, 8, 12, i, o, 1, 1, None, p)]
    assert bad == [-1] * len(bad)
    assert L.gol_last_error()
    assert np.all(out == GAP) and (found.value, period.value) == (77, 77)
    assert L.gol_batch_cycles_host(8, 512, 8, 12, i, o, 8, 1, f, p) == 0 and (found.value, period.value) == (1, 1)


def test_batch_check_cycles_under_sanitizers():
    """gol_batch_cycles_host in the stand-alone program, every buffer a heap block of its exact size,
    against a scan written in the program itself; without an argument the program runs what it ran
    before."""
    r = subprocess.run([check_program("batch_check"), "cycles"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "batch_check cycles:" in r.stdout and " 0 bad" in r.stdout
    r = subprocess.run([check_program("batch_check"), "no-such-mode"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 2
