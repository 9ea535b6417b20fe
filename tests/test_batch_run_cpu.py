"""Retirement of found boards, the part that needs no GPU: gol_batch_run_cycles_host (the scheme of
gol_batch_run_cycles on one board: the search in launches, the board retired at the end of the launch
it is found in, its remainder from the function the retire pass runs) against tests/cycle_ref.py and
the `made` formula of include/golhip.h, written out below; and the same code in the stand-alone
program under AddressSanitizer + UndefinedBehaviorSanitizer (build/asan/batch_check run, a plain child
process; nothing loaded into Python is sanitized).  All comparisons are exact, every expectation is
the reference's, and each test first asserts on the reference alone that its input exercises its case."""
import ctypes
import subprocess

import numpy as np
import pytest

import cycle_ref as C
import rule_ref as R
from batch_ref import GAP, PATTERNS, tail_mask, to_words
from testlib import check_program, cpu_lib as G  # noqa: F401 (the fixture)


def made_ref(found, period, turns, launch, t0=0):
    """The turns a board computes: to the end of the first launch that ends at t_L >= found, then
    (t0 + turns - t_L) mod period; all of them when it is never found."""
    if found < 0:
        return turns
    at = t0 + min(turns, launch * -(-(found - t0) // launch))
    return (at - t0) + (t0 + turns - at) % period


def run_host(G, cells, rule, turns, launch, pad=0, in_place=False, want_period=True, want_made=True):
    """gol_batch_run_cycles_host on rows Ww + pad words apart, every padding bit of the input set.
    Returns (rc, found, period, made, the buffer written)."""
    H, W = cells.shape
    Ww = (W + 63) // 64
    b, s = R.masks(rule) if isinstance(rule, str) else rule
    buf = np.full((H, Ww + pad), GAP, np.uint64)
    buf[:, :Ww] = to_words(cells)
    buf[:, Ww - 1] |= ~tail_mask(W)
    out = buf if in_place else np.full((H, Ww + pad), GAP, np.uint64)
    found, period, made = ctypes.c_int64(77), ctypes.c_int64(77), ctypes.c_int64(77)
    rc = G.lib().gol_batch_run_cycles_host(H, W, b, s, buf.ctypes.data, out.ctypes.data, Ww + pad, turns, launch,
                                           ctypes.byref(found), ctypes.byref(period) if want_period else None,
                                           ctypes.byref(made) if want_made else None)
    return rc, found.value, period.value, made.value, out


def check(G, cells, rule, turns, launch, want, pad=0, in_place=False):
    H, W = cells.shape
    Ww = (W + 63) // 64
    rc, found, period, made, out = run_host(G, cells, rule, turns, launch, pad, in_place)
    where = (H, W, rule, turns, launch, pad, in_place)
    assert rc == 0, G.lib().gol_last_error()
    assert (found, period) == want[:2], where
    assert made == made_ref(want[0], want[1], turns, launch), where
    assert np.array_equal(out[:, :Ww], to_words(want[2])), where
    assert np.all(out[:, Ww:] == GAP)
    return made


@pytest.mark.parametrize("k", range(len(PATTERNS)))
def test_run_host_known_patterns(G, k):
    cells, turns, stated = PATTERNS[k]
    want = C.scan(cells, R.CONWAY, turns)
    assert want[:2] == stated  # (the reference alone)
    for i, launch in enumerate((1, 5, 7, 64, turns)):
        made = check(G, cells, R.CONWAY, turns, launch, want, 2 * (i % 2), i % 3 == 1)
        assert stated[0] <= made <= turns


def test_run_host_soups(G):
    """24 soups of 16 x 16, 600 turns in launches of 7: every board leaves early, and the turns made are
    less than 0.4 of the turns step_cycles makes."""
    soups = [R.random_board(1000 + i, 16, 16, 0.35) for i in range(24)]
    want = [C.scan(b, R.CONWAY, 600) for b in soups]
    ref = [made_ref(f, p, 600, 7) for f, p, _ in want]
    assert all(f >= 0 for f, _, _ in want) and all(m < 600 for m in ref) and sum(ref) < 0.4 * 24 * 600
    got = [check(G, b, R.CONWAY, 600, 7, w, 2 * (i % 2), i % 3 == 0) for i, (b, w) in enumerate(zip(soups, want))]
    assert got == ref


def test_run_host_long_remainder(G):
    """The 7 x 9 glider (found 507, period 252) at 1100 turns: launches of 7 retire it at 511 with 85
    turns left, launches of 100 at 600 with 248."""
    cells = C.place(7, 9, C.GLIDER)
    want = C.scan(cells, R.CONWAY, 1100)
    assert want[:2] == (507, 252)
    assert (made_ref(507, 252, 1100, 7), (1100 - 511) % 252) == (596, 85)
    assert (made_ref(507, 252, 1100, 100), (1100 - 600) % 252) == (848, 248)
    assert check(G, cells, R.CONWAY, 1100, 7, want) == 596
    assert check(G, cells, R.CONWAY, 1100, 100, want, 1, True) == 848


def test_run_host_other_rules(G):
    """One 5 x 33 soup under 18 rules, 300 turns in launches of 7: five boards never found (they make every
    turn), and one of period 28 with 27 turns left."""
    b = R.random_board(4243, 5, 33, 0.4)
    want = [C.scan(b, r, 300) for r in C.RULES]
    assert sum(f < 0 for f, _, _ in want) == 5
    long = [f for f, p, _ in want if p == 28]
    assert len(long) == 1 and (300 - 7 * -(-long[0] // 7)) % 28 == 27
    for i, (r, w) in enumerate(zip(C.RULES, want)):
        made = check(G, b, r, 300, 7, w, 1, i % 2 == 0)
        if w[0] < 0:
            assert made == 300


def test_run_host_stride_and_in_place(G):
    """Rows three words apart with the padding bits of the input set, out of place and in place."""
    cells = R.random_board(73, 9, 70, 0.4)
    want = C.scan(cells, R.CONWAY, 200)
    assert want[0] > 7 and made_ref(want[0], want[1], 200, 7) < 200
    for in_place in (False, True):
        check(G, cells, R.CONWAY, 200, 7, want, 1, in_place)


def test_run_host_zero_turns_and_null_outputs(G):
    cells = R.random_board(9, 5, 70, 0.5)
    rc, found, period, made, out = run_host(G, cells, R.CONWAY, 0, 7, pad=1)
    assert (rc, found, period, made) == (0, -1, -1, 0)
    assert np.array_equal(out[:, :2], to_words(cells)) and np.all(out[:, 2:] == GAP)  # the board, its padding cleared
    blinker = C.place(5, 5, C.BLINKER, 2, 1)
    assert C.scan(blinker, R.CONWAY, 10)[:2] == (3, 2)
    assert run_host(G, blinker, R.CONWAY, 10, 4, want_period=False)[:4] == (0, 3, 77, 4)
    assert run_host(G, blinker, R.CONWAY, 10, 4, want_made=False)[:4] == (0, 3, 2, 77)
    assert run_host(G, blinker, R.CONWAY, 11, 4)[:4] == (0, 3, 2, 5)


def test_run_host_einval(G):
    L = G.lib()
    buf = np.zeros((8, 9), np.uint64)
    out = np.full((8, 9), GAP, np.uint64)
    found, period, made = ctypes.c_int64(77), ctypes.c_int64(77), ctypes.c_int64(77)
    f, p, m = ctypes.byref(found), ctypes.byref(period), ctypes.byref(made)
    i, o = buf.ctypes.data, out.ctypes.data
    run = L.gol_batch_run_cycles_host
    bad = [run(0, 8, 8, 12, i, o, 1, 1, 1, f, p, m), run(8, 0, 8, 12, i, o, 1, 1, 1, f, p, m),
           run(513, 8, 8, 12, i, o, 1, 1, 1, f, p, m), run(8, 513, 8, 12, i, o, 9, 1, 1, f, p, m),
           run(-1, 8, 8, 12, i, o, 1, 1, 1, f, p, m), run(8, 8, 512, 12, i, o, 1, 1, 1, f, p, m),
           run(8, 8, 8, 512, i, o, 1, 1, 1, f, p, m), run(8, 65, 8, 12, i, o, 1, 1, 1, f, p, m),
           run(8, 512, 8, 12, i, o, 7, 1, 1, f, p, m), run(8, 8, 8, 12, i, o, 0, 1, 1, f, p, m),
           run(8, 8, 8, 12, None, o, 1, 1, 1, f, p, m), run(8, 8, 8, 12, i, None, 1, 1, 1, f, p, m),
           run(8, 8, 8, 12, i, o, 1, -1, 1, f, p, m), run(8, 8, 8, 12, i, o, 1, 1, 1, None, p, m),
           run(8, 8, 8, 12, i, o, 1, 1, 0, f, p, m), run(8, 8, 8, 12, i, o, 1, 1, -3, f, p, m)]
    assert bad == [-1] * len(bad)
    assert L.gol_last_error()
    assert np.all(out == GAP) and (found.value, period.value, made.value) == (77, 77, 77)
    assert run(8, 512, 8, 12, i, o, 8, 1, 1, f, p, m) == 0 and (found.value, period.value, made.value) == (1, 1, 1)


def test_batch_check_run_under_sanitizers():
    """gol_batch_run_cycles_host in the stand-alone program, every buffer a heap block of its exact size,
    against gol_batch_cycles_host over a grid of shapes, turns and launch lengths."""
    r = subprocess.run([check_program("batch_check"), "run"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "batch_check run:" in r.stdout and " 0 bad" in r.stdout
