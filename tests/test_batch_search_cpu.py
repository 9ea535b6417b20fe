"""The soup search, the part that needs no GPU: gol_batch_soup_host (the word function of the fill kernels),
gol_batch_verdict_host (the restock pass's verdict) and gol_batch_search_host (the scheme of gol_batch_search:
slots, launches, the restock pass and the census of the kept snapshot) against tests/search_ref.py; and
the same code in the stand-alone program under AddressSanitizer + UndefinedBehaviorSanitizer
(build/asan/batch_check search, a plain child process; nothing loaded into Python is sanitized).  All
comparisons are exact, every expectation is the reference's, and the main case first asserts on the
reference alone that it cannot pass on an empty result."""
import ctypes
import subprocess

import numpy as np
import pytest

import rule_ref as R
import search_ref as S
from oracle import oracle as O
from batch_ref import GAP, tail_mask
from testlib import GOL_EINVAL, check_program, cpu_lib as G  # noqa: F401 (the fixture)

SEED = 1  # (picked: the conditions of test_main_case_is_not_empty hold for it)
MAIN = dict(H=16, W=16, rule="B3/S23", total=40, horizon=300)
FILL = np.int64(-0x5A5A5A5A5A5A5A5B)


def main_ref(first=0, total=MAIN["total"], horizon=MAIN["horizon"], rule=MAIN["rule"]):
    return S.search(SEED, first, total, MAIN["H"], MAIN["W"], rule, horizon)


def search_host(G, H, W, rule, seed, first, total, slots, launch, horizon, want=(True, True, True)):
    """gol_batch_search_host on arrays of exactly `total` entries between two guard words.  Returns
    (rc, found, period, alive, hash); an output not wanted is passed as NULL and returned as None."""
    b, s = R.masks(rule) if isinstance(rule, str) else rule
    m = max(total, 0)
    arrs = [np.full(m + 2, FILL, np.int64) for _ in range(4)]
    ptr = [a[1:].ctypes.data for a in arrs]
    rc = G.lib().gol_batch_search_host(H, W, b, s, seed, first, total, slots, launch, horizon, ptr[0],
                                       ptr[1] if want[0] else None, ptr[2] if want[1] else None, ptr[3] if want[2] else None)
    for a in arrs:
        assert a[0] == FILL and a[-1] == FILL
    out = [arrs[0][1:-1]] + [a[1:-1] if w else None for a, w in zip(arrs[1:], want)]
    for a, w in zip(arrs[1:], want):
        assert w or np.all(a == FILL)
    return (rc, out[0], out[1], None if out[2] is None else out[2].view(np.uint64), None if out[3] is None else out[3].view(np.uint64))


def assert_equal(got, want, where=None):
    for g, w in zip(got, want):
        assert g.dtype == w.dtype and g.tolist() == w.tolist(), where


# ---------------------------------------------------------------- the soup's words

@pytest.mark.parametrize("W", [16, 65, 70, 512])
def test_soup_host_matches_oracle(G, W):
    H, Ww = 5, (W + 63) // 64
    for index in (0, 1, 1 << 33):
        want = S.soup_words(77, index, H, W)
        assert want.any() and np.all(want[:, Ww - 1] & ~tail_mask(W) == 0)
        buf = np.full((H, Ww + 2), GAP, np.uint64)  # rows two words apart: the words between them stay
        assert G.lib().gol_batch_soup_host(H, W, 77, index, buf.ctypes.data, Ww + 2) == 0
        assert np.array_equal(buf[:, :Ww], want) and np.all(buf[:, Ww:] == GAP)
        assert np.array_equal(G.Batch.soup(H, W, 77, index), want)
    # soup g is board g of one supply: rows g H .. of the oracle's words
    both = O.random_words(77, 0, 2 * H, Ww)
    both[:, Ww - 1] &= tail_mask(W)
    assert np.array_equal(np.concatenate([G.Batch.soup(H, W, 77, 0), G.Batch.soup(H, W, 77, 1)]), both)


def test_soup_host_einval(G):
    L = G.lib()
    buf = np.full((8, 9), GAP, np.uint64)
    p = buf.ctypes.data
    bad = [L.gol_batch_soup_host(0, 8, 1, 0, p, 1), L.gol_batch_soup_host(8, 0, 1, 0, p, 1), L.gol_batch_soup_host(513, 8, 1, 0, p, 1),
           L.gol_batch_soup_host(8, 513, 1, 0, p, 9), L.gol_batch_soup_host(8, 8, 1, -1, p, 1),
           L.gol_batch_soup_host(8, 8, 1, (1 << 40) + 1, p, 1), L.gol_batch_soup_host(8, 65, 1, 0, p, 1),
           L.gol_batch_soup_host(8, 8, 1, 0, None, 1)]
    assert bad == [GOL_EINVAL] * len(bad) and np.all(buf == GAP)
    with pytest.raises(G.GolError):
        G.Batch.soup(8, 8, 1, -1)


# ---------------------------------------------------------------- the verdict

STAY, FOUND, EXPIRED = 0, 1, 2
VERDICTS = [  # (found age, age, horizon) -> verdict
    ((-1, 0, 300), STAY), ((-1, 299, 300), STAY), ((-1, 300, 300), EXPIRED), ((-1, 301, 300), EXPIRED),
    ((1, 7, 300), FOUND), ((300, 300, 300), FOUND), ((300, 301, 300), FOUND), ((298, 350, 300), FOUND),
    ((301, 301, 300), EXPIRED), ((301, 350, 300), EXPIRED),  # the overshoot: found in a launch that ran past the horizon
    ((257, 300, 257), FOUND), ((257, 300, 256), EXPIRED), ((256, 300, 256), FOUND),
    ((-1, 0, 0), EXPIRED), ((1, 1, 0), EXPIRED), ((1, 1, 1), FOUND), ((-1, 1, 1), EXPIRED), ((-1, 0, 1), STAY),
]


def test_verdict_table(G):
    got = [G.lib().gol_batch_verdict_host(*args) for args, _ in VERDICTS]
    assert got == [v for _, v in VERDICTS]


# ---------------------------------------------------------------- the search on host memory

def test_main_case_is_not_empty():
    """(the reference alone) what keeps the tests of the main case from passing on an empty result."""
    found, period, alive, hashes = main_ref()
    assert int(np.sum(found >= 0)) >= 10 and int(np.sum(found < 0)) >= 2
    assert period.max() > 2
    assert 256 in found.tolist() and 257 in found.tolist()
    assert np.all((found >= 0) == (period >= 1)) and np.all(hashes[found < 0] == 0) and np.all(alive[found < 0] == 0)
    assert np.any(alive > 0) and len(set(hashes[found >= 0].tolist())) > 10


@pytest.mark.parametrize("slots", [1, 5, 64])
def test_search_host_main_case(G, slots):
    want = main_ref()
    for launch in (1, 7, 64, 300):
        rc, *got = search_host(G, 16, 16, MAIN["rule"], SEED, 0, 40, slots, launch, 300)
        assert rc == 0, G.lib().gol_last_error()
        assert_equal(got, want, (slots, launch))


def test_search_host_overshoot(G):
    """Launches of 100 turns reach age 300 before the pass sees a soup found at 257: with horizon 256 that is no find."""
    for horizon in (257, 256):
        want = main_ref(horizon=horizon)
        rc, *got = search_host(G, 16, 16, MAIN["rule"], SEED, 0, 40, 5, 100, horizon)
        assert rc == 0
        assert_equal(got, want, horizon)
    at257 = main_ref(horizon=257)[0] == 257
    assert at257.any() and np.all(main_ref(horizon=256)[0][at257] == -1)


def test_search_host_other_rule_and_shape(G):
    want = main_ref(rule="B36/S23")
    assert int(np.sum(want[0] >= 0)) >= 10 and int(np.sum(want[0] < 0)) >= 2
    rc, *got = search_host(G, 16, 16, "B36/S23", SEED, 0, 40, 5, 7, 300)
    assert rc == 0
    assert_equal(got, want)
    want = S.search(SEED, 0, 7, 130, 70, "B/S23", 64)
    assert np.all(want[0] >= 0)
    rc, *got = search_host(G, 130, 70, "B/S23", SEED, 0, 7, 3, 5, 64)
    assert rc == 0
    assert_equal(got, want)


def test_search_host_first(G):
    want = main_ref()
    rc, *got = search_host(G, 16, 16, MAIN["rule"], SEED, 17, 10, 4, 7, 300)
    assert rc == 0
    assert_equal(got, [a[17:27] for a in want])
    assert_equal(got, main_ref(17, 10))


def test_search_host_edges(G):
    rc, *got = search_host(G, 16, 16, MAIN["rule"], SEED, 0, 0, 5, 7, 300)
    assert rc == 0 and all(len(a) == 0 for a in got)
    rc, *got = search_host(G, 16, 16, MAIN["rule"], SEED, 0, 12, 5, 7, 0)
    assert rc == 0
    assert [a.tolist() for a in got] == [[-1] * 12, [-1] * 12, [0] * 12, [0] * 12]
    # horizon 1: only a soup that is a still life is found, at 1.  B3/S23 has none among these soups, B/S012345678
    # (nothing is born, nothing dies) finds every one (the reference alone)
    assert main_ref(0, 12, 1)[0].tolist() == [-1] * 12
    still = main_ref(0, 12, 1, "B/S012345678")
    assert still[0].tolist() == [1] * 12 and still[1].tolist() == [1] * 12 and np.all(still[2] > 0)
    for rule, want in ((MAIN["rule"], main_ref(0, 12, 1)), ("B/S012345678", still)):
        for slots, launch in ((5, 7), (12, 1), (1, 1)):
            rc, *got = search_host(G, 16, 16, rule, SEED, 0, 12, slots, launch, 1)
            assert rc == 0
            assert_equal(got, want, (rule, slots, launch))


def test_search_host_null_outputs(G):
    want = main_ref(0, 12)
    for keep in ((False, False, False), (True, False, False), (False, True, False), (False, False, True)):
        rc, found, period, alive, hashes = search_host(G, 16, 16, MAIN["rule"], SEED, 0, 12, 5, 7, 300, keep)
        assert rc == 0 and found.tolist() == want[0].tolist()
        for got, w in zip((period, alive, hashes), want[1:]):
            assert got is None or got.tolist() == w.tolist()


def test_search_host_refusals(G):
    L = G.lib()
    out = np.full(16, FILL, np.int64)
    o = out.ctypes.data
    run = L.gol_batch_search_host
    bad = [run(0, 16, 8, 12, 1, 0, 4, 2, 7, 10, o, o, o, o), run(16, 0, 8, 12, 1, 0, 4, 2, 7, 10, o, o, o, o),
           run(513, 16, 8, 12, 1, 0, 4, 2, 7, 10, o, o, o, o), run(16, 513, 8, 12, 1, 0, 4, 2, 7, 10, o, o, o, o),
           run(16, 16, 512, 12, 1, 0, 4, 2, 7, 10, o, o, o, o), run(16, 16, 8, 512, 1, 0, 4, 2, 7, 10, o, o, o, o),
           run(16, 16, 8, 12, 1, -1, 4, 2, 7, 10, o, o, o, o), run(16, 16, 8, 12, 1, 0, -1, 2, 7, 10, o, o, o, o),
           run(16, 16, 8, 12, 1, 0, 4, 2, 7, -1, o, o, o, o), run(16, 16, 8, 12, 1, 0, 4, 0, 7, 10, o, o, o, o),
           run(16, 16, 8, 12, 1, 0, 4, 2, 0, 10, o, o, o, o), run(16, 16, 8, 12, 1, 0, 4, 2, 7, 10, None, o, o, o),
           run(16, 16, 8, 12, 1, (1 << 40) - 3, 4, 2, 7, 10, o, o, o, o), run(16, 16, 8, 12, 1, 0, (1 << 26) + 1, 2, 7, 10, o, o, o, o)]
    assert bad == [GOL_EINVAL] * len(bad) and L.gol_last_error()
    assert np.all(out == FILL)
    assert run(16, 16, 8, 12, 1, (1 << 40) - 4, 4, 2, 7, 0, o, None, None, None) == 0  # (the last four soups of the supply)
    assert out[:4].tolist() == [-1] * 4 and np.all(out[4:] == FILL)


def test_batch_check_search_under_sanitizers():
    """gol_batch_soup_host and gol_batch_search_host in the stand-alone program, every buffer a heap block of its
    exact size, against a scan written in the driver, over shapes, rules, slot counts and launch lengths."""
    r = subprocess.run([check_program("batch_check"), "search"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "batch_check search:" in r.stdout and " 0 bad" in r.stdout
