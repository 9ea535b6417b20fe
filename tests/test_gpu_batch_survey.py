"""Batch surveys on the GPU: a rule per board (gol_batch_set_rules) and the cycle scan of any period
(gol_batch_step_cycles).  Every comparison is exact.  The expectations come from tests/rule_ref.py
(numpy rolls) and tests/cycle_ref.py (the scan's definition), never from the library, and each test
first asserts on the reference's own results that its input still exercises the case it is here for."""
import ctypes

import numpy as np
import pytest

import cycle_ref as C
import rule_ref as R
from cycle_ref import RULES
from batch_ref import batch_n, check_queries, random_boards, ref_settle, tail_mask
from testlib import GOL_EINVAL, GOL_ESTATE, gpu_lib as G  # noqa: F401 (the fixture)

pytestmark = pytest.mark.gpu

MASKS = np.array([R.masks(r) for r in RULES], np.uint32)


def ref_each(cells, rules, turns):
    return np.stack([R.run(c, r, turns)[0] for c, r in zip(cells, rules)])


# ---------------------------------------------------------------- a rule per board

# four boards of four rules in one workgroup (37 boards: the last workgroup holds one); two waves per
# board and two boards per workgroup; three waves, one board per workgroup; a row of two words
@pytest.mark.parametrize("H,W,n", [(16, 16, 37), (65, 31, 0), (129, 65, 0), (5, 33, 0)])
def test_rules_per_board(G, H, W, n):
    n = n or batch_n(G, H, W)
    rules = [RULES[i % 18] for i in range(n)]
    cells = random_boards(7 * H + W, n, H, W)
    want = ref_each(cells, rules, 9)
    # (the reference alone) a batch stepped under the rule of board 0 would be wrong on every other board
    conway = ref_each(cells, [RULES[0]] * n, 9)
    assert all(np.array_equal(want[i], conway[i]) == (i % 18 == 0) for i in range(n))
    with G.Batch(n, H, W, turns_per_launch=4) as b:
        if H == 16:
            assert b.info()["boards_per_workgroup"] == 4 and n % 4 == 1
        b.load(cells)
        b.set_rules(rules)
        assert b.turn == 0 and np.array_equal(b.rules(), MASKS[np.arange(n) % 18])
        with pytest.raises(G.GolError) as ei:
            b.rule
        assert ei.value.code == GOL_ESTATE
        b.step(9)
        assert b.turn == 9
        check_queries(b, want)
        # B0 gives birth in every empty neighbourhood: the padding must stay empty all the same
        assert not np.any(b.store_words()[..., -1] & ~tail_mask(W))
        # one rule again: the uniform batch
        b.set_rule("B36/S23")
        assert b.rule == "B36/S23" and np.array_equal(b.rules(), np.tile(MASKS[1], (n, 1)))
        b.step(5)
        check_queries(b, ref_each(want, ["B36/S23"] * n, 5))


def test_set_rules_on_a_sub_range(G):
    H, W = 65, 31
    n = 7
    cells = random_boards(55, n, H, W)
    with G.Batch(n, H, W, rule="B36/S23", turns_per_launch=3) as b:
        b.load(cells)
        b.step(2)
        b.set_rules(["B2/S", (0x001, 0x100), "B3/S23"], first=2)  # the mask pair is B0/S8
        rules = ["B36/S23", "B36/S23", "B2/S", "B0/S8", "B3/S23", "B36/S23", "B36/S23"]
        assert b.turn == 2 and np.array_equal(b.rules(), np.array([R.masks(r) for r in rules], np.uint32))
        assert np.array_equal(b.rules(3, 2), np.array([R.masks(r) for r in rules[3:5]], np.uint32))
        mid = ref_each(cells, ["B36/S23"] * n, 2)
        check_queries(b, mid)
        b.step(7)
        want = ref_each(mid, rules, 7)
        assert not any(np.array_equal(want[i], R.run(mid[i], "B36/S23", 7)[0]) for i in (2, 3, 4))
        check_queries(b, want)
        # a second sub-range, as a uint32[m, 2] array, leaves the first one alone
        b.set_rules(np.array([R.masks("B1357/S1357")] * 2, np.uint32), first=5)
        rules[5:7] = ["B1357/S1357"] * 2
        assert np.array_equal(b.rules(), np.array([R.masks(r) for r in rules], np.uint32))
        b.step(4)
        check_queries(b, ref_each(want, rules, 4))


def test_equal_masks_are_the_uniform_batch(G):
    H, W = 16, 16
    n = batch_n(G, H, W)
    cells = random_boards(91, n, H, W)
    with G.Batch(n, H, W, turns_per_launch=4) as b:
        b.load(cells)
        b.set_rules(["B3678/S34678"] * n)
        assert b.rule == "B3678/S34678"
        b.step(9)
        check_queries(b, ref_each(cells, ["B3678/S34678"] * n, 9))
        # mixed, then equal again through set_rules on the one board that differed
        b.set_rules(["B2/S"], first=n - 1)
        with pytest.raises(G.GolError):
            b.rule
        b.set_rules(["B3678/S34678"], first=n - 1)
        assert b.rule == "B3678/S34678"
        b.set_rules(["B3/S23"] * n)
        assert b.rule == "B3/S23"
        b.load(cells)
        b.step(9)
        check_queries(b, ref_each(cells, ["B3/S23"] * n, 9))


@pytest.mark.parametrize("H,W", [(16, 16), (129, 65)])
def test_conway_boards_in_a_mixed_batch(G, H, W):
    """All B3/S23 except board 1: every board is right (B3/S23 on the table circuit)."""
    n = batch_n(G, H, W)
    cells = random_boards(17, n, H, W)
    rules = ["B3/S23"] * n
    rules[1] = "B36/S23"
    want = ref_each(cells, rules, 9)
    assert not np.array_equal(want[1], R.run(cells[1], R.CONWAY, 9)[0])
    with G.Batch(n, H, W, turns_per_launch=4) as b:
        b.load(cells)
        b.set_rules(["B36/S23"], first=1)
        b.step(9)
        check_queries(b, want)


def test_set_rules_refusals_change_nothing(G):
    H, W = 16, 16
    n = 9
    L = G.lib()
    cells = random_boards(23, n, H, W)
    rules = [RULES[i % 18] for i in range(n)]
    with G.Batch(n, H, W, turns_per_launch=4) as b:
        b.load(cells)
        b.set_rules(rules)
        for bad in ([(8, 12), (512, 12), (8, 12)], [(8, 12), (8, 512)], np.array([[4, 0], [1 << 20, 3]], np.uint32)):
            with pytest.raises(G.GolError) as ei:
                b.set_rules(bad, first=2)
            assert ei.value.code == GOL_EINVAL
        with pytest.raises(G.GolError):
            b.set_rules(["B9/S"], first=0)
        ok = np.array([8, 8], np.uint32)
        out = np.full(4, 77, np.uint32)
        p, o, bh = ok.ctypes.data, out.ctypes.data, b._h
        calls = [L.gol_batch_set_rules(bh, -1, 1, p, p), L.gol_batch_set_rules(bh, 2, 1, p, p),
                 L.gol_batch_set_rules(bh, n - 1, n + 1, p, p), L.gol_batch_set_rules(bh, 0, 2, None, p),
                 L.gol_batch_set_rules(bh, 0, 2, p, None), L.gol_batch_set_rules(None, 0, 2, p, p),
                 L.gol_batch_rules(bh, -1, 1, o, o), L.gol_batch_rules(bh, 2, 1, o, o), L.gol_batch_rules(bh, n - 1, n + 1, o, o),
                 L.gol_batch_rules(bh, 0, 2, None, o), L.gol_batch_rules(bh, 0, 2, o, None), L.gol_batch_rules(None, 0, 2, o, o)]
        assert calls == [GOL_EINVAL] * len(calls) and np.all(out == 77)
        birth, survive = ctypes.c_uint32(77), ctypes.c_uint32(77)
        assert L.gol_batch_rule(bh, ctypes.byref(birth), ctypes.byref(survive)) == GOL_ESTATE
        assert (birth.value, survive.value) == (77, 77)
        assert L.gol_batch_set_rules(bh, 3, 3, p, p) == 0  # an empty range is legal
        assert np.array_equal(b.rules(), MASKS[:n]) and b.turn == 0
        b.step(9)
        check_queries(b, ref_each(cells, rules, 9))


# ---------------------------------------------------------------- the cycle scan

def check_cycles(b, turns, want, t0=0):
    found, period = b.step_cycles(turns)
    assert found.dtype == np.int64 and period.dtype == np.int64
    assert found.tolist() == want[0].tolist() and period.tolist() == want[1].tolist()
    assert b.turn == t0 + turns
    check_queries(b, want[2])


# (H, W, turns, [(pattern, y, x, found, period)]): the patterns of one batch, random boards beside them
GROUPS = [
    (5, 5, 10, [([], 0, 0, 1, 1), (C.BLOCK, 1, 1, 1, 1), (C.BLINKER, 2, 1, 3, 2)]),
    (17, 17, 40, [(C.PULSAR, 2, 2, 6, 3)]),
    (129, 65, 40, [(C.PULSAR, 57, 58, 6, 3)]),    # over the waves' seam, wrapping in x
    (20, 20, 100, [(C.ROW10, 10, 5, 30, 15)]),
    (130, 33, 100, [(C.ROW10, 0, 28, 30, 15)]),   # over the column wrap
    (129, 65, 100, [(C.ROW10, 63, 60, 30, 15)]),  # on the last row of wave 0
    (8, 8, 200, [(C.GLIDER, 0, 0, 63, 32)]),
    (16, 16, 400, [(C.GLIDER, 0, 0, 127, 64)]),
    (7, 9, 600, [(C.GLIDER, 0, 0, 507, 252)]),
    (16, 16, 300, [(C.R_PENTOMINO, 6, 6, 129, 2)]),
]


@pytest.mark.parametrize("k", range(len(GROUPS)))
def test_cycles_known_patterns(G, k):
    """Launches of 1, 5 and 7 turns and the automatic length: 5 and 7 put d = 15 and d = 7 on a launch
    end that is also a mark."""
    H, W, turns, patterns = GROUPS[k]
    n = max(batch_n(G, H, W), len(patterns) + 2)
    cells = random_boards(13 * H + W + turns, n, H, W)
    for i, (rows, y, x, _, _) in enumerate(patterns):
        cells[i] = C.place(H, W, rows, y, x)
    want = C.scan_all(cells, R.CONWAY, turns)
    for i, (_, _, _, found, period) in enumerate(patterns):
        assert (want[0][i], want[1][i]) == (found, period)  # (the reference alone)
    for tpl in (1, 5, 7, 0):
        with G.Batch(n, H, W, turns_per_launch=tpl) as b:
            b.load(cells)
            check_cycles(b, turns, want)


def test_cycles_soups(G):
    """24 soups, 600 turns in one call and in two calls of 300: the second call scans from its own t0."""
    soups = np.stack([R.random_board(1000 + i, 16, 16, 0.35) for i in range(24)])
    want = C.scan_all(soups, R.CONWAY, 600)
    assert np.all(want[0] >= 0) and want[0].max() == 512 and set(want[1].tolist()) == {1, 2}
    first = C.scan_all(soups, R.CONWAY, 300)
    second = C.scan_all(first[2], R.CONWAY, 300, t0=300)
    assert np.any(first[0] < 0) and np.all(second[0] > 300)  # every board is found again
    for tpl in (7, 0):
        with G.Batch(24, 16, 16, turns_per_launch=tpl) as b:
            b.load(soups)
            check_cycles(b, 600, want)
            b.load(soups)
            check_cycles(b, 300, first)
            check_cycles(b, 300, second, t0=300)


@pytest.mark.parametrize("seed,H,W,density,periods", [(4243, 5, 33, 0.4, {1, 2, 4, 28}), (4242, 16, 16, 0.35, {1, 2})])
def test_cycles_with_rules_per_board(G, seed, H, W, density, periods):
    cells = np.stack([R.random_board(seed, H, W, density)] * 18)
    want = C.scan_all(cells, RULES, 300)
    assert set(want[1][want[1] > 0].tolist()) == periods and int(np.sum(want[0] < 0)) == 5
    for tpl in (7, 0):
        with G.Batch(18, H, W, turns_per_launch=tpl) as b:
            b.load(cells)
            b.set_rules(RULES)
            check_cycles(b, 300, want)


def test_cycles_edges(G):
    """No turn, one turn, the scans sharing their device buffer, and a plain step beside them."""
    H, W = 16, 16
    cells = np.zeros((6, H, W), np.uint8)
    cells[1] = C.place(H, W, C.BLOCK, 3, 3)
    cells[2] = C.place(H, W, C.BLINKER, 5, 4)
    cells[3] = C.place(H, W, C.GLIDER, 1, 1)
    cells[4:] = random_boards(40, 2, H, W)
    with G.Batch(6, H, W, turns_per_launch=3) as b:
        b.load(cells)
        b.step(5)
        now = np.stack([R.run(c, R.CONWAY, 5)[0] for c in cells])
        found, period = b.step_cycles(0)
        assert found.tolist() == [-1] * 6 and period.tolist() == [-1] * 6 and b.turn == 5
        check_queries(b, now)
        # one turn finds the still lifes (and nothing else) at t0 + 1
        want = C.scan_all(now, R.CONWAY, 1, t0=5)
        assert want[0].tolist()[:4] == [6, 6, -1, -1] and want[1].tolist()[:4] == [1, 1, -1, -1]
        check_cycles(b, 1, want, t0=5)
        # step_cycles, then the settle scan, then step_cycles: each is right after the other
        want = C.scan_all(want[2], R.CONWAY, 20, t0=6)
        assert want[0].tolist()[:4] == [7, 7, 9, -1] and want[1].tolist()[:4] == [1, 1, 2, -1]
        check_cycles(b, 20, want, t0=6)
        ref = [ref_settle(c, R.CONWAY, 11) for c in want[2]]
        assert [t for t, _ in ref][:4] == [2, 2, 2, -1]
        assert b.step(11, settled=True).tolist() == [t + 26 if t >= 0 else -1 for t, _ in ref]
        check_queries(b, np.stack([s for _, s in ref]))
        want = C.scan_all(np.stack([s for _, s in ref]), R.CONWAY, 40, t0=37)
        check_cycles(b, 40, want, t0=37)
        # the boards after step_cycles are those of a plain step
        b.load(cells)
        b.step(77)
        plain = b.store_words()
        b.load(cells)
        b.step_cycles(77)
        assert np.array_equal(b.store_words(), plain)
        assert np.array_equal(b.store(), np.stack([R.run(c, R.CONWAY, 77)[0] for c in cells]) * 255)
        # refusals leave everything alone
        L = G.lib()
        out = np.full(6, 77, np.int64)
        calls = [L.gol_batch_step_cycles(b._h, -1, out.ctypes.data, out.ctypes.data),
                 L.gol_batch_step_cycles(b._h, 3, None, out.ctypes.data), L.gol_batch_step_cycles(None, 3, out.ctypes.data, None)]
        assert calls == [GOL_EINVAL] * 3 and np.all(out == 77) and b.turn == 77
        assert L.gol_batch_step_cycles(b._h, 3, out.ctypes.data, None) == 0 and b.turn == 80  # (period may be NULL)
        assert out.tolist()[:4] == [78, 78, 80, -1]
