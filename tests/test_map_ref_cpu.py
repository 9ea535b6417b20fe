"""The reference of the MAP tests (tests/map_ref.py) against what is known without it: the numpy stepper of life-like
rules, np.roll, and Golly's published MAP string of Conway's Life.  Nothing of the library runs here."""
import numpy as np
import pytest

import cycle_ref as C
import map_ref as M
import rule_ref as R


@pytest.mark.parametrize("rule", C.RULES)
def test_a_life_like_rule_as_a_map_steps_like_the_rule(rule):
    birth, survive = R.masks(rule)
    m = M.from_rule(birth, survive)
    for H, W in ((5, 7), (1, 1), (2, 3)):
        b = R.random_board(3 * H + W, H, W, 0.4)
        for _ in range(4):
            want = R.step(b, birth, survive)
            assert np.array_equal(M.step(b, m), want), (rule, H, W)
            b = want


@pytest.mark.parametrize("k", range(9))
def test_a_projection_map_is_a_translation(k):
    """Bit i of P_k = bit k of i: the next cell is one neighbour, so a turn rolls the board.  The nine offsets written
    out here pin the neighbour order and the bit weights: 256 NW ... 16 C ... 1 SE, N the row above."""
    offsets = {8: (1, 1), 7: (1, 0), 6: (1, -1), 5: (0, 1), 4: (0, 0), 3: (0, -1), 2: (-1, 1), 1: (-1, 0), 0: (-1, -1)}
    assert M.projection_roll(k) == offsets[k]
    b = R.random_board(k, 6, 7, 0.4)
    got = M.step(b, M.projection(k))
    assert np.array_equal(got, np.roll(b, offsets[k], (0, 1)))
    # (said once more without np.roll: under P_8, NW, the cell (y, x) becomes what (y - 1, x - 1) was)
    y, x = 2, 3
    dy, dx = offsets[k]
    assert got[y, x] == b[(y - dy) % 6, (x - dx) % 7]


def test_gollys_life_string():
    m = M.parse(M.GOLLY_LIFE)
    assert np.array_equal(m, M.from_rule(*R.CONWAY))
    assert M.fmt(m) == M.GOLLY_LIFE and len(M.GOLLY_LIFE) == 3 + 86
    assert np.array_equal(M.parse(M.GOLLY_LIFE + "=="), m)
    r = M.random_map(5)
    assert np.array_equal(M.parse(M.fmt(r)), r) and np.array_equal(M.from_bits(M.bits(r)), r)


def test_the_case_table_covers_the_kernel():
    cases = M.cases()
    assert len(cases) == 2 * len(M.WIDTHS) and len({c[0] for c in cases}) == len(cases)
    by_w = {W: sorted(H for _, H, w, _, _ in cases if w == W) for W in M.WIDTHS}
    assert all(len(set(hs)) == 2 for hs in by_w.values())
    for H in M.HEIGHTS:  # every height with a narrow and a wide row
        ws = [w for _, h, w, _, _ in cases if h == H]
        assert min(ws) <= 32 and max(ws) > 128, (H, ws)
    # every NW class at both its edges: the narrowest and the widest row it holds
    edges = {1: (1, 32), 2: (33, 64), 4: (65, 128), 8: (129, 256), 16: (257, 512)}
    for nw, (lo, hi) in edges.items():
        assert M.words_per_lane(lo) == M.words_per_lane(hi) == nw and lo in by_w and hi in by_w
        assert lo == 1 or M.words_per_lane(lo - 1) == nw // 2
    # every wave count the heights give, every number of boards in a workgroup, a partly filled last wave and workgroup
    assert {(H + 63) // 64 for _, H, _, _, _ in cases} == {1, 2, 3, 8}
    assert {max(1, 4 // ((H + 63) // 64)) for _, H, _, _, _ in cases} == {1, 2, 4}
    assert any(H % 64 for _, H, _, _, _ in cases) and all(M.N_BOARDS % max(1, 4 // ((H + 63) // 64)) or H > 128 for _, H, _, _, _ in cases)
    assert {t for _, _, _, t, _ in cases} == set(range(1, 10)) and {k for *_, k in cases} == set(M.KINDS)
    # the torus's degenerate shapes, and a row that ends inside a word behind a full one
    assert any(H == 1 for _, H, _, _, _ in cases) and any(H == 2 for _, H, _, _, _ in cases) and 1 in by_w and 33 in by_w


def test_the_launch_model_is_the_scan():
    """launch_model cut into launches of 3 reproduces scan() on a glider (found 63, period 32 on 8 x 8)."""
    m = M.from_rule(*R.CONWAY)
    cells = C.place(8, 8, C.GLIDER)
    assert M.scan(cells, m, 70)[:2] == (63, 32)
    boards, prev, settled = M.pack(cells)[None], np.zeros((1, 8, 1), np.uint64), np.full(1, -1, np.int64)
    for done in range(0, 69, 3):
        out = M.launch_model(boards, prev, settled, None, H=8, W=8, turns=3, maps=m, map_each=False, turn0=done, have_prev=done > 0,
                             write_prev=True, scan=M.SCAN_CYCLES, done=done)
        boards, prev, settled = out["boards"], out["prev"], out["settled"]
    assert settled.tolist() == [63]
