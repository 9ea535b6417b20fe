"""Batches of small boards on the GPU (gol_batch_*, golhip.Batch): many tori stepped in one launch,
each resident in its workgroup.  Every comparison is exact; the reference is tests/rule_ref.py (numpy
rolls), the oracle (O.random_words, O.hash_words, O.popcount_words, O.read_pgm) and the goldens, never
the library.  n is taken from info() so that two workgroups are full and a third one partly."""
import ctypes
import os

import numpy as np
import pytest

import rule_ref as R
from batch_ref import batch_n, check_queries, random_boards, ref_settle, tail_mask, to_words
from oracle import oracle as O
from testlib import gpu_lib as G  # noqa: F401 (the fixture)

pytestmark = pytest.mark.gpu

# degenerate wraps; one, two, three and eight waves per board; a partly filled last wave; one to
# sixteen words per lane; a partly used last word; the largest board; eight words per lane and an odd count of
# words below the eight or sixteen held
SHAPES = [(1, 1), (2, 5), (5, 2), (3, 3), (16, 16), (63, 33), (64, 32), (64, 64), (65, 31), (129, 65), (100, 512),
          (512, 32), (511, 481), (512, 512), (5, 129), (3, 150), (4, 256), (3, 270)]
GAP = np.uint64(0x5A5A5A5A5A5A5A5A)


def ref_run(boards, rule, turns):
    return np.stack([R.run(b, rule, turns)[0] for b in boards])


@pytest.mark.parametrize("H,W", SHAPES)
def test_shapes_match_reference(G, H, W):
    """13 turns in launches of 5, 5 and 3."""
    n = batch_n(G, H, W)
    cells = random_boards(31 * H + W, n, H, W)
    with G.Batch(n, H, W, turns_per_launch=5) as b:
        assert b.info()["turns_per_launch"] == 5 and b.info()["n"] == n and b.rule == "B3/S23"
        b.load(cells * 255)
        check_queries(b, cells)
        b.step(13)
        assert b.turn == 13
        check_queries(b, ref_run(cells, R.CONWAY, 13))


@pytest.mark.parametrize("N", [16, 64, 512])
def test_goldens(G, golden_dir, N):
    """Board 0 is the reference's image, the others random; after 1 and 100 turns board 0 is the
    reference's check image and its count the check CSV's."""
    n = batch_n(G, N, N)
    _, _, image = O.read_pgm(os.path.join(golden_dir, "images", f"{N}x{N}.pgm"), N, N)
    alive = O.read_alive_csv(os.path.join(golden_dir, "check", "alive", f"{N}x{N}.csv"))
    cells = random_boards(N, n, N, N)
    cells[0] = image == 255
    with G.Batch(n, N, N) as b:
        b.load(cells)
        for turns, at in ((1, 1), (99, 100)):
            b.step(turns)
            assert b.turn == at
            with open(os.path.join(golden_dir, "check", "images", f"{N}x{N}x{at}.pgm"), "rb") as f:
                assert O.pgm_bytes(b.store(0, 1)[0]) == f.read(), at
            assert int(b.alive_counts()[0]) == alive[at]
        # (the neighbours of board 0 did not leak into it, nor it into them)
        assert np.array_equal(b.store(1, 1)[0], R.run(cells[1], R.CONWAY, 100)[0] * 255)


@pytest.mark.parametrize("H,W", [(16, 16), (65, 31), (64, 64)])
@pytest.mark.parametrize("rule", ["B36/S23", "B3678/S34678", "B2/S", "B0/S8"])
def test_rules(G, H, W, rule):
    n = batch_n(G, H, W)
    cells = random_boards(5 * H + W, n, H, W)
    with G.Batch(n, H, W, rule=rule, turns_per_launch=4) as b:
        assert b.rule == rule
        b.load(cells)
        b.step(9)
        want = ref_run(cells, rule, 9)
        check_queries(b, want)
        # B0 gives birth in every empty neighbourhood: the padding must stay empty all the same
        assert not np.any(b.store_words()[..., -1] & ~tail_mask(W))


def test_set_rule_between_steps(G):
    H, W = 65, 31
    n = batch_n(G, H, W)
    cells = random_boards(77, n, H, W)
    with G.Batch(n, H, W, turns_per_launch=3) as b:
        b.load(cells)
        b.step(4)
        b.set_rule("B0/S8")
        assert b.rule == "B0/S8" and b.turn == 4
        mid = ref_run(cells, R.CONWAY, 4)
        check_queries(b, mid)
        b.step(5)
        assert b.turn == 9
        check_queries(b, ref_run(mid, "B0/S8", 5))
        b.set_rule((0x008, 0x00C))
        b.step(2)
        check_queries(b, ref_run(ref_run(mid, "B0/S8", 5), R.CONWAY, 2))


def test_partial_load_and_strided_store(G):
    H, W = 5, 65
    Ww = 2
    n = batch_n(G, H, W)
    cells = random_boards(3, n, H, W)
    with G.Batch(n, H, W) as b:
        b.load(cells)
        b.step(3)
        assert b.turn == 3
        now = ref_run(cells, R.CONWAY, 3)
        # boards [2, 4) from rows three words apart whose padding bits and third words are set
        new = random_boards(900, 2, H, W)
        src = np.full((2, H, 3), np.uint64(2 ** 64 - 1), np.uint64)
        src[..., :Ww] = to_words(new)
        src[..., Ww - 1] |= ~tail_mask(W)
        b.load_words(src, first=2)
        assert b.turn == 0
        now[2:4] = new
        check_queries(b, now)
        b.load(cells[:1], first=n - 1)
        now[n - 1] = cells[0]
        check_queries(b, now)
        # a store with wider strides: rows 4 words apart, boards H * 4 + 3 words apart
        flat = np.full(2 * (H * 4 + 3), GAP, np.uint64)
        rc = G.lib().gol_batch_store_words(b._h, 1, 3, flat.ctypes.data, 4, H * 4 + 3)
        assert rc == 0
        want = np.full_like(flat, GAP)
        for k in range(2):
            for y in range(H):
                o = k * (H * 4 + 3) + y * 4
                want[o:o + Ww] = to_words(now[1 + k])[y]
        assert np.array_equal(flat, want)
        out = np.full((n, H, 3), GAP, np.uint64)
        assert b.store_words(out=out) is out
        assert np.array_equal(out[..., :Ww], to_words(now)) and np.all(out[..., Ww:] == GAP)
        b.step(2)
        assert b.turn == 2
        check_queries(b, ref_run(now, R.CONWAY, 2))


@pytest.mark.parametrize("H,W", [(16, 64), (63, 33), (129, 512)])
def test_load_random(G, H, W):
    n = batch_n(G, H, W)
    Ww = (W + 63) // 64
    with G.Batch(n, H, W) as b:
        b.step(2)
        b.load_random(12345)
        assert b.turn == 0
        want = O.random_words(12345, 0, n * H, Ww).reshape(n, H, Ww)
        want[..., -1] &= tail_mask(W)
        assert np.array_equal(b.store_words(), want)
        assert b.alive_counts().tolist() == [O.popcount_words(w) for w in want]


def test_settle_random_soups(G):
    """24 soups of 16 x 16, 300 turns in launches of 7: boards that settle at many different turns
    (and launch boundaries) and boards that never do."""
    boards = np.stack([R.random_board(100 + i, 16, 16, 0.35) for i in range(24)])
    ref = [ref_settle(b, R.CONWAY, 300) for b in boards]
    want = [t for t, _ in ref]
    settled = [t for t in want if t >= 0]
    assert len(settled) == 22 and min(settled) == 35 and max(settled) == 280  # (the reference alone: both outcomes are there)
    with G.Batch(24, 16, 16, turns_per_launch=7) as b:
        b.load(boards)
        got = b.step(300, settled=True)
        assert got.dtype == np.int64 and got.tolist() == want
        assert b.turn == 300
        check_queries(b, np.stack([s for _, s in ref]))
    # the same boards without the scan, and with the automatic launch length, end the same
    with G.Batch(24, 16, 16) as b:
        b.load(boards)
        assert b.step(300) is None
        check_queries(b, np.stack([s for _, s in ref]))
        b.load(boards)
        assert b.step(300, settled=True).tolist() == want


def test_settle_known_patterns(G):
    """An empty board, a block, a blinker and a glider: the scan is per call, every board makes all
    the turns (the blinker is in the phase of turn 301), and fewer than two turns find nothing."""
    cells = np.zeros((4, 16, 16), np.uint8)
    cells[1, 3:5, 3:5] = 1
    cells[2, 5, 4:7] = 1
    cells[3, 1, 2] = cells[3, 2, 3] = cells[3, 3, 1] = cells[3, 3, 2] = cells[3, 3, 3] = 1
    for tpl in (0, 7, 1):
        with G.Batch(4, 16, 16, turns_per_launch=tpl) as b:
            b.load(cells)
            assert b.step(301, settled=True).tolist() == [2, 2, 2, -1]
            assert b.turn == 301
            check_queries(b, ref_run(cells, R.CONWAY, 301))
            assert b.step(4, settled=True).tolist() == [303, 303, 303, -1]
            assert b.step(1, settled=True).tolist() == [-1, -1, -1, -1]
            assert b.step(0, settled=True).tolist() == [-1, -1, -1, -1]
            assert b.turn == 306
            check_queries(b, ref_run(cells, R.CONWAY, 306))


def test_settle_on_tall_boards(G):
    """More than one wave per board: the waves agree on one answer.  A blinker across the rows 63 |
    64 of a 129-row board, a block at the wrap of a 512-row board's rows, and a soup beside them."""
    for H, W in [(129, 65), (512, 40)]:
        n = batch_n(G, H, W)
        cells = np.zeros((n, H, W), np.uint8)
        cells[0, 62:65, 7] = 1            # a vertical blinker over the waves' seam
        cells[1, [H - 1, 0], 3:5] = 1     # a block over the torus seam
        cells[2] = R.random_board(5, H, W, 0.4)
        ref = [ref_settle(c, R.CONWAY, 21) for c in cells]
        with G.Batch(n, H, W, turns_per_launch=4) as b:
            b.load(cells)
            assert b.step(21, settled=True).tolist() == [t for t, _ in ref]
            check_queries(b, np.stack([s for _, s in ref]))


def test_refusals(G):
    L = G.lib()
    h = ctypes.c_void_p()
    for n, H, W, tpl in [(0, 8, 8, 0), (2 ** 20 + 1, 8, 8, 0), (-1, 8, 8, 0), (3, 0, 8, 0), (3, 513, 8, 0), (3, 8, 0, 0),
                         (3, 8, 513, 0), (3, 8, 8, -1)]:
        assert L.gol_batch_create(n, H, W, 0, tpl, ctypes.byref(h)) == -1 and not h.value, (n, H, W, tpl)
    with pytest.raises(G.GolError) as ei:
        G.Batch(3, 8, 600)
    assert ei.value.code == -1
    with pytest.raises(G.GolError):
        G.Batch(3, 8, 8, rule="B9/S")
    H, W, Ww = 6, 70, 2
    n = batch_n(G, H, W)
    cells = random_boards(11, n, H, W)
    with G.Batch(n, H, W, turns_per_launch=2) as b:
        b.load(cells)
        b.step(3)
        now = ref_run(cells, R.CONWAY, 3)
        buf = np.full(n * H * Ww + 8, GAP, np.uint64)
        cnt = np.full(n, GAP, np.uint64)
        p, bh = buf.ctypes.data, b._h
        bad = [L.gol_batch_load_words(bh, 2, 1, p, Ww, H * Ww), L.gol_batch_load_words(bh, 0, n + 1, p, Ww, H * Ww),
               L.gol_batch_load_words(bh, -1, 1, p, Ww, H * Ww), L.gol_batch_load_words(bh, 0, 1, p, Ww - 1, H * Ww),
               L.gol_batch_load_words(bh, 0, 2, p, Ww, H * Ww - 1), L.gol_batch_load_words(bh, 0, 1, None, Ww, H * Ww),
               L.gol_batch_store_words(bh, 2, 1, p, Ww, H * Ww), L.gol_batch_store_words(bh, 0, n + 1, p, Ww, H * Ww),
               L.gol_batch_store_words(bh, 0, 1, p, Ww - 1, H * Ww), L.gol_batch_store_words(bh, 0, 2, p, Ww, Ww - 1),
               L.gol_batch_store_words(bh, 0, 1, None, Ww, H * Ww),
               L.gol_batch_alive_counts(bh, cnt.ctypes.data, n - 1), L.gol_batch_hashes(bh, cnt.ctypes.data, n - 1),
               L.gol_batch_alive_counts(bh, None, n), L.gol_batch_step(bh, -1, None),
               L.gol_batch_step(bh, -5, cnt.ctypes.data), L.gol_batch_set_rule(bh, 512, 12), L.gol_batch_set_rule(bh, 8, 512),
               L.gol_batch_turn(bh, None), L.gol_batch_turn(None, None), L.gol_batch_step(None, 1, None)]
        assert bad == [-1] * len(bad)
        assert L.gol_last_error()
        assert np.all(buf == GAP) and np.all(cnt == GAP)
        assert b.turn == 3 and b.rule == "B3/S23"
        check_queries(b, now)
        b.step(0)  # a no-op
        assert b.turn == 3
        check_queries(b, now)
        # empty ranges are legal and change nothing but (load) the turn
        assert L.gol_batch_store_words(bh, 1, 1, p, Ww, H * Ww) == 0 and np.all(buf == GAP)
        b.step(2)
        check_queries(b, ref_run(now, R.CONWAY, 2))
