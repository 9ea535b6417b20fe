"""The pair step's tail tables on the GPU: a safety net for the constants.

The band pipeline (k = 12: 4 waves x 3 pair-step stages) and the byte pipeline (k = 32) both call
gol_pipe.h pair_tail.  The boards are the smallest at which each pipeline still runs all its stages:
48 x 1024 in the band layout (one column group, which is the wrap group, every lane's rotation
live) and 64 x 2048, 12 and 24 turns with the count fused; 64 x 64 bytes, one k = 32 launch.  The
inputs make both polarities of every gate occur densely: all dead, all alive, a 50 % and a 5 % soup,
and gliders that cross the band-wrap column (x = W/32), the board's last column and its last row
(a strip edge).  Every cell and every count is compared with the CPU oracle.
"""
import functools

import numpy as np
import pytest

from oracle import oracle as O
from testlib import gpu_lib as golhip  # noqa: F401 (the fixture)

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(120)]

INPUTS = ("dead", "alive", "soup50", "soup5", "gliders")
GLIDER = ((0, 1), (1, 2), (2, 0), (2, 1), (2, 2))  # heads down and to the right, one cell per 4 turns


@functools.lru_cache(maxsize=None)
def _board(name, H, W):
    if name == "dead":
        cells = np.zeros((H, W), dtype=bool)
    elif name == "alive":
        cells = np.ones((H, W), dtype=bool)
    elif name in ("soup50", "soup5"):
        cells = np.random.default_rng(H * 131 + W).random((H, W)) < (0.5 if name == "soup50" else 0.05)
    else:
        cells = np.zeros((H, W), dtype=bool)
        Wd = W // 32
        # about to cross the last column; the last row; on a band board (Wd words per row) the band-wrap
        # column together with the last row, and a band-wrap column further in
        spots = [(H // 2, W - 3), (H - 3, W // 2 + 5)] + ([(H - 4, Wd - 3), (5, 7 * Wd - 2)] if Wd >= 8 else [])
        for y, x in spots:
            for dy, dx in GLIDER:
                cells[(y + dy) % H, (x + dx) % W] = True
    board = cells.astype(np.uint8) * 255
    board.setflags(write=False)
    return board


@functools.lru_cache(maxsize=None)
def _reference(name, H, W, turns):
    """(cells after `turns`, the alive count after every turn) from the CPU oracle."""
    ref, counts = O.bits_run(O.pack(_board(name, H, W)), turns, with_counts=True)
    cells = O.unpack(ref)
    cells.setflags(write=False)
    return cells, counts


@pytest.mark.parametrize("name", INPUTS)
@pytest.mark.parametrize("shape", [(48, 1024), (64, 2048)])
def test_band_pipeline_against_the_oracle(golhip, shape, name):
    H, W = shape
    with golhip.Engine(H, W, device=0, layout="band") as e:
        info = e.info()
        assert info["layout"] == "band" and info["turns_per_launch"] == 12
        e.load_bytes(_board(name, H, W))
        for turns in (12, 24):
            want, counts = _reference(name, H, W, turns)
            got = e.step_counted(12, 12)
            assert got.tolist() == [counts[turns - 1]], (name, turns)
            assert np.array_equal(e.store_bytes(), want), (name, turns)
        assert e.turn == 24 and e.alive_count() == counts[23]
    if name == "gliders":  # they did move, and none was lost at a wrap
        assert counts.tolist() == [20] * 24 and not np.array_equal(want, _board(name, H, W))


@pytest.mark.parametrize("name", INPUTS)
def test_byte_pipeline_against_the_oracle(golhip, name):
    H = W = 64
    want, counts = _reference(name, H, W, 32)
    with golhip.Engine(H, W, device=0, layout="bytes") as e:
        info = e.info()
        assert info["layout"] == "bytes" and info["turns_per_launch"] == 32
        e.load_bytes(_board(name, H, W))
        got = e.step_counted(32, 32)
        assert got.tolist() == [counts[31]], name
        assert np.array_equal(e.store_bytes(), want), name
        assert e.alive_count() == counts[31]
