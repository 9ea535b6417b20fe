"""Batches of small boards, the part that needs no GPU: the batch kernel's row function on host
memory (gol_batch_step_host, csrc/gol_batch.h) against the numpy stepper of rule_ref.py for every
shape and rule, the caller's buffer contract, the ABI edges, the same code in a stand-alone program
under AddressSanitizer + UndefinedBehaviorSanitizer (build/asan/batch_check, a plain child process;
nothing loaded into Python is sanitized), and the Python class's byte <-> word packing.  All
comparisons are exact; the reference is rule_ref (np.roll sums), never the library."""
import subprocess

import numpy as np
import pytest

import rule_ref
from batch_ref import GAP, from_words, tail_mask, to_words
from testlib import check_program, cpu_lib as G  # noqa: F401 (the fixture)

# degenerate wraps, one to sixteen words per row, a last word partly and wholly used, more than 64 rows; five to
# eight words (the 8-word row function) and an odd count of words below the 8 or 16 held
SHAPES = [(1, 1), (1, 2), (2, 1), (2, 2), (3, 3), (2, 5), (5, 2), (16, 16), (7, 31), (7, 32), (7, 33), (5, 63), (5, 64),
          (5, 65), (3, 96), (4, 511), (4, 512), (3, 481), (64, 1), (65, 31), (5, 129), (3, 150), (4, 256), (3, 270)]
RULES = ["B3/S23", "B36/S23", "B3678/S34678", "B2/S", "B0/S8", "B012345678/S012345678"]
TURNS = 4


def host_step(G, H, W, rule, buf_in, buf_out, stride):
    b, s = rule_ref.masks(rule) if isinstance(rule, str) else rule
    return G.lib().gol_batch_step_host(H, W, b, s, buf_in.ctypes.data if buf_in is not None else None,
                                       buf_out.ctypes.data if buf_out is not None else None, stride)


@pytest.mark.parametrize("rule", RULES)
def test_step_host_matches_reference(G, rule):
    """Every shape, four turns, dense rows and rows two words apart; the first input of each run has
    every padding bit set, which no output may show, and the words between the rows stay."""
    for i, (H, W) in enumerate(SHAPES):
        Ww = (W + 63) // 64
        for pad in (0, 2):
            stride = Ww + pad
            cells = rule_ref.random_board(1000 + i, H, W, 0.2 + 0.1 * (i % 5))
            buf = np.full((H, stride), GAP, np.uint64)
            buf[:, :Ww] = to_words(cells)
            buf[:, Ww - 1] |= ~tail_mask(W)  # alive "cells" at c >= W
            for t in range(1, TURNS + 1):
                cells = rule_ref.step(cells, *rule_ref.masks(rule))
                out = np.full((H, stride), GAP, np.uint64)
                assert host_step(G, H, W, rule, buf, out, stride) == 0, G.lib().gol_last_error()
                assert np.array_equal(out[:, :Ww], to_words(cells)), (H, W, pad, rule, t)
                assert np.all(out[:, Ww:] == GAP), (H, W, pad, rule, t)
                buf = out


def test_step_host_in_place(G):
    for H, W in [(1, 1), (2, 5), (65, 31), (4, 511), (16, 16)]:
        Ww = (W + 63) // 64
        cells = rule_ref.random_board(7, H, W, 0.4)
        buf = np.full((H, Ww + 1), GAP, np.uint64)
        buf[:, :Ww] = to_words(cells)
        assert host_step(G, H, W, "B36/S23", buf, buf, Ww + 1) == 0
        assert np.array_equal(buf[:, :Ww], to_words(rule_ref.step(cells, *rule_ref.masks("B36/S23"))))
        assert np.all(buf[:, Ww:] == GAP)


def test_step_host_einval(G):
    buf = np.zeros((8, 9), np.uint64)
    out = np.full((8, 9), GAP, np.uint64)
    bad = [(0, 8, (8, 12), buf, out, 1), (8, 0, (8, 12), buf, out, 1), (513, 8, (8, 12), buf, out, 1),
           (8, 513, (8, 12), buf, out, 9), (-1, 8, (8, 12), buf, out, 1), (8, 8, (512, 12), buf, out, 1),
           (8, 8, (8, 512), buf, out, 1), (8, 65, (8, 12), buf, out, 1), (8, 512, (8, 12), buf, out, 7),
           (8, 8, (8, 12), buf, out, 0), (8, 8, (8, 12), None, out, 1), (8, 8, (8, 12), buf, None, 1)]
    for H, W, rule, a, b, stride in bad:
        assert host_step(G, H, W, rule, a, b, stride) == -1, (H, W, rule, stride)
        assert G.lib().gol_last_error()
    assert np.all(out == GAP)
    assert host_step(G, 8, 512, (8, 12), buf, out, 8) == 0 and host_step(G, 8, 8, (511, 511), buf, out, 1) == 0


def test_batch_check_under_sanitizers():
    """The same shapes and rules in the stand-alone program, every buffer a heap block of its exact
    size, against a cell-by-cell neighbour count."""
    r = subprocess.run([check_program("batch_check")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "0 bad" in r.stdout


@pytest.mark.parametrize("W", [1, 33, 64, 65, 512])
def test_pack_round_trip(G, W):
    cells = (np.random.default_rng(W).random((3, 5, W)) < 0.5).astype(np.uint8) * np.uint8(1 + W % 200)
    words = G.Batch.pack(cells)
    assert words.dtype == np.uint64 and words.shape == (3, 5, (W + 63) // 64)
    assert np.array_equal(words, to_words(cells))
    assert not np.any(words[..., -1] & ~tail_mask(W))
    back = G.Batch.unpack(words, W)
    assert back.dtype == np.uint8 and np.array_equal(back, (cells != 0) * 255)
    assert np.array_equal(from_words(words, W) * 255, back)
