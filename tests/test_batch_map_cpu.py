"""MAP rules on the host (no GPU needed): the circuit the map kernel runs (gol_map_eval_host), the row function in
turns of one torus (gol_batch_step_map_host) and the text codec, against tests/map_ref.py; the refusals; and the
sanitizer build's stand-alone program."""
import ctypes
import subprocess

import numpy as np
import pytest

import map_ref as M
import rule_ref as R
from batch_ref import from_words, tail_mask, to_words
from testlib import GOL_EINVAL, GOL_OK, check_program
from testlib import cpu_lib as G  # noqa: F401 (the fixture)


def eval_host(L, m, x):
    x = np.ascontiguousarray(x, dtype=np.uint32)
    out = ctypes.c_uint32(0x77)
    assert L.gol_map_eval_host(m.ctypes.data, x.ctypes.data, ctypes.byref(out)) == GOL_OK
    return out.value


def test_the_circuit_on_every_index(G):
    L = G.lib()
    for seed in range(3):
        m = M.random_map(seed)
        t = M.bits(m)
        for i in range(512):  # x[k] has weight 2^(8 - k): NW, N, NE, W, C, E, SW, S, SE
            x = [0xFFFFFFFF if i >> (8 - k) & 1 else 0 for k in range(9)]
            assert eval_host(L, m, x) == (0xFFFFFFFF if t[i] else 0), (seed, i)


def test_the_circuit_on_random_planes(G):
    L = G.lib()
    rng = np.random.default_rng(11)
    for seed in range(20):
        m = M.random_map(100 + seed)
        t = M.bits(m)
        x = rng.integers(0, 1 << 32, 9, dtype=np.uint64).astype(np.uint32)
        want = 0
        for j in range(32):
            i = sum(((int(x[k]) >> j) & 1) << (8 - k) for k in range(9))
            want |= int(t[i]) << j
        assert eval_host(L, m, x) == want


def step_host(L, H, W, m, cells, turns, stride_pad=0, in_place=False):
    Ww = (W + 63) // 64
    words = np.full((H, Ww + stride_pad), 0xA5A5A5A5A5A5A5A5, np.uint64)
    words[:, :Ww] = to_words(cells)
    words[:, Ww - 1] |= ~tail_mask(W)  # set padding bits of the input are ignored
    out = words if in_place else np.full_like(words, 0x5A5A5A5A5A5A5A5A)
    gaps = out[:, Ww:].copy()
    assert L.gol_batch_step_map_host(H, W, m.ctypes.data, words.ctypes.data, out.ctypes.data, Ww + stride_pad, turns) == GOL_OK
    assert np.array_equal(out[:, Ww:], gaps)  # the words between the rows stay
    assert not np.any(out[:, Ww - 1] & ~tail_mask(W))  # the padding is clear
    return from_words(out[:, :Ww], W)


WIDTHS = list(range(1, 67)) + [127, 128, 129, 255, 256, 257, 511, 512]


@pytest.mark.parametrize("H", [1, 2, 3, 5])
def test_step_map_host_at_every_width(G, H):
    L = G.lib()
    for W in WIDTHS:
        cells = R.random_board(1000 * H + W, H, W, 0.45)
        for kind, m in (("random", M.random_map(W, zero_bit=0)), ("birth on empty ground", M.random_map(W + 7, zero_bit=1))):
            turns = 1 + W % 3
            got = step_host(L, H, W, m, cells, turns, stride_pad=W % 2, in_place=bool(W & 2))
            assert np.array_equal(got, M.run(cells, m, turns)), (H, W, kind)


def test_step_map_host_translates_under_the_projections(G):
    L = G.lib()
    cells = R.random_board(3, 5, 70, 0.4)
    for k in range(9):
        got = step_host(L, 5, 70, M.projection(k), cells, 3)
        dy, dx = M.projection_roll(k)
        assert np.array_equal(got, np.roll(cells, (3 * dy, 3 * dx), (0, 1))), k
    assert np.array_equal(step_host(L, 5, 70, M.projection(4), cells, 0), cells)  # no turn


def test_the_codec_against_the_reference(G):
    assert np.array_equal(G.parse_map(M.GOLLY_LIFE), M.from_rule(*R.CONWAY))
    assert G.format_map(G.parse_map(M.GOLLY_LIFE)) == M.GOLLY_LIFE
    assert np.array_equal(G.parse_map(M.GOLLY_LIFE + "=="), G.parse_map(M.GOLLY_LIFE))
    for seed in range(10):
        m = M.random_map(seed)
        assert G.format_map(m) == M.fmt(m) and np.array_equal(G.parse_map(M.fmt(m)), m)
    for rule in ("B3/S23", "B36/S23", "B0/S8", "B/S", "B012345678/S012345678"):
        want = M.from_rule(*R.masks(rule))
        assert np.array_equal(G.map_from_rule(rule), want) and np.array_equal(G.parse_map(rule), want)
        assert np.array_equal(G.map_from_rule(R.masks(rule)), want)


def test_refusals(G):
    L = G.lib()
    good = M.fmt(M.random_map(1))
    bad = ["MAP", "MAP" + "A" * 85, good + "A", good + "=", good[:40] + "*" + good[41:], good[:-1] + "B", good[:50] + "=" + good[51:],
           "map" + good[3:], "B3/S9", "", "B2-a/S12"]
    for text in bad:
        with pytest.raises(G.GolError) as ei:
            G.parse_map(text)
        assert ei.value.code == GOL_EINVAL, text
    m = M.random_map(2)
    w = np.zeros((4, 2), np.uint64)
    step = L.gol_batch_step_map_host
    for args in [(0, 8, m.ctypes.data, w.ctypes.data, w.ctypes.data, 2, 1), (8, 513, m.ctypes.data, w.ctypes.data, w.ctypes.data, 9, 1),
                 (4, 65, m.ctypes.data, w.ctypes.data, w.ctypes.data, 1, 1), (4, 8, None, w.ctypes.data, w.ctypes.data, 2, 1),
                 (4, 8, m.ctypes.data, None, w.ctypes.data, 2, 1), (4, 8, m.ctypes.data, w.ctypes.data, None, 2, 1),
                 (4, 8, m.ctypes.data, w.ctypes.data, w.ctypes.data, 2, -1)]:
        assert step(*args) == GOL_EINVAL, args
    assert not w.any()
    for table in (np.zeros(15, np.uint32), np.zeros(16, np.float32), np.full(16, -1, np.int64), np.zeros((2, 16), np.uint32)):
        with pytest.raises(G.GolError):
            G.format_map(table)
    with pytest.raises(G.GolError):
        G.map_from_rule((512, 0))
    # the launch check under maps: of a pointer only whether it is NULL counts
    chk = L.gol_batch_step_map_check_host
    p = 64
    plain = [p, None, None, 5, 5, 17, 3, 0, 0, 0, p, 0, 0, 0, None, None, 0, None, None]
    aged = [p, p, p, 5, 5, 17, 3, 0, 0, 1, p, 0, 2, 0, p, p, 5, None, p]
    assert chk(*plain) == GOL_OK and chk(*aged) == GOL_OK
    each = list(plain)
    each[11] = 1
    assert chk(*each) == GOL_OK
    for at, value in ((10, None), (0, None), (6, 0), (12, 1), (4, 513)):
        a = list(plain)
        a[at] = value
        assert chk(*a) == GOL_EINVAL, (at, value)
    a = list(aged)
    a[11] = 1  # the aged search has one map
    assert chk(*a) == GOL_EINVAL


def test_map_check_program():
    """build/asan/map_check: the host twin, the codec and the launch check under AddressSanitizer + UBSan, on heap
    blocks of exact size (a plain child process)."""
    r = subprocess.run([check_program("map_check")], capture_output=True, text=True)
    assert r.returncode == 0 and ", 0 bad" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
