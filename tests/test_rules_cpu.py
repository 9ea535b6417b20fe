"""Life-like rules, the parts that need no GPU: the rule text codec (gol_rule_parse /
gol_rule_format), the numpy reference stepper the GPU tests compare against (tests/rule_ref.py,
itself checked against the oracle and the reference's golden board), and the circuit of the rule
kernels (csrc/gol_rule.h through gol_rule_eval_host) on every 3x3 neighbourhood.
"""
import ctypes
import os

import numpy as np
import pytest

import rule_ref as R
from oracle import oracle as O
from testlib import cpu_lib as G  # noqa: F401 (the fixture)

CANONICAL = {
    "B3/S23": (0x008, 0x00C),
    "B36/S23": (0x048, 0x00C),
    "B3678/S34678": (0x1C8, 0x1D8),
    "B2/S": (0x004, 0x000),
    "B/S": (0x000, 0x000),
    "B012345678/S012345678": (0x1FF, 0x1FF),
}
MALFORMED = [
    "B9/S23", "B3/S29",            # a digit 9
    "B33/S23", "B3/S232",          # a repeated digit
    "B3", "B3/", "/S23", "S23", "", "3/23", "B3S23",  # a missing half
    "B3/S23x", "B3/S23 ", "B3/S23/", "B3/S23\n", "B3/S2 3",  # trailing text
]
SINGLE_BIT = [(1 << n, 0) for n in range(9)] + [(0, 1 << n) for n in range(9)]
CIRCUIT_RULES = SINGLE_BIT + [R.masks(t) for t in ("B3/S23", "B36/S23", "B3678/S34678", "B0123478/S01234678")]


@pytest.mark.parametrize("text", sorted(CANONICAL))
def test_parse_format_round_trip(G, text):
    assert G.parse_rule(text) == CANONICAL[text] == R.masks(text)
    assert G.format_rule(*CANONICAL[text]) == text
    assert G.parse_rule(text.lower()) == CANONICAL[text]


def test_parse_accepts_any_digit_order(G):
    assert G.parse_rule("b8763/s87643") == CANONICAL["B3678/S34678"]
    assert G.format_rule(*G.parse_rule("B63/S32")) == "B36/S23"


@pytest.mark.parametrize("text", MALFORMED)
def test_parse_rejects_malformed(G, text):
    with pytest.raises(G.GolError) as x:
        G.parse_rule(text)
    assert x.value.code == G._lib.GOL_EINVAL


def test_format_errors(G):
    L = G.lib()
    buf = ctypes.create_string_buffer(32)
    assert L.gol_rule_format(512, 0, buf, 32) == G._lib.GOL_EINVAL
    assert L.gol_rule_format(0, 512, buf, 32) == G._lib.GOL_EINVAL
    assert L.gol_rule_format(0x1FF, 0x1FF, buf, 21) == G._lib.GOL_EINVAL  # 22 bytes with the NUL
    assert L.gol_rule_format(0x1FF, 0x1FF, buf, 22) == 0 and buf.value == b"B012345678/S012345678"
    assert L.gol_rule_format(0, 0, buf, 4) == 0 and buf.value == b"B/S"


# ------------------------------------------------------------------ the numpy stepper itself
@pytest.mark.parametrize("size", [16, 64])
def test_stepper_is_the_oracle_for_conway(size):
    rng = np.random.default_rng(size)
    for density in (0.1, 0.5, 0.9):
        board = (rng.random((size, size)) < density).astype(np.uint8)
        want = O.run(R.to_bytes(board), 1)
        assert np.array_equal(R.to_bytes(R.step(board, *R.CONWAY)), want)


def test_stepper_reproduces_golden_512(golden_dir):
    _, _, board = O.read_pgm(os.path.join(golden_dir, "images", "512x512.pgm"), 512, 512)
    _, _, gold = O.read_pgm(os.path.join(golden_dir, "check", "images", "512x512x100.pgm"))
    final, counts, _ = R.run(R.from_bytes(board), "B3/S23", 100)
    assert np.array_equal(R.to_bytes(final), gold)
    csv = O.read_alive_csv(os.path.join(golden_dir, "check", "alive", "512x512.csv"))
    assert counts == [csv[t] for t in range(1, 101)]


# ------------------------------------------------------------------ the kernels' circuit on the host
def _all_neighbourhoods():
    """All 512 (centre, 8 neighbours) patterns bit-sliced into 16 words: cell i = 32 w + bit has
    neighbour j = bit j of i and centre = bit 8 of i."""
    idx = np.arange(512, dtype=np.uint32).reshape(16, 32)
    weights = (np.uint32(1) << np.arange(32, dtype=np.uint32))[None, :]
    planes = [(((idx >> j) & 1) * weights).sum(axis=1).astype(np.uint32) for j in range(9)]
    return planes[:8], planes[8]


@pytest.mark.parametrize("birth,survive", CIRCUIT_RULES)
def test_eval_host_is_the_mask_definition(G, birth, survive):
    L = G.lib()
    nb, centre = _all_neighbourhoods()
    for w in range(16):
        arr = (ctypes.c_uint32 * 8)(*[int(p[w]) for p in nb])
        out = ctypes.c_uint32()
        assert L.gol_rule_eval_host(birth, survive, arr, int(centre[w]), ctypes.byref(out)) == 0
        for bit in range(32):
            i = 32 * w + bit
            n = bin(i & 0xFF).count("1")
            want = (survive >> n) & 1 if i >> 8 else (birth >> n) & 1
            assert (out.value >> bit) & 1 == want, (birth, survive, i)


def test_eval_host_errors(G):
    L = G.lib()
    arr = (ctypes.c_uint32 * 8)()
    out = ctypes.c_uint32()
    assert L.gol_rule_eval_host(512, 0, arr, 0, ctypes.byref(out)) == G._lib.GOL_EINVAL
    assert L.gol_rule_eval_host(0, 512, arr, 0, ctypes.byref(out)) == G._lib.GOL_EINVAL
    assert L.gol_rule_eval_host(8, 12, None, 0, ctypes.byref(out)) == G._lib.GOL_EINVAL
    assert L.gol_rule_eval_host(8, 12, arr, 0, None) == G._lib.GOL_EINVAL
