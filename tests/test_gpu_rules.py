"""Life-like rules on the GPU (gol_engine_set_rule, csrc/gol_kernels.hip: TableRule) against the numpy torus
stepper of tests/rule_ref.py (itself checked against the oracle in test_rules_cpu.py).  Boards come
from a seeded numpy RNG at densities 0.1, 0.5 and 0.9 and are loaded through load_bytes as 0/255.
"""
import ctypes
import functools
import os

import numpy as np
import pytest

import rule_ref as R
from oracle import oracle as O
from testlib import gpu_lib as golhip  # noqa: F401 (the fixture)

pytestmark = pytest.mark.gpu

DENSITIES = (0.1, 0.5, 0.9)
TURNS = (1, 7, 8, 29)
RULES = ["B36/S23", "B3678/S34678", "B2/S", "B1357/S1357", "B0123478/S01234678"]
# (layout, H, W): the rule kernels hold 64 cells per lane in both layouts, so a standard wave's
# column group is 124 words -- 33 x 2112 (Wd = 66) fits one group, 100 x 4032 (Wd = 126) takes
# two and 33 x 8000 (Wd = 250) three; a band wave at k = 8 keeps 112 words, so Wd = 128 / 288 are
# two / three groups with the band-wrap rotation in the last.
SHAPES = [
    ("standard", 16, 64),
    ("standard", 5, 192),
    ("standard", 33, 2112),
    ("standard", 100, 4032),
    ("standard", 33, 8000),
    ("band", 40, 1024),
    ("band", 64, 4096),
    ("band", 24, 9216),
]
SINGLE_BIT = [(1 << n, 0) for n in range(9)] + [(0, 1 << n) for n in range(9)]


def _seed(H, W, density):
    return H * 1000003 + W * 101 + int(density * 10)


@functools.lru_cache(maxsize=None)
def _reference(H, W, density, rule, turns=max(TURNS)):
    """(start board, counts after every turn, boards after the turns of TURNS) -- computed once."""
    start = R.random_board(_seed(H, W, density), H, W, density)
    _, counts, kept = R.run(start, rule, turns, keep=TURNS)
    for a in (start, *kept.values()):
        a.setflags(write=False)
    return start, counts, kept


def _engine(G, layout, H, W, **kw):
    e = G.Engine(H, W, device=0, layout="standard" if layout == "standard" else "auto", **kw)
    assert e.info()["layout"] == layout
    return e


# ------------------------------------------------------------------ every mask bit
@pytest.mark.parametrize("layout", ["band", "standard"])
def test_single_bit_rules_one_turn(golhip, layout):
    H, W = 64, 1024
    start = R.random_board(_seed(H, W, 0.5), H, W, 0.5)
    n = R.neighbours(start)
    for centre in (0, 1):  # the board exercises every mask bit
        assert sorted(set(n[start == centre].tolist())) == list(range(9))
    with _engine(golhip, layout, H, W) as e:
        for birth, survive in SINGLE_BIT:
            e.load_bytes(R.to_bytes(start))
            e.set_rule((birth, survive))
            e.step(1)
            want = R.step(start, birth, survive)
            assert np.array_equal(e.store_bytes(), R.to_bytes(want)), (birth, survive)
            assert e.alive_count() == int(want.sum())


# ------------------------------------------------------------------ rules x turns x layouts
@pytest.mark.parametrize("rule", RULES)
@pytest.mark.parametrize("layout,H,W", SHAPES)
def test_rules_turns_layouts(golhip, layout, H, W, rule):
    with _engine(golhip, layout, H, W, rule=rule) as e:
        assert e.rule == rule and e.rule_generic and e.info()["turns_per_launch"] == min(8, 1 << (H.bit_length() - 1))
        for density in DENSITIES:
            start, counts, kept = _reference(H, W, density, rule)
            for turns in TURNS:
                e.load_bytes(R.to_bytes(start))
                e.step(turns)
                assert np.array_equal(e.store_bytes(), R.to_bytes(kept[turns])), (density, turns)
                assert e.alive_count() == counts[turns - 1], (density, turns)
            e.load_bytes(R.to_bytes(start))
            assert e.step_counted(max(TURNS), 1).tolist() == counts, density
            assert np.array_equal(e.store_bytes(), R.to_bytes(kept[max(TURNS)])), density


# ------------------------------------------------------------------ Conway through the rule kernels
def test_conway_on_the_rule_kernels_is_golden(golhip, golden_dir):
    _, _, board = O.read_pgm(os.path.join(golden_dir, "images", "512x512.pgm"), 512, 512)
    csv = O.read_alive_csv(os.path.join(golden_dir, "check", "alive", "512x512.csv"))
    with golhip.Engine(512, 512, device=0) as e:
        default_info = e.info()
        e.load_bytes(board)
        e.set_rule("B3/S23", generic=True)
        assert e.rule == "B3/S23" and e.rule_generic
        assert e.step_counted(100, 1).tolist() == [csv[t] for t in range(1, 101)]
        got = e.store_bytes()
        with open(os.path.join(golden_dir, "check", "images", "512x512x100.pgm"), "rb") as f:
            assert O.pgm_bytes(got) == f.read()
        e.set_rule("B3/S23")
        assert e.rule == "B3/S23" and not e.rule_generic and e.info() == default_info
        assert e.step_counted(20, 1).tolist() == [csv[t] for t in range(101, 121)]
        assert e.turn == 120 and np.array_equal(e.store_bytes(), O.run(got, 20))


def test_generic_flag_switches_the_band_kernels(golhip):
    """On a band board the default path is the k = 12 pipeline at 128 cells per lane; under the
    rule kernels info() reports their k = 8 at 64, and B3/S23 with flags 0 restores the default."""
    with golhip.Engine(64, 1024, device=0) as e:
        default_info = e.info()
        assert default_info["layout"] == "band" and default_info["turns_per_launch"] == 12
        e.load_random(5)
        ref = O.bits_run(O.random_words(5, 0, 64, 16), 37)
        e.set_rule("B3/S23", generic=True)
        assert e.info()["turns_per_launch"] == 8 and e.info()["cells_per_lane"] == 64 and e.info()["layout"] == "band"
        e.step(37)
        assert e.hash() == O.hash_words(ref)
        e.set_rule("B3/S23")
        assert e.info() == default_info
        e.step(24)
        assert e.hash() == O.hash_words(O.bits_run(ref, 24)) and e.turn == 61


# ------------------------------------------------------------------ rule changed mid-run
@pytest.mark.parametrize("layout,H,W", [("band", 40, 1024), ("standard", 33, 2112)])
def test_rule_changed_mid_run(golhip, layout, H, W):
    start = R.random_board(_seed(H, W, 0.5), H, W, 0.5)
    mid, _, _ = R.run(start, "B3/S23", 8)
    want, counts, _ = R.run(mid, "B36/S23", 8)
    with _engine(golhip, layout, H, W) as e:
        e.load_bytes(R.to_bytes(start))
        e.step(8)
        e.set_rule("B36/S23")
        assert e.turn == 8 and np.array_equal(e.store_bytes(), R.to_bytes(mid))
        e.step(8)
        assert e.turn == 16
        assert np.array_equal(e.store_bytes(), R.to_bytes(want)) and e.alive_count() == counts[-1]


# ------------------------------------------------------------------ step_flips and views
@pytest.mark.parametrize("layout,H,W", [("band", 40, 1024), ("standard", 16, 64)])
def test_step_flips_and_views_under_highlife(golhip, layout, H, W):
    start = R.random_board(_seed(H, W, 0.5), H, W, 0.5)
    with _engine(golhip, layout, H, W, rule="B36/S23") as e:
        e.load_bytes(R.to_bytes(start))
        prev = start
        for _ in range(3):
            cur = R.step(prev, *R.masks("B36/S23"))
            ys, xs = np.nonzero(prev ^ cur)  # row-major
            flips = e.step_flips()
            assert flips.tolist() == np.stack([xs, ys], axis=1).tolist()
            prev = cur
        assert e.turn == 3
        e.step(8)  # (back in the stepping layout)
        scale = 8
        tiles = e.view_counts(0, 0, scale, W // scale, H // scale)
        assert int(tiles.sum()) == e.alive_count() == R.run(prev, "B36/S23", 8)[1][-1]


# ------------------------------------------------------------------ shards
@pytest.mark.parametrize("layout,H,W", [("band", 96, 1024), ("standard", 50, 192)])
def test_three_loopback_shards(golhip, layout, H, W):
    rule, turns = "B3678/S34678", 29
    start = R.random_board(_seed(H, W, 0.5), H, W, 0.5)
    want, counts, _ = R.run(start, rule, turns)
    got = []
    for shards in (1, 3):
        kw = dict(shards=3, same_device=True, transport="loopback") if shards == 3 else {}
        with _engine(golhip, layout, H, W, rule=rule, **kw) as e:
            assert e.topology()["shards"] == shards
            e.load_bytes(R.to_bytes(start))
            assert e.step_counted(turns, 1).tolist() == counts
            got.append(e.store_bytes())
    assert np.array_equal(got[0], got[1]) and np.array_equal(got[1], R.to_bytes(want))


# ------------------------------------------------------------------ reference-free at scale
def test_parity_rule_at_scale(golhip):
    """B1357/S02468: a cell is alive next turn iff its 3x3 block (centre included) holds an odd
    number of alive cells -- linear over GF(2), so 2^m turns are the XOR of the nine copies of the
    start board rolled by (+-2^m or 0, +-2^m or 0).  64 turns on 8192^2, checked on the words."""
    N, turns = 8192, 64
    with golhip.Engine(N, N, device=0, rule="B1357/S02468") as e:
        assert e.info()["layout"] == "band"
        e.load_random(11)
        start = e.store_words(0, N)
        e.step(turns)
        got = e.store_words(0, N)
        assert e.turn == turns
    want = np.zeros_like(start)
    for dy in (-turns, 0, turns):
        for dw in (-turns // 64, 0, turns // 64):  # 64 cells = one uint64 word
            want ^= np.roll(np.roll(start, dy, axis=0), dw, axis=1)
    assert np.array_equal(got, want)


# ------------------------------------------------------------------ errors
def _unchanged(e, board, turn):
    return e.turn == turn and np.array_equal(e.store_bytes(), board)


def test_set_rule_errors_change_nothing(golhip):
    EINVAL, ESTATE = golhip._lib.GOL_EINVAL, golhip._lib.GOL_ESTATE
    L = golhip.lib()
    board = R.to_bytes(R.random_board(3, 16, 64, 0.5))
    with golhip.Engine(16, 64, device=0) as e:
        e.load_bytes(board)
        e.step(2)
        now = e.store_bytes()
        for masks in ((512, 0), (0, 512), (1 << 31, 12)):
            with pytest.raises(golhip.GolError) as x:
                e.set_rule(masks)
            assert x.value.code == EINVAL
        for flags in (2, 3, -1, 1 << 16):
            assert L.gol_engine_set_rule(e._h, 0x048, 0x00C, flags) == EINVAL
        assert e.rule == "B3/S23" and not e.rule_generic and _unchanged(e, now, 2)
    for kw, W in ((dict(), 100), (dict(layout="bytes"), 64)):  # not bit-capable
        wide = R.to_bytes(R.random_board(4, 16, W, 0.5))
        with golhip.Engine(16, W, device=0, **kw) as e:
            e.load_bytes(wide)
            e.step(1)
            now = e.store_bytes()
            for rule, generic in (("B36/S23", False), ("B3/S23", True)):
                with pytest.raises(golhip.GolError) as x:
                    e.set_rule(rule, generic=generic)
                assert x.value.code == EINVAL
            e.set_rule("B3/S23")  # the default rule is always accepted
            assert e.rule == "B3/S23" and not e.rule_generic and _unchanged(e, now, 1)
    # loaded bytes other than 0/255: their first turn is defined for B3/S23 only
    odd = board.copy()
    odd[3, 5] = 7
    with golhip.Engine(16, 64, device=0, rule="B36/S23") as e:
        e.load_bytes(odd)
        xy = np.zeros((16, 2), dtype=np.int32)
        n = ctypes.c_int64()
        counts = np.zeros(4, dtype=np.uint64)
        assert L.gol_engine_step(e._h, 1) == ESTATE
        assert L.gol_engine_step_counted(e._h, 4, 1, counts.ctypes.data, 4) == ESTATE
        assert L.gol_engine_step_flips(e._h, xy.ctypes.data, 16, ctypes.byref(n)) == ESTATE
        assert _unchanged(e, odd, 0)
        e.set_rule("B3/S23")  # B3/S23 takes the exact first turn
        e.step(1)
        assert e.turn == 1 and np.array_equal(e.store_bytes(), O.run(odd, 1))


# ------------------------------------------------------------------ the device launcher
@pytest.mark.parametrize("layout", ["standard", "band"])
def test_dev_rule_step_on_caller_memory(golhip, layout):
    import torch
    L = golhip.lib()
    H, W, rule = 64, 4096, "B36/S23"
    birth, survive = R.masks(rule)
    start, counts, kept = _reference(H, W, 0.5, rule)
    Wd = W // 32
    words = O.pack(R.to_bytes(start))
    src32 = O.to_band(words) if layout == "band" else words.view(np.uint32)
    lay = golhip._lib.GOL_LAYOUT_BAND if layout == "band" else golhip._lib.GOL_LAYOUT_STANDARD
    a = torch.from_numpy(np.ascontiguousarray(src32).view(np.int32).copy()).cuda()
    b = torch.zeros_like(a)
    slots = torch.zeros(golhip._lib.GOL_COUNT_SLOTS * 8, dtype=torch.int64, device="cuda")
    ref, t = (start != 0).astype(np.uint8), 0
    for k in (1, 2, 4, 8):
        slots.zero_()
        torch.cuda.synchronize()
        mid = a.data_ptr()
        rc = L.gol_dev_rule_step(mid + (H - k) * Wd * 4, mid, mid, b.data_ptr(), H, Wd, Wd, 0, H, k, lay, birth, survive,
                                 0, 0, slots.data_ptr(), None)
        assert rc == 0, L.gol_last_error()
        torch.cuda.synchronize()
        flags = ctypes.c_uint32()
        assert L.gol_dev_error(-1, ctypes.byref(flags)) == 0 and flags.value == 0
        ref, cs, _ = R.run(ref, rule, k)
        t += k
        out32 = b.cpu().numpy().view(np.uint32)
        got = O.from_band(out32) if layout == "band" else np.ascontiguousarray(out32).view(np.uint64)
        assert np.array_equal(O.unpack(got), R.to_bytes(ref)), k
        assert int(slots.sum().item()) == cs[-1] == counts[t - 1], k
        a, b = b, a
    # bad arguments are refused before any launch
    for bad in (dict(k=3), dict(k=16), dict(lay=0), dict(lay=3), dict(birth=512), dict(survive=512), dict(cpl=128)):
        args = dict(k=1, lay=lay, birth=birth, survive=survive, cpl=0)
        args.update(bad)
        rc = L.gol_dev_rule_step(a.data_ptr(), a.data_ptr(), a.data_ptr(), b.data_ptr(), H, Wd, Wd, 0, H, args["k"],
                                 args["lay"], args["birth"], args["survive"], args["cpl"], 0, None, None)
        assert rc == golhip._lib.GOL_EINVAL, bad
