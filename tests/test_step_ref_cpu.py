"""tests/step_ref.py on the CPU: its layout helpers and expected() against the C oracle, and the
coverage of its case table, so that a later edit cannot silently thin what
tests/test_gpu_step_kernels.py runs."""
import os
import re

import numpy as np
import pytest

import rule_ref as RR
import step_ref as S
from oracle import oracle as O


def _cells(seed, H, Wd):
    return RR.random_board(seed, H, 32 * Wd, S.DENSITY)


# ------------------------------------------------------------------ layouts
@pytest.mark.parametrize("Wd", [1, 2, 3, 4, 61, 63, 64, 126])
def test_layouts_round_trip(Wd):
    cells = _cells(Wd, 5, Wd)
    for pack, unpack in ((S.std_pack, S.std_unpack), (S.band_pack, S.band_unpack)):
        words = pack(cells)
        assert words.dtype == np.uint32 and words.shape == (5, Wd)
        assert np.array_equal(unpack(words), cells)
        assert S.popcount(words) == int(cells.sum())
    # the definitions, cell by cell
    std, band = S.std_pack(cells), S.band_pack(cells)
    for x in (0, 1, 31, 32 * Wd - 1, (32 * Wd) // 2, Wd, Wd - 1):
        assert np.array_equal((std[:, x // 32] >> np.uint32(x % 32)) & 1, cells[:, x])
        assert np.array_equal((band[:, x % Wd] >> np.uint32(x // Wd)) & 1, cells[:, x])


@pytest.mark.parametrize("Wd", [2, 4, 6, 32, 96])
def test_layouts_agree_with_the_oracle(Wd):
    cells = _cells(100 + Wd, 7, Wd)
    words = O.pack(RR.to_bytes(cells))  # uint64 rows, W % 64 == 0
    assert np.array_equal(S.std_pack(cells), words.view(np.uint32))
    assert np.array_equal(S.std_unpack(words.view(np.uint32)), RR.from_bytes(O.unpack(words)))
    band = O.to_band(words)
    assert np.array_equal(S.band_pack(cells), band)
    assert np.array_equal(O.from_band(S.band_pack(cells)), words)
    assert np.array_equal(S.band_unpack(band), cells)
    assert S.popcount(band) == O.popcount_words(words)


# ------------------------------------------------------------------ expected()
@pytest.mark.parametrize("H,Wd,y0,R,k", [
    (16, 2, 0, 16, 8),    # the whole torus
    (1, 1, 0, 1, 1),      # one row, one word: every neighbour is a wrapped copy
    (9, 3, 0, 9, 4),      # an odd number of words
    (30, 3, 5, 19, 2),    # a shard cut from a taller torus
    (59, 5, 17, 24, 16),
])
def test_expected_agrees_with_the_oracle(H, Wd, y0, R, k):
    cells = _cells(1000 * H + Wd, H, Wd)
    want = RR.from_bytes(O.run(RR.to_bytes(cells), k))[y0:y0 + R]
    assert np.array_equal(S.expected(cells, y0, R, k, S.CONWAY), want)
    assert np.array_equal(S.expected(cells, y0, R, k, RR.CONWAY), want)
    assert RR.masks(S.CONWAY) == (0x008, 0x00C)


def test_stepped_is_expected_and_shared():
    c = S.cases_of(("band", 4, 2))[3]
    t = S.torus(c.seed, c.H, c.Wd)
    assert abs(float(t.mean()) - S.DENSITY) < 0.05
    assert np.array_equal(S.stepped(c.seed, c.H, c.Wd, c.rule, c.k), S.expected(t, 0, c.H, c.k, c.rule))
    assert S.stepped(c.seed, c.H, c.Wd, c.rule, c.k) is S.stepped(c.seed, c.H, c.Wd, c.rule, c.k)
    assert not t.flags.writeable


# ------------------------------------------------------------------ the case table
def test_every_instantiation_is_listed():
    """step_ref's table is the library's: what gol_step_check_host (the kernel table of
    csrc/gol_step_launch.h) answers for every (family, k, words per lane), no hand-kept second list."""
    import golhip
    check, fam = golhip.lib().gol_step_check_host, golhip._lib.STEP_FAMILIES
    P = S.P

    def is_kernel(f, k, dw, as_entry):
        W = 128 if f != "bytes" else 4096  # a multiple of every unit; R = 64 rows >= every k
        return check(fam[f], P, P, P, P, 64, W, W, 0, 64, k, dw, 0, 0, 0, 0, as_entry, None) == 0
    every = [(f, k, dw) for f in S.FAMILIES for k in range(1, 34) for dw in (1, 2, 3, 4)]
    listed = {i for i in every if is_kernel(*i, 0)}
    offered = {i for i in every if is_kernel(*i, 1)}
    assert listed == set(S.TABLE) and listed - offered == set(S.ENGINE_ONLY) == {("band", 12, 2)}
    want = {i for i in listed if i[0] != "bytes" and "pipelined" not in S.TABLE[i]}
    assert set(S.INSTANTIATIONS) == want and len(S.INSTANTIATIONS) == len(want) == 32
    assert set(S.PUBLIC) == want & offered and len(S.PUBLIC) == 31
    assert {c.inst for c in S.CASES} == set(S.PUBLIC)
    assert len({c.id for c in S.CASES}) == len(S.CASES)
    # the rule kernels' words per lane, from the source
    h = os.path.join(os.path.dirname(__file__), "..", "gol-distributed-final_amd", "csrc", "gol_step_launch.h")
    with open(h) as f:
        assert int(re.search(r"#define GOLK_RULE_DW (\d+)", f.read()).group(1)) == S.RULE_DW


def test_width_classes_are_the_column_group_edges():
    assert S.widths(("bits", 8, 1)) == {"one-lane": 1, "under-group": 61, "exact-group": 62, "one-lane-over": 63}
    assert S.useful_words(("band", 16, 2)) == 96 and S.useful_words(("band", 8, 4)) == 240
    assert S.useful_words(("band", 1, 4)) == 248 and S.useful_words(("rule_band", 8, 2)) == 112
    assert S.useful_words(("rule_std", 8, 2)) == 124
    assert max(c.Wd for c in S.CASES) == 252
    for c in S.CASES:
        U = S.useful_words(c.inst)
        assert c.Wd == {"one-lane": c.dw, "under-group": U - c.dw, "exact-group": U, "one-lane-over": U + c.dw}[c.wclass]


@pytest.mark.parametrize("inst", S.PUBLIC, ids=S.inst_id)
def test_coverage_of_an_instantiation(inst):
    cases = S.cases_of(inst)
    rules = S.RULES if inst[0].startswith("rule") else (S.CONWAY,)
    assert RR.masks(S.RULES[2])[0] & 1  # birth on 0 neighbours
    for rule in rules:
        mine = [c for c in cases if c.rule == rule]
        for wclass in S.WIDTH_CLASSES:
            at = [c for c in mine if c.wclass == wclass]
            assert {c.form for c in at} == set(S.FORMS), (rule, wclass)
            assert any(c.R == c.k and c.form == "wrap" and c.rows == c.R for c in at), (rule, wclass)
            assert any(c.R >= 19 and c.row0 > 0 and c.row0 + c.rows < c.R for c in at), (rule, wclass)
            # both values of the contiguity predicate the band launcher computes, on word
            # addresses with the allocations far apart
            bases = {"src": 1 << 20, "top": 2 << 20, "mid": 3 << 20, "bot": 4 << 20, "dst": 5 << 20}
            assert {c.contiguous(bases) for c in at} == {False, True}, (rule, wclass)
            for c in at:
                assert c.contiguous(bases) == (c.form == "contig")
        full = {n for c in mine for n in c.strips() if n == c.strip}
        tail = {n for c in mine for n in c.strips() if n < c.strip}
        assert full >= set(S.STRIP_LENGTHS) and tail >= set(S.STRIP_LENGTHS), (rule, full, tail)
        sweep = [c for c in mine if c.tag == "sweep"]
        assert {c.strip for c in sweep} >= {0, 1, 2, 3, 4, 5, 6}
        assert len({c.wclass for c in sweep}) == 1
    assert {c.rule for c in cases} == set(rules)


def test_the_sweep_reaches_every_width_class():
    for kind in ("bits", "band", "rule_std", "rule_band"):
        assert {c.wclass for c in S.CASES if c.tag == "sweep" and c.kind == kind} == set(S.WIDTH_CLASSES)


def test_every_case_is_a_valid_call():
    for c in S.CASES:
        S.check_args(c)
        assert c.pitch > c.Wd and c.pitch % 4 == 0
        if c.form == "wrap":
            assert c.H == c.R and c.y0 == 0
        else:  # no ghost row is a wrap row of the shard
            assert c.H >= c.R + 2 * c.k + 3 and c.y0 - c.k >= 1 and c.y0 + c.R + c.k <= c.H - 1


def test_buffers_hold_the_torus_and_the_sentinel():
    for c in (S.cases_of(("bits", 2, 1))[0], S.cases_of(("band", 4, 4))[9], S.cases_of(("rule_band", 8, 2))[-1],
              S.cases_of(("bits", 16, 2))[4]):
        bufs, ptr = c.buffers(), c.pointers()
        unpack = S.band_unpack if c.band else S.std_unpack
        t = S.torus(c.seed, c.H, c.Wd)
        assert set(bufs) == set(c.allocs()) and bool((bufs["dst"] == S.SENT).all())

        def row(name, i):  # row i of what pointer `name` addresses
            al, off = ptr[name]
            return bufs[al].reshape(-1)[off + i * c.pitch: off + i * c.pitch + c.Wd][None, :]
        for y in range(-c.k, c.R + c.k):  # the header's row addressing
            got = row("top", y + c.k) if y < 0 else (row("mid", y) if y < c.R else row("bot", y - c.R))
            assert np.array_equal(unpack(got)[0], t[(c.y0 + y) % c.H]), (c.id, y)
        for name, b in bufs.items():
            assert bool((b[:S.GUARD] == S.SENT).all()) and bool((b[-S.GUARD:] == S.SENT).all())
            assert bool((b[:, c.Wd:] == S.SENT).all())
        if c.form == "separate":  # mid's neighbours are the sentinel, not the ghost rows
            al, off = ptr["mid"]
            flat = bufs[al].reshape(-1)
            assert bool((flat[off - c.pitch: off] == S.SENT).all())
            assert bool((flat[off + c.R * c.pitch: off + (c.R + 1) * c.pitch] == S.SENT).all())
        assert np.array_equal(unpack(c.want_words()),
                              S.expected(t, c.y0 + c.row0, c.rows, c.k, c.rule))
