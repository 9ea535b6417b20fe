"""The island census without a GPU: the reference of tests/island_ref.py against the pins of its definition
and under torus translations, the coverage of the GPU tests' case table, the host twin
(gol_batch_islands_host: the row functions of csrc/gol_island.h that the kernel runs) against the reference
over every width class and height class, the stand-alone driver under AddressSanitizer +
UndefinedBehaviorSanitizer (build/asan/island_check, a plain child process; nothing loaded into Python is
sanitized), the refusals of the launch check, golhip.island, and the precondition of the GPU soup test.  All
comparisons are exact."""
import ctypes
import subprocess

import numpy as np
import pytest

import island_ref as I
from testlib import GOL_EINVAL, check_program, cpu_lib as G  # noqa: F401 (the fixture)


def host_census(G, cells, reach, cap=None, stride_pad=0):
    """(count, records[:min(count, cap)], fingerprint) of one board through the host twin; the rows `stride_pad`
    words apart more than they need, the gaps and the padding bits set."""
    cells = np.asarray(cells) != 0
    H, W = cells.shape
    cap = H * W if cap is None else cap
    packed = G.Batch.pack(cells.astype(np.uint8))
    Ww = packed.shape[1]
    words = np.full((H, Ww + stride_pad), 0xA5A5A5A5A5A5A5A5, dtype=np.uint64)
    words[:, :Ww] = packed
    if W % 64:
        words[:, Ww - 1] |= np.uint64(0xA5A5A5A5A5A5A5A5) & ~np.uint64((1 << (W % 64)) - 1)
    count, fp = ctypes.c_int64(-7), ctypes.c_uint64(7)
    recs = np.zeros(cap, dtype=I.DTYPE)
    rc = G.lib().gol_batch_islands_host(H, W, reach, words.ctypes.data, words.shape[1], cap, ctypes.byref(count),
                                        recs.ctypes.data if cap else None, ctypes.byref(fp))
    assert rc == 0, G.lib().gol_last_error()
    return count.value, recs[:min(count.value, cap)], fp.value


def assert_same(got, want, where):
    count, recs, fp = got
    wrecs, wfp = want
    assert count == len(wrecs), (where, count, len(wrecs))
    assert fp == wfp, (where, hex(fp), hex(wfp))
    assert np.array_equal(recs, wrecs[:len(recs)]), (where, recs[:4], wrecs[:4])


def _board(H, W, cells):
    b = np.zeros((H, W), dtype=bool)
    for y, x in cells:
        b[y, x] = True
    return b


PINS = [
    # board, reach 1 records, reach 2 records (None: only the hash of the one island is pinned)
    (_board(20, 23, [(0, 0), (0, 22), (19, 0), (19, 22)]), [(0, 0, 4, 2, 2, 0x2f7e9475b36427ed)], [0x9a56b1010f39d79e]),
    (_board(20, 23, [(7, 5), (7, 6), (7, 7)]), [(7, 5, 3, 1, 3, 0xfb99c73de5f3c455)], [0x6472b898654a3662]),
    (_board(1, 1, [(0, 0)]), [0x78e38ffaab5e3d13], [0xb9ea5f4af8d1b97c]),
    (_board(9, 9, [(0, 0), (0, 2), (3, 0)]), [0xdba967c400668247] * 3,
     [(0, 0, 2, 1, 2, 0xfb12bf5c90da5ae1), (3, 0, 1, 1, 1, 0x2c717d4ad4345753)]),
]


def _check_pin(recs, pin):
    assert len(recs) == len(pin)
    for r, p in zip(recs, pin):
        if isinstance(p, tuple):
            assert tuple(int(v) for v in r.tolist()) == p
        else:
            assert int(r["hash"]) == p


@pytest.mark.parametrize("k", range(len(PINS)))
def test_pins_reference(k):
    board, p1, p2 = PINS[k]
    for reach, pin in ((1, p1), (2, p2)):
        recs, fp = I.census(board, reach)
        _check_pin(recs, pin)
        assert fp == sum(int(r["hash"]) for r in recs) & I.M64


@pytest.mark.parametrize("k", range(len(PINS)))
def test_pins_host_twin(G, k):
    board, p1, p2 = PINS[k]
    for reach, pin in ((1, p1), (2, p2)):
        count, recs, _ = host_census(G, board, reach)
        assert count == len(pin)
        _check_pin(recs, pin)


def test_reference_translation_invariance():
    """Shifts that carry an island over the row seam, the column seam, a word boundary and the corner, and
    random ones: equal fingerprints and equal multisets of (cells, rows, cols, hash)."""
    rng = np.random.default_rng(5)
    for H, W in ((20, 23), (9, 70), (66, 40)):
        board = rng.random((H, W)) < 0.12
        board[2:4, 3:5] = True  # a block, carried over each seam below
        for reach in (1, 2):
            recs, fp = I.census(board, reach)
            shifts = [(H - 3, 0), (0, W - 4), (H - 3, W - 4), (0, 32 - 4), (0, 64 - 4), (H - 2, W - 3)]
            shifts += [tuple(int(v) for v in rng.integers(0, (H, W))) for _ in range(4)]
            for dy, dx in shifts:
                r2, fp2 = I.census(np.roll(board, (dy, dx), axis=(0, 1)), reach)
                assert fp2 == fp and I.key(r2) == I.key(recs), (H, W, reach, dy, dx)
    # and it does change under rotation
    glider = np.array([[0, 1, 0], [0, 0, 1], [1, 1, 1]])
    assert I.lone(glider, 1)[3] != I.lone(np.rot90(glider), 1)[3]


def test_case_table_coverage():
    tags = set().union(*(c.tags for c in I.CASES))
    assert len({c.id for c in I.CASES}) == len(I.CASES)
    for nw in I.WORDS:
        mine = [c for c in I.CASES if f"nw{nw}" in c.tags]
        assert {I.nw_of(c.shape[1]) for c in mine} == {nw}
        assert {c.shape[1] for c in mine} >= {16 * nw + 1, 32 * nw - 1, 32 * nw}
        assert {c.shape[0] for c in mine} == set(I.HEIGHTS), nw
        if nw >= 4:  # an odd word count below NW
            assert any(((c.shape[1] + 31) // 32) % 2 == 1 and (c.shape[1] + 31) // 32 < nw for c in mine)
    for W in I.NARROW:
        assert {c.shape[0] for c in I.CASES if c.shape[1] == W} >= set(I.HEIGHTS)
    assert any(c.shape[0] == 512 for c in I.CASES) and any(c.shape == (512, 512) for c in I.CASES)
    assert tags >= {"colwrap", "bits31-32", "bits63-64", "rowwrap", "rows63-64", "corner", "serpentine", "diagonal",
                    "lattice2", "lattice3", "empty", "full", "five", "cap0", "cap3", "cap20"}
    # a block across every seam is one island with the block's hash, at both reaches
    for c in I.CASES:
        if "seam" in c.tags:
            for reach in c.reaches:
                recs, _ = I.want(c, reach)[0]
                assert len(recs) == 1 and I.key(recs)[0] == I.lone(I.BLOCK, reach), (c.id, reach)
            assert c.shape[1] % 32 != 0
    by = {c.id: c for c in I.CASES}
    for reach in (1, 2):
        assert len(I.want(by["serpentine-65"], reach)[0][0]) == 1
        assert len(I.want(by["diagonal-65"], reach)[0][0]) == 1
        assert len(I.want(by["lattice-3"], reach)[0][0]) == 22 * 21
    assert int(I.want(by["serpentine-65"], 1)[0][0][0]["cells"]) > 2000
    assert len(I.want(by["lattice-2"], 1)[0][0]) == 1024 > by["lattice-2"].cap  # truncation
    assert len(I.want(by["lattice-2"], 2)[0][0]) == 1
    assert [len(r) for r, _ in I.want(by["empty-full"], 1)] == [0, 1]
    five = [len(r) for r, _ in I.want(by["five-cap3"], 2)]
    assert five == [0, 1, 4, 9, 2] and by["five-cap0"].cap == 0 and min(five[2:4]) > 3 and max(five) < 20
    # the shape cases hold boards above and below their cap
    counts = [len(r) for c in I.CASES if "shape" in c.tags for r, _ in I.want(c, 1)]
    assert max(counts) > I.CAP > min(counts)


WIDTHS = list(range(1, 71)) + [95, 96, 97, 129, 257, 511, 512]


@pytest.mark.parametrize("W", WIDTHS)
def test_host_twin_widths(G, W):
    rng = np.random.default_rng(1000 + W)
    for H, dens in ((5, 0.3), (3, 0.6), (67 if W <= 70 else 9, 0.08)):
        board = rng.random((H, W)) < dens
        board[0, 0] = board[H - 1, W - 1] = True  # the corner
        for reach in (1, 2):
            assert_same(host_census(G, board, reach, stride_pad=W % 3), I.census(board, reach), (H, W, reach))


@pytest.mark.parametrize("H", [1, 2, 3, 4, 63, 64, 65, 128, 129, 512])
def test_host_twin_heights(G, H):
    rng = np.random.default_rng(2000 + H)
    for W, dens in ((7, 0.3), (33, 0.1 if H > 100 else 0.3), (130, 0.02 if H > 100 else 0.15)):
        board = rng.random((H, W)) < dens
        board[0, 0] = board[H - 1, W - 1] = True
        for reach in (1, 2):
            assert_same(host_census(G, board, reach), I.census(board, reach), (H, W, reach))


def test_host_twin_on_the_case_table_specials(G):
    for c in I.CASES:
        if "shape" in c.tags:
            continue
        for reach in c.reaches:
            for b, w in zip(c.cells, I.want(c, reach)):
                assert_same(host_census(G, b, reach), w, (c.id, reach))


def test_host_twin_cap(G):
    """count and the fingerprint cover every island; records past min(count, cap) are not touched."""
    board = _board(9, 9, [(0, 0), (0, 2), (3, 0), (6, 6)])
    wrecs, wfp = I.census(board, 1)
    words = G.Batch.pack(board.astype(np.uint8))
    for cap in (0, 2, 4, 7):
        recs = np.frombuffer(b"\xa5" * (24 * max(cap, 1)), dtype=I.DTYPE).copy()
        count, fp = ctypes.c_int64(), ctypes.c_uint64()
        rc = G.lib().gol_batch_islands_host(9, 9, 1, words.ctypes.data, 1, cap, ctypes.byref(count),
                                            recs.ctypes.data if cap else None, ctypes.byref(fp))
        assert rc == 0 and count.value == 4 and fp.value == wfp
        k = min(cap, 4)
        assert np.array_equal(recs[:k], wrecs[:k])
        assert recs[k:].tobytes() == b"\xa5" * (24 * (len(recs) - k))


def test_island_check_under_sanitizers():
    """The host twin in the stand-alone program, the board and the records heap blocks of their exact sizes,
    against a cell-by-cell flood fill."""
    r = subprocess.run([check_program("island_check")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "0 bad" in r.stdout


def test_launch_check_refusals(G):
    """gol_batch_islands_check_host: the one check every launch passes; of a pointer only its value counts."""
    check = G.lib().gol_batch_islands_check_host
    P = 0x1000  # never dereferenced
    good = dict(boards=P, n=3, H=64, W=64, reach=1, cap=8, count=P, islands=P, fingerprint=P)
    order = ("boards", "n", "H", "W", "reach", "cap", "count", "islands", "fingerprint")

    def rc(**over):
        a = dict(good, **over)
        return check(*[a[k] for k in order])

    assert rc() == 0
    assert rc(fingerprint=None) == 0 and rc(cap=0, islands=None) == 0 and rc(reach=2) == 0
    assert rc(n=1 << 20, H=512, W=512) == 0 and rc(H=1, W=1) == 0
    for bad in (dict(boards=None), dict(count=None), dict(islands=None), dict(n=0), dict(n=(1 << 20) + 1), dict(H=0),
                dict(H=513), dict(W=0), dict(W=513), dict(reach=0), dict(reach=3), dict(reach=-1), dict(cap=-1)):
        assert rc(**bad) == GOL_EINVAL, bad


BLOCK = "x = 2, y = 2\n2o$2o!"
BLINKER = "x = 3, y = 1\n3o!"
BEEHIVE = "x = 4, y = 3\nb2o$o2bo$b2o!"


def test_island_of_a_pattern(G):
    for text in (BLOCK, BLINKER, BEEHIVE):
        cells = G.parse_rle(text)[0]
        for reach in (1, 2):
            r = G.island(text, reach)
            assert r.dtype == G.ISLAND_DTYPE == I.DTYPE
            assert (int(r["cells"]), int(r["rows"]), int(r["cols"]), int(r["hash"])) == I.lone(cells, reach)
            assert G.island(np.pad(cells, 2), reach) == r  # an array, and empty margins
    assert int(G.island(BLOCK)["hash"]) == 0x2f7e9475b36427ed
    apart = np.array([[1, 0, 1]])  # two islands at reach 1, one at reach 2
    assert int(G.island(apart, 2)["cells"]) == 2
    for bad in (np.zeros((3, 3)), apart, np.ones(4)):
        with pytest.raises(G.GolError):
            G.island(bad, 1)


def test_soups_fit_the_cap(G):
    """The precondition of the GPU soup test: on those very soups, re-made on the host and stepped there, the
    reference's largest count fits the cap the GPU test asks for."""
    S = I.SOUPS
    side, most = S["side"], 0
    for i in range(S["n"]):
        words = G.Batch.soup(side, side, S["seed"], i)
        out = np.zeros_like(words)
        found, period = ctypes.c_int64(), ctypes.c_int64()
        rc = G.lib().gol_batch_cycles_host(side, side, 0x008, 0x00C, words.ctypes.data, out.ctypes.data, words.shape[1],
                                           S["turns"], ctypes.byref(found), ctypes.byref(period))
        assert rc == 0
        cells = G.Batch.unpack(out, side)
        for reach in (1, 2):
            most = max(most, len(I.census(cells, reach)[0]))
    assert 0 < most <= S["cap"], most
