"""Island kinds free of orientation without a GPU (include/golhip.h, "island kinds free of orientation"):
gol_island_orient_host (the function of csrc/gol_island.h the kernel runs) against numpy on the window as a small
array; the FREE host twin (gol_batch_islands_sym_host) against the reference of tests/island_sym_ref.py, which
turns and mirrors the board and never a code, on every board of island_ref.CASES; symmetry 0 through the _sym
entries against the entries without _sym, byte for byte; the invariance under the eight images of a board and of
named patterns; the tally and the census twin over free hashes; the refusals, the launch checks' new field, and
the stand-alone driver under AddressSanitizer + UndefinedBehaviorSanitizer (build/asan/island_sym_check, a plain
child process; nothing loaded into Python is sanitized).  All comparisons are exact."""
import ctypes
import itertools
import subprocess

import numpy as np
import pytest

import island_ref as I
import island_sym_ref as F
import rule_ref as R
import tally_ref as T
from tally_ref import DENSE, LISTED, ORDER, REFUSED
from testlib import GOL_EINVAL, check_program, cpu_lib  # noqa: F401 (the fixture)

FIXED, FREE = F.FIXED, F.FREE


@pytest.fixture(scope="module")
def G(cpu_lib):
    assert (cpu_lib.ISLAND_FIXED, cpu_lib.ISLAND_FREE) == (FIXED, FREE)
    return cpu_lib


# ------------------------------------------------------------------------------------------------------ orient
def code_array(code, reach):
    k = 2 * reach + 1
    return np.array([(code >> i) & 1 for i in range(k * k)], dtype=np.uint8).reshape(k, k)


def array_code(a):
    return sum(int(v) << i for i, v in enumerate(np.asarray(a).ravel()))


def orient_numpy(code, reach, s):
    """orient(code, reach, s) on the window as an array: the bit at (dy, dx) is the bit of the code at (+-a, +-b),
    (a, b) = (dx, dy) with t: F.image's flips, then its transpose."""
    return array_code(F.image(code_array(code, reach), s))


def codes_of(reach):
    if reach == 1:
        return list(range(512))
    few = [0] + [1 << i for i in range(25)] + [1 << i | 1 << j for i, j in itertools.combinations(range(25), 2)]
    rng = np.random.default_rng(25)
    return few + [int(v) for v in rng.integers(0, 1 << 25, 4096)]


@pytest.mark.parametrize("reach", [1, 2])
def test_orient_against_numpy(G, reach):
    orient = G.lib().gol_island_orient_host
    codes = codes_of(reach)
    assert len(codes) == (512 if reach == 1 else 1 + 25 + 300 + 4096)
    for s in range(8):
        got = [orient(c, reach, s) for c in codes]
        assert got == [orient_numpy(c, reach, s) for c in codes], s
        assert len(set(got)) == len(set(codes)), s  # a bijection on them
        if s == 0:
            assert got == codes
        if reach == 1:
            assert sorted(got) == codes  # all 512: a permutation
    # the definition, spelled out on one code: the bit at (dy, dx) is the bit of c at (dy', dx')
    c = codes[-1] if reach == 2 else 0b011010001
    k = 2 * reach + 1
    for s in range(8):
        t, fy, fx = s & 1, (s >> 1) & 1, (s >> 2) & 1
        want = 0
        for dy in range(-reach, reach + 1):
            for dx in range(-reach, reach + 1):
                a, b = (dx, dy) if t else (dy, dx)
                sy, sx = (-a if fy else a), (-b if fx else b)
                want |= ((c >> ((sy + reach) * k + sx + reach)) & 1) << ((dy + reach) * k + dx + reach)
        assert orient(c, reach, s) == want, s


@pytest.mark.parametrize("reach", [1, 2])
def test_orient_is_closed(G, reach):
    """orient(orient(c, a), b) is one of the eight orient(c, s): the eight maps are a group."""
    orient = G.lib().gol_island_orient_host
    rng = np.random.default_rng(8)
    k = 2 * reach + 1
    for c in [int(v) for v in rng.integers(0, 1 << (k * k), 40)]:
        eight = {orient(c, reach, s) for s in range(8)}
        for a in range(8):
            for b in range(8):
                assert orient(orient(c, reach, a), reach, b) in eight, (c, a, b)
    # a code without symmetry has eight different images
    c = 0b000100011 if reach == 1 else 0x103  # the cells (0, 0), (0, 1) and (1, 2), or (1, 3) of the 5 x 5 window
    assert len({orient(c, reach, s) for s in range(8)}) == 8


def test_orient_outside_its_domain(G):
    orient = G.lib().gol_island_orient_host
    assert [orient(0x1ff, 1, s) for s in (-1, 8, 100)] == [0, 0, 0]
    assert [orient(0x1ff, r, 1) for r in (0, 3, -1)] == [0, 0, 0]


# ---------------------------------------------------------------------------------------------- the host twin
def host_census(G, cells, reach, symmetry, cap=None, stride_pad=0, sym_entry=True):
    """(count, records[:min(count, cap)], fingerprint) of one board through gol_batch_islands_sym_host (or the entry
    without _sym); the rows `stride_pad` words apart more than they need, the gaps and the padding bits set."""
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
    tail = (words.ctypes.data, words.shape[1], cap, ctypes.byref(count), recs.ctypes.data if cap else None, ctypes.byref(fp))
    if sym_entry:
        rc = G.lib().gol_batch_islands_sym_host(H, W, reach, symmetry, *tail)
    else:
        rc = G.lib().gol_batch_islands_host(H, W, reach, *tail)
    assert rc == 0, G.lib().gol_last_error()
    return count.value, recs[:min(count.value, cap)], fp.value


def assert_same(got, want, where):
    count, recs, fp = got
    wrecs, wfp = want
    assert count == len(wrecs), (where, count, len(wrecs))
    assert fp == wfp, (where, hex(fp), hex(wfp))
    assert np.array_equal(recs, wrecs[:len(recs)]), (where, recs[:4], wrecs[:4])  # every field of every record


@pytest.mark.parametrize("c", I.CASES, ids=lambda c: c.id)
def test_free_host_twin_on_the_case_table(G, c):
    for reach in c.reaches:
        for i, (b, w) in enumerate(zip(c.cells, F.want(c, reach))):
            assert_same(host_census(G, b, reach, FREE, stride_pad=i % 2), w, (c.id, reach, i))
            # y, x, cells, rows, cols and the order are those of the fixed census
            fixed = I.want(c, reach)[i][0]
            for f in ("y", "x", "cells", "rows", "cols"):
                assert np.array_equal(w[0][f], fixed[f]), (c.id, reach, i, f)


def test_symmetry_0_is_the_entry_without_sym(G):
    rng = np.random.default_rng(31)
    for H, W in ((9, 9), (20, 70), (65, 33), (3, 130)):
        board = rng.random((H, W)) < 0.2
        for reach in (1, 2):
            for cap in (0, 3, None):
                a = host_census(G, board, reach, FIXED, cap=cap, stride_pad=1)
                b = host_census(G, board, reach, FIXED, cap=cap, stride_pad=1, sym_entry=False)
                assert a[0] == b[0] and a[2] == b[2] and a[1].tobytes() == b[1].tobytes(), (H, W, reach, cap)
            assert_same(host_census(G, board, reach, FIXED), I.census(board, reach), (H, W, reach))
    # the census twin
    c = T.SOUP_CASES[0]
    for reach in (1, 2):
        a, b = host_soup_census(G, c, reach, FIXED, 8, 64), host_soup_census(G, c, reach, None, 8, 64)
        for k in a:
            assert np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes(), (reach, k)
    # the two launch checks
    P = 0x1000
    L = G.lib()
    for reach, cap, isl in ((1, 8, P), (2, 0, None), (0, 8, P), (1, -1, P), (1, 8, None)):
        assert L.gol_batch_islands_sym_check_host(P, 3, 64, 64, reach, FIXED, cap, P, isl, P) == \
            L.gol_batch_islands_check_host(P, 3, 64, 64, reach, cap, P, isl, P)
    for log2, dropped in ((10, P), (3, P), (10, None)):
        assert L.gol_batch_islands_tally_sym_check_host(P, 3, 64, 64, 1, FIXED, None, None, 0, None, 0, P, P, P, log2, dropped) == \
            L.gol_batch_islands_tally_check_host(P, 3, 64, 64, 1, None, None, 0, None, 0, P, P, P, log2, dropped)


# -------------------------------------------------------------------------------------------------- invariance
@pytest.mark.parametrize("H,W,dens", [(65, 65, 0.1), (20, 70, 0.15)])
def test_free_hash_under_the_eight_images(G, H, W, dens):
    rng = np.random.default_rng(H * 1000 + W)
    board = rng.random((H, W)) < dens
    for reach in (1, 2):
        base = host_census(G, board, reach, FREE)
        fixed0 = host_census(G, board, reach, FIXED)
        fixed_differs = False
        for s in range(8):
            img = np.ascontiguousarray(F.image(board, s))
            assert img.shape == ((W, H) if s & 1 else (H, W))
            got = host_census(G, img, reach, FREE)
            assert got[0] == base[0] and got[2] == base[2], (reach, s)  # the count and the free fingerprint
            assert F.key(got[1]) == F.key(base[1]), (reach, s)  # the multiset of (cells, free hash)
            shape = lambda recs, a, b: sorted((int(r["cells"]), int(r[a]), int(r[b]), int(r["hash"])) for r in recs)
            if s & 1:  # rows and cols describe the island as it lies: swapped under a transposing image
                assert shape(got[1], "cols", "rows") == shape(base[1], "rows", "cols"), (reach, s)
            else:
                assert shape(got[1], "rows", "cols") == shape(base[1], "rows", "cols"), (reach, s)
            fixed = host_census(G, img, reach, FIXED)
            fixed_differs |= I.key(fixed[1]) != I.key(fixed0[1]) and fixed[2] != fixed0[2]
            # and the reference agrees on the image
            assert_same(got, F.census(img, reach), (reach, s))
        assert fixed_differs  # (or the test would have no power: the fixed hash does see the orientation)


BLOCK = "x = 2, y = 2\n2o$2o!"
BEEHIVE = "x = 4, y = 3\nb2o$o2bo$b2o!"
BOAT = "x = 3, y = 3\n2o$obo$bo!"
BLINKER = "x = 3, y = 1\n3o!"
GLIDER = "x = 3, y = 3\nbo$2bo$3o!"


def test_named_patterns(G):
    for reach in (1, 2):
        free = lambda p: int(G.island(p, reach, symmetry=FREE)["hash"])
        fixed = lambda p: int(G.island(p, reach)["hash"])
        # both blinker phases are one free kind, two fixed ones
        assert free(BLINKER) == free(np.ones((3, 1))) and fixed(BLINKER) != fixed(np.ones((3, 1)))
        for text, lines in ((BOAT, 4), (GLIDER, 8)):  # (a boat is its own mirror image across a diagonal)
            cells = G.parse_rle(text)[0]
            eight = [np.ascontiguousarray(F.image(cells, s)) for s in range(8)]
            assert len({free(p) for p in eight}) == 1, (text, reach)
            assert len({fixed(p) for p in eight}) == lines, (text, reach)  # so many lines of a fixed tally
            assert free(cells) == F.lone(cells, reach) == min(fixed(p) for p in eight)
        assert len({free(BLOCK), free(BEEHIVE), free(BOAT)}) == 3
        assert len({fixed(p) for p in (BEEHIVE, np.ascontiguousarray(G.parse_rle(BEEHIVE)[0].T))}) == 2
        assert free(BLOCK) == fixed(BLOCK)  # every image of a block is a block
        r = G.island(BOAT, reach, symmetry=FREE)
        assert (int(r["cells"]), int(r["rows"]), int(r["cols"])) == (5, 3, 3)
    with pytest.raises(G.GolError) as e:
        G.island(BLOCK, 1, symmetry=2)
    assert e.value.code == GOL_EINVAL


# ------------------------------------------------------------------------------------- the tally and the census
def host_tally(G, pairs):
    pairs = list(pairs)
    recs = np.array([r for _, r in pairs], dtype=I.DTYPE) if pairs else np.zeros(0, dtype=I.DTYPE)
    owners = np.array([o for o, _ in pairs], dtype=np.int64)
    kinds = np.zeros(max(len(pairs), 1), dtype=T.KIND_DTYPE)
    n = ctypes.c_int64(-7)
    rc = G.lib().gol_island_tally_host(recs.ctypes.data, owners.ctypes.data, len(pairs), kinds.ctypes.data, len(kinds), ctypes.byref(n))
    assert rc == 0, G.lib().gol_last_error()
    return kinds[:n.value]


def host_soup_census(G, c, reach, symmetry, slots, launch, cap=4096):
    """gol_batch_census_sym_host (symmetry None: gol_batch_census_host) as the dict Batch.census returns."""
    b, s = R.masks(T.RULE)
    out = [np.zeros(c.total, dtype=t) for t in (np.int64, np.int64, np.uint64, np.uint64, np.int64, np.uint64)]
    kinds = np.zeros(cap, dtype=T.KIND_DTYPE)
    n = ctypes.c_int64(-7)
    tail = [*[a.ctypes.data for a in out], kinds.ctypes.data, cap, ctypes.byref(n)]
    if symmetry is None:
        rc = G.lib().gol_batch_census_host(c.H, c.W, b, s, T.SEED, 0, c.total, slots, launch, c.horizon, reach, *tail)
    else:
        rc = G.lib().gol_batch_census_sym_host(c.H, c.W, b, s, T.SEED, 0, c.total, slots, launch, c.horizon, reach, symmetry, *tail)
    assert rc == 0, G.lib().gol_last_error()
    return dict(zip(("found", "period", "alive", "hash", "islands", "fingerprint"), out), kinds=kinds[:min(n.value, cap)],
                n_kinds=n.value)


def test_tally_over_free_records(G):
    cells = F.boards_case()
    for reach in (1, 2):
        pairs = []
        for i, b in enumerate(cells):
            count, recs, _ = host_census(G, b, reach, FREE)
            pairs += [(50 + i, r) for r in recs]
        counts, fps, kinds = F.of_boards(cells, reach, owner0=50)
        assert len(pairs) == int(counts.sum())
        assert np.array_equal(host_tally(G, pairs), kinds), reach
        # the free tally merges lines of the fixed one, and keeps every island
        fixed = T.of_boards(cells, reach)[2]
        assert len(kinds) < len(fixed) and int(kinds["count"].sum()) == int(fixed["count"].sum())


@pytest.mark.parametrize("c", T.SOUP_CASES, ids=lambda c: c.id)
def test_free_census_twin(G, c):
    for reach in (1, 2):
        want = F.soup_census(c, reach)
        for slots, launch in ((17, 7), (8, 64)):
            got = host_soup_census(G, c, reach, FREE, slots, launch)
            for k, w in want.items():
                assert np.array_equal(got[k], w), (c.id, reach, k)
        fixed = T.census(c, reach)
        assert want["n_kinds"] < fixed["n_kinds"] and int(want["kinds"]["count"].sum()) == int(fixed["kinds"]["count"].sum())


# ---------------------------------------------------------------------------------------------------- refusals
def test_refusals_write_nothing(G):
    L = G.lib()
    words = np.zeros(8, dtype=np.uint64)
    count, fp, nk = ctypes.c_int64(77), ctypes.c_uint64(77), ctypes.c_int64(77)
    recs = np.frombuffer(b"\xa5" * 24, dtype=I.DTYPE).copy()
    for reach, sym in ((1, 2), (1, -1), (2, 7), (0, FREE), (3, FREE)):
        rc = L.gol_batch_islands_sym_host(8, 8, reach, sym, words.ctypes.data, 1, 1, ctypes.byref(count), recs.ctypes.data, ctypes.byref(fp))
        assert rc == GOL_EINVAL, (reach, sym)
    assert L.gol_batch_islands_sym_host(8, 8, 1, FREE, None, 1, 1, ctypes.byref(count), recs.ctypes.data, ctypes.byref(fp)) == GOL_EINVAL
    assert L.gol_batch_islands_sym_host(8, 65, 1, FREE, words.ctypes.data, 1, 1, ctypes.byref(count), recs.ctypes.data, ctypes.byref(fp)) == GOL_EINVAL
    out = np.full(4, 77, dtype=np.int64)
    kinds = np.zeros(4, dtype=T.KIND_DTYPE)
    p = out.ctypes.data
    for reach, sym in ((1, 2), (1, -1), (0, FREE)):
        rc = L.gol_batch_census_sym_host(8, 8, 8, 12, 1, 0, 4, 2, 4, 10, reach, sym, p, None, None, None, None, None, kinds.ctypes.data, 4,
                                         ctypes.byref(nk))
        assert rc == GOL_EINVAL, (reach, sym)
    assert (count.value, fp.value, nk.value) == (77, 77, 77) and recs.tobytes() == b"\xa5" * 24
    assert np.all(out == 77) and not kinds.tobytes().strip(b"\0")


def test_launch_checks_take_the_symmetry(G):
    """gol_island_launch_ok's new field, through the two exports: 0 and 1 pass, everything else is refused, and the
    other refusals are those of the entries without _sym."""
    L = G.lib()
    P = 0x1000
    good = dict(boards=P, n=3, H=64, W=64, reach=1, symmetry=FREE, cap=8, count=P, islands=P, fingerprint=P)
    order = ("boards", "n", "H", "W", "reach", "symmetry", "cap", "count", "islands", "fingerprint")
    plain = lambda **over: L.gol_batch_islands_sym_check_host(*[dict(good, **over)[k] for k in order])
    assert plain() == 0 and plain(symmetry=FIXED) == 0 and plain(reach=2, fingerprint=None) == 0 and plain(cap=0, islands=None) == 0
    for bad in (dict(symmetry=2), dict(symmetry=-1), dict(symmetry=8), dict(symmetry=1 << 30), dict(boards=None), dict(count=None),
                dict(islands=None), dict(n=0), dict(H=513), dict(W=0), dict(reach=0), dict(reach=3), dict(cap=-1)):
        assert plain(**bad) == GOL_EINVAL, bad
    sym_order = ORDER[:5] + ("symmetry",) + ORDER[5:]
    tally = lambda base, **over: L.gol_batch_islands_tally_sym_check_host(*[dict(dict(base, symmetry=FREE), **over)[k] for k in sym_order])
    assert tally(DENSE) == 0 and tally(LISTED) == 0 and tally(DENSE, symmetry=FIXED) == 0 and tally(LISTED, reach=2) == 0
    for base in (DENSE, LISTED):
        for sym in (2, -1, 8):
            assert tally(base, symmetry=sym) == GOL_EINVAL, sym
    for base, bad in REFUSED:
        assert tally(base, **bad) == GOL_EINVAL, bad


def test_island_sym_check_under_sanitizers():
    """The FREE twins in the stand-alone program, the board and the records heap blocks of their exact sizes,
    against a cell-by-cell flood fill that reads every orientation's code off the board."""
    r = subprocess.run([check_program("island_sym_check")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "0 bad" in r.stdout
