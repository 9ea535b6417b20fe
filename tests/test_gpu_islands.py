"""The island census on the GPU: every instantiation of batch_islands_kernel<NW, REACH> (csrc/gol_island.hip) on
caller memory through gol_dev_batch_islands, against the reference of tests/island_ref.py (a plain-Python flood
fill written from include/golhip.h), every compared field bit for bit.  The case table is island_ref's (its
coverage is asserted in tests/test_island_ref_cpu.py).  Every buffer of a launch lies between two margins of
sentinel bytes; the records are filled with 0xA5 before the launch, so a record written past min(count, cap)
shows; the boards are compared byte for byte after the call.  Then the same census through golhip.Batch: on
settled soups against the reference, under random torus translations, and of named patterns."""
import ctypes

import numpy as np
import pytest

import island_ref as I
from testlib import GOL_EINVAL, Guarded, gpu_lib as G  # noqa: F401 (the fixture)

pytestmark = pytest.mark.gpu

FILL = 0xA5


def _launch(G, cells, reach, cap, with_fp=True):
    """One launch on caller memory; returns (rc, count, records[n, cap], fingerprint) after checking that the
    boards and every margin are as before."""
    import torch
    n, H, W = cells.shape
    words = G.Batch.pack(cells.astype(np.uint8))
    boards = Guarded(words, name="boards")
    count = Guarded(np.full(n * 8, FILL, dtype=np.uint8), name="count")
    recs = Guarded(np.full(n * cap * 24, FILL, dtype=np.uint8), fill=FILL, name="islands")
    fp = Guarded(np.full(n * 8, FILL, dtype=np.uint8), name="fingerprint")
    rc = G.lib().gol_dev_batch_islands(boards.ptr, n, H, W, reach, cap, count.ptr, recs.ptr if cap else None,
                                       fp.ptr if with_fp else None, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert boards.unchanged(), "the boards or their margins changed"
    return rc, count.read(np.int64), recs.read(I.DTYPE, (n, cap)), fp.read(np.uint64)


def _check_case(G, c, reach):
    want = I.want(c, reach)
    rc, count, recs, fp = _launch(G, c.cells, reach, c.cap)
    assert rc == 0, (c.id, G.lib().gol_last_error())
    untouched = np.frombuffer(bytes([FILL]) * 24, dtype=I.DTYPE)[0]
    for i, (wrecs, wfp) in enumerate(want):
        where = (c.id, reach, i)
        assert int(count[i]) == len(wrecs), (where, int(count[i]), len(wrecs))
        assert int(fp[i]) == wfp, (where, hex(int(fp[i])), hex(wfp))
        k = min(len(wrecs), c.cap)
        assert np.array_equal(recs[i, :k], wrecs[:k]), (where, recs[i, :3], wrecs[:3])
        assert np.all(recs[i, k:] == untouched), (where, "a record past min(count, cap) was written")


@pytest.mark.parametrize("c", I.CASES, ids=lambda c: c.id)
def test_case(G, c):
    for reach in c.reaches:
        _check_case(G, c, reach)


def test_null_fingerprint(G):
    c = next(c for c in I.CASES if c.id == "five-cap20")
    rc, count, recs, fp = _launch(G, c.cells, 1, c.cap, with_fp=False)
    assert rc == 0 and count.tolist() == [0, 1, 4, 9, 2]
    assert fp.tobytes() == bytes([FILL]) * fp.nbytes


def test_refusals_launch_nothing(G):
    import torch
    c = next(c for c in I.CASES if c.id == "five-cap3")
    n, H, W = c.cells.shape
    words = G.Batch.pack(c.cells.astype(np.uint8))
    boards, count = Guarded(words, name="boards"), Guarded(np.full(n * 8, FILL, dtype=np.uint8), name="count")
    recs = Guarded(np.full(n * 3 * 24, FILL, dtype=np.uint8), name="islands")
    pb, pc, pr = boards.ptr, count.ptr, recs.ptr
    s = torch.cuda.current_stream().cuda_stream
    f = G.lib().gol_dev_batch_islands
    bad = [f(None, n, H, W, 1, 3, pc, pr, None, s), f(pb, n, H, W, 1, 3, None, pr, None, s), f(pb, n, H, W, 1, 3, pc, None, None, s),
           f(pb, 0, H, W, 1, 3, pc, pr, None, s), f(pb, n, 0, W, 1, 3, pc, pr, None, s), f(pb, n, H, 513, 1, 3, pc, pr, None, s),
           f(pb, n, H, W, 0, 3, pc, pr, None, s), f(pb, n, H, W, 3, 3, pc, pr, None, s), f(pb, n, H, W, 1, -1, pc, pr, None, s)]
    torch.cuda.synchronize()
    assert bad == [GOL_EINVAL] * len(bad)
    assert count.unchanged() and recs.unchanged()


# ------------------------------------------------------------------------------------------------ through Batch
@pytest.fixture(scope="module")
def soups(G):
    """The settled soups: (cells uint8[n, side, side], reference per reach), made once."""
    S = I.SOUPS
    with G.Batch(S["n"], S["side"], S["side"], device=0) as b:
        b.load_soups(S["seed"])
        b.run_cycles(S["turns"])
        cells = b.store()
        got = {reach: b.islands(reach=reach, cap=S["cap"], fingerprints=True) for reach in (1, 2)}
        assert np.array_equal(b.store(), cells) and b.turn == S["turns"]
    want = {reach: [I.census(c, reach) for c in cells] for reach in (1, 2)}
    return cells, got, want


def test_batch_islands_on_settled_soups(G, soups):
    cells, got, want = soups
    assert cells.any()
    for reach in (1, 2):
        counts, recs, fps = got[reach]
        assert recs.dtype == G.ISLAND_DTYPE and recs.shape == (len(cells), I.SOUPS["cap"])
        for i, (wrecs, wfp) in enumerate(want[reach]):
            k = len(wrecs)
            assert int(counts[i]) == k <= I.SOUPS["cap"] and int(fps[i]) == wfp, (reach, i)
            assert np.array_equal(recs[i, :k], wrecs), (reach, i)
            assert not recs[i, k:].tobytes().strip(b"\0"), (reach, i)  # zero-initialised


def test_batch_islands_under_translation(G, soups):
    cells, got, _ = soups
    rng = np.random.default_rng(9)
    rolled = np.stack([np.roll(c, tuple(int(v) for v in rng.integers(0, c.shape)), axis=(0, 1)) for c in cells])
    with G.Batch(len(cells), cells.shape[1], cells.shape[2], device=0) as b:
        b.load(rolled)
        for reach in (1, 2):
            counts, recs, fps = b.islands(reach=reach, cap=I.SOUPS["cap"], fingerprints=True)
            c0, r0, f0 = got[reach]
            assert np.array_equal(counts, c0) and np.array_equal(fps, f0)
            for i in range(len(cells)):
                assert I.key(recs[i, :counts[i]]) == I.key(r0[i, :c0[i]]), (reach, i)


def test_batch_islands_ranges_and_refusals(G, soups):
    cells, got, _ = soups
    with G.Batch(len(cells), cells.shape[1], cells.shape[2], device=0) as b:
        b.load(cells)
        counts, recs = b.islands(reach=1, cap=5, first=7, count=3)
        assert np.array_equal(counts, got[1][0][7:10]) and np.array_equal(recs, got[1][1][7:10, :5])
        counts, recs = b.islands(cap=0)
        assert np.array_equal(counts, got[1][0]) and recs.shape == (len(cells), 0)
        for bad in (dict(reach=0), dict(reach=3), dict(cap=-1), dict(first=-1), dict(first=1, count=len(cells))):
            with pytest.raises(G.GolError):
                b.islands(**bad)
        out = ctypes.c_int64(77)
        assert G.lib().gol_batch_islands(b._h, 0, 1, 1, 4, ctypes.byref(out), None, None) == GOL_EINVAL and out.value == 77
        assert G.lib().gol_batch_islands(None, 0, 1, 1, 0, ctypes.byref(out), None, None) == GOL_EINVAL


def test_named_patterns_are_found_again(G):
    """A board holding a block, a blinker and a beehive: each is found under the record golhip.island gives it."""
    pats = {"block": "x = 2, y = 2\n2o$2o!", "blinker": "x = 3, y = 1\n3o!", "beehive": "x = 4, y = 3\nb2o$o2bo$b2o!"}
    board = np.zeros((1, 40, 70), dtype=np.uint8)
    for (y, x), text in zip(((38, 68), (10, 30), (20, 62)), pats.values()):  # the block over the corner, the beehive over bit 63|64
        p = G.parse_rle(text)[0]
        for dy, dx in np.argwhere(p):
            board[0, (y + dy) % 40, (x + dx) % 70] = 1
    with G.Batch(1, 40, 70, device=0) as b:
        b.load(board)
        for reach in (1, 2):
            counts, recs = b.islands(reach=reach)
            assert counts.tolist() == [3]
            names = {(int(r["cells"]), int(r["rows"]), int(r["cols"]), int(r["hash"])): k
                     for k, r in ((k, G.island(t, reach)) for k, t in pats.items())}
            assert sorted(names[k] for k in I.key(recs[0, :3])) == ["beehive", "blinker", "block"]


# --------------------------------------------------------------------------------- more than one scratch chunk
CHUNK_N, CHUNK_SIDE, CHUNK_FIRST = 44, 512, 1
CHUNK_PATTERNS = ("x = 3, y = 3\nbo$2bo$3o!", "x = 2, y = 2\n2o$2o!", "x = 4, y = 3\nb2o$o2bo$b2o!", "x = 3, y = 3\n2o$obo$bo!",
                  "x = 3, y = 3\nbo$2bo$3o!")  # glider, block, beehive, boat, glider


def _chunk_boards(G):
    """Board i: 1 + i % 5 objects, CHUNK_PATTERNS[k] at a place that depends on i.  Object 0, a glider, lies in rows
    63 to 65 (the lanes of two waves); object 1, a block, in rows 511 and 0, for i % 3 == 0 in columns 511 and 0 too."""
    side = CHUNK_SIDE
    pats = [G.parse_rle(t)[0] for t in CHUNK_PATTERNS]
    cells = np.zeros((CHUNK_N, side, side), dtype=np.uint8)
    for i in range(CHUNK_N):
        places = ((63, 5 + 11 * i), (side - 1, side - 1 if i % 3 == 0 else 40 + 7 * i), (150 + i, 300 - 5 * i),
                  (260 + 2 * i, 17 + 9 * i), (400 - i, 100 + 3 * i))
        for k in range(1 + i % 5):
            for dy, dx in np.argwhere(pats[k]):
                cells[i, (places[k][0] + dy) % side, (places[k][1] + dx) % side] = 1
    return cells


def _host_twin(G, words, reach, symmetry, cap=16):
    """(count, records, fingerprint) of one board of CHUNK_SIDE from the host twin, symmetry 0 through the entry without _sym."""
    count, fp = ctypes.c_int64(-7), ctypes.c_uint64(7)
    recs = np.zeros(cap, dtype=I.DTYPE)
    tail = (words.ctypes.data, words.shape[1], cap, ctypes.byref(count), recs.ctypes.data, ctypes.byref(fp))
    if symmetry == 0:
        rc = G.lib().gol_batch_islands_host(CHUNK_SIDE, CHUNK_SIDE, reach, *tail)
    else:
        rc = G.lib().gol_batch_islands_sym_host(CHUNK_SIDE, CHUNK_SIDE, reach, symmetry, *tail)
    assert rc == 0 and 0 <= count.value <= cap, G.lib().gol_last_error()
    return count.value, recs[:count.value], fp.value


def test_batch_islands_across_scratch_chunks(G):
    """gol_batch_islands over more boards than one chunk of its device scratch holds (GOL_ISLAND_SCRATCH_BYTES,
    csrc/gol_batch_census.cpp): boards [1, 44) of 44 boards of 512 x 512 with cap = H W are a chunk of 42 boards and a
    chunk of one, so the second trip of the chunk loop, its offsets into the caller's arrays and its own strided
    copy of the records run.  Every board against the host twins (pinned to the Python references on the CPU), the
    three boards at the chunk boundary against the Python references themselves."""
    import island_sym_ref as Y
    side, first, count = CHUNK_SIDE, CHUNK_FIRST, CHUNK_N - CHUNK_FIRST
    cap = side * side
    each = 16 + 24 * cap  # bytes of a board's scratch: its count, its fingerprint, cap records
    per = (256 << 20) // each
    assert (each, per) == (6291472, 42) and count > per, "the call must take more than one chunk"
    cells = _chunk_boards(G)
    words = G.Batch.pack(cells)
    assert len({w.tobytes() for w in words}) == CHUNK_N
    with G.Batch(CHUNK_N, side, side, device=0) as b:
        b.load(cells)
        for reach, symmetry, ref in ((1, G.ISLAND_FIXED, I), (2, G.ISLAND_FREE, Y)):
            counts, recs, fps = b.islands(reach=reach, cap=cap, first=first, count=count, fingerprints=True, symmetry=symmetry)
            assert recs.shape == (count, cap)
            for j in range(count):  # (never the whole of recs: its pages past the records are untouched)
                i = first + j
                where = (reach, symmetry, i)
                wcount, wrecs, wfp = _host_twin(G, words[i], reach, symmetry)
                assert 1 <= wcount <= 1 + i % 5, where
                assert int(counts[j]) == wcount and int(fps[j]) == wfp, (where, int(counts[j]), wcount)
                assert np.array_equal(recs[j, :wcount], wrecs), (where, recs[j, :wcount], wrecs)
                assert not recs[j, wcount:wcount + 8].tobytes().strip(b"\0"), (where, "a record past count was written")
                if i >= first + per - 2:  # boards 41 and 42, the first chunk's last, and 43, the second chunk's only one
                    prec, pfp = ref.census(cells[i], reach)
                    assert wcount == len(prec) and wfp == pfp and np.array_equal(wrecs, prec), where
        assert np.array_equal(b.store_words(), words)
