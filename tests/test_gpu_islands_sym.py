"""Island kinds free of orientation on the GPU: every FREE instantiation of batch_islands_kernel<NW, REACH, TALLY,
FREE> (csrc/gol_island.hip) on caller memory through gol_dev_batch_islands_sym and gol_dev_batch_islands_tally_sym,
against the reference of tests/island_sym_ref.py (which turns and mirrors the board with numpy and never a window
code), every compared field bit for bit.  The harness is that of tests/test_gpu_islands.py and
tests/test_gpu_tally.py (testlib.Guarded, tally_ref.Launch): every buffer of a launch lies between two margins of sentinel bytes, the records are
filled with 0xA5 before the launch, and the boards are compared byte for byte after the call.  Then the same
through golhip.Batch: the census of a soup search, the eight images of a batch of boards, a batch against its
transpose, and named patterns."""
import ctypes

import numpy as np
import pytest

import island_ref as I
import island_sym_ref as F
import tally_ref as T
from tally_ref import Launch
from testlib import GOL_EINVAL, Guarded, gpu_lib

pytestmark = pytest.mark.gpu

FILL = 0xA5
FIXED, FREE = F.FIXED, F.FREE


@pytest.fixture(scope="module")
def G(gpu_lib):
    assert (gpu_lib.ISLAND_FIXED, gpu_lib.ISLAND_FREE) == (FIXED, FREE)
    return gpu_lib


def _launch(G, cells, reach, symmetry, cap, with_fp=True, sym_entry=True):
    """One launch on caller memory; returns (rc, count, records[n, cap], fingerprint) after checking that the
    boards and every margin are as before."""
    import torch
    n, H, W = cells.shape
    words = G.Batch.pack(cells.astype(np.uint8))
    boards = Guarded(words, name="boards")
    count = Guarded(np.full(n * 8, FILL, dtype=np.uint8), name="count")
    recs = Guarded(np.full(n * cap * 24, FILL, dtype=np.uint8), fill=FILL, name="islands")
    fp = Guarded(np.full(n * 8, FILL, dtype=np.uint8), name="fingerprint")
    tail = (cap, count.ptr, recs.ptr if cap else None, fp.ptr if with_fp else None, torch.cuda.current_stream().cuda_stream)
    if sym_entry:
        rc = G.lib().gol_dev_batch_islands_sym(boards.ptr, n, H, W, reach, symmetry, *tail)
    else:
        rc = G.lib().gol_dev_batch_islands(boards.ptr, n, H, W, reach, *tail)
    torch.cuda.synchronize()
    assert boards.unchanged(), "the boards or their margins changed"
    return rc, count.read(np.int64), recs.read(I.DTYPE, (n, cap)), fp.read(np.uint64)


@pytest.mark.parametrize("c", I.CASES, ids=lambda c: c.id)
def test_case(G, c):
    untouched = np.frombuffer(bytes([FILL]) * 24, dtype=I.DTYPE)[0]
    for reach in c.reaches:
        want = F.want(c, reach)
        rc, count, recs, fp = _launch(G, c.cells, reach, FREE, c.cap)
        assert rc == 0, (c.id, G.lib().gol_last_error())
        for i, (wrecs, wfp) in enumerate(want):
            where = (c.id, reach, i)
            assert int(count[i]) == len(wrecs), (where, int(count[i]), len(wrecs))
            assert int(fp[i]) == wfp, (where, hex(int(fp[i])), hex(wfp))
            k = min(len(wrecs), c.cap)
            assert np.array_equal(recs[i, :k], wrecs[:k]), (where, recs[i, :3], wrecs[:3])
            assert np.all(recs[i, k:] == untouched), (where, "a record past min(count, cap) was written")


@pytest.mark.parametrize("id", ["shape-65x255", "narrow-3x2", "serpentine-65"])
def test_symmetry_0_is_the_entry_without_sym(G, id):
    c = next(c for c in I.CASES if c.id == id)
    for reach in c.reaches:
        a = _launch(G, c.cells, reach, FIXED, c.cap)
        b = _launch(G, c.cells, reach, None, c.cap, sym_entry=False)
        assert a[0] == b[0] == 0
        for x, y in zip(a[1:], b[1:]):
            assert x.tobytes() == y.tobytes(), (id, reach)
        for i, (wrecs, wfp) in enumerate(I.want(c, reach)):
            assert int(a[1][i]) == len(wrecs) and int(a[3][i]) == wfp, (id, reach, i)


def test_null_fingerprint(G):
    c = next(c for c in I.CASES if c.id == "five-cap20")
    rc, count, recs, fp = _launch(G, c.cells, 1, FREE, c.cap, with_fp=False)
    assert rc == 0 and count.tolist() == [0, 1, 4, 9, 2]
    assert fp.tobytes() == bytes([FILL]) * fp.nbytes


# ------------------------------------------------------------------------------------------------ the TALLY form
class SymLaunch(Launch):
    def run(self, reach, symmetry, owner0=0):
        import torch
        rc = self.G.lib().gol_dev_batch_islands_tally_sym(
            self.boards.ptr, self.n, self.H, self.W, reach, symmetry, None, None, 0, None, owner0, self.count.ptr, self.fp.ptr,
            self.table.ptr, self.log2, self.dropped.ptr, torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        return rc


def _dense(G, cells, owner0=0):
    for reach in (1, 2):
        counts, fps, kinds = F.of_boards(cells, reach, owner0=owner0)
        L = SymLaunch(G, cells, max(4, int(np.ceil(np.log2(2 * max(len(kinds), 1))))))
        assert L.run(reach, FREE, owner0=owner0) == 0, G.lib().gol_last_error()
        got = L.results()
        assert np.array_equal(got[0], counts) and np.array_equal(got[1], fps), reach
        assert got[3] == 0 and np.array_equal(got[2], kinds), (reach, got[2][:3], kinds[:3])
    return kinds


def test_tally_dense_boards_case(G):
    cells = F.boards_case()
    kinds = _dense(G, cells, owner0=1000)
    assert len(kinds) < len(T.of_boards(cells, 2)[2])  # lines of the fixed tally merged


def test_tally_dense_distinct_islands(G):
    _dense(G, F.distinct_islands(1200))


def test_tally_dense_flushes_mid_board(G):
    """More than GOL_ISLAND_TALLY_BUFFER = 64 islands on a board: the buffer of gathered free hashes is inserted while
    the board is still being labelled (lattice-3 has 462 islands at reach 1 and 2)."""
    c = next(c for c in I.CASES if c.id == "lattice-3")
    assert len(I.want(c, 1)[0][0]) > 64
    _dense(G, c.cells)


@pytest.mark.parametrize("c", T.SOUP_CASES, ids=lambda c: c.id)
def test_census(G, c):
    for reach in (1, 2):
        want = F.soup_census(c, reach)
        for slots, tpl in ((8, 1), (17, 7)):
            with G.Batch(slots, c.H, c.W, rule=T.RULE, device=0, turns_per_launch=tpl) as b:
                got = b.census(T.SEED, c.total, c.horizon, reach=reach, symmetry=FREE)
                for k, w in want.items():
                    assert np.array_equal(got[k], w), (c.id, reach, slots, k, got[k][:4], w[:4])
                assert got["kinds"].dtype == G.ISLAND_KIND_DTYPE
                assert not b.store_words().any() and b.turn == 0  # as after search
                # found, period, alive and hash are those of search on the same build
                found, period, alive, hashes = b.search(T.SEED, c.total, c.horizon)
                for k, a in zip(("found", "period", "alive", "hash"), (found, period, alive, hashes)):
                    assert np.array_equal(got[k], a), (c.id, k)


# --------------------------------------------------------------------------------------- invariance through Batch
def _free(b, reach, cap):
    counts, recs, fps = b.islands(reach=reach, cap=cap, fingerprints=True, symmetry=FREE)
    assert counts.max() <= cap
    return counts, recs, fps


def test_batch_eight_images_in_one_batch(G):
    rng = np.random.default_rng(65)
    boards = rng.random((16, 65, 65)) < 0.08
    images = np.stack([np.ascontiguousarray(F.image(bd, s)) for bd in boards for s in range(8)]).astype(np.uint8)
    with G.Batch(len(images), 65, 65, device=0) as b:
        b.load(images)
        for reach in (1, 2):
            counts, recs, fps = _free(b, reach, 512)  # (the boards hold up to 265 islands)
            fc, frecs, ffps = b.islands(reach=reach, cap=512, fingerprints=True)
            tc, tfps, kinds = b.islands_tally(reach=reach, symmetry=FREE)
            assert np.array_equal(tc, counts) and np.array_equal(tfps, fps) and np.array_equal(fc, counts)
            differs = False
            for i in range(16):
                wrecs, wfp = F.census(boards[i], reach)
                for s in range(8):
                    j = 8 * i + s
                    assert int(counts[j]) == len(wrecs) and int(fps[j]) == wfp, (reach, i, s)
                    assert F.key(recs[j, :counts[j]]) == F.key(wrecs), (reach, i, s)
                    differs |= int(ffps[j]) != int(ffps[8 * i])
                assert np.array_equal(recs[8 * i, :counts[8 * i]], wrecs)  # image 0 is the board
            assert differs  # the fixed fingerprint does see the orientation
            # every kind's count is a multiple of 8: an island and its seven images are one kind
            assert np.all(kinds["count"] % 8 == 0) and int(kinds["count"].sum()) == int(counts.sum())
        assert np.array_equal(b.store(), images * 255)


def test_batch_against_its_transpose(G):
    rng = np.random.default_rng(2070)
    boards = (rng.random((12, 20, 70)) < 0.15).astype(np.uint8)
    turned = np.ascontiguousarray(boards.transpose(0, 2, 1))
    with G.Batch(12, 20, 70, device=0) as b, G.Batch(12, 70, 20, device=0) as t:
        b.load(boards)
        t.load(turned)
        for reach in (1, 2):
            c0, r0, f0 = _free(b, reach, 256)
            c1, r1, f1 = _free(t, reach, 256)
            assert np.array_equal(c0, c1) and np.array_equal(f0, f1), reach
            for i in range(12):
                a = sorted((int(r["cells"]), int(r["rows"]), int(r["cols"]), int(r["hash"])) for r in r0[i, :c0[i]])
                d = sorted((int(r["cells"]), int(r["cols"]), int(r["rows"]), int(r["hash"])) for r in r1[i, :c1[i]])
                assert a == d, (reach, i)  # rows and cols swapped
                assert int(f0[i]) == F.census(boards[i], reach)[1]
            k0, k1 = b.islands_tally(reach=reach, symmetry=FREE)[2], t.islands_tally(reach=reach, symmetry=FREE)[2]
            for f in ("hash", "count", "first", "cells"):
                assert np.array_equal(k0[f], k1[f]), (reach, f)
            assert not np.array_equal(b.islands(reach=reach, cap=0, fingerprints=True)[2], t.islands(reach=reach, cap=0, fingerprints=True)[2])


def test_named_patterns(G):
    """A board holding a blinker in both phases, a boat in its four and a glider phase in its eight orientations, a
    block and a beehive: the free tally has one line for each object, under the free hash golhip.island gives it."""
    pats = {"block": "x = 2, y = 2\n2o$2o!", "blinker": "x = 3, y = 1\n3o!", "beehive": "x = 4, y = 3\nb2o$o2bo$b2o!",
            "boat": "x = 3, y = 3\n2o$obo$bo!", "glider": "x = 3, y = 3\nbo$2bo$3o!"}
    cells = {k: G.parse_rle(t)[0] for k, t in pats.items()}
    placed = [("block", 0), ("beehive", 0), ("beehive", 1), ("blinker", 0), ("blinker", 1)]
    placed += [("boat", s) for s in range(8)] + [("glider", s) for s in range(8)]
    board = np.zeros((1, 64, 70), dtype=np.uint8)
    for i, (name, s) in enumerate(placed):
        p = F.image(cells[name], s)
        y, x = 8 * (i // 8) + 60, 8 * (i % 8) + 60  # from the corner on: some lie over the seams and over bit 63|64
        for dy, dx in np.argwhere(p):
            board[0, (y + dy) % 64, (x + dx) % 70] = 1
    with G.Batch(1, 64, 70, device=0) as b:
        b.load(board)
        for reach in (1, 2):
            counts, fps, kinds = b.islands_tally(reach=reach, symmetry=FREE)
            assert counts.tolist() == [len(placed)]
            want = {int(G.island(t, reach, symmetry=FREE)["hash"]): k for k, t in pats.items()}
            assert len(want) == 5
            got = {want[int(k["hash"])]: int(k["count"]) for k in kinds}
            assert got == {"block": 1, "beehive": 2, "blinker": 2, "boat": 8, "glider": 8}, (reach, got)
            fixed = b.islands_tally(reach=reach)[2]
            assert len(fixed) == 1 + 2 + 2 + 4 + 8  # one line per orientation that differs


# ---------------------------------------------------------------------------------------------------- refusals
def test_refusals_launch_nothing(G):
    import torch
    c = next(c for c in I.CASES if c.id == "five-cap3")
    n, H, W = c.cells.shape
    words = G.Batch.pack(c.cells.astype(np.uint8))
    boards, count = Guarded(words, name="boards"), Guarded(np.full(n * 8, FILL, dtype=np.uint8), name="count")
    recs = Guarded(np.full(n * 3 * 24, FILL, dtype=np.uint8), name="islands")
    pb, pc, pr = boards.ptr, count.ptr, recs.ptr
    s = torch.cuda.current_stream().cuda_stream
    f = G.lib().gol_dev_batch_islands_sym
    bad = [f(pb, n, H, W, 1, 2, 3, pc, pr, None, s), f(pb, n, H, W, 1, -1, 3, pc, pr, None, s), f(pb, n, H, W, 2, 8, 3, pc, pr, None, s),
           f(None, n, H, W, 1, FREE, 3, pc, pr, None, s), f(pb, n, H, W, 1, FREE, 3, None, pr, None, s),
           f(pb, n, H, W, 1, FREE, 3, pc, None, None, s), f(pb, 0, H, W, 1, FREE, 3, pc, pr, None, s),
           f(pb, n, H, 513, 1, FREE, 3, pc, pr, None, s), f(pb, n, H, W, 0, FREE, 3, pc, pr, None, s),
           f(pb, n, H, W, 3, FREE, 3, pc, pr, None, s), f(pb, n, H, W, 1, FREE, -1, pc, pr, None, s)]
    L = SymLaunch(G, c.cells, 10)
    bad += [L.run(1, 2), L.run(1, -1), L.run(0, FREE), L.run(3, FREE), L.run(1, FREE, owner0=-1)]
    torch.cuda.synchronize()
    assert bad == [GOL_EINVAL] * len(bad)
    assert count.unchanged() and recs.unchanged()
    for buf in (L.count, L.fp, L.table, L.dropped, L.boards):
        assert buf.unchanged()
    # and through Batch, before any GPU work
    with G.Batch(n, H, W, device=0) as b:
        b.load(c.cells.astype(np.uint8))
        for call in (lambda: b.islands(symmetry=2), lambda: b.islands_tally(symmetry=-1), lambda: b.census(1, 4, 10, symmetry=2)):
            with pytest.raises(G.GolError) as e:
                call()
            assert e.value.code == GOL_EINVAL
        out, nk = ctypes.c_int64(77), ctypes.c_int64(77)
        assert G.lib().gol_batch_islands_sym(b._h, 0, 1, 1, 2, 0, ctypes.byref(out), None, None) == GOL_EINVAL
        assert G.lib().gol_batch_islands_tally_sym(b._h, 0, 1, 1, 2, ctypes.byref(out), None, None, 0, ctypes.byref(nk)) == GOL_EINVAL
        assert out.value == 77 and nk.value == 77
        assert np.array_equal(b.store(), c.cells.astype(np.uint8) * 255)
