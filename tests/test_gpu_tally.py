"""The tally of island kinds on the GPU: every TALLY instantiation of batch_islands_kernel (csrc/gol_island.hip) on
caller memory through gol_dev_batch_islands_tally, dense and listed, against the reference of tests/tally_ref.py (a
collections tally over island_ref.census, written from include/golhip.h), every compared field bit for bit; then
Batch.census and Batch.islands_tally.  The case tables are island_ref's and tally_ref's (their preconditions are
asserted in tests/test_tally_ref_cpu.py).  Every buffer of a launch lies between two margins of sentinel bytes,
count and fingerprint are filled with 0xA5 before the launch, and the boards are compared byte for byte after it."""
import ctypes

import numpy as np
import pytest

import island_ref as I
import tally_ref as T
from tally_ref import ORDER, REFUSED, Launch
from testlib import GOL_EINVAL, GOL_ENOMEM, GOL_ESTATE, Guarded, gpu_lib as G  # noqa: F401 (the fixture)

pytestmark = pytest.mark.gpu

FILL = T.FILL
SENTINEL = int.from_bytes(bytes([FILL]) * 8, "little")


def want_of_case(c, reach, owner0=0):
    res = I.want(c, reach)
    counts = np.array([len(r) for r, _ in res], dtype=np.int64)
    fps = np.array([fp for _, fp in res], dtype=np.uint64)
    return counts, fps, T.tally((owner0 + i, r) for i, (recs, _) in enumerate(res) for r in recs)


def log2_for(kinds, least=4):
    return max(least, int(np.ceil(np.log2(max(kinds, 1)))))


# ------------------------------------------------------------------------------------------- the raw entry, dense
@pytest.mark.parametrize("c", I.CASES, ids=lambda c: c.id)
def test_dense_case(G, c):
    for reach in c.reaches:
        counts, fps, kinds = want_of_case(c, reach, owner0=1000)
        L = Launch(G, c.cells, log2_for(2 * len(kinds)))
        assert L.run(reach, owner0=1000) == 0, (c.id, G.lib().gol_last_error())
        got = L.results()
        assert np.array_equal(got[0], counts) and np.array_equal(got[1], fps), (c.id, reach)
        assert got[3] == 0 and np.array_equal(got[2], kinds), (c.id, reach, got[2][:3], kinds[:3])


@pytest.fixture(scope="module")
def boards():
    cells = T.boards_case()
    return cells, {reach: T.of_boards(cells, reach) for reach in (1, 2)}


def test_table_sizes(G, boards):
    cells, want = boards
    for reach in (1, 2):
        counts, fps, kinds = want[reach]
        D = len(kinds)
        small = log2_for(D)  # the smallest table that holds every kind: probes wrap
        home = G.lib().gol_island_tally_home_host
        homes = [home(int(h), small) for h in kinds["hash"]]
        pair = next((a, b) for a in range(D) for b in range(a + 1, D) if homes[a] == homes[b])
        for log2 in (small, 10):
            L = Launch(G, cells, log2)
            assert L.run(reach) == 0
            got = L.results()
            assert np.array_equal(got[0], counts) and np.array_equal(got[1], fps)
            assert got[3] == 0 and np.array_equal(got[2], kinds), (reach, log2)
            assert {int(kinds["hash"][i]) for i in pair} <= set(got[2]["hash"].tolist())  # two kinds of one home slot
        # a table of D / 2 slots or fewer is full: what it turns away is counted, what it holds is genuine
        log2 = int(np.floor(np.log2(D // 2)))
        L = Launch(G, cells, log2)
        assert L.run(reach) == 0
        c2, f2, k2, dropped = L.results()
        assert np.array_equal(c2, counts) and np.array_equal(f2, fps)
        assert dropped > 0 and int(k2["count"].sum()) + dropped == int(counts.sum()) and len(k2) == 1 << log2
        ref = {int(k["hash"]): k for k in kinds}
        for k in k2:
            w = ref[int(k["hash"])]
            assert 0 < k["count"] <= w["count"] and k["first"] >= w["first"]
            assert (k["cells"], k["rows"], k["cols"]) >= (w["cells"], w["rows"], w["cols"])


def test_accumulation(G, boards):
    cells, want = boards
    half = len(cells) // 2
    for reach in (1, 2):
        counts, fps, kinds = want[reach]
        # two launches into one table: the tally of the union, the owners those of the whole stack
        L = Launch(G, cells[:half], 10)
        assert L.run(reach) == 0
        first = L.results()
        assert np.array_equal(first[2], T.of_boards(cells[:half], reach)[2])
        M = Launch(G, cells[half:], 10)
        M.table = L.table
        assert M.run(reach, owner0=half) == 0
        got = M.results()
        assert np.array_equal(got[0], counts[half:]) and np.array_equal(got[2], kinds) and got[3] == 0
        # the same boards again under higher owners: the counts double, first stays the lower owner
        assert L.run(reach, owner0=500) == 0 and M.run(reach, owner0=500 + half) == 0
        twice = kinds.copy()
        twice["count"] *= 2
        assert np.array_equal(M.results()[2], twice)
        # and one board twice in one stack
        L = Launch(G, np.stack([cells[1], cells[3], cells[1]]), 10)
        assert L.run(reach, owner0=7) == 0
        assert np.array_equal(L.results()[2], T.tally([(7 + i, r) for i, b in enumerate((1, 3, 1)) for r in I.census(cells[b], reach)[0]]))


# ------------------------------------------------------------------------------------------ the raw entry, listed
def _listed(G, cells, reach, k, max_pairs, owner0=0, expired=True):
    """A launch over the first k of a shuffled list of (slot, soup) pairs, the soups scattered over 0 .. 99; the last
    listed pair's soup expired (found -1), its board poisoned.  Returns (Launch, rc, pairs, soups that work)."""
    n = len(cells)
    rng = np.random.default_rng(11)
    slots = rng.permutation(n)[:max_pairs]
    soups = rng.permutation(100)[:max_pairs]
    found = np.full(100, 5, dtype=np.int64)
    cells = cells.copy()
    dead = k - 1 if expired and k > 0 else None
    if dead is not None:
        found[soups[dead]] = -1
        cells[slots[dead]] = 1  # a full board: one huge island, were it read
    L = Launch(G, cells, 10, outs=100)
    pairs = Guarded(np.stack([slots, soups], axis=1).astype(np.int32), name="pairs")
    rc = L.run(reach, owner0=owner0, pairs=pairs, pair_count=Guarded(np.array([k, 0], dtype=np.int32), name="pair_count"),
               max_pairs=max_pairs, found=Guarded(found, name="found"))
    assert pairs.unchanged()
    return L, rc, [(int(s), int(g)) for s, g in zip(slots[:k], soups[:k])], dead


@pytest.mark.parametrize("k", [0, 9, 16])
def test_listed(G, boards, k):
    cells, _ = boards
    for reach in (1, 2):
        L, rc, pairs, dead = _listed(G, cells, reach, k, 16, owner0=3000)
        assert rc == 0, G.lib().gol_last_error()
        count, fp, kinds, dropped = L.results()
        want_count, want_fp = np.full(100, SENTINEL, dtype=np.uint64).view(np.int64), np.full(100, SENTINEL, dtype=np.uint64)
        tallied = []
        for i, (slot, soup) in enumerate(pairs):
            recs, f = ([], 0) if i == dead else I.census(cells[slot], reach)
            want_count[soup], want_fp[soup] = len(recs), f
            tallied += [(3000 + soup, r) for r in recs]
        # the soups not listed, and with k = 0 everything, stay at the sentinel
        assert np.array_equal(count, want_count) and np.array_equal(fp, want_fp), (reach, k)
        assert dropped == 0 and np.array_equal(kinds, T.tally(tallied)), (reach, k)
        assert k > 0 or len(kinds) == 0


def test_listed_passes_over_bad_pairs(G, boards):
    """A slot outside the boards or a negative soup (the restock pass writes -1 for a soup it cannot place) is passed over."""
    cells, _ = boards
    L = Launch(G, cells[:4], 10, outs=8)
    pairs = Guarded(np.array([[0, 2], [4, 1], [-1, 3], [1, -1], [3, 5]], dtype=np.int32), name="pairs")
    rc = L.run(1, pairs=pairs, pair_count=Guarded(np.array([5, 0], dtype=np.int32), name="pair_count"), max_pairs=4,
               found=Guarded(np.zeros(8, dtype=np.int64), name="found"), n=4)
    assert rc == 0
    count, _, kinds, _ = L.results()
    # (max_pairs 4: the fifth pair is not run)
    assert [int(c) for c in count] == [SENTINEL - (1 << 64)] * 2 + [len(I.census(cells[0], 1)[0])] + [SENTINEL - (1 << 64)] * 5
    assert np.array_equal(kinds, T.tally((2, r) for r in I.census(cells[0], 1)[0]))


# --------------------------------------------------------------------------------------- the raw entry, refusals
def test_refusals_launch_nothing(G, boards):
    cells, _ = boards
    L = Launch(G, cells[:3], 10)
    pairs, pc, found = Guarded(np.zeros((3, 2), dtype=np.int32)), Guarded(np.array([3, 0], dtype=np.int32)), Guarded(np.zeros(3, dtype=np.int64))
    real = dict(boards=L.boards.ptr, count=L.count.ptr, fingerprint=L.fp.ptr, table=L.table.ptr, dropped=L.dropped.ptr,
                pairs=pairs.ptr, pair_count=pc.ptr, found=found.ptr)
    check, launch = G.lib().gol_batch_islands_tally_check_host, G.lib().gol_dev_batch_islands_tally
    import torch
    for base, bad in REFUSED:
        a = dict(base, H=cells.shape[1], W=cells.shape[2])
        a.update({k: real[k] for k, v in a.items() if v is not None and k in real})
        a.update({k: (real[k] if v is not None and k in real else v) for k, v in bad.items()})
        args = [a[k] for k in ORDER]
        assert check(*args) == GOL_EINVAL, bad
        assert launch(*args, torch.cuda.current_stream().cuda_stream) == GOL_EINVAL, bad
    torch.cuda.synchronize()
    for b in (L.count, L.fp, L.table, L.dropped, L.boards):
        assert b.unchanged()


def test_table_clear(G):
    import torch
    t = Guarded(np.full(64 * 32, 0x77, dtype=np.uint8), name="table")
    d = Guarded(np.full(8, 0x77, dtype=np.uint8), name="dropped")
    s = torch.cuda.current_stream().cuda_stream
    assert G.lib().gol_dev_island_table_clear(t.ptr, 6, d.ptr, s) == 0
    torch.cuda.synchronize()
    assert np.array_equal(t.read(T.SLOT_DTYPE), T.empty_table(6)) and d.read(np.int64)[0] == 0
    assert G.lib().gol_dev_island_table_clear(t.ptr, 3, d.ptr, s) == GOL_EINVAL
    assert G.lib().gol_dev_island_table_clear(None, 6, d.ptr, s) == GOL_EINVAL


# -------------------------------------------------------------------------------------------------- Batch.census
def assert_census(got, want, where):
    for k, w in want.items():
        assert np.array_equal(got[k], w), (where, k, got[k][:4], w[:4])


@pytest.mark.parametrize("c", T.SOUP_CASES, ids=lambda c: c.id)
def test_census(G, c):
    for reach in (1, 2):
        want = T.census(c, reach)
        for slots, tpl in ((8, 1), (17, 7), (64, 0)):
            with G.Batch(slots, c.H, c.W, rule=T.RULE, device=0, turns_per_launch=tpl) as b:
                got = b.census(T.SEED, c.total, c.horizon, reach=reach, stats=True)
                assert_census(got, want, (c.id, reach, slots, tpl))
                assert got["kinds"].dtype == G.ISLAND_KIND_DTYPE
                assert not b.store_words().any() and b.turn == 0  # as after search
                if tpl != 7:
                    continue
                # the first four outputs and the stats are those of search on the same build
                found, period, alive, hashes, st = b.search(T.SEED, c.total, c.horizon, stats=True)
                assert st == got["stats"]
                for k, a in zip(("found", "period", "alive", "hash"), (found, period, alive, hashes)):
                    assert np.array_equal(got[k], a), (c.id, k)


def test_census_first_truncation_and_empty(G):
    c = T.SOUP_CASES[0]
    want = T.census(c, 1, 5, 20)
    with G.Batch(6, c.H, c.W, rule=T.RULE, device=0, turns_per_launch=16) as b:
        got = b.census(T.SEED, 20, c.horizon, first=5)
        assert_census(got, want, "first")
        assert got["kinds"]["first"].min() >= 5
        cut = b.census(T.SEED, 20, c.horizon, first=5, kinds=3)
        assert cut["n_kinds"] == want["n_kinds"] > 3 and np.array_equal(cut["kinds"], want["kinds"][:3])
        assert np.array_equal(cut["islands"], want["islands"])
        none = b.census(T.SEED, 20, c.horizon, first=5, kinds=0)
        assert none["n_kinds"] == want["n_kinds"] and len(none["kinds"]) == 0
        for total, horizon in ((0, 100), (7, 0)):
            e = b.census(T.SEED, total, horizon)
            assert e["n_kinds"] == 0 and len(e["kinds"]) == 0 and len(e["found"]) == total
            assert np.all(e["found"] == -1) and not e["islands"].any() and not e["fingerprint"].any()
        # the refusals: nothing is written
        out = np.full(4, 77, dtype=np.int64)
        nk = ctypes.c_int64(77)
        f = G.lib().gol_batch_census
        p, kinds = out.ctypes.data, np.zeros(4, dtype=G.ISLAND_KIND_DTYPE)
        bad = [f(b._h, 1, 0, 4, 10, 0, p, None, None, None, None, None, kinds.ctypes.data, 4, ctypes.byref(nk), None),
               f(b._h, 1, 0, 4, 10, 3, p, None, None, None, None, None, kinds.ctypes.data, 4, ctypes.byref(nk), None),
               f(b._h, 1, 0, 4, 10, 1, p, None, None, None, None, None, kinds.ctypes.data, -1, ctypes.byref(nk), None),
               f(b._h, 1, 0, 4, 10, 1, p, None, None, None, None, None, kinds.ctypes.data, (1 << 23) + 1, ctypes.byref(nk), None),
               f(b._h, 1, 0, 4, 10, 1, p, None, None, None, None, None, None, 4, ctypes.byref(nk), None),
               f(b._h, 1, 0, 4, 10, 1, p, None, None, None, None, None, kinds.ctypes.data, 4, None, None),
               f(b._h, 1, 0, 4, 10, 1, None, None, None, None, None, None, kinds.ctypes.data, 4, ctypes.byref(nk), None),
               f(b._h, 1, 0, 4, -1, 1, p, None, None, None, None, None, kinds.ctypes.data, 4, ctypes.byref(nk), None),
               f(None, 1, 0, 4, 10, 1, p, None, None, None, None, None, kinds.ctypes.data, 4, ctypes.byref(nk), None)]
        assert bad == [GOL_EINVAL] * len(bad) and np.all(out == 77) and nk.value == 77 and not kinds.tobytes().strip(b"\0")
        # a rule per board
        b.set_rules(["B36/S23"], first=2)
        with pytest.raises(G.GolError) as e:
            b.census(T.SEED, 20, c.horizon)
        assert e.value.code == GOL_ESTATE


# ------------------------------------------------------------------------------------------- Batch.islands_tally
def _numpy_tally(counts, recs, owner0=0):
    return T.tally((owner0 + i, r) for i in range(len(counts)) for r in recs[i, :counts[i]])


def test_islands_tally_on_settled_soups(G):
    S = I.SOUPS
    n = 64  # of the census's own soups: enough for kinds that repeat
    rng = np.random.default_rng(9)
    with G.Batch(n, S["side"], S["side"], device=0) as b:
        b.load_soups(S["seed"])
        b.run_cycles(S["turns"])
        cells = b.store()
        for reach in (1, 2):
            counts, fps, kinds = b.islands_tally(reach=reach)
            c0, recs, f0 = b.islands(reach=reach, cap=256, fingerprints=True)
            assert c0.max() <= 256 and np.array_equal(counts, c0) and np.array_equal(fps, f0)
            assert np.array_equal(kinds, _numpy_tally(c0, recs)) and len(kinds) >= 15
            assert np.array_equal(kinds, T.of_boards(cells, reach)[2]), reach
            # a range in the middle of the batch: the owners are the boards' indices
            c1, f1, k1 = b.islands_tally(reach=reach, first=7, count=20)
            assert np.array_equal(c1, c0[7:27]) and np.array_equal(f1, f0[7:27])
            assert np.array_equal(k1, _numpy_tally(c0[7:27], recs[7:27], owner0=7))
            cut = b.islands_tally(reach=reach, kinds=5)[2]
            assert np.array_equal(cut, kinds[:5])
        assert np.array_equal(b.store(), cells) and b.turn == S["turns"]
        want = {reach: b.islands_tally(reach=reach) for reach in (1, 2)}
        for bad in (dict(reach=0), dict(reach=3), dict(kinds=-1), dict(first=-1), dict(first=1, count=n), dict(kinds=(1 << 23) + 1)):
            with pytest.raises(G.GolError) as e:
                b.islands_tally(**bad)
            assert e.value.code == GOL_EINVAL
    # unchanged under a random torus translation per board, apart from `first`
    rolled = np.stack([np.roll(c, tuple(int(v) for v in rng.integers(0, c.shape)), axis=(0, 1)) for c in cells])
    with G.Batch(n, S["side"], S["side"], device=0) as b:
        b.load(rolled[::-1])  # the boards in the reverse order: `first` does change
        for reach in (1, 2):
            counts, fps, kinds = b.islands_tally(reach=reach)
            assert np.array_equal(counts[::-1], want[reach][0]) and np.array_equal(fps[::-1], want[reach][1])
            for f in ("hash", "count", "cells", "rows", "cols"):
                assert np.array_equal(kinds[f], want[reach][2][f]), (reach, f)


def test_table_full_through_the_public_call(G):
    cells = T.distinct_islands()
    with G.Batch(len(cells), 16, 16, device=0) as b:
        b.load(cells)
        with pytest.raises(G.GolError) as e:
            b.islands_tally(kinds=1)  # a table of 1024 slots for 1200 kinds
        assert e.value.code == GOL_ENOMEM and "kinds_cap" in str(e.value)
        assert np.all(e.value.counts == 1)
        counts, fps, kinds = b.islands_tally(kinds=4096)
        assert np.array_equal(e.value.fingerprints, fps) and np.all(counts == 1)
        # (a few of the 1200 islands share their multiset of window codes with another: they are one kind)
        assert len(kinds) >= 1100 and int(kinds["count"].sum()) == len(cells)
        assert np.array_equal(kinds, T.of_boards(cells, 1)[2])
        assert set(kinds["hash"].tolist()) == set(fps.tolist())  # one island a board: its hash is the fingerprint
        assert np.array_equal(b.store(), cells * 255)
