"""The tally of island kinds without a GPU: the reference of tests/tally_ref.py (a collections tally over
island_ref.census) against the two host twins (gol_island_tally_host, the definition by a sort and a merge, and
gol_batch_census_host, the scheme of a search with the census of every s(found)), the stand-alone driver under
AddressSanitizer + UndefinedBehaviorSanitizer (build/asan/tally_check, a plain child process; nothing loaded into
Python is sanitized), the refusals of the launch check argument by argument, the home slot function, and the
preconditions of the GPU tests (tests/test_gpu_tally.py), asserted on the reference alone.  All comparisons are
exact."""
import ctypes
import subprocess

import numpy as np
import pytest

import island_ref as I
import rule_ref as R
import tally_ref as T
from tally_ref import DENSE, LISTED, ORDER, P, REFUSED
from testlib import GOL_EINVAL, check_program, cpu_lib as G  # noqa: F401 (the fixture)


def host_tally(G, pairs, cap=None):
    """(kinds[:min(n_kinds, cap)], n_kinds) of the pairs through gol_island_tally_host."""
    pairs = list(pairs)
    recs = np.array([r for _, r in pairs], dtype=I.DTYPE) if pairs else np.zeros(0, dtype=I.DTYPE)
    owners = np.array([o for o, _ in pairs], dtype=np.int64)
    cap = len(pairs) if cap is None else cap
    kinds = np.zeros(cap, dtype=T.KIND_DTYPE)
    n = ctypes.c_int64(-7)
    rc = G.lib().gol_island_tally_host(recs.ctypes.data, owners.ctypes.data, len(pairs), kinds.ctypes.data if cap else None, cap,
                                       ctypes.byref(n))
    assert rc == 0, G.lib().gol_last_error()
    return kinds[:min(n.value, cap)], n.value


def test_dtype_and_reference_pins(G):
    assert G.ISLAND_KIND_DTYPE == T.KIND_DTYPE and T.KIND_DTYPE.itemsize == T.SLOT_DTYPE.itemsize == 32
    r = np.array([(0, 0, 4, 2, 2, 9), (1, 1, 3, 1, 3, 5), (2, 2, 3, 3, 1, 9), (0, 0, 1, 1, 1, 0), (5, 5, 4, 1, 4, 9)], dtype=I.DTYPE)
    kinds = T.tally(zip((7, 3, 4, 8, 6), r))
    # 9 three times (lowest owner 4, smallest shape (3, 3, 1)), then hash 0 under 1, then 5
    assert kinds.tolist() == [(9, 3, 4, 3, 3, 1), (1, 1, 8, 1, 1, 1), (5, 1, 3, 3, 1, 3)]
    got, n = host_tally(G, zip((7, 3, 4, 8, 6), r))
    assert n == 3 and np.array_equal(got, kinds)
    # the order of the pairs does not matter
    got, _ = host_tally(G, list(zip((7, 3, 4, 8, 6), r))[::-1])
    assert np.array_equal(got, kinds)


def test_host_tally_on_the_case_table(G):
    for c in I.CASES:
        if c.cells.size > 70000:
            continue
        for reach in c.reaches:
            pairs = [(100 + i, r) for i, (recs, _) in enumerate(I.want(c, reach)) for r in recs]
            want = T.tally(pairs)
            got, n = host_tally(G, pairs)
            assert n == len(want) and np.array_equal(got, want), (c.id, reach)
            for cap in (0, 1, max(len(want) - 1, 0)):  # truncation in the tally's order, n_kinds the same
                got, n = host_tally(G, pairs, cap)
                assert n == len(want) and np.array_equal(got, want[:cap]), (c.id, reach, cap)


def host_census(G, c, reach, slots, launch, first=0, total=None, cap=4096):
    total = c.total if total is None else total
    b, s = R.masks(T.RULE)
    out = [np.zeros(total, dtype=t) for t in (np.int64, np.int64, np.uint64, np.uint64, np.int64, np.uint64)]
    kinds = np.zeros(cap, dtype=T.KIND_DTYPE)
    n = ctypes.c_int64(-7)
    rc = G.lib().gol_batch_census_host(c.H, c.W, b, s, T.SEED, first, total, slots, launch, c.horizon, reach,
                                       *[a.ctypes.data for a in out], kinds.ctypes.data, cap, ctypes.byref(n))
    assert rc == 0, G.lib().gol_last_error()
    return dict(zip(("found", "period", "alive", "hash", "islands", "fingerprint"), out), kinds=kinds[:min(n.value, cap)],
                n_kinds=n.value)


def assert_census(got, want, where):
    for k, w in want.items():
        assert np.array_equal(got[k], w), (where, k)


@pytest.mark.parametrize("c", T.SOUP_CASES, ids=lambda c: c.id)
def test_host_census_twin_and_soup_preconditions(G, c):
    """The census twin against the reference at both reaches, through two slot counts and launch lengths; and what
    the GPU soup tests need so that they show something: at least half the soups found, one not found, 15 kinds,
    8 of them more than once."""
    for reach in (1, 2):
        want = T.census(c, reach)
        assert_census(host_census(G, c, reach, 17, 7), want, (c.id, reach))
        assert_census(host_census(G, c, reach, 8, 64), want, (c.id, reach))
        found = int((want["found"] >= 0).sum())
        assert found >= c.total // 2 and found < c.total, (c.id, found)
        assert want["n_kinds"] >= 15 and int((want["kinds"]["count"] > 1).sum()) >= 8, (c.id, reach, want["n_kinds"])
        assert int(want["islands"].sum()) == int(want["kinds"]["count"].sum())
        assert np.all(want["islands"][want["found"] < 0] == 0) and np.all(want["fingerprint"][want["found"] < 0] == 0)
    # first > 0 shifts the soup numbers, and truncation keeps n_kinds
    want = T.census(c, 1, 5, 20)
    assert_census(host_census(G, c, 1, 6, 16, first=5, total=20), want, c.id)
    assert want["kinds"]["first"].min() >= 5
    got = host_census(G, c, 1, 6, 16, first=5, total=20, cap=3)
    assert got["n_kinds"] == want["n_kinds"] > 3 and np.array_equal(got["kinds"], want["kinds"][:3])


def test_tally_check_under_sanitizers():
    """The two host twins in the stand-alone program, every block a heap block of its exact size."""
    r = subprocess.run([check_program("tally_check")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "0 bad" in r.stdout


def test_launch_check_refusals(G):
    """gol_batch_islands_tally_check_host: the one check every launch passes; of a pointer only its value counts."""
    check = G.lib().gol_batch_islands_tally_check_host

    def rc(base, **over):
        a = dict(base, **over)
        return check(*[a[k] for k in ORDER])

    assert rc(DENSE) == 0 and rc(LISTED) == 0
    assert rc(DENSE, fingerprint=None) == 0 and rc(LISTED, fingerprint=None) == 0 and rc(DENSE, reach=2) == 0
    assert rc(DENSE, table_log2=4) == 0 and rc(DENSE, table_log2=24) == 0 and rc(DENSE, owner0=1 << 40) == 0
    assert rc(DENSE, n=1 << 20, H=512, W=512) == 0 and rc(LISTED, H=1, W=1, max_pairs=1) == 0
    for base, bad in REFUSED:
        assert rc(base, **bad) == GOL_EINVAL, bad
    # the plain launch's check is as it was
    assert G.lib().gol_batch_islands_check_host(P, 3, 64, 64, 1, 8, P, P, P) == 0


def test_home_slot(G):
    home = G.lib().gol_island_tally_home_host
    rng = np.random.default_rng(3)
    for log2 in range(4, 25):
        at = [home(int(h), log2) for h in rng.integers(0, 1 << 63, 200, dtype=np.int64)] + [home(0, log2), home((1 << 64) - 1, log2)]
        assert min(at) >= 0 and max(at) < 1 << log2
        assert home(0, log2) == home(1, log2)  # hash 0 is tallied under 1
    assert len({home(int(h), 10) for h in rng.integers(0, 1 << 63, 200, dtype=np.int64)}) > 150  # it spreads
    assert home(5, 3) == -1 and home(5, 25) == -1


def test_boards_case_preconditions(G):
    """The case of the raw entry's table sizes: its kinds D, a pair of kinds that share a home slot in the smallest
    table that holds them all, and kinds that occur more than once."""
    cells = T.boards_case()
    home = G.lib().gol_island_tally_home_host
    for reach in (1, 2):
        counts, _, kinds = T.of_boards(cells, reach)
        D = len(kinds)
        log2 = max(4, int(np.ceil(np.log2(D))))
        assert 32 < D <= 1 << log2 < 2 * D and counts.sum() > D  # (a load above 1/2; kinds that repeat)
        homes = [home(int(h), log2) for h in kinds["hash"]]
        assert len(set(homes)) < len(homes), "no two kinds share a home slot"
        assert int((kinds["count"] > 1).sum()) >= 8 and (D // 2) >= 16


def test_distinct_islands_precondition():
    """The batch of the table-full test: one island per board, at least 1100 kinds (a public table has at least
    1024 slots)."""
    cells = T.distinct_islands()
    for reach in (1, 2):
        counts, _, kinds = T.of_boards(cells, reach)
        assert np.all(counts == 1) and len(kinds) >= 1100
