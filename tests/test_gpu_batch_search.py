"""The soup search on the GPU (gol_batch_search, Batch.search, gol_batch_load_soups): soups streamed through the
batch's boards as slots, a census per soup; and the restock pass alone on caller memory
(gol_dev_batch_restock).  Every comparison is exact: the four result arrays against tests/search_ref.py (the
oracle's soups, cycle_ref.scan, the numpy stepper, the oracle's popcount and hash), never against the library.
The main case is that of tests/test_batch_search_cpu.py, whose conditions on the reference are asserted
there (test_main_case_is_not_empty)."""
import ctypes

import numpy as np
import pytest

import cycle_ref as C
import rule_ref as R
import search_ref as S
from oracle import oracle as O
from batch_ref import tail_mask
from testlib import GOL_EINVAL, GOL_ESTATE, gpu_lib as G  # noqa: F401 (the fixture)

pytestmark = pytest.mark.gpu

SEED = 1
FILL32, FILL64 = np.int32(-0x5A5A5A5B), np.int64(-0x5A5A5A5A5A5A5A5B)  # bytes 0xA5


def assert_equal(got, want, where=None):
    assert len(got) == len(want) == 4
    for g, w in zip(got, want):
        assert g.dtype == w.dtype and g.tolist() == w.tolist(), where


def check_after(b, rule):
    """After a search every board is empty, the turn counter is 0 and the rule is kept."""
    assert b.turn == 0 and b.rule == rule
    assert not b.store_words().any() and not b.alive_counts().any()


def check_stats(st, slots, total, launch=None):
    assert st["slots"] == min(slots, total) and st["launches"] >= 1 and st["launch_turns"] >= 1
    if launch:
        assert st["launch_turns"] == launch
    assert st["full_turns"] == st["launches"] * st["slots"] * st["launch_turns"]
    assert 0 < st["board_turns"] <= st["full_turns"] and st["board_turns"] % st["launch_turns"] == 0
    assert st["occupancy"] == st["board_turns"] / st["full_turns"]


# ---------------------------------------------------------------- the main case: 40 soups of 16 x 16 through 5 slots

@pytest.mark.parametrize("tpl", [7, 64, 300, 0])
def test_main_case(G, tpl):
    want = S.search(SEED, 0, 40, 16, 16, "B3/S23", 300)
    with G.Batch(5, 16, 16, turns_per_launch=tpl) as b:
        assert b.info()["boards_per_workgroup"] == 4  # two workgroups, the second partly filled
        *got, st = b.search(SEED, 40, 300, stats=True)
        assert_equal(got, want, tpl)
        check_after(b, "B3/S23")
        check_stats(st, 5, 40, tpl)
        assert st["launch_turns"] <= 300
        # a slot idles only after the supply has run out, for less than one soup's stay (at most 300 + L turns),
        # while every soup stays at least 16 turns (the reference's earliest find) and 5 expire at 300: at L <= 64 the
        # four other slots idle under 4 * 364 turns against more than 40 * 64 made, and at L = 300 every launch is full
        assert st["occupancy"] > 0.5


def test_table_rule(G):
    want = S.search(SEED, 0, 40, 16, 16, "B36/S23", 300)
    assert int(np.sum(want[0] >= 0)) >= 10 and int(np.sum(want[0] < 0)) >= 2  # (the reference alone)
    with G.Batch(5, 16, 16, rule="B36/S23", turns_per_launch=7) as b:
        assert_equal(b.search(SEED, 40, 300), want)
        check_after(b, "B36/S23")


def test_overshoot(G):
    """Launches of 100 turns: a soup found at 257 is seen by the pass at age 300, a find with horizon 257 and none
    with horizon 256."""
    first, second = S.search(SEED, 0, 40, 16, 16, "B3/S23", 257), S.search(SEED, 0, 40, 16, 16, "B3/S23", 256)
    at257 = first[0] == 257
    assert at257.any() and np.all(second[0][at257] == -1) and np.any(second[0] == 256)  # (the reference alone)
    with G.Batch(5, 16, 16, turns_per_launch=100) as b:
        assert_equal(b.search(SEED, 40, 257), first)
        assert_equal(b.search(SEED, 40, 256), second)


# ---------------------------------------------------------------- the edges of the supply

def test_supply_edges(G):
    full = S.search(SEED, 0, 40, 16, 16, "B3/S23", 300)
    with G.Batch(8, 16, 16, turns_per_launch=7) as b:
        *got, st = b.search(SEED, 3, 300, stats=True)  # fewer soups than slots
        assert_equal(got, [a[:3] for a in full])
        check_stats(st, 8, 3, 7)
        check_after(b, "B3/S23")
        assert_equal(b.search(SEED, 8, 300), [a[:8] for a in full])  # total == n
        *got, st = b.search(SEED, 0, 300, stats=True)  # no soup
        assert all(len(a) == 0 for a in got) and st["launches"] == 0 and st["board_turns"] == 0 and st["occupancy"] == 0.0
        got = b.search(SEED, 12, 0)  # no turn: every soup at -1
        assert [a.tolist() for a in got] == [[-1] * 12, [-1] * 12, [0] * 12, [0] * 12]
        assert_equal(b.search(SEED, 12, 1), S.search(SEED, 0, 12, 16, 16, "B3/S23", 1))
        assert_equal(b.search(SEED, 10, 300, first=17), [a[17:27] for a in full])
        check_after(b, "B3/S23")
    still = S.search(SEED, 0, 12, 16, 16, "B/S012345678", 1)  # nothing is born, nothing dies: found at 1, the soup itself
    assert still[0].tolist() == [1] * 12 and np.all(still[2] > 0)
    with G.Batch(5, 16, 16, rule="B/S012345678", turns_per_launch=7) as b:
        assert_equal(b.search(SEED, 12, 1), still)


# ---------------------------------------------------------------- other shapes

@pytest.mark.parametrize("H,W,rule,horizon,total,slots,tpl", [
    (33, 65, "B3/S23", 600, 12, 4, 16),   # two words per lane, a row that ends inside a word; found and expired
    (130, 70, "B/S23", 64, 7, 3, 5),      # three waves per board, one board per workgroup
    (100, 200, "B/S23", 64, 5, 3, 5),     # NW = 8, two waves, two boards per workgroup
    (64, 64, "B1357/S1357", 200, 6, 4, 16),
    (512, 512, "B/S23", 40, 3, 2, 5),     # eight waves, NW = 16
])
def test_other_shapes(G, H, W, rule, horizon, total, slots, tpl):
    want = S.search(SEED, 0, total, H, W, rule, horizon)
    assert np.any(want[0] >= 0)
    if (H, W) == (33, 65):
        assert int(np.sum(want[0] >= 0)) == 5 and int(np.sum(want[0] < 0)) == 7  # (the reference alone)
    with G.Batch(slots, H, W, rule=rule, turns_per_launch=tpl) as b:
        info = b.info()
        assert info["waves_per_board"] == (H + 63) // 64 and info["words_per_lane"] >= (W + 31) // 32
        *got, st = b.search(SEED, total, horizon, stats=True)
        assert_equal(got, want, (H, W))
        check_stats(st, slots, total, min(tpl, horizon))
        check_after(b, rule)


# ---------------------------------------------------------------- after a search

def test_after_a_search(G):
    want = S.search(SEED, 0, 40, 16, 16, "B3/S23", 300)
    cells = np.stack([S.soup_cells(SEED, g, 16, 16) for g in range(5)])
    scan = C.scan_all(cells, R.CONWAY, 300)
    assert scan[0].tolist() == want[0][:5].tolist() and scan[1].tolist() == want[1][:5].tolist()
    final = [O.hash_words(S.to_words(c)) for c in scan[2]]
    with G.Batch(5, 16, 16, turns_per_launch=7) as b:
        b.load_soups(SEED)
        b.step(3)
        first = b.search(SEED, 40, 300)
        check_after(b, "B3/S23")
        again = b.search(SEED, 40, 300)
        assert_equal(first, want)
        assert_equal(again, want)
        for call in (b.step_cycles, b.run_cycles):  # the other scans keep their results on a freshly loaded batch
            b.load_soups(SEED)
            found, period = call(300)
            assert found.tolist() == scan[0].tolist() and period.tolist() == scan[1].tolist()
            assert b.turn == 300 and b.hashes().tolist() == final
        assert_equal(b.search(SEED, 40, 300), want)


def test_refusals_leave_everything(G):
    L = G.lib()
    with G.Batch(5, 16, 16, turns_per_launch=7) as b:
        b.load_soups(SEED)
        b.step(2)
        before = b.store_words()
        out = np.full(8, FILL64, np.int64)
        o = out.ctypes.data
        h = b._h
        bad = [L.gol_batch_search(None, 1, 0, 4, 10, o, o, o, o, None), L.gol_batch_search(h, 1, 0, 4, 10, None, o, o, o, None),
               L.gol_batch_search(h, 1, -1, 4, 10, o, o, o, o, None), L.gol_batch_search(h, 1, 0, -1, 10, o, o, o, o, None),
               L.gol_batch_search(h, 1, 0, 4, -1, o, o, o, o, None),
               L.gol_batch_search(h, 1, (1 << 40) - 3, 4, 10, o, o, o, o, None),
               L.gol_batch_search(h, 1, 0, (1 << 26) + 1, 10, o, o, o, o, None),
               L.gol_batch_load_soups(None, 1, 0), L.gol_batch_load_soups(h, 1, -1), L.gol_batch_load_soups(h, 1, (1 << 40) - 4)]
        assert bad == [GOL_EINVAL] * len(bad) and L.gol_last_error()
        b.set_rules(["B3/S23", "B36/S23"], first=1)
        st = (ctypes.c_int64 * 5)(*[77] * 5)
        assert L.gol_batch_search(h, 1, 0, 4, 10, o, o, o, o, ctypes.addressof(st)) == GOL_ESTATE
        assert np.all(out == FILL64) and list(st) == [77] * 5
        assert b.turn == 2 and np.array_equal(b.store_words(), before)
        b.set_rules(["B3/S23"], first=2)  # one rule again
        assert_equal(b.search(SEED, 8, 300), [a[:8] for a in S.search(SEED, 0, 40, 16, 16, "B3/S23", 300)])


# ---------------------------------------------------------------- load_soups

@pytest.mark.parametrize("H,W", [(16, 64), (63, 33), (129, 512)])
def test_load_soups(G, H, W):
    Ww = (W + 63) // 64
    first, n = 7, 5
    want = O.random_words(12345, 0, (first + n) * H, Ww).reshape(first + n, H, Ww)
    want[..., -1] &= tail_mask(W)
    with G.Batch(n, H, W) as b:
        b.load_random(12345)
        plain = b.hashes()
        b.step(2)
        b.load_soups(12345, 0)
        assert b.turn == 0 and np.array_equal(b.hashes(), plain) and np.array_equal(b.store_words(), want[:n])
        b.step(2)
        b.load_soups(12345, first)
        assert b.turn == 0 and np.array_equal(b.store_words(), want[first:])
    with G.Batch(first + n, H, W) as b:  # boards [first, first + n) of a larger load_random
        b.load_random(12345)
        assert np.array_equal(b.store_words(first), want[first:])
    big = 1 << 33
    with G.Batch(2, H, W) as b:
        b.load_soups(12345, big)
        assert np.array_equal(b.store_words(), np.stack([S.soup_words(12345, big + i, H, W) for i in range(2)]))


# ---------------------------------------------------------------- the restock pass alone

NOW, HORIZON = 700, 300


def restock_ref(active, counts, age, born, soup, total, out_found, out_period, harvest):
    """The pass in plain Python, on copies: the nine arrays after it."""
    active, counts, age, born, soup = active.copy(), counts.copy(), age.copy(), born.copy(), soup.copy()
    out_found, out_period, harvest = out_found.copy(), out_period.copy(), harvest.copy()
    nxt, stay, r = int(counts[3]), [], 0
    for slot in active[:counts[0]].tolist():
        f = int(age[slot])
        if f < 0 and NOW - int(born[slot]) < HORIZON:
            stay.append(slot)
            continue
        hit = 0 <= f <= HORIZON  # (found above the horizon: the overshoot, not a find)
        g = int(soup[slot])
        out_found[g] = f if hit else -1
        out_period[g] = f - C.last_mark(f) if hit else -1
        harvest[2 * r], harvest[2 * r + 1] = slot, g
        if nxt + r < total:
            soup[slot], born[slot], age[slot] = nxt + r, NOW, -1
            stay.append(slot)
        r += 1
    active[:len(stay)] = stay
    refilled = min(r, total - nxt)
    counts[:] = [len(stay), r, refilled, nxt + refilled]
    return active, counts, age, born, soup, out_found, out_period, harvest


@pytest.mark.parametrize("count", [0, 5, 1025, 16384 + 3])  # (16384 + 3: a second tile of the pass)
@pytest.mark.parametrize("which", ["mixed", "none", "all"])
def test_restock_pass_alone(G, count, which):
    import torch
    L = G.lib()
    n = count + 40
    rng = np.random.default_rng(count)
    slots = rng.permutation(n).astype(np.int32)[:count]  # the active slots, in no order
    kinds = {"mixed": [0, 1, 2, 3, 1, 0, 4], "none": [0], "all": [1, 2, 3, 4]}[which]
    done = sum(kinds[k % len(kinds)] != 0 for k in range(count))
    # the supply: plenty, ending in the middle of the list (for 16384 + 3: of the first tile), exhausted
    for left in sorted({done + 9, done // 2, 0}):
        active = np.full(count + 8, FILL32, np.int32)
        active[:count] = slots
        age, born, soup = np.full(n, FILL64, np.int64), np.full(n, FILL64, np.int64), np.full(n, FILL32, np.int32)
        for k, s in enumerate(slots):
            kind = kinds[k % len(kinds)]
            soup[s] = k
            # 0 stays; 1 found at 3 (period 2); 2 expired; 3 found at 507 (period 252) > horizon; 4 found at the horizon
            age[s] = {0: -1, 1: 3, 2: -1, 3: 507, 4: 300}[kind]
            born[s] = NOW - {0: 299, 1: 7, 2: 300, 3: 511, 4: 301}[kind]
        total = count + left
        counts = np.array([count, 77, 77, count], np.int32)
        out_found, out_period = np.full(total + 4, FILL64, np.int64), np.full(total + 4, FILL64, np.int64)
        harvest = np.full(2 * n, FILL32, np.int32)
        host = (active, counts, age, born, soup, out_found, out_period, harvest)
        want = restock_ref(active, counts, age, born, soup, total, out_found, out_period, harvest)
        if count >= 1025 and which == "mixed":  # (the reference alone) every verdict, finds of two periods, the supply's end
            assert want[1][1] == done and set(want[5][:count].tolist()) >= {3, 300, -1} and set(want[6][:count].tolist()) >= {2, 45}
            assert FILL64 in want[5][:count].tolist() and want[1][2] == min(done, left)
        dev = [torch.from_numpy(a).cuda() for a in host]
        p = [t.data_ptr() for t in dev]
        rc = L.gol_dev_batch_restock(p[0], p[1], p[2], p[3], p[4], n, NOW, HORIZON, total, p[5], p[6], p[7], None)
        assert rc == 0, L.gol_last_error()
        torch.cuda.synchronize()
        for i, (t, w) in enumerate(zip(dev, want)):
            got = t.cpu().numpy()
            if i == 0:  # the active list is compacted in place: the entries past the new count are not specified
                m = int(want[1][0])
                assert np.array_equal(got[:m], w[:m]) and np.all(got[count:] == FILL32), (left, i)
            else:
                assert np.array_equal(got, w), (left, i)


def test_restock_pass_refusals(G):
    import torch
    L = G.lib()
    t = torch.zeros(64, dtype=torch.int64, device="cuda")
    p = t.data_ptr()
    ok = [p] * 5 + [4, 10, 5, 3, p, p, p, None]
    bad = []
    for i in (0, 1, 2, 3, 4, 9, 10, 11):
        args = list(ok)
        args[i] = None
        bad.append(L.gol_dev_batch_restock(*args))
    for i, v in ((5, 0), (5, (1 << 20) + 1), (6, -1), (7, -1), (8, -1), (8, (1 << 26) + 1)):
        args = list(ok)
        args[i] = v
        bad.append(L.gol_dev_batch_restock(*args))
    assert bad == [GOL_EINVAL] * len(bad)
    torch.cuda.synchronize()
    assert not t.any()
