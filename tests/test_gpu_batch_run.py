"""Retirement of found boards on the GPU (gol_batch_run_cycles, Batch.run_cycles): the boards, found,
period and the turn counter are those of gol_batch_step_cycles, and `made` says how much less was
computed; and the retire pass alone on caller memory (gol_dev_batch_retire).  Every comparison is
exact.  The expectations come from tests/cycle_ref.py (the scan's definition) and the `made` formula of
include/golhip.h, written out in made_ref below, never from the library, and each test first asserts on
the reference's own results that its input exercises the case it is here for."""
import numpy as np
import pytest

import cycle_ref as C
import rule_ref as R
from cycle_ref import RULES
from batch_ref import batch_n, check_queries, random_boards, ref_settle
from testlib import GOL_EINVAL, gpu_lib as G  # noqa: F401 (the fixture)

pytestmark = pytest.mark.gpu


def made_ref(found, period, turns, launch, t0=0):
    """The turns a board computes: to the end of the first launch that ends at t_L >= found, t_L = t0 +
    min(turns, launch * ceil((found - t0) / launch)), then (t0 + turns - t_L) mod period; all the turns
    when it is never found."""
    if found < 0:
        return turns
    at = t0 + min(turns, launch * -(-(found - t0) // launch))
    return (at - t0) + (t0 + turns - at) % period


def made_all(want, turns, launch, t0=0):
    return [made_ref(int(f), int(p), turns, launch, t0) for f, p in zip(want[0], want[1])]


def check_run(b, turns, want, launch, t0=0):
    """run_cycles against the reference's scan; `launch` 0: the automatic length, made within its bounds."""
    found, period, made = b.run_cycles(turns, made=True)
    assert found.dtype == period.dtype == made.dtype == np.int64
    assert found.tolist() == want[0].tolist() and period.tolist() == want[1].tolist()
    if launch:
        assert made.tolist() == made_all(want, turns, launch, t0)
    else:
        assert all(m <= turns and (f < 0 and m == turns or f >= 0 and m >= f - t0) for f, m in zip(found.tolist(), made.tolist()))
    assert b.turn == t0 + turns
    check_queries(b, want[2])
    return made


# ---------------------------------------------------------------- boards of one workgroup with different remainders

def mix_16():
    cells = np.zeros((13, 16, 16), np.uint8)
    for i, (rows, y, x) in enumerate([([], 0, 0), (C.BLOCK, 3, 3), (C.BLINKER, 5, 4), (C.GLIDER, 1, 1), (C.R_PENTOMINO, 6, 6),
                                      (C.PULSAR, 1, 1)]):
        cells[i] = C.place(16, 16, rows, y, x)
    for i in range(7):
        cells[6 + i] = R.random_board(1000 + i, 16, 16, 0.35)
    return cells


@pytest.fixture(scope="module")
def mix_16_ref():
    cells = mix_16()
    return cells, C.scan_all(cells, R.CONWAY, 400)


@pytest.mark.parametrize("tpl", [1, 5, 7, 64, 400, 0])
def test_one_workgroup_different_remainders(G, mix_16_ref, tpl):
    cells, want = mix_16_ref
    n = len(cells)
    # (the reference alone) the first workgroup's four boards leave at different launches with different remainders
    assert want[0][:4].tolist() == [1, 1, 3, 127] and want[1][:4].tolist() == [1, 1, 2, 64]
    at = [7 * -(-int(f) // 7) for f in want[0][:4]]
    assert [(400 - a) % int(p) for a, p in zip(at, want[1][:4])] == [0, 0, 1, 11]
    assert [i for i in range(n) if want[0][i] < 0] == [8, 10]  # the soups of seeds 1002 and 1004 are never found
    assert sum(made_all(want, 400, 7)) < 0.5 * n * 400
    with G.Batch(n, 16, 16, turns_per_launch=tpl) as b:
        assert b.info()["boards_per_workgroup"] == 4 and n >= 2 * 4 + 1
        b.load(cells)
        check_run(b, 400, want, tpl)


# ---------------------------------------------------------------- boards of several waves, a row of two words

@pytest.mark.parametrize("H,W,patterns", [
    (129, 65, [(C.PULSAR, 57, 58), (C.ROW10, 63, 60), (C.GLIDER, 60, 30)]),  # three waves, one board per workgroup
    (65, 31, [(C.PULSAR, 57, 20), (C.ROW10, 63, 25), (C.GLIDER, 60, 3), (C.BLINKER, 64, 30)]),  # two waves, two boards
    (5, 33, [(C.BLINKER, 2, 31), (C.BLOCK, 4, 32), ([], 0, 0)]),
])
def test_boards_of_several_waves(G, H, W, patterns):
    n = max(batch_n(G, H, W), len(patterns) + 2)
    cells = random_boards(3 * H + W, n, H, W)
    for i, (rows, y, x) in enumerate(patterns):
        cells[i] = C.place(H, W, rows, y, x)
    want = C.scan_all(cells, R.CONWAY, 100)
    made = made_all(want, 100, 7)
    # (the reference alone) boards that leave with and without a remainder, and one that stays to the end
    left = [m - min(100, 7 * -(-int(f) // 7)) for f, m in zip(want[0], made) if f >= 0]
    assert 0 in left and any(v > 0 for v in left) and (H == 5 or np.any(want[0] < 0))
    with G.Batch(n, H, W, turns_per_launch=7) as b:
        assert b.info()["waves_per_board"] == (H + 63) // 64
        b.load(cells)
        check_run(b, 100, want, 7)


# ---------------------------------------------------------------- a finish of many launches on a shrinking list

def test_long_finish(G):
    H, W = 7, 9
    n = batch_n(G, H, W)
    cells = random_boards(99, n, H, W)
    cells[2] = C.place(H, W, C.GLIDER)
    want = C.scan_all(cells, R.CONWAY, 1100)
    made = made_all(want, 1100, 7)
    assert (want[0][2], want[1][2], made[2]) == (507, 252, 596) and made[2] - 511 == 85  # 13 finish launches of 7
    left = sorted(m - min(1100, 7 * -(-int(f) // 7)) for f, m in zip(want[0], made) if f >= 0)
    assert left[-1] == 85 and len(set(left)) >= 3  # the finish list shrinks from launch to launch
    with G.Batch(n, H, W, turns_per_launch=7) as b:
        b.load(cells)
        check_run(b, 1100, want, 7)


# ---------------------------------------------------------------- a rule per board

@pytest.mark.parametrize("seed,H,W,density", [(4243, 5, 33, 0.4), (4242, 16, 16, 0.35)])
def test_run_with_rules_per_board(G, seed, H, W, density):
    cells = np.stack([R.random_board(seed, H, W, density)] * 18)
    want = C.scan_all(cells, RULES, 300)
    assert int(np.sum(want[0] < 0)) == 5 and len(set(want[1][want[1] > 0].tolist())) >= 2
    if H == 5:  # one board of period 28 leaves with 27 turns to make
        i = want[1].tolist().index(28)
        assert made_ref(int(want[0][i]), 28, 300, 7) - 7 * -(-int(want[0][i]) // 7) == 27
    for tpl in (7, 0):
        with G.Batch(18, H, W, turns_per_launch=tpl) as b:
            b.load(cells)
            b.set_rules(RULES)
            check_run(b, 300, want, tpl)
            assert np.array_equal(b.rules(), np.array([R.masks(r) for r in RULES], np.uint32))


# ---------------------------------------------------------------- equivalence and sequencing

def test_run_equals_step_cycles_and_step(G, mix_16_ref):
    cells, want = mix_16_ref
    with G.Batch(len(cells), 16, 16, turns_per_launch=7) as b:
        b.load(cells)
        b.step(400)
        plain = (b.store_words(), b.hashes())
        b.load(cells)
        sc = b.step_cycles(400)
        scanned = (b.store_words(), b.hashes())
        b.load(cells)
        rc = b.run_cycles(400)
        retired = (b.store_words(), b.hashes())
        assert b.turn == 400
    assert sc[0].tolist() == rc[0].tolist() == want[0].tolist() and sc[1].tolist() == rc[1].tolist() == want[1].tolist()
    for other in (plain, scanned):
        assert np.array_equal(retired[0], other[0]) and np.array_equal(retired[1], other[1])


def test_run_sequencing_and_edges(G):
    """run_cycles, the settle scan, step_cycles and run_cycles again on one batch (the scans share their device
    buffers); no turn and one turn; the refusals."""
    H, W = 16, 16
    cells = np.zeros((6, H, W), np.uint8)
    cells[1] = C.place(H, W, C.BLOCK, 3, 3)
    cells[2] = C.place(H, W, C.BLINKER, 5, 4)
    cells[3] = C.place(H, W, C.GLIDER, 1, 1)
    cells[4:] = random_boards(40, 2, H, W)
    with G.Batch(6, H, W, turns_per_launch=3) as b:
        b.load(cells)
        b.step(5)
        now = np.stack([R.run(c, R.CONWAY, 5)[0] for c in cells])
        found, period, made = b.run_cycles(0, made=True)
        assert found.tolist() == [-1] * 6 and period.tolist() == [-1] * 6 and made.tolist() == [0] * 6 and b.turn == 5
        check_queries(b, now)
        want = C.scan_all(now, R.CONWAY, 1, t0=5)  # one turn finds the still lifes (and nothing else) at t0 + 1
        assert want[0].tolist()[:4] == [6, 6, -1, -1]
        assert check_run(b, 1, want, 3, t0=5).tolist() == [1] * 6
        want = C.scan_all(want[2], R.CONWAY, 20, t0=6)  # a call that starts at t0 > 0
        assert want[0].tolist()[:4] == [7, 7, 9, -1] and want[1].tolist()[:4] == [1, 1, 2, -1]
        assert check_run(b, 20, want, 3, t0=6).tolist()[:4] == [3, 3, 4, 20]
        ref = [ref_settle(c, R.CONWAY, 11) for c in want[2]]
        assert [t for t, _ in ref][:4] == [2, 2, 2, -1]
        assert b.step(11, settled=True).tolist() == [t + 26 if t >= 0 else -1 for t, _ in ref]
        check_queries(b, np.stack([s for _, s in ref]))
        want = C.scan_all(np.stack([s for _, s in ref]), R.CONWAY, 40, t0=37)
        f, p = b.step_cycles(40)
        assert f.tolist() == want[0].tolist() and p.tolist() == want[1].tolist()
        check_queries(b, want[2])
        again = C.scan_all(want[2], R.CONWAY, 40, t0=77)  # a second scan starts from its own t0: found again
        assert np.all(again[0][:3] > 77) and again[0].tolist()[:3] == [78, 78, 80]
        check_run(b, 40, again, 3, t0=77)
        # refusals leave everything alone
        L = G.lib()
        out = np.full(6, 77, np.int64)
        o = out.ctypes.data
        calls = [L.gol_batch_run_cycles(b._h, -1, o, o, o), L.gol_batch_run_cycles(b._h, 3, None, o, o),
                 L.gol_batch_run_cycles(None, 3, o, None, None)]
        assert calls == [GOL_EINVAL] * 3 and np.all(out == 77) and b.turn == 117
        check_queries(b, again[2])
        assert L.gol_batch_run_cycles(b._h, 3, o, None, None) == 0 and b.turn == 120  # (period and made may be NULL)
        assert out.tolist()[:4] == [118, 118, 120, -1]


# ---------------------------------------------------------------- the retire pass alone

LAST_MARK = {1: 1, 2: 3, 252: 507}  # period -> a found turn (relative to t0) with that period: 1 - 0, 3 - 1, 507 - 255
FILL32, FILL64 = np.int32(-0x5A5A5A5B), np.int64(-0x5A5A5A5A5A5A5A5B)  # bytes 0xA5


def retire_ref(list_in, n_in, finish, n_fin, found, left, t0, t_now, t_end):
    """The pass in plain Python, on copies: (active, its count, finish, its count, left)."""
    active, finish, left = np.full_like(list_in, FILL32), finish.copy(), left.copy()
    keep = [b for b in finish[:n_fin] if left[b] > 0]
    stay = []
    for b in list_in[:n_in]:
        if found[b] < 0:
            stay.append(b)
        else:
            d = int(found[b]) - t0
            left[b] = (t_end - t_now) % (d - C.last_mark(d))
            if left[b] > 0:
                keep.append(b)
    active[:len(stay)] = stay
    finish[:len(keep)] = keep
    return active, len(stay), finish, len(keep), left


@pytest.mark.parametrize("count", [0, 1, 63, 64, 65, 1025, 4097, 16385])  # (16385: a second tile of the pass)
@pytest.mark.parametrize("which", ["all", "none", "alternating"])
def test_retire_pass_alone(G, count, which):
    import torch
    L = G.lib()
    t0, t_now = 5, 5 + 511
    n = 2 * count + 40
    rng = np.random.default_rng(count)
    boards = rng.permutation(n).astype(np.int32)  # the list's boards, then those of the finish list, in no order
    for rest, before in [(0, 0), (1, 0), (1000, 0), (1, 20), (1000, 20)]:
        list_in = np.full(count + 8, FILL32, np.int32)
        list_in[:count] = boards[:count]
        finish = np.full(n, FILL32, np.int32)
        finish[:before] = boards[count:count + before]
        found = np.full(n, -1, np.int64)
        left = np.full(n, FILL64, np.int64)
        left[finish[:before]] = [0, 3, 0, 0, 1] * (before // 5)  # some of the finish list have nothing left
        for k, b in enumerate(list_in[:count]):
            if which == "all" or (which == "alternating" and k % 2 == 0):
                found[b] = t0 + LAST_MARK[(1, 2, 252)[k % 3]]
        want = retire_ref(list_in, count, finish, before, found, left, t0, t_now, t_now + rest)
        if count >= 63 and which != "none" and rest:  # (the reference alone) the three periods, zero and non-zero remainders
            got = {int(want[4][b]) for b in list_in[:count] if found[b] >= 0}
            assert 0 in got and rest % 2 in got and rest % 252 in got
        dev = [torch.from_numpy(a).cuda() for a in (list_in, np.array([count, before], np.int32), found,
                                                     np.full_like(list_in, FILL32), finish, left)]
        p = [t.data_ptr() for t in dev]
        rc = L.gol_dev_batch_retire(p[0], p[1], p[2], n, t0, t_now, t_now + rest, p[3], p[4], p[5], None)
        assert rc == 0, L.gol_last_error()
        torch.cuda.synchronize()
        got = [t.cpu().numpy() for t in dev]
        assert got[1].tolist() == [want[1], want[3]], (rest, before)
        assert np.array_equal(got[3], want[0]) and np.array_equal(got[4], want[2]) and np.array_equal(got[5], want[4])
        assert np.array_equal(got[0], list_in) and np.array_equal(got[2], found)
        # in place: the active list written over the list it is read from
        dev = [torch.from_numpy(a).cuda() for a in (list_in, np.array([count, before], np.int32), found, finish, left)]
        p = [t.data_ptr() for t in dev]
        assert L.gol_dev_batch_retire(p[0], p[1], p[2], n, t0, t_now, t_now + rest, p[0], p[3], p[4], None) == 0
        torch.cuda.synchronize()
        assert dev[1].cpu().numpy().tolist() == [want[1], want[3]]
        assert np.array_equal(dev[0].cpu().numpy()[:want[1]], want[0][:want[1]])
        assert np.array_equal(dev[3].cpu().numpy(), want[2]) and np.array_equal(dev[4].cpu().numpy(), want[4])


def test_retire_pass_refusals(G):
    import torch
    L = G.lib()
    t = torch.zeros(64, dtype=torch.int64, device="cuda")
    p = t.data_ptr()
    bad = [L.gol_dev_batch_retire(None, p, p, 4, 0, 1, 2, p, p, p, None), L.gol_dev_batch_retire(p, None, p, 4, 0, 1, 2, p, p, p, None),
           L.gol_dev_batch_retire(p, p, None, 4, 0, 1, 2, p, p, p, None), L.gol_dev_batch_retire(p, p, p, 4, 0, 1, 2, None, p, p, None),
           L.gol_dev_batch_retire(p, p, p, 4, 0, 1, 2, p, None, p, None), L.gol_dev_batch_retire(p, p, p, 4, 0, 1, 2, p, p, None, None),
           L.gol_dev_batch_retire(p, p, p, 0, 0, 1, 2, p, p, p, None), L.gol_dev_batch_retire(p, p, p, (1 << 20) + 1, 0, 1, 2, p, p, p, None),
           L.gol_dev_batch_retire(p, p, p, 4, 2, 1, 2, p, p, p, None), L.gol_dev_batch_retire(p, p, p, 4, 0, 3, 2, p, p, p, None),
           L.gol_dev_batch_retire(p, p, p, 4, -1, 1, 2, p, p, p, None)]
    assert bad == [GOL_EINVAL] * len(bad)
    torch.cuda.synchronize()
    assert not t.any()
