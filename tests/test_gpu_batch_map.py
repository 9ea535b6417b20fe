"""MAP rules of a batch on the GPU: batch_map_kernel<NW, SCAN, LIST, AGED> (csrc/gol_batch_map.hip) one launch at a
time through gol_dev_batch_step_map against tests/map_ref.py (nine np.rolls and a table lookup, written from
include/golhip.h), bit for bit, every buffer of a launch between two margins of sentinel bytes and compared whole,
the maps included; then golhip.Batch under maps: differential against the life-like kernels for 18 rules, an
analytic period, the retiring call, and a soup search and census under a map that is not totalistic."""
import numpy as np
import pytest

import batch_ref as B
import cycle_ref as C
import island_ref as I
import map_ref as M
import rule_ref as R
import tally_ref as T
from testlib import GOL_EINVAL, GOL_ESTATE, Guarded, error_word, gpu_lib as G  # noqa: F401 (the fixture)

pytestmark = pytest.mark.gpu

NAMES = ("boards", "prev", "settled", "maps", "list", "count", "left", "born")


def _buffers(host):
    return {k: Guarded(v, name=k) for k, v in host.items() if v is not None}


def _launch(G, buf, *, n, H, W, turns, turn0=0, have_prev=0, write_prev=0, map_each=0, scan=0, done=0, slots=0):
    import torch
    p = {k: (buf[k].ptr if k in buf else None) for k in NAMES}
    rc = G.lib().gol_dev_batch_step_map(p["boards"], p["prev"], p["settled"], n, H, W, turns, turn0, int(have_prev), int(write_prev),
                                        p["maps"], int(map_each), scan, done, p["list"], p["count"], slots, p["left"], p["born"],
                                        torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return rc


def _compare(buf, host, want, where):
    """Every buffer whole (margins included) against `want` (a name not in it, or None: unchanged, as in `host`)."""
    for name, g in buf.items():
        g.expect(host[name] if want.get(name) is None else want[name], (where, name))


# ---------------------------------------------------------------- one plain launch at every width and height class

@pytest.mark.parametrize("case", M.cases(), ids=lambda c: c[0])
def test_one_launch(G, case):
    cid, H, W, turns, kind = case
    n = M.N_BOARDS
    cells = B.random_boards(H + 3 * W, n, H, W)
    maps, each = M.case_maps(kind, 7 * H + W)
    host = dict(boards=B.pack(cells), maps=maps)
    buf = _buffers(host)
    assert _launch(G, buf, n=n, H=H, W=W, turns=turns, map_each=each) == 0, G.lib().gol_last_error()
    if kind.startswith("P"):  # a pure translation
        dy, dx = M.projection_roll(int(kind[1:]))
        want = np.roll(cells, (turns * dy, turns * dx), (1, 2))
    else:
        want = np.stack([M.run(cells[b], maps[b] if each else maps, turns) for b in range(n)])
    _compare(buf, host, {"boards": B.pack(want)}, cid)
    assert error_word(G) == (0, 0)


# ---------------------------------------------------------------- every mode at 65 x 33 and 129 x 65

def _mode_maps(n, seed):
    """A map per board: B3/S23 as a map where the scans are to find something (blocks, a blinker), a random map with
    birth on empty ground, and a projection (a translation: found only after a whole trip round the torus)."""
    life = M.from_rule(*R.CONWAY)
    return np.stack([life, life, M.random_map(seed, zero_bit=1), life, M.projection(5)][:n])


@pytest.mark.parametrize("H,W", [(65, 33), (129, 65)])
def test_modes(G, H, W):
    n, Ww = 5, (W + 63) // 64
    cells = B._compose(n, H, W, 100 + H)  # a glider, blocks, a soup, a blinker, blocks
    maps = _mode_maps(n, H)
    gap = np.full((n, H, Ww), B.GAP, np.uint64)
    model = dict(H=H, W=W, maps=maps, map_each=True)

    def chain(scan, launches, where):
        """Launches of one scanning call on the same buffers, each against the model."""
        host = dict(boards=B.pack(cells), prev=gap.copy(), settled=np.full(n, -1, np.int64), maps=maps)
        buf = _buffers(host)
        state = {k: v.copy() for k, v in host.items()}
        for turns, turn0, hp, wp, done in launches:
            assert _launch(G, buf, n=n, H=H, W=W, turns=turns, turn0=turn0, have_prev=hp, write_prev=wp, map_each=1, scan=scan,
                           done=done) == 0, G.lib().gol_last_error()
            w = M.launch_model(state["boards"], state["prev"], state["settled"], None, turns=turns, turn0=turn0, have_prev=hp,
                               write_prev=wp, scan=scan, done=done, **model)
            state.update(boards=w["boards"], prev=w["prev"], settled=w["settled"])
            _compare(buf, host, state, (where, turn0))
        return state

    # settle: without and with the state before the launch; blocks and the blinker settle at turn0 + 2
    s = chain(M.SCAN_SETTLE, [(4, 10, False, True, 0), (3, 14, True, False, 0)], "settle")
    assert s["settled"].tolist() == [-1, 12, -1, 12, -1]
    s = chain(M.SCAN_SETTLE, [(1, 10, False, True, 0), (1, 11, True, True, 0), (1, 12, True, False, 0)], "settle by single turns")
    assert s["settled"].tolist() == [-1, 12, -1, 12, -1]
    # cycles: the first launch ends on the mark 1, the second crosses the marks 3 and 7
    s = chain(M.SCAN_CYCLES, [(2, 20, False, True, 0), (6, 22, True, True, 2)], "cycles")
    assert s["settled"].tolist() == [-1, 21, -1, 23, -1]
    want = [M.scan(cells[b], maps[b], 8, 20)[0] for b in range(n)]
    assert s["settled"].tolist() == want

    # list + cycles: a shuffled subset, *count below, at and zero of the slots
    order = np.array([3, 0, 4, 1], np.int32)  # all but board 2
    for slots, count in ((5, 4), (4, 4), (4, 0)):
        lst = np.full(slots, B.FILL32, np.int32)
        lst[:4] = order
        host = dict(boards=B.pack(cells), prev=gap.copy(), settled=np.full(n, -1, np.int64), maps=maps, list=lst,
                    count=np.array([count], np.int32))
        buf = _buffers(host)
        assert _launch(G, buf, n=n, H=H, W=W, turns=4, turn0=30, write_prev=1, map_each=1, scan=M.SCAN_CYCLES, slots=slots) == 0
        w = M.launch_model(host["boards"], host["prev"], host["settled"], None, turns=4, turn0=30, write_prev=True,
                           scan=M.SCAN_CYCLES, list=lst, count=count, **model)
        _compare(buf, host, w, ("list", slots, count))
        assert w["settled"].tolist() == ([-1, 31, -1, 33, -1] if count else [-1] * 5)

    # the finish: turns left of 0, below, at and above the launch's turns
    turns = 4
    left = np.full(n, B.FILL64, np.int64)
    left[order] = [0, turns - 2, turns, turns + 5]
    host = dict(boards=B.pack(cells), maps=maps, list=order, count=np.array([4], np.int32), left=left)
    buf = _buffers(host)
    assert _launch(G, buf, n=n, H=H, W=W, turns=turns, turn0=40, map_each=1, slots=4) == 0, G.lib().gol_last_error()
    w = M.launch_model(host["boards"], None, None, left, turns=turns, turn0=40, list=order, count=4, **model)
    _compare(buf, host, w, "finish")
    assert w["left"][order].tolist() == [0, 0, 0, 5] and w["left"][2] == B.FILL64

    # aged, one map: ages 2 (across the mark 3), 0 (its first launch: prev is not read), 5 and 1 at done = 6
    life = maps[0]
    one = dict(H=H, W=W, maps=life, map_each=False)
    ages = {3: 2, 0: 0, 4: 5, 1: 1}
    boards, prev, settled, born = B.pack(cells), gap.copy(), np.full(n, -1, np.int64), np.full(n, B.FILL64, np.int64)
    for b, a in ages.items():
        born[b] = 6 - a
        if a > 0:  # the slot's soup at its age: the model's own scan of it from age 0
            pre = M.launch_model(boards[b:b + 1], prev[b:b + 1], np.array([-1], np.int64), None, turns=a, write_prev=True,
                                 scan=M.SCAN_CYCLES, list=[0], count=1, born=np.zeros(1, np.int64), **one)
            boards[b], prev[b], settled[b] = pre["boards"][0], pre["prev"][0], pre["settled"][0]
    host = dict(boards=boards, prev=prev, settled=settled, maps=life, list=order, count=np.array([4], np.int32), born=born)
    buf = _buffers(host)
    assert _launch(G, buf, n=n, H=H, W=W, turns=4, have_prev=1, write_prev=1, scan=M.SCAN_CYCLES, done=6, slots=4) == 0
    w = M.launch_model(boards, prev, settled, None, turns=4, have_prev=True, write_prev=True, scan=M.SCAN_CYCLES, done=6, list=order,
                       count=4, born=born, **one)
    _compare(buf, host, w, "aged")
    assert w["settled"].tolist() == [-1, 1, -1, 3, 1]  # in the boards' own ages; a found board keeps s(found) in prev
    assert np.array_equal(w["prev"][3], B.pack(M.run(cells[3], life, 3)))
    assert error_word(G) == (0, 0)


# ---------------------------------------------------------------- golhip.Batch under maps

def test_batch_under_maps_equals_batch_under_rules(G):
    """The 18 rules of the survey tests, a board each: map_from_rule(r) against set_rule(r) on the existing kernels,
    per board and as one map for the batch."""
    H, W, n = 33, 70, len(C.RULES)
    cells = B.random_boards(5, n, H, W)
    maps = np.stack([G.map_from_rule(r) for r in C.RULES])
    assert all(np.array_equal(maps[i], M.from_rule(*R.masks(r))) for i, r in enumerate(C.RULES))
    out = {}
    for kind in ("rules", "maps"):
        with G.Batch(n, H, W, turns_per_launch=7) as b:
            if kind == "rules":
                b.set_rules(C.RULES)
            else:
                b.set_maps(maps)
                assert np.array_equal(b.maps(), maps)
            b.load(cells)
            b.step(5)
            a = b.store_words()
            settled = b.step(9, settled=True)
            found, period = b.step_cycles(40)
            c = b.store_words()
            b.load(cells)
            out[kind] = (a, settled, found, period, c, b.run_cycles(54), b.store_words(), b.turn)
    for x, y in zip(out["rules"], out["maps"]):
        assert np.array_equal(np.asarray(x), np.asarray(y))
    assert np.array_equal(B.unpack(out["maps"][0], W), np.stack([R.run(cells[i], r, 5)[0] for i, r in enumerate(C.RULES)]))
    for r in C.RULES:  # one map for the batch against one rule (the 7-gate kernel for B3/S23, else the table kernel)
        res = []
        for rule in (r, G.format_map(G.map_from_rule(r))):
            with G.Batch(3, H, W, rule=rule, turns_per_launch=5) as b:
                b.load(cells[:3])
                res.append((b.step_cycles(12), b.store_words()))
        assert np.array_equal(res[0][1], res[1][1]) and np.array_equal(res[0][0], res[1][0]), r


def test_a_cell_under_the_nw_projection(G):
    """One cell on a 7 x 9 torus under P_8 moves one row down and one column right per turn: period lcm(7, 9) = 63, and
    by the marks 0, 1, 3, ..., 63, 127 it is found at 126, the first turn one period after a mark."""
    cells = np.zeros((1, 7, 9), np.uint8)
    cells[0, 2, 3] = 1
    with G.Batch(1, 7, 9, turns_per_launch=50) as b:
        b.set_map(M.projection(8))
        b.load(cells)
        found, period = b.step_cycles(130)
        assert (found.tolist(), period.tolist()) == ([126], [63])
        assert np.array_equal(b.store()[0] != 0, np.roll(cells[0], (130, 130), (0, 1)) != 0)


def test_run_cycles_is_step_cycles_under_mixed_maps(G):
    H = W = 17
    pats = [(C.BLOCK, 3, 3), (C.BLINKER, 5, 4), (C.PULSAR, 2, 2), (C.GLIDER, 1, 1), None, ([], 0, 0), (C.BLINKER, 9, 8),
            (C.BLOCK, 7, 9), (C.PULSAR, 2, 1)]
    cells = np.stack([R.random_board(77, H, W, 0.3) if p is None else C.place(H, W, *p) for p in pats])
    n = len(cells)
    life, b38 = M.from_rule(*R.CONWAY), M.from_rule(*R.masks("B38/S23"))
    maps = np.stack([life, b38, b38, M.projection(7), M.random_map(9, zero_bit=0), M.random_map(10, zero_bit=1), life,
                     M.projection(3), life])
    want = [M.scan(cells[i], maps[i], 60, 0) for i in range(n)]
    res = []
    for call in ("step_cycles", "run_cycles"):
        with G.Batch(n, H, W, turns_per_launch=7) as b:
            b.set_maps(maps)
            b.load(cells)
            found, period = getattr(b, call)(60)
            res.append((found, period, b.store_words(), b.turn))
    for x, y in zip(*res):
        assert np.array_equal(np.asarray(x), np.asarray(y))
    assert res[1][0].tolist() == [w[0] for w in want] and res[1][1].tolist() == [w[1] for w in want]
    assert np.array_equal(B.unpack(res[1][2], W), np.stack([w[2] for w in want]))
    assert {1, 3, 6, -1} <= set(res[1][0].tolist()) and 17 in res[1][1].tolist()  # still, period 2, 3, never; a trip round


def not_totalistic():
    """B3/S23 with every birth entry whose N cell is alive cleared: no birth below an alive cell.  The reference alone
    finds all 24 soups of 16 x 16 (seed 1) within 400 turns under it (asserted below: at least 3/4), most as still
    lifes of a few cells."""
    t = M.bits(M.from_rule(*R.CONWAY)).copy()
    for i in range(512):
        if not i & 16 and i & 128:
            t[i] = 0
    m = M.from_bits(t)
    life = R.masks("B3/S23")
    assert not any(np.array_equal(m, M.from_rule(bm, sm)) for bm in (life[0], 0) for sm in (life[1], 0))
    return m


def test_search_and_census_under_a_map_that_is_not_totalistic(G):
    seed, total, side, horizon = 1, 24, 16, 400
    m = not_totalistic()
    found, period, alive, hashes, states = M.search(seed, 0, total, side, side, m, horizon)
    assert np.count_nonzero(found >= 0) >= 3 * total // 4 and alive.any()
    pairs, islands, fps = [], np.zeros(total, np.int64), np.zeros(total, np.uint64)
    for g, s in states.items():
        recs, fp = I.census(s, 1)
        islands[g], fps[g] = len(recs), fp
        pairs += [(g, r) for r in recs]
    kinds = T.tally(pairs)
    for slots, tpl in ((5, 7), (24, 32)):
        with G.Batch(slots, side, side, rule=G.format_map(m), turns_per_launch=tpl) as b:
            got = b.search(seed, total, horizon)
            for x, y in zip(got, (found, period, alive, hashes)):
                assert np.array_equal(x, y), (slots, tpl)
            c = b.census(seed, total, horizon, reach=1)
            for k, w in dict(found=found, period=period, alive=alive, hash=hashes, islands=islands, fingerprint=fps).items():
                assert np.array_equal(c[k], w), (slots, tpl, k)
            assert c["n_kinds"] == len(kinds) and np.array_equal(c["kinds"], kinds.astype(G.ISLAND_KIND_DTYPE))
            assert np.array_equal(b.maps(0, 1)[0], m)  # the map stays


def test_refusals(G):
    n, H, W = 5, 5, 17
    boards = B.pack(B.random_boards(1, n, H, W))
    host = dict(boards=boards, prev=np.full_like(boards, B.GAP), settled=np.full(n, -1, np.int64), maps=np.stack([M.random_map(i) for i in range(n)]),
                list=np.arange(n, dtype=np.int32), count=np.array([n], np.int32), left=np.full(n, 2, np.int64), born=np.zeros(n, np.int64))
    buf = _buffers(host)
    plain = {k: buf[k] for k in ("boards", "maps")}
    aged = {k: buf[k] for k in ("boards", "prev", "settled", "maps", "list", "count", "born")}
    assert _launch(G, {"boards": buf["boards"]}, n=n, H=H, W=W, turns=3) == GOL_EINVAL  # no maps
    assert _launch(G, plain, n=n, H=H, W=W, turns=0) == GOL_EINVAL
    assert _launch(G, plain, n=n, H=513, W=W, turns=3) == GOL_EINVAL
    assert _launch(G, plain, n=n, H=H, W=W, turns=3, scan=1) == GOL_EINVAL
    assert _launch(G, aged, n=n, H=H, W=W, turns=3, write_prev=1, map_each=1, scan=2, slots=n) == GOL_EINVAL  # a map per soup
    _compare(buf, host, {}, "refusals")
    with G.Batch(3, 8, 8) as b:
        b.set_maps(np.stack([M.random_map(i) for i in range(3)]))
        for call in (lambda: b.rule, lambda: b.rules(), lambda: b.search(1, 4, 10), lambda: b.census(1, 4, 10)):
            with pytest.raises(G.GolError) as ei:
                call()
            assert ei.value.code == GOL_ESTATE
        b.set_map(M.random_map(1))
        with pytest.raises(G.GolError) as ei:
            b.rule
        assert ei.value.code == GOL_ESTATE
        b.set_rule("B36/S23")  # a rule clears the maps, and the reverse
        assert b.rule == "B36/S23" and np.array_equal(b.maps(0, 1)[0], M.from_rule(*R.masks("B36/S23")))
        b.set_rules(["B3/S23"], first=1)
        b.set_map("B2/S")
        assert np.array_equal(b.maps(), np.stack([M.from_rule(*R.masks("B2/S"))] * 3))
        for bad in (np.zeros((2, 15), np.uint32), np.zeros((2, 16), np.int64)):
            with pytest.raises(G.GolError) as ei:
                b.set_maps(bad)
            assert ei.value.code == GOL_EINVAL
        with pytest.raises(G.GolError) as ei:
            b.set_maps(np.zeros((2, 16), np.uint32), first=2)
        assert ei.value.code == GOL_EINVAL
    assert error_word(G) == (0, 0)
