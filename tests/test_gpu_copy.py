"""Region reads on the GPU (gol_engine_copy / gol_engine_bounds / gol_broker_copy / _bounds, and
Engine.to_rle on top of them): a rectangle read from the running board in the layout it is stepped
in.  Every comparison is exact, against numpy on the oracle's board (O.random_words / O.bits_run /
O.unpack, tests/rule_ref.py for other rules): the cells, the alive counts, the boxes, the board after
a cut, and the boards that stepping makes of them."""
import ctypes
import json
import os
import subprocess
import sys
import threading
import time

import numpy as np
import pytest

import rule_ref as R
from oracle import oracle as O
from region_ref import BYTE_EDITS, SEED, apply_cuts, check_reads, np_box, np_paste, np_region, random_cells, words_of
from testlib import gpu_lib as G  # noqa: F401 (the fixture)

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORKER = os.path.join(ROOT, "tests", "_copy_rank_worker.py")
GUN = ("x = 36, y = 9, rule = B3/S23\n24bo$22bobo$12b2o6b2o12b2o$11bo3bo4b2o12b2o$2o8bo5bo3b2o$2o8bo3bob2o4bobo$"
       "10bo5bo7bo$11bo3bo$12b2o!\n")  # Gosper's glider gun


# ---------------------------------------------------------------- band, in place
BAND_RECTS = {
    (96, 1024): [(1000, 90, 50, 12), (5, 0, 36, 12), (300, 84, 33, 12), (1023, 40, 1, 1), (17, 20, 32, 5), (10, 50, 1024, 3),
                 (700, 94, 400, 4)],                                  # (the rectangles of test_band_paste_in_place)
    (64, 2048): [(2000, 60, 100, 9), (3, 0, 100, 12), (0, 52, 2048, 12)],
    (48, 3072): [(3000, 40, 200, 9), (95, 0, 97, 4), (0, 10, 3072, 2)],  # Wd = 96: an odd number of 32-cell groups
}


@pytest.mark.parametrize("H,W", sorted(BAND_RECTS))
def test_band_copy_in_place(G, H, W):
    cells = random_cells(H, W, 24)
    with G.Engine(H, W, layout="band", device=0) as e:
        e.load_random(SEED)
        e.step(24)
        check_reads(e, cells, BAND_RECTS[(H, W)] + [(0, 0, W, H)], "band")
        assert e.turn == 24 and e.info()["layout"] == "band" and e.info()["bit_mode"]  # nothing was converted
        assert e.alive_count() == np.count_nonzero(cells) == e.bounds()[4]
        assert e.hash() == O.hash_words(words_of(cells))
        e.step(12)
        assert e.turn == 36 and e.hash() == O.hash_words(O.bits_run(words_of(cells), 12))


def test_caller_buffer_contract(G):
    """A caller's buffer of ones with stride > ceil(w / 64): the words past ceil(w / 64) stay, the tail
    bits of the last word are zero; NULL alive / src_layout are fine."""
    H, W = 96, 1024
    cells = random_cells(H, W, 24)
    with G.Engine(H, W, layout="band", device=0) as e:
        e.load_random(SEED)
        e.step(24)
        for x0, y0, w, h in [(1000, 90, 50, 12), (10, 50, 1024, 3), (95, 3, 65, 4)]:
            pw = (w + 63) // 64
            buf = np.full((h, pw + 2), 2 ** 64 - 1, np.uint64)
            assert G.lib().gol_engine_copy(e._h, x0, y0, w, h, buf.ctypes.data, pw + 2, 0, None, None) == 0
            assert (buf[:, pw:] == np.uint64(2 ** 64 - 1)).all()
            bits = np.unpackbits(np.ascontiguousarray(buf[:, :pw]).view(np.uint8), axis=1, bitorder="little")
            assert np.array_equal(bits[:, :w] != 0, np_region(cells, x0, y0, w, h)) and not bits[:, w:].any()


# ---------------------------------------------------------------- standard bit rows
STANDARD_RECTS = [(37, 95, 192, 10), (1, 3, 31, 4), (191, 50, 3, 3), (64, 0, 64, 12), (31, 0, 192, 100), (95, 98, 97, 4)]


def test_standard_copy(G):
    H, W = 100, 192
    cells = random_cells(H, W, 9)
    with G.Engine(H, W, layout="standard", device=0) as e:
        e.load_random(SEED)
        e.step(9)
        check_reads(e, cells, STANDARD_RECTS, "standard")
        assert e.turn == 9 and e.info()["layout"] == "standard"
        e.step(8)
        assert e.hash() == O.hash_words(O.bits_run(words_of(cells), 8))


# ---------------------------------------------------------------- byte rows
def byte_rects(W):
    return [(x0 % W, y0, min(w, W), h) for x0, y0, w, h, _, _ in BYTE_EDITS]


@pytest.mark.parametrize("H,W", [(50, 100), (50, 50)])  # aligned 4-byte words in the bounds (W % 4 == 0); one byte per lane
def test_bytes_copy_odd_width(G, H, W):
    rng = np.random.default_rng(5)
    start = (rng.random((H, W)) < 0.4).astype(np.uint8) * 255
    board = O.run(start, 5)
    with G.Engine(H, W, device=0) as e:
        e.load_bytes(start)
        e.step(5)
        check_reads(e, board != 0, byte_rects(W) + [(0, 0, W, H), (W - 1, H - 1, W, H)], "bytes")
        assert e.turn == 5 and np.array_equal(e.store_bytes(), board)
        e.step(5)
        assert np.array_equal(e.store_bytes(), O.run(board, 5))


def test_bytes_copy_bytes_layout(G):
    H, W = 64, 128
    cells = random_cells(H, W, 33)
    with G.Engine(H, W, layout="bytes", device=0) as e:
        e.load_random(SEED)
        e.step(33)
        check_reads(e, cells, byte_rects(W) + [(1, 60, 128, 8)], "bytes")
        e.step(40)
        assert np.array_equal(e.store_bytes(), O.unpack(O.bits_run(words_of(cells), 40)))


def test_bytes_copy_counts_any_non_zero_byte(G):
    """A byte board loaded with bytes in {0, 7, 255}, before its first turn: alive = non-zero."""
    H, W = 50, 100
    board = np.random.default_rng(6).choice(np.array([0, 7, 255], dtype=np.uint8), size=(H, W))
    with G.Engine(H, W, device=0) as e:
        e.load_bytes(board)
        check_reads(e, board != 0, byte_rects(W), "bytes")
        assert e.turn == 0 and np.array_equal(e.store_bytes(), board)
        e.step(3)
        assert np.array_equal(e.store_bytes(), O.run(board, 3))


def test_exact_first_turn_pending(G):
    """A bit-capable board still holding its loaded bytes (one of them 7): copy and bounds read byte
    rows, a cut is GOL_ESTATE and changes nothing."""
    rng = np.random.default_rng(7)
    board = (rng.random((64, 64)) < 0.4).astype(np.uint8) * 255
    board[10, 10] = 7
    with G.Engine(64, 64, device=0) as e:
        e.load_bytes(board)
        check_reads(e, board != 0, [(5, 5, 10, 10), (60, 60, 9, 9), (0, 0, 64, 64)], "bytes")
        with pytest.raises(G.GolError) as ei:
            e.cut(5, 5, 10, 10)
        assert ei.value.code == G._lib.GOL_ESTATE
        assert np.array_equal(e.store_bytes(), board) and e.turn == 0
        e.step(1)
        after = O.run(board, 1)
        got, lay = e.cut(8, 8, 5, 5, return_layout=True)  # a bit board now
        assert lay != "bytes" and np.array_equal(got, after[8:13, 8:13] != 0)
        after[8:13, 8:13] = 0
        assert np.array_equal(e.store_bytes(), after)


# ---------------------------------------------------------------- cut
def test_band_cut(G):
    H, W = 96, 1024
    cells = random_cells(H, W, 24)
    with G.Engine(H, W, layout="band", device=0) as e:
        e.load_random(SEED)
        e.step(24)
        cells = apply_cuts(e, cells, BAND_RECTS[(H, W)][:5], "band")
        assert e.turn == 24 and np.array_equal(e.view(0, 0, 1, W, H) != 0, cells)
        e.step(12)
        assert e.hash() == O.hash_words(O.bits_run(words_of(cells), 12))


def test_standard_and_bytes_cut(G):
    cells = random_cells(100, 192, 9)
    with G.Engine(100, 192, layout="standard", device=0) as e:
        e.load_random(SEED)
        e.step(9)
        cells = apply_cuts(e, cells, STANDARD_RECTS[:4], "standard")
        assert np.array_equal(e.view(0, 0, 1, 192, 100) != 0, cells)
        e.step(8)
        assert e.hash() == O.hash_words(O.bits_run(words_of(cells), 8))
    for H, W in [(50, 100), (50, 50)]:
        start = (np.random.default_rng(5).random((H, W)) < 0.4).astype(np.uint8) * 255
        with G.Engine(H, W, device=0) as e:
            e.load_bytes(start)
            e.step(5)
            cells = apply_cuts(e, O.run(start, 5) != 0, byte_rects(W)[:4], "bytes")
            board = cells.astype(np.uint8) * 255
            assert np.array_equal(e.store_bytes(), board)
            e.step(5)
            assert np.array_equal(e.store_bytes(), O.run(board, 5))


@pytest.mark.parametrize("shards", [2, 3])
def test_cut_invalidates_the_halo(G, shards):
    H, W = 96, 1024
    cells = random_cells(H, W, 12)
    with G.Engine(H, W, shards=shards, same_device=True, transport="loopback", device=0) as e:
        e.load_random(SEED)
        e.step(12)  # a halo has been issued for the next step
        rects = [(100, 28, 200, 40),   # rows 28..67: across the boundaries 32, 48 and 64
                 (1000, 90, 60, 12)]   # rows 90..95 and 0..5: the last shard and the first
        check_reads(e, cells, rects + [(0, 0, W, H)], "band")  # every shard's runs, unioned
        cells = apply_cuts(e, cells, rects, "band")
        e.step(24)
        assert e.hash() == O.hash_words(O.bits_run(words_of(cells), 24))


def test_cut_and_paste_move_a_region(G):
    H, W = 96, 1024
    cells = random_cells(H, W, 24)
    with G.Engine(H, W, layout="band", device=0) as e:
        e.load_random(SEED)
        e.step(24)
        words, alive = e.copy_words(990, 88, 70, 20, cut=True)
        region = np_region(cells, 990, 88, 70, 20)
        cells, _, _ = np_paste(cells, 990, 88, np.ones((20, 70), bool), "andnot")
        cells, changed, _ = np_paste(cells, 300, 40, region, "copy")
        assert e.paste_words(words, 70, 300, 40) == changed and alive == np.count_nonzero(region)
        assert np.array_equal(e.view(0, 0, 1, W, H) != 0, cells)
        assert np.array_equal(e.copy(300, 40, 70, 20), region)
        e.step(12)
        assert e.hash() == O.hash_words(O.bits_run(words_of(cells), 12))


# ---------------------------------------------------------------- bounds
LAYOUT_BOARDS = [("band", 96, 1024, dict(layout="band")), ("standard", 100, 192, dict(layout="standard")),
                 ("bytes", 50, 100, {}), ("bytes", 50, 50, {}), ("bytes", 64, 128, dict(layout="bytes"))]


@pytest.mark.parametrize("layout,H,W,kw", LAYOUT_BOARDS)
def test_bounds(G, layout, H, W, kw):
    """A dead board stepped once (so it is in its stepping layout); then, pasted into it, single cells
    at the four corners of a rectangle that wraps both seams, and a sparse random board."""
    rng = np.random.default_rng(H + W)
    w, h = W // 2 + 7, H // 2 + 3
    x0, y0 = W - 20, H - 9
    with G.Engine(H, W, device=0, **kw) as e:
        e.load_bytes(np.zeros((H, W), np.uint8))
        e.step(1)
        assert e.bounds() == (0, 0, 0, 0, 0) and e.bounds(x0, y0, w, h) == (0, 0, 0, 0, 0)
        assert e.copy(0, 0, 1, 1, return_layout=True)[1] == layout
        corners = [(0, 0), (w - 1, 0), (0, h - 1), (w - 1, h - 1)]
        cells = np.zeros((H, W), bool)
        for c, r in corners:  # one at a time, then all four
            one = np.zeros((H, W), bool)
            one[(y0 + r) % H, (x0 + c) % W] = True
            e.paste(one, 0, 0)
            assert e.bounds(x0, y0, w, h) == (c, r, 1, 1, 1) and e.bounds() == np_box(one)
            cells |= one
        e.paste(cells, 0, 0)
        assert e.bounds(x0, y0, w, h) == (0, 0, w, h, 4)
        assert e.bounds(x0 + 1, y0, w - 2, h) == (0, 0, 0, 0, 0)  # between the corner columns
        cells = rng.random((H, W)) < 1 / 200
        e.paste(cells, 0, 0)
        assert e.bounds() == np_box(cells) and e.bounds()[4] == e.alive_count() > 0
        rects = [(x0, y0, w, h), (3, 5, W // 3, H // 3), (W - 1, H - 1, W, H), (0, 0, W, 1), (W // 2, 0, 1, H),
                 (1, 1, W - 1, H - 1)]
        check_reads(e, cells, rects, layout)
        assert e.turn == 1


# ---------------------------------------------------------------- ranks
def run_copy_ranks(G, nranks, H, W, turns, rects, cuts, more):
    uid = G.engine.unique_id("ipc").hex()
    procs = []
    for r in range(nranks):  # a fresh child per rank: nranks GPU processes beside this one
        a = dict(uid=uid, H=H, W=W, nranks=nranks, rank=r, seed=SEED, turns=turns, rects=rects, cuts=cuts, more=more)
        procs.append(subprocess.Popen([sys.executable, WORKER, json.dumps(a)], stdout=subprocess.PIPE,
                                      stderr=subprocess.PIPE, text=True,
                                      env=dict(os.environ, GOL_IPC_TIMEOUT_MS="30000")))
    res, errs = {}, []
    try:
        for p in procs:
            out, err = p.communicate(timeout=120)
            lines = [ln for ln in out.splitlines() if ln.startswith("{")]
            if p.returncode != 0 or not lines:
                errs.append(f"rc {p.returncode}: {err[-3000:]}")
                break
            d = json.loads(lines[-1])
            res[d["rank"]] = d
    finally:
        for q in procs:  # on the first failure (or a timeout) the others go too
            if q.poll() is None:
                q.kill()
                q.communicate()
    assert not errs, "\n".join(errs)
    return res


def test_ranks_read_their_rows(G):
    """Two IPC rank processes (rows 0..31 and 32..63): each returns its own rows of a rectangle, the
    others zero, and the box of its own cells in rectangle coordinates; the OR of the patterns and
    the union of the boxes are numpy's.  A cut by the holders only, then a collective step."""
    H, W = 64, 1024
    rects = [[1000, 25, 60, 14], [10, 60, 40, 8], [500, 40, 33, 5], [0, 0, 1024, 64]]
    cuts = [[1000, 25, 60, 14], [500, 40, 33, 5]]
    cells = random_cells(H, W, 12)
    res = run_copy_ranks(G, 2, H, W, 12, rects, cuts, 24)
    parts = [O.partition(H, 2, r) for r in range(2)]
    for i, (x0, y0, w, h) in enumerate(rects):
        want = np_region(cells, x0, y0, w, h)
        total, boxes = np.zeros((h, w), bool), []
        for r in range(2):
            c = res[r]["copies"][i]
            got = np.unpackbits(np.array(c["words"], np.uint64).view(np.uint8), axis=1, bitorder="little")[:, :w] != 0
            mine = np.array([parts[r][0] <= (y0 + j) % H < parts[r][1] for j in range(h)])
            assert np.array_equal(got, want & mine[:, None]), (i, r)
            assert c["alive"] == np.count_nonzero(got) and c["layout"] == "band"
            assert tuple(c["bounds"]) == np_box(got), (i, r)
            total |= got
            boxes.append(c["bounds"])
        assert np.array_equal(total, want)
        live = [b for b in boxes if b[4]]
        bx, by = min(b[0] for b in live), min(b[1] for b in live)
        union = (bx, by, max(b[0] + b[2] for b in live) - bx, max(b[1] + b[3] for b in live) - by, sum(b[4] for b in live))
        assert union == np_box(want), i
    for i, (x0, y0, w, h) in enumerate(cuts):
        cells, cleared, _ = np_paste(cells, x0, y0, np.ones((h, w), bool), "andnot")
        assert sum(res[r]["cuts"][i] or 0 for r in range(2)) == cleared
    assert res[0]["cuts"][1] is None and None not in res[1]["cuts"]  # rows 40..44 are rank 1's alone
    for r in range(2):
        assert (res[r]["y0"], res[r]["y1"]) == parts[r] and res[r]["turn"] == 12
        assert res[r]["hash"] == O.hash_words(O.bits_run(words_of(cells), 24))


# ---------------------------------------------------------------- RLE out
def test_to_rle_round_trips_a_glider_gun(G):
    H, W = 96, 1024
    with G.Engine(H, W, layout="band", device=0) as e:
        gun = G.parse_rle(GUN)[0]
        e.load_bytes(np.zeros((H, W), np.uint8))
        e.step(1)
        assert e.to_rle() == "x = 1, y = 1, rule = B3/S23\n!\n"  # nothing alive: the 1 x 1 dead pattern
        assert not G.parse_rle(e.to_rle(5, 5, 20, 20))[0].any() and G.parse_rle(e.to_rle())[0].shape == (1, 1)
        assert e.paste(GUN, 500, 40) == gun.sum() == 36
        assert e.bounds() == (500, 40, 36, 9, 36)
        back, rule = G.parse_rle(e.to_rle())
        assert np.array_equal(back, gun) and rule == "B3/S23" and e.to_rle().startswith(GUN[:29])
        assert G.parse_rle(e.to_rle(490, 38, 100, 20, trim=False))[0].shape == (20, 100)
        e.fill(500, 40, 36, 9, "andnot")
        e.paste(GUN, 1000, 90)  # across both seams: its box relative to a rectangle that holds it
        assert e.bounds(990, 85, 100, 20) == (10, 5, 36, 9, 36)
        assert np.array_equal(G.parse_rle(e.to_rle(990, 85, 100, 20))[0], gun)
        assert e.turn == 1 and e.info()["layout"] == "band"
    with G.Engine(H, W, rule="B36/S23", device=0) as e:
        e.load_bytes(np.zeros((H, W), np.uint8))
        e.paste(GUN, 3, 3)
        text = e.to_rle()
        assert text.startswith("x = 36, y = 9, rule = B36/S23\n")
        assert np.array_equal(G.parse_rle(text)[0], gun) and G.parse_rle(text)[1] == "B36/S23"
        e.step(4)
        want = R.run(np.pad(gun, ((3, H - 12), (3, W - 39))).astype(np.uint8) * 255, "B36/S23", 4)[0]
        bx, by, bw, bh, n = e.bounds()
        assert n == want.sum() and np.array_equal(G.parse_rle(e.to_rle())[0], want[by:by + bh, bx:bx + bw] != 0)


# ---------------------------------------------------------------- broker
def test_broker_reads_during_a_run(G):
    """A Run paused at turn 0, resumed and paused again one or more chunks later: copy and bounds
    return the board of the turn they report, and a cut lands after it."""
    H, W, N = 64, 1024, 6000
    rng = np.random.default_rng(8)
    start = (rng.random((H, W)) < 0.35).astype(np.uint8) * 255
    ops = G.Operations(device=0)
    size = G.Request(ImageHeight=H, ImageWidth=W)
    for call in (lambda: ops.copy(0, 0, 8, 8), lambda: ops.bounds(0, 0, 8, 8)):
        with pytest.raises(G.GolError) as ei:
            call()
        assert ei.value.code == G._lib.GOL_ESTATE  # no board yet
    ops.Pause()
    out = {}
    th = threading.Thread(target=lambda: out.update(res=ops.Run(
        G.Request(World=start, Turns=N, ImageHeight=H, ImageWidth=W, Threads=4))))
    th.start()
    done = False
    try:
        deadline = time.time() + 60

        def state():
            try:
                return ops.RetrieveCurrentData(size, alive=False, world=False).TurnsCompleted, ops.paused
            except G.GolError as x:  # the Run thread has not loaded its board yet
                assert x.code == G._lib.GOL_ESTATE
                return 0, False
        while state() != (0, True):
            assert time.time() < deadline
        got0, t0 = ops.copy(1000, 55, 70, 20)
        ops.Pause()  # resume ...
        ops.Pause()  # ... and pause again after the chunk
        while th.is_alive() and not (state()[0] > 0 and state()[1]):
            assert time.time() < deadline
        got, t = ops.copy(1000, 55, 70, 20)
        box, t2 = ops.bounds(1000, 55, 70, 20)
        whole, t3 = ops.bounds(0, 0, W, H)
        cut, t4 = ops.cut(3, 62, 9, 4)
        assert 0 < t <= N and t2 == t3 == t4 == t
        if th.is_alive():
            ops.Pause()
        done = True
    finally:
        if not done:
            ops.Quit()
        th.join(60)
    assert not th.is_alive() and out["res"].TurnsCompleted == N
    assert t0 == 0 and np.array_equal(got0, np_region(start != 0, 1000, 55, 70, 20))
    cells = O.unpack(O.bits_run(O.pack(start), t)) != 0
    assert np.array_equal(got, np_region(cells, 1000, 55, 70, 20))
    assert box == np_box(np_region(cells, 1000, 55, 70, 20)) and whole == np_box(cells)
    assert np.array_equal(cut, np_region(cells, 3, 62, 9, 4))
    cells, _, _ = np_paste(cells, 3, 62, np.ones((4, 9), bool), "andnot")
    final = O.unpack(O.bits_run(words_of(cells), N - t))
    pix, turns = ops.view(0, 0, 1, W, H)
    assert turns == N and np.array_equal(pix, final)
    ops.close()


# ---------------------------------------------------------------- errors
def test_invalid_reads_are_einval(G):
    H, W = 64, 1024
    L, EINVAL = G.lib(), G._lib.GOL_EINVAL
    with G.Engine(H, W, device=0) as e:
        e.load_random(SEED)
        e.step(12)
        pat = np.full((H, W // 64), 3, np.uint64)
        n, lay = ctypes.c_int64(-1), ctypes.c_int32(-1)
        box = [ctypes.c_int64(-1) for _ in range(4)]
        region = [dict(w=0), dict(w=W + 1), dict(h=H + 1), dict(h=0), dict(x0=W), dict(x0=-1), dict(y0=-1), dict(y0=H)]
        for kw in region + [dict(w=65, stride=1), dict(stride=0), dict(flags=2), dict(flags=-1), dict(flags=3), dict(pattern=None)]:
            a = dict(x0=0, y0=0, w=8, h=8, stride=W // 64, flags=0, pattern=pat.ctypes.data)
            a.update(kw)
            rc = L.gol_engine_copy(e._h, a["x0"], a["y0"], a["w"], a["h"], a["pattern"], a["stride"], a["flags"],
                                   ctypes.byref(n), ctypes.byref(lay))
            assert rc == EINVAL, kw
        for kw in region:
            a = dict(x0=0, y0=0, w=8, h=8)
            a.update(kw)
            rc = L.gol_engine_bounds(e._h, a["x0"], a["y0"], a["w"], a["h"], *(ctypes.byref(x) for x in box), ctypes.byref(n),
                                     ctypes.byref(lay))
            assert rc == EINVAL, kw
        assert (n.value, lay.value) == (-1, -1) and all(x.value == -1 for x in box) and (pat == 3).all()
        for args in [(0, 0, 0, 1), (0, 0, W + 1, 1), (0, 0, 1, H + 1), (W, 0, 1, 1), (0, -1, 1, 1)]:
            for call in (e.copy, e.cut, e.bounds, e.to_rle):
                with pytest.raises(G.GolError) as ei:
                    call(*args)
                assert ei.value.code == EINVAL
        assert e.turn == 12 and e.info()["layout"] == "band"
        assert e.hash() == O.hash_words(O.bits_run(O.random_words(SEED, 0, H, W // 64), 12))
        # NULL outputs are fine
        assert L.gol_engine_bounds(e._h, 0, 0, W, H, None, None, None, None, None, None) == 0


def test_copy_cell_limit(G):
    """At most 2^26 cells per copy, on a 16384 x 8192 board (all dead): 8192 x 8193 cells is EINVAL,
    exactly 2^26 cells is accepted; bounds has no such limit, and to_rle raises the copy's error."""
    H, W = 16384, 8192
    L = G.lib()
    with G.Engine(H, W, device=0) as e:
        pat = np.full((8193, W // 64), 3, np.uint64)
        n = ctypes.c_int64(-1)
        for flags in (0, G._lib.GOL_COPY_CUT):
            assert L.gol_engine_copy(e._h, 0, 0, 8192, 8193, pat.ctypes.data, W // 64, flags, ctypes.byref(n), None) == G._lib.GOL_EINVAL
        assert n.value == -1 and (pat == 3).all()
        e.fill(5, 16380, 3, 8)  # rows 16380..16383 and 0..3
        assert L.gol_engine_copy(e._h, 5, 8200, 8192, 8192, pat.ctypes.data, W // 64, 0, ctypes.byref(n), None) == 0
        assert n.value == 24 and not pat[:8180].any() and (pat[8180:8188, 0] == 7).all() and not pat[8180:8188, 1:].any()
        assert e.bounds() == (5, 0, 3, H, 24) and e.bounds(0, 16000, W, 1000) == (5, 380, 3, 8, 24)
        e.fill(8000, 9000, 1, 1)
        with pytest.raises(G.GolError) as ei:
            e.to_rle()  # the box is 7996 x 16384 cells
        assert ei.value.code == G._lib.GOL_EINVAL
        assert e.alive_count() == 25
