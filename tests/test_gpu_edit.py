"""Board edits on the GPU (gol_engine_paste / gol_broker_paste): a rectangle pasted into the running
board in the layout it is stepped in.  Every comparison is exact, against numpy on the oracle's
board (O.random_words / O.bits_run / O.unpack, tests/rule_ref.py for other rules): the cells after
the edit, the `changed` count, and the boards that stepping makes of them."""
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
from region_ref import BYTE_EDITS, SEED, apply_edits, np_paste, random_cells, words_of
from testlib import gpu_lib as G  # noqa: F401 (the fixture)

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORKER = os.path.join(ROOT, "tests", "_edit_rank_worker.py")


# ---------------------------------------------------------------- band, in place
@pytest.mark.parametrize("H,W,edits", [
    (96, 1024, [(1000, 90, 50, 12, "copy", 1),    # wraps both axes: rows 90..95 and 0..5, bands 31 and 0
                (5, 0, 36, 12, "or", 2),           # rows 0..11; w just above Wd = 32
                (300, 84, 33, 12, "xor", 3),       # rows H-12..H-1
                (1023, 40, 1, 1, "andnot", 4),     # one cell, the last bit of the last word
                (17, 20, 32, 5, "copy", 5),        # w = Wd
                (10, 50, 1024, 3, "xor", None),    # fill: the full width from the middle of a band
                (700, 94, 400, 4, "andnot", None)]),
    (64, 2048, [(2000, 60, 100, 9, "copy", 6),    # w = 100 > Wd = 64, wraps both axes
                (3, 0, 100, 12, "xor", 7),
                (0, 52, 2048, 12, "or", 8)]),
])
def test_band_paste_in_place(G, H, W, edits):
    cells = random_cells(H, W, 24)
    with G.Engine(H, W, layout="band", device=0) as e:
        e.load_random(SEED)
        e.step(24)
        cells = apply_edits(e, cells, edits, "band", 24)
        pix, lay = e.view(0, 0, 1, W, H, return_layout=True)
        assert lay == "band" and np.array_equal(pix != 0, cells)
        e.step(12)
        assert e.turn == 36 and e.hash() == O.hash_words(O.bits_run(words_of(cells), 12))


# ---------------------------------------------------------------- standard bit rows
def test_standard_paste(G):
    H, W = 100, 192
    cells = random_cells(H, W, 9)
    with G.Engine(H, W, layout="standard", device=0) as e:
        e.load_random(SEED)
        e.step(9)
        edits = [(37, 95, 192, 10, "copy", 1),   # the full width at x0 % 32 = 5: first and last span are one word
                 (1, 3, 31, 4, "xor", 2),         # inside one word
                 (191, 50, 3, 3, "or", 3),        # the last bit and the wrap
                 (64, 0, 64, 12, "andnot", 4),    # whole words
                 (31, 0, 192, 100, "xor", None),  # every cell inverted, from bit 31
                 (95, 98, 97, 4, "copy", 5)]
        cells = apply_edits(e, cells, edits, "standard", 9)
        assert np.array_equal(e.view(0, 0, 1, W, H) != 0, cells)
        e.step(8)
        assert e.hash() == O.hash_words(O.bits_run(words_of(cells), 8))


# ---------------------------------------------------------------- byte rows
@pytest.mark.parametrize("H,W", [(50, 100), (50, 50)])  # aligned 4-byte words (W % 4 == 0); one byte per lane
def test_bytes_paste_odd_width(G, H, W):
    rng = np.random.default_rng(5)
    start = (rng.random((H, W)) < 0.4).astype(np.uint8) * 255
    cells = O.run(start, 5) != 0
    with G.Engine(H, W, device=0) as e:
        e.load_bytes(start)
        e.step(5)
        edits = [(x0 % W, y0, min(w, W), h, op, seed) for x0, y0, w, h, op, seed in BYTE_EDITS]
        cells = apply_edits(e, cells, edits, "bytes", 5)
        board = cells.astype(np.uint8) * 255
        assert np.array_equal(e.store_bytes(), board)
        e.step(5)
        assert np.array_equal(e.store_bytes(), O.run(board, 5))


def test_bytes_paste_bytes_layout(G):
    H, W = 64, 128
    cells = random_cells(H, W, 33)
    with G.Engine(H, W, layout="bytes", device=0) as e:
        e.load_random(SEED)
        e.step(33)
        cells = apply_edits(e, cells, BYTE_EDITS + [(1, 60, 128, 8, "copy", 9)], "bytes", 33)
        board = cells.astype(np.uint8) * 255
        assert np.array_equal(e.store_bytes(), board)
        e.step(40)  # the 32-turn byte pipeline and the k-turn kernel behind it
        assert np.array_equal(e.store_bytes(), O.unpack(O.bits_run(words_of(cells), 40)))


def test_bytes_paste_keeps_untouched_odd_bytes(G):
    """A byte board loaded with bytes in {0, 7, 255}: written cells become 0 / 255, every other byte
    stays, and the board then steps exactly as the oracle (its exact semantics)."""
    H, W = 50, 100
    rng = np.random.default_rng(6)
    board = rng.choice(np.array([0, 7, 255], dtype=np.uint8), size=(H, W))
    with G.Engine(H, W, device=0) as e:
        e.load_bytes(board)
        for x0, y0, w, h, op, seed in BYTE_EDITS:
            p = np.ones((h, w), bool) if seed is None else np.random.default_rng(seed).random((h, w)) < 0.5
            n = e.fill(x0, y0, w, h, op) if seed is None else e.paste(p, x0, y0, op)
            cells, want, written = np_paste(board != 0, x0, y0, p, op)
            assert n == want and e.turn == 0
            board = np.where(written, cells.astype(np.uint8) * 255, board)
            assert np.array_equal(e.store_bytes(), board), (x0, y0, op)
        assert (board == 7).any()
        e.step(3)
        assert np.array_equal(e.store_bytes(), O.run(board, 3))


def test_exact_first_turn_pending_is_estate(G):
    rng = np.random.default_rng(7)
    board = (rng.random((64, 64)) < 0.4).astype(np.uint8) * 255
    board[10, 10] = 7
    with G.Engine(64, 64, device=0) as e:
        e.load_bytes(board)
        for call in (lambda: e.paste(np.ones((3, 3)), 5, 5), lambda: e.fill(0, 0, 64, 64, "andnot")):
            with pytest.raises(G.GolError) as ei:
                call()
            assert ei.value.code == G._lib.GOL_ESTATE
        assert np.array_equal(e.store_bytes(), board) and e.turn == 0
        e.step(1)
        after = O.run(board, 1)
        assert e.fill(8, 8, 5, 5, "xor") == 25  # a bit board now
        after[8:13, 8:13] ^= 255
        assert np.array_equal(e.store_bytes(), after)


# ---------------------------------------------------------------- shards and ranks: the halo is made again
@pytest.mark.parametrize("shards", [2, 3])
def test_paste_invalidates_the_halo(G, shards):
    H, W = 96, 1024
    cells = random_cells(H, W, 12)
    with G.Engine(H, W, shards=shards, same_device=True, transport="loopback", device=0) as e:
        e.load_random(SEED)
        e.step(12)  # a halo has been issued for the next step
        edits = [(100, 28, 200, 40, "copy", 1),    # rows 28..67: across the boundaries 32, 48 and 64
                 (1000, 90, 60, 12, "xor", 2)]     # rows 90..95 and 0..5: the last shard and the first
        cells = apply_edits(e, cells, edits, "band", 12)
        e.step(24)
        assert e.hash() == O.hash_words(O.bits_run(words_of(cells), 24))


def run_edit_ranks(G, nranks, H, W, turns, pastes, only_holders, more):
    uid = G.engine.unique_id("ipc").hex()
    procs = []
    for r in range(nranks):
        a = dict(uid=uid, H=H, W=W, nranks=nranks, rank=r, seed=SEED, turns=turns, pastes=pastes,
                 only_holders=only_holders, more=more)
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


@pytest.mark.parametrize("only_holders", [False, True])
def test_ranks_paste_their_rows(G, only_holders):
    """Two IPC rank processes (rows 0..31 and 32..63): a rectangle across their boundary, one across
    row H-1 -> 0 and one inside rank 1's rows alone, which rank 0 may skip; the collective step after
    them is the oracle's, and the ranks' changed counts add up."""
    H, W = 64, 1024
    pastes = [[1000, 25, 60, 14, "copy", 1], [10, 60, 40, 8, "xor", 2], [500, 40, 33, 5, "or", 3]]
    cells = random_cells(H, W, 12)
    want = []
    for x0, y0, w, h, op, seed in pastes:
        cells, n, _ = np_paste(cells, x0, y0, np.random.default_rng(seed).random((h, w)) < 0.5, op)
        want.append(n)
    res = run_edit_ranks(G, 2, H, W, 12, pastes, only_holders, 24)
    for r in range(2):
        assert (res[r]["y0"], res[r]["y1"]) == O.partition(H, 2, r)
        assert res[r]["turn"] == 12 and set(res[r]["layouts"]) == {"band"}
        assert res[r]["hash"] == O.hash_words(O.bits_run(words_of(cells), 24))
    assert (res[0]["changed"][2] is None) == only_holders and None not in res[1]["changed"]
    assert [sum(res[r]["changed"][i] or 0 for r in range(2)) for i in range(3)] == want


# ---------------------------------------------------------------- rules
def test_rle_glider_under_another_rule(G):
    H, W = 64, 1024
    glider = "#N Glider\nx = 3, y = 3, rule = B3/S23\nbob$2bo$3o!\n"
    with G.Engine(H, W, rule="B36/S23", device=0) as e:
        e.load_bytes(np.zeros((H, W), np.uint8))
        assert e.paste(glider, 1020, 60) == 5  # an empty board: the glider's five cells
        packed = np.array([[2 | 1 << 40], [4], [7]], np.uint64)  # the same cells bit-packed (bits past w = 3: ignored)
        assert e.paste_words(packed, 3, 1020, 60) == 0 and e.paste_words(packed, 3, 1020, 60, "xor") == 5
        assert e.alive_count() == 0 and e.paste_words(packed, 3, 1020, 60, "or") == 5
        e.step(40)
        board = np.zeros((H, W), np.uint8)
        board[np.ix_([60, 61, 62], [1020, 1021, 1022])] = G.parse_rle(glider)[0]
        want = R.run(board, "B36/S23", 40)[0]
        assert want.sum() == 5 and np.array_equal(e.store_bytes(), R.to_bytes(want))


# ---------------------------------------------------------------- broker
def test_broker_paste_during_a_run(G):
    """A Run paused at turn 0 (a Pause queued before it), resumed and paused again one or more chunks
    later; the paste lands after the reported turn, and the Run's final board is the oracle's run
    split there with the edit applied."""
    H, W, N = 64, 1024, 6000
    rng = np.random.default_rng(8)
    start = (rng.random((H, W)) < 0.35).astype(np.uint8) * 255
    p = rng.random((20, 70)) < 0.5
    ops = G.Operations(device=0)
    size = G.Request(ImageHeight=H, ImageWidth=W)
    with pytest.raises(G.GolError) as ei:
        ops.paste(p, 0, 0)
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
        ops.Pause()  # resume ...
        ops.Pause()  # ... and pause again after the chunk
        while th.is_alive() and not (state()[0] > 0 and state()[1]):
            assert time.time() < deadline
        n, t = ops.paste(p, 1000, 55, "xor")
        assert 0 < t <= N
        n2, t2 = ops.paste((9, 4), 3, 62, "andnot")  # a cleared rectangle at the same turn
        assert t2 == t
        if th.is_alive():
            ops.Pause()
        done = True
    finally:
        if not done:
            ops.Quit()
        th.join(60)
    assert not th.is_alive() and out["res"].TurnsCompleted == N
    cells, want, _ = np_paste(O.unpack(O.bits_run(O.pack(start), t)) != 0, 1000, 55, p, "xor")
    cells, want2, _ = np_paste(cells, 3, 62, np.ones((4, 9), bool), "andnot")
    assert (n, n2) == (want, want2)
    final = O.unpack(O.bits_run(words_of(cells), N - t))
    pix, turns = ops.view(0, 0, 1, W, H)
    assert turns == N and np.array_equal(pix, final)
    if t < N:  # (t == N: the Run had ended, and its response predates the edit)
        assert np.array_equal(out["res"].World, final)
    ops.close()


# ---------------------------------------------------------------- errors
def test_invalid_pastes_are_einval(G):
    H, W = 64, 1024
    L = G.lib()
    with G.Engine(H, W, device=0) as e:
        e.load_random(SEED)
        e.step(12)
        before = e.hash()
        pat = np.zeros((H, W // 64), np.uint64)
        n, lay = ctypes.c_int64(-1), ctypes.c_int32(-1)
        bad = [dict(w=0), dict(w=W + 1), dict(h=H + 1), dict(h=0), dict(x0=W), dict(x0=-1), dict(y0=-1), dict(y0=H),
               dict(op=4), dict(op=-1), dict(w=65, stride=1)]
        for kw in bad:
            a = dict(x0=0, y0=0, w=8, h=8, stride=W // 64, op=0)
            a.update(kw)
            rc = L.gol_engine_paste(e._h, a["x0"], a["y0"], a["w"], a["h"], pat.ctypes.data, a["stride"], a["op"],
                                    ctypes.byref(n), ctypes.byref(lay))
            assert rc == G._lib.GOL_EINVAL, kw
        assert (n.value, lay.value) == (-1, -1)
        for args in [(0, 0, 0, 1), (0, 0, W + 1, 1), (0, 0, 1, H + 1), (W, 0, 1, 1), (0, -1, 1, 1)]:
            with pytest.raises(G.GolError) as ei:
                e.fill(*args)
            assert ei.value.code == G._lib.GOL_EINVAL
        with pytest.raises(G.GolError):
            e.fill(0, 0, 1, 1, "nand")
        assert e.hash() == before and e.turn == 12
        # NULL changed / dst_layout are fine; a NULL pattern ignores the stride
        assert L.gol_engine_paste(e._h, 0, 0, 8, 8, None, 0, G._lib.GOL_PASTE_XOR, None, None) == 0
        assert L.gol_engine_paste(e._h, 0, 0, 8, 8, None, 0, G._lib.GOL_PASTE_XOR, None, None) == 0
        assert e.hash() == before


def test_paste_cell_limit(G):
    """At most 2^26 cells per paste, on a board large enough to hold more (8200 x 8192, all dead):
    8192 x 8193 cells is EINVAL and changes nothing, exactly 2^26 cells is accepted."""
    H, W = 8200, 8192
    L = G.lib()
    with G.Engine(H, W, device=0) as e:
        n = ctypes.c_int64(-1)
        assert L.gol_engine_paste(e._h, 0, 0, W, 8193, None, 0, G._lib.GOL_PASTE_XOR, ctypes.byref(n), None) == G._lib.GOL_EINVAL
        assert L.gol_engine_paste(e._h, 0, 0, 8191, 8194, None, 0, G._lib.GOL_PASTE_XOR, ctypes.byref(n), None) == G._lib.GOL_EINVAL
        assert n.value == -1 and e.alive_count() == 0
        assert e.fill(5, 8190, W, 8192, "xor") == 1 << 26  # rows 8190..8199 and 0..8181
        assert e.alive_count() == 1 << 26
        assert e.view_counts(0, 8182, 8, W // 8, 1).sum() == 0 and e.view_counts(0, 8190, 2, W // 2, 5).sum() == 10 * W


def test_paste_words_takes_packed_rows(G):
    """Engine.paste_words: rows that are already bit-packed, with a stride wider than ceil(w / 64) and
    garbage in the bits past w and in the pad words, give the cells of Engine.paste."""
    H, W, w, h = 64, 1024, 100, 20
    rng = np.random.default_rng(12)
    p = rng.random((h, w)) < 0.5
    words = rng.integers(0, 1 << 63, (h, 4), dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, (h, 4), dtype=np.uint64)
    words[:, :2] = G._lib.pack_pattern(p)
    words[:, 1] |= rng.integers(0, 1 << 63, h, dtype=np.uint64) << np.uint64(w - 64)
    cells = random_cells(H, W, 12)
    with G.Engine(H, W, device=0) as e:
        e.load_random(SEED)
        e.step(12)
        for x0, y0, op in [(990, 55, "copy"), (3, 3, "xor"), (500, 30, "andnot"), (1023, 63, "or")]:
            cells, want, _ = np_paste(cells, x0, y0, p, op)
            assert e.paste_words(words, w, x0, y0, op, return_layout=True) == (want, "band")
        with pytest.raises(ValueError):
            e.paste_words(words[:, :1], w, 0, 0)
        assert np.array_equal(e.view(0, 0, 1, W, H) != 0, cells)
        e.step(12)
        assert e.hash() == O.hash_words(O.bits_run(words_of(cells), 12))
