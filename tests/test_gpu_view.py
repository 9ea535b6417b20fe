"""Viewport frames on the GPU (gol_engine_view / gol_engine_view_counts / gol_broker_view): the
alive cells of every scale x scale box of a torus rectangle, read from the board in the layout it
is stepped in.  The reference is always numpy on the oracle's board (gather with wrap, reshape,
sum over the box); counts and pixels must be equal, no tolerance."""
import ctypes
import json
import os
import subprocess
import sys
import threading
import time

import numpy as np
import pytest

from oracle import oracle as O
from region_ref import check_view, ref_counts, ref_pixels
from testlib import gpu_lib as G  # noqa: F401 (the fixture)

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORKER = os.path.join(ROOT, "tests", "_view_rank_worker.py")
SEED = 11


_boards = {}


def random_board(H, W, turns, seed=SEED):
    """The oracle's board of load_random(seed) after `turns` turns, as bytes (computed once)."""
    key = (H, W, turns, seed)
    if key not in _boards:
        words = O.bits_run(O.random_words(seed, 0, H, W // 64), turns)
        board = O.unpack(words)
        board.setflags(write=False)
        _boards[key] = (words, board)
    return _boards[key]


# ---------------------------------------------------------------- band, in place
@pytest.mark.parametrize("H,W,views", [
    (300, 1024, [(0, 0, 1, 1024, 300), (29, 293, 3, 341, 100)]),
    (97, 2048, [(0, 0, 1, 2048, 97), (2040, 60, 7, 290, 13)]),
])
def test_band_view_reads_the_board_in_place(G, H, W, views):
    """A band board stays in the band layout through views (a store converts it), the frames of
    both layouts are the oracle's, and the next step is still right."""
    words, board = random_board(H, W, 24)
    with G.Engine(H, W, layout="band", device=0) as e:
        e.load_random(SEED)
        e.step(24)
        first = [check_view(e, board, v, "band") for v in views]
        again = [check_view(e, board, v, "band") for v in views]  # still band on a second view
        assert np.array_equal(e.store_rows(3, 9), board[3:9])  # the readers convert to the standard layout
        after = [check_view(e, board, v, "standard") for v in views]
        for a, b, c in zip(first, again, after):
            assert np.array_equal(a[0], b[0]) and np.array_equal(a[0], c[0])
            assert np.array_equal(a[1], b[1]) and np.array_equal(a[1], c[1])
        e.step(12)
        assert e.hash() == O.hash_words(O.bits_run(words, 12))


@pytest.fixture(scope="module")
def band_engine(G):
    e = G.Engine(300, 1024, layout="band", device=0)
    e.load_random(SEED)
    e.step(24)
    yield e
    e.close()


@pytest.mark.parametrize("view", [
    (0, 0, 1, 1024, 300),      # the whole board: the PGM's bytes
    (1019, 297, 1, 64, 16),    # wraps both axes
    (29, 293, 3, 341, 100),    # scale divides neither Wd = 32 nor the rows; boxes straddle band boundaries and the bit 31 -> 0 wrap; all 300 rows
    (8, 0, 16, 64, 18),
    (1000, 150, 256, 4, 1),    # boxes of 8 bands x 2 row groups
    (1000, 149, 150, 6, 2),    # 150 rows per box: two row groups each; 900 cells = 29 bits of a word
])
def test_band_viewports(G, band_engine, view):
    _, board = random_board(300, 1024, 24)
    counts, pix = check_view(band_engine, board, view, "band")
    if view == (0, 0, 1, 1024, 300):
        assert np.array_equal(pix, board)


# ---------------------------------------------------------------- standard bit rows
@pytest.mark.parametrize("H,W", [(128, 256), (100, 192)])
def test_standard_viewports(G, H, W):
    _, board = random_board(H, W, 9)
    with G.Engine(H, W, layout="standard", device=0) as e:
        e.load_random(SEED)
        e.step(9)
        for view in [(W - 27, H - 3, 1, 100, 20),          # x0 % 32 != 0, wraps both axes
                     (13, 5, 1, W, H),                      # every cell, the first word read from both ends
                     (W - 13, H - 7, 5, W // 5, H // 5),    # boxes across word boundaries and both wraps
                     (45, H - 10, 32, W // 32, H // 32),    # one box = parts of two words
                     (31, 1, 1, 1, 1), (0, 0, 1, 33, 2)]:
            check_view(e, board, view, "standard")
        assert e.hash() == O.hash_words(O.bits_run(O.random_words(SEED, 0, H, W // 64), 9))


# ---------------------------------------------------------------- byte rows
@pytest.mark.parametrize("H,W,views", [
    # W % 64 != 0: the byte board.  W % 4 == 0 reads aligned 4-byte words (4 cells per lane) ...
    (33, 48, [(0, 0, 1, 48, 33), (40, 30, 1, 48, 33), (47, 32, 5, 9, 6), (3, 3, 33, 1, 1), (2, 1, 2, 24, 16),
              (45, 1, 3, 16, 11)]),
    # ... any other width one byte per lane
    (31, 50, [(0, 0, 1, 50, 31), (47, 29, 3, 16, 10), (49, 30, 7, 7, 4)]),
])
def test_bytes_viewports_odd_width(G, H, W, views):
    rng = np.random.default_rng(5)
    start = (rng.random((H, W)) < 0.4).astype(np.uint8) * 255
    board = O.run(start, 5)
    with G.Engine(H, W, device=0) as e:
        e.load_bytes(start)
        e.step(5)
        for view in views:
            check_view(e, board, view, "bytes")
        assert np.array_equal(e.store_bytes(), board)


def test_bytes_viewports_bytes_layout(G):
    _, board = random_board(50, 128, 33)
    with G.Engine(50, 128, layout="bytes", device=0) as e:
        e.load_random(SEED)
        e.step(33)
        for view in [(0, 0, 1, 128, 50), (100, 40, 3, 42, 16), (5, 45, 2, 64, 25)]:
            check_view(e, board, view, "bytes")


def test_exact_first_turn(G):
    """Bytes other than 0/255 at turn 0: the view counts bytes != 0 (what alive_count counts);
    after the exact first turn it reads the bit board."""
    rng = np.random.default_rng(6)
    start = rng.choice(np.array([0, 7, 255], dtype=np.uint8), size=(40, 128))
    with G.Engine(40, 128, device=0) as e:
        e.load_bytes(start)
        for view in [(0, 0, 1, 128, 40), (120, 35, 3, 42, 13), (1, 39, 8, 16, 5)]:
            check_view(e, start, view, "bytes")
        whole = e.view_counts(0, 0, 8, 16, 5)
        assert int(whole.sum()) == e.alive_count() == int(np.count_nonzero(start))
        e.step(1)
        after = O.run(start, 1)
        for view in [(0, 0, 1, 128, 40), (120, 35, 3, 42, 13)]:
            check_view(e, after, view, "standard")


# ---------------------------------------------------------------- shards and ranks
def test_shards_sum_partial_frames(G):
    """Three shards (rows 0-66, 67-133, 134-199): boxes of 7 rows straddle both boundaries."""
    _, board = random_board(200, 2048, 24)
    with G.Engine(200, 2048, shards=3, same_device=True, transport="loopback", device=0) as e:
        e.load_random(SEED)
        e.step(24)
        assert [e.shard(i)["y0"] for i in range(3)] == [0, 67, 134]
        check_view(e, board, (2040, 60, 7, 290, 28), "band")
        check_view(e, board, (5, 190, 1, 64, 20))  # wraps from the last shard to the first
        tiles, _ = check_view(e, board, (0, 0, 8, 256, 25))
        assert int(tiles.sum(dtype=np.int64)) == e.alive_count()


def run_view_ranks(G, tmp_path, nranks, H, W, view, turns):
    uid = G.engine.unique_id("ipc").hex()
    procs = []
    for r in range(nranks):
        a = dict(uid=uid, H=H, W=W, nranks=nranks, rank=r, seed=SEED, turns=turns, view=list(view),
                 out=str(tmp_path / f"rank{r}.npy"))
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


def test_ranks_return_their_rows(G, tmp_path):
    """Two IPC rank processes: each rank's view_counts is the oracle restricted to its rows, the
    two frames add up to the whole view, and view (pixels) needs every row local."""
    H, W, view = 300, 1024, (1000, 140, 5, 200, 40)
    _, board = random_board(H, W, 24)
    res = run_view_ranks(G, tmp_path, 2, H, W, view, 24)
    total = np.zeros((view[4], view[3]), dtype=np.uint32)
    for r in range(2):
        d = res[r]
        assert (d["y0"], d["y1"]) == O.partition(H, 2, r)
        mine = np.zeros_like(board)
        mine[d["y0"]:d["y1"]] = board[d["y0"]:d["y1"]]
        got = np.load(d["out"])
        assert got.dtype == np.uint32 and np.array_equal(got, ref_counts(mine, *view)), f"rank {r}"
        assert d["layout"] == "band"
        assert d["view_error"] == G._lib.GOL_EINVAL
        assert d["hash"] == O.hash_words(O.bits_run(O.random_words(SEED, 0, H, W // 64), 24))
        total += got
    assert np.array_equal(total, ref_counts(board, *view))


# ---------------------------------------------------------------- broker
def test_broker_view_during_a_run(G):
    rng = np.random.default_rng(8)
    start = (rng.random((256, 1024)) < 0.35).astype(np.uint8) * 255
    ops = G.Operations(device=0)
    size = G.Request(ImageHeight=256, ImageWidth=1024)
    with pytest.raises(G.GolError) as ei:
        ops.view(0, 0, 1, 1024, 256)
    assert ei.value.code == G._lib.GOL_ESTATE  # no board yet
    out = {}
    th = threading.Thread(target=lambda: out.update(res=ops.Run(
        G.Request(World=start, Turns=10**9, ImageHeight=256, ImageWidth=1024, Threads=4))))
    th.start()
    quit_sent = False
    try:
        deadline = time.time() + 60

        def turns_completed():
            try:
                return ops.RetrieveCurrentData(size, alive=False, world=False).TurnsCompleted
            except G.GolError as x:  # the Run thread has not loaded its board yet
                assert x.code == G._lib.GOL_ESTATE
                return 0
        while turns_completed() == 0:
            assert time.time() < deadline
        ops.Pause()
        while not ops.paused:
            assert time.time() < deadline
        pix, turns, layout = ops.view(0, 0, 1, 1024, 256, return_layout=True)
        assert layout == "band"  # read as it is stepped: nothing converted it
        r = ops.RetrieveCurrentData(size, alive=False)
        assert turns == r.TurnsCompleted > 0
        assert np.array_equal(pix, r.World)
        pix4, turns4 = ops.view(1000, 250, 4, 256, 64)
        assert turns4 == turns
        assert np.array_equal(pix4, ref_pixels(ref_counts(r.World, 1000, 250, 4, 256, 64), 4))
        ops.Pause()
        ops.Quit()
        quit_sent = True
    finally:
        if not quit_sent:
            ops.Quit()
        th.join(60)
    assert not th.is_alive()
    assert out["res"].TurnsCompleted >= turns
    ops.close()


def test_broker_view_at_turn_zero_shows_the_loaded_board(G):
    """Unlike RetrieveCurrentData's all-zero board at turn 0 (broker.go:67-70)."""
    rng = np.random.default_rng(9)
    start = (rng.random((64, 128)) < 0.5).astype(np.uint8) * 255
    ops = G.Operations(device=0)
    res = ops.Run(G.Request(World=start, Turns=0, ImageHeight=64, ImageWidth=128, Threads=1))
    assert res.TurnsCompleted == 0
    pix, turns = ops.view(0, 0, 1, 128, 64)
    assert turns == 0 and np.array_equal(pix, start)
    assert not ops.RetrieveCurrentData(G.Request(ImageHeight=64, ImageWidth=128), alive=False).World.any()
    ops.close()


# ---------------------------------------------------------------- errors
def test_invalid_views_are_einval(G):
    H, W = 8256, 8192  # large enough for a view of more than 2^26 pixels
    L = G.lib()
    with G.Engine(H, W, device=0) as e:
        e.load_random(SEED)
        e.step(12)
        buf = np.zeros(64 * 64, dtype=np.uint32)
        lay = ctypes.c_int32(-1)
        bad = [
            (0, 0, 0, 8, 8, 8), (0, 0, 4097, 1, 1, 1), (0, 0, -1, 8, 8, 8),   # scale
            (0, 0, 1, 0, 8, 8), (0, 0, 1, 8, 0, 8), (0, 0, 1, -2, 8, 8),       # out_w, out_h
            (0, 0, 2, W // 2 + 1, 8, W), (0, 0, 2, 8, H // 2 + 1, 8),          # more than one turn of the torus
            (-1, 0, 1, 8, 8, 8), (W, 0, 1, 8, 8, 8), (0, -1, 1, 8, 8, 8), (0, H, 1, 8, 8, 8),
            (0, 0, 1, 8192, 8193, 8192),                                       # 2^26 + 8192 pixels
            (0, 0, 1, 8, 8, 7),                                                # stride < out_w
        ]
        for fn in (L.gol_engine_view_counts, L.gol_engine_view):
            for x0, y0, scale, ow, oh, stride in bad:
                rc = fn(e._h, x0, y0, scale, ow, oh, buf.ctypes.data, stride, ctypes.byref(lay))
                assert rc == G._lib.GOL_EINVAL, (x0, y0, scale, ow, oh, stride)
            assert fn(e._h, 0, 0, 1, 8, 8, None, 8, None) == G._lib.GOL_EINVAL
        assert lay.value == -1 and not buf.any()
        for args in [(0, 0, 1, 0, 8), (0, 0, 1, 8192, 8193), (0, 0, 5000, 1, 1)]:
            with pytest.raises(G.GolError) as ei:
                e.view(*args)
            assert ei.value.code == G._lib.GOL_EINVAL
        # a valid view with a wider stride leaves the padding alone; NULL src_layout is fine
        buf[:] = 7
        assert L.gol_engine_view_counts(e._h, 5, 5, 2, 8, 4, buf.ctypes.data, 10, None) == 0
        got = buf[:40].reshape(4, 10)
        assert (got[:, 8:] == 7).all() and (got[:, :8] <= 4).all() and (buf[40:] == 7).all()
        e.step(12)
        assert e.hash() == O.mt_hash_words(mt_run(H, W, 24))


def mt_run(H, W, turns):
    words = O.mt_random_words(SEED, H, W // 64)
    O.mt_bits_run(words, turns, turns)
    return words
