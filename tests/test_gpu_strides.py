"""Every `stride` and `cap` argument of the C ABI with a value other than the trivial one.  The Python
wrappers pass stride == W (W / 64 for words) and a cap that holds every cell, so the suite never
sees the row arithmetic of a caller that passes more -- the Go drop-ins and any C host may.  Here
the C functions are called through the library handle with explicit strides: inputs with poisoned
padding (byte 7, all-ones words) that must have no effect, outputs poisoned with 0xA5 whose padding
and outer rows must come back untouched, and cell lists under every capacity at which a running cap
can go wrong.  The boards are the six of tests/engine_model.py CONFIGS (the smallest on which every
path exists): one and several shards, band, standard and byte rows.

GOLHIP_SEQUENCE_LIBRARY names another build of the library to run the same cases on.
"""
import ctypes

import numpy as np
import pytest

import engine_model as M
import io_ref as IO
from oracle import oracle as O
from testlib import env  # noqa: F401 (the fixture)

pytestmark = pytest.mark.gpu

CIDS = list(M.CONFIGS)
BIT_CIDS = [cid for cid in CIDS if M.Model.of(M.CONFIGS[cid]).bit]
assert CIDS == ["band1", "band3", "std2", "bytes", "w32", "odd"] and BIT_CIDS == ["band1", "band3", "std2"]


def engine(env, c):
    return env.G.Engine(c["H"], c["W"], device=0, library=env.L, **c["engine"])


def ok(env, rc):
    assert rc == 0, env.L.gol_last_error()


def load_bytes(env, e, board, stride):
    buf = IO.pitched(board, stride, IO.PAD_BYTE)
    ok(env, env.L.gol_engine_load_bytes(e._h, buf.ctypes.data, stride))


def store_bytes(env, e, stride):
    """(the board, True if the padding of the caller's rows is untouched)"""
    out = IO.poisoned(e.H, stride, np.uint8)
    ok(env, env.L.gol_engine_store_bytes(e._h, out.ctypes.data, stride))
    return IO.split_written(out, 0, e.H, e.W)


def store_words(env, e, y0, y1, stride):
    """(status, rows [y0, y1) as words, True if the padding and the rows around them are untouched)"""
    out = IO.poisoned(y1 - y0 + 2, stride, np.uint64)
    rc = env.L.gol_engine_store_words(e._h, y0, y1, out.ctypes.data + 8 * stride, stride)
    return (rc, *IO.split_written(out, 1, y1 - y0 if rc == 0 else 0, e.W // 64))


# ------------------------------------------------------------------ load_bytes / store_bytes
@pytest.mark.parametrize("cid", CIDS)
def test_load_bytes_and_store_bytes_with_wide_strides(env, cid):
    c = M.CONFIGS[cid]
    H, W, bit = c["H"], c["W"], cid in BIT_CIDS
    board = M.make_bytes(H, W, 11, .4, False)
    with engine(env, c) as e:
        load_bytes(env, e, board, W + 5)
        got, clean = store_bytes(env, e, W + 9)
        assert clean and np.array_equal(got, board) and e.alive_count() == np.count_nonzero(board)
        if bit:  # byte 7 in the padding leaves no exact first turn pending
            rc, words, clean = store_words(env, e, 0, H, W // 64 + 3)
            assert rc == 0 and clean and np.array_equal(words, O.pack(board))
        e.step(5)
        got, clean = store_bytes(env, e, W + 9)
        assert clean and e.turn == 5 and np.array_equal(got, O.run(board, 5))
        for y, x in ((H - 1, W - 1), (0, 0)):  # one byte 7 inside the board, next to the padding
            odd = board.copy()
            odd[y, x] = IO.PAD_BYTE
            load_bytes(env, e, odd, W + 5)
            got, clean = store_bytes(env, e, W + 9)
            assert clean and np.array_equal(got, odd) and e.alive_count() == np.count_nonzero(odd)
            if bit:
                rc, _, clean = store_words(env, e, 0, H, W // 64 + 3)
                assert rc == env.ESTATE and clean
            e.step(1)
            got, clean = store_bytes(env, e, W + 9)
            assert clean and e.turn == 1 and np.array_equal(got, O.run(odd, 1))


def test_byte_board_whose_last_cells_are_a_second_loop_item(env):
    """The byte board's count and 0/255 check run one thread per cell in a grid-stride loop
    (csrc/gol_launch.h: grid_for's default cap, 256 * 16 blocks of 256): three odd bytes among
    the cells only a second item reaches must be counted, and must send turn 1 to the exact kernel
    (read as alive they would be a blinker; under the exact rule they die and nothing is born)."""
    W = 1056  # W % 64 == 32: a byte board that steps 0/255 bytes on the k-turn kernels
    H = IO.second_trip_rows(256 * 16 * 256, W)
    board = M.make_bytes(H, W, 17, .4, False)
    with env.G.Engine(H, W, device=0, library=env.L) as e:
        assert e.info()["layout"] == "bytes"
        load_bytes(env, e, board, W + 5)
        assert e.alive_count() == np.count_nonzero(board)
        odd = board.copy()
        odd[[H - 2, H - 1, 0], W - 8:] = 0
        odd[H - 1, W - 5:W - 2] = 129
        assert (H - 1) * W + W - 5 >= 256 * 16 * 256
        load_bytes(env, e, odd, W + 5)
        assert e.alive_count() == np.count_nonzero(odd)
        e.step(1)
        got, clean = store_bytes(env, e, W + 9)
        want = O.run(odd, 1)
        assert clean and np.array_equal(got, want) and not want[H - 1, W - 6:W - 2].any() and e.alive_count() == np.count_nonzero(want)


# ------------------------------------------------------------------ store_rows
@pytest.mark.parametrize("cid", CIDS)
def test_store_rows_around_the_shard_seams(env, cid):
    c = M.CONFIGS[cid]
    H, W, stride = c["H"], c["W"], c["W"] + 9
    board = M.make_bytes(H, W, 12, .4, False)
    ranges = IO.seam_ranges(H, M.shard_seams(c))
    with engine(env, c) as e:
        e.load_bytes(board)
        e.step(3)  # (a band board is in the band layout now: the first range converts it)
        assert [e.shard(i)["y0"] for i in range(e.topology()["shards"])] == M.shard_seams(c)
        seen = []
        for y0, y1 in ranges:
            out = IO.poisoned(y1 - y0 + 2, stride, np.uint8)
            ok(env, env.L.gol_engine_store_rows(e._h, y0, y1, out.ctypes.data + stride, stride))
            seen.append(IO.split_written(out, 1, y1 - y0, W))
        full, clean = store_bytes(env, e, stride)
        assert clean and np.array_equal(full, O.run(board, 3))
        for (y0, y1), (got, clean) in zip(ranges, seen):
            assert clean and np.array_equal(got, full[y0:y1]), (y0, y1)


# ------------------------------------------------------------------ load_words / store_words
@pytest.mark.parametrize("cid", BIT_CIDS)
def test_load_words_and_store_words_with_wide_strides(env, cid):
    c = M.CONFIGS[cid]
    H, Ww = c["H"], c["W"] // 64
    stride = Ww + 3
    seams = M.shard_seams(c)
    ranges = [(max(s - 2, 0), min(s + 3, H)) for s in seams] + [(H - 2, H)]  # both sides of every seam, the wrap's too
    with engine(env, c) as e:
        e.load_random(21)
        e.step(2)
        want = O.bits_run(O.random_words(21, 0, H, Ww), 2)
        for i, (a, b) in enumerate(ranges):
            new = M.make_words(b - a, Ww, 30 + i)
            buf = IO.pitched(new, stride, IO.all_ones(np.uint64), 1, 1)
            ok(env, env.L.gol_engine_load_words(e._h, a, b, buf.ctypes.data + 8 * stride, stride))
            want[a:b] = new
        assert e.turn == 0 and e.alive_count() == O.popcount_words(want)  # the all-ones padding is not on the board
        got, clean = store_bytes(env, e, c["W"] + 9)
        assert clean and np.array_equal(got, O.unpack(want))
        for a, b in ranges + [(0, H), (1, 1)]:
            rc, got, clean = store_words(env, e, a, b, stride)
            assert rc == 0 and clean and np.array_equal(got, want[a:b]), (a, b)
        e.step(13)  # the halo was made again from the new rows
        rc, got, clean = store_words(env, e, 0, H, stride)
        assert rc == 0 and clean and e.turn == 13 and np.array_equal(got, O.bits_run(want, 13))


# ------------------------------------------------------------------ alive_cells / step_flips under a cap
def list_call(fn, e, cap, room, null=False):
    xy = np.full((room, 2), IO.POISON_I32, dtype=np.int32)
    n = ctypes.c_int64(-1)
    rc = fn(e._h, None if null else xy.ctypes.data, cap, ctypes.byref(n))
    return rc, n.value, xy


@pytest.mark.parametrize("odd", [False, True], ids=["binary", "odd_bytes"])
@pytest.mark.parametrize("cid", CIDS)
def test_alive_cells_under_every_cap(env, cid, odd):
    """binary: the board after two turns (a band board converts); odd_bytes: the loaded bytes at turn
    0, on the bit-capable boards with their exact first turn pending.  Alive = byte != 0."""
    c = M.CONFIGS[cid]
    board = M.make_bytes(c["H"], c["W"], 13, .3, odd)
    with engine(env, c) as e:
        e.load_bytes(board)
        if not odd:
            e.step(2)
            board = O.run(board, 2)
        xy = IO.alive_xy(board)
        total, room = len(xy), len(xy) + 8
        rc, n, _ = list_call(env.L.gol_engine_alive_cells, e, 0, 1, null=True)
        assert rc == 0 and n == total
        for cap in [0] + IO.caps_for(xy, e.shard(0)["y1"]):
            rc, n, buf = list_call(env.L.gol_engine_alive_cells, e, cap, room)
            assert rc == 0 and n == total and np.array_equal(buf, IO.capped(xy, cap, room)), cap
        assert e.turn == (0 if odd else 2)


@pytest.mark.parametrize("odd", [False, True], ids=["binary", "odd_bytes"])
@pytest.mark.parametrize("cid", CIDS)
def test_step_flips_under_every_cap(env, cid, odd):
    """The three modes of gol_engine_step_flips: a bit board (bit-capable, binary), the exact first
    turn after odd bytes (bit-capable, odd_bytes) and a byte board (the other three boards)."""
    c = M.CONFIGS[cid]
    board = M.make_bytes(c["H"], c["W"], 14, .3, odd)
    nxt = O.run(board, 1)
    xy = IO.flips_xy(board, nxt)
    total, room = len(xy), len(xy) + 8
    with engine(env, c) as e:
        shard0 = e.shard(0)["y1"]
        e.load_bytes(board)
        rc, n, _ = list_call(env.L.gol_engine_step_flips, e, 0, 1, null=True)
        assert rc == 0 and n == total and e.turn == 1
        for cap in [0] + IO.caps_for(xy, shard0):
            e.load_bytes(board)  # the call advances a turn
            rc, n, buf = list_call(env.L.gol_engine_step_flips, e, cap, room)
            assert rc == 0 and n == total and np.array_equal(buf, IO.capped(xy, cap, room)), cap
            assert e.turn == 1
        assert np.array_equal(e.store_bytes(), nxt)


# ------------------------------------------------------------------ the worker path
@pytest.mark.parametrize("W", [70, 512])
def test_next_state_slab_and_worker_update_with_three_strides(env, W):
    L, lib = env.L, env.G._lib
    H = 20
    board = IO.random_bytes(np.random.default_rng(16 + W), H, W)
    world_stride, out_stride, work_stride = W + 5, W + 7, W + 11
    world = IO.pitched(board, world_stride, IO.PAD_BYTE)
    for y0, y1 in ((0, H), (3, 9), (H - 1, H), (0, 1)):
        want = O.next_state_slab(board, y0, y1)
        out = IO.poisoned(y1 - y0 + 2, out_stride, np.uint8)
        ok(env, L.gol_next_state_slab(world.ctypes.data, H, W, world_stride, y0, y1, out.ctypes.data + out_stride, out_stride))
        got, clean = IO.split_written(out, 1, y1 - y0, W)
        assert clean and np.array_equal(got, want), (y0, y1)
        work = IO.poisoned(y1 - y0 + 2, work_stride, np.uint8)
        req = lib.gol_request(World=world.ctypes.data, world_stride=world_stride, Turns=1, ImageHeight=H, ImageWidth=W,
                              Threads=1, StartY=y0, EndY=y1, Worker=3)
        res = lib.gol_response(WorkSlice=work.ctypes.data + work_stride, work_stride=work_stride)
        ok(env, L.gol_worker_update(ctypes.byref(req), ctypes.byref(res)))
        got, clean = IO.split_written(work, 1, y1 - y0, W)
        assert clean and res.Worker == 3 and np.array_equal(got, want), (y0, y1)
    out = IO.poisoned(2, out_stride, np.uint8)
    assert L.gol_next_state_slab(world.ctypes.data, H, W, W - 1, 0, 1, out.ctypes.data, out_stride) == env.EINVAL
    assert L.gol_next_state_slab(world.ctypes.data, H, W, world_stride, 0, 1, out.ctypes.data, W - 1) == env.EINVAL
    assert IO.split_written(out, 0, 0, 0)[1]


# ------------------------------------------------------------------ the broker
@pytest.mark.parametrize("H,W", [(64, 128), (16, 16)], ids=["bit_board", "byte_board"])
def test_broker_run_and_retrieve_with_strides_and_a_short_alive_buffer(env, H, W):
    L, lib = env.L, env.G._lib
    turns = 3
    board = M.make_bytes(H, W, 15, .4, False)
    want = O.run(board, turns)
    xy = IO.alive_xy(want)
    total, room = len(xy), len(xy) + 4
    assert total > 8
    world = IO.pitched(board, W + 5, IO.PAD_BYTE)
    req = lib.gol_request(World=world.ctypes.data, world_stride=W + 5, Turns=turns, ImageHeight=H, ImageWidth=W, Threads=1)
    cfg = lib.gol_config(device=0)
    h = ctypes.c_void_p()
    ok(env, L.gol_broker_create(ctypes.byref(cfg), ctypes.byref(h)))
    try:
        for fn, stride, cap in ((L.gol_broker_run, W + 9, total // 2), (L.gol_broker_retrieve, W + 13, total - 1),
                                (L.gol_broker_retrieve, W + 9, 1), (L.gol_broker_retrieve, W + 9, total + 3)):
            out = IO.poisoned(H, stride, np.uint8)
            alive = np.full((room, 2), IO.POISON_I32, dtype=np.int32)
            res = lib.gol_response(Alive=alive.ctypes.data, alive_cap=cap, World=out.ctypes.data, world_stride=stride)
            ok(env, fn(h, ctypes.byref(req), ctypes.byref(res)))
            assert res.alive_len == res.AliveCount == total and res.TurnsCompleted == turns, cap
            got, clean = IO.split_written(out, 0, H, W)
            assert clean and np.array_equal(got, want), cap
            assert np.array_equal(alive, IO.capped(xy, cap, room)), cap
    finally:
        L.gol_broker_destroy(h)


# ------------------------------------------------------------------ after the last launch
def test_no_device_fault_was_reported(env):
    env.torch.cuda.synchronize()
    flags = ctypes.c_uint32(1)
    assert env.L.gol_dev_error(-1, ctypes.byref(flags)) == 0 and flags.value == 0
