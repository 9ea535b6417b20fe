"""tests/io_ref.py, the expectations of the two edge-pinning GPU files, against the oracle (no GPU)."""
import numpy as np

import engine_model as M
import io_ref as IO
from oracle import oracle as O


def test_cell_lists_are_the_oracles():
    board = M.make_bytes(9, 21, 3, .4, True)
    nxt = O.run(board, 1)
    assert IO.alive_xy(board).tolist() == [list(c) for c in O.alive_cells(board)]
    assert IO.flips_xy(board, nxt).tolist() == [list(c) for c in O.flipped_cells(board, nxt)]
    assert IO.alive_xy(np.zeros((3, 4), np.uint8)).shape == (0, 2)


def test_bits_and_bytes_are_the_oracles():
    rng = np.random.default_rng(5)
    board = IO.random_bytes(rng, 7, 128)
    assert set(np.unique(board).tolist()) == set(IO.ODD_BYTES)
    assert np.array_equal(IO.bits_of_bytes(board).view("<u8"), O.pack(board))
    words = IO.bits_of_bytes(board)
    assert np.array_equal(IO.bytes_of_bits(words), O.unpack(words.view("<u8")))
    odd = IO.bits_of_bytes(board[:, :96])  # three words a row: no uint64 view
    assert np.array_equal(IO.bytes_of_bits(odd), O.unpack(words.view("<u8"))[:, :96])
    assert IO.hash_of(words, 7) == O.hash_words(words.view("<u8"), 7) != IO.hash_of(words, 0)


def test_capped_list_and_caps():
    xy = IO.alive_xy(M.make_bytes(6, 10, 1, .5, False))
    n = len(xy)
    for cap in IO.caps_for(xy, 3):
        buf = IO.capped(xy, cap, n + 8)
        m = min(n, cap)
        assert np.array_equal(buf[:m], xy[:m]) and (buf[m:] == IO.POISON_I32).all()
    caps = IO.caps_for(xy, 3)
    assert caps[0] == 1 and n - 1 in caps and n in caps and n + 5 in caps and len(set(caps)) == len(caps)
    assert int((xy[:, 1] < 3).sum()) in caps and int((xy[:, 1] == 0).sum()) in caps


def test_pitched_buffers_and_the_written_window():
    pay = np.arange(6, dtype=np.uint32).reshape(2, 3)
    buf = IO.pitched(pay, 5, IO.all_ones(np.uint32), before=1, after=2)
    assert buf.shape == (5, 5) and np.array_equal(buf[1:3, :3], pay) and (buf[0] == 0xFFFFFFFF).all() and (buf[1:3, 3:] == 0xFFFFFFFF).all()
    out = IO.poisoned(4, 5, np.uint32)
    assert out.shape == (4, 5) and (out == 0xA5A5A5A5).all()
    out[1:3, :3] = pay
    got, clean = IO.split_written(out, 1, 2, 3)
    assert np.array_equal(got, pay) and clean
    out[3, 4] = 0
    assert not IO.split_written(out, 1, 2, 3)[1]


def test_second_trip_rows_and_seam_ranges():
    for threads, units in ((256 * 16 * 256, 2101), (256 * 64 * 256, 66), (256 * 64 * 256, 2050), (256 * 16 * 256, 1050)):
        rows = IO.second_trip_rows(threads, units)
        over = rows * units - threads
        assert 0 < over < threads and over % 64 and (rows - 1) * units <= threads + 64 * units
    ranges = IO.seam_ranges(80, M.shard_seams(M.CONFIGS["band3"]))
    assert (0, 80) in ranges and any(a == b for a, b in ranges)
    for s in (27, 54):
        assert (s - 1, s + 1) in ranges and (s, s + 3) in ranges and (s - 3, s) in ranges
    assert all(0 <= a <= b <= 80 for a, b in ranges)
