"""The board utilities of csrc/gol_util.hip through their public launchers
(gol_dev_random_fill, _popcount, _hash, _pack, _unpack, _bytes_step) on caller memory, each against
the oracle or plain numpy.  Every parity test of the suite loads, counts, hashes and reads its board
back through these kernels, so an error two of them share, or one at an edge the engine never
presents, is invisible there; here each is alone.

Two rules hold for every case: every buffer has a row pitch larger than its width, with the padding
poisoned (inputs: all-ones words or byte 7, outputs: 0xA5), and an output's padding and every row
outside the written ones must come back as they were.  The shapes are the smallest that reach the
branch; SECOND_TRIP holds, per launcher, the threads of its largest grid (grid_for's cap x 256),
from which the one shape per kernel is made that sends some threads round the grid-stride loop again.

GOLHIP_SEQUENCE_LIBRARY names another build of the library to run the same cases on.
"""
import ctypes

import numpy as np
import pytest

import io_ref as IO
from oracle import oracle as O
from testlib import Guarded, env  # noqa: F401 (the fixture)

pytestmark = pytest.mark.gpu

SLOT_WORDS = 256 * 8  # GOL_COUNT_SLOTS * 8 uint64: "sum them all"
ONES32 = 0xFFFFFFFF
# threads of each launcher's largest grid (csrc/gol_util.hip: grid_for(n, 256, cap) of gol_launch.h, cap x 256)
SECOND_TRIP = {"random_fill": 256 * 64 * 256, "popcount": 256 * 16 * 256, "hash": 256 * 16 * 256,
               "pack": 256 * 64 * 256, "unpack": 256 * 64 * 256, "bytes_step_scalar": 256 * 16 * 256}
GROW0 = [0, 7, 1 << 33]


def dev(arr, off=0):
    """A numpy array in device memory, `off` bytes past a 16-byte boundary, between poisoned margins that read() finds untouched."""
    return Guarded(arr, fill=IO.OUT_POISON, off=off)


def ok(env, rc):
    assert rc == 0, env.L.gol_last_error()


def slots_sum(slots):
    return int(slots.read().sum(dtype=np.uint64))


def new_slots(env):
    return dev(np.zeros(SLOT_WORDS, dtype=np.uint64))


def rng_of(*key):
    return np.random.default_rng(list(key))


# ------------------------------------------------------------------ gol_dev_random_fill
FILL_SHAPES = [(1, 64), (5, 192), (3, 1024), (IO.second_trip_rows(SECOND_TRIP["random_fill"], 2050), 2050 * 64)]


def fill(env, out, row0, rows, grow0, W, pitch, seed):
    ok(env, env.L.gol_dev_random_fill(out.ptr + 4 * pitch * row0, rows, grow0, W, pitch, seed, None))


@pytest.mark.parametrize("grow0", GROW0)
@pytest.mark.parametrize("rows,W", FILL_SHAPES)
def test_random_fill_is_the_oracles_board(env, rows, W, grow0):
    Wd, pitch, seed = W // 32, W // 32 + 2, 0x9E3779B97F4A7C15 ^ rows
    out = dev(IO.poisoned(rows + 2, pitch, np.uint32))
    fill(env, out, 1, rows, grow0, W, pitch, seed)
    got, clean = IO.split_written(out.read(), 1, rows, Wd)
    assert clean
    assert np.array_equal(np.ascontiguousarray(got).view("<u8"), O.random_words(seed, grow0, rows, W // 64))


@pytest.mark.parametrize("grow0", GROW0)
def test_random_fill_in_two_calls_and_of_no_rows(env, grow0):
    H, W, seed = 5, 192, 77
    Wd, pitch = W // 32, W // 32 + 4
    for a in range(H + 1):  # a = 0 and a = H: one of the calls has no rows
        out = dev(IO.poisoned(H + 2, pitch, np.uint32))
        fill(env, out, 1, a, grow0, W, pitch, seed)
        fill(env, out, 1 + a, H - a, grow0 + a, W, pitch, seed)
        got, clean = IO.split_written(out.read(), 1, H, Wd)
        assert clean and np.array_equal(np.ascontiguousarray(got).view("<u8"), O.random_words(seed, grow0, H, W // 64)), a
    out = dev(IO.poisoned(2, pitch, np.uint32))
    fill(env, out, 1, 0, grow0, W, pitch, seed)
    assert IO.split_written(out.read(), 0, 0, 0)[1]


# ------------------------------------------------------------------ gol_dev_popcount
POP_SHAPES = [(5, 1), (7, 3), (4, 2), (9, 66), (IO.second_trip_rows(SECOND_TRIP["popcount"], 2101), 2101)]


@pytest.mark.parametrize("rows,Wd", POP_SHAPES)
def test_popcount_counts_the_words_and_not_the_padding(env, rows, Wd):
    L, pitch = env.L, Wd + 3
    words = rng_of(1, rows, Wd).integers(0, 1 << 32, (rows, Wd), dtype=np.uint32)
    want = int(np.unpackbits(words.view(np.uint8)).sum(dtype=np.int64))
    src = dev(IO.pitched(words, pitch, ONES32, 1, 1))
    slots = new_slots(env)
    ok(env, L.gol_dev_popcount(src.ptr + 4 * pitch, rows, Wd, pitch, slots.ptr, None))
    assert slots_sum(slots) == want
    ok(env, L.gol_dev_popcount(src.ptr + 4 * pitch, rows, Wd, pitch, slots.ptr, None))  # adds to the slots
    assert slots_sum(slots) == 2 * want
    ok(env, L.gol_dev_popcount(src.ptr + 4 * pitch, 0, Wd, pitch, slots.ptr, None))
    assert slots_sum(slots) == 2 * want
    if rows > 1:  # a part of the rows
        ok(env, L.gol_dev_popcount(src.ptr + 8 * pitch, rows - 1, Wd, pitch, slots.ptr, None))
        assert slots_sum(slots) == 3 * want - int(np.unpackbits(words[:1].view(np.uint8)).sum())


# ------------------------------------------------------------------ gol_dev_hash
HASH_SHAPES = [(7, 6), (5, 2), (IO.second_trip_rows(SECOND_TRIP["hash"], 2100), 4200)]


def dev_hash(env, words, grow0, pad=ONES32, slots=None, pitch=None):
    rows, Wd = words.shape
    pitch = pitch or Wd + 2
    src = dev(IO.pitched(words, pitch, pad, 1, 1))
    slots = slots or new_slots(env)
    ok(env, env.L.gol_dev_hash(src.ptr + 4 * pitch, rows, grow0, Wd, pitch, slots.ptr, None))
    return slots_sum(slots)


@pytest.mark.parametrize("grow0", GROW0)
@pytest.mark.parametrize("rows,Wd", HASH_SHAPES)
def test_hash_is_the_oracles(env, rows, Wd, grow0):
    words = rng_of(2, rows, Wd).integers(0, 1 << 32, (rows, Wd), dtype=np.uint32)
    assert dev_hash(env, words, grow0) == IO.hash_of(words, grow0)


@pytest.mark.parametrize("grow0", GROW0)
def test_hash_adds_over_splits_and_sees_rows_bits_and_no_padding(env, grow0):
    rows, Wd = 7, 6
    words = rng_of(3, grow0 % 1000).integers(0, 1 << 32, (rows, Wd), dtype=np.uint32)
    whole = IO.hash_of(words, grow0)
    assert dev_hash(env, words, grow0) == whole
    for cuts in [(a,) for a in range(1, rows)] + [(2, 5), (1, 2)]:
        slots = new_slots(env)
        edges = (0, *cuts, rows)
        for a, b in zip(edges, edges[1:]):  # each part with its own first global row, into the same slots
            got = dev_hash(env, words[a:b], grow0 + a, slots=slots)
        assert got == whole, cuts
    swapped = words.copy()
    swapped[[1, 4]] = words[[4, 1]]
    assert not np.array_equal(words[1], words[4])
    assert dev_hash(env, swapped, grow0) == IO.hash_of(swapped, grow0) != whole
    for y, w, b in ((0, 0, 0), (rows - 1, Wd - 1, 31), (3, 2, 17)):
        flipped = words.copy()
        flipped[y, w] ^= np.uint32(1 << b)
        assert dev_hash(env, flipped, grow0) == IO.hash_of(flipped, grow0) != whole
    assert dev_hash(env, words, grow0, pad=0) == dev_hash(env, words, grow0, pad=0x12345678, pitch=Wd + 6) == whole


# ------------------------------------------------------------------ gol_dev_pack
def dev_pack(env, board, stride, pitch, flag=True):
    """(bits written, output padding and outer rows untouched, *nonbinary or None)"""
    rows, W = board.shape
    src = dev(IO.pitched(board, stride, IO.PAD_BYTE, 1, 1))
    bits = dev(IO.poisoned(rows + 2, pitch, np.uint32))
    f = dev(np.zeros(1, dtype=np.uint32)) if flag else None
    ok(env, env.L.gol_dev_pack(src.ptr + stride, rows, W, stride, bits.ptr + 4 * pitch, pitch, f.ptr if f else None, None))
    got, clean = IO.split_written(bits.read(), 1, rows, W // 32)
    return got, clean, int(f.read()[0]) if f else None


@pytest.mark.parametrize("W", [32, 96, 2112])
def test_pack_sets_the_bit_of_255_only_and_flags_other_bytes_inside_the_board(env, W):
    rows, stride, pitch = 5, W + 5, W // 32 + 1
    board = IO.random_bytes(rng_of(4, W), rows, W)
    assert set(np.unique(board).tolist()) == set(IO.ODD_BYTES)
    got, clean, flag = dev_pack(env, board, stride, pitch)
    assert clean and np.array_equal(got, IO.bits_of_bytes(board)) and flag == 1
    binary = np.where(board == 255, 255, 0).astype(np.uint8)
    got, clean, flag = dev_pack(env, binary, stride, pitch)  # byte 7 in the padding only
    assert clean and np.array_equal(got, IO.bits_of_bytes(binary)) and flag == 0
    for y, x in ((0, 0), (rows - 1, W - 1)):
        for odd in (1, 254):
            one = binary.copy()
            one[y, x] = odd
            got, clean, flag = dev_pack(env, one, stride, pitch)
            assert clean and np.array_equal(got, IO.bits_of_bytes(one)) and flag == 1, (y, x, odd)
    got, clean, flag = dev_pack(env, board, stride, pitch, flag=False)  # nonbinary = NULL
    assert clean and np.array_equal(got, IO.bits_of_bytes(board)) and flag is None
    got, clean, flag = dev_pack(env, board[:0], stride, pitch)  # no rows
    assert clean and flag == 0


def test_pack_on_the_second_trip(env):
    W = 2112
    rows, stride, pitch = IO.second_trip_rows(SECOND_TRIP["pack"], W // 32), W + 5, W // 32 + 1
    base = IO.random_bytes(rng_of(5), 997, W, values=[0, 255])
    board = base[np.arange(rows) % 997]
    got, clean, flag = dev_pack(env, board, stride, pitch)
    assert clean and np.array_equal(got, IO.bits_of_bytes(board)) and flag == 0
    assert (rows - 1) * (W // 32) + W // 32 - 1 >= SECOND_TRIP["pack"]  # the last word is a second item
    board[rows - 1, W - 1] = 128
    got, clean, flag = dev_pack(env, board, stride, pitch)
    assert clean and flag == 1 and np.array_equal(got[-1], IO.bits_of_bytes(board[-1:])[0])


# ------------------------------------------------------------------ gol_dev_unpack
def dev_unpack(env, words, stride, off=0):
    rows, Wd = words.shape
    pitch = Wd + 1
    src = dev(IO.pitched(words, pitch, ONES32, 1, 1))
    out = dev(IO.poisoned(rows + 2, stride, np.uint8), off=off)
    ok(env, env.L.gol_dev_unpack(src.ptr + 4 * pitch, rows, 32 * Wd, pitch, out.ptr + stride, stride, None))
    got, clean = IO.split_written(out.read(), 1, rows, 32 * Wd)
    return got, clean, [(out.ptr + (1 + y) * stride) % 16 == 0 for y in range(rows)]


@pytest.mark.parametrize("pad", [16, 1])
@pytest.mark.parametrize("off", [0, 1, 4, 15])
@pytest.mark.parametrize("W", [32, 96])
def test_unpack_at_any_alignment_of_the_destination(env, W, off, pad):
    rows = 18
    words = rng_of(6, W, off, pad).integers(0, 1 << 32, (rows, W // 32), dtype=np.uint32)
    got, clean, aligned = dev_unpack(env, words, W + pad, off)
    assert clean and np.array_equal(got, IO.bytes_of_bits(words))
    if pad == 1:  # rows of both kinds: 16-byte stores and single bytes
        assert any(aligned) and not all(aligned)
    else:
        assert all(aligned) == (off == 0) and any(aligned) == (off == 0)


def test_pack_unpack_pack_round_trip(env):
    rows, W = 6, 96
    board = IO.random_bytes(rng_of(7), rows, W, values=[0, 255])
    bits, clean, flag = dev_pack(env, board, W + 5, W // 32 + 1)
    assert clean and flag == 0
    back, clean, _ = dev_unpack(env, np.ascontiguousarray(bits), W + 1, off=4)
    assert clean and np.array_equal(back, board)
    again, clean, flag = dev_pack(env, np.ascontiguousarray(back), W + 7, W // 32 + 2)
    assert clean and flag == 0 and np.array_equal(again, bits)


def test_unpack_on_the_second_trip(env):
    W = 2112
    rows = IO.second_trip_rows(SECOND_TRIP["unpack"], W // 32)
    base = rng_of(8).integers(0, 1 << 32, (997, W // 32), dtype=np.uint32)
    words = base[np.arange(rows) % 997]
    got, clean, aligned = dev_unpack(env, words, W + 16)
    assert clean and all(aligned) and np.array_equal(got, IO.bytes_of_bits(words))


# ------------------------------------------------------------------ gol_dev_bytes_step
def dev_bytes_step(env, src, board, stride, y0, y1, out_stride, out_off):
    H, W = board.shape
    out = dev(IO.poisoned(y1 - y0 + 2, out_stride, np.uint8), off=out_off)
    ok(env, env.L.gol_dev_bytes_step(src.ptr, H, W, stride, y0, y1, out.ptr + out_stride, out_stride, None))
    return IO.split_written(out.read(), 1, y1 - y0, W)


@pytest.mark.parametrize("H", [1, 2, 3, 40])
@pytest.mark.parametrize("W", [16, 48, 992, 1008, 33])
def test_bytes_step_vector_and_scalar_kernel_on_one_board(env, W, H):
    """The launcher takes the 16-bytes-per-lane kernel when W, both strides and both pointers are
    multiples of 16 and the one-thread-per-cell kernel otherwise: the same board through both.  (The
    input padding is 255 here, the byte a neighbour count would see.)"""
    board = IO.random_bytes(rng_of(9, W, H), H, W)
    a16 = (W + 15) // 16 * 16
    variants = [("aligned", a16 + 16, a16 + 32, 0, 0), ("input + 1", a16 + 16, a16 + 32, 1, 0),
                ("output + 1", a16 + 16, a16 + 32, 0, 1), ("strides", W + 5, W + 9, 0, 0)]
    slabs = sorted({(0, H), (0, 1), (H - 1, H), (H // 3, H // 3 + max(1, H // 2))})
    for name, stride, out_stride, in_off, out_off in variants:
        src = dev(IO.pitched(board, stride, 255), off=in_off)
        for y0, y1 in slabs:
            got, clean = dev_bytes_step(env, src, board, stride, y0, y1, out_stride, out_off)
            assert clean and np.array_equal(got, O.next_state_slab(board, y0, y1)), (name, y0, y1)


def test_bytes_step_scalar_kernel_on_the_second_trip(env):
    W = 1050
    H = IO.second_trip_rows(SECOND_TRIP["bytes_step_scalar"], W)
    board = IO.random_bytes(rng_of(10), H, W)
    src = dev(IO.pitched(board, W + 5, 255))
    got, clean = dev_bytes_step(env, src, board, W + 5, 0, H, W + 9, 0)
    assert clean and np.array_equal(got, O.next_state_slab(board, 0, H))


# ------------------------------------------------------------------ refusals
def test_bad_arguments_are_refused_before_any_launch(env):
    L = env.L
    src, dst = dev(IO.poisoned(64, 1024, np.uint8)), dev(IO.poisoned(64, 1024, np.uint8))
    slots, flag = dev(IO.poisoned(1, SLOT_WORDS, np.uint64)), dev(IO.poisoned(1, 1, np.uint32))
    s, d, sl = src.ptr, dst.ptr, slots.ptr
    tables = [  # launcher, arguments it accepts, single changes it must refuse
        (L.gol_dev_random_fill, dict(dst=d, rows=2, grow0=0, W=128, pitch=6, seed=1, stream=None),
         [dict(dst=None), dict(rows=-1), dict(grow0=-1), dict(W=0), dict(W=-64), dict(W=96), dict(W=32), dict(pitch=2),
          dict(pitch=5)]),
        (L.gol_dev_popcount, dict(src=s, rows=2, Wd=3, pitch=4, slots=sl, stream=None),
         [dict(src=None), dict(slots=None), dict(rows=-1), dict(Wd=0), dict(pitch=2)]),
        (L.gol_dev_hash, dict(src=s, rows=2, grow0=0, Wd=4, pitch=6, slots=sl, stream=None),
         [dict(src=None), dict(slots=None), dict(rows=-1), dict(grow0=-1), dict(Wd=0), dict(Wd=3), dict(pitch=2),
          dict(pitch=5)]),
        (L.gol_dev_pack, dict(bytes=s, rows=2, W=64, stride=70, bits=d, pitch=3, nonbinary=flag.ptr, stream=None),
         [dict(bytes=None), dict(bits=None), dict(rows=-1), dict(W=0), dict(W=48), dict(W=16), dict(stride=63),
          dict(pitch=1)]),
        (L.gol_dev_unpack, dict(bits=s, rows=2, W=64, pitch=3, bytes=d, stride=70, stream=None),
         [dict(bits=None), dict(bytes=None), dict(rows=-1), dict(W=0), dict(W=48), dict(W=16), dict(stride=63),
          dict(pitch=1)]),
        (L.gol_dev_bytes_step, dict(world=s, H=4, W=32, stride=48, y0=1, y1=3, out=d, out_stride=40, stream=None),
         [dict(world=None), dict(out=None), dict(H=0), dict(W=0), dict(stride=31), dict(out_stride=31), dict(y0=-1),
          dict(y1=5), dict(y0=3, y1=2)]),
    ]
    for fn, good, bad in tables:
        for change in bad:
            assert fn(*{**good, **change}.values()) == env.EINVAL, (fn.__name__, change)
            assert L.gol_last_error()
    for buf in (src, dst, slots, flag):  # nothing ran
        assert (buf.read().view(np.uint8) == IO.OUT_POISON).all()
    src2 = dev(np.zeros((64, 1024), dtype=np.uint8))
    zero = dev(np.zeros(SLOT_WORDS, dtype=np.uint64))
    for fn, good, _ in tables:  # and what the tables change is accepted
        good = {k: {s: src2.ptr, sl: zero.ptr}.get(v, v) if isinstance(v, int) else v for k, v in good.items()}
        ok(env, fn(*good.values()))
    env.torch.cuda.synchronize()


# ------------------------------------------------------------------ after the last launch
def test_no_device_fault_was_reported(env):
    env.torch.cuda.synchronize()
    flags = ctypes.c_uint32(1)
    assert env.L.gol_dev_error(-1, ctypes.byref(flags)) == 0 and flags.value == 0
