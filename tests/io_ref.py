"""Expectations shared by tests/test_gpu_util_kernels.py and tests/test_gpu_strides.py (a helper, not
a test; numpy only): buffers whose row pitch exceeds their width with poisoned padding, the bytes <->
bits mapping at any W % 32 == 0, cell lists under a capacity, and the shapes that reach a grid-stride
loop's second trip.  tests/test_io_ref_cpu.py checks them against the oracle.
"""
import numpy as np

from oracle import oracle as O

ODD_BYTES = [0, 255, 1, 7, 128, 254]  # what a loaded byte may be (engine_model.ODD_BYTES)
OUT_POISON = 0xA5                     # every byte of an output buffer before the call
PAD_BYTE = 7                          # input padding of byte rows: neither dead nor alive
POISON_I32 = np.frombuffer(bytes([OUT_POISON] * 4), dtype=np.int32)[0]


def all_ones(dtype):
    return np.iinfo(dtype).max


def pitched(payload, pitch, pad, before=0, after=0):
    """`payload` (rows, width) inside a (before + rows + after, pitch) array of `pad`."""
    rows, width = payload.shape
    assert pitch >= width
    buf = np.full((before + rows + after, pitch), pad, dtype=payload.dtype)
    buf[before:before + rows, :width] = payload
    return buf


def poisoned(rows, pitch, dtype):
    """An output buffer: (rows, pitch) elements, every byte OUT_POISON."""
    return np.full((rows, pitch * np.dtype(dtype).itemsize), OUT_POISON, dtype=np.uint8).view(dtype)


def split_written(buf, row0, rows, width):
    """(the rows x width window at row0, True if every byte outside it is still OUT_POISON)."""
    rest = np.ascontiguousarray(buf).view(np.uint8).copy()
    rest[row0:row0 + rows, :width * buf.dtype.itemsize] = OUT_POISON
    return buf[row0:row0 + rows, :width], bool((rest == OUT_POISON).all())


def random_bytes(rng, rows, W, values=ODD_BYTES, density=.5):
    """Dead cells 0; the others drawn from `values` without 0."""
    alive = np.array([v for v in values if v != 0], dtype=np.uint8)
    return np.where(rng.random((rows, W)) < density, rng.choice(alive, size=(rows, W)), 0).astype(np.uint8)


def bits_of_bytes(board):
    """(rows, W / 32) uint32: bit x % 32 of word x / 32 is (byte x == 255), the mapping of oracle.pack."""
    board = np.asarray(board, dtype=np.uint8)
    assert board.shape[1] % 32 == 0
    return np.ascontiguousarray(np.packbits(board == 255, axis=1, bitorder="little")).view("<u4")


def bytes_of_bits(words32):
    """The inverse on a 0/255 board, through oracle.unpack (which takes W % 64 == 0: an odd word
    count is padded with one dead word and cut again)."""
    words32 = np.ascontiguousarray(words32, dtype="<u4")
    rows, Wd = words32.shape
    even = np.zeros((rows, Wd + Wd % 2), dtype="<u4")
    even[:, :Wd] = words32
    return O.unpack(even.view("<u8"))[:, :32 * Wd]


def hash_of(words32, grow0):
    """oracle.hash_words of (rows, Wd) uint32 rows, Wd even."""
    return O.hash_words(np.ascontiguousarray(words32, dtype="<u4").view("<u8"), grow0)


def alive_xy(board):
    """(n, 2) int32 (x, y) of the cells != 0, row-major: oracle.alive_cells as an array."""
    ys, xs = np.nonzero(np.asarray(board))
    return np.stack([xs, ys], axis=1).astype(np.int32).reshape(-1, 2)


def flips_xy(prev, cur):
    """(n, 2) int32 (x, y) of the cells whose alive state differs: oracle.flipped_cells as an array."""
    return alive_xy((np.asarray(prev) != 0) != (np.asarray(cur) != 0))


def capped(xy, cap, room):
    """The caller's (room, 2) int32 buffer, poisoned before the call, after a list call with `cap`:
    the first min(n, cap) pairs of `xy`, the rest untouched."""
    buf = np.full((room, 2), POISON_I32, dtype=np.int32)
    m = min(len(xy), cap)
    buf[:m] = xy[:m]
    return buf


def caps_for(xy, shard0_rows, extra=5):
    """The capacities at which a running cap can go wrong: 1, the cells of row 0, those of shard
    0's rows, one more, all but one, all, more than all (in this order, without repeats; 0 is the
    caller's, with xy = NULL)."""
    total = len(xy)
    row0 = int((xy[:, 1] == 0).sum())
    shard0 = int((xy[:, 1] < shard0_rows).sum())
    caps = []
    for c in (1, row0, shard0, shard0 + 1, total - 1, total, total + extra):
        if c >= 0 and c not in caps:
            caps.append(c)
    return caps


def second_trip_rows(threads, units):
    """Rows of `units` loop items each for a grid-stride launch of `threads` threads: the fewest that
    give some threads a second item, with a count of such threads that is no multiple of a wave."""
    rows = threads // units + 1
    while (rows * units - threads) % 64 == 0:
        rows += 1
    assert 0 < rows * units - threads < threads
    return rows


def seam_ranges(H, seams):
    """Row ranges [y0, y1) around the first rows `seams` of the shards (0 among them) and the board's
    end: those that start or end on a seam, one row either side of it, all rows, and an empty one."""
    out = [(0, H), (H // 2, H // 2)]
    for s in sorted(set(seams) | {H}):
        for y0, y1 in ((s, s + 3), (s - 3, s), (s - 1, s + 1), (s - 1, s), (s, s + 1), (s - 2, s + 5)):
            y0, y1 = max(y0, 0), min(y1, H)
            if y0 < y1 and (y0, y1) not in out:
                out.append((y0, y1))
    return out
