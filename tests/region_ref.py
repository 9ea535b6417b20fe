"""What the region twins must refuse (csrc/gol_edit.h, gol_region_ok): one list for gol_paste_host,
gol_copy_host and gol_bounds_host, which fill a gol_region from their arguments and ask the one
check the kernels' launchers ask.  A row names what it changes in DEFAULT by the descriptor's member
(`at`: prow of the paste and the copy; gol_bounds_host's signature has no such argument, so that one
row cannot be put to it).  Every row differs from a call that succeeds (ACCEPTED) in one clause.

Below the twins' callers: the boards, layouts and shapes the CPU tests of the paste and the copy share, and the
numpy references with which the GPU tests edit, read, cut and view an engine's board (random_cells keeps each
oracle board once, in _boards, for every module that asks)."""
import numpy as np

from oracle import oracle as O

DEFAULT = dict(layout=2, base=True, pitch=32, W=1024, x0=0, w=10, row=0, rows=2, at=0)
ACCEPTED = [dict(), dict(layout=1), dict(layout=0, W=128, pitch=128)]
REFUSED = [
    dict(layout=-1), dict(layout=3),                                           # the layout's range
    dict(layout=0, W=128, pitch=127), dict(layout=1, pitch=31), dict(pitch=31),  # a pitch one under the layout's units
    dict(W=1000), dict(layout=1, W=100),                                       # the layout's width rule
    dict(row=-1), dict(rows=-1), dict(at=-1),
    dict(x0=-1), dict(x0=1024), dict(w=0), dict(w=1025),
    dict(base=False),                                                          # NULL
]


def buffers():
    """(a board of 2 rows x 32 words of zeros, a pattern of 2 rows x 2 words of fives)."""
    return np.zeros((2, 32), np.uint32), np.full((2, 2), 5, np.uint64)


def _args(buf, kw):
    a = dict(DEFAULT, **kw)
    a["base"] = buf.ctypes.data if a["base"] else None
    return a


def paste(L, buf, pat, stride=1, op=0, pattern=True, **kw):
    a = _args(buf, kw)
    return L.gol_paste_host(a["layout"], a["base"], a["pitch"], a["W"], a["row"], a["rows"], a["at"], a["x0"], a["w"],
                            pat.ctypes.data if pattern else None, stride, op, None)


def copy(L, buf, pat, stride=1, pattern=True, **kw):
    a = _args(buf, kw)
    return L.gol_copy_host(a["layout"], a["base"], a["pitch"], a["W"], a["row"], a["rows"], a["at"], a["x0"], a["w"],
                           pat.ctypes.data if pattern else None, stride, None)


def bounds(L, buf, pat=None, **kw):
    a = _args(buf, kw)
    assert a["at"] == 0, "gol_bounds_host takes no `at`"
    return L.gol_bounds_host(a["layout"], a["base"], a["pitch"], a["W"], a["row"], a["rows"], a["x0"], a["w"],
                             None, None, None, None, None)


# ------------------------------------------------------------------ the paste twin's boards and shapes (CPU tests)
def board_cells(seed, rows, W):
    """rows x W bool cells of the oracle's random board (a width that is no multiple of 64: cut)."""
    return O.unpack(O.random_words(seed, 0, rows, (W + 63) // 64))[:, :W] != 0


def to_layout(layout, cells, pitch, rng):
    """The cells as a host buffer in `layout` with row pitch `pitch`; the pad units hold garbage."""
    rows, W = cells.shape
    if layout == 0:
        buf = rng.integers(0, 256, (rows, pitch), dtype=np.uint8)
        # alive cells as 255 or another non-zero byte: the untouched ones must keep it
        buf[:, :W] = np.where(cells, np.where(rng.random((rows, W)) < 0.3, 7, 255), 0)
        return buf
    Wd = W // 32
    buf = rng.integers(0, 2 ** 32, (rows, pitch), dtype=np.uint32)
    grouped = cells.reshape(rows, Wd, 32) if layout == 1 else cells.reshape(rows, 32, Wd).transpose(0, 2, 1)
    buf[:, :Wd] = np.packbits(grouped, axis=2, bitorder="little").view("<u4")[:, :, 0]
    return buf


def from_layout(layout, buf, W):
    rows = buf.shape[0]
    if layout == 0:
        return buf[:, :W] != 0
    Wd = W // 32
    bits = np.unpackbits(np.ascontiguousarray(buf[:, :Wd]).view(np.uint8).reshape(rows, Wd, 4), axis=2,
                         bitorder="little").reshape(rows, Wd, 32).astype(bool)
    return bits.reshape(rows, W) if layout == 1 else bits.transpose(0, 2, 1).reshape(rows, W)


# (layout, W, [(x0, w)]): band w = 1, w < Wd, w = Wd, Wd < w < W, w = W, x0 in band 0 and band 31, wraps in x;
# standard x0 % 32 in {0, 1, 31}, w = W at x0 % 32 != 0, w <= 32 inside one word; bytes W = 100, 128 (one byte
# per lane, or with a pitch that is a multiple of 4 aligned 4-byte words: both, see paste_cases) and W = 50
SHAPES = [
    (2, 1024, [(0, 1), (5, 1), (1023, 1), (3, 20), (30, 32), (17, 32), (10, 100), (0, 1024), (700, 1024), (1000, 40),
               (995, 29), (1023, 33), (31, 993)]),
    (2, 2048, [(2047, 1), (60, 10), (1, 64), (63, 64), (2000, 100), (100, 1900), (1999, 2048), (0, 2048), (2040, 65)]),
    (1, 192, [(0, 192), (1, 192), (31, 192), (37, 192), (0, 32), (1, 31), (33, 5), (31, 1), (31, 2), (64, 64),
              (65, 100), (191, 3), (160, 33), (95, 97), (1, 191)]),
    (0, 100, [(0, 100), (99, 1), (99, 100), (37, 64), (50, 70), (3, 5)]),
    (0, 128, [(0, 128), (127, 2), (1, 127), (64, 65), (2, 128), (6, 3)]),
    (0, 50, [(49, 50), (3, 5), (0, 50)]),
]
CASES = [(layout, W, x0, w) for layout, W, xs in SHAPES for x0, w in xs]
# The smallest shapes at which the unit step the kernels share with the host (gol_edit_paste_unit, the
# bounds' gol_copy_occ_unit) can go wrong, each at a dense pitch: standard rows of 2 words with the
# full width from the middle of a word (wrap_c: lane 0 also takes the cells that wrapped); byte rows
# of 2 aligned 4-byte words, the same wrap in the 4-byte form; byte rows of 7 bytes, one per lane;
# band rows with the carry into the next band and the wrap from bit 31 to bit 0.
EDGES = [(1, 64, 33, 64), (0, 8, 3, 8), (0, 7, 5, 7), (2, 1024, 1023, 34)]


# ------------------------------------------------------------------ edits, reads, cuts and views of an engine's board (GPU tests)
SEED = 11
_boards = {}


def random_cells(H, W, turns, seed=SEED):
    """The oracle's board of load_random(seed) after `turns` turns as bool cells (computed once)."""
    key = (H, W, turns, seed)
    if key not in _boards:
        cells = O.unpack(O.bits_run(O.random_words(seed, 0, H, W // 64), turns)) != 0
        cells.setflags(write=False)
        _boards[key] = cells
    return _boards[key]


def words_of(cells):
    return O.pack(cells.astype(np.uint8) * 255)


def np_paste(cells, x0, y0, p, op):
    """(edited cells, cells changed, mask of written cells): pattern cell (c, r) lands on
    ((x0 + c) mod W, (y0 + r) mod H)."""
    H, W = cells.shape
    p = np.asarray(p) != 0
    ix = np.ix_((y0 + np.arange(p.shape[0])) % H, (x0 + np.arange(p.shape[1])) % W)
    old = cells[ix]
    new = {"copy": p, "or": old | p, "xor": old ^ p, "andnot": old & ~p}[op]
    out = cells.copy()
    out[ix] = new
    written = np.zeros_like(cells)
    written[ix] = True if op == "copy" else p
    return out, int(np.count_nonzero(new != old)), written


def apply_edits(e, cells, edits, layout, turn):
    """Each edit (x0, y0, w, h, op, pattern seed or None = fill) on engine and numpy board alike."""
    for x0, y0, w, h, op, seed in edits:
        if seed is None:
            p = np.ones((h, w), bool)
            n, lay = e.fill(x0, y0, w, h, op, return_layout=True)
        else:
            p = np.random.default_rng(seed).random((h, w)) < 0.5
            n, lay = e.paste(p, x0, y0, op, return_layout=True)
        cells, want, _ = np_paste(cells, x0, y0, p, op)
        assert (n, lay, e.turn) == (want, layout, turn), (x0, y0, w, h, op)
    return cells


BYTE_EDITS = [(90, 45, 30, 10, "copy", 1), (0, 0, 100, 3, "xor", 2), (99, 49, 2, 2, "or", 3), (13, 20, 64, 7, "andnot", 4),
              (50, 10, 70, 5, "xor", None)]


def np_region(cells, x0, y0, w, h):
    """Rectangle cell (c, r) = board cell ((x0 + c) mod W, (y0 + r) mod H)."""
    H, W = cells.shape
    return cells[np.ix_((y0 + np.arange(h)) % H, (x0 + np.arange(w)) % W)]


def np_box(sub):
    """(bx, by, bw, bh, alive) of a bool array: the header's box, all zero without an alive cell."""
    ys, xs = np.nonzero(sub)
    if len(ys) == 0:
        return 0, 0, 0, 0, 0
    return int(xs.min()), int(ys.min()), int(xs.max() - xs.min() + 1), int(ys.max() - ys.min() + 1), len(ys)


def check_reads(e, cells, rects, layout):
    """copy, copy_words and bounds of every rectangle against numpy."""
    for x0, y0, w, h in rects:
        want = np_region(cells, x0, y0, w, h)
        got, lay = e.copy(x0, y0, w, h, return_layout=True)
        assert lay == layout and got.shape == (h, w) and got.dtype == bool, (x0, y0, w, h)
        assert np.array_equal(got, want), (x0, y0, w, h)
        words, alive = e.copy_words(x0, y0, w, h)
        assert alive == np.count_nonzero(want) and words.shape == (h, (w + 63) // 64), (x0, y0, w, h)
        bits = np.unpackbits(words.view(np.uint8), axis=1, bitorder="little")
        assert np.array_equal(bits[:, :w] != 0, want) and not bits[:, w:].any(), (x0, y0, w, h)
        assert e.bounds(x0, y0, w, h) == np_box(want), (x0, y0, w, h)


def apply_cuts(e, cells, rects, layout):
    for x0, y0, w, h in rects:
        want = np_region(cells, x0, y0, w, h)
        words, alive, lay = e.copy_words(x0, y0, w, h, cut=True, return_layout=True)
        assert np.array_equal(np.unpackbits(words.view(np.uint8), axis=1, bitorder="little")[:, :w] != 0, want), (x0, y0, w, h)
        cells, cleared, _ = np_paste(cells, x0, y0, np.ones((h, w), bool), "andnot")
        assert (alive, lay) == (cleared, layout) and cleared == np.count_nonzero(want), (x0, y0, w, h)
    return cells


def ref_counts(board, x0, y0, scale, out_w, out_h):
    """n(i, j) of the issue's definition on a byte board (alive = byte != 0)."""
    rows = np.take(board, y0 + np.arange(out_h * scale), axis=0, mode="wrap")
    box = np.take(rows, x0 + np.arange(out_w * scale), axis=1, mode="wrap") != 0
    return box.reshape(out_h, scale, out_w, scale).sum(axis=(1, 3)).astype(np.uint32)


def ref_pixels(counts, scale):
    s2 = scale * scale
    return ((255 * counts.astype(np.int64) + s2 - 1) // s2).astype(np.uint8)


def check_view(e, board, view, layout=None):
    """Counts and pixels of `view` on engine e against the numpy reference on `board`."""
    want = ref_counts(board, *view)
    got, lay = e.view_counts(*view, return_layout=True)
    assert got.dtype == np.uint32 and got.shape == (view[4], view[3])
    bad = np.argwhere(got != want)
    assert bad.size == 0, f"view {view}: {len(bad)} counts differ, first (j, i) = {bad[0]}: {got[tuple(bad[0])]} != {want[tuple(bad[0])]}"
    pix, lay2 = e.view(*view, return_layout=True)
    assert pix.dtype == np.uint8 and np.array_equal(pix, ref_pixels(want, view[2])), f"view {view}: pixels differ"
    assert lay == lay2
    if layout is not None:
        assert lay == layout
    return got, pix
