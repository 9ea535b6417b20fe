"""Region reads, the part that needs no GPU: the copy and bounds kernels' mapping on host buffers
(gol_copy_host, gol_bounds_host, csrc/gol_copy.h) against numpy for every layout, the contract of
the caller's buffer, copy -> paste as the identity, the ABI edges, and the same code in a stand-alone
program under AddressSanitizer + UndefinedBehaviorSanitizer (build/asan/copy_check, a plain child
process; nothing loaded into Python is sanitized).  All comparisons are exact; the reference is numpy
on the oracle's board (O.random_words / O.unpack), never the library."""
import ctypes
import os
import struct
import subprocess

import numpy as np

import region_ref as RR
from region_ref import CASES as PASTE_SHAPES, EDGES, board_cells, to_layout
from testlib import check_program, cpu_lib as G  # noqa: F401 (the fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (layout, W, x0, w, cells): the paste's shapes on the random board, then band rows with an odd number
# of 32-cell groups per band (W = 3072: Wd = 96), w = 63, 64, 65 at x0 % 64 = 31, one cell in the last
# bit of the last word, a rectangle without an alive cell, and one alive cell at each corner of a
# rectangle that wraps the seam -- the last two in every layout (bytes: both lane forms, by the pitch)
EXTRA = [(2, 3072, x0, w, "random") for x0, w in [(3000, 200), (95, 97), (0, 3072), (95, 63), (95, 64), (95, 65), (3071, 1),
                                                 (96, 96), (1, 3071), (2000, 3072), (31, 33)]]
EXTRA += [(2, 1024, 95, w, "random") for w in (63, 64, 65)] + [(2, 2048, 31, w, "random") for w in (63, 64, 65)]
EXTRA += [(2, 1024, 1023, 1, "last"), (2, 3072, 3071, 1, "last")]
for _lay, _W, _x0, _w in [(2, 1024, 1000, 50), (2, 3072, 3000, 200), (2, 1024, 700, 1024), (1, 192, 160, 70), (1, 192, 37, 192),
                          (0, 100, 90, 30), (0, 100, 37, 100), (0, 50, 45, 11)]:
    EXTRA += [(_lay, _W, _x0, _w, "empty"), (_lay, _W, _x0, _w, "corners")]
SHAPES = [(layout, W, x0, w, "random") for layout, W, x0, w in PASTE_SHAPES] + EXTRA
BROWS, ROW, ROWS, PROW = 6, 1, 4, 2


def region(cells, x0, w):
    """The rows [ROW, ROW + ROWS) x columns (x0 + c) mod W of the board's cells."""
    return cells[ROW:ROW + ROWS][:, (x0 + np.arange(w)) % cells.shape[1]]


def np_bounds(sub):
    """(cmin, cmax, rmin, rmax, alive) of a bool array, inclusive; empty: minima above maxima."""
    ys, xs = np.nonzero(sub)
    if len(ys) == 0:
        return sub.shape[1], -1, sub.shape[0], -1, 0
    return int(xs.min()), int(xs.max()), int(ys.min()), int(ys.max()), len(ys)


def cases(binary_bytes=False, shapes=SHAPES, pads=(0, 3)):
    """(args of gol_copy_host, buffer, the board's cells): every shape with a plain and a padded pitch
    (bytes: the one-byte and the 4-byte lane form) and a dense and a wider pattern stride."""
    rng = np.random.default_rng(17)
    for i, (layout, W, x0, w, kind) in enumerate(shapes):
        units = W if layout == 0 else W // 32
        for pad in pads if kind == "random" or layout == 0 else (0,):
            cells = board_cells(11 + i % 4, BROWS, W).copy()
            xs = (x0 + np.arange(w)) % W
            if kind == "empty":  # alive all around the rectangle, nothing inside
                cells[ROW:ROW + ROWS, xs] = False
            elif kind == "corners":
                cells[:] = False
                cells[np.ix_([ROW, ROW + ROWS - 1], [xs[0], xs[-1]])] = True
            elif kind == "last":
                cells[:] = False
                cells[ROW + 1, W - 1] = True
            buf = to_layout(layout, cells, units + pad, rng)
            if binary_bytes and layout == 0:
                buf[:, :W][buf[:, :W] != 0] = 255
            stride = (w + 63) // 64 + (i + pad) % 2
            yield (layout, W, units + pad, BROWS, ROW, ROWS, PROW, x0, w, stride), buf, cells


def pattern_block(args, fill=np.uint64(2 ** 64 - 1)):
    """A caller's pattern of exactly the words the call may write, all ones."""
    *_, rows, prow, x0, w, stride = args
    return np.full((prow + rows - 1) * stride + (w + 63) // 64, fill, np.uint64)


def check_pattern(args, flat, want):
    """The pattern rows [PROW, PROW + ROWS) hold `want` in words [0, ceil(w / 64)), tail bits zero;
    every other word of the block is still all ones."""
    *_, rows, prow, x0, w, stride = args
    pw = (w + 63) // 64
    full = np.concatenate([flat, np.zeros((prow + rows) * stride - len(flat), np.uint64)]).reshape(prow + rows, stride)
    got = np.unpackbits(np.ascontiguousarray(full[prow:, :pw]).view(np.uint8), axis=1, bitorder="little")
    assert np.array_equal(got[:, :w] != 0, want), args
    assert not got[:, w:].any(), args  # the bits at c >= w
    mask = np.ones(full.shape, bool)
    mask[prow:, :pw] = False
    mask = mask.reshape(-1)[:len(flat)]
    assert (flat[mask] == np.uint64(2 ** 64 - 1)).all(), args  # rows before prow, words past ceil(w / 64)


def test_copy_host_matches_numpy(G):
    assert {(0, False), (0, True)} <= run_copy_cases(G, cases())  # byte rows that allow aligned 4-byte words, and not


def run_copy_cases(G, cs):
    """gol_copy_host on each case against numpy; returns the (layout, rows 4-byte aligned) pairs seen."""
    L = G.lib()
    forms = set()
    for args, buf, cells in cs:
        layout, W, pitch, brows, row, rows, prow, x0, w, stride = args
        before = buf.copy()
        pat = pattern_block(args)
        alive = ctypes.c_int64(-1)
        rc = L.gol_copy_host(layout, buf.ctypes.data, pitch, W, row, rows, prow, x0, w, pat.ctypes.data, stride, ctypes.byref(alive))
        assert rc == 0, (args, L.gol_last_error())
        want = region(cells, x0, w)
        check_pattern(args, pat, want)
        assert alive.value == np.count_nonzero(want), args
        assert np.array_equal(buf, before)  # a read
        forms.add((layout, pitch % 4 == 0 and W % 4 == 0))
    return forms


def test_bounds_host_matches_numpy(G):
    L = G.lib()
    assert run_bounds_cases(G, cases()) >= 8
    args, buf, _ = list(cases())[-1]
    layout, W, pitch, brows, row, rows, prow, x0, w, stride = args
    assert L.gol_bounds_host(layout, buf.ctypes.data, pitch, W, row, rows, x0, w, None, None, None, None, None) == 0


def test_copy_and_bounds_host_at_the_geometry_edges(G):
    """test_edit_cpu.EDGES at a dense pitch, on the random board and with one alive cell at each
    corner of the rectangle: the copy's one-byte form and the bounds' 4-byte form of the 8-cell rows."""
    shapes = [(layout, W, x0, w, kind) for layout, W, x0, w in EDGES for kind in ("random", "corners")]
    assert all(buf.ctypes.data % 4 == 0 for _, buf, _ in cases(shapes=shapes, pads=(0,)))
    assert {(0, True), (0, False)} <= run_copy_cases(G, cases(shapes=shapes, pads=(0,)))  # W = 8 and W = 7
    run_bounds_cases(G, cases(shapes=shapes, pads=(0,)))


def run_bounds_cases(G, cs):
    """gol_bounds_host on each case against numpy; returns how many rectangles held no alive cell."""
    L = G.lib()
    n_empty = 0
    for args, buf, cells in cs:
        layout, W, pitch, brows, row, rows, prow, x0, w, stride = args
        v = [ctypes.c_int64(-7) for _ in range(5)]
        rc = L.gol_bounds_host(layout, buf.ctypes.data, pitch, W, row, rows, x0, w, *(ctypes.byref(x) for x in v))
        assert rc == 0, (args, L.gol_last_error())
        want = np_bounds(region(cells, x0, w))
        got = tuple(x.value for x in v)
        if want[4] == 0:
            n_empty += 1
            assert got[0] > got[1] and got[2] > got[3] and got[4] == 0, args
        else:
            assert got == want, args
    return n_empty


def test_copy_then_paste_is_the_identity(G):
    """gol_paste_host(COPY) of what gol_copy_host read, at the same place: every buffer byte for byte
    as it was (byte boards of 0 / 255: a paste writes alive cells as 255)."""
    L = G.lib()
    for args, buf, cells in cases(binary_bytes=True):
        layout, W, pitch, brows, row, rows, prow, x0, w, stride = args
        before = buf.copy()
        pat = pattern_block(args)
        assert L.gol_copy_host(layout, buf.ctypes.data, pitch, W, row, rows, prow, x0, w, pat.ctypes.data, stride, None) == 0
        changed = ctypes.c_int64(-1)
        assert L.gol_paste_host(layout, buf.ctypes.data, pitch, W, row, rows, prow, x0, w, pat.ctypes.data, stride, 0,
                                ctypes.byref(changed)) == 0
        assert changed.value == 0 and np.array_equal(buf, before), args


def test_copy_host_argument_errors(G):
    """The refusals every twin shares (region_ref.REFUSED), then those of the copy's own arguments."""
    L, E = G.lib(), G._lib
    buf, pat = RR.buffers()
    assert RR.bounds(L, buf) == 0
    for kw in RR.REFUSED:
        assert "at" in kw or RR.bounds(L, buf, **kw) == E.GOL_EINVAL, kw
        assert RR.copy(L, buf, pat, **kw) == E.GOL_EINVAL, kw
    for kw in (dict(stride=0), dict(w=65, stride=1), dict(pattern=False)):
        assert RR.copy(L, buf, pat, **kw) == E.GOL_EINVAL, kw
    assert (pat == 5).all() and not buf.any()
    assert RR.copy(L, buf, pat, stride=2) == 0 and pat.tolist() == [[0, 5], [0, 5]]  # words past ceil(w / 64) stay


def test_every_twin_refuses_the_same_regions(G):
    """One list for gol_paste_host, gol_copy_host and gol_bounds_host: each call of region_ref.ACCEPTED
    succeeds, each row of REFUSED is GOL_EINVAL from all three, and board and pattern are untouched."""
    L, E = G.lib(), G._lib
    for twin in (RR.paste, RR.copy, RR.bounds):
        for kw in RR.ACCEPTED:
            assert twin(L, *RR.buffers(), **kw) == 0, (twin.__name__, kw, L.gol_last_error())
        buf, pat = RR.buffers()
        for kw in RR.REFUSED:
            if twin is RR.bounds and "at" in kw:
                continue  # (its signature has no such argument)
            assert twin(L, buf, pat, **kw) == E.GOL_EINVAL, (twin.__name__, kw)
        assert not buf.any() and (pat == 5).all(), twin.__name__


def test_copy_abi_edges(G):
    """NULL handles are EINVAL, not a crash; the header's flag is the binding's."""
    L, E = G.lib(), G._lib
    n, lay, t = ctypes.c_int64(), ctypes.c_int32(), ctypes.c_int64()
    pat = np.zeros(1, np.uint64)
    box = [ctypes.c_int64() for _ in range(4)]
    assert L.gol_engine_copy(None, 0, 0, 1, 1, pat.ctypes.data, 1, 0, ctypes.byref(n), ctypes.byref(lay)) == E.GOL_EINVAL
    assert L.gol_engine_bounds(None, 0, 0, 1, 1, *(ctypes.byref(x) for x in box), ctypes.byref(n), ctypes.byref(lay)) == E.GOL_EINVAL
    assert L.gol_broker_copy(None, 0, 0, 1, 1, pat.ctypes.data, 1, 0, ctypes.byref(n), ctypes.byref(t)) == E.GOL_EINVAL
    assert L.gol_broker_bounds(None, 0, 0, 1, 1, *(ctypes.byref(x) for x in box), ctypes.byref(n), ctypes.byref(t)) == E.GOL_EINVAL
    text = open(os.path.join(ROOT, "include", "golhip.h")).read()
    assert "#define GOL_COPY_CUT %d\n" % E.GOL_COPY_CUT in text and E.GOL_COPY_CUT == 1
    assert "#define GOL_ABI_VERSION 6\n" in text


# ------------------------------------------------------------------ the same code under the sanitizers
def _run_check(mode, blob):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:exitcode=23", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1:exitcode=24")
    p = subprocess.run([check_program("copy_check"), mode], input=blob, env=env, capture_output=True, timeout=300)
    err = p.stderr.decode(errors="replace")
    assert p.returncode == 0 and "Sanitizer" not in err and "runtime error" not in err, err[-4000:]
    return p.stdout


def test_copy_host_under_asan_ubsan(G):
    """The shapes of test_copy_host_matches_numpy on exact-size heap buffers (the pattern block ends
    with the last word the call may write): no report, the cells and counts of numpy, and the
    driver's paste of the result back leaves the buffer as it was."""
    cs = list(cases(binary_bytes=True))
    blob = b"".join(struct.pack("<10q", *args) + buf.tobytes() for args, buf, _ in cs)
    out = _run_check("copy", blob)
    off = 0
    for args, buf, cells in cs:
        x0, w = args[7], args[8]
        n = len(pattern_block(args))
        rc, alive = struct.unpack_from("<2q", out, off)
        pat = np.frombuffer(out, np.uint64, n, off + 16)
        (rc2,) = struct.unpack_from("<q", out, off + 16 + 8 * n)
        after = np.frombuffer(out, buf.dtype, buf.size, off + 24 + 8 * n).reshape(buf.shape)
        off += 24 + 8 * n + buf.nbytes
        want = region(cells, x0, w)
        assert (rc, rc2, alive) == (0, 0, np.count_nonzero(want)), args
        check_pattern(args, pat, want)
        assert np.array_equal(after, buf), args
    assert off == len(out)


def test_bounds_host_under_asan_ubsan(G):
    cs = list(cases())
    blob = b""
    for args, buf, _ in cs:
        layout, W, pitch, brows, row, rows, prow, x0, w, stride = args
        blob += struct.pack("<8q", layout, W, pitch, brows, row, rows, x0, w) + buf.tobytes()
    out = _run_check("bounds", blob)
    assert len(out) == 48 * len(cs)
    for i, (args, buf, cells) in enumerate(cs):
        rc, *got = struct.unpack_from("<6q", out, 48 * i)
        want = np_bounds(region(cells, args[7], args[8]))
        assert rc == 0 and got[4] == want[4], args
        assert tuple(got) == want if want[4] else (got[0] > got[1] and got[2] > got[3]), args
