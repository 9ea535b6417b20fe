"""Board edits, the part that needs no GPU: the RLE codec (gol_rle_parse / gol_rle_format), the
paste kernels' word function on host buffers (gol_paste_host, csrc/gol_edit.h) against numpy for
every layout and operation, the ABI edges, and the same code in a stand-alone program under
AddressSanitizer + UndefinedBehaviorSanitizer (build/asan/rle_check, a plain child process; nothing
loaded into Python is sanitized).  All comparisons are exact; the reference is numpy on the
oracle's board (O.random_words / O.unpack), never the library."""
import ctypes
import os
import struct
import subprocess

import numpy as np
import pytest

import region_ref as RR
from region_ref import CASES, EDGES, board_cells, from_layout, to_layout
from testlib import check_program, cpu_lib as G  # noqa: F401 (the fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OPS = ["copy", "or", "xor", "andnot"]
GLIDER = np.array([[0, 1, 0], [0, 0, 1], [1, 1, 1]], bool)


# ------------------------------------------------------------------ RLE parse
def test_rle_parses_the_glider_with_and_without_a_rule(G):
    cells, rule = G.parse_rle("x = 3, y = 3, rule = B3/S23\nbob$2bo$3o!\n")
    assert np.array_equal(cells, GLIDER) and rule == "B3/S23"
    cells, rule = G.parse_rle("x = 3, y = 3\nbob$2bo$3o!")
    assert np.array_equal(cells, GLIDER) and rule == ""
    cells, rule = G.parse_rle("x=3,y=3,rule=b36/s23  \nbob$2bo$3o!")  # free blanks; the rule verbatim
    assert np.array_equal(cells, GLIDER) and rule == "b36/s23"


def test_rle_parse_forms(G):
    # comment lines, an upper-case header, a body broken across lines (also inside a token)
    text = "#N Glider\n#C a comment\nX = 3, Y = 3\nbo\nb$2b\no$3\no!"
    assert np.array_equal(G.parse_rle(text)[0], GLIDER)
    # 3$: two empty rows; rows shorter than x are dead to the right; text after '!' is ignored
    cells = G.parse_rle("x = 4, y = 5\no3$2o$o!this is ignored $$ x y z 0o")[0]
    want = np.zeros((5, 4), bool)
    want[0, 0] = want[3, 0] = want[3, 1] = want[4, 0] = True
    assert np.array_equal(cells, want)
    # a '$' may close the last row; a wide row crosses a 64-bit word
    cells = G.parse_rle("x = 70, y = 1\n63b3o4b$!")[0]
    assert cells.shape == (1, 70) and np.flatnonzero(cells[0]).tolist() == [63, 64, 65]
    assert np.array_equal(G.parse_rle(b"x = 1, y = 1\n!")[0], np.zeros((1, 1), bool))


MALFORMED = {
    "no header": "bob$2bo$3o!",
    "no header at all": "",
    "header without y": "x = 3\nbob!",
    "x < 1": "x = 0, y = 3\n!",
    "y < 1": "x = 3, y = 0\n!",
    "negative x": "x = -3, y = 3\n!",
    "x * y > 2^26": "x = 8193, y = 8192\n!",
    "x overflows": "x = 99999999999999999999, y = 1\n!",
    "multi-state": "x = 3, y = 3\nbob$2bA$3o!",
    "upper-case tag": "x = 3, y = 3\nbOb!",
    "other character": "x = 3, y = 3\nbob$2b.$3o!",
    "count of 0": "x = 3, y = 3\n0o!",
    "count overflows": "x = 3, y = 3\n99999999999999999999999o!",
    "run past x": "x = 3, y = 3\n4o!",
    "run past x after cells": "x = 3, y = 3\n2b2o!",
    "rows past y": "x = 3, y = 3\no$o$o$o!",
    "rows past y by count": "x = 3, y = 3\no4$!",
    "missing !": "x = 3, y = 3\nbob$2bo$3o",
    "count then end": "x = 3, y = 3\nbob$2",
    "count before !": "x = 3, y = 3\nbob$2!",
}


@pytest.mark.parametrize("name", sorted(MALFORMED))
def test_rle_malformed_is_eformat(G, name):
    with pytest.raises(G.GolError) as ei:
        G.parse_rle(MALFORMED[name])
    assert ei.value.code == G._lib.GOL_EFORMAT, str(ei.value)
    assert "offset" in str(ei.value)


def test_rle_parse_argument_errors(G):
    L, E = G.lib(), G._lib
    text = b"x = 65, y = 2\n65o$65o!"
    w, h = ctypes.c_int64(), ctypes.c_int64()
    pat = np.zeros((2, 2), np.uint64)
    args = (text, len(text), ctypes.byref(w), ctypes.byref(h))
    assert L.gol_rle_parse(*args, None, 0, 0, None, 0) == 0 and (w.value, h.value) == (65, 2)  # the two-call form
    assert L.gol_rle_parse(*args, pat.ctypes.data, 1, 2, None, 0) == E.GOL_EINVAL  # stride < ceil(65 / 64)
    assert L.gol_rle_parse(*args, pat.ctypes.data, 2, 1, None, 0) == E.GOL_EINVAL  # cap_rows < y
    assert L.gol_rle_parse(*args, pat.ctypes.data, 2, 2, None, 0) == 0
    assert pat.tolist() == [[2 ** 64 - 1, 1]] * 2
    assert L.gol_rle_parse(None, 0, ctypes.byref(w), ctypes.byref(h), None, 0, 0, None, 0) == E.GOL_EINVAL
    assert L.gol_rle_parse(text, len(text), None, None, None, 0, 0, None, 0) == E.GOL_EINVAL
    rule = ctypes.create_string_buffer(3)
    t2 = b"x = 1, y = 1, rule = B3/S23\no!"
    assert L.gol_rle_parse(t2, len(t2), ctypes.byref(w), ctypes.byref(h), None, 0, 0, rule, 3) == E.GOL_EINVAL
    # text[0, len) only: the '!' beyond len does not count
    assert L.gol_rle_parse(text, len(text) - 1, ctypes.byref(w), ctypes.byref(h), None, 0, 0, None, 0) == E.GOL_EFORMAT


# ------------------------------------------------------------------ RLE format
@pytest.mark.parametrize("w", [1, 63, 64, 65, 200])
@pytest.mark.parametrize("h", [1, 5])
def test_rle_format_round_trips(G, w, h):
    rng = np.random.default_rng(1000 * h + w)
    for density in (0.5, 0.05, 0.0, 1.0):
        p = rng.random((h, w)) < density
        for rule in (None, "B36/S23"):
            text = G.format_rle(p, rule)
            lines = text.split("\n")
            assert text.endswith("!\n") and max(len(ln) for ln in lines) <= 70
            assert lines[0] == f"x = {w}, y = {h}" + (f", rule = {rule}" if rule else "")
            back, r = G.parse_rle(text)
            assert np.array_equal(back, p) and r == (rule or "")


def test_rle_format_is_compact_and_checks_its_buffer(G):
    L, E = G.lib(), G._lib
    p = np.zeros((6, 5), bool)
    p[0, :3] = True
    p[4, 1] = True
    assert G.format_rle(p) == "x = 5, y = 6\n3o4$bo!\n"  # trailing dead cells dropped, empty rows merged
    assert G.format_rle(GLIDER, "B3/S23") == "x = 3, y = 3, rule = B3/S23\nbo$2bo$3o!\n"
    words = G._lib.pack_pattern(p)
    need = ctypes.c_int64()
    assert L.gol_rle_format(words.ctypes.data, 1, 5, 6, None, None, 0, ctypes.byref(need)) == 0  # the two-call form
    assert need.value == len("x = 5, y = 6\n3o4$bo!\n") + 1
    buf = ctypes.create_string_buffer(need.value)
    n2 = ctypes.c_int64()
    assert L.gol_rle_format(words.ctypes.data, 1, 5, 6, None, buf, need.value - 1, ctypes.byref(n2)) == E.GOL_EINVAL
    assert n2.value == need.value
    assert L.gol_rle_format(words.ctypes.data, 1, 5, 6, None, buf, need.value, None) == 0
    assert buf.value == b"x = 5, y = 6\n3o4$bo!\n"
    assert L.gol_rle_format(words.ctypes.data, 0, 5, 6, None, buf, need.value, None) == E.GOL_EINVAL  # stride
    assert L.gol_rle_format(words.ctypes.data, 1, 0, 6, None, buf, need.value, None) == E.GOL_EINVAL
    assert L.gol_rle_format(words.ctypes.data, 1, 5, 6, b"a\nb", buf, need.value, None) == E.GOL_EINVAL


# ------------------------------------------------------------------ gol_paste_host against numpy
def np_paste(cells, row, rows, x0, p, op):
    """The edited cells and the mask of written cells (numpy restatement of the header's rules)."""
    out = cells.copy()
    xs = (x0 + np.arange(p.shape[1])) % cells.shape[1]
    old = cells[row:row + rows][:, xs]
    new = {"copy": p, "or": old | p, "xor": old ^ p, "andnot": old & ~p}[op]
    out[row:row + rows, xs] = new
    written = np.zeros_like(cells)
    written[row:row + rows, xs] = True if op == "copy" else p
    return out, written


def pattern_words(G, p, stride, rng):
    """p as pattern rows of `stride` words whose bits past w (and pad words) hold garbage."""
    h, w = p.shape
    words = rng.integers(0, 2 ** 63, (h, stride), dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, (h, stride), dtype=np.uint64)
    packed = G._lib.pack_pattern(p)
    pw = packed.shape[1]
    words[:, :pw] = packed
    if w % 64:
        words[:, pw - 1] |= rng.integers(0, 2 ** 63, h, dtype=np.uint64) << np.uint64(w % 64)
    return words


def paste_cases(G, cases=CASES, pad=None):
    """Every shape x op x {pattern, NULL pattern}: (args of gol_paste_host, buffer, pattern words or
    None, expected buffer cells, expected written mask, expected changed).  pad: the units a row
    has past its last one (None: 0 and 3 in turn)."""
    rng = np.random.default_rng(7)
    for layout, W, x0, w in cases:
        units = W if layout == 0 else W // 32
        for i, op in enumerate(OPS):
            for null in (False, True):
                brows, row, rows, prow = 5, 1, 3, 2
                pitch = units + ((0 if (i + null) % 2 else 3) if pad is None else pad)
                cells = board_cells(11 + i, brows, W)
                buf = to_layout(layout, cells, pitch, rng)
                p_all = np.ones((prow + rows, w), bool) if null else rng.random((prow + rows, w)) < 0.5
                stride = (w + 63) // 64 + (i % 2)
                words = None if null else pattern_words(G, p_all, stride, rng)
                want, written = np_paste(cells, row, rows, x0, p_all[prow:], op)
                yield ((layout, W, pitch, brows, row, rows, prow, x0, w, stride, i), buf, words, cells, want, written)


def check_result(layout, W, before, after, cells, want, written):
    units = W if layout == 0 else W // 32
    assert np.array_equal(from_layout(layout, after, W), want)
    assert np.array_equal(after[:, units:], before[:, units:])  # the pad units are never written
    if layout == 0:  # written cells are 0 / 255; the others keep their byte, whatever it was
        a, b = after[:, :W], before[:, :W]
        assert np.array_equal(a[~written], b[~written])
        assert set(np.unique(a[written]).tolist()) <= {0, 255}
    return int(np.count_nonzero(want != cells))


def run_paste_cases(G, cases):
    """gol_paste_host on each case against numpy; returns how many ran."""
    L = G.lib()
    n = 0
    for args, buf, words, cells, want, written in cases:
        layout, W, pitch, brows, row, rows, prow, x0, w, stride, op = args
        after = buf.copy()
        changed = ctypes.c_int64(-1)
        rc = L.gol_paste_host(layout, after.ctypes.data, pitch, W, row, rows, prow, x0, w,
                              None if words is None else words.ctypes.data, stride, op, ctypes.byref(changed))
        assert rc == 0, (args, L.gol_last_error())
        assert changed.value == check_result(layout, W, buf, after, cells, want, written), args
        n += 1
    return n


def test_paste_host_matches_numpy(G):
    assert run_paste_cases(G, paste_cases(G)) == len(CASES) * 8


def test_paste_host_at_the_geometry_edges(G):
    """EDGES under ops 0..3, with a pattern and without: the byte rows of 8 cells take the 4-byte
    form (W, the dense pitch and the buffer are 4-byte aligned), those of 7 the one-byte form."""
    cases = list(paste_cases(G, EDGES, pad=0))
    assert all(buf.ctypes.data % 4 == 0 for _, buf, *_ in cases)
    assert run_paste_cases(G, cases) == len(EDGES) * 8


def test_paste_host_argument_errors(G):
    """The refusals every twin shares (region_ref.REFUSED), then those of the paste's own arguments."""
    L, E = G.lib(), G._lib
    buf, _ = RR.buffers()
    pat = np.zeros((2, 1), np.uint64)
    assert RR.paste(L, buf, pat) == 0
    for bad in RR.REFUSED + [dict(stride=0), dict(op=4), dict(op=-1)]:
        assert RR.paste(L, buf, pat, **bad) == E.GOL_EINVAL, bad
    assert not buf.any() and not pat.any()


def test_paste_abi_edges(G):
    """NULL handles are EINVAL, not a crash."""
    L, E = G.lib(), G._lib
    n, lay, t = ctypes.c_int64(), ctypes.c_int32(), ctypes.c_int64()
    assert L.gol_engine_paste(None, 0, 0, 1, 1, None, 0, 0, ctypes.byref(n), ctypes.byref(lay)) == E.GOL_EINVAL
    assert L.gol_broker_paste(None, 0, 0, 1, 1, None, 0, 0, ctypes.byref(n), ctypes.byref(t)) == E.GOL_EINVAL
    assert E.PASTE_OPS == {"copy": 0, "or": 1, "xor": 2, "andnot": 3}
    text = open(os.path.join(ROOT, "include", "golhip.h")).read()
    for name, v in E.PASTE_OPS.items():
        assert "#define GOL_PASTE_%s" % name.upper() in text and getattr(E, "GOL_PASTE_" + name.upper()) == v


# ------------------------------------------------------------------ the same code under the sanitizers
def _run_check(mode, blob):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:exitcode=23", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1:exitcode=24")
    p = subprocess.run([check_program("rle_check"), mode], input=blob, env=env, capture_output=True, timeout=300)
    err = p.stderr.decode(errors="replace")
    assert p.returncode == 0 and "Sanitizer" not in err and "runtime error" not in err, err[-4000:]
    return p.stdout


def test_rle_codec_under_asan_ubsan(G):
    """The malformed texts, every truncation of valid texts and seeded random patterns through the
    stand-alone driver: each verdict equals the library's, and valid texts survive format + parse."""
    rng = np.random.default_rng(3)
    valid = ["#C c\nx = 3, y = 3, rule = B3/S23\nbob$2bo$3o!\n", "X = 70 , Y = 4\n63b3o4b3$\n70o!tail",
             G.format_rle(rng.random((5, 200)) < 0.5, "B36/S23"), G.format_rle(rng.random((1, 65)) < 0.5)]
    texts = [t.encode() for t in valid] + [t.encode() for t in MALFORMED.values()]
    for t in valid:
        texts += [t.encode()[:n] for n in range(len(t))]
    blob = b"".join(struct.pack("<I", len(t)) + t for t in texts)
    lines = _run_check("rle", blob).decode().splitlines()
    assert len(lines) == len(texts)
    for t, ln in zip(texts, lines):
        rc, w, h, same = (int(v) for v in ln.split())
        try:
            cells, _ = G.parse_rle(t)
            assert (rc, h, w, same) == (0,) + cells.shape + (1,), t
        except G.GolError as x:
            assert rc == x.code == G._lib.GOL_EFORMAT, t
    assert all(int(ln.split()[0]) == 0 for ln in lines[:len(valid)])


def test_paste_host_under_asan_ubsan(G):
    """The paste shapes of test_paste_host_matches_numpy on exact-size heap buffers (the pattern cut
    after the last word the call may read): no report, and the same cells and counts as numpy."""
    cases = list(paste_cases(G))
    blob = b""
    for args, buf, words, *_ in cases:
        layout, W, pitch, brows, row, rows, prow, x0, w, stride, op = args
        pw = 0 if words is None else (prow + rows - 1) * stride + (w + 63) // 64
        blob += struct.pack("<12q", *args, pw) + buf.tobytes() + (b"" if words is None else words.tobytes()[:8 * pw])
    out = _run_check("paste", blob)
    off = 0
    for args, buf, words, cells, want, written in cases:
        layout, W = args[0], args[1]
        rc, changed = struct.unpack_from("<2q", out, off)
        after = np.frombuffer(out, buf.dtype, buf.size, off + 16).reshape(buf.shape)
        off += 16 + buf.nbytes
        assert rc == 0, args
        assert changed == check_result(layout, W, buf, after, cells, want, written), args
    assert off == len(out)
