"""The free hash of an island by its definition (include/golhip.h, "island kinds free of orientation"), in plain
Python and numpy (helper of the free-hash tests, not a test).  It does not call the library and never moves a bit
of a window code: it floods the board itself, keeps every island's cell list, turns and mirrors the BOARD with
numpy (B, B.T, [::-1], [:, ::-1] and their compositions), takes island_ref.window_codes of each image and sums
island_ref.term over the images of the island's cells.  The free hash is the smallest of the eight sums.

image(a, s) -> the s-th of the eight images of a 2-D array: rows flipped if s & 2, columns flipped if s & 4, then
transposed if s & 1 (applied to a (2 reach + 1)^2 window this is orient(code, reach, s) of the header).
census(cells, reach) -> (records, fingerprint): as island_ref.census, hash the free hash, fingerprint their sum.
want(case, reach) -> [(records, fingerprint)] of a case of island_ref.CASES, computed once and read-only.
of_boards(cells, reach, owner0) -> (counts, fingerprints, kinds) of a stack of boards, as tally_ref.of_boards.
soup_census(case, reach) -> what Batch.census(..., symmetry=ISLAND_FREE) returns for a case of tally_ref.SOUP_CASES.
The case tables are those of island_ref and tally_ref, by import."""
import functools

import numpy as np

import island_ref as I
import tally_ref as T
from island_ref import CASES, DTYPE, M64  # noqa: F401  (the GPU and CPU tests take them from here)
from tally_ref import SOUP_CASES, boards_case, distinct_islands, tally  # noqa: F401

FIXED, FREE = 0, 1


def image(a, s):
    a = np.asarray(a)
    if s & 2:
        a = a[::-1]
    if s & 4:
        a = a[:, ::-1]
    return a.T if s & 1 else a


def _image_of_cells(ys, xs, H, W, s):
    """Where the cells (ys, xs) of an H x W board lie in image(board, s)."""
    if s & 2:
        ys = H - 1 - ys
    if s & 4:
        xs = W - 1 - xs
    return (xs, ys) if s & 1 else (ys, xs)


@functools.lru_cache(maxsize=None)
def _term(code, reach):
    return I.term(code, reach)


def islands_of(a, reach):
    """The islands of bool[H, W] as lists of cells, ordered by their first cell in row-major order (a flood fill
    over the link, written here)."""
    H, W = a.shape
    seen = np.zeros((H, W), dtype=bool)
    out = []
    for y0, x0 in np.argwhere(a):
        if seen[y0, x0]:
            continue
        cells, stack = [], [(int(y0), int(x0))]
        seen[y0, x0] = True
        while stack:
            y, x = stack.pop()
            cells.append((y, x))
            for dy in range(-reach, reach + 1):
                for dx in range(-reach, reach + 1):
                    yy, xx = (y + dy) % H, (x + dx) % W
                    if a[yy, xx] and not seen[yy, xx]:
                        seen[yy, xx] = True
                        stack.append((yy, xx))
        out.append(cells)
    return out


def sums(cells, reach):
    """Per island of the board its eight sums: the hash (symmetry 0) of its image in each of the board's eight images."""
    a = np.asarray(cells) != 0
    H, W = a.shape
    codes = [I.window_codes(image(a, s), reach) for s in range(8)]
    out = []
    for isle in islands_of(a, reach):
        ys, xs = np.array([c[0] for c in isle]), np.array([c[1] for c in isle])
        eight = []
        for s in range(8):
            iy, ix = _image_of_cells(ys, xs, H, W, s)
            eight.append(sum(_term(int(c), reach) for c in codes[s][iy, ix]) & M64)
        out.append((isle, eight))
    return out


def census(cells, reach):
    out, fp = [], 0
    for isle, eight in sums(cells, reach):
        y0, x0 = min(isle)
        h = min(eight)
        out.append((y0, x0, len(isle), len({y for y, _ in isle}), len({x for _, x in isle}), h))
        fp = (fp + h) & M64
    return np.array(out, dtype=DTYPE), fp


_WANT = {}


def want(case, reach):
    if (case.id, reach) not in _WANT:
        res = [census(b, reach) for b in case.cells]
        for recs, _ in res:
            recs.setflags(write=False)
        _WANT[case.id, reach] = res
    return _WANT[case.id, reach]


def key(recs):
    """The part of the records that no translation, rotation or reflection changes: the multiset of (cells, hash)."""
    return sorted((int(r["cells"]), int(r["hash"])) for r in recs)


def lone(pattern, reach):
    """The free hash of a pattern alone on a torus padded by 2 reach + 1 cells."""
    p = np.asarray(pattern) != 0
    board = np.zeros((p.shape[0] + 2 * reach + 1, p.shape[1] + 2 * reach + 1), dtype=bool)
    board[:p.shape[0], :p.shape[1]] = p
    recs, _ = census(board, reach)
    assert len(recs) == 1
    return int(recs[0]["hash"])


def of_boards(cells, reach, owner0=0):
    res = [census(b, reach) for b in cells]
    counts = np.array([len(r) for r, _ in res], dtype=np.int64)
    fps = np.array([fp for _, fp in res], dtype=np.uint64)
    return counts, fps, tally((owner0 + i, r) for i, (recs, _) in enumerate(res) for r in recs)


@functools.lru_cache(maxsize=None)
def soup_census(c, reach):
    """What Batch.census(SEED, c.total, c.horizon, reach=reach, symmetry=ISLAND_FREE, kinds=large) returns, without
    stats: found, period, alive and hash those of the search (tally_ref.census has them)."""
    fixed = T.census(c, reach)
    islands, fps, pairs = np.zeros(c.total, dtype=np.int64), np.zeros(c.total, dtype=np.uint64), []
    for g in range(c.total):
        cells = T.found_cells(c, g)
        if cells is None:
            continue
        recs, fp = census(cells, reach)
        islands[g], fps[g] = len(recs), fp
        pairs += [(g, r) for r in recs]
    kinds = tally(pairs)
    assert np.array_equal(islands, fixed["islands"])
    out = dict(fixed, islands=islands, fingerprint=fps, kinds=kinds, n_kinds=len(kinds))
    for a in (islands, fps, kinds):
        a.setflags(write=False)
    return out
