"""The island census of a torus by its definition (include/golhip.h, "the island census of a batch"), in plain
Python and numpy: a flood fill over the link, the window code of every alive cell from np.roll, splitmix64
written out here.  It does not call the library.  And the case table of the GPU tests (tests/test_gpu_islands.py),
whose coverage tests/test_island_ref_cpu.py asserts.

census(cells, reach) -> (records, fingerprint): cells a 2-D array (non-zero = alive); records a structured array
of DTYPE ordered by (y, x), fingerprint a Python int."""
from dataclasses import dataclass, field

import numpy as np

DTYPE = np.dtype([("y", "<i4"), ("x", "<i4"), ("cells", "<i4"), ("rows", "<u2"), ("cols", "<u2"), ("hash", "<u8")])
M64 = (1 << 64) - 1


def splitmix64(x):
    z = (x + 0x9E3779B97F4A7C15) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def window_codes(cells, reach):
    """int64[H, W]: the window code of every cell (of the alive ones it is used)."""
    a = (np.asarray(cells) != 0).astype(np.int64)
    k = 2 * reach + 1
    code = np.zeros(a.shape, dtype=np.int64)
    for dy in range(-reach, reach + 1):
        for dx in range(-reach, reach + 1):
            # alive((y + dy) mod H, (x + dx) mod W)
            code += np.roll(a, (-dy, -dx), axis=(0, 1)) << ((dy + reach) * k + (dx + reach))
    return code


def term(code, reach):
    return splitmix64(int(code) ^ (reach << 32))


def census(cells, reach):
    a = np.asarray(cells) != 0
    H, W = a.shape
    codes = window_codes(a, reach)
    seen = np.zeros((H, W), dtype=bool)
    out = []
    fp = 0
    for y0, x0 in np.argwhere(a):  # row-major: an island's first cell is met first
        if seen[y0, x0]:
            continue
        stack = [(int(y0), int(x0))]
        seen[y0, x0] = True
        n, h, rows, cols = 0, 0, set(), set()
        while stack:
            y, x = stack.pop()
            n += 1
            rows.add(y)
            cols.add(x)
            h = (h + term(codes[y, x], reach)) & M64
            for dy in range(-reach, reach + 1):
                for dx in range(-reach, reach + 1):
                    yy, xx = (y + dy) % H, (x + dx) % W
                    if a[yy, xx] and not seen[yy, xx]:
                        seen[yy, xx] = True
                        stack.append((yy, xx))
        out.append((int(y0), int(x0), n, len(rows), len(cols), h))
        fp = (fp + h) & M64
    return np.array(out, dtype=DTYPE), fp


def lone(pattern, reach):
    """The (cells, rows, cols, hash) of a pattern alone on a torus padded by 2 reach + 1 cells."""
    p = np.asarray(pattern) != 0
    board = np.zeros((p.shape[0] + 2 * reach + 1, p.shape[1] + 2 * reach + 1), dtype=bool)
    board[:p.shape[0], :p.shape[1]] = p
    recs, _ = census(board, reach)
    assert len(recs) == 1
    return tuple(int(recs[0][f]) for f in ("cells", "rows", "cols", "hash"))


def key(recs):
    """The translation-invariant part of the records, as a sorted list (a multiset)."""
    return sorted((int(r["cells"]), int(r["rows"]), int(r["cols"]), int(r["hash"])) for r in recs)


# ----------------------------------------------------------------------------------------------- the case table
BLOCK = np.ones((2, 2), dtype=bool)
HEIGHTS = (1, 2, 3, 64, 65, 129)
WORDS = (1, 2, 4, 8, 16)  # the kernel's NW
CAP = 48  # of the shape cases: below the count of the busy boards, above that of the sparse ones


def nw_of(W):
    nwr, nw = (W + 31) // 32, 1
    while nw < nwr:
        nw *= 2
    return nw


def widths_of(nw):
    """The width classes of one NW: 16 NW + 1, an odd word count below NW, 32 NW - 1 and 32 NW."""
    odd = {4: [32 * 3 - 5], 8: [32 * 5 - 10], 16: [32 * 9 - 8]}.get(nw, [])  # 3, 5 and 9 words
    return [16 * nw + 1] + odd + [32 * nw - 1, 32 * nw]


NARROW = (1, 2, 3, 4)  # narrower than the reach-2 window


@dataclass
class Case:
    id: str
    cells: np.ndarray  # bool[n, H, W]
    cap: int = CAP
    reaches: tuple = (1, 2)
    tags: set = field(default_factory=set)

    @property
    def shape(self):
        return self.cells.shape[1:]


def _random_boards(rng, H, W):
    dens = (0.5, 0.15, 0.03) if H * W <= 20000 else (0.08, 0.02)
    return np.stack([rng.random((H, W)) < d for d in dens])


def _board(H, W, cells):
    b = np.zeros((H, W), dtype=bool)
    for y, x in cells:
        b[y % H, x % W] = True
    return b


def _block_at(H, W, y, x):
    return _board(H, W, [(y, x), (y, x + 1), (y + 1, x), (y + 1, x + 1)])


def serpentine(n=65):
    """A path that fills an n x n torus but for its last two columns: every even column whole, joined to the next
    one by a single cell of the odd column between them, by turns in row 0 and in the middle row."""
    b = np.zeros((n, n), dtype=bool)
    for x in range(0, n - 2, 2):
        b[:, x] = True
        if x + 2 < n - 2:
            b[0 if x % 4 == 0 else n // 2, x + 1] = True
    return b


def _cases():
    rng = np.random.default_rng(20240611)
    out = []
    # the width classes of every NW, each at two heights so that every NW meets every height
    for nw in WORDS:
        ws = widths_of(nw)
        for k, W in enumerate(ws):
            for H in (HEIGHTS[(2 * k) % 6], HEIGHTS[(2 * k + 1) % 6]):
                out.append(Case(f"shape-{H}x{W}", _random_boards(rng, H, W), tags={"shape", f"nw{nw}", f"h{H}", f"w{W}"}))
    for W in NARROW:
        for H in HEIGHTS:
            out.append(Case(f"narrow-{H}x{W}", _random_boards(rng, H, W), tags={"shape", "narrow", f"h{H}", f"w{W}"}))
    out.append(Case("shape-512x40", np.stack([rng.random((512, 40)) < 0.03]), tags={"shape", "h512"}))
    out.append(Case("shape-512x512", np.stack([rng.random((512, 512)) < 0.004]), tags={"shape", "h512", "w512"}))
    # a block across every seam: one island with the block's hash
    seams = {"colwrap": _block_at(20, 23, 7, 22), "bits31-32": _block_at(5, 70, 2, 31), "bits63-64": _block_at(5, 70, 2, 63),
             "rowwrap": _block_at(20, 23, 19, 5), "rows63-64": _block_at(130, 23, 63, 5), "corner": _block_at(20, 23, 19, 22)}
    for name, b in seams.items():
        out.append(Case(f"seam-{name}", b[None], tags={"seam", name}))
    out.append(Case("serpentine-65", serpentine(65)[None], tags={"serpentine"}))
    out.append(Case("diagonal-65", np.eye(65, dtype=bool)[None], tags={"diagonal"}))
    out.append(Case("diagonal-64x64", np.eye(64, dtype=bool)[None], tags={"diagonal"}))
    lat2 = np.zeros((64, 64), dtype=bool)
    lat2[::2, ::2] = True
    out.append(Case("lattice-2", lat2[None], cap=64, tags={"lattice2"}))
    lat3 = np.zeros((66, 63), dtype=bool)
    lat3[::3, ::3] = True
    out.append(Case("lattice-3", lat3[None], cap=64, tags={"lattice3"}))
    out.append(Case("empty-full", np.stack([np.zeros((65, 33), dtype=bool), np.ones((65, 33), dtype=bool)]), tags={"empty", "full"}))
    # five boards with different counts in one launch, at a cap of 0, below and above their counts
    five = np.stack([_board(40, 70, [(3 * i, 5 * i) for i in range(k)]) for k in (0, 1, 4, 9, 2)])
    for cap in (0, 3, 20):
        out.append(Case(f"five-cap{cap}", five, cap=cap, tags={"five", f"cap{cap}"}))
    return out


CASES = _cases()
_WANT = {}


def want(case, reach):
    """[(records, fingerprint)] of the case's boards, computed once."""
    if (case.id, reach) not in _WANT:
        _WANT[case.id, reach] = [census(b, reach) for b in case.cells]
    return _WANT[case.id, reach]

# the soups of the census's end-to-end test: SOUPS["n"] soups of side x side cells, run for `turns` turns; `cap` is the
# records per board the GPU test asks for, which the CPU test asserts to hold the largest count
SOUPS = {"n": 256, "side": 64, "seed": 0x15A4D, "turns": 2000, "cap": 64}
