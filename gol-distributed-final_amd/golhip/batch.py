"""Many small Game-of-Life boards stepped in one launch (ctypes wrapper of gol_batch_*).

An ``Engine`` steps one board per launch, and on the reference's own boards (16² … 512²) a launch is
latency-bound.  A ``Batch`` holds n independent H x W tori (1 <= H, W <= 512, any width, n <= 2^20) on
one GPU, with one turn counter and one rule or a rule per board; a launch keeps every board resident
in one workgroup for all its turns, and can report the turn at which each board settled into a still
life or a period-2 oscillator, or find the period of any cycle it enters.  Boards are bit-packed
like ``Engine.load_words``: bit c % 64 of word c // 64 of a row is cell c, ceil(W / 64) uint64 words per
row, the bits at c >= W zero.
"""
from __future__ import annotations

import ctypes

import numpy as np

from ._lib import GOL_EINVAL, GOL_ENOMEM, GolError, _as_map, format_rule, lib, parse_map, parse_rle, parse_rule

# gol_island (include/golhip.h): the record of an island, 24 bytes
ISLAND_DTYPE = np.dtype([("y", "<i4"), ("x", "<i4"), ("cells", "<i4"), ("rows", "<u2"), ("cols", "<u2"), ("hash", "<u8")])
# gol_island_kind (include/golhip.h): one kind of a tally, 32 bytes
ISLAND_KIND_DTYPE = np.dtype([("hash", "<u8"), ("count", "<i8"), ("first", "<i8"), ("cells", "<i4"), ("rows", "<u2"), ("cols", "<u2")])
# GOL_ISLAND_FIXED, GOL_ISLAND_FREE (include/golhip.h): the hash of an island as it lies, or the smallest of its hashes in
# the eight orientations of the square, which no rotation or reflection changes
ISLAND_FIXED, ISLAND_FREE = 0, 1


def island(pattern, reach: int = 1, library=None, symmetry: int = ISLAND_FIXED):
    """The record of a lone pattern (a 2-D array of cells, non-zero = alive, or RLE text) as the island census
    gives it: a numpy record of ISLAND_DTYPE whose cells, rows, cols and hash are those of the same pattern
    anywhere on any torus where nothing else lies within `reach` of it, so a caller can name what a tally of
    Batch.islands finds.  Computed on the host (gol_batch_islands_host) on a torus padded by 2 reach cells; no GPU
    needed.  symmetry=ISLAND_FREE gives the free hash, the same for the pattern turned or mirrored.
    GolError(GOL_EINVAL) when the pattern is empty, is not one island at this reach, or does not fit a 512 x 512
    torus."""
    L = library or lib()
    cells = parse_rle(pattern, L)[0] if isinstance(pattern, (str, bytes, bytearray)) else np.asarray(pattern) != 0
    if cells.ndim != 2 or not cells.any():
        raise GolError(GOL_EINVAL, f"a pattern is a 2-D array with at least one alive cell, got shape {cells.shape}")
    ys, xs = np.nonzero(cells)
    cells = cells[ys.min():ys.max() + 1, xs.min():xs.max() + 1]
    h, w = cells.shape
    board = np.zeros((h + 2 * reach, w + 2 * reach), dtype=np.uint8)
    board[:h, :w] = cells
    words = Batch.pack(board)
    count, out = ctypes.c_int64(), np.zeros(1, dtype=ISLAND_DTYPE)
    rc = L.gol_batch_islands_sym_host(board.shape[0], board.shape[1], reach, symmetry, words.ctypes.data, words.shape[1], 1,
                                      ctypes.byref(count), out.ctypes.data, None)
    if rc:
        raise GolError(rc, L.gol_last_error().decode(errors="replace"))
    if count.value != 1:
        raise GolError(GOL_EINVAL, f"the pattern is {count.value} islands at reach {reach}, not one")
    return out[0]


class Batch:
    def __init__(self, n: int, height: int, width: int, rule="B3/S23", device: int = 0, turns_per_launch: int = 0,
                 library=None):
        self.n, self.H, self.W = int(n), int(height), int(width)
        self.Ww = (self.W + 63) // 64
        self._L = library or lib()
        h = ctypes.c_void_p()
        self._check(self._L.gol_batch_create(self.n, self.H, self.W, device, turns_per_launch, ctypes.byref(h)))
        self._h = h
        if rule is not None:
            try:
                self.set_rule(rule)
            except BaseException:
                self.close()
                raise

    def _check(self, rc: int) -> None:
        if rc:
            raise GolError(rc, self._L.gol_last_error().decode(errors="replace"))

    # -- lifetime
    def close(self) -> None:
        if getattr(self, "_h", None) and self._h.value:
            self._L.gol_batch_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    # -- bytes <-> words (host only)
    @staticmethod
    def pack(boards) -> np.ndarray:
        """uint8[..., H, W] cells (non-zero = alive) as uint64[..., H, ceil(W / 64)] words, padding zero."""
        a = np.asarray(boards)
        if a.ndim < 2 or a.shape[-1] < 1:
            raise GolError(GOL_EINVAL, f"boards are arrays of at least one column, got shape {a.shape}")
        W = a.shape[-1]
        bits = np.zeros(a.shape[:-1] + ((W + 63) // 64 * 64,), dtype=np.uint8)
        bits[..., :W] = a != 0
        return np.ascontiguousarray(np.packbits(bits, axis=-1, bitorder="little")).view("<u8")

    @staticmethod
    def unpack(words, width: int) -> np.ndarray:
        """The inverse of pack: uint8[..., H, width] of 0 / 255."""
        w = np.ascontiguousarray(words, dtype="<u8")
        return np.unpackbits(w.view(np.uint8), axis=-1, bitorder="little")[..., :width] * np.uint8(255)

    # -- boards in / out
    def load(self, boards, first: int = 0) -> None:
        """Boards [first, first + len(boards)) from uint8[m, H, W] (non-zero = alive); the others stay.
        Resets the turn counter."""
        a = np.asarray(boards)
        if a.ndim != 3 or a.shape[1:] != (self.H, self.W):
            raise ValueError(f"expected (m, {self.H}, {self.W}) cells, got {a.shape}")
        self.load_words(self.pack(a), first)

    def store(self, first: int = 0, count: int | None = None) -> np.ndarray:
        """Boards [first, first + count) as uint8[count, H, W] of 0 / 255 (default: all from `first`)."""
        return self.unpack(self.store_words(first, count), self.W)

    def load_words(self, words, first: int = 0) -> None:
        """Boards [first, first + m) from uint64[m, H, S] rows, S >= ceil(W / 64) (the words past
        ceil(W / 64) of a row and set bits at c >= W are ignored).  Resets the turn counter."""
        w = np.ascontiguousarray(words, dtype=np.uint64)
        if w.ndim != 3 or w.shape[1] != self.H or w.shape[2] < self.Ww:
            raise ValueError(f"expected (m, {self.H}, >= {self.Ww}) uint64 words, got {w.shape}")
        self._check(self._L.gol_batch_load_words(self._h, first, first + w.shape[0], w.ctypes.data, w.shape[2],
                                                 self.H * w.shape[2]))

    def store_words(self, first: int = 0, count: int | None = None, out=None) -> np.ndarray:
        """Boards [first, first + count) as uint64[count, H, ceil(W / 64)]; with `out`, a C-contiguous
        uint64[count, H, S >= ceil(W / 64)], into it: the words past ceil(W / 64) of its rows stay."""
        if out is None:
            count = self.n - first if count is None else count
            out = np.empty((max(count, 0), self.H, self.Ww), dtype=np.uint64)
        elif (not isinstance(out, np.ndarray) or out.dtype != np.uint64 or not out.flags.c_contiguous or out.ndim != 3
              or out.shape[1] != self.H or out.shape[2] < self.Ww or (count is not None and count != out.shape[0])):
            raise ValueError(f"out must be C-contiguous uint64 (count, {self.H}, >= {self.Ww})")
        self._check(self._L.gol_batch_store_words(self._h, first, first + out.shape[0], out.ctypes.data, out.shape[2],
                                                  self.H * out.shape[2]))
        return out

    def load_random(self, seed: int) -> None:
        """word(i, y, w) = splitmix64(seed ^ ((i*H + y)*Ww + w)) masked to W, generated on the GPU."""
        self._check(self._L.gol_batch_load_random(self._h, seed))

    def load_soups(self, seed: int, first: int = 0) -> None:
        """Board i becomes soup first + i of `seed`: board first + i of load_random(seed) on a batch large
        enough to hold it.  Resets the turn counter."""
        self._check(self._L.gol_batch_load_soups(self._h, seed, first))

    @staticmethod
    def soup(height: int, width: int, seed: int, index: int, library=None) -> np.ndarray:
        """Soup `index` of (seed, height, width) as uint64[height, ceil(width / 64)] words, made on the
        host with the word function the fill kernels run (no GPU needed)."""
        L = library or lib()
        out = np.zeros((max(int(height), 0), (max(int(width), 0) + 63) // 64), dtype=np.uint64)
        rc = L.gol_batch_soup_host(height, width, seed, index, out.ctypes.data, out.shape[1])
        if rc:
            raise GolError(rc, L.gol_last_error().decode(errors="replace"))
        return out

    def search(self, seed: int, total: int, horizon: int, first: int = 0, stats: bool = False):
        """Run soups [first, first + total) of `seed` through the batch's boards as slots: a slot whose
        soup is found, or has outlived `horizon`, hands over its result and takes the next soup at the
        same launch boundary.  Returns (found, period, alive, hash), arrays of `total` entries indexed
        g - first: found and period as step_cycles defines them from t0 = 0 (int64), alive and hash the
        alive cells and oracle_hash_words of the soup's state at `found` (uint64); -1, -1, 0, 0 for a soup
        not found within the horizon.  stats=True appends a dict: launches, slots, launch_turns,
        board_turns, full_turns and occupancy = board_turns / full_turns.  Afterwards every board is
        empty and the turn counter is 0."""
        m = max(int(total), 0)
        found = np.full(m, -1, dtype=np.int64)
        period = np.full(m, -1, dtype=np.int64)
        alive = np.zeros(m, dtype=np.uint64)
        hashes = np.zeros(m, dtype=np.uint64)
        st = (ctypes.c_int64 * 5)()
        self._check(self._L.gol_batch_search(self._h, seed, first, total, horizon, found.ctypes.data, period.ctypes.data,
                                             alive.ctypes.data, hashes.ctypes.data, ctypes.addressof(st) if stats else None))
        if not stats:
            return found, period, alive, hashes
        d = dict(zip(("launches", "slots", "launch_turns", "board_turns", "full_turns"), (int(v) for v in st)))
        d["occupancy"] = d["board_turns"] / d["full_turns"] if d["full_turns"] else 0.0
        return found, period, alive, hashes, d

    def census(self, seed: int, total: int, horizon: int, first: int = 0, reach: int = 1, kinds: int = 4096,
               stats: bool = False, symmetry: int = ISLAND_FIXED) -> dict:
        """search() with the island census of every soup's state at `found` taken inside the search, and the tally
        of the kinds of island the soups turned into, built on the GPU: nothing per island comes back.  Returns a
        dict: found, period, alive, hash as search() returns them; islands (int64) and fingerprint (uint64), the
        island count and fingerprint of each soup's state at `found` at `reach` (0, 0 for a soup not found);
        n_kinds, the number of distinct kinds (a kind is an island's hash); kinds, a structured array of
        ISLAND_KIND_DTYPE with the first min(n_kinds, kinds) of them, ordered by count descending, then hash: per
        kind its hash, count, first (the lowest soup number that holds one: Batch.soup re-makes it) and the
        smallest (cells, rows, cols) among its islands; with stats=True also stats, the dict of search().
        symmetry=ISLAND_FREE: fingerprint and the kinds' hash are the free ones, so an object is one kind however it is
        turned or mirrored (islands() has the definition).
        GolError(GOL_ENOMEM) when the kind table that `kinds` sizes (at least 1024 slots) is full."""
        m, cap = max(int(total), 0), max(int(kinds), 0)
        out = {"found": np.full(m, -1, dtype=np.int64), "period": np.full(m, -1, dtype=np.int64),
               "alive": np.zeros(m, dtype=np.uint64), "hash": np.zeros(m, dtype=np.uint64),
               "islands": np.zeros(m, dtype=np.int64), "fingerprint": np.zeros(m, dtype=np.uint64)}
        table = np.zeros(cap, dtype=ISLAND_KIND_DTYPE)
        n_kinds, st = ctypes.c_int64(), (ctypes.c_int64 * 5)()
        rest = [*[a.ctypes.data for a in out.values()], table.ctypes.data if kinds > 0 else None, kinds, ctypes.byref(n_kinds),
                ctypes.addressof(st) if stats else None]
        if symmetry == ISLAND_FIXED:
            self._check(self._L.gol_batch_census(self._h, seed, first, total, horizon, reach, *rest))
        else:
            self._check(self._L.gol_batch_census_sym(self._h, seed, first, total, horizon, reach, symmetry, *rest))
        out["n_kinds"] = n_kinds.value
        out["kinds"] = table[:min(n_kinds.value, cap)]
        if stats:
            d = dict(zip(("launches", "slots", "launch_turns", "board_turns", "full_turns"), (int(v) for v in st)))
            d["occupancy"] = d["board_turns"] / d["full_turns"] if d["full_turns"] else 0.0
            out["stats"] = d
        return out

    # -- the rule
    def set_rule(self, rule) -> None:
        """The rule of every later turn: "B36/S23" or a (birth, survive) pair of 9-bit masks, or "MAP..." (set_map).
        The boards and the turn counter stay."""
        if isinstance(rule, str) and rule.startswith("MAP"):
            return self.set_map(rule)
        birth, survive = parse_rule(rule, self._L) if isinstance(rule, str) else (int(rule[0]), int(rule[1]))
        if not (0 <= birth < 1 << 32 and 0 <= survive < 1 << 32):
            raise GolError(GOL_EINVAL, f"rule masks out of range ({birth}, {survive})")
        self._check(self._L.gol_batch_set_rule(self._h, birth, survive))

    @property
    def rule(self) -> str:
        """The rule all boards share; GolError(GOL_ESTATE) when their rules differ (see rules()) and under MAP rules
        (see maps())."""
        b, s = ctypes.c_uint32(), ctypes.c_uint32()
        self._check(self._L.gol_batch_rule(self._h, ctypes.byref(b), ctypes.byref(s)))
        return format_rule(b.value, s.value, self._L)

    def set_rules(self, rules, first: int = 0) -> None:
        """The rules of boards [first, first + m): a sequence of "B36/S23" strings or (birth, survive)
        mask pairs, or a uint32[m, 2] array.  The other boards keep theirs; the boards and the turn
        counter stay.  One bad rule and none is set."""
        if isinstance(rules, np.ndarray):
            if rules.ndim != 2 or rules.shape[1] != 2 or rules.dtype.kind not in "ui":
                raise GolError(GOL_EINVAL, f"rules are an integer array of shape (m, 2), got {rules.dtype} {rules.shape}")
            pairs = rules.astype(np.int64)
        else:
            pairs = np.array([parse_rule(r, self._L) if isinstance(r, str) else (int(r[0]), int(r[1])) for r in rules],
                             dtype=np.int64).reshape(-1, 2)
        if np.any(pairs < 0) or np.any(pairs >= 1 << 32):
            raise GolError(GOL_EINVAL, "rule masks out of range")
        birth = np.ascontiguousarray(pairs[:, 0], dtype=np.uint32)
        survive = np.ascontiguousarray(pairs[:, 1], dtype=np.uint32)
        self._check(self._L.gol_batch_set_rules(self._h, first, first + len(birth), birth.ctypes.data, survive.ctypes.data))

    def rules(self, first: int = 0, count: int | None = None) -> np.ndarray:
        """uint32[count, 2]: (birth, survive) of boards [first, first + count) (default: all from `first`)."""
        count = self.n - first if count is None else count
        birth, survive = (np.zeros(max(count, 0), dtype=np.uint32) for _ in range(2))
        self._check(self._L.gol_batch_rules(self._h, first, first + count, birth.ctypes.data, survive.ctypes.data))
        return np.stack([birth, survive], axis=1)

    # -- MAP rules: any two-state rule of the 3x3 block as a table of 512 bits (gol_batch_set_map in golhip.h)
    def set_map(self, table) -> None:
        """Every board under one map from now on: "MAP..." text (or "B36/S23", as its map) or uint32[16], bit
        i = 256 NW + 128 N + 64 NE + 32 W + 16 C + 8 E + 4 SW + 2 S + SE of the table = the cell is alive next turn.
        Clears the rules; set_rule / set_rules clear the maps.  The boards and the turn counter stay."""
        m = parse_map(table, self._L) if isinstance(table, str) else _as_map(table)
        self._check(self._L.gol_batch_set_map(self._h, m.ctypes.data))

    def set_maps(self, maps, first: int = 0) -> None:
        """The maps of boards [first, first + k) from uint32[k, 16]; the other boards keep what they run under (a
        life-like rule as its map)."""
        a = np.asarray(maps)
        if a.ndim != 2 or a.shape[1] != 16 or a.dtype != np.uint32:
            raise GolError(GOL_EINVAL, f"maps are a uint32 array of shape (k, 16), got {a.dtype} {a.shape}")
        a = np.ascontiguousarray(a)
        self._check(self._L.gol_batch_set_maps(self._h, first, first + a.shape[0], a.ctypes.data))

    def maps(self, first: int = 0, count: int | None = None) -> np.ndarray:
        """uint32[count, 16]: the maps of boards [first, first + count) (default: all from `first`) as the batch
        stands; a board under a life-like rule has that rule's map."""
        count = self.n - first if count is None else count
        out = np.zeros((max(count, 0), 16), dtype=np.uint32)
        self._check(self._L.gol_batch_maps(self._h, first, first + count, out.ctypes.data))
        return out

    # -- stepping and queries
    def step(self, turns: int, settled: bool = False):
        """Advance every board `turns` turns.  settled=True returns int64[n]: per board the first
        turn t, turn + 2 <= t <= turn + turns, at which it equals its own state two turns earlier
        (a still life or a period-2 oscillator), else -1; every board still makes all the turns."""
        if not settled:
            self._check(self._L.gol_batch_step(self._h, turns, None))
            return None
        out = np.full(self.n, -1, dtype=np.int64)
        self._check(self._L.gol_batch_step(self._h, turns, out.ctypes.data))
        return out

    def step_cycles(self, turns: int):
        """Advance every board `turns` turns and scan each for a cycle of any period.  Returns
        (found, period), both int64[n]: with t0 the turn before the call and the marks t0 + 2^j - 1,
        found is the first turn t in (t0, t0 + turns] at which the board equals its state at the
        last mark before t, period = t minus that mark, the exact period of the board's cycle; -1 in
        both for a board not found.  found is an upper bound of the settle turn (at most t0 +
        3 max(mu + 1, period) for a board that enters its cycle mu turns after t0); every board makes
        all the turns, and each call scans from its own t0."""
        found = np.full(self.n, -1, dtype=np.int64)
        period = np.full(self.n, -1, dtype=np.int64)
        self._check(self._L.gol_batch_step_cycles(self._h, turns, found.ctypes.data, period.ctypes.data))
        return found, period

    def run_cycles(self, turns: int, made: bool = False):
        """step_cycles with the boards retired as they are found: the same (found, period), boards and
        turn counter, for less work.  A board found at f with period p repeats from f - p on, so it
        leaves the search at the end of the launch it is found in, makes (turns still to come) mod p
        turns and is then in its state of turn t0 + turns.  made=True also returns int64[n], the turns
        each board computed (see gol_batch_run_cycles in golhip.h for its exact value).  The host
        reads two counts back after every launch; when most boards are never found, step_cycles is
        the cheaper call."""
        found = np.full(self.n, -1, dtype=np.int64)
        period = np.full(self.n, -1, dtype=np.int64)
        work = np.zeros(self.n, dtype=np.int64) if made else None
        self._check(self._L.gol_batch_run_cycles(self._h, turns, found.ctypes.data, period.ctypes.data,
                                                 work.ctypes.data if made else None))
        return (found, period, work) if made else (found, period)

    @property
    def turn(self) -> int:
        t = ctypes.c_int64()
        self._check(self._L.gol_batch_turn(self._h, ctypes.byref(t)))
        return t.value

    def alive_counts(self) -> np.ndarray:
        out = np.zeros(self.n, dtype=np.uint64)
        self._check(self._L.gol_batch_alive_counts(self._h, out.ctypes.data, self.n))
        return out

    def hashes(self) -> np.ndarray:
        """Per board oracle_hash_words of its zero-padded words (Engine.hash's definition)."""
        out = np.zeros(self.n, dtype=np.uint64)
        self._check(self._L.gol_batch_hashes(self._h, out.ctypes.data, self.n))
        return out

    def islands(self, reach: int = 1, cap: int = 64, first: int = 0, count: int | None = None, fingerprints: bool = False,
                symmetry: int = ISLAND_FIXED):
        """The island census of boards [first, first + count) (default: all from `first`), labelled on the GPU
        where the boards lie; boards, turn and rules stay.  An island is a connected group of alive cells: two
        cells are linked when they are within `reach` (1: the 8-connected islands; 2: everything that shares a
        neighbour cell) of each other on the torus.  Returns (counts, islands): counts int64[count], the full
        number of islands per board; islands a zero-initialised structured array of shape (count, cap) and
        ISLAND_DTYPE whose first min(counts[i], cap) records of row i are board i's islands ordered by their
        first cell (y, x) in row-major order, with cells (the population), rows and cols (the distinct rows and
        columns occupied) and hash (the sum of the cells' window terms, gol_batch_islands in golhip.h).
        cells, rows, cols and hash do not change under a torus translation of the board; they do under
        rotation and reflection.  fingerprints=True appends uint64[count]: per board the wrapping sum of the
        hashes of all its islands, those past `cap` included.  symmetry=ISLAND_FREE: hash is the free hash, the
        smallest of the island's hashes in the eight orientations of the square ("island kinds free of orientation"
        in golhip.h), which no rotation or reflection changes, and the fingerprint their sum; y, x, rows and cols
        still describe the island as it lies."""
        count = self.n - first if count is None else count
        m = max(int(count), 0)
        counts = np.zeros(m, dtype=np.int64)
        recs = np.zeros((m, max(int(cap), 0)), dtype=ISLAND_DTYPE)
        fps = np.zeros(m, dtype=np.uint64) if fingerprints else None
        rest = [cap, counts.ctypes.data, recs.ctypes.data if cap > 0 else None, fps.ctypes.data if fingerprints else None]
        if symmetry == ISLAND_FIXED:
            self._check(self._L.gol_batch_islands(self._h, first, first + count, reach, *rest))
        else:
            self._check(self._L.gol_batch_islands_sym(self._h, first, first + count, reach, symmetry, *rest))
        return (counts, recs, fps) if fingerprints else (counts, recs)

    def islands_tally(self, reach: int = 1, kinds: int = 4096, first: int = 0, count: int | None = None,
                      symmetry: int = ISLAND_FIXED):
        """The tally of the island kinds of boards [first, first + count) as they stand (default: all from `first`),
        built on the GPU; boards, turn and rules stay.  Returns (counts, fingerprints, kinds): per board the number
        of islands (int64) and the fingerprint (uint64) as islands() gives them, and the kinds as census() returns
        them, all of them up to `kinds`, `first` being the lowest board index that holds one.  When the kind table
        is full GolError(GOL_ENOMEM) is raised; its `counts` and `fingerprints` attributes hold the per-board
        outputs, which are right.  symmetry=ISLAND_FREE: the fingerprints and the kinds' hash are the free ones."""
        count = self.n - first if count is None else count
        m, cap = max(int(count), 0), max(int(kinds), 0)
        counts, fps = np.zeros(m, dtype=np.int64), np.zeros(m, dtype=np.uint64)
        table = np.zeros(cap, dtype=ISLAND_KIND_DTYPE)
        n_kinds = ctypes.c_int64()
        rest = [counts.ctypes.data, fps.ctypes.data, table.ctypes.data if kinds > 0 else None, kinds, ctypes.byref(n_kinds)]
        if symmetry == ISLAND_FIXED:
            rc = self._L.gol_batch_islands_tally(self._h, first, first + count, reach, *rest)
        else:
            rc = self._L.gol_batch_islands_tally_sym(self._h, first, first + count, reach, symmetry, *rest)
        if rc == GOL_ENOMEM:
            e = GolError(rc, self._L.gol_last_error().decode(errors="replace"))
            e.counts, e.fingerprints = counts, fps
            raise e
        self._check(rc)
        return counts, fps, table[:min(n_kinds.value, cap)]

    def info(self) -> dict:
        n, H, W = (ctypes.c_int64() for _ in range(3))
        wpb, bpw, nw, tpl = (ctypes.c_int32() for _ in range(4))
        self._check(self._L.gol_batch_info(self._h, ctypes.byref(n), ctypes.byref(H), ctypes.byref(W), ctypes.byref(wpb),
                                           ctypes.byref(bpw), ctypes.byref(nw), ctypes.byref(tpl)))
        return {"n": n.value, "height": H.value, "width": W.value, "waves_per_board": wpb.value,
                "boards_per_workgroup": bpw.value, "words_per_lane": nw.value, "turns_per_launch": tpl.value}
