"""The tally of island kinds by its definition (include/golhip.h, "the tally of island kinds"), in plain Python
(helper of the tally tests, not a test).  It does not call the library: records come from island_ref.census, a
soup's s(found) from search_ref.one / soup_cells and rule_ref.run, and the kinds from a collections tally.

tally(pairs) -> kinds: pairs an iterable of (owner, record of island_ref.DTYPE); kinds a structured array of
KIND_DTYPE in the tally's order (count descending, then hash ascending).
of_boards(cells, reach, owner0) -> (counts, fingerprints, kinds) of a stack of boards, owner = owner0 + index.
census(case, reach) -> the dict Batch.census returns for a soup case, computed once and read-only.
table(raw) -> (kinds, empties_ok): a device table read back as bytes, its non-empty slots unpacked and sorted.
And the case tables of the GPU tests (tests/test_gpu_tally.py), whose preconditions tests/test_tally_ref_cpu.py
asserts."""
import collections
import functools
from dataclasses import dataclass

import numpy as np

import island_ref as I
import rule_ref as R
import search_ref as S
from testlib import Guarded

KIND_DTYPE = np.dtype([("hash", "<u8"), ("count", "<i8"), ("first", "<i8"), ("cells", "<i4"), ("rows", "<u2"), ("cols", "<u2")])
# a slot of the device table: the last word is cells << 32 | rows << 16 | cols
SLOT_DTYPE = np.dtype([("hash", "<u8"), ("count", "<i8"), ("first", "<i8"), ("shape", "<u8")])
EMPTY = np.array([(0, 0, (1 << 63) - 1, (1 << 64) - 1)], dtype=SLOT_DTYPE)[0]


def tally(pairs):
    count = collections.Counter()
    first, shape = {}, {}
    for owner, r in pairs:
        h = int(r["hash"]) or 1  # hash 0 is tallied under 1
        count[h] += 1
        first[h] = min(first.get(h, owner), owner)
        s = (int(r["cells"]), int(r["rows"]), int(r["cols"]))
        shape[h] = min(shape.get(h, s), s)
    order = sorted(count, key=lambda h: (-count[h], h))
    return np.array([(h, count[h], first[h]) + shape[h] for h in order], dtype=KIND_DTYPE)


def of_boards(cells, reach, owner0=0):
    res = [I.census(b, reach) for b in cells]
    counts = np.array([len(r) for r, _ in res], dtype=np.int64)
    fps = np.array([fp for _, fp in res], dtype=np.uint64)
    return counts, fps, tally((owner0 + i, r) for i, (recs, _) in enumerate(res) for r in recs)


def empty_table(log2):
    return np.full(1 << log2, EMPTY, dtype=SLOT_DTYPE)


def table(raw):
    """A device table's bytes as (kinds in the tally's order, True when every slot without a tag is exactly empty)."""
    slots = np.frombuffer(bytes(raw), dtype=SLOT_DTYPE)
    used = slots[slots["hash"] != 0]
    kinds = np.zeros(len(used), dtype=KIND_DTYPE)
    for f in ("hash", "count", "first"):
        kinds[f] = used[f]
    kinds["cells"] = (used["shape"] >> np.uint64(32)).astype(np.int64)
    kinds["rows"] = (used["shape"] >> np.uint64(16)) & np.uint64(0xffff)
    kinds["cols"] = used["shape"] & np.uint64(0xffff)
    order = sorted(range(len(kinds)), key=lambda i: (-int(kinds["count"][i]), int(kinds["hash"][i])))
    return kinds[order], bool(np.all(slots[slots["hash"] == 0] == EMPTY))


# ------------------------------------------------------------------------------------------------ the soup cases
RULE = "B3/S23"
SEED = 0x15A4D


@dataclass(frozen=True)
class SoupCase:
    id: str
    total: int
    H: int
    W: int
    horizon: int


SOUP_CASES = (SoupCase("64x16x16", 64, 16, 16, 512), SoupCase("48x32x32", 48, 32, 32, 1024), SoupCase("32x20x70", 32, 20, 70, 1024))


@functools.lru_cache(maxsize=None)
def found_cells(c, g):
    """uint8[H, W]: s(found) of soup g of the case, or None for a soup not found."""
    found = S.one(SEED, g, c.H, c.W, RULE, c.horizon)[0]
    if found < 0:
        return None
    out = R.run(S.soup_cells(SEED, g, c.H, c.W), RULE, found)[0]
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def census(c, reach, first=0, total=None):
    """What Batch.census(SEED, total, c.horizon, first, reach, kinds=large) returns, without stats."""
    total = c.total if total is None else total
    found, period, alive, hashes = S.search(SEED, first, total, c.H, c.W, RULE, c.horizon)
    islands, fps, pairs = np.zeros(total, dtype=np.int64), np.zeros(total, dtype=np.uint64), []
    for i in range(total):
        cells = found_cells(c, first + i)
        if cells is None:
            continue
        recs, fp = I.census(cells, reach)
        islands[i], fps[i] = len(recs), fp
        pairs += [(first + i, r) for r in recs]
    kinds = tally(pairs)
    out = {"found": found, "period": period, "alive": alive, "hash": hashes, "islands": islands, "fingerprint": fps,
           "kinds": kinds, "n_kinds": len(kinds)}
    for a in (islands, fps, kinds):
        a.setflags(write=False)
    return out


# -------------------------------------------------------------------------------------- the raw entry's own cases
# the case of the table sizes, of the accumulation and of the listed mode: 40 boards of 24 x 40 at two densities
def boards_case():
    rng = np.random.default_rng(777)
    return np.stack([rng.random((24, 40)) < (0.10 if i % 2 else 0.22) for i in range(40)])


def distinct_islands(n=1200):
    """uint8[n, 16, 16]: per board one island, no two alike: a bar of six cells with a different choice of the
    twelve cells above and below it on every board (each touches the bar, so the board is one island at either
    reach)."""
    rng = np.random.default_rng(4242)
    picks = rng.choice(1 << 12, size=n, replace=False)
    out = np.zeros((n, 16, 16), dtype=np.uint8)
    out[:, 5, 2:8] = 1
    for i, p in enumerate(picks):
        for k in range(12):
            if p >> k & 1:
                out[i, 4 if k < 6 else 6, 2 + k % 6] = 1
    return out


# ------------------------------------------------- the arguments of the launch check (gol_batch_islands_tally_check_host)
P = 0x1000  # a pointer that is never dereferenced
ORDER = ("boards", "n", "H", "W", "reach", "pairs", "pair_count", "max_pairs", "found", "owner0", "count", "fingerprint", "table",
         "table_log2", "dropped")
DENSE = dict(boards=P, n=3, H=64, W=64, reach=1, pairs=None, pair_count=None, max_pairs=0, found=None, owner0=0, count=P,
             fingerprint=P, table=P, table_log2=10, dropped=P)
LISTED = dict(DENSE, pairs=P, pair_count=P, max_pairs=3, found=P)
REFUSED = [(DENSE, bad) for bad in (
    dict(boards=None), dict(count=None), dict(table=None), dict(dropped=None), dict(n=0), dict(n=(1 << 20) + 1), dict(H=0),
    dict(H=513), dict(W=0), dict(W=513), dict(reach=0), dict(reach=3), dict(reach=-1), dict(table_log2=3), dict(table_log2=25),
    dict(table_log2=0), dict(owner0=-1), dict(owner0=(1 << 40) + 1), dict(pair_count=P), dict(found=P), dict(max_pairs=1))]
REFUSED += [(LISTED, bad) for bad in (dict(pair_count=None), dict(found=None), dict(max_pairs=0), dict(max_pairs=4),
                                      dict(max_pairs=-1), dict(table=None), dict(dropped=None), dict(table_log2=25))]


# ------------------------------------------------------------------------------ the buffers of a launch (GPU tests)
FILL = 0xA5


class Launch:
    """The buffers of tally launches on one stack of boards: a table of 2^log2 slots (empty, made here), dropped,
    and count / fingerprint of `outs` entries filled with the sentinel."""

    def __init__(self, G, cells, log2, outs=None):
        self.G, self.cells, self.log2 = G, cells, log2
        self.n, self.H, self.W = cells.shape
        self.boards = Guarded(G.Batch.pack(cells.astype(np.uint8)), name="boards")
        outs = self.n if outs is None else outs
        self.count = Guarded(np.full(outs * 8, FILL, dtype=np.uint8), name="count")
        self.fp = Guarded(np.full(outs * 8, FILL, dtype=np.uint8), name="fingerprint")
        self.table, self.dropped = Guarded(empty_table(log2), name="table"), Guarded(np.zeros(1, dtype=np.int64), name="dropped")

    def run(self, reach, owner0=0, pairs=None, pair_count=None, max_pairs=0, found=None, n=None):
        import torch
        rc = self.G.lib().gol_dev_batch_islands_tally(
            self.boards.ptr, self.n if n is None else n, self.H, self.W, reach, pairs.ptr if pairs else None,
            pair_count.ptr if pair_count else None, max_pairs, found.ptr if found else None, owner0, self.count.ptr, self.fp.ptr,
            self.table.ptr, self.log2, self.dropped.ptr, torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        return rc

    def results(self):
        """(count, fingerprint, kinds sorted, dropped) after checking the boards, every margin and the empty slots."""
        assert self.boards.unchanged(), "the boards or their margins changed"
        kinds, empties_ok = table(self.table.read(np.uint8).tobytes())
        assert empties_ok, "a slot without a tag is not the empty pattern"
        return self.count.read(np.int64), self.fp.read(np.uint64), kinds, int(self.dropped.read(np.int64)[0])
