"""Reference for MAP rules of a batch (helper of the map tests, not a test), written from the text of
include/golhip.h ("MAP rules of a batch") alone, never from the library or its host twins:

  a map is 512 bits, bit i = (map[i >> 5] >> (i & 31)) & 1; for a cell of an H x W torus
  i = 256 NW + 128 N + 64 NE + 32 W + 16 C + 8 E + 4 SW + 2 S + SE, N the row above, W the column to the left, and the
  cell is alive next turn iff bit i is set;
  text: "MAP" and the base64 of the 64 bytes whose bit i is bit 7 - (i & 7) of byte i >> 3.

Here: the index by nine np.rolls and a table lookup (step), the text codec (parse, fmt), the life-like rule as a map by
counting (from_rule), the cycle scan with cycle_ref.last_mark (scan), a search over search_ref.soup_cells (search), the
launch model of gol_dev_batch_step_map (launch_model: the definitions of gol_dev_batch_step with this stepper), the
projection maps P_k (bit i of P_k = bit k of i), whose turn is a pure translation, and the generated case table of
the raw-kernel test with its coverage (CASES)."""
import base64
import functools

import numpy as np

import cycle_ref as C
import search_ref as SR
from batch_ref import pack, unpack
from oracle import oracle as O

# (dy, dx, weight): np.roll(board, (dy, dx)) brings the neighbour at (y - dy, x - dx) to (y, x)
NEIGHBOURS = [(1, 1, 256), (1, 0, 128), (1, -1, 64), (0, 1, 32), (0, 0, 16), (0, -1, 8), (-1, 1, 4), (-1, 0, 2), (-1, -1, 1)]
GOLLY_LIFE = "MAPARYXfhZofugWaH7oaIDogBZofuhogOiAaIDogIAAgAAWaH7oaIDogGiA6ICAAIAAaIDogIAAgACAAIAAAAAAAA"


def bits(m) -> np.ndarray:
    """uint8[512]: the table of a map given as uint32[16]."""
    m = np.asarray(m, dtype=np.uint32)
    assert m.shape == (16,)
    return np.array([(int(m[i >> 5]) >> (i & 31)) & 1 for i in range(512)], np.uint8)


def from_bits(t) -> np.ndarray:
    m = np.zeros(16, np.uint32)
    for i in range(512):
        if t[i]:
            m[i >> 5] |= np.uint32(1 << (i & 31))
    return m


def index(board: np.ndarray) -> np.ndarray:
    b = (np.asarray(board) != 0).astype(np.int64)
    i = np.zeros(b.shape, np.int64)
    for dy, dx, weight in NEIGHBOURS:
        i += weight * np.roll(np.roll(b, dy, axis=0), dx, axis=1)
    return i


def step(board: np.ndarray, m) -> np.ndarray:
    """One turn of a board of 0 / 1 under the map m (uint32[16])."""
    return bits(m)[index(board)]


def run(board, m, turns: int) -> np.ndarray:
    t = bits(m)
    b = (np.asarray(board) != 0).astype(np.uint8)
    for _ in range(turns):
        b = t[index(b)]
    return b


def from_rule(birth: int, survive: int) -> np.ndarray:
    """The life-like rule as a map: the masks looked up at the count of the eight cells round C."""
    t = np.zeros(512, np.uint8)
    for i in range(512):
        n = bin(i & ~16).count("1")
        t[i] = ((survive if i & 16 else birth) >> n) & 1
    return from_bits(t)


def projection(k: int) -> np.ndarray:
    """P_k: bit i = bit k of i: the next cell is the neighbour of weight 2^k, so a turn is a translation."""
    return from_bits([(i >> k) & 1 for i in range(512)])


def projection_roll(k: int):
    """(dy, dx): a turn under P_k is np.roll(board, (dy, dx), (0, 1))."""
    return next((dy, dx) for dy, dx, weight in NEIGHBOURS if weight == 1 << k)


def random_map(seed: int, zero_bit=None) -> np.ndarray:
    m = np.random.default_rng(seed).integers(0, 1 << 32, 16, dtype=np.uint64).astype(np.uint32)
    if zero_bit is not None:
        m[0] = (m[0] & ~np.uint32(1)) | np.uint32(zero_bit)
    return m


def fmt(m) -> str:
    t = bits(m)
    raw = bytes(sum(int(t[8 * j + b]) << (7 - b) for b in range(8)) for j in range(64))
    return "MAP" + base64.b64encode(raw).decode().rstrip("=")


def parse(text: str) -> np.ndarray:
    assert text.startswith("MAP")
    body = text[3:]
    raw = base64.b64decode(body + "=" * (-len(body) % 4), validate=True)
    assert len(raw) == 64
    return from_bits([(raw[i >> 3] >> (7 - (i & 7))) & 1 for i in range(512)])


def scan(board, m, turns: int, t0: int = 0):
    """(found, period, s(t0 + turns)): cycle_ref.scan under a map."""
    states = [(np.asarray(board) != 0).astype(np.uint8)]
    t = bits(m)
    found = period = -1
    for d in range(1, turns + 1):
        states.append(t[index(states[-1])])
        mk = C.last_mark(d)
        if found < 0 and np.array_equal(states[d], states[mk]):
            found, period = t0 + d, d - mk
    return found, period, states[-1]


def search(seed: int, first: int, total: int, H: int, W: int, m, horizon: int):
    """(found, period, alive, hash, states): gol_batch_search's results under the map, and s(found) per found soup."""
    found, period = np.full(total, -1, np.int64), np.full(total, -1, np.int64)
    alive, hashes, states = np.zeros(total, np.uint64), np.zeros(total, np.uint64), {}
    for g in range(total):
        cells = SR.soup_cells(seed, first + g, H, W)
        f, p, _ = scan(cells, m, horizon)
        if f >= 0:
            s = run(cells, m, f)
            w = pack(s)
            found[g], period[g], alive[g], hashes[g], states[g] = f, p, O.popcount_words(w), O.hash_words(w), s
    return found, period, alive, hashes, states


SCAN_NONE, SCAN_SETTLE, SCAN_CYCLES = 0, 1, 2
MARKSET = set(C.MARKS)


def launch_model(boards, prev, settled, left, *, H, W, turns, maps, map_each, turn0=0, have_prev=False, write_prev=False,
                 scan=SCAN_NONE, done=0, list=None, count=None, born=None):
    """One launch of gol_dev_batch_step_map on copies of the buffers, by the mode definitions of gol_dev_batch_step in
    golhip.h (boards, prev: uint64[n, H, Ww]; settled, left, born: int64[n] or None; maps: uint32[16] or [n, 16]; list:
    board numbers, `count` of them listed, or None).  Returns {"boards", "prev", "settled", "left"}."""
    n = len(boards)
    out = {"boards": boards.copy(), "prev": None if prev is None else prev.copy(),
           "settled": None if settled is None else settled.copy(), "left": None if left is None else left.copy()}
    for b in (range(n) if list is None else [int(v) for v in list[:count]]):
        t = bits(maps[b] if map_each else maps)
        s = [unpack(boards[b], W)]
        if scan == SCAN_NONE:
            m = turns if left is None else min(turns, int(left[b]))
            for _ in range(m):
                s.append(t[index(s[-1])])
            out["boards"][b] = pack(s[m])
            if left is not None and m > 0:
                out["left"][b] = left[b] - m
            continue
        for _ in range(turns):
            s.append(t[index(s[-1])])
        out["boards"][b] = pack(s[turns])
        f = -1
        if scan == SCAN_SETTLE:
            before = unpack(prev[b], W) if have_prev else None  # s(turn0 - 1)
            for it in range(1, turns + 1):
                two_back = s[it - 2] if it >= 2 else before
                if f < 0 and two_back is not None and np.array_equal(s[it], two_back):
                    f = turn0 + it
            snap = s[turns - 1]
        else:
            a = done if born is None else done - int(born[b])
            base = turn0 if born is None else a
            snap = unpack(prev[b], W) if a > 0 else s[0]
            for it in range(1, turns + 1):
                if f < 0 and np.array_equal(s[it], snap):
                    f = base + it
                if (a + it) in MARKSET and not (born is not None and f >= 0):
                    snap = s[it]
        if write_prev:
            out["prev"][b] = pack(snap)
        if f >= 0 and settled[b] < 0:
            out["settled"][b] = f
    return out


# ---------------------------------------------------------------- the case table of the raw-kernel test

WIDTHS = [1, 2, 3, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 512]
HEIGHTS = [1, 2, 3, 63, 64, 65, 128, 129, 512]
N_BOARDS = 5
KINDS = ["each", "one"] + [f"P{k}" for k in range(9)]


def words_per_lane(W):
    nw = 1
    while nw < (W + 31) // 32:
        nw *= 2
    return nw


@functools.lru_cache(maxsize=None)
def cases():
    """(id, H, W, turns, kind): every width with two heights.  The heights go round within the narrow widths (one
    word: W <= 32), the wide ones (W > 128) and the ones between, so that every height meets a narrow and a wide row;
    the kinds (a random map per board, one shared map, a projection: each of the nine in turn) and 1..9 turns go
    round over all."""
    out = []
    groups = [[W for W in WIDTHS if W <= 32], [W for W in WIDTHS if 32 < W <= 128], [W for W in WIDTHS if W > 128]]
    for g, widths in enumerate(groups):
        for j, W in enumerate(widths):
            for r in range(2):
                s = 2 * j + r
                H = HEIGHTS[(2 * s + 1 if g == 1 else s) % len(HEIGHTS)]
                k = len(out)
                kind = ("each", "one", f"P{(k // 3) % 9}")[k % 3]
                out.append((f"{H}x{W}-{kind}", H, W, 1 + k % 9, kind))
    return out


def case_maps(kind, seed):
    """(maps, map_each) of a case: uint32[n, 16] or uint32[16]."""
    if kind == "each":  # (odd boards give birth on empty ground)
        return np.stack([random_map(seed + b, zero_bit=b & 1) for b in range(N_BOARDS)]), True
    if kind == "one":
        return random_map(seed, zero_bit=1), False
    return projection(int(kind[1:])), False
