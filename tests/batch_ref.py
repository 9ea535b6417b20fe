"""Reference for one launch of the batch step kernel (helper of the batch-kernel tests, not a test):
the launch model of gol_dev_batch_step and the case table that pins every instantiation of
batch_step_kernel<NW, RULE, SCAN, LIST, AGED> (csrc/gol_batch.hip).

The model is written from the definitions of include/golhip.h (gol_dev_batch_step) with the numpy
stepper of rule_ref.py and the brute-force mark list of cycle_ref.py, never from the library or its
host twins.  launch_model takes the buffers of one launch as numpy arrays and returns what they hold
afterwards, and per board the turn (aged: the age) f at which this launch found it.

The table.  An instantiation is the kernel's own tuple (NW, RULE, SCAN, LIST, AGED): 5 words per lane
x 3 rule modes x 5 modes (plain, settle, cycles, list + cycles, finish) + 10 aged ones = 85.  Every
case is one launch of 3..9 turns on n = 2 * boards_per_workgroup + 1 boards (the sensitivity cases:
as many as their words or waves need), so the last workgroup is partly filled.  cases_of(inst) gives:
  - width classes at H = 5 (width_classes): 16 NW + 1 ("min"); for NW >= 4 a width whose 32-bit word
    count is odd and below NW ("odd-nwr": 90, 150, 270; at 150 and 270 also 2 Ww < NW); 32 NW - 1
    ("full-1"); 32 NW ("full"); for NW = 1 also W = 1, 2, 3;
  - height classes at the "min" width (HEIGHTS): 1, 2, 64, 65, 128, 129, 193, 257, 512: one to eight
    waves per board, 4, 2 and 1 boards per workgroup, a full last wave and a last wave of one row;
  - NW = 16, B3/S23 only: 512 x 512 once per mode ("big");
  - the boards: soups alone in a launch without a scan; with one, a glider, blocks, a soup, a blinker, blocks,
    a glider, an empty board, a soup, blocks (of three boards: a glider and two of blocks), so that a launch
    finds some boards and not others;
  - list modes: the list is a shuffled strict subset of the boards; *count < slots and *count == slots
    alternate over the cases above, and one more case has *count == 0 ("zero-count"); the finish gives
    the list's places left[] = 0, below, equal to and above `turns` (the first four of one workgroup
    when it holds four boards) and a later workgroup whose boards all need fewer turns than the launch;
  - scans: have_prev / done and write_prev both ways over the cases; with have_prev the boards, prev
    and settled are the model's own results of an earlier launch (so boards found there carry their
    earlier turn, which must survive), without it settled is seeded by hand with -1 and an earlier turn;
  - aged: ages 0, 2, 5, 1, 0, 6, 3, 0, 2 (of three boards 2, 0, 2) at done = 6, so one workgroup holds boards born
    at different turns, age 2 crosses the mark 3, and a find and a non-find share a workgroup; and one case with
    pulsars ("freeze", 17 rows, 6 turns from age 2): found at age 6 before the mark 7, where s(7) != s(6);
  - a rule per board: board i under ERULES[i % 3] (B3/S23, B36/S23, B3678/S34678), so boards of one
    workgroup differ; the sensitivity cases use SENS_RULES, under which their patterns evolve as in B3/S23;
  - scan sensitivity, every scanning instantiation: boards of blocks only but for one glider (never
    found) or, in the twin, one blinker (the settle scan finds it at turn 2, the cycle scan at turn 3)
    confined to the columns of one 32-bit word ("sens-words": every word j < nwr at W = 32 NW and at the
    odd-nwr width, H = 20) or to the rows of one wave ("sens-waves": every wave at H = 512 and H = 128,
    "min" width).  No mover straddles two words: every last word used here has at least five columns.
    One more board is still with four cells in a row in its last row: at H = 20 the lanes after it have no
    row, and what they would compute from the row above them must not reach the comparison.
Nothing was thinned: the whole table (1376 cases) takes about 11 s of reference on a CPU, the largest
instantiation 0.4 s.

Every case carries check(): assertions on the model's results alone that the case shows what it is
there for."""
import dataclasses
import functools

import numpy as np

import cycle_ref as C
import rule_ref as R
from oracle import oracle as O

GAP = np.uint64(0xA5A5A5A5A5A5A5A5)
FILL32, FILL64 = np.int32(-0x5A5A5A5B), np.int64(-0x5A5A5A5A5A5A5A5B)  # bytes 0xA5

RULE_CONWAY, RULE_TABLE, RULE_EACH = 0, 1, 2
SCAN_NONE, SCAN_SETTLE, SCAN_CYCLES = 0, 1, 2
MODES = {"plain": (SCAN_NONE, False, False), "settle": (SCAN_SETTLE, False, False), "cycles": (SCAN_CYCLES, False, False),
         "list": (SCAN_CYCLES, True, False), "finish": (SCAN_NONE, True, False), "aged": (SCAN_CYCLES, True, True)}
MODE_OF = {v: k for k, v in MODES.items()}
RULE_NAME = {RULE_CONWAY: "conway", RULE_TABLE: "table", RULE_EACH: "each"}
NWS = [1, 2, 4, 8, 16]
INSTANTIATIONS = [(nw, rule) + MODES[m] for nw in NWS for rule in (RULE_CONWAY, RULE_TABLE, RULE_EACH)
                  for m in ("plain", "settle", "cycles", "list", "finish")]
INSTANTIATIONS += [(nw, rule) + MODES["aged"] for nw in NWS for rule in (RULE_CONWAY, RULE_TABLE)]

HEIGHTS = [1, 2, 64, 65, 128, 129, 193, 257, 512]
TABLE_RULE = "B36/S23"
ERULES = ["B3/S23", "B36/S23", "B3678/S34678"]
SENS_RULES = ["B3/S23", "B36/S23", "B38/S23"]
MARKSET = set(C.MARKS)
AGES = [0, 2, 5, 1, 0, 6, 3, 0, 2]
BLOCK_ON_TABLE = ["OO..", "OO..", "....", "OOOO", "O..O"]


def inst_id(inst):
    nw, rule, scan, lst, aged = inst
    return f"nw{nw}-{RULE_NAME[rule]}-{MODE_OF[(scan, lst, aged)]}"


def words_per_lane(W):
    nw = 1
    while nw < (W + 31) // 32:
        nw *= 2
    return nw


def shape(H):
    """(waves per board, boards per workgroup)."""
    wpb = (H + 63) // 64
    return wpb, max(1, 4 // wpb)


def width_classes(nw):
    w = {"min": 16 * nw + 1, "full-1": 32 * nw - 1, "full": 32 * nw}
    if nw == 1:
        w.update(w1=1, w2=2, w3=3)
    if nw >= 4:
        w["odd-nwr"] = {4: 90, 8: 150, 16: 270}[nw]
    return w


def pack(cells):
    """uint8[..., H, W] (non-zero = alive) -> uint64[..., H, ceil(W / 64)], bit c % 64 of word c // 64 = cell c."""
    c = (np.asarray(cells) != 0).astype(np.uint8)
    W = c.shape[-1]
    padded = np.zeros(c.shape[:-1] + (64 * ((W + 63) // 64),), np.uint8)
    padded[..., :W] = c
    return np.packbits(padded, axis=-1, bitorder="little").view("<u8").astype(np.uint64)


def unpack(words, W):
    """The inverse: uint8[..., H, W] of 0 / 1."""
    b = np.ascontiguousarray(np.asarray(words, dtype="<u8")).view(np.uint8)
    return np.unpackbits(b, axis=-1, bitorder="little")[..., :W]


# ---------------------------------------------------------------- the launch model

def _states(s0, rule, turns):
    out = [s0]
    for _ in range(turns):
        out.append(R.step(out[-1], *rule))
    return out


def launch_model(boards, prev, settled, left, *, H, W, turns, turn0=0, have_prev=False, write_prev=False, rule=R.CONWAY,
                 rules=None, scan=SCAN_NONE, done=0, list=None, count=None, born=None):
    """One launch on copies of the buffers (boards, prev: uint64[n, H, Ww]; settled, left, born: int64[n] or None;
    rules: [n, 2] masks or None; list: board numbers, count of them listed, or None for every board).
    Returns {"boards", "prev", "settled", "left", "f"}: f[b] = the turn (aged: the age) at which this launch found
    board b, -1 where it did not (or does not scan, or does not run the board)."""
    n = len(boards)
    out = {"boards": boards.copy(), "prev": None if prev is None else prev.copy(),
           "settled": None if settled is None else settled.copy(), "left": None if left is None else left.copy(),
           "f": np.full(n, -1, np.int64)}
    for b in (range(n) if list is None else [int(v) for v in list[:count]]):
        rl = rule if rules is None else (int(rules[b][0]), int(rules[b][1]))
        s0 = unpack(boards[b], W)
        if scan == SCAN_NONE:
            m = turns if left is None else min(turns, int(left[b]))
            out["boards"][b] = pack(_states(s0, rl, m)[m])
            if left is not None and m > 0:
                out["left"][b] = left[b] - m
            continue
        s = _states(s0, rl, turns)
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
            a = done if born is None else done - int(born[b])  # the turns of the board's scan before the launch
            base = turn0 if born is None else a
            snap = unpack(prev[b], W) if a > 0 else s[0]
            for it in range(1, turns + 1):
                if f < 0 and np.array_equal(s[it], snap):
                    f = base + it
                if (a + it) in MARKSET and not (born is not None and f >= 0):
                    snap = s[it]
        if write_prev:
            out["prev"][b] = pack(snap)
        out["f"][b] = f
        if f >= 0 and settled[b] < 0:
            out["settled"][b] = f
    return out


# ---------------------------------------------------------------- the cases

@dataclasses.dataclass
class Case:
    id: str
    inst: tuple
    tag: str       # "width" / "height" / "big" / "zero-count" / "freeze" / "sens-words" / "sens-waves"
    wclass: str    # the width class, or ""
    H: int
    W: int
    n: int
    turns: int
    turn0: int
    done: int
    have_prev: bool
    write_prev: bool
    rule: tuple                # (birth, survive) of a one-rule launch
    rules: np.ndarray | None   # uint32[n, 2]
    boards: np.ndarray
    prev: np.ndarray
    settled: np.ndarray | None = None
    left: np.ndarray | None = None
    born: np.ndarray | None = None
    list: np.ndarray | None = None   # int32[slots]
    count: int | None = None
    slots: int = 0
    count_kind: str = ""             # "lt" / "eq" / "zero"
    expect: dict = dataclasses.field(default_factory=dict)

    @property
    def mode(self):
        return MODE_OF[self.inst[2:]]

    @property
    def scan(self):
        return self.inst[2]

    @functools.cached_property
    def want(self):
        return launch_model(self.boards, self.prev, self.settled, self.left, H=self.H, W=self.W, turns=self.turns,
                            turn0=self.turn0, have_prev=self.have_prev, write_prev=self.write_prev, rule=self.rule,
                            rules=self.rules, scan=self.scan, done=self.done, list=self.list, count=self.count, born=self.born)

    def listed(self):
        return range(self.n) if self.list is None else [int(v) for v in self.list[:self.count]]

    def valid(self):
        """The entry's preconditions and the launchers' checks, on the arguments alone."""
        nw, rule, scan, lst, aged = self.inst
        Ww = (self.W + 63) // 64
        assert 1 <= self.H <= 512 and 1 <= self.W <= 512 and words_per_lane(self.W) == nw and 3 <= self.turns <= 9
        assert self.boards.shape == self.prev.shape == (self.n, self.H, Ww) and self.boards.dtype == np.uint64
        tail = np.uint64((1 << (self.W % 64)) - 1 if self.W % 64 else 2 ** 64 - 1)
        assert not np.any(self.boards[..., -1] & ~tail)
        assert (self.rules is not None) == (rule == RULE_EACH)
        if rule == RULE_EACH:
            assert self.rules.shape == (self.n, 2) and self.rules.dtype == np.uint32 and np.all(self.rules < 512)
            pairs = {tuple(r) for r in self.rules.tolist()}
            assert len(pairs) >= 3 and R.CONWAY in pairs
        else:
            assert (self.rule == R.CONWAY) == (rule == RULE_CONWAY) and max(self.rule) < 512
        assert (self.settled is not None) == (scan != SCAN_NONE) and self.done >= 0
        assert (self.list is not None) == lst and (self.born is not None) == aged
        assert (self.left is not None) == (lst and scan == SCAN_NONE)
        if scan == SCAN_NONE:
            assert not self.have_prev and not self.write_prev
        if scan == SCAN_CYCLES:
            assert self.have_prev == (self.done > 0)
        if aged:
            assert self.turn0 == 0 and self.write_prev and rule != RULE_EACH
        if lst:
            assert 1 <= self.slots <= self.n and 0 <= self.count <= self.slots and len(self.list) == self.slots
            ent = self.listed()
            assert len(set(ent)) == len(ent) and all(0 <= v < self.n for v in ent)
            if self.left is not None:
                assert all(self.left[v] >= 0 for v in ent)
            if aged:
                assert all(self.born[v] <= self.done for v in ent)
        else:
            assert self.slots == 0 and self.count is None
        # a state that is read is a real state: prev of the boards whose snapshot or state before is read
        for b in self.listed():
            reads = self.have_prev if not aged else self.done - int(self.born[b]) > 0
            if scan != SCAN_NONE and reads:
                assert not np.any(self.prev[b][..., -1] & ~tail)

    def check(self):
        """(the reference alone) the case shows what it is there for."""
        w, ent = self.want, self.listed()
        _, bpw = shape(self.H)
        groups = [ent[i:i + bpw] for i in range(0, len(ent), bpw)]
        roomy = self.H >= 5 and self.W >= 5
        untouched = [b for b in range(self.n) if b not in ent]
        for b in untouched:  # (the model itself: nothing of a board that is not listed)
            assert np.array_equal(w["boards"][b], self.boards[b]) and np.array_equal(w["prev"][b], self.prev[b])
        if self.tag in ("sens-words", "sens-waves"):
            want_f = self.expect["f"]
            assert w["f"].tolist() == want_f and w["settled"].tolist() == want_f
            assert -1 in want_f and max(want_f) > 0
            return
        if self.mode == "finish" and self.count:
            made = [min(self.turns, int(self.left[b])) for b in ent]
            assert any(m < self.turns for m in made) and self.turns in made
            if bpw == 4:
                four = [int(self.left[b]) for b in ent[:4]]
                assert four[0] == 0 and 0 < four[1] < self.turns and four[2] == self.turns and four[3] > self.turns
            if len(groups) > 1:  # a workgroup whose trip count is below the launch's
                assert any(0 < max(int(self.left[b]) for b in g) < self.turns for g in groups)
            if roomy:
                assert any(not np.array_equal(w["boards"][b], self.boards[b]) for b in ent)
        if self.scan != SCAN_NONE and self.count != 0 and roomy:
            new = [b for b in ent if self.settled[b] < 0 and w["settled"][b] >= 0]
            kept = [b for b in ent if self.settled[b] >= 0]
            none = [b for b in ent if w["settled"][b] < 0]
            assert new and (len(ent) < 3 or (none and kept)), (self.id, new, none, kept)
            assert all(w["settled"][b] == self.settled[b] for b in kept)
            if self.mode == "aged" and bpw > 1:  # a find and a non-find in one workgroup
                assert any(any(w["f"][b] >= 0 for b in g) and any(w["f"][b] < 0 for b in g) for g in groups)
        if self.mode == "aged" and self.tag != "zero-count":
            ages = [self.done - int(self.born[b]) for b in ent]
            if self.tag == "freeze":
                b = next(b for b in self.expect["pulsars"] if b in ent)
                a, f = self.done - int(self.born[b]), int(w["f"][b])
                assert f == 6 and a < f < 7 <= a + self.turns
                s = R.run(unpack(self.boards[b], self.W), self.rule, 7 - a, keep=(f - a, 7 - a))[2]
                assert not np.array_equal(s[f - a], s[7 - a]) and np.array_equal(w["prev"][b], pack(s[f - a]))
            else:
                assert 0 in ages and len(set(ages)) >= 2
                assert any(any(m in MARKSET for m in range(a + 1, a + self.turns + 1)) for a in ages if a > 0)
        if self.count == 0:
            assert all(np.array_equal(w[k], getattr(self, k)) for k in ("boards", "prev", "settled", "left")
                       if getattr(self, k) is not None)


def _blocks(H, W, *avoid):
    """Blocks on a grid, none within a box of avoid, each (y0, y1, x0, x1) (inclusive), or touching another."""
    b = np.zeros((H, W), np.uint8)
    for y in range(1, H - 2, 8):
        for x in range(1, W - 2, 16):
            if any(y + 2 >= a[0] and y - 1 <= a[1] and x + 2 >= a[2] and x - 1 <= a[3] for a in avoid):
                continue
            b[y:y + 2, x:x + 2] = 1
    return b


KINDS = ("glider", "blocks", "soup", "blinker", "blocks", "glider", "empty", "soup", "blocks")


def _kinds(n, H, W, scans=True):
    """What board i holds.  Three boards: a glider and two of blocks.  Without room for a pattern (H or W < 5) a
    glider is a soup and a blinker an empty board.  A launch without a scan has soups alone."""
    if not scans:
        return ["soup"] * n
    kinds = list(KINDS[:n]) if n > 3 else ["glider", "blocks", "blocks"]
    if H < 5 or W < 5:
        kinds = [{"glider": "soup", "blinker": "empty"}.get(k, k) for k in kinds]
    return kinds


def _compose(n, H, W, seed, scans=True):
    out = np.zeros((n, H, W), np.uint8)
    for i, kind in enumerate(_kinds(n, H, W, scans)):
        if kind == "soup":
            out[i] = R.random_board(seed + i, H, W, 0.25 + 0.05 * (i % 5))
        elif kind == "glider":
            out[i] = C.place(H, W, C.GLIDER, 1, 1)
        elif kind == "blinker":
            out[i] = C.place(H, W, C.BLINKER, 2, 1)
        elif kind == "blocks":
            out[i] = _blocks(H, W)
    return out


def _rule_args(rule_mode, n, names=ERULES):
    if rule_mode == RULE_EACH:
        return R.CONWAY, np.array([R.masks(names[i % len(names)]) for i in range(n)], np.uint32)
    return (R.CONWAY if rule_mode == RULE_CONWAY else R.masks(TABLE_RULE)), None


def _gap_like(words):
    return np.full_like(words, GAP)


def _subset_list(n, slots_kind, k, seed, kinds):
    """A shuffled strict subset of the boards as (list int32[slots], count, slots): all but the second glider and
    the second soup of nine boards, the last board of five, the first or the last of three; shuffled, then the
    boards a scan cannot find within a launch (gliders, soups) and the others take turns, so that a workgroup of
    two or four boards has both."""
    drop = {9: (5, 7), 5: (4,), 3: ((2, 0)[(k >> 2) & 1],)}[n]
    order = [int(b) for b in np.random.default_rng(seed).permutation(n) if b not in drop]
    movers = [b for b in order if kinds[b] in ("glider", "soup")]
    others = [b for b in order if b not in movers]
    order = [x for pair in zip(movers, others) for x in pair] + movers[len(others):] + others[len(movers):]
    if order == sorted(order):  # (two boards may come out in order)
        order = order[::-1]
    order = np.array(order, np.int32)
    m = len(order)
    if slots_kind == "zero":
        return order, 0, m
    slots = m if slots_kind == "eq" else min(n, m + 2)
    lst = np.full(slots, FILL32, np.int32)
    lst[:m] = order
    return lst, m, slots


def _general(inst, tag, wclass, H, W, k, count_kind=None, cells=None, extra=None, turns=None, table_rule=None):
    nw, rule_mode, scan, lst, aged = inst
    mode = MODE_OF[(scan, lst, aged)]
    _, bpw = shape(H)
    n = 2 * bpw + 1
    seed = 1000 * H + W + 17 * k
    turns = turns or 3 + (2 * k + H + W) % 7
    rule, rules = _rule_args(rule_mode, n)
    if table_rule and rule_mode == RULE_TABLE:
        rule = R.masks(table_rule)
    kinds = _kinds(n, H, W, scan != SCAN_NONE)
    if cells is None:
        cells = _compose(n, H, W, seed, scan != SCAN_NONE)
    boards = pack(cells)
    hp, wp = bool(k & 1), bool(k & 2)
    c = dict(id=f"{inst_id(inst)}-{tag}-{wclass or H}-{H}x{W}", inst=inst, tag=tag, wclass=wclass, H=H, W=W, n=n, turns=turns,
             turn0=10, done=0, have_prev=False, write_prev=False, rule=rule, rules=rules, boards=boards, prev=_gap_like(boards),
             expect=dict(extra or {}))
    ent = list(range(n))
    if lst:
        ck = count_kind or ("lt", "eq")[(k + (k >> 2)) & 1]
        c["list"], c["count"], c["slots"] = _subset_list(n, ck, k, seed, kinds)
        c["count_kind"] = ck
        ent = [int(v) for v in c["list"][:len(c["list"]) if ck == "zero" else c["count"]]]
    if mode == "finish":
        left = np.full(n, FILL64, np.int64)
        vals = [0, turns - 2, turns, turns + 5, turns - 1, 0, 1] if len(ent) > 2 else [turns - 2, turns + 5]
        for place, b in enumerate(ent):
            left[b] = vals[place]
        c["left"] = left
    elif mode == "aged":
        c.update(turn0=0, done=6, have_prev=True, write_prev=True)
        born, settled, prev = np.full(n, FILL64, np.int64), np.full(n, -1, np.int64), c["prev"]
        for b in range(n):  # the slot's soup at its age: the model's own scan of it from age 0
            a = 2 if tag == "freeze" else (2, 0, 2)[b] if n == 3 else AGES[b]
            born[b] = 6 - a
            if a > 0:
                one = launch_model(boards[b:b + 1], prev[b:b + 1], np.array([-1], np.int64), None, H=H, W=W, turns=a, rule=rule,
                                   write_prev=True, scan=SCAN_CYCLES, done=0, list=[0], count=1, born=np.zeros(1, np.int64))
                boards[b], prev[b], settled[b] = one["boards"][0], one["prev"][0], one["settled"][0]
        c.update(born=born, settled=settled)
    elif scan != SCAN_NONE:
        settled = np.full(n, -1, np.int64)
        if hp:  # an earlier launch of the same scan: its boards, prev and settled
            pre = 2 + k % 4
            one = launch_model(boards, c["prev"], settled, None, H=H, W=W, turns=pre, turn0=10, write_prev=True, rule=rule,
                               rules=rules, scan=scan, done=0)
            c.update(boards=one["boards"], prev=one["prev"], turn0=10 + pre, have_prev=True, done=pre if scan == SCAN_CYCLES else 0)
            settled = one["settled"]
        # the listed boards that this launch finds, in the list's order: one starts (again) at -1, the next
        # carries an earlier turn (the earlier launch's, or 7), and so on
        for i, b in enumerate([b for b in ent if kinds[b] in ("blocks", "empty", "blinker")]):
            settled[b] = -1 if i % 2 == 0 else (settled[b] if settled[b] >= 0 else 7)
        c.update(settled=settled, write_prev=wp)
    return Case(**c)


def _pulsar_boards(n, H, W):
    cells = _compose(n, H, W, 5)
    for b in (0, 5):
        cells[b] = C.place(H, W, C.PULSAR, 2, 2)
    return cells


def _sens(inst, tag, H, W, places):
    """Boards of blocks; pair i has a glider (even board) or a blinker (odd board) at places[i]; the last board but
    one has a block on a table across the torus seam, the table's four cells in the last row and its legs in row 0
    (a still life: where the last wave is partly filled, the lane after the last row sees three cells above it and
    must stay empty), the last board nothing that moves.
    One launch of 4 turns from turn 0 with nothing before it."""
    nw, rule_mode, scan, lst, aged = inst
    n = 2 * len(places) + 2
    cells = np.zeros((n, H, W), np.uint8)
    for i, (y, x) in enumerate(places):
        back = _blocks(H, W, (y - 3, y + 8, x - 3, x + 8))
        cells[2 * i] = back | C.place(H, W, C.GLIDER, y, x)
        cells[2 * i + 1] = back | C.place(H, W, C.BLINKER, y + 1, x)
    cells[n - 2] = _blocks(H, W, (0, 3, 0, W), (H - 6, H - 1, 0, W)) | C.place(H, W, BLOCK_ON_TABLE, H - 4, 6)
    cells[n - 1] = _blocks(H, W)
    rule, rules = _rule_args(rule_mode, n, SENS_RULES)
    boards = pack(cells)
    hit = 2 if scan == SCAN_SETTLE else 3
    c = dict(id=f"{inst_id(inst)}-{tag}-{H}x{W}", inst=inst, tag=tag, wclass="", H=H, W=W, n=n, turns=4, turn0=0, done=0,
             have_prev=False, write_prev=bool(aged), rule=rule, rules=rules, boards=boards, prev=_gap_like(boards),
             settled=np.full(n, -1, np.int64), expect={"f": [-1, hit] * len(places) + [2 if scan == SCAN_SETTLE else 1] * 2,
                                                        "places": places})
    if lst:
        c["list"] = np.arange(n, dtype=np.int32)[::-1].copy()  # (neighbours in the list: different rules)
        c["count"] = c["slots"] = n
        c["count_kind"] = "eq"
    if aged:
        c["born"] = np.zeros(n, np.int64)
    return Case(**c)


@functools.lru_cache(maxsize=None)
def cases_of(inst):
    nw, rule_mode, scan, lst, aged = inst
    wc = width_classes(nw)
    out, k = [], 0
    for name, W in wc.items():
        out.append(_general(inst, "width", name, 5, W, k))
        k += 1
    for H in HEIGHTS:
        out.append(_general(inst, "height", "min", H, wc["min"], k))
        k += 1
    if nw == 16 and rule_mode == RULE_CONWAY:
        out.append(_general(inst, "big", "full", 512, 512, k))
    if lst:
        out.append(_general(inst, "zero-count", "min", 5, wc["min"], 3, count_kind="zero"))
    if aged:
        H, W = 17, max(17, wc["min"])
        out.append(_general(inst, "freeze", "", H, W, 1, count_kind="eq", cells=_pulsar_boards(9, H, W),
                            extra={"pulsars": (0, 5)}, turns=6, table_rule="B38/S23"))  # (a pulsar is one under B38/S23)
    if scan != SCAN_NONE:
        for W in sorted({32 * nw, wc.get("odd-nwr", 32 * nw)}):
            out.append(_sens(inst, "sens-words", 20, W, [(8, 32 * j + min(10, min(W - 32 * j, 32) - 8)) for j in range((W + 31) // 32)]))
        for H in (128, 512):
            out.append(_sens(inst, "sens-waves", H, wc["min"], [(64 * w + 20, 4) for w in range((H + 63) // 64)]))
    return out


# ---------------------------------------------------------------- the arguments of gol_dev_batch_step

STEP_ARGS = ("boards", "prev", "settled", "n", "H", "W", "turns", "turn0", "have_prev", "write_prev", "birth", "survive", "rules",
             "scan", "done", "list", "count", "slots", "left", "born")  # the entry's order, without the stream
BUFFERS = ("boards", "prev", "settled", "left", "born", "list", "count", "rules")


def launch_args(c, ptr):
    """The arguments of a case's launch by name: ptr(name) is the address of the buffer `name`, asked for the
    buffers the case has (a case always has boards and prev); a buffer it does not have is NULL."""
    has = {k: getattr(c, k) is not None for k in BUFFERS}
    a = {k: (ptr(k) if has[k] else None) for k in BUFFERS}
    a.update(n=c.n, H=c.H, W=c.W, turns=c.turns, turn0=c.turn0, have_prev=int(c.have_prev), write_prev=int(c.write_prev),
             birth=c.rule[0], survive=c.rule[1], scan=c.scan, done=c.done, slots=c.slots)
    return a


REFUSAL_SHAPE = (5, 5, 17)  # n, H, W of the buffers the refusal list is called on


def refusals(p):
    """(bad, good): the argument sets of gol_dev_batch_step, each a dict by name, that the entry refuses with
    GOL_EINVAL -- every path of its check -- and the six good ones they are made from, one per mode.  p: name ->
    the address of that buffer of REFUSAL_SHAPE (any non-null value where nothing is launched)."""
    n, H, W = REFUSAL_SHAPE
    base = dict(boards=p["boards"], prev=None, settled=None, n=n, H=H, W=W, turns=3, turn0=0, have_prev=0, write_prev=0, birth=8,
                survive=12, rules=None, scan=0, done=0, list=None, count=None, slots=0, left=None, born=None)
    scan = dict(prev=p["prev"], settled=p["settled"])
    lst = dict(list=p["list"], count=p["count"], slots=n)
    cyc = dict(scan, scan=2, **lst)
    aged = dict(cyc, born=p["born"], write_prev=1)
    bad = [
        # the shape, the turns, the masks
        dict(boards=None), dict(n=0), dict(n=(1 << 20) + 1), dict(H=0), dict(H=513), dict(W=0), dict(W=513), dict(turns=0),
        dict(turns=-1), dict(birth=512), dict(survive=512), dict(done=-1),
        # the scan's buffers and flags
        dict(settled=p["settled"], scan=1), dict(have_prev=1), dict(write_prev=1), dict(scan=1), dict(scan=2), dict(scan, scan=0),
        dict(scan, scan=3), dict(scan=-1), dict(scan, scan=2, have_prev=1), dict(scan, scan=2, done=4), dict(slots=n),
        # the list
        dict(cyc, count=None), dict(cyc, list=None), dict(cyc, slots=0), dict(cyc, slots=n + 1), dict(cyc, left=p["left"]),
        dict(lst), dict(cyc, scan=1), dict(cyc, scan=0), dict(lst, left=p["left"], scan=2), dict(lst, left=p["left"], have_prev=1),
        dict(lst, left=p["left"], write_prev=1), dict(left=p["left"]),
        # the aged launch
        dict(aged, settled=None), dict(aged, prev=None), dict(aged, list=None), dict(aged, count=None), dict(aged, slots=0),
        dict(aged, slots=n + 1), dict(aged, rules=p["rules"]), dict(aged, left=p["left"]), dict(aged, turn0=1), dict(aged, write_prev=0),
        dict(aged, have_prev=1), dict(aged, done=3), dict(aged, scan=0), dict(aged, scan=1), dict(born=p["born"]),
    ]
    # (each family's base arguments are good)
    good = [dict(), dict(scan, scan=1), dict(cyc), dict(lst, left=p["left"]), dict(aged), dict(aged, have_prev=1, done=3)]
    return [dict(base, **kw) for kw in bad], [dict(base, **kw) for kw in good]


# ---------------------------------------------------------------- what the tests of golhip.Batch and its host twins share


def to_words(cells):
    """uint8[..., H, W] cells (non-zero = alive) as uint64[..., H, ceil(W / 64)]: bit c % 64 of word
    c // 64 of a row is cell c, written out bit by bit (independent of the library's packing)."""
    cells = np.asarray(cells) != 0
    W = cells.shape[-1]
    out = np.zeros(cells.shape[:-1] + ((W + 63) // 64,), dtype=np.uint64)
    for c in range(W):
        out[..., c // 64] |= cells[..., c].astype(np.uint64) << np.uint64(c % 64)
    return out


def from_words(words, W):
    """The inverse: uint8[..., H, W] of 0 / 1."""
    words = np.asarray(words, dtype=np.uint64)
    out = np.zeros(words.shape[:-1] + (W,), dtype=np.uint8)
    for c in range(W):
        out[..., c] = (words[..., c // 64] >> np.uint64(c % 64)) & np.uint64(1)
    return out


def tail_mask(W):
    return np.uint64((1 << (W % 64)) - 1 if W % 64 else 2 ** 64 - 1)


# (board, turns, (found, period) as the reference must give them)
PATTERNS = [
    (C.place(5, 5, []), 10, (1, 1)),
    (C.place(5, 5, C.BLOCK, 1, 1), 10, (1, 1)),
    (C.place(5, 5, C.BLINKER, 2, 1), 10, (3, 2)),
    (C.place(17, 17, C.PULSAR, 2, 2), 40, (6, 3)),
    (C.place(129, 65, C.PULSAR, 57, 58), 40, (6, 3)),
    (C.place(20, 20, C.ROW10, 10, 5), 100, (30, 15)),
    (C.place(130, 33, C.ROW10, 0, 28), 100, (30, 15)),
    (C.place(129, 65, C.ROW10, 63, 60), 100, (30, 15)),
    (C.place(8, 8, C.GLIDER), 200, (63, 32)),
    (C.place(16, 16, C.GLIDER), 400, (127, 64)),
    (C.place(7, 9, C.GLIDER), 600, (507, 252)),
    (C.place(16, 16, C.R_PENTOMINO, 6, 6), 300, (129, 2)),
]


def batch_n(G, H, W):
    """Two full workgroups and one board in a third; at least 3."""
    with G.Batch(1, H, W) as b:
        info = b.info()
    assert info["waves_per_board"] == (H + 63) // 64 and info["words_per_lane"] >= (W + 31) // 32
    return max(3, 2 * info["boards_per_workgroup"] + 1)


def random_boards(seed, n, H, W):
    """n different boards of 0 / 1 at densities 0.2 .. 0.6."""
    return np.stack([R.random_board(seed + i, H, W, 0.2 + 0.4 * i / max(n - 1, 1)) for i in range(n)])


def check_queries(b, cells):
    """store, store_words, alive_counts and hashes of the batch against the cells (0 / 1) it should hold."""
    words = to_words(cells)
    got = b.store_words()
    assert got.shape == words.shape and np.array_equal(got, words)
    assert np.array_equal(b.store(), cells * 255)
    assert b.alive_counts().tolist() == [O.popcount_words(w) for w in words]
    assert b.hashes().tolist() == [O.hash_words(w) for w in words]


def ref_settle(board, rule, turns):
    """(the first t in [2, turns] with state(t) == state(t - 2), else -1; state(turns))."""
    states = [np.asarray(board, dtype=np.uint8)]
    found = -1
    for t in range(1, turns + 1):
        states.append(R.step(states[-1], *rule))
        if found < 0 and t >= 2 and np.array_equal(states[t], states[t - 2]):
            found = t
    return found, states[-1]
