"""A numpy model of the board engine's documented behaviour and a generator of random sequences of
its public calls (helper of tests/test_engine_model_cpu.py and tests/test_gpu_sequences.py, not a
test; no GPU, and golhip is imported only inside run()).

The model holds what include/golhip.h lets a caller observe -- the board's raw bytes, the turn, the
rule, whether the exact first turn is pending, and the layout an in-place call reports next -- and
nothing of buffers, halos, slots or streams.  It steps with the references the suite already trusts
(oracle.run for B3/S23 on bytes, tests/rule_ref.py for every other rule); its paste, copy and bounds
are numpy index arithmetic.  Where the header is silent the model does what an existing per-feature
test pins, named in a comment at that place.

An op is a record (name, args) of plain Python values, so a list of ops prints as a literal that
can be pasted back into replay().  apply(model, op) is the expected result, run(engine, op) the
engine's in the same shape; a call that must fail is ("error", code) in both.
"""
import numpy as np

import rule_ref as R
from oracle import oracle as O

EINVAL, ESTATE = -1, -6  # GOL_EINVAL, GOL_ESTATE (include/golhip.h)
CONWAY = (0x008, 0x00C)
RULES = [("B3/S23", False), ("B3/S23", True), ("B36/S23", False), ("B3678/S34678", False), ("B1357/S1357", False)]
ODD_BYTES = [0, 255, 1, 7, 128, 254]
STEP_TURNS = [0, 1, 2, 3, 5, 8, 12, 13, 24, 33, 40]
SCALES = [1, 2, 3, 8]
PASTE_OPS = ["copy", "or", "xor", "andnot"]

# The smallest boards on which every path still exists (tests/test_gpu_sequences.py has the table).
CONFIGS = {c["id"]: c for c in [
    dict(id="band1", H=48, W=1024, engine=dict(layout="band")),
    dict(id="band3", H=80, W=2048, engine=dict(layout="band", shards=3, same_device=True)),
    dict(id="std2", H=50, W=192, engine=dict(layout="standard", shards=2, same_device=True)),
    dict(id="bytes", H=40, W=128, engine=dict(layout="bytes")),
    dict(id="w32", H=36, W=96, engine=dict()),
    dict(id="odd", H=33, W=48, engine=dict()),
]}

# The fixed sequences of both test files: LENGTH ops from each of these seeds.  The seeds are chosen
# so that the conditions of tests/test_engine_model_cpu.py hold (it asserts them).
LENGTH = 40
SEEDS = {"band1": [456, 457, 458, 459, 460, 461], "band3": [24, 62, 108, 128, 142, 215],
         "std2": [2976, 2977, 2978, 2979, 2980, 2981], "bytes": [60, 61, 62, 63, 64, 65],
         "w32": [138, 139, 140, 141, 142, 143], "odd": [138, 139, 140, 141, 142, 143]}

CLASSES = {
    "load": ["load_random", "load_bytes", "load_words"],
    "step": ["step", "step_counted", "step_flips"],
    "convert": ["store_bytes", "store_rows", "store_words", "hash", "alive_cells", "write_pgm_to"],
    "inplace": ["alive_count", "turn", "view_counts", "view", "copy", "bounds", "to_rle", "info_k"],
    "edit": ["paste", "fill", "cut"],
    "setting": ["set_rule", "set_timing"],
}
CLASS_OF = {name: cls for cls, names in CLASSES.items() for name in names}
HALO_STALE = ("paste", "fill", "cut", "load_words")  # the calls after which the generator steps half of the time
CLASS_WEIGHTS = {"load": .13, "step": .20, "convert": .16, "inplace": .21, "edit": .17, "setting": .13}


class ModelError(Exception):
    def __init__(self, code):
        super().__init__(code)
        self.code = code


class Mismatch(AssertionError):
    """replay()'s first difference: .index is the op's index (len(ops) for the checks at the end)."""

    def __init__(self, message, index):
        super().__init__(message)
        self.index = index


# ------------------------------------------------------------------ the data of an op, from its seeds
def make_bytes(H, W, seed, density, odd):
    """A byte board: alive cells 255, with `odd` one in five of them another byte of ODD_BYTES."""
    rng = np.random.default_rng(seed)
    board = np.where(rng.random((H, W)) < density, 255, 0).astype(np.uint8)
    if odd:
        other = rng.choice(np.array(ODD_BYTES[2:], dtype=np.uint8), size=(H, W))
        board = np.where((board != 0) & (rng.random((H, W)) < 0.2), other, board).astype(np.uint8)
        if np.isin(board, (0, 255)).all():
            board[H // 2, W // 2] = 7
    return board


def make_words(rows, Ww, seed):
    return np.random.default_rng(seed).integers(0, 2 ** 64, (rows, Ww), dtype=np.uint64)


def make_pattern(h, w, pseed, flip=None):
    p = np.random.default_rng(pseed).random((h, w)) < 0.5
    if flip is not None:
        p[flip] = ~p[flip]
    return p


def shard_seams(config):
    """The first row of every shard (gol_partition_rows): row 0 is the seam of the torus wrap."""
    n = config["engine"].get("shards", 1)
    return [O.partition(config["H"], n, i)[0] for i in range(n)]


def crosses_seam(y0, h, H, seams):
    return any(0 < (b - y0) % H < h for b in seams)


# ------------------------------------------------------------------ the model
class Model:
    def __init__(self, H, W, layout="auto", shards=1):
        self.H, self.W, self.shards = H, W, shards
        self.bit = W % 64 == 0 and layout != "bytes"  # golhip.h, "Bit-board layout used while stepping"
        self.band = self.bit and layout != "standard" and W % 1024 == 0
        self.board = np.zeros((H, W), np.uint8)
        self.turn = 0
        self.rule, self.birth, self.survive, self.generic = "B3/S23", *CONWAY, False
        self.pending = False  # the exact first turn of a bit board loaded with bytes other than 0/255
        self.layout = "standard" if self.bit else "bytes"

    @classmethod
    def of(cls, config):
        e = config["engine"]
        return cls(config["H"], config["W"], e.get("layout", "auto"), e.get("shards", 1))

    def alive(self):
        return self.board != 0  # "Number of cells != 0": what alive_count, the views and the copy count

    def density(self):
        return np.count_nonzero(self.board) / self.board.size

    # -- helpers
    def _loaded(self):
        self.turn = 0
        self.pending = self.bit and not np.isin(self.board, (0, 255)).all()
        self.layout = "standard" if self.bit and not self.pending else "bytes"

    def _to_standard(self):
        """The readers that see the standard layout convert a band board to it (golhip.h, layouts)."""
        if self.layout == "band":
            self.layout = "standard"

    def _conway(self):
        return (self.birth, self.survive) == CONWAY

    def _step_check(self):
        if self.pending and not self._conway():  # golhip.h, gol_engine_set_rule
            raise ModelError(ESTATE)

    def _run(self, n):
        if self._conway():
            return O.run(self.board, n)
        return R.to_bytes(R.run(self.board, (self.birth, self.survive), n)[0])

    def _advance(self, n, band=True):
        if n <= 0:
            return
        if self.pending:  # turn 1 from the loaded bytes, then a bit board in the standard layout
            self.board = O.run(self.board, 1)
            self.pending = False
            self.layout = "standard"
            self.turn += 1
            n -= 1
        if n > 0:
            self.board = self._run(n)
            self.turn += n
            if self.bit:
                self.layout = "band" if self.band and band else "standard"

    def _rect_check(self, x0, y0, w, h):
        if not (1 <= w <= self.W and 1 <= h <= self.H and 0 <= x0 < self.W and 0 <= y0 < self.H):
            raise ModelError(EINVAL)

    def _ix(self, x0, y0, w, h):
        return np.ix_((y0 + np.arange(h)) % self.H, (x0 + np.arange(w)) % self.W)

    def _paste(self, x0, y0, p, op):
        """As np_paste of tests/test_gpu_edit.py; written cells become 0 / 255 and, on byte rows, the
        others keep their byte (test_bytes_paste_keeps_untouched_odd_bytes)."""
        h, w = p.shape
        self._rect_check(x0, y0, w, h)
        if self.pending:
            raise ModelError(ESTATE)
        ix = self._ix(x0, y0, w, h)
        old = self.board[ix] != 0
        new = {"copy": p, "or": old | p, "xor": old ^ p, "andnot": old & ~p}[op]
        written = np.ones_like(p) if op == "copy" else p
        self.board[ix] = np.where(written, np.where(new, 255, 0), self.board[ix]).astype(np.uint8)
        return int(np.count_nonzero(new != old)), self.layout

    def _cells_list(self, mask, cap):
        ys, xs = np.nonzero(mask)  # row-major
        out = [[int(x), int(y)] for x, y in zip(xs, ys)]
        return out if cap is None else out[:cap]

    # -- loads
    def op_load_random(self, seed):
        if self.W % 64:
            raise ModelError(EINVAL)
        self.board = O.unpack(O.random_words(seed, 0, self.H, self.W // 64))
        self._loaded()

    def op_load_bytes(self, seed, density, odd):
        self.board = make_bytes(self.H, self.W, seed, density, odd)
        self._loaded()

    def op_load_words(self, y0, rows, seed):
        if not self.bit or y0 < 0 or y0 + rows > self.H:
            raise ModelError(EINVAL)
        if self.pending:  # golhip.h, load_words: the pending first turn is void, the 255-cells stay
            self.board = np.where(self.board == 255, 255, 0).astype(np.uint8)
            self.pending = False
        self.board = self.board.copy()
        self.board[y0:y0 + rows] = O.unpack(make_words(rows, self.W // 64, seed))
        self.turn = 0
        self.layout = "standard"

    # -- steps
    def op_step(self, n):
        self._step_check()
        self._advance(n)

    def op_step_counted(self, turns, every):
        self._step_check()
        counts, left = [], turns
        while left > 0:
            seg = min(every, left)
            self._advance(seg)
            if seg == every:
                counts.append(int(np.count_nonzero(self.board)))
            left -= seg
        return counts

    def op_step_flips(self, cap):
        """One turn on standard rows whatever the layout was; a non-zero byte that dies is a flip
        (test_step_flips_non_binary_first_turn)."""
        self._step_check()
        before = self.alive()
        if not self.pending:
            self._to_standard()
        self._advance(1, band=False)
        return self._cells_list(before != self.alive(), cap)

    # -- reads that see the standard layout
    def op_store_bytes(self):
        self._to_standard()
        return self.board.copy()

    def op_store_rows(self, y0, y1):
        if not 0 <= y0 <= y1 <= self.H:
            raise ModelError(EINVAL)
        self._to_standard()
        return self.board[y0:y1].copy()

    def op_store_words(self, y0, y1):
        if not self.bit or not 0 <= y0 <= y1 <= self.H:
            raise ModelError(EINVAL)
        if self.pending:
            raise ModelError(ESTATE)
        self._to_standard()
        return O.pack(self.board[y0:y1])

    def op_hash(self):
        """Before the exact first turn: of the 255-cells (test_uneven_shards_exact_rows_from_pgm)."""
        if not self.bit:
            raise ModelError(EINVAL)
        self._to_standard()
        return O.hash_words(O.pack(np.where(self.board == 255, 255, 0).astype(np.uint8)))

    def op_alive_cells(self, cap):
        """Bytes != 0 before turn 1 (test_non_binary_bytes_first_turn)."""
        self._to_standard()
        return self._cells_list(self.alive(), cap)

    def op_write_pgm_to(self):
        self._to_standard()
        return O.pgm_bytes(self.board)

    # -- reads in place
    def op_alive_count(self):
        return int(np.count_nonzero(self.board))

    def op_turn(self):
        return self.turn

    def _view_counts(self, x0, y0, scale, out_w, out_h):
        if not (1 <= scale and out_w >= 1 and out_h >= 1 and out_w * scale <= self.W and out_h * scale <= self.H
                and 0 <= x0 < self.W and 0 <= y0 < self.H):
            raise ModelError(EINVAL)
        box = np.roll(self.alive(), (-y0, -x0), (0, 1))[:out_h * scale, :out_w * scale]
        return box.reshape(out_h, scale, out_w, scale).sum(axis=(1, 3)).astype(np.uint32)

    def op_view_counts(self, x0, y0, scale, out_w, out_h):
        return self._view_counts(x0, y0, scale, out_w, out_h), self.layout

    def op_view(self, x0, y0, scale, out_w, out_h):
        n = self._view_counts(x0, y0, scale, out_w, out_h).astype(np.int64)
        return ((255 * n + scale * scale - 1) // (scale * scale)).astype(np.uint8), self.layout

    def op_copy(self, x0, y0, w, h):
        self._rect_check(x0, y0, w, h)
        cells = self.alive()[self._ix(x0, y0, w, h)]
        return cells, int(np.count_nonzero(cells)), self.layout

    def op_bounds(self, x0, y0, w, h):
        self._rect_check(x0, y0, w, h)
        ys, xs = np.nonzero(self.alive()[self._ix(x0, y0, w, h)])
        if len(ys) == 0:
            return (0, 0, 0, 0, 0)
        return (int(xs.min()), int(ys.min()), int(xs.max() - xs.min() + 1), int(ys.max() - ys.min() + 1), len(ys))

    def op_to_rle(self, x0, y0, w, h):
        """Engine.to_rle with trim: the bounding box of the alive cells (none: the 1 x 1 dead pattern)
        under the current rule's canonical text."""
        bx, by, bw, bh, _ = self.op_bounds(x0, y0, w, h)
        cells = self.alive()[self._ix((x0 + bx) % self.W, (y0 + by) % self.H, max(bw, 1), max(bh, 1))]
        return cells, self.rule

    def op_info_k(self):
        """turns_per_launch, where the header states it: 1 while the exact first turn is pending
        (None: not compared)."""
        return 1 if self.pending else None

    # -- edits
    def op_paste(self, x0, y0, w, h, op, pseed, flip=None):
        return self._paste(x0, y0, make_pattern(h, w, pseed, flip), op)

    def op_fill(self, x0, y0, w, h, op):
        return self._paste(x0, y0, np.ones((h, w), bool), op)

    def op_cut(self, x0, y0, w, h):
        self._rect_check(x0, y0, w, h)
        if self.pending:
            raise ModelError(ESTATE)
        got = self.op_copy(x0, y0, w, h)
        self._paste(x0, y0, np.ones((h, w), bool), "andnot")
        return got

    # -- settings
    def op_set_rule(self, text, generic):
        birth, survive = R.masks(text)
        if ((birth, survive) != CONWAY or generic) and not self.bit:
            raise ModelError(EINVAL)
        self.rule, self.birth, self.survive = text, birth, survive
        self.generic = (birth, survive) != CONWAY or generic

    def op_set_timing(self, on, exchanges):
        return None


def is_error(res):
    return isinstance(res, tuple) and len(res) == 2 and isinstance(res[0], str) and res[0] == "error"


def apply(model, op):
    """The expected result of op; a call that must fail is ("error", code) and changes nothing."""
    name, args = op
    try:
        return getattr(model, "op_" + name)(*args)
    except ModelError as x:
        return ("error", x.code)


# ------------------------------------------------------------------ the same call on an engine
def run(engine, op):
    """Perform op on a golhip.Engine (or a ModelEngine); the result in apply()'s shape."""
    if hasattr(engine, "apply_op"):
        return engine.apply_op(op)
    name, a = op
    e = engine
    try:
        if name == "load_random":
            return e.load_random(*a)
        if name == "load_bytes":
            return e.load_bytes(make_bytes(e.H, e.W, *a))
        if name == "load_words":
            return e.load_words(a[0], make_words(a[1], e.W // 64, a[2]))
        if name == "step":
            return e.step(*a)
        if name == "step_counted":
            return e.step_counted(*a).tolist()
        if name in ("step_flips", "alive_cells"):
            return getattr(e, name)(*a).tolist()
        if name in ("store_bytes", "store_rows", "store_words", "hash", "alive_count", "bounds"):
            return getattr(e, name)(*a)
        if name == "write_pgm_to":
            buf = bytearray()

            def sink(off, data):
                if len(buf) < off + len(data):
                    buf.extend(bytes(off + len(data) - len(buf)))
                buf[off:off + len(data)] = bytes(data)
            e.write_pgm_to(sink)
            return bytes(buf)
        if name == "turn":
            return e.turn
        if name in ("view_counts", "view"):
            return getattr(e, name)(*a, return_layout=True)
        if name in ("copy", "cut"):
            import golhip
            words, n, lay = e.copy_words(*a, cut=name == "cut", return_layout=True)
            return golhip._lib.unpack_pattern(words, a[2]), n, lay
        if name == "to_rle":
            import golhip
            return golhip.parse_rle(e.to_rle(*a))
        if name == "info_k":
            return e.info()["turns_per_launch"]
        if name == "paste":
            x0, y0, w, h, pop, pseed = a[:6]
            return e.paste(make_pattern(h, w, pseed, *a[6:]), x0, y0, pop, return_layout=True)
        if name == "fill":
            return e.fill(*a, return_layout=True)
        if name == "set_rule":
            return e.set_rule(*a)
        if name == "set_timing":
            return e.set_timing(*a)
    except Exception as x:  # GolError: the documented code
        if not hasattr(x, "code"):
            raise
        return ("error", x.code)
    raise ValueError(f"unknown op {name!r}")


def same(want, got):
    """Exact equality of two results: arrays by shape and values, sequences element by element."""
    if isinstance(want, np.ndarray) or isinstance(got, np.ndarray):
        return (isinstance(want, np.ndarray) and isinstance(got, np.ndarray) and want.shape == got.shape
                and np.array_equal(want, got))
    if isinstance(want, (tuple, list)):
        return (isinstance(got, (tuple, list)) and len(want) == len(got)
                and all(same(a, b) for a, b in zip(want, got)))
    return type(want) is type(got) and want == got


def same_result(op, want, got):
    if op[0] == "info_k" and want is None:  # the header names no value here
        return got is None or isinstance(got, int)  # (None: a ModelEngine)
    return same(want, got)


class ModelEngine:
    """A second model behind the few calls replay() makes, standing in for the engine (the
    self-check of tests/test_engine_model_cpu.py).  tamper = (index, (r, c)): the paste that is op
    `index` gets cell (r, c) of its pattern flipped."""

    def __init__(self, config, tamper=None):
        self.model = Model.of(config)
        self.H, self.W = config["H"], config["W"]
        self.tamper, self.n = tamper, 0

    def apply_op(self, op):
        if self.tamper and self.n == self.tamper[0]:
            assert op[0] == "paste" and len(op[1]) == 6
            op = (op[0], op[1] + (self.tamper[1],))
        self.n += 1
        return apply(self.model, op)

    def view(self, x0, y0, scale, out_w, out_h, return_layout=False):
        return self.model.op_view(x0, y0, scale, out_w, out_h)

    def alive_count(self):
        return self.model.op_alive_count()

    @property
    def turn(self):
        return self.model.turn

    def store_bytes(self):
        return self.model.op_store_bytes()

    def hash(self):
        return self.model.op_hash()

    def close(self):
        pass


# ------------------------------------------------------------------ comparing the whole board
def check_board(engine, model):
    """The whole board without disturbing the state under test: one full view at scale 1 (read in
    place, with the layout it reports), the alive count and the turn.  Never store_bytes: it converts
    the layout.  Returns the first difference as text, None if there is none."""
    pix, lay = engine.view(0, 0, 1, model.W, model.H, return_layout=True)
    if lay != model.layout:
        return f"view reads layout {lay!r}, expected {model.layout!r}"
    want = np.where(model.alive(), 255, 0).astype(np.uint8)  # test_gpu_view: a non-zero byte is alive
    if not np.array_equal(pix, want):
        ys, xs = np.nonzero(pix != want)
        return f"board differs in {len(ys)} cells, rows {sorted(set(ys.tolist()))[:12]}, first (x, y) = ({xs[0]}, {ys[0]})"
    n = engine.alive_count()
    if n != model.op_alive_count():
        return f"alive_count {n}, expected {model.op_alive_count()}"
    if engine.turn != model.turn:
        return f"turn {engine.turn}, expected {model.turn}"
    return None


def check_end(engine, model):
    """The end of a sequence: check_board, then the bytes and (bit boards, no exact turn pending) the hash."""
    bad = check_board(engine, model)
    if bad:
        return bad
    if not same(model.op_store_bytes(), engine.store_bytes()):
        return "store_bytes differs"
    if model.bit and not model.pending and engine.hash() != model.op_hash():
        return "hash differs"
    return None


def short(x, limit=300):
    s = repr(x.tolist() if isinstance(x, np.ndarray) else x)
    return s if len(s) <= limit else s[:limit] + " ..."


def replay(engine_factory, config, ops, checks=None, seed=None):
    """Run ops against a fresh engine (engine_factory(config)) and a fresh model; checks[i] = run
    check_board after op i; check_end after the last.  Raises Mismatch at the first difference, with
    the config, the seed, the index and the ops up to there as a literal for another replay()."""
    model = Model.of(config)
    engine = engine_factory(config)

    def fail(i, what):
        n = min(i + 1, len(ops))
        return Mismatch(f"{what}\nconfig = {config!r}\nseed = {seed!r}\nindex = {i}\n"
                        f"ops = {list(ops[:n])!r}\nchecks = {list(checks[:n]) if checks else None!r}\n"
                        "# replay(engine_factory, config, ops, checks)", i)
    try:
        for i, op in enumerate(ops):
            want = apply(model, op)
            got = run(engine, op)
            if not same_result(op, want, got):
                raise fail(i, f"op {i} {op!r} returned {short(got)}, expected {short(want)}")
            if checks and checks[i]:
                bad = check_board(engine, model)
                if bad:
                    raise fail(i, f"after op {i} {op!r}: {bad}")
        bad = check_end(engine, model)
        if bad:
            raise fail(len(ops), f"at the end: {bad}")
    finally:
        engine.close()
    return model


# ------------------------------------------------------------------ the generator
def check_points(seed, length):
    """After which ops check_board runs: probability one half, from the sequence's seed."""
    return (np.random.default_rng([seed, 1]).random(length) < 0.5).tolist()


def valid_names(config):
    """The op names that can succeed on this board."""
    bit = Model.of(config).bit
    out = []
    for names in CLASSES.values():
        for n in names:
            if n == "load_random" and config["W"] % 64:
                continue
            if n in ("load_words", "store_words", "hash") and not bit:
                continue
            out.append(n)  # (set_rule: plain B3/S23 is legal on every board)
    return out


class _Gen:
    def __init__(self, config, seed, length):
        self.c, self.rng, self.length = config, np.random.default_rng([seed, 0]), length
        self.m = Model.of(config)
        self.seams = shard_seams(config)
        self.ops, self.failures = [], 0
        self.names = valid_names(config)

    def ri(self, lo, hi):  # [lo, hi]
        return int(self.rng.integers(lo, hi + 1))

    def pick(self, xs):
        return xs[int(self.rng.integers(0, len(xs)))]

    def emit(self, name, *args):
        if self.m.pending and name in ("paste", "fill", "cut", "store_words") and not self.budget():
            return  # (ESTATE while the exact turn is pending: only as a deliberate failure)
        op = (name, tuple(args))
        res = apply(self.m, op)
        if is_error(res):
            self.failures += 1
        self.last_ok = not is_error(res)
        self.ops.append(op)

    def rect(self, small=None, cross=False):
        H, W, r = self.m.H, self.m.W, self.rng.random()
        if small:
            w, h = self.ri(1, min(W, small)), self.ri(1, min(H, small))
        elif r < .10:
            w = h = 1
        elif r < .45:
            w, h = self.ri(1, min(W, 40)), self.ri(1, min(H, 16))
        elif r < .85:
            w, h = self.ri(1, W), self.ri(1, H)
        elif r < .93:
            w, h = W, self.ri(1, H)
        else:
            w, h = W, H
        x0, y0 = self.ri(0, W - 1), self.ri(0, H - 1)
        if w > 1 and self.rng.random() < .3:
            x0 = W - self.ri(1, w - 1)  # wraps in x
        if cross and h > 1:
            y0 = (self.pick(self.seams) - self.ri(1, h - 1)) % H
        return x0, y0, w, h

    # -- one op of each class
    def load(self):
        kinds = ["bytes", "odd"] + (["random"] if "load_random" in self.names else [])
        kinds += ["words_all", "words_part"] if self.m.bit else []
        if self.m.bit and self.ops and CLASS_OF[self.ops[-1][0]] == "step":
            kinds += ["words_all", "words_part", "words_part"]  # rows replaced under a halo a step left valid
        kind = self.pick(kinds)
        if kind == "random":
            self.emit("load_random", self.ri(1, 1 << 30))
        elif kind in ("bytes", "odd"):
            self.emit("load_bytes", self.ri(1, 1 << 30), self.pick([.2, .35, .5]), kind == "odd")
        elif kind == "words_all":
            self.emit("load_words", 0, self.m.H, self.ri(1, 1 << 30))
        else:
            y0 = self.ri(0, self.m.H - 2)
            self.emit("load_words", y0, self.ri(1, self.m.H - 1 - y0), self.ri(1, 1 << 30))

    def step(self):
        kind = self.pick(["step", "step", "step_counted", "step_flips"])
        if kind == "step":
            self.emit("step", self.pick(STEP_TURNS))
        elif kind == "step_counted":
            turns = self.pick(STEP_TURNS[1:])
            every = self.pick([1, turns + self.ri(1, 3), self.ri(1, turns), 12, 5])
            self.emit("step_counted", turns, every)
        else:
            self.emit("step_flips", self.ri(1, 40) if self.rng.random() < .25 else None)

    def convert(self):
        names = [n for n in CLASSES["convert"] if n in self.names]
        name = self.pick(names)
        if name in ("store_rows", "store_words"):
            y0 = self.ri(0, self.m.H - 1)
            self.emit(name, y0, self.ri(y0 + 1, self.m.H))
        elif name == "alive_cells":
            n = self.m.op_alive_count()
            self.emit(name, self.ri(0, n - 1) if n and self.rng.random() < .25 else None)
        else:
            self.emit(name)

    def inplace(self):
        name = self.pick(CLASSES["inplace"])
        if name in ("view", "view_counts"):
            s = self.pick([s for s in SCALES if s <= min(self.m.H, self.m.W)])
            ow, oh = self.ri(1, self.m.W // s), self.ri(1, self.m.H // s)
            x0, y0 = self.ri(0, self.m.W - 1), self.ri(0, self.m.H - 1)
            if self.rng.random() < .4:
                x0 = self.m.W - self.ri(1, max(1, ow * s - 1))
            if self.rng.random() < .4:
                y0 = self.m.H - self.ri(1, max(1, oh * s - 1))
            self.emit(name, x0, y0, s, ow, oh)
        elif name in ("copy", "bounds"):
            self.emit(name, *self.rect(cross=self.rng.random() < .5))
        elif name == "to_rle":
            self.emit(name, *self.rect(small=24))
        else:
            self.emit(name)

    def edit(self):
        """An edit that keeps the board between 3 % and 97 % alive (a board that is all dead or all
        alive tests nothing); half of them across a shard seam on purpose."""
        for _ in range(8):
            name = self.pick(["paste", "paste", "fill", "cut"])
            x0, y0, w, h = self.rect(cross=self.rng.random() < .5)
            if name == "paste":
                args = (x0, y0, w, h, self.pick(PASTE_OPS), self.ri(1, 1 << 30))
            elif name == "fill":
                args = (x0, y0, w, h, self.pick(PASTE_OPS))
            else:
                args = (x0, y0, w, h)
            if self.m.pending:
                break  # (fails with ESTATE: nothing to keep alive)
            trial = Model.of(self.c)
            trial.board, trial.layout = self.m.board.copy(), self.m.layout
            apply(trial, (name, args))
            if .03 < trial.density() < .97:
                break
        else:
            name, args = "paste", (x0, y0, 1, 1, "xor", 1)
        self.emit(name, *args)

    def setting(self):
        if self.rng.random() < .3:
            self.emit("set_timing", bool(self.rng.random() < .7), bool(self.rng.random() < .5))
        elif not self.m.bit:
            self.emit("set_rule", "B3/S23", False)
        else:
            rules = RULES if not self.m.pending or self.budget() else RULES[:2]
            self.emit("set_rule", *self.pick(rules))

    # -- calls that must fail
    def budget(self):
        return self.failures < self.length // 10

    def failure(self):
        H, W = self.m.H, self.m.W
        kinds = ["wide", "rows"]
        if not self.m.bit:
            kinds += ["hash", "load_words", "store_words", "rule"]
        if self.m.pending:
            kinds += ["pending"] * 3
        kind = self.pick(kinds)
        if kind == "wide":
            x0, y0, w, h = self.rect()
            if self.rng.random() < .5:
                w = W + self.ri(1, 5)
            else:
                h = H + self.ri(1, 5)
            name = self.pick(["paste", "fill", "copy", "cut", "bounds"])
            extra = {"paste": (self.pick(PASTE_OPS), 3), "fill": (self.pick(PASTE_OPS),)}.get(name, ())
            self.emit(name, x0, y0, w, h, *extra)
        elif kind == "rows":
            self.emit("store_rows", self.ri(0, H - 1), H + self.ri(1, 3))
        elif kind == "hash":
            self.emit("hash")
        elif kind == "load_words":
            self.emit("load_words", 0, self.ri(1, H), 5)
        elif kind == "store_words":
            self.emit("store_words", 0, self.ri(1, H))
        elif kind == "rule":
            self.emit("set_rule", *self.pick(RULES[1:]))
        else:
            name = self.pick(["paste", "store_words", "cut"])
            if name == "store_words":
                self.emit(name, 0, self.ri(1, H))
            else:
                x0, y0, w, h = self.rect()
                self.emit(name, x0, y0, w, h, *(("xor", 7) if name == "paste" else ()))

    def generate(self):
        classes = list(CLASS_WEIGHTS)
        p = np.array([CLASS_WEIGHTS[c] for c in classes])
        self.load()
        while len(self.ops) < self.length:
            m = self.m
            stuck = m.pending and not m._conway()  # every step fails until the rule or the board changes
            if self.ops[-1][0] in HALO_STALE and self.last_ok and not stuck and self.rng.random() < .5:
                self.emit("step", self.pick(STEP_TURNS[6:]))  # 12 .. 40 turns: launches behind the stale halo
                continue
            if self.budget() and self.rng.random() < (.3 if m.pending else .07):
                self.failure()
                continue
            cls = classes[int(self.rng.choice(len(classes), p=p / p.sum()))]
            if not m.pending and not .04 < m.density() < .96:
                cls = "load"  # reloads keep the board interesting
            if cls == "step" and stuck and not self.budget():
                self.emit("set_rule", "B3/S23", False)
                continue
            getattr(self, cls)()
        return self.ops


def generate(config, seed, length):
    """`length` ops for this board from np.random.default_rng: only ops valid for its mode, plus at
    most one in ten that must fail; the first is a load.  Deterministic."""
    return _Gen(config, seed, length).generate()


def trace(config, ops):
    """The model's walk through ops: (index, op, result, model) after each op (the model is live:
    read what you need at once)."""
    m = Model.of(config)
    for i, op in enumerate(ops):
        res = apply(m, op)
        yield i, op, res, m
