"""Expectations and the case table of the step-kernel tests (a helper, not a test; pure numpy).

The step kernels of csrc/gol_kernels.hip behind gol_dev_bits_step, gol_dev_band_step and
gol_dev_rule_step are about 40 template instantiations.  tests/test_gpu_step_kernels.py runs
every one of them on caller-owned memory at the smallest shapes that sit on an edge of its
arithmetic and compares the written rows, bit for bit, with the numpy torus stepper of
tests/rule_ref.py.  This module holds what that comparison needs and no GPU:

* the two bit layouts for ANY width in words (odd ones too): standard rows (bit i of word s =
  cell 32 s + i) and band rows (bit b of word w = cell b Wd + w);
* expected(): rows [y0, y0 + R) of a torus after k turns;
* CASES: the generated case table, with the memory picture of every case (which allocations,
  where top / mid / bot / dst point into them, what they hold before the launch);
* check_args(): the argument rules of include/golhip.h, restated;
* TABLE: the step kernels as csrc/gol_step_launch.h lists them, the engine-only one and the two
  pipelines included; refusals(): calls one change away from a good one, per family and clause of
  the launch check, shared by the CPU and GPU tests of the refusals.

tests/test_step_ref_cpu.py checks the helpers against the oracle and asserts the table's coverage.
"""
import functools
from dataclasses import dataclass

import numpy as np

import rule_ref as RR

SENT = 0x5A5A5A5A  # every word that is not board data: pitch padding, guard rows, all of dst
GUARD = 2          # sentinel rows above and below every allocation
RULE_DW = 2        # GOLK_RULE_DW (csrc/gol_step_launch.h): words per lane of the rule kernels
COUNT_SEED = (5, 1000003)  # (slot, value) the count slots hold before a launch
DENSITY = 0.4

CONWAY = "B3/S23"
RULES = (CONWAY, "B36/S23", "B0123478/S01234678")  # the last: birth on 0 neighbours (test_gpu_rules.py)

WIDTH_CLASSES = ("one-lane", "under-group", "exact-group", "one-lane-over")
FORMS = ("wrap", "contig", "separate")
STRIP_LENGTHS = tuple(range(1, 7))
R_SUB = 24  # shard rows of the wrap-form sub-range and strip-sweep cases


# ------------------------------------------------------------------ layouts
def std_pack(cells: np.ndarray) -> np.ndarray:
    """cells (H x 32 Wd, 0/1) -> standard rows (H x Wd uint32): bit i of word s = cell 32 s + i."""
    cells = np.ascontiguousarray(cells, dtype=np.uint8)
    H, W = cells.shape
    assert W % 32 == 0
    return np.packbits(cells, axis=1, bitorder="little").view("<u4").astype(np.uint32).reshape(H, W // 32)


def std_unpack(words: np.ndarray) -> np.ndarray:
    words = np.ascontiguousarray(words, dtype="<u4")
    H, Wd = words.shape
    return np.unpackbits(words.view(np.uint8), axis=1, bitorder="little").reshape(H, 32 * Wd)


def band_pack(cells: np.ndarray) -> np.ndarray:
    """cells (H x 32 Wd, 0/1) -> band rows (H x Wd uint32): bit b of word w = cell b Wd + w."""
    cells = np.ascontiguousarray(cells, dtype=np.uint8)
    H, W = cells.shape
    assert W % 32 == 0
    Wd = W // 32
    by_word = np.ascontiguousarray(cells.reshape(H, 32, Wd).transpose(0, 2, 1))  # [y, w, b]
    return np.packbits(by_word, axis=2, bitorder="little").view("<u4").astype(np.uint32).reshape(H, Wd)


def band_unpack(words: np.ndarray) -> np.ndarray:
    words = np.ascontiguousarray(words, dtype="<u4")
    H, Wd = words.shape
    by_word = np.unpackbits(words.view(np.uint8).reshape(H, Wd, 4), axis=2, bitorder="little")  # [y, w, b]
    return np.ascontiguousarray(by_word.transpose(0, 2, 1)).reshape(H, 32 * Wd)


def popcount(words: np.ndarray) -> int:
    return int(np.unpackbits(np.ascontiguousarray(words, dtype="<u4").view(np.uint8)).sum())


# ------------------------------------------------------------------ expectations
def expected(cells_torus: np.ndarray, y0: int, R: int, k: int, rule) -> np.ndarray:
    """Rows [y0, y0 + R) of the torus `cells_torus` (0/1) after k turns of `rule` (text or masks)."""
    H = cells_torus.shape[0]
    assert 0 <= y0 and y0 + R <= H
    after, _, _ = RR.run(cells_torus, rule, k)
    return after[y0:y0 + R]


@functools.lru_cache(maxsize=None)
def torus(seed: int, H: int, Wd: int) -> np.ndarray:
    t = RR.random_board(seed, H, 32 * Wd, DENSITY)
    t.setflags(write=False)
    return t


@functools.lru_cache(maxsize=None)
def stepped(seed: int, H: int, Wd: int, rule: str, k: int) -> np.ndarray:
    """The whole torus (seed, H, Wd) after k turns: one reference per (torus, rule, k), shared."""
    t = expected(torus(seed, H, Wd), 0, H, k, rule)
    t.setflags(write=False)
    return t


# ------------------------------------------------------------------ the kernel table
FAMILIES = ("bits", "band", "rule_std", "rule_band", "bytes")  # GOL_FAMILY_* 0..4 (include/golhip.h)


def _table():
    """(family, k, words per lane) -> flags, as GOL_STEP_KERNELS of csrc/gol_step_launch.h states it:
    "pipelined" (a split pipeline), "engine_only" (the engine launches it, gol_dev_band_step refuses it)."""
    t = {("bits", k, dw): () for dw in (1, 2, 4) for k in (1, 2, 4, 8, 16) if not (k == 16 and dw == 4)}
    t.update({("band", k, 2): () for k in (1, 2, 4, 8, 16)})
    t.update({("band", k, 4): () for k in (1, 2, 4, 8)})
    t[("band", 12, 2)] = ("engine_only",)
    t[("band", 12, 4)] = ("pipelined",)
    t.update({(kind, k, RULE_DW): () for kind in ("rule_std", "rule_band") for k in (1, 2, 4, 8)})
    t.update({("bytes", k, 1): () for k in (1, 2, 4, 8, 16)})
    t[("bytes", 32, 1)] = ("pipelined",)
    return t


TABLE = _table()
# The instantiations of bits_step_kernel and band_step_kernel: the table's one-wave kernels of the
# bit families.  PUBLIC: those a gol_dev_* entry launches (the case table below); ENGINE_ONLY: the
# rest, reached through the engine alone (tests/test_gpu_engine.py).
INSTANTIATIONS = tuple(i for i, f in TABLE.items() if i[0] != "bytes" and "pipelined" not in f)
ENGINE_ONLY = tuple(i for i in INSTANTIATIONS if "engine_only" in TABLE[i])
PUBLIC = tuple(i for i in INSTANTIATIONS if i not in ENGINE_ONLY)


def words_per_lane(family: str, cells_per_lane: int) -> int:
    """The words per lane a gol_dev_* entry makes of its cells_per_lane (include/golhip.h); 0: none."""
    if family == "bits":
        return cells_per_lane // 32 if cells_per_lane > 0 else 2
    if family == "band":
        return {64: 2, 128: 4}.get(cells_per_lane, 4 if cells_per_lane <= 0 else 0)
    if family == "bytes":
        return 1
    return RULE_DW if cells_per_lane <= 0 or cells_per_lane == 32 * RULE_DW else 0


def inst_id(inst) -> str:
    kind, k, dw = inst
    return f"{kind}-k{k}-dw{dw}"


def is_band(kind: str) -> bool:
    return kind in ("band", "rule_band")


def useful_words(inst) -> int:
    """Output words of one wave: 62 lanes (standard), 64 less ceil(k / dw) halo lanes a side (band)."""
    kind, k, dw = inst
    return (64 - 2 * -(-k // dw)) * dw if is_band(kind) else 62 * dw  # (bytes: dw = 1, 62 words of 32 cells)


def widths(inst) -> dict:
    U, dw = useful_words(inst), inst[2]
    return dict(zip(WIDTH_CLASSES, (dw, U - dw, U, U + dw)))


# ------------------------------------------------------------------ a case
@dataclass(frozen=True)
class Case:
    inst: tuple     # (kind, k, dw)
    wclass: str
    Wd: int
    pitch: int
    form: str       # wrap / contig / separate
    H: int          # rows of the torus the shard is cut from
    y0: int         # torus row of the shard's row 0
    R: int
    row0: int
    rows: int
    strip: int      # strip_rows as passed (0: automatic)
    rule: str
    tag: str        # what the case is in the table for: "R==k", "sub" or "sweep"

    @property
    def kind(self):
        return self.inst[0]

    @property
    def k(self):
        return self.inst[1]

    @property
    def dw(self):
        return self.inst[2]

    @property
    def band(self):
        return is_band(self.kind)

    @property
    def seed(self):
        return 1000003 * self.H + 101 * self.Wd + 7

    @property
    def id(self):
        return (f"{inst_id(self.inst)}:{self.wclass}:Wd{self.Wd}:{self.form}:R{self.R}:"
                f"rows{self.row0}+{self.rows}:strip{self.strip}:{self.rule}")

    # -- the memory picture: allocations (rows of `pitch` words, GUARD rows included) and the word
    #    offsets of the four pointers into them
    def allocs(self) -> dict:
        k, R, g = self.k, self.R, 2 * GUARD
        if self.form == "wrap":
            a = {"src": R + g}
        elif self.form == "contig":
            a = {"src": k + R + k + g}
        else:
            a = {"top": k + g, "mid": R + g, "bot": k + g}
        a["dst"] = R + g
        return a

    def pointers(self) -> dict:
        """name -> (allocation, offset in words)."""
        k, R, p, g = self.k, self.R, self.pitch, GUARD
        if self.form == "wrap":
            ptr = {"top": ("src", (g + R - k) * p), "mid": ("src", g * p), "bot": ("src", g * p)}
        elif self.form == "contig":
            ptr = {"top": ("src", g * p), "mid": ("src", (g + k) * p), "bot": ("src", (g + k + R) * p)}
        else:
            ptr = {n: (n, g * p) for n in ("top", "mid", "bot")}
        ptr["dst"] = ("dst", g * p)
        return ptr

    def contiguous(self, bases: dict) -> bool:
        """The launch geometry's predicate (gol_step_geometry_of) on word addresses: bases = allocation -> word address."""
        a = {n: bases[al] + off for n, (al, off) in self.pointers().items()}
        return a["top"] + self.k * self.pitch == a["mid"] and a["bot"] == a["mid"] + self.R * self.pitch

    def torus_rows(self) -> dict:
        """allocation -> the torus rows its data rows hold (wrapped), input allocations only."""
        k, R, H, y0 = self.k, self.R, self.H, self.y0
        top = [(y0 - k + i) % H for i in range(k)]
        mid = [(y0 + i) % H for i in range(R)]
        bot = [(y0 + R + i) % H for i in range(k)]
        if self.form == "wrap":
            return {"src": mid}
        if self.form == "contig":
            return {"src": top + mid + bot}
        return {"top": top, "mid": mid, "bot": bot}

    def buffers(self) -> dict:
        """allocation -> its uint32 words before the launch: board data in the kernel's layout,
        the sentinel everywhere else."""
        pack = band_pack if self.band else std_pack
        t = pack(torus(self.seed, self.H, self.Wd))
        out = {}
        for name, n in self.allocs().items():
            out[name] = np.full((n, self.pitch), SENT, dtype=np.uint32)
        for name, ys in self.torus_rows().items():
            out[name][GUARD:GUARD + len(ys), :self.Wd] = t[ys]
        return out

    def want_words(self) -> np.ndarray:
        """Rows [row0, row0 + rows) after k turns, in the kernel's layout."""
        after = stepped(self.seed, self.H, self.Wd, self.rule, self.k)
        ys = [(self.y0 + self.row0 + i) % self.H for i in range(self.rows)]
        return (band_pack if self.band else std_pack)(after[ys])

    def strips(self) -> list:
        """Lengths of the launch's strips, [] under the automatic strip length."""
        if self.strip <= 0:
            return []
        full, tail = divmod(self.rows, self.strip)
        return [self.strip] * full + ([tail] if tail else [])


def _pitch(Wd: int) -> int:
    """Wd plus a pad of 5..8 words: a multiple of 4 words, so every row start stays 16-byte
    aligned and pitch % dw == 0 for 1, 2 and 4 words per lane."""
    return (Wd // 4 + 2) * 4


def _rules(inst):
    return RULES if inst[0].startswith("rule") else (CONWAY,)


def _cut(k: int):
    """Torus height and shard position of the contig / separate forms: one torus per width for
    every R <= R_SUB, H >= R + 2k + 3, so that no ghost row is a wrap row of the shard."""
    return R_SUB + 2 * k + 3, k + 1


def _cases_of(index: int, inst):
    kind, k, dw = inst
    W = widths(inst)
    Hc, yc = _cut(k)
    out = []

    def add(wclass, form, R, row0, rows, strip, tag):
        H, y0 = (R, 0) if form == "wrap" else (Hc, yc)
        for rule in _rules(inst):
            out.append(Case(inst, wclass, W[wclass], _pitch(W[wclass]), form, H, y0, R, row0, rows, strip, rule, tag))

    for wi, wclass in enumerate(WIDTH_CLASSES):
        for fi, form in enumerate(FORMS):
            # R == k, the smallest shard the entries take: the whole shard, one strip and strips of one row
            add(wclass, form, k, 0, k, (0, k, 1)[fi], "R==k")
            # R >= 19, a sub-range
            R = R_SUB if form == "wrap" else 19 + wi
            row0 = 1 + wi
            add(wclass, form, R, row0, R - row0 - 2, (0, 3 + wi, 6 - wi)[fi], "sub")
    # strips of 1..6 rows, each as a full strip and (strips of s rows ending in a tail of s - 1) as a
    # tail: the residues of the three-row block loop and of the band kernels' two-block ring.
    # strip_rows = 7 is there for its 6-row tail.  One width class per instantiation, all four
    # across the table.
    wclass = WIDTH_CLASSES[index % 4]
    for s in (0, 1, 2, 3, 4, 5, 6, 7):
        rows = 19 if s == 0 else (2 if s == 1 else 3 * s - 1)
        add(wclass, FORMS[s % 3], R_SUB, 2, rows, s, "sweep")
    return out


CASES = tuple(c for i, inst in enumerate(PUBLIC) for c in _cases_of(i, inst))


def cases_of(inst):
    return [c for c in CASES if c.inst == inst]


# ------------------------------------------------------------------ include/golhip.h, "device launchers"
def check_args(c: Case) -> None:
    """The argument rules of the three step entries as the header states them."""
    assert c.R > 0 and c.Wd > 0 and c.pitch >= c.Wd
    assert c.row0 >= 0 and c.rows >= 0 and c.row0 + c.rows <= c.R
    assert c.k <= c.R
    assert c.Wd % c.dw == 0 and c.pitch % c.dw == 0  # multiples of the words per lane
    assert (c.pitch * 4) % 16 == 0                   # with 16-byte aligned allocations: aligned rows
    for _, off in c.pointers().values():
        assert (off * 4) % 16 == 0
    if c.kind == "bits":
        assert c.dw in (1, 2, 4) and (c.k in (1, 2, 4, 8) or (c.k == 16 and c.dw <= 2))
    elif c.kind == "band":
        assert c.dw in (2, 4) and (c.k in (1, 2, 4, 8) or (c.k == 16 and c.dw == 2))
    else:
        assert c.dw == RULE_DW and c.k in (1, 2, 4, 8)
        assert all(0 <= m < 512 for m in RR.masks(c.rule))
    assert c.strip >= 0


# ------------------------------------------------------------------ refusals
P = 0x10000  # a pointer's value, aligned; a refused call reads nothing through it
_GPU = dict(top=P, mid=P, bot=P, dst=P, R=20, Wd=8, pitch=16, row0=0, rows=20, k=4)
GOOD = {  # name -> (family, a good call in the C entry's arguments; Wd, pitch: W, stride for bytes)
    "bits": ("bits", dict(_GPU, cells_per_lane=128)),
    "band": ("band", dict(_GPU, cells_per_lane=128)),
    "rule_std": ("rule_std", dict(_GPU, cells_per_lane=64, layout=1, birth=0x008, survive=0x00C)),
    "rule_band": ("rule_band", dict(_GPU, cells_per_lane=64, layout=2, birth=0x008, survive=0x00C)),
    "twin_band": ("band", dict(top=P, mid=P, bot=P, dst=P, R=24, Wd=128, pitch=128, row0=0, rows=24, k=12, cells_per_lane=128)),
    "twin_bytes": ("bytes", dict(top=P, mid=P, bot=P, dst=P, R=32, Wd=64, pitch=64, row0=0, rows=32, k=32)),
}
# The clause classes of the launch check (gol_step_launch_ok) and the families that have them.
CLAUSES = {c: FAMILIES for c in ("null", "kernel", "k>R", "board", "unit", "rows", "pretend")}
CLAUSES["align"] = ("band", "rule_std", "rule_band", "bytes")  # (the bits entry has no alignment clause)
CLAUSES["mask"] = ("rule_std", "rule_band")


def refusals():
    """[(good, change, clause, via)]: GOOD[good] with `change` applied is refused under `clause`.  via: "entry" the
    plain gol_dev_* entry can be given it, "on" the _on entries (cus, slots) alone, "check" only gol_step_check_host."""
    R = _GPU["R"]
    out = []
    for g in ("bits", "band"):  # the shape tests/test_gpu_step_kernels.py launches: 4 words per lane, k = 4
        out += [(g, c, "unit", "entry") for c in (dict(Wd=6), dict(Wd=2), dict(pitch=18), dict(cells_per_lane=64, Wd=6, pitch=7))]
        out += [(g, c, "k>R", "entry") for c in (dict(k=8, R=7, rows=7), dict(k=4, R=3, rows=3))]
        out += [(g, dict(k=16), "kernel", "entry")]  # no k = 16 at 128 cells per lane
        out += [(g, c, "rows", "entry") for c in (dict(row0=1), dict(row0=R, rows=1), dict(row0=5, rows=R - 4))]
        out += [(g, dict(top=0), "null", "entry"), (g, dict(pitch=4), "board", "entry"), (g, dict(Wd=0), "board", "entry")]
    out += [("bits", dict(cells_per_lane=96), "kernel", "entry"), ("bits", dict(k=12), "kernel", "entry")]
    for g in ("rule_std", "rule_band"):
        out += [(g, dict(birth=512), "mask", "entry"), (g, dict(survive=512), "mask", "entry")]
        out += [(g, dict(layout=7), "kernel", "entry"), (g, dict(cells_per_lane=128), "kernel", "entry"), (g, dict(k=16), "kernel", "entry")]
        out += [(g, dict(Wd=7), "unit", "entry"), (g, dict(pitch=17), "unit", "entry"), (g, dict(k=8, R=7, rows=7), "k>R", "entry")]
        out += [(g, dict(row0=1), "rows", "entry"), (g, dict(dst=0), "null", "entry"), (g, dict(pitch=4), "board", "entry")]
        out += [(g, dict(mid=P + 4), "align", "entry")]
    b = "twin_band"
    out += [(b, dict(**{n: 0}), "null", "entry") for n in ("top", "mid", "bot", "dst")]
    out += [(b, dict(row0=1), "rows", "entry"), (b, dict(rows=25), "rows", "entry")]
    out += [(b, dict(k=3), "kernel", "entry"), (b, dict(k=16), "kernel", "entry"), (b, dict(k=12, cells_per_lane=64), "kernel", "entry")]
    out += [(b, dict(k=12, R=8, rows=8), "k>R", "entry")]
    out += [(b, dict(cells_per_lane=c), "kernel", "entry") for c in (32, 96, 256)]
    out += [(b, dict(mid=P + 4), "align", "entry"), (b, dict(top=P + 8), "align", "entry"), (b, dict(dst=P + 2), "align", "entry")]
    out += [(b, dict(pitch=124), "board", "entry"), (b, dict(Wd=130, pitch=130), "unit", "entry")]
    b = "twin_bytes"
    out += [(b, dict(**{n: 0}), "null", "entry") for n in ("top", "mid", "bot", "dst")]
    out += [(b, dict(row0=1), "rows", "entry"), (b, dict(rows=33), "rows", "entry")]
    out += [(b, dict(k=3), "kernel", "entry"), (b, dict(k=12), "kernel", "entry"), (b, dict(k=64), "kernel", "entry")]
    out += [(b, dict(k=32, R=16, rows=16), "k>R", "entry")]
    out += [(b, dict(mid=P + 4), "align", "entry"), (b, dict(bot=P + 8), "align", "entry"), (b, dict(dst=P + 1), "align", "entry")]
    out += [(b, dict(pitch=48), "board", "entry"), (b, dict(pitch=72), "unit", "entry"), (b, dict(Wd=48), "unit", "entry")]
    # a pretended device: one of the two left 0, CUs not in eights, a negative count, a k that is not pipelined
    for b, k in (("twin_band", 8), ("twin_bytes", 16)):
        out += [(b, dict(cus=c, slots=n), "pretend", "on") for c, n in ((8, 0), (0, 8), (12, 12), (-8, 8))]
        out += [(b, dict(k=k, cus=8, slots=8), "pretend", "on")]
    out += [(g, dict(cus=8, slots=8), "pretend", "check") for g in ("bits", "rule_std", "rule_band")]
    return out


def twin_refusals():
    """The refusals of the twin entries (tests/test_abi_cpu.py): [(family, change)]."""
    return [(GOOD[g][0], c) for g, c, _, via in refusals() if g.startswith("twin_") and via == "entry"]


def refusal_args(good: str, change: dict) -> dict:
    """The call: family, the arguments of gol_step_check_host by name (words_per_lane resolved), and the entry's own."""
    family, a = GOOD[good]
    a = dict(dict(cells_per_lane=0, birth=0, survive=0, cus=0, slots=0), **a)
    a.update(change)
    if "layout" in a and a["layout"] not in (1, 2):
        family = None  # a layout that is neither: no family
    return dict(a, family=family, words_per_lane=words_per_lane(family or "rule_std", a["cells_per_lane"]))


def check_refusal_coverage(entries=None):
    """Every (family, clause class) pair the check has is hit at least once."""
    hit = {(GOOD[g][0], clause) for g, _, clause, _ in (entries or refusals())}
    want = {(f, c) for c, fams in CLAUSES.items() for f in fams}
    assert hit == want, (sorted(want - hit), sorted(hit - want))
