"""A Game-of-Life board resident in HBM (ctypes wrapper of gol_engine_*).

Replaces the broker's per-turn board handling (broker.go:62-234): the board is
loaded once into HBM and stepped in k-turn kernel launches; queries (alive
count, alive list, the board bytes, a PGM snapshot) are served from the device.
The board may be row-sharded over several GPUs (broker.go:135-206's partition
applied to GPUs) with a k-row halo exchange per launch: `shards=` in one process
(RCCL between distinct GPUs, device copies between shards sharing a GPU), or
`Engine.rank(...)` with one process per GPU (RCCL; or HIP IPC between the processes of one node,
which may share a GPU).
"""
from __future__ import annotations

import ctypes

import numpy as np

from ._lib import (GOL_COPY_CUT, GOL_EINVAL, GOL_IPC_ID_BYTES, GOL_RCCL_ID_BYTES, GOL_RULE_GENERIC, GOL_SHARDS_SAME_DEVICE,
                   GOL_TIMING_EXCHANGE, GOL_WRITE_FN, LAYOUTS, PASTE_OPS, STEP_MODES, TRANSPORT_NAMES, TRANSPORTS,
                   VIEW_LAYOUTS, GolError, check, format_rle_words, format_rule, gol_config, lib, pack_pattern, parse_rle, parse_rule,
                   unpack_pattern)


def rccl_unique_id(library=None) -> bytes:
    """A fresh RCCL unique id (gol_rccl_unique_id) for Engine.rank; share it with every rank."""
    L = library or lib()
    buf = (ctypes.c_uint8 * GOL_RCCL_ID_BYTES)()
    rc = L.gol_rccl_unique_id(buf, GOL_RCCL_ID_BYTES)
    if rc:
        raise GolError(rc, L.gol_last_error().decode(errors="replace"))
    return bytes(buf)


def ipc_unique_id(library=None) -> bytes:
    """A fresh id for Engine.rank(..., transport="ipc") (gol_ipc_unique_id: host only, no GPU);
    share it with every rank."""
    L = library or lib()
    buf = (ctypes.c_uint8 * GOL_IPC_ID_BYTES)()
    rc = L.gol_ipc_unique_id(buf, GOL_IPC_ID_BYTES)
    if rc:
        raise GolError(rc, L.gol_last_error().decode(errors="replace"))
    return bytes(buf)


def unique_id(transport: str = "rccl", library=None) -> bytes:
    """The id Engine.rank needs for `transport` ("rccl" or "ipc")."""
    return ipc_unique_id(library) if transport == "ipc" else rccl_unique_id(library)


class Engine:
    def __init__(self, height: int, width: int, *, turns_per_launch: int = 0, cells_per_lane: int = 0,
                 strip_rows: int = 0, device: int = -1, layout: str = "auto", shards: int = 1,
                 transport: str = "auto", same_device: bool = False, step: str = "auto", rule=None, library=None,
                 _rank=None):
        self.H, self.W = int(height), int(width)
        self._L = library or lib()
        cfg = gol_config(device=device, turns_per_launch=turns_per_launch, strip_rows=strip_rows,
                         cells_per_lane=cells_per_lane, layout=LAYOUTS[layout], shards=shards,
                         transport=TRANSPORTS[transport],
                         flags=(GOL_SHARDS_SAME_DEVICE if same_device else 0) | STEP_MODES[step])
        h = ctypes.c_void_p()
        if _rank is None:
            self._check(self._L.gol_engine_create(self.H, self.W, ctypes.byref(cfg), ctypes.byref(h)))
        else:
            nranks, rank, uid = _rank
            idbuf = None
            if uid is not None:
                # the C side reads exactly GOL_RCCL_ID_BYTES (= GOL_IPC_ID_BYTES) bytes of the id: a
                # shorter buffer would be read past its end
                if len(uid) != GOL_RCCL_ID_BYTES or len(uid) != GOL_IPC_ID_BYTES:
                    raise GolError(GOL_EINVAL, f"rank id must be {GOL_RCCL_ID_BYTES} bytes, got {len(uid)}")
                idbuf = (ctypes.c_uint8 * GOL_RCCL_ID_BYTES).from_buffer_copy(uid)
            self._check(self._L.gol_engine_create_rank(self.H, self.W, nranks, rank, idbuf, ctypes.byref(cfg),
                                                       ctypes.byref(h)))
        self._h = h
        if rule is not None:  # default: B3/S23 on the Conway kernels
            try:
                self.set_rule(rule)
            except BaseException:
                self.close()
                raise

    @classmethod
    def rank(cls, height: int, width: int, nranks: int, rank: int, uid: bytes | None, **kw) -> "Engine":
        """This process's shard `rank` of an `nranks`-rank board (collective: every rank constructs
        it with the same uid).  transport="rccl" (default with nranks > 1: one process per GPU, uid
        from rccl_unique_id) or "ipc" (processes of one node that may share a GPU, uid from
        ipc_unique_id)."""
        return cls(height, width, _rank=(nranks, rank, uid), **kw)

    def _check(self, rc: int) -> None:
        if rc:
            raise GolError(rc, self._L.gol_last_error().decode(errors="replace"))

    # -- lifetime
    def close(self) -> None:
        if getattr(self, "_h", None) and self._h.value:
            self._L.gol_engine_destroy(self._h)
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

    # -- board in / out
    def load_bytes(self, world: np.ndarray) -> None:
        world = np.ascontiguousarray(world, dtype=np.uint8)
        if world.shape != (self.H, self.W):
            raise ValueError(f"board shape {world.shape} != {(self.H, self.W)}")
        self._check(self._L.gol_engine_load_bytes(self._h, world.ctypes.data, self.W))

    def load_random(self, seed: int) -> None:
        self._check(self._L.gol_engine_load_random(self._h, seed))

    def load_pgm(self, path: str) -> None:
        """readPgmImage (gol/io.go:90-126): every shard streams its own rows of the file."""
        self._check(self._L.gol_engine_load_pgm(self._h, path.encode()))

    def store_bytes(self) -> np.ndarray:
        out = np.empty((self.H, self.W), dtype=np.uint8)
        self._check(self._L.gol_engine_store_bytes(self._h, out.ctypes.data, self.W))
        return out

    def store_rows(self, y0: int, y1: int) -> np.ndarray:
        out = np.empty((max(y1 - y0, 0), self.W), dtype=np.uint8)
        self._check(self._L.gol_engine_store_rows(self._h, y0, y1, out.ctypes.data, self.W))
        return out

    def write_pgm(self, path: str) -> None:
        self._check(self._L.gol_engine_write_pgm(self._h, path.encode()))

    def write_pgm_to(self, sink) -> None:
        """The P5 byte stream (gol/io.go:52-81) into sink(offset, memoryview) instead of a file:
        the header, then chunks of rows in row order (this process's rows, at their file
        offsets).  The memoryview is only valid during the call."""
        err = []

        def cb(_user, off, data, n):
            try:
                sink(off, (ctypes.c_uint8 * n).from_address(data))
                return 0
            except BaseException as x:  # noqa: BLE001 -- reported after the call
                err.append(x)
                return 1
        fn = GOL_WRITE_FN(cb)
        rc = self._L.gol_engine_write_pgm_to(self._h, fn, None)
        if err:
            raise err[0]
        self._check(rc)

    def load_words(self, y0: int, words: np.ndarray) -> None:
        """Rows [y0, y0 + len(words)) from bit-packed uint64 rows (64 cells per word, LSB = lowest x)."""
        words = np.ascontiguousarray(words, dtype=np.uint64)
        if words.ndim != 2 or words.shape[1] != self.W // 64:
            raise ValueError(f"expected (rows, {self.W // 64}) uint64 words")
        self._check(self._L.gol_engine_load_words(self._h, y0, y0 + words.shape[0], words.ctypes.data, words.shape[1]))

    def store_words(self, y0: int, y1: int) -> np.ndarray:
        out = np.empty((max(y1 - y0, 0), self.W // 64), dtype=np.uint64)
        self._check(self._L.gol_engine_store_words(self._h, y0, y1, out.ctypes.data, self.W // 64))
        return out

    # -- the rule
    def set_rule(self, rule, generic: bool = False) -> None:
        """The life-like rule of every later turn (gol_engine_set_rule): "B36/S23" or a (birth,
        survive) pair of 9-bit masks.  The board and the turn counter stay.  Rules other than
        B3/S23 run on the rule kernels (bit boards only); generic=True runs B3/S23 on them too.
        With several ranks every rank sets the same rule before the next stepping call."""
        birth, survive = parse_rule(rule, self._L) if isinstance(rule, str) else (int(rule[0]), int(rule[1]))
        if not (0 <= birth < 1 << 32 and 0 <= survive < 1 << 32):
            raise GolError(GOL_EINVAL, f"rule masks out of range ({birth}, {survive})")
        self._check(self._L.gol_engine_set_rule(self._h, birth, survive, GOL_RULE_GENERIC if generic else 0))

    def _rule(self):
        b, s, g = ctypes.c_uint32(), ctypes.c_uint32(), ctypes.c_int32()
        self._check(self._L.gol_engine_rule(self._h, ctypes.byref(b), ctypes.byref(s), ctypes.byref(g)))
        return b.value, s.value, bool(g.value)

    @property
    def rule(self) -> str:
        """The current rule's canonical text, e.g. "B3/S23"."""
        b, s, _ = self._rule()
        return format_rule(b, s, self._L)

    @property
    def rule_generic(self) -> bool:
        """The rule kernels step the board (any rule but plain B3/S23)."""
        return self._rule()[2]

    # -- stepping and queries
    def step(self, turns: int) -> None:
        self._check(self._L.gol_engine_step(self._h, turns))

    def step_counted(self, turns: int, every: int) -> np.ndarray:
        """Advance `turns` turns; the alive count after every `every` turns (fused on the GPU)."""
        n = turns // every if every > 0 else 0
        out = np.zeros(max(n, 1), dtype=np.uint64)
        self._check(self._L.gol_engine_step_counted(self._h, turns, every, out.ctypes.data, n))
        return out[:n]

    @property
    def turn(self) -> int:
        t = ctypes.c_int64()
        self._check(self._L.gol_engine_turn(self._h, ctypes.byref(t)))
        return t.value

    def alive_count(self) -> int:
        c = ctypes.c_uint64()
        self._check(self._L.gol_engine_alive_count(self._h, ctypes.byref(c)))
        return c.value

    def alive_cells(self, cap: int | None = None) -> np.ndarray:
        """(n, 2) int32 array of (x, y) in row-major order (broker.go:47-58)."""
        if cap is None:
            cap = self.alive_count()
        xy = np.zeros((max(cap, 1), 2), dtype=np.int32)
        n = ctypes.c_int64()
        self._check(self._L.gol_engine_alive_cells(self._h, xy.ctypes.data, cap, ctypes.byref(n)))
        return xy[:min(n.value, cap)]

    def step_flips(self, cap: int | None = None) -> np.ndarray:
        """Advance one turn; (n, 2) int32 (x, y) of the cells that changed, row-major: the
        CellFlipped events of that turn (gol/event.go:50-60)."""
        if cap is None:
            cap = self.H * self.W
        xy = np.zeros((max(cap, 1), 2), dtype=np.int32)
        n = ctypes.c_int64()
        self._check(self._L.gol_engine_step_flips(self._h, xy.ctypes.data, cap, ctypes.byref(n)))
        return xy[:min(n.value, cap)]

    def _view(self, fn, dtype, x0, y0, scale, out_w, out_h, return_layout):
        if out_w < 1 or out_h < 1 or out_w * out_h > 1 << 26:  # (before the frame is allocated here)
            raise GolError(GOL_EINVAL, f"bad view size {out_w} x {out_h} pixels (at most 2^26)")
        out = np.empty((out_h, out_w), dtype=dtype)
        lay = ctypes.c_int32()
        self._check(fn(self._h, x0, y0, scale, out_w, out_h, out.ctypes.data, out_w, ctypes.byref(lay)))
        return (out, VIEW_LAYOUTS[lay.value]) if return_layout else out

    def view_counts(self, x0: int, y0: int, scale: int, out_w: int, out_h: int, *, return_layout: bool = False):
        """(out_h, out_w) uint32: the alive cells of every scale x scale box of the torus rectangle
        at (x0, y0) (gol_engine_view_counts), counted on the GPU from the board as it is stepped (no
        layout conversion; the work follows the viewport).  With ranks in several processes: the
        cells of this rank's rows.  return_layout=True also returns what was read: "bytes",
        "standard" or "band"."""
        return self._view(self._L.gol_engine_view_counts, np.uint32, x0, y0, scale, out_w, out_h, return_layout)

    def view(self, x0: int, y0: int, scale: int, out_w: int, out_h: int, *, return_layout: bool = False):
        """(out_h, out_w) uint8 greyscale frame: ceil(255 n / scale^2) per box (gol_engine_view); at
        scale 1 the board's 0/255 bytes.  Needs every row in this process."""
        return self._view(self._L.gol_engine_view, np.uint8, x0, y0, scale, out_w, out_h, return_layout)

    # -- edits of the running board
    def _paste(self, x0, y0, w, h, words, stride, op, return_layout):
        if op not in PASTE_OPS:
            raise GolError(GOL_EINVAL, f"paste op {op!r}: one of {sorted(PASTE_OPS)}")
        n, lay = ctypes.c_int64(), ctypes.c_int32()
        self._check(self._L.gol_engine_paste(self._h, x0, y0, w, h, None if words is None else words.ctypes.data, stride,
                                             PASTE_OPS[op], ctypes.byref(n), ctypes.byref(lay)))
        return (n.value, VIEW_LAYOUTS[lay.value]) if return_layout else n.value

    def paste(self, pattern, x0: int, y0: int, op: str = "copy", *, return_layout: bool = False):
        """Write a pattern into the running board in place (gol_engine_paste): a 2-D array (non-zero
        = alive) or RLE text; pattern cell (c, r) lands on ((x0 + c) mod W, (y0 + r) mod H) under op
        "copy" (the whole rectangle is overwritten), "or", "xor" or "andnot".  The board keeps its
        layout and its turn counter; returns the number of cells (of this process's rows) whose
        state changed, with return_layout=True also the layout written: "bytes", "standard" or "band"."""
        cells = parse_rle(pattern, self._L)[0] if isinstance(pattern, (str, bytes)) else pattern
        words = pack_pattern(cells)
        h, w = np.shape(cells)
        return self._paste(x0, y0, w, h, words, words.shape[1], op, return_layout)

    def paste_words(self, words: np.ndarray, w: int, x0: int, y0: int, op: str = "copy", *, return_layout: bool = False):
        """paste of a pattern that is already bit-packed: (h, >= ceil(w / 64)) uint64 rows, bit c % 64
        of word c // 64 = cell c (as load_words packs them; bits at c >= w are ignored)."""
        words = np.ascontiguousarray(words, dtype=np.uint64)
        if words.ndim != 2 or words.shape[0] < 1 or words.shape[1] < (w + 63) // 64:
            raise ValueError(f"expected (rows, >= {(w + 63) // 64}) uint64 words for {w} cells per row")
        return self._paste(x0, y0, w, words.shape[0], words, words.shape[1], op, return_layout)

    def fill(self, x0: int, y0: int, w: int, h: int, op: str = "copy", *, return_layout: bool = False):
        """paste with every pattern cell alive: "copy" / "or" set the w x h rectangle at (x0, y0),
        "andnot" clears it, "xor" inverts it.  Returns the number of cells that changed."""
        return self._paste(x0, y0, w, h, None, 0, op, return_layout)

    # -- reads of a region of the running board
    def copy_words(self, x0: int, y0: int, w: int, h: int, *, cut: bool = False, return_layout: bool = False):
        """The exact cells of the w x h rectangle at (x0, y0) (cell (c, r) = board cell ((x0 + c) mod
        W, (y0 + r) mod H)) as bit-packed rows (gol_engine_copy): ((h, ceil(w / 64)) uint64 words as
        paste_words takes them, alive cells), gathered on the GPU from the board as it is stepped; the
        board, its layout and the turn counter stay.  cut=True clears the rectangle after reading
        it.  With ranks in several processes: this rank's rows, the others zero.  return_layout=True
        appends what was read: "bytes", "standard" or "band"."""
        if w < 1 or h < 1 or w * h > 1 << 26:  # (before the pattern is allocated here)
            raise GolError(GOL_EINVAL, f"bad copy size {w} x {h} cells (at most 2^26)")
        out = np.empty((h, (w + 63) // 64), dtype=np.uint64)
        n, lay = ctypes.c_int64(), ctypes.c_int32()
        self._check(self._L.gol_engine_copy(self._h, x0, y0, w, h, out.ctypes.data, out.shape[1], GOL_COPY_CUT if cut else 0,
                                            ctypes.byref(n), ctypes.byref(lay)))
        return (out, n.value, VIEW_LAYOUTS[lay.value]) if return_layout else (out, n.value)

    def copy(self, x0: int, y0: int, w: int, h: int, *, cut: bool = False, return_layout: bool = False):
        """copy_words as an (h, w) bool array (with return_layout=True: the array and the layout read)."""
        words, _, lay = self.copy_words(x0, y0, w, h, cut=cut, return_layout=True)
        cells = unpack_pattern(words, w)
        return (cells, lay) if return_layout else cells

    def cut(self, x0: int, y0: int, w: int, h: int, *, return_layout: bool = False):
        """copy, then the rectangle is cleared (as fill(..., "andnot"): the next step exchanges its halo again)."""
        return self.copy(x0, y0, w, h, cut=True, return_layout=return_layout)

    def bounds(self, x0: int = 0, y0: int = 0, w: int | None = None, h: int | None = None):
        """(bx, by, bw, bh, alive): the smallest box, in the rectangle's own coordinates, that holds
        every alive cell of the w x h rectangle at (x0, y0) (default: the rest of the board from
        there), and their number (gol_engine_bounds); (0, 0, 0, 0, 0) if there is none.  With ranks in
        several processes: of this rank's rows."""
        w = self.W - x0 if w is None else w
        h = self.H - y0 if h is None else h
        v = [ctypes.c_int64() for _ in range(5)]
        self._check(self._L.gol_engine_bounds(self._h, x0, y0, w, h, *(ctypes.byref(x) for x in v), None))
        return tuple(x.value for x in v)

    def to_rle(self, x0: int = 0, y0: int = 0, w: int | None = None, h: int | None = None, *, trim: bool = True) -> str:
        """The rectangle (default: as bounds) as RLE text under the engine's current rule; trim=True
        cuts it to the bounding box of its alive cells first (none: the 1 x 1 dead pattern).  A box
        above 2^26 cells raises the copy's GolError."""
        w = self.W - x0 if w is None else w
        h = self.H - y0 if h is None else h
        if trim:
            bx, by, bw, bh, _ = self.bounds(x0, y0, w, h)
            x0, y0, w, h = (x0 + bx) % self.W, (y0 + by) % self.H, max(bw, 1), max(bh, 1)
        words, _ = self.copy_words(x0, y0, w, h)
        return format_rle_words(words, w, self.rule, self._L)

    def hash(self) -> int:
        h = ctypes.c_uint64()
        self._check(self._L.gol_engine_hash(self._h, ctypes.byref(h)))
        return h.value

    def info(self) -> dict:
        k, cpl, strip, bm = (ctypes.c_int32() for _ in range(4))
        self._check(self._L.gol_engine_info(self._h, ctypes.byref(k), ctypes.byref(cpl), ctypes.byref(strip),
                                    ctypes.byref(bm)))
        return {"turns_per_launch": k.value, "cells_per_lane": cpl.value, "strip_rows": strip.value,
                "bit_mode": bool(bm.value), "layout": {0: "bytes", 1: "standard", 2: "band"}[bm.value]}

    def topology(self) -> dict:
        s, n, r, t = (ctypes.c_int32() for _ in range(4))
        self._check(self._L.gol_engine_topology(self._h, ctypes.byref(s), ctypes.byref(n), ctypes.byref(r),
                                                ctypes.byref(t)))
        return {"shards": s.value, "nranks": n.value, "rank": r.value, "transport": TRANSPORT_NAMES[t.value]}

    def shard(self, i: int) -> dict:
        d, a, b = ctypes.c_int32(), ctypes.c_int64(), ctypes.c_int64()
        self._check(self._L.gol_engine_shard(self._h, i, ctypes.byref(d), ctypes.byref(a), ctypes.byref(b)))
        return {"device": d.value, "y0": a.value, "y1": b.value}

    def set_timing(self, enable: bool, exchanges: bool = False) -> None:
        """HIP-event timing of the stepping calls; exchanges=True also times every halo exchange
        of them (GOL_TIMING_EXCHANGE: one event pair each, on the stream it runs on)."""
        level = (GOL_TIMING_EXCHANGE if exchanges else 1) if enable else 0
        self._check(self._L.gol_engine_set_timing(self._h, level))

    def exchange_timing(self) -> dict:
        """Halo exchanges timed since set_timing(True, exchanges=True): their mean duration, and
        its split (gol_engine_exchange_split) into the wait for the ring neighbours to reach the
        exchange and the transfer of the halo rows."""
        n, ms, w, x = ctypes.c_int64(), ctypes.c_double(), ctypes.c_double(), ctypes.c_double()
        self._check(self._L.gol_engine_exchange_timing(self._h, ctypes.byref(n), ctypes.byref(ms)))
        self._check(self._L.gol_engine_exchange_split(self._h, ctypes.byref(n), ctypes.byref(w), ctypes.byref(x)))
        return {"exchanges": n.value, "mean_ms": ms.value, "wait_ms": w.value, "transfer_ms": x.value}

    def timing(self) -> dict:
        """HIP-event timing of every shard-step since set_timing(True) (edge launches included)."""
        n, ms, cells = ctypes.c_int64(), ctypes.c_double(), ctypes.c_double()
        self._check(self._L.gol_engine_timing(self._h, ctypes.byref(n), ctypes.byref(ms), ctypes.byref(cells)))
        return {"launches": n.value, "mean_ms": ms.value, "mean_cell_updates": cells.value}

    def device_bits(self):
        p = ctypes.c_void_p()
        pitch = ctypes.c_int64()
        self._check(self._L.gol_engine_device_bits(self._h, ctypes.byref(p), ctypes.byref(pitch)))
        return p.value, pitch.value


def next_state_slab(world: np.ndarray, start_y: int, end_y: int) -> np.ndarray:
    """worker.go:15-42 calculateNextState(startY, endY, world) on the GPU."""
    world = np.ascontiguousarray(world, dtype=np.uint8)
    H, W = world.shape
    out = np.empty((max(end_y - start_y, 0), W), dtype=np.uint8)
    check(lib().gol_next_state_slab(world.ctypes.data, H, W, W, start_y, end_y, out.ctypes.data, W))
    return out


def partition_rows(height: int, parts: int, i: int) -> tuple[int, int]:
    """broker.go:135-139 / 172-206 row split -> (StartY, EndY)."""
    a, b = ctypes.c_int64(), ctypes.c_int64()
    check(lib().gol_partition_rows(height, parts, i, ctypes.byref(a), ctypes.byref(b)))
    return a.value, b.value
