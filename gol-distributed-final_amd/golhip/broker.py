"""The broker's RPC service `Operations` (broker.go:62-277) over the C ABI.

``Operations`` keeps the reference's method names and argument meaning; the
work is done by the C++ service object in libgolhip.so (gol_host.cpp), which
keeps the board resident on the GPU instead of scattering it to workers every
turn.  Errors come back as ``GolError`` instead of a panic.
"""
from __future__ import annotations

import ctypes

import numpy as np

from ._lib import (GOL_COPY_CUT, GOL_EINVAL, LAYOUTS, PASTE_OPS, TRANSPORTS, VIEW_LAYOUTS, GolError, check, gol_config, gol_request,
                   gol_response, lib, pack_pattern, parse_rle, unpack_pattern)
from .stubs import CellList, Request, Response


def _request(req: Request, keep: list) -> gol_request:
    r = gol_request()
    if req.World is not None:
        world = np.ascontiguousarray(req.World, dtype=np.uint8)
        if world.ndim != 2 or world.shape != (req.ImageHeight, req.ImageWidth):
            # the reference indexes World[y][x] for y < ImageHeight, x < ImageWidth and would
            # panic on a smaller board (broker.go:67-70, 96-105)
            raise ValueError(f"World has shape {world.shape}, expected (ImageHeight, ImageWidth) = "
                             f"{(req.ImageHeight, req.ImageWidth)}")
        keep.append(world)
        r.World = world.ctypes.data
        r.world_stride = world.shape[1]
    r.Turns, r.ImageHeight, r.ImageWidth = req.Turns, req.ImageHeight, req.ImageWidth
    r.Threads, r.EndY, r.StartY, r.Worker = req.Threads, req.EndY, req.StartY, req.Worker
    return r


def _cells(xy: np.ndarray, n: int) -> CellList:
    return CellList(xy[:n].copy())  # the copy lets the H*W-pair buffer go


class Operations:
    """broker.go:60 `type Operations struct{}` with its five RPC methods."""

    def __init__(self, *, device: int = -1, turns_per_launch: int = 0, cells_per_lane: int = 0, shards: int = 1,
                 transport: str = "auto", same_device: bool = False, layout: str = "auto"):
        """shards > 1: the board of a Run is row-sharded over that many GPUs (the reference's
        Threads split, broker.go:135-206, applied to GPUs), with the same results.  layout="bytes":
        the board stays one byte per cell on one GPU (GOL_LAYOUT_BYTES, the byte pipeline)."""
        cfg = gol_config(device=device, turns_per_launch=turns_per_launch, cells_per_lane=cells_per_lane,
                         shards=shards, transport=TRANSPORTS[transport], flags=1 if same_device else 0,
                         layout=LAYOUTS[layout])
        h = ctypes.c_void_p()
        check(lib().gol_broker_create(ctypes.byref(cfg), ctypes.byref(h)))
        self._h = h

    def close(self):
        if getattr(self, "_h", None) and self._h.value:
            lib().gol_broker_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _call(self, fn, req: Request, alive: bool, world: bool) -> Response:
        keep: list = []
        r = _request(req, keep)
        H, W = req.ImageHeight, req.ImageWidth
        res = gol_response()
        out_world = np.zeros((H, W), dtype=np.uint8) if world else None
        cap = H * W if alive else 0
        xy = np.zeros((max(cap, 1), 2), dtype=np.int32)
        if out_world is not None:
            res.World = out_world.ctypes.data
            res.world_stride = W
        if alive:
            res.Alive = xy.ctypes.data
            res.alive_cap = cap
        check(fn(self._h, ctypes.byref(r), ctypes.byref(res)))
        return Response(Alive=_cells(xy, res.alive_len) if alive else [], AliveCount=res.AliveCount,
                        TurnsCompleted=res.TurnsCompleted, World=out_world)

    def Run(self, req: Request) -> Response:  # broker.go:62-234
        return self._call(lib().gol_broker_run, req, alive=True, world=True)

    def RetrieveCurrentData(self, req: Request, *, alive: bool = True, world: bool = True) -> Response:
        """broker.go:256-277.  ``alive=False`` / ``world=False`` skip the list / board copy
        (the count is always returned)."""
        return self._call(lib().gol_broker_retrieve, req, alive=alive, world=world)

    def view(self, x0: int, y0: int, scale: int, out_w: int, out_h: int, *, return_layout: bool = False):
        """A viewport frame of the broker's board (gol_broker_view; no reference counterpart): the
        (out_h, out_w) uint8 pixels of Engine.view and the turns completed when it was taken, served
        between the chunks of a running Run.  It shows the board as it is: at turn 0 the loaded
        board, not RetrieveCurrentData's all-zero one.  return_layout=True appends "bytes",
        "standard" or "band"."""
        if out_w < 1 or out_h < 1 or out_w * out_h > 1 << 26:
            raise GolError(GOL_EINVAL, f"bad view size {out_w} x {out_h} pixels (at most 2^26)")
        out = np.empty((out_h, out_w), dtype=np.uint8)
        turns, lay = ctypes.c_int64(), ctypes.c_int32()
        check(lib().gol_broker_view(self._h, x0, y0, scale, out_w, out_h, out.ctypes.data, out_w, ctypes.byref(turns),
                                    ctypes.byref(lay)))
        return (out, turns.value, VIEW_LAYOUTS[lay.value]) if return_layout else (out, turns.value)

    def paste(self, pattern, x0: int, y0: int, op: str = "copy"):
        """Engine.paste on the broker's board (gol_broker_paste; no reference counterpart), served
        between the chunks of a running Run: `pattern` is a 2-D array, RLE text, or a (w, h) pair
        for a rectangle of alive cells (Engine.fill).  Returns (cells changed, the turn the edit
        landed after)."""
        if op not in PASTE_OPS:
            raise GolError(GOL_EINVAL, f"paste op {op!r}: one of {sorted(PASTE_OPS)}")
        if isinstance(pattern, tuple):
            (w, h), words, stride = pattern, None, 0
        else:
            cells = parse_rle(pattern)[0] if isinstance(pattern, (str, bytes)) else pattern
            words = pack_pattern(cells)
            (h, w), stride = np.shape(cells), words.shape[1]
        n, turns = ctypes.c_int64(), ctypes.c_int64()
        check(lib().gol_broker_paste(self._h, x0, y0, w, h, None if words is None else words.ctypes.data, stride,
                                     PASTE_OPS[op], ctypes.byref(n), ctypes.byref(turns)))
        return n.value, turns.value

    def copy(self, x0: int, y0: int, w: int, h: int, *, cut: bool = False):
        """Engine.copy on the broker's board (gol_broker_copy; no reference counterpart), served
        between the chunks of a running Run: ((h, w) bool cells, the turn they were read after).
        cut=True clears the rectangle after reading it."""
        if w < 1 or h < 1 or w * h > 1 << 26:
            raise GolError(GOL_EINVAL, f"bad copy size {w} x {h} cells (at most 2^26)")
        out = np.empty((h, (w + 63) // 64), dtype=np.uint64)
        turns = ctypes.c_int64()
        check(lib().gol_broker_copy(self._h, x0, y0, w, h, out.ctypes.data, out.shape[1], GOL_COPY_CUT if cut else 0, None,
                                    ctypes.byref(turns)))
        return unpack_pattern(out, w), turns.value

    def cut(self, x0: int, y0: int, w: int, h: int):
        """copy with cut=True."""
        return self.copy(x0, y0, w, h, cut=True)

    def bounds(self, x0: int, y0: int, w: int, h: int):
        """Engine.bounds on the broker's board (gol_broker_bounds): ((bx, by, bw, bh, alive), turn)."""
        v = [ctypes.c_int64() for _ in range(6)]
        check(lib().gol_broker_bounds(self._h, x0, y0, w, h, *(ctypes.byref(x) for x in v)))
        return tuple(x.value for x in v[:5]), v[5].value

    def Pause(self, req: Request | None = None) -> Response:  # broker.go:251-254
        check(lib().gol_broker_pause(self._h))
        return Response()

    def Quit(self, req: Request | None = None) -> Response:  # broker.go:236-239
        check(lib().gol_broker_quit(self._h))
        return Response()

    def SuperQuit(self, req: Request | None = None) -> Response:  # broker.go:241-249
        check(lib().gol_broker_superquit(self._h))
        return Response()

    @property
    def paused(self) -> bool:
        p = ctypes.c_int32()
        check(lib().gol_broker_paused(self._h, ctypes.byref(p)))
        return bool(p.value)
