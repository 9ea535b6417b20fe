"""What the region twins must refuse (csrc/gol_edit.h, gol_region_ok): one list for gol_paste_host,
gol_copy_host and gol_bounds_host, which fill a gol_region from their arguments and ask the one
check the kernels' launchers ask.  A row names what it changes in DEFAULT by the descriptor's member
(`at`: prow of the paste and the copy; gol_bounds_host's signature has no such argument, so that one
row cannot be put to it).  Every row differs from a call that succeeds (ACCEPTED) in one clause."""
import numpy as np

DEFAULT = dict(layout=2, base=True, pitch=32, W=1024, x0=0, w=10, row=0, rows=2, at=0)
ACCEPTED = [dict(), dict(layout=1), dict(layout=0, W=128, pitch=128)]
REFUSED = [
    dict(layout=-1), dict(layout=3),                                           # the layout's range
    dict(layout=0, W=128, pitch=127), dict(layout=1, pitch=31), dict(pitch=31),  # a pitch one under the layout's units
    dict(W=1000), dict(layout=1, W=100),                                       # the layout's width rule
    dict(row=-1), dict(rows=-1), dict(at=-1),
    dict(x0=-1), dict(x0=1024), dict(w=0), dict(w=1025),
    dict(base=False),                                                          # NULL
]


def buffers():
    """(a board of 2 rows x 32 words of zeros, a pattern of 2 rows x 2 words of fives)."""
    return np.zeros((2, 32), np.uint32), np.full((2, 2), 5, np.uint64)


def _args(buf, kw):
    a = dict(DEFAULT, **kw)
    a["base"] = buf.ctypes.data if a["base"] else None
    return a


def paste(L, buf, pat, stride=1, op=0, pattern=True, **kw):
    a = _args(buf, kw)
    return L.gol_paste_host(a["layout"], a["base"], a["pitch"], a["W"], a["row"], a["rows"], a["at"], a["x0"], a["w"],
                            pat.ctypes.data if pattern else None, stride, op, None)


def copy(L, buf, pat, stride=1, pattern=True, **kw):
    a = _args(buf, kw)
    return L.gol_copy_host(a["layout"], a["base"], a["pitch"], a["W"], a["row"], a["rows"], a["at"], a["x0"], a["w"],
                           pat.ctypes.data if pattern else None, stride, None)


def bounds(L, buf, pat=None, **kw):
    a = _args(buf, kw)
    assert a["at"] == 0, "gol_bounds_host takes no `at`"
    return L.gol_bounds_host(a["layout"], a["base"], a["pitch"], a["W"], a["row"], a["rows"], a["x0"], a["w"],
                             None, None, None, None, None)
