"""Viewport frames, the part that needs no GPU: gol_view_plan (which rows of a viewport a shard
holds) against a brute-force enumeration of (y0 + v) mod H, and the new entry points in the
header, the library and the ctypes table."""
import ctypes
import os
import re

import pytest

from oracle import oracle as O
from testlib import cpu_lib as G  # noqa: F401 (the fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "golhip.h")
NEW = ["gol_engine_view", "gol_engine_view_counts", "gol_view_plan", "gol_broker_view"]


def brute(H, nranks, rank, y0, vrows):
    """Runs of consecutive viewport rows v whose global row (y0 + v) mod H lies in the shard, with
    consecutive shard-local rows: [(row, rows, vrow)] in viewport order."""
    a, b = O.partition(H, nranks, rank)
    runs = []
    for v in range(vrows):
        y = (y0 + v) % H
        if not a <= y < b:
            continue
        if runs and runs[-1][2] + runs[-1][1] == v and runs[-1][0] + runs[-1][1] == y - a:
            runs[-1][1] += 1
        else:
            runs.append([y - a, 1, v])
    return [tuple(r) for r in runs]


def test_view_plan_matches_brute_force(G):
    """Every H in 1..24, nranks in 1..min(H, 5), rank, y0 and vrows in 1..H: the plan is the
    brute-force run list, at most 2 runs per rank, and the ranks' runs tile [0, vrows) once."""
    L = G.lib()
    runs = (G._lib.gol_view_run * 2)()
    n = ctypes.c_int32()
    for H in range(1, 25):
        for nranks in range(1, min(H, 5) + 1):
            want = {}
            for y0 in range(H):
                for vrows in range(1, H + 1):
                    seen = [0] * vrows
                    for rank in range(nranks):
                        assert L.gol_view_plan(H, nranks, rank, y0, vrows, runs, 2, ctypes.byref(n)) == 0
                        assert 0 <= n.value <= 2
                        got = [(r.row, r.rows, r.vrow) for r in runs[:n.value]]
                        key = (rank, y0, vrows)
                        want[key] = brute(H, nranks, rank, y0, vrows)
                        assert got == want[key], (H, nranks) + key
                        a, b = O.partition(H, nranks, rank)
                        for row, rows, vrow in got:
                            assert rows >= 1 and 0 <= row and row + rows <= b - a
                            for i in range(rows):
                                assert (y0 + vrow + i) % H == a + row + i
                                seen[vrow + i] += 1
                    assert seen == [1] * vrows, (H, nranks, y0, vrows)
    assert G.view_plan(10, 3, 0, 8, 5) == [(0, 3, 2)]  # rows 8, 9 | 0, 1, 2: rank 0 holds rows 0..3
    assert G.view_plan(10, 1, 0, 8, 5) == [(8, 2, 0), (0, 3, 2)]


def test_view_plan_count_without_buffer(G):
    """cap = 0 with runs = NULL reports the number of runs only."""
    n = ctypes.c_int32(-1)
    assert G.lib().gol_view_plan(10, 1, 0, 8, 5, None, 0, ctypes.byref(n)) == 0 and n.value == 2
    runs = (G._lib.gol_view_run * 2)()
    runs[1].rows = -7
    assert G.lib().gol_view_plan(10, 1, 0, 8, 5, runs, 1, ctypes.byref(n)) == 0 and n.value == 2
    assert (runs[0].row, runs[0].rows, runs[0].vrow) == (8, 2, 0) and runs[1].rows == -7


@pytest.mark.parametrize("args", [
    (10, 0, 0, 0, 1), (10, 2, 2, 0, 1), (10, 2, -1, 0, 1), (3, 4, 0, 0, 1),  # ranks
    (10, 2, 0, -1, 1), (10, 2, 0, 10, 1),  # y0 outside [0, H)
    (10, 2, 0, 0, 0), (10, 2, 0, 0, 11), (10, 2, 0, 0, -3),  # vrows outside [1, H]
    (0, 1, 0, 0, 1),
])
def test_view_plan_bad_arguments(G, args):
    with pytest.raises(G.GolError) as ei:
        G.view_plan(*args)
    assert ei.value.code == G._lib.GOL_EINVAL
    L = G.lib()
    runs = (G._lib.gol_view_run * 2)()
    n = ctypes.c_int32()
    assert L.gol_view_plan(10, 2, 0, 0, 4, runs, 2, None) == G._lib.GOL_EINVAL  # n is NULL
    assert L.gol_view_plan(10, 2, 0, 0, 4, None, 2, ctypes.byref(n)) == G._lib.GOL_EINVAL  # cap without a buffer
    assert L.gol_view_plan(10, 2, 0, 0, 4, runs, -1, ctypes.byref(n)) == G._lib.GOL_EINVAL


def test_view_symbols_declared_exported_and_bound(G):
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    lib = ctypes.CDLL(G._lib.LIB_PATH)
    bound = {n for n, _, _ in G._lib.SIGNATURES}
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, text), name
        assert hasattr(lib, name), name
        assert name in bound, name
    assert re.search(r"typedef struct gol_view_run \{[^}]*row;[^}]*rows;[^}]*vrow;[^}]*\} gol_view_run;", text, re.S)
    assert ctypes.sizeof(G._lib.gol_view_run) == 24
    assert G.lib().gol_abi_version() == 6  # added without a version bump: probed by symbol
    for cls, names in ((G.Engine, ["view", "view_counts"]), (G.Operations, ["view"])):
        for m in names:
            assert callable(getattr(cls, m)), m
    assert G._lib.VIEW_LAYOUTS == {0: "bytes", 1: "standard", 2: "band"}


def test_go_shim_has_view():
    text = open(os.path.join(ROOT, "go", "golhip", "golhip.go")).read()
    assert "C.gol_broker_view(" in text and "func (s *Broker) View(" in text
