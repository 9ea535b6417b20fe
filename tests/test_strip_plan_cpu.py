"""The pipeline kernels' strip schedule, as libgolhip.so exports it (gol_strip_plan; no GPU).

band_pipe_kernel (k = 12) and bytes_pipe_kernel (k = 32) take their rows from a StripMap that
the launch code picks from the launch's shape, the device's CU count and the workgroups of
the kernel resident on it (csrc/gol_strips.h).  gol_strip_plan runs that choice and then the
kernels' own work_item / work_dir / pair_extent for every workgroup id, so what is checked
here is the arithmetic the GPU runs: for every plan of a sweep over devices, widths, pitches,
row counts (every BASELINE board, its shares for 1..8 shards and each launch of their step
plans) and the two sides of every mode switch,

* the ranges partition [row0, row0 + rows) of every column group (a pair counts once);
* every workgroup id has a record, and no two ids share a range unless they are a pair;
* pairs have two members with one range, opposite directions, a claim counter of their own
  inside the device's buffer, and are empty together;
* whatever the split of a pair's claims, the two walkers' stores meet exactly;
* every range fits the 32-bit buffer its stores go through, and ranked ranges keep the
  minimum length the split was asked for.

K, RPB and NS come from the library (gol_strip_info).
"""
import numpy as np
import pytest
from testlib import cpu_lib as G  # noqa: F401 (the fixture)

BAND_U = 232  # words per column group of the band pipeline: (64 - 2 * 3 halo lanes) * 4
BYTES_U = 62 * 32  # cells per column group of the byte pipeline
BAND_MODES = {"small", "explicit", "plain", "round_tiled", "tail", "ranked_static", "ranked_paired"}
BYTES_MODES = BAND_MODES - {"small", "tail"}
CUS = (8, 64, 256, 304, 100)  # 100: not a multiple of 8, never ranked
# BASELINE.json's boards: (kernel, H, W)
BOARDS = (("bytes", 16384, 16384), ("band", 65536, 65536), ("band", 262144, 262144), ("band", 1 << 20, 1 << 20))


def _width(kernel, ngroups):
    """A board width (as the launcher takes it) of exactly `ngroups` column groups."""
    return ngroups * (BAND_U if kernel == "band" else BYTES_U)


def _pitch(kernel, width, padded):
    return width + ((8 if kernel == "band" else 48) if padded else 0)


def check_plan(G, kernel, rows, row0, width, pitch, cus, slots, strip_rows=0):
    """Every property of one plan; returns its mode."""
    info, r = G.strip_plan(kernel, rows, row0, width, pitch, cus, slots, strip_rows)
    what = f"{kernel} rows {rows} at {row0}, width {width}, pitch {pitch}, cus {cus}, slots {slots}, strip {strip_rows}: {info}"
    K, RPB, NS, ng, mode = info["K"], info["RPB"], info["NS"], info["ngroups"], info["mode"]
    assert K == (12 if kernel == "band" else 32), what
    unit = BAND_U if kernel == "band" else BYTES_U
    assert ng == -(-width // unit), what
    end = row0 + rows
    s0, s1, grp, d = (r[f].astype(np.int64) for f in ("s0", "s1", "group", "dir"))
    # ---- workgroup ids: one record each, a column group of the board each
    assert len(r) == info["nwg"] >= 1, what
    assert ((grp >= 0) & (grp < ng)).all(), what
    full = s0 < s1
    assert (s0[full] >= row0).all() and (s1[full] <= end).all(), what
    # ---- modes
    ranked = mode in ("ranked_static", "ranked_paired")
    assert mode in (BAND_MODES if kernel == "band" else BYTES_MODES), what
    assert (mode == "explicit") == (strip_rows > 0), what
    if cus % 8:
        assert not ranked, what
    if ranked:
        per_cu = info["per_cu"]
        assert 1 <= per_cu <= min(4 if kernel == "band" else 3, slots // cus) and info["nwg"] == cus * per_cu, what
        assert (mode == "ranked_paired") == bool(d.any()), what
    else:
        assert not d.any(), what
    # ---- pairs
    static = d == 0
    assert (r["claim"][static] == -1).all() and (r["s1e"][static] == r["s1"][static]).all(), what
    pi = np.flatnonzero(~static)
    order = pi[np.argsort(r["claim"][pi], kind="stable")]
    assert len(order) % 2 == 0, what
    a, b = order[0::2], order[1::2]
    if len(order):
        claims = r["claim"][a]
        assert (claims == r["claim"][b]).all() and (np.diff(claims) > 0).all(), what  # two members, no shared counter
        assert claims[0] >= 0 and claims[-1] < 2 * cus, what
        for f in ("group", "s0", "s1", "s1e", "nclaim"):
            assert (r[f][a] == r[f][b]).all(), (f, what)
        assert (d[a] + d[b] == 0).all() and (np.abs(d[a]) == 1).all(), what
        assert (full[a] == full[b]).all(), what  # empty together: an empty member never resets the counter
    # ---- exact cover: static strips and one member of every pair, per column group
    units = np.concatenate([np.flatnonzero(static & full), a[full[a]]]).astype(np.int64)
    o = units[np.lexsort((s0[units], grp[units]))]
    g, u0, u1 = grp[o], s0[o], s1[o]
    first = np.r_[True, g[1:] != g[:-1]]
    last = np.r_[first[1:], True]
    assert np.array_equal(g[first], np.arange(ng)), what  # every group has rows
    assert (u0[first] == row0).all() and (u1[last] == end).all(), what
    assert (u1[:-1][~last[:-1]] == u0[1:][~first[1:]]).all(), what  # no gap, no overlap
    if mode == "tail":
        t0, trow = info["tail_first"], row0 + info["tail_row"]
        ids = np.arange(len(r))
        long_, short = full & (ids < t0), full & (ids >= t0)
        assert 0 < t0 < len(r) and row0 < trow < end, what
        assert (s1[long_] <= trow).all() and (s0[short] >= trow).all(), what
        ends = np.full(ng, -1)
        np.maximum.at(ends, grp[long_], s1[long_])
        assert (ends == trow).all(), what  # the long strips end exactly at tail_row
        assert ((s1 - s0)[short] <= info["tail_strip"]).all(), what
    # ---- the meeting point of every pair, for every split of its claims
    if len(order):
        shapes = np.unique(np.stack([s1[a] - s0[a], r["s1e"][a].astype(np.int64) - s0[a], r["nclaim"][a]], axis=1), axis=0)
        for length, ext, nclaim in shapes:
            if length <= 0:
                continue
            assert nclaim % NS == 0 and length <= ext < length + RPB * NS, what
            na = np.arange(0, nclaim + 1, NS)  # blocks of the down-walker; the up-walker has the rest
            down_end = np.maximum(RPB * na - 2 * K, 0)  # stores [0, down_end) relative to s0
            up_start = ext - np.maximum(RPB * (nclaim - na) - 2 * K, 0)  # stores [up_start, ext)
            lo = np.minimum(down_end, length)
            hi = np.clip(up_start, 0, length)
            assert (lo == hi).all(), (int(length), int(ext), int(nclaim), what)  # together [s0, s1), once
    # ---- limits the kernels rely on
    n_rows = (s1 - s0)[full]
    if kernel == "band":
        bound = (1 << 31) - 1 if ranked else 1 << 30
        assert (n_rows * pitch * 4 <= max(bound, pitch * 4)).all(), what
        if ranked:
            assert info["period"] * pitch * 4 < 1 << 31, what
    else:
        assert (n_rows <= max(1, ((1 << 31) - 1) // pitch - 1)).all(), what
    if ranked:
        unclipped = full & (s1 < end)
        assert ((s1 - s0)[unclipped] >= (8 * K if kernel == "band" else 2 * K)).all(), what
    return mode


def _devices(kernel, cus_list=CUS):
    top = 4 if kernel == "band" else 3  # the byte pipeline takes at most GOL_BYTES_PER_CU per CU
    return [(c, c * p) for c in cus_list for p in range(1, top + 1)]


def generic_cases(kernel):
    """Widths of 1 to a few hundred column groups, rows from 1 to 2^20, both pitches, every device."""
    rows_all = (1, 2, 13, 95, 96, 97, 191, 193, 600, 1000, 4097, 30000, 65537, 131071, 1 << 20)
    out = []
    for i, ng in enumerate((1, 2, 3, 5, 9, 17, 33, 64, 65, 133, 255, 300)):
        w = _width(kernel, ng) - (4 if kernel == "band" else 32) * (i % 2)  # a partly filled last group too
        for j, rows in enumerate(rows_all):
            if rows * ng > 9 << 20:  # (bounds a plan to ~10^4 workgroups)
                continue
            for m, (cus, slots) in enumerate(_devices(kernel)):
                if (i + j + m) % 3 and rows not in (30000, 65537):  # a third of the grid, the ranked sizes whole
                    continue
                out.append((kernel, rows, (0, 7, 1000)[(i + j) % 3], w, _pitch(kernel, w, (j + m) % 2), cus, slots, 0))
    for strip in (1, 7, 96, 1000, 1 << 25):
        for rows, ng in ((1, 1), (999, 2), (5000, 9), (40000, 1)):
            w = _width(kernel, ng)
            out.append((kernel, rows, 11, w, _pitch(kernel, w, strip % 2), 256, 768, strip))
    return out


def threshold_cases(kernel):
    """One below and one at (or one past) every mode switch, with the mode each side must give."""
    k = 12 if kernel == "band" else 32
    per = 4 if kernel == "band" else 3
    out = []

    def add(rows, ng, cus, slots, want):
        w = _width(kernel, ng)
        out.append(((kernel, rows, 0, w, w, cus, slots, 0), want))
    if kernel == "band":
        # `small`: rows * ngroups < 8 * k * 256
        add(8 * k * 256 - 1, 1, 256, 1024, {"small"})
        add(8 * k * 256, 1, 256, 1024, {"round_tiled"})  # (96 rows per CU: too few for two pairs)
        add(8 * k * 256 // 4 - 1, 4, 100, 400, {"small"})
        add(8 * k * 256 // 4, 4, 100, 400, {"round_tiled"})
    # the 0.94 fill rule: (cus // ngroups) * ngroups * 100 >= cus * 94
    add(4096, 120, 256, 256 * per, {"round_tiled"})  # 240 of 256 CUs
    add(4096, 121, 256, 256 * per, {"ranked_paired"})  # 242
    add(4096, 20, 64, 64, {"round_tiled"})  # 60 of 64
    add(4096, 21, 64, 64, {"ranked_static"})  # 63
    # max_rounds: ngroups * ceil(rows / 1024) <= max_rounds * cus * per_cu (band 16, bytes 2)
    mr = 16 if kernel == "band" else 2
    add(mr * 8 * per * 1024, 1, 8, 8 * per, {"ranked_paired"})
    add(mr * 8 * per * 1024 + 1, 1, 8, 8 * per, {"tail"} if kernel == "band" else {"round_tiled"})
    # the 4-round limit of round_tiled_strip, on a device that never ranks
    add(4 * 100 * 1024, 1, 100, 100, {"round_tiled"})
    add(4 * 100 * 1024 + 1, 1, 100, 100, {"tail"} if kernel == "band" else {"plain"})
    if kernel == "band":
        # nwg > 4 * slots: 133 groups on 1024 slots, strips of 1024 rows
        add(30 * 1024, 133, 256, 1024, {"plain"})  # 3990 workgroups
        add(30 * 1024 + 1, 133, 256, 1024, {"tail"})  # 4123
    # the minimum rows of a rank: band pairs 8 * KW * P each, the byte split 2k per rank
    if kernel == "band":
        add(256 * 2 * 96, 1, 256, 1024, {"ranked_paired"})
        add(256 * (2 * 96 - 1), 1, 256, 1024, {"round_tiled"})
    return out


def baseline_cases(G):
    """Every BASELINE board, its shares for 1..8 shards (gol_partition_rows) and each launch of their
    step plans (serial, edge-first, overlap; row0 > 0), on the two full-size devices."""
    out = set()
    for kernel, H, W in BOARDS:
        k = 12 if kernel == "band" else 32
        width = W // 32 if kernel == "band" else W
        for n in range(1, 9):
            shares = sorted({y1 - y0 for y0, y1 in (G.partition_rows(H, n, i) for i in range(n))})
            for R in shares:
                launches = {(row0, rows) for mode in ("serial", "edge_first", "overlap")
                            for _, _, row0, rows in G.step_plan(R, k, k, mode)}
                for row0, rows in sorted(launches):
                    for cus, slots in _devices(kernel, (256, 304)):
                        out.add((kernel, rows, row0, width, _pitch(kernel, width, n in (3, 8)), cus, slots, 0))
    return sorted(out)


@pytest.mark.parametrize("kernel", ["band", "bytes"])
def test_generic_sweep(G, kernel):
    for case in generic_cases(kernel):
        check_plan(G, *case)


@pytest.mark.parametrize("kernel", ["band", "bytes"])
def test_mode_thresholds(G, kernel):
    for case, want in threshold_cases(kernel):
        assert check_plan(G, *case) in want, (case, want)


def test_baseline_boards_shares_and_step_plans(G):
    cases = baseline_cases(G)
    assert len(cases) > 300 and any(c[2] > 0 for c in cases)
    for case in cases:
        check_plan(G, *case)


def test_every_mode_occurs_in_the_sweep(G):
    """A later change of thresholds must not empty a mode of the sweep silently."""
    seen = {"band": set(), "bytes": set()}
    cases = baseline_cases(G)
    for kernel in seen:
        cases += generic_cases(kernel) + [c for c, _ in threshold_cases(kernel)]
    for c in cases:
        seen[c[0]].add(G.strip_plan(*c, records=False)[0]["mode"])
    assert seen == {"band": BAND_MODES, "bytes": BYTES_MODES}


def test_device_that_is_no_multiple_of_8_never_ranks(G):
    for kernel in ("band", "bytes"):
        for case in generic_cases(kernel):
            if case[5] % 8:
                assert not G.strip_plan(*case, records=False)[0]["mode"].startswith("ranked"), case


def test_bad_arguments(G):
    L = G.lib()
    import ctypes
    info, n = G._lib.gol_strip_info(), ctypes.c_int64()
    ok = (0, 1000, 0, 232, 232, 12, 0, 8, 32)

    def call(*a):
        return L.gol_strip_plan(*a, ctypes.byref(info), None, 0, ctypes.byref(n))
    assert call(*ok) == 0 and n.value > 0
    for i, v in ((0, 2), (1, 0), (2, -1), (3, 0), (3, 230), (4, 228), (5, 8), (7, -8), (8, -1)):
        bad = list(ok)
        bad[i] = v
        assert call(*bad) == G._lib.GOL_EINVAL, bad
    assert call(1, 1000, 0, 1024, 1024, 12, 0, 8, 24) == G._lib.GOL_EINVAL  # the byte pipeline is k = 32
    assert L.gol_strip_plan(*ok, None, None, 0, ctypes.byref(n)) == G._lib.GOL_EINVAL
