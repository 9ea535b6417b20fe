"""The engine model (tests/engine_model.py) is right and its sequences are worth running: the part
of the differential test that needs no GPU.  The model's stepping against oracle.run, bits_run and
tests/rule_ref.py; its paste, copy and bounds against the library's host twins (gol_paste_host,
gol_copy_host, gol_bounds_host) on the very rectangles the generator emits; the coverage and
liveliness conditions of the fixed seeds that tests/test_gpu_sequences.py runs; and replay() against
a second model, whole and with one paste cell flipped."""
import ctypes
import functools

import numpy as np
import pytest

import engine_model as M
import rule_ref as R
from oracle import oracle as O
from region_ref import from_layout
from testlib import cpu_lib as G  # noqa: F401 (the fixture)

IDS = list(M.CONFIGS)
BIT_IDS = [i for i in IDS if M.Model.of(M.CONFIGS[i]).bit]
SHARDED_IDS = [i for i in IDS if M.CONFIGS[i]["engine"].get("shards", 1) > 1]


@functools.lru_cache(maxsize=None)
def sequences(cid, seeds=None):
    """(seed, ops, check points) of every fixed sequence of a config."""
    return [(s, M.generate(M.CONFIGS[cid], s, M.LENGTH), M.check_points(s, M.LENGTH)) for s in seeds or M.SEEDS[cid]]


failed = M.is_error


# ------------------------------------------------------------------ stepping
@pytest.mark.parametrize("cid", ["std2", "odd"])  # a bit board (exact first turn) and a byte board
@pytest.mark.parametrize("odd", [False, True])
def test_model_steps_as_the_oracle(cid, odd):
    c = M.CONFIGS[cid]
    start = M.make_bytes(c["H"], c["W"], 3, .4, odd)
    assert odd == (not np.isin(start, (0, 255)).all())
    for n in (1, 2, 3):
        m = M.Model.of(c)
        assert M.apply(m, ("load_bytes", (3, .4, odd))) is None and m.pending == (odd and m.bit)
        assert M.apply(m, ("step", (n,))) is None
        assert np.array_equal(m.board, O.run(start, n)) and m.turn == n and not m.pending
        if not odd and m.bit:  # the word-parallel restatement agrees
            assert np.array_equal(m.board, O.unpack(O.bits_run(O.pack(start), n)))


@pytest.mark.parametrize("rule,generic", M.RULES[1:])
def test_model_steps_other_rules_as_rule_ref(rule, generic):
    c = M.CONFIGS["std2"]
    m = M.Model.of(c)
    M.apply(m, ("load_random", (5,)))
    start = m.board.copy()
    assert M.apply(m, ("set_rule", (rule, generic))) is None and m.generic
    M.apply(m, ("step", (2,)))
    M.apply(m, ("step", (3,)))
    assert np.array_equal(m.board, R.to_bytes(R.run(start, rule, 5)[0])) and m.turn == 5
    assert M.apply(m, ("to_rle", (0, 0, 1, 1)))[1] == rule


@pytest.mark.parametrize("turns,every", [(12, 1), (13, 5), (24, 12), (5, 8), (33, 33)])
def test_model_step_counted_gives_the_oracle_counts(turns, every):
    m = M.Model.of(M.CONFIGS["std2"])
    M.apply(m, ("load_random", (9,)))
    words = O.pack(m.board)
    _, counts = O.bits_run(words, turns, with_counts=True)
    got = M.apply(m, ("step_counted", (turns, every)))
    assert got == [int(counts[t - 1]) for t in range(every, turns + 1, every)] and len(got) == turns // every
    assert m.turn == turns and np.array_equal(O.pack(m.board), O.bits_run(words, turns))


# ------------------------------------------------------------------ the host twins
def host_buffers(model, board):
    """The board as host buffers of every layout its engine may hold it in: (layout, buffer, pitch)."""
    if not model.bit or model.pending:
        return [(0, board.copy(), model.W)]
    cells = board != 0
    Wd = model.W // 32
    out = [(1, np.packbits(cells.reshape(model.H, Wd, 32), axis=2, bitorder="little").view("<u4")[:, :, 0].copy(), Wd)]
    if model.band:
        out.append((2, np.packbits(cells.reshape(model.H, 32, Wd).transpose(0, 2, 1), axis=2,
                                   bitorder="little").view("<u4")[:, :, 0].copy(), Wd))
    return out


def row_runs(y0, h, H):
    """A rectangle's rows as runs that do not wrap: (board row, rows, pattern row)."""
    first = min(h, H - y0)
    return [(y0, first, 0)] + ([(0, h - first, first)] if h > first else [])


def twin_paste(L, model, before, op, want_changed):
    name, a = op
    x0, y0, w, h = a[:4]
    pop = "andnot" if name == "cut" else a[4]
    import golhip
    packed = golhip._lib.pack_pattern(M.make_pattern(h, w, a[5])) if name == "paste" else None
    for layout, buf, pitch in host_buffers(model, before):
        total = 0
        for row, rows, prow in row_runs(y0, h, model.H):
            n = ctypes.c_int64(-1)
            rc = L.gol_paste_host(layout, buf.ctypes.data, pitch, model.W, row, rows, prow, x0, w,
                                  None if packed is None else packed.ctypes.data, 0 if packed is None else packed.shape[1],
                                  M.PASTE_OPS.index(pop), ctypes.byref(n))
            assert rc == 0, (op, L.gol_last_error())
            total += n.value
        assert total == want_changed, (op, layout)
        if layout == 0:
            assert np.array_equal(buf, model.board), op  # byte for byte: untouched odd bytes stay
        else:
            assert np.array_equal(from_layout(layout, buf, model.W), model.board != 0), (op, layout)


def twin_copy(L, model, before, op, want_cells, want_alive):
    x0, y0, w, h = op[1][:4]
    pw = (w + 63) // 64
    for layout, buf, pitch in host_buffers(model, before):
        pat = np.zeros((h, pw), np.uint64)
        total = 0
        for row, rows, prow in row_runs(y0, h, model.H):
            n = ctypes.c_int64(-1)
            rc = L.gol_copy_host(layout, buf.ctypes.data, pitch, model.W, row, rows, prow, x0, w, pat.ctypes.data, pw,
                                 ctypes.byref(n))
            assert rc == 0, (op, L.gol_last_error())
            total += n.value
        cells = np.unpackbits(pat.view(np.uint8), axis=1, bitorder="little")[:, :w].astype(bool)
        assert np.array_equal(cells, want_cells) and total == want_alive, (op, layout)


def twin_bounds(L, model, before, op, want):
    x0, y0, w, h = op[1][:4]
    for layout, buf, pitch in host_buffers(model, before):
        c0, c1, r0, r1, alive = w, -1, h, -1, 0
        for row, rows, prow in row_runs(y0, h, model.H):
            v = [ctypes.c_int64(-7) for _ in range(5)]
            rc = L.gol_bounds_host(layout, buf.ctypes.data, pitch, model.W, row, rows, x0, w, *(ctypes.byref(x) for x in v))
            assert rc == 0, (op, L.gol_last_error())
            cmin, cmax, rmin, rmax, n = (x.value for x in v)
            if n:
                c0, c1, r0, r1, alive = min(c0, cmin), max(c1, cmax), min(r0, prow + rmin), max(r1, prow + rmax), alive + n
        got = (c0, r0, c1 - c0 + 1, r1 - r0 + 1, alive) if alive else (0, 0, 0, 0, 0)
        assert got == want, (op, layout)


@pytest.mark.parametrize("cid", IDS)
def test_model_edits_and_reads_agree_with_the_host_twins(G, cid):
    """Every paste, fill, cut, copy and bounds the fixed sequences hold, on the model's board at that
    point in every layout the engine may hold it in: model and library share one definition."""
    L = G.lib()
    done = dict(paste=0, fill=0, cut=0, copy=0, bounds=0)
    for seed, ops, _ in sequences(cid):
        m = M.Model.of(M.CONFIGS[cid])
        for op in ops:
            before, was = m.board.copy(), M.Model.of(M.CONFIGS[cid])
            was.pending = m.pending
            res = M.apply(m, op)
            if op[0] not in done or failed(res):
                continue
            done[op[0]] += 1
            if op[0] in ("paste", "fill"):
                twin_paste(L, m, before, op, res[0])
            elif op[0] == "bounds":
                twin_bounds(L, was, before, op, res)
            else:
                twin_copy(L, was, before, op, res[0], res[1])
                if op[0] == "cut":
                    twin_paste(L, m, before, op, res[1])
    assert min(done.values()) >= 3, done


# ------------------------------------------------------------------ the fixed seeds are worth running
@functools.lru_cache(maxsize=None)
def seed_stats(cid, seed):
    """What one sequence contributes to the conditions below, as counters that add up."""
    c = M.CONFIGS[cid]
    ops, checks = M.generate(c, seed, M.LENGTH), M.check_points(seed, M.LENGTH)
    bad = []
    names, pairs, fails, crossing, truncated = {}, {}, {}, 0, dict(step_flips=0, alive_cells=0)
    odd_read_step, points, lively = 0, 0, 0
    seams = M.shard_seams(c)
    # a step, then an edit (or load_words) with nothing between that makes the halo again -- a load,
    # another edit, a layout conversion -- then, again with nothing such between, the next step: the
    # windows in which a halo that the call failed to mark stale would be used
    windows = dict(edit=0, load_words=0)
    if ops != M.generate(c, seed, M.LENGTH) or len(ops) != M.LENGTH:
        bad.append(f"seed {seed}: not deterministic")
    if M.CLASS_OF[ops[0][0]] != "load":
        bad.append(f"seed {seed}: does not begin with a load")
    stage, nfail = 0, 0
    halo, armed, lay, turn = False, None, None, 0  # see `windows` above
    for (i, op, res, m), before in zip(M.trace(c, ops), [None] + ops[:-1]):
        cls = M.CLASS_OF[op[0]]
        if not failed(res):
            stepped = cls == "step" and m.turn != turn
            if stepped and armed and lay == m.layout:  # (a layout change converts, which makes the halo anyway)
                windows[armed] += 1
            if stepped or cls == "load" or lay != m.layout:
                armed = None
            if op[0] in M.HALO_STALE and halo and (cls == "edit" or lay == m.layout):
                armed = "load_words" if cls == "load" else "edit"
            halo = stepped or (halo and cls not in ("load", "edit") and lay == m.layout)
        lay, turn = m.layout, m.turn
        if before is not None:
            k = (M.CLASS_OF[before[0]], cls)
            pairs[k] = pairs.get(k, 0) + 1
        if failed(res):
            nfail += 1
            fails[(op[0], res[1])] = fails.get((op[0], res[1]), 0) + 1
        else:
            names[op[0]] = names.get(op[0], 0) + 1
            if cls == "edit" and M.crosses_seam(op[1][1], op[1][3], c["H"], seams):
                crossing += 1
            if op[0] in truncated and op[1][0] is not None and len(res) == op[1][0]:
                truncated[op[0]] += 1
            # an odd-byte load, an in-place read before turn 1, a step: in order
            if op[0] == "load_bytes" and m.pending:
                stage = max(stage, 1)
            elif stage == 1 and cls == "inplace" and m.pending:
                stage = 2
            elif stage == 2 and cls == "step" and m.turn > 0:
                stage = 3
            elif stage in (1, 2) and not m.pending:
                stage = 0
        if checks[i] or i == len(ops) - 1:
            points += 1
            lively += .02 < m.density() < .98
    if nfail > M.LENGTH // 10:
        bad.append(f"seed {seed}: {nfail} failing calls")
    odd_read_step += stage == 3
    return dict(names=names, pairs=pairs, fails=fails, truncated=truncated, windows=windows, bad=bad,
                n=dict(crossing=crossing, odd_read_step=odd_read_step, points=points, lively=lively))


def conditions(cid, seeds=None):
    """What the sequences of a config must cover; returns the conditions that do not hold."""
    c = M.CONFIGS[cid]
    stats = [seed_stats(cid, s) for s in seeds or M.SEEDS[cid]]

    def total(key):
        out = {}
        for st in stats:
            for k, v in st[key].items():
                out[k] = out.get(k, 0) + v
        return out
    names, pairs, fails, truncated, windows, n = (total(k) for k in ("names", "pairs", "fails", "truncated", "windows", "n"))
    crossing, odd_read_step, points, lively = n["crossing"], n["odd_read_step"], n["points"], n["lively"]
    bad = [b for st in stats for b in st["bad"]]
    for n in M.valid_names(c):
        if names.get(n, 0) < 3:
            bad.append(f"op {n} succeeds {names.get(n, 0)} times")
    for a in M.CLASSES:
        for b in M.CLASSES:
            if pairs.get((a, b), 0) < 2:
                bad.append(f"pair {a} -> {b} occurs {pairs.get((a, b), 0)} times")
    m = M.Model.of(c)
    must_fail = [(("store_rows",), M.EINVAL)]
    must_fail += [(M.CLASSES["edit"], M.ESTATE), (("store_words",), M.ESTATE), (M.CLASSES["step"], M.ESTATE)] if m.bit else \
                 [(("hash",), M.EINVAL), (("load_words",), M.EINVAL), (("store_words",), M.EINVAL), (("set_rule",), M.EINVAL)]
    for ns, code in must_fail:
        if not any(fails.get((n, code)) for n in ns):
            bad.append(f"no {'/'.join(ns)} that fails with {code}")
    if not any(k[1] == M.EINVAL and k[0] in ("paste", "fill", "copy", "cut", "bounds") for k in fails):
        bad.append("no rectangle wider than the board")
    if m.bit and odd_read_step < 1:
        bad.append("no odd-byte load, in-place read before turn 1, step in order")
    if m.shards > 1 and crossing < 5:
        bad.append(f"{crossing} edits across a shard seam")
    if m.shards > 1 and windows["edit"] < 4:
        bad.append(f"{windows['edit']} edits between two steps with the halo left to them")
    if m.shards > 1 and not m.band and windows["load_words"] < 3:  # (a band board converts, which makes the halo)
        bad.append(f"{windows['load_words']} load_words between two steps with the halo left to them")
    if min(truncated.values()) < 1:
        bad.append(f"capped lists {truncated}")
    if lively < .9 * points:
        bad.append(f"the board is between 2 % and 98 % alive at {lively} of {points} comparisons")
    return bad


@pytest.mark.parametrize("cid", IDS)
def test_fixed_seeds_cover_the_engine(cid):
    """Every op name at least 3 times, every ordered pair of op classes at least twice, every
    documented failure, the odd-byte path and the seam-crossing edits, on a board that stays
    between 2 % and 98 % alive at no fewer than 90 % of the comparisons."""
    assert conditions(cid) == []


def test_ops_fall_into_the_six_classes():
    assert sorted(M.CLASSES) == ["convert", "edit", "inplace", "load", "setting", "step"]
    assert len(M.CLASS_OF) == sum(len(v) for v in M.CLASSES.values()) == 25
    for cid in IDS:
        for _, ops, _ in sequences(cid):
            assert all(name in M.CLASS_OF for name, _ in ops)
            assert eval(repr(ops)) == ops  # an op list is a Python literal


# ------------------------------------------------------------------ replay checks itself
@pytest.mark.parametrize("cid", IDS)
def test_replay_passes_against_a_second_model(cid):
    c = M.CONFIGS[cid]
    for seed, ops, checks in sequences(cid):
        M.replay(M.ModelEngine, c, ops, checks, seed)


@pytest.mark.parametrize("cid", ["band3", "bytes"])
def test_replay_fails_where_one_paste_cell_is_flipped(cid):
    """One cell of one paste flipped in the stand-in engine: replay fails at exactly that op when the
    board is compared after it, and the message's literal fails there again."""
    c = M.CONFIGS[cid]
    # the first sequence with a paste under copy or xor (the flipped pattern cell always changes the board)
    seed, ops, at = next((seed, ops, i) for seed, ops, _ in sequences(cid) for i, op, res, m in M.trace(c, ops)
                         if op[0] == "paste" and op[1][4] in ("copy", "xor") and not failed(res) and i > 5)
    checks = [True] * len(ops)
    with pytest.raises(M.Mismatch) as ei:
        M.replay(lambda cfg: M.ModelEngine(cfg, tamper=(at, (0, 0))), c, ops, checks, seed)
    assert ei.value.index == at
    text = str(ei.value)
    scope = {}
    exec(text[text.index("config = "):], scope)  # the message is Python: config, seed, index, ops, checks
    assert (scope["config"], scope["seed"], scope["index"]) == (c, seed, at) and scope["ops"] == ops[:at + 1]
    with pytest.raises(M.Mismatch) as again:
        M.replay(lambda cfg: M.ModelEngine(cfg, tamper=(at, (0, 0))), scope["config"], scope["ops"], scope["checks"])
    assert again.value.index == at
    M.replay(M.ModelEngine, scope["config"], scope["ops"], scope["checks"])  # and the untampered one passes
