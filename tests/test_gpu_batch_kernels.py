"""Every instantiation of batch_step_kernel<NW, RULE, SCAN, LIST, AGED> (csrc/gol_batch.hip) on caller
memory, one launch at a time through gol_dev_batch_step, against the launch model of tests/batch_ref.py
(numpy rolls and a brute-force mark list, written from include/golhip.h), bit for bit.  The case table
is batch_ref's (its coverage is asserted in tests/test_batch_ref_cpu.py): per instantiation the width
and height classes of its words per lane, the list, scan, finish and aged variants, and the boards whose
only moving cells sit in one word or one wave.  Every buffer of a launch -- boards, prev, settled, left,
and the inputs born, list, count and rules -- lies between two margins of sentinel bytes and is compared
whole, margins included, so a word written for a board that is not listed, past *count or out of place
shows."""
import numpy as np
import pytest

import batch_ref as B
import cycle_ref as C
import rule_ref as R
from testlib import GOL_EINVAL, Guarded, error_word, gpu_lib as G  # noqa: F401 (the fixture)

pytestmark = pytest.mark.gpu

NAMES = ("boards", "prev", "settled", "left", "born", "list", "count", "rules")


def _buffers(host):
    """The device buffers of a launch: name -> Guarded of the host array (a buffer the launch does not have: absent)."""
    return {k: Guarded(v, name=k) for k, v in host.items() if v is not None}


def _ptr(buf, name):
    return buf[name].ptr if name in buf else None


def _host_buffers(c):
    return {"boards": c.boards, "prev": c.prev, "settled": c.settled, "left": c.left, "born": c.born, "list": c.list,
            "count": None if c.count is None else np.array([c.count], np.int32),
            "rules": None if c.rules is None else c.rules}


def _call(G, buf, c, **over):
    import torch
    a = dict(n=c.n, H=c.H, W=c.W, turns=c.turns, turn0=c.turn0, have_prev=int(c.have_prev), write_prev=int(c.write_prev),
             birth=c.rule[0], survive=c.rule[1], scan=c.scan, done=c.done, slots=c.slots)
    a.update(over)
    return G.lib().gol_dev_batch_step(_ptr(buf, "boards"), _ptr(buf, "prev"), _ptr(buf, "settled"), a["n"], a["H"], a["W"], a["turns"],
                                      a["turn0"], a["have_prev"], a["write_prev"], a["birth"], a["survive"], _ptr(buf, "rules"),
                                      a["scan"], a["done"], _ptr(buf, "list"), _ptr(buf, "count"), a["slots"], _ptr(buf, "left"),
                                      _ptr(buf, "born"), torch.cuda.current_stream().cuda_stream)


def _compare(buf, host, want, where):
    """Every buffer whole (margins included) against `want` (name -> array; a name not in it: unchanged, as in `host`)."""
    for name, g in buf.items():
        g.expect(host[name] if want.get(name) is None else want[name], where)


def _run_case(G, c):
    import torch
    host = _host_buffers(c)
    buf = _buffers(host)
    rc = _call(G, buf, c)
    assert rc == 0, (c.id, G.lib().gol_last_error())
    torch.cuda.synchronize()
    w = c.want
    _compare(buf, host, {"boards": w["boards"], "prev": w["prev"], "settled": w["settled"], "left": w["left"]}, c.id)


@pytest.mark.parametrize("inst", B.INSTANTIATIONS, ids=B.inst_id)
def test_instantiation(G, inst):
    cases = B.cases_of(inst)
    assert cases
    for c in cases:
        _run_case(G, c)
    assert error_word(G) == (0, 0)


# ---------------------------------------------------------------- three launches, prev / done / turn0 threaded through

CHAIN = (5, 7, 4)
CHAIN_INSTS = [(1, B.RULE_TABLE) + B.MODES["plain"], (2, B.RULE_CONWAY) + B.MODES["settle"], (4, B.RULE_EACH) + B.MODES["cycles"],
               (8, B.RULE_TABLE) + B.MODES["list"], (2, B.RULE_EACH) + B.MODES["finish"], (16, B.RULE_CONWAY) + B.MODES["aged"]]


def chain_boards(H, W):
    """Blocks, a blinker, a pulsar, a glider, a soup, an empty board, a blinker, blocks and a pulsar, 17 rows."""
    pats = [(C.BLOCK, 3, 3), (C.BLINKER, 5, 4), (C.PULSAR, 2, 2), (C.GLIDER, 1, 1), None, ([], 0, 0), (C.BLINKER, 9, 8),
            (C.BLOCK, 7, 9), (C.PULSAR, 2, 1)]
    return np.stack([R.random_board(77, H, W, 0.3) if p is None else C.place(H, W, *p) for p in pats])


@pytest.mark.parametrize("inst", CHAIN_INSTS, ids=B.inst_id)
def test_chained_launches(G, inst):
    """The result is the model's, launch by launch, and the whole call's: rule_ref's run, the settle definition,
    cycle_ref.scan of every board from the call's (aged: the board's own) first turn."""
    import torch
    nw, rule_mode, scan, lst, aged = inst
    mode = B.MODE_OF[(scan, lst, aged)]
    H, W, n, t0 = 17, B.width_classes(nw)["min"], 9, 0 if aged else 20
    cells = chain_boards(H, W)
    names = B.SENS_RULES if mode in ("cycles", "list") else B.ERULES
    rule, rules = B._rule_args(rule_mode, n, names)
    if rule_mode == B.RULE_TABLE:
        rule = R.masks("B38/S23")  # (a pulsar is one under it)
    total = sum(CHAIN)
    host = dict(boards=B.pack(cells), prev=np.full((n, H, (W + 63) // 64), B.GAP, np.uint64), settled=None, left=None, born=None,
                list=None, count=None, rules=rules)
    if scan != B.SCAN_NONE:
        host["settled"] = np.full(n, -1, np.int64)
    order = [4, 8, 1, 0, 3, 2, 6]  # all but boards 5 and 7
    if lst:
        host["list"], host["count"] = np.array(order, np.int32), np.array([len(order)], np.int32)
    if mode == "finish":
        host["left"] = np.full(n, B.FILL64, np.int64)
        host["left"][order] = [0, 3, 5, 16, 20, 9, 12]
    if aged:  # board 6 (a blinker) comes into its slot before the second launch
        host["born"] = np.full(n, B.FILL64, np.int64)
        host["born"][order] = [0, 0, 0, 0, 0, 0, CHAIN[0]]
    buf = _buffers(host)
    state = {k: (None if v is None else v.copy()) for k, v in host.items()}
    done = 0
    for i, turns in enumerate(CHAIN):
        count = None if not lst else len(order) if not aged or i > 0 else len(order) - 1
        if aged:
            buf["count"].write(np.array([count], np.int32))
        hp = scan != B.SCAN_NONE and i > 0
        wp = scan != B.SCAN_NONE and (aged or i < 2)
        a = dict(turns=turns, turn0=0 if aged else t0 + done, have_prev=int(hp), write_prev=int(wp), birth=rule[0], survive=rule[1],
                 scan=scan, done=done if scan == B.SCAN_CYCLES else 0, slots=len(order) if lst else 0, n=n, H=H, W=W)
        rc = G.lib().gol_dev_batch_step(_ptr(buf, "boards"), _ptr(buf, "prev"), _ptr(buf, "settled"), n, H, W, turns, a["turn0"], a["have_prev"],
                                        a["write_prev"], rule[0], rule[1], _ptr(buf, "rules"), scan, a["done"], _ptr(buf, "list"),
                                        _ptr(buf, "count"), a["slots"], _ptr(buf, "left"), _ptr(buf, "born"),
                                        torch.cuda.current_stream().cuda_stream)
        assert rc == 0, G.lib().gol_last_error()
        w = B.launch_model(state["boards"], state["prev"], state["settled"], state["left"], H=H, W=W, turns=turns, turn0=a["turn0"],
                           have_prev=hp, write_prev=wp, rule=rule, rules=rules, scan=scan, done=a["done"],
                           list=state["list"], count=count, born=state["born"])
        state.update({k: w[k] for k in ("boards", "prev", "settled", "left")})
        done += turns
    torch.cuda.synchronize()
    if aged:
        state["count"] = np.array([len(order)], np.int32)
    _compare(buf, host, state, B.inst_id(inst))
    # the whole call, from the references that know nothing of launches
    run = list(range(n)) if not lst else order
    rl = [rule if rules is None else tuple(int(v) for v in rules[b]) for b in range(n)]
    made = {b: total for b in run}
    if mode == "finish":
        made = {b: min(total, int(host["left"][b])) for b in run}
        assert state["left"][order].tolist() == [int(host["left"][b]) - made[b] for b in order]
    if aged:
        made = {b: total - int(host["born"][b]) for b in run}
    for b in range(n):
        want = R.run(cells[b], rl[b], made[b])[0] if b in run else cells[b]
        assert np.array_equal(B.unpack(state["boards"][b], W), want), b
    if scan == B.SCAN_SETTLE:
        for b in run:
            s = [cells[b]]
            for _ in range(total):
                s.append(R.step(s[-1], *rl[b]))
            want = next((t0 + t for t in range(2, total + 1) if np.array_equal(s[t], s[t - 2])), -1)
            assert state["settled"][b] == want, b
        assert {-1, t0 + 2} <= set(state["settled"].tolist())  # (a pulsar and a glider never settle)
    if scan == B.SCAN_CYCLES:
        found = {b: C.scan(cells[b], rl[b], made[b], t0)[0] for b in run}
        assert [int(state["settled"][b]) for b in run] == [found[b] for b in run]
        assert all(state["settled"][b] == -1 for b in range(n) if b not in run)
        got = {found[b] - t0 for b in run}
        assert {-1 - t0, 1, 3, 6} <= got  # never, a still life, period 2, period 3 past the first launch
    assert error_word(G) == (0, 0)


# ---------------------------------------------------------------- refusals

def test_refusals(G):
    """Every GOL_EINVAL path of the entry; nothing is launched, so every buffer stays."""
    import torch
    n, H, W = B.REFUSAL_SHAPE
    boards = B.pack(B._compose(n, H, W, 3))
    host = dict(boards=boards, prev=np.full_like(boards, B.GAP), settled=np.full(n, -1, np.int64), left=np.full(n, 2, np.int64),
                born=np.zeros(n, np.int64), list=np.arange(n, dtype=np.int32), count=np.array([n], np.int32),
                rules=np.array([R.CONWAY] * n, np.uint32))
    buf = _buffers(host)
    L = G.lib()
    p = {k: _ptr(buf, k) for k in NAMES}
    st = torch.cuda.current_stream().cuda_stream

    def call(a):
        return L.gol_dev_batch_step(*[a[k] for k in B.STEP_ARGS], st)

    bad, good = B.refusals(p)  # (the list of tests/test_batch_ref_cpu.py, which asks the check alone)
    for a in bad:
        assert call(a) == GOL_EINVAL, a
        assert L.gol_last_error()
    torch.cuda.synchronize()
    _compare(buf, host, {}, "refusals")
    # (each family's base arguments are good: one launch of each, on the same buffers)
    assert len(good) == 6
    for a in good:
        assert call(a) == 0, (a, L.gol_last_error())
    torch.cuda.synchronize()
    assert error_word(G) == (0, 0)
