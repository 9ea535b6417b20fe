"""The launch model and the case table of tests/batch_ref.py, the part that needs no GPU: the table
covers all 85 instantiations of batch_step_kernel with every width and height class; every case meets
the preconditions of gol_dev_batch_step and shows, on the reference alone, what it is there for; the
model, cut into launches of 1, 5 and 7 turns, gives the whole call's results as cycle_ref, search_ref and
the settle definition have them; it agrees with the host twins where they define the same thing; and
gol_batch_step_host agrees with rule_ref.step at every width 1..512."""
import ctypes

import numpy as np
import pytest

import batch_ref as B
import cycle_ref as C
import rule_ref as R
from batch_ref import to_words
from testlib import GOL_EINVAL, check_program, cpu_lib as G  # noqa: F401 (the fixture)


# ---------------------------------------------------------------- the table

def test_the_85_instantiations():
    want = set()
    for nw in (1, 2, 4, 8, 16):
        for rule in (0, 1, 2):  # B3/S23, one table rule, a rule per board
            for scan, lst in ((0, False), (1, False), (2, False), (2, True), (0, True)):
                want.add((nw, rule, scan, lst, False))
        for rule in (0, 1):
            want.add((nw, rule, 2, True, True))
    assert len(want) == 85 and len(B.INSTANTIATIONS) == 85 and set(B.INSTANTIATIONS) == want
    assert len({B.inst_id(i) for i in B.INSTANTIATIONS}) == 85


@pytest.mark.parametrize("inst", B.INSTANTIATIONS, ids=B.inst_id)
def test_coverage_of_an_instantiation(inst):
    nw, rule, scan, lst, aged = inst
    cases = B.cases_of(inst)
    assert len({c.id for c in cases}) == len(cases)
    assert all(c.inst == inst and B.words_per_lane(c.W) == nw and 3 <= c.turns <= 9 for c in cases)
    # the width classes, at a small height
    classes = {"min": 16 * nw + 1, "full-1": 32 * nw - 1, "full": 32 * nw}
    if nw == 1:
        classes.update(w1=1, w2=2, w3=3)
    if nw >= 4:
        classes["odd-nwr"] = {4: 90, 8: 150, 16: 270}[nw]
        nwr, Ww = (classes["odd-nwr"] + 31) // 32, (classes["odd-nwr"] + 63) // 64
        assert nwr % 2 == 1 and nwr < nw and (nw == 4 or 2 * Ww < nw)
    assert {(c.wclass, c.W) for c in cases if c.tag == "width"} == set(classes.items())
    assert all(c.H == 5 for c in cases if c.tag == "width")
    # the height classes, at one width of the class
    tall = [c for c in cases if c.tag == "height"]
    assert [c.H for c in tall] == [1, 2, 64, 65, 128, 129, 193, 257, 512] and {c.W for c in tall} == {classes["min"]}
    assert {B.shape(c.H) for c in tall} == {(1, 4), (2, 2), (3, 1), (4, 1), (5, 1), (8, 1)}
    for c in cases:
        if c.tag in ("width", "height", "big", "zero-count", "freeze"):
            assert c.n == 2 * B.shape(c.H)[1] + 1  # two workgroups and one board of a third
    assert sum(c.tag == "big" for c in cases) == (1 if nw == 16 and rule == B.RULE_CONWAY else 0)
    plain = [c for c in cases if c.tag in ("width", "height")]
    if lst:
        assert {c.count_kind for c in cases} == {"lt", "eq", "zero"}
        for c in cases:
            assert {"lt": c.count < c.slots, "eq": c.count == c.slots > 0, "zero": c.count == 0}[c.count_kind]
            if c.tag not in ("sens-words", "sens-waves"):  # a shuffled strict subset
                ent = c.list[:len(c.list) if c.count_kind == "zero" else c.count].tolist()
                assert len(ent) < c.n and ent != sorted(ent)
    if scan != B.SCAN_NONE and not aged:
        assert {(c.have_prev, c.write_prev) for c in plain} == {(a, b) for a in (False, True) for b in (False, True)}
        assert {c.done > 0 for c in plain} == ({False, True} if scan == B.SCAN_CYCLES else {False})
    if aged:
        assert all(c.write_prev and c.turn0 == 0 for c in cases) and any(c.tag == "freeze" for c in cases)
        assert {c.done for c in cases} == {0, 6}
    if rule == B.RULE_EACH:
        for c in cases:
            _, bpw = B.shape(c.H)
            assert len({tuple(r) for r in c.rules.tolist()}) >= 3
            if bpw > 1:  # boards of one workgroup under different rules
                ent = list(c.listed()) or list(range(c.n))
                assert any(len({tuple(c.rules[b].tolist()) for b in ent[i:i + bpw]}) > 1 for i in range(0, len(ent), bpw))
    # scan sensitivity: every word at the full and the odd width, every wave of two and of eight
    sens = [c for c in cases if c.tag.startswith("sens")]
    if scan == B.SCAN_NONE:
        assert not sens
    else:
        words = {(c.W, x // 32) for c in sens if c.tag == "sens-words" for _, x in c.expect["places"]}
        assert words == {(W, j) for W in {32 * nw, classes.get("odd-nwr", 32 * nw)} for j in range((W + 31) // 32)}
        for c in sens:
            for y, x in c.expect["places"]:  # the mover's box over the launch, inside one word and one wave
                assert x // 32 == (x + 6) // 32 and x + 6 < c.W and y // 64 == (y + 6) // 64 and y + 6 < c.H
        waves = {(c.H, y // 64) for c in sens if c.tag == "sens-waves" for y, _ in c.expect["places"]}
        assert waves == {(128, w) for w in range(2)} | {(512, w) for w in range(8)}


@pytest.mark.parametrize("inst", B.INSTANTIATIONS, ids=B.inst_id)
def test_cases_are_valid_and_show_their_point(inst):
    for c in B.cases_of(inst):
        c.valid()
        c.check()


# ---------------------------------------------------------------- the launch check, without a launch


def fake_ptr(name):
    """A non-null address per buffer: the check reads no memory."""
    return 0x1000 * (1 + B.BUFFERS.index(name))


def check_sets():
    """(accept, refuse): the arguments of every case's launch and the six good launches of the refusal list; the
    refusal list.  Each a list of the arguments in the entry's order."""
    bad, good = B.refusals({k: fake_ptr(k) for k in B.BUFFERS})
    accept = [B.launch_args(c, fake_ptr) for inst in B.INSTANTIATIONS for c in B.cases_of(inst)] + good
    return [[a[k] for k in B.STEP_ARGS] for a in accept], [[a[k] for k in B.STEP_ARGS] for a in bad]


def test_the_check_accepts_every_case_and_refuses_the_list(G):
    """gol_batch_step_check_host (gol_batch_launch_ok, the check of every launch) on the table's 1376 launches and
    on the refusal list that tests/test_gpu_batch_kernels.py::test_refusals runs through gol_dev_batch_step."""
    check = G.lib().gol_batch_step_check_host
    accept, refuse = check_sets()
    assert len(accept) == 1376 + 6 and len(refuse) == 50
    for a in accept:
        assert check(*a) == 0, a
    for a in refuse:
        assert check(*a) == GOL_EINVAL, a


def test_the_check_under_sanitizers(tmp_path):
    """The same two sets through gol_batch_launch_ok in the stand-alone program (build/asan/batch_check launch): a
    line per launch, the expected answer first, NULL as 0."""
    import subprocess
    accept, refuse = check_sets()
    path = tmp_path / "launches.txt"
    path.write_text("".join(" ".join(str(int(v or 0)) for v in [ok] + a) + "\n"
                            for ok, group in ((1, accept), (0, refuse)) for a in group))
    r = subprocess.run([check_program("batch_check"), "launch", str(path)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert f"batch_check launch: {len(accept)} accepted, {len(refuse)} refused, 0 bad" in r.stdout


def test_pack_is_the_bit_order_of_load_words():
    for H, W in [(1, 1), (3, 63), (3, 64), (2, 65), (3, 150), (2, 512)]:
        cells = R.random_board(W, H, W, 0.5)
        assert np.array_equal(B.pack(cells), to_words(cells)) and np.array_equal(B.unpack(B.pack(cells), W), cells)


# ---------------------------------------------------------------- chains of launches against the whole call

def mix_16():
    cells = np.zeros((9, 16, 16), np.uint8)
    for i, (rows, y, x) in enumerate([([], 0, 0), (C.BLOCK, 3, 3), (C.BLINKER, 5, 4), (C.GLIDER, 1, 1), (C.R_PENTOMINO, 6, 6),
                                      (C.PULSAR, 1, 1)]):
        cells[i] = C.place(16, 16, rows, y, x)
    for i in range(6, 9):
        cells[i] = R.random_board(1000 + i, 16, 16, 0.35)
    return cells


def chain(cells, L, total, scan, t0, rules=None, left=None, lst=None):
    """The call in launches of L turns (the last one shorter), prev / done / turn0 threaded through."""
    n = len(cells)
    st = dict(boards=B.pack(cells), prev=np.full((n, 16, 1), B.GAP, np.uint64),
              settled=None if scan == B.SCAN_NONE else np.full(n, -1, np.int64), left=left)
    done = 0
    while done < total:
        turns = min(L, total - done)
        w = B.launch_model(st["boards"], st["prev"], st["settled"], st["left"], H=16, W=16, turns=turns, turn0=t0 + done,
                           have_prev=scan != B.SCAN_NONE and done > 0, write_prev=scan != B.SCAN_NONE, rules=rules, scan=scan,
                           done=done if scan == B.SCAN_CYCLES else 0, list=lst, count=None if lst is None else len(lst))
        st = {k: w[k] for k in st}
        done += turns
    return st


@pytest.mark.parametrize("L", [1, 5, 7, 40])
def test_chain_of_launches_is_the_whole_call(L):
    cells, total, t0 = mix_16(), 40, 5
    rules = np.array([R.masks(C.RULES[i % 4]) for i in range(9)], np.uint32)
    for rl in (None, rules):
        each = [R.CONWAY if rl is None else tuple(int(v) for v in rl[b]) for b in range(9)]
        final = np.stack([R.run(c, r, total)[0] for c, r in zip(cells, each)])
        # plain
        assert np.array_equal(B.unpack(chain(cells, L, total, B.SCAN_NONE, t0, rl)["boards"], 16), final)
        # the cycle scan, of every board and of a list of them
        want = C.scan_all(cells, each, total, t0)
        got = chain(cells, L, total, B.SCAN_CYCLES, t0, rl)
        assert got["settled"].tolist() == want[0].tolist() and np.array_equal(B.unpack(got["boards"], 16), want[2])
        if rl is None:
            assert want[0].tolist()[:6] == [6, 6, 8, -1, -1, 11]  # still, still, period 2, none, none, period 3
        lst = [7, 2, 5, 0]
        got = chain(cells, L, total, B.SCAN_CYCLES, t0, rl, lst=lst)
        assert got["settled"].tolist() == [int(want[0][b]) if b in lst else -1 for b in range(9)]
        assert all(np.array_equal(B.unpack(got["boards"][b], 16), want[2][b] if b in lst else cells[b]) for b in range(9))
        # the settle scan: the first t >= t0 + 2 with s(t) == s(t - 2)
        got = chain(cells, L, total, B.SCAN_SETTLE, t0, rl)
        for b in range(9):
            s = [cells[b]]
            for _ in range(total):
                s.append(R.step(s[-1], *each[b]))
            assert got["settled"][b] == next((t0 + t for t in range(2, total + 1) if np.array_equal(s[t], s[t - 2])), -1), b
        assert np.array_equal(B.unpack(got["boards"], 16), final)
        # the finish: every listed board its own number of turns
        left = np.array([0, 3, 40, 41, 7, 12, 100, 5, 1], np.int64)
        got = chain(cells, L, total, B.SCAN_NONE, t0, rl, left=left, lst=list(range(8)))
        assert got["left"].tolist() == [0, 0, 0, 1, 0, 0, 60, 0, 1]
        for b in range(9):
            made = min(int(left[b]), total) if b < 8 else 0
            assert np.array_equal(B.unpack(got["boards"][b], 16), R.run(cells[b], each[b], made)[0]), b


@pytest.mark.parametrize("L", [1, 5, 7])
def test_aged_chain_is_the_search(L):
    """Six soups through six slots, soup g put into its slot before launch g: found at its own age, and the
    snapshot left in prev is s(found), as search_ref has them (cycle_ref.scan from the soup; the oracle's count
    and hash of the state the numpy stepper reaches)."""
    import search_ref as S
    from oracle import oracle as O
    H = W = 16
    seed, horizon, n = 1, 300, 6
    want = S.search(seed, 0, n, H, W, "B3/S23", horizon)
    assert np.sum(want[0] > 0) >= 4 and len(set(want[1][want[1] > 0].tolist())) >= 2  # (the reference alone)
    boards = np.stack([S.soup_words(seed, g, H, W) for g in range(n)])
    prev, settled = np.full_like(boards, B.GAP), np.full(n, -1, np.int64)
    born = np.array([L * g for g in range(n)], np.int64)
    done = 0
    while True:
        lst = [g for g in range(n) if born[g] <= done and settled[g] < 0 and done - born[g] < horizon]
        if not lst and done >= born[-1]:
            break
        if lst:
            w = B.launch_model(boards, prev, settled, None, H=H, W=W, turns=L, have_prev=done > 0, write_prev=True,
                               scan=B.SCAN_CYCLES, done=done, list=lst, count=len(lst), born=born)
            boards, prev, settled = w["boards"], w["prev"], w["settled"]
        done += L
    for g in range(n):
        hit = 0 <= settled[g] <= horizon
        assert (int(settled[g]) if hit else -1) == want[0][g], g
        if hit:
            assert settled[g] - C.last_mark(int(settled[g])) == want[1][g]
            assert O.popcount_words(prev[g]) == want[2][g] and O.hash_words(prev[g]) == want[3][g], g


# ---------------------------------------------------------------- the host twins

@pytest.mark.parametrize("H,W", [(5, 17), (3, 150), (4, 256), (3, 270), (65, 31), (2, 512)])
def test_model_agrees_with_step_host(G, H, W):
    Ww = (W + 63) // 64
    for rule in ("B3/S23", "B36/S23", "B0/S8"):
        b, s = R.masks(rule)
        boards = B.pack(R.random_board(H + W, H, W, 0.4))[None]
        want = B.launch_model(boards, None, None, None, H=H, W=W, turns=1, rule=(b, s))["boards"]
        out = np.zeros((H, Ww), np.uint64)
        assert G.lib().gol_batch_step_host(H, W, b, s, boards.ctypes.data, out.ctypes.data, Ww) == 0
        assert np.array_equal(out, want[0]), rule


def test_model_agrees_with_cycles_host(G):
    cells = mix_16()
    boards = B.pack(cells)
    for rule in ("B3/S23", "B36/S23"):
        b, s = R.masks(rule)
        w = B.launch_model(boards, np.full_like(boards, B.GAP), np.full(9, -1, np.int64), None, H=16, W=16, turns=40, rule=(b, s),
                           scan=B.SCAN_CYCLES)
        for i in range(9):
            out = np.zeros((16, 1), np.uint64)
            found, period = ctypes.c_int64(0), ctypes.c_int64(0)
            assert G.lib().gol_batch_cycles_host(16, 16, b, s, boards[i].ctypes.data, out.ctypes.data, 1, 40, ctypes.byref(found),
                                                 ctypes.byref(period)) == 0
            f = int(w["settled"][i])
            assert (found.value, period.value) == (f, f - C.last_mark(f) if f > 0 else -1), i
            assert np.array_equal(out, w["boards"][i])
        assert np.sum(w["settled"] > 0) >= 4 and np.any(w["settled"] < 0)


@pytest.mark.parametrize("rule", ["B3/S23", "B36/S23", "B0/S8"])
def test_step_host_at_every_width(G, rule):
    """gol_batch_step_host against rule_ref.step at every width 1..512, one row and three, three turns: every
    count of words in use, every place of the last cell in its word."""
    b, s = R.masks(rule)
    step = G.lib().gol_batch_step_host
    for W in range(1, 513):
        Ww = (W + 63) // 64
        for H in (1, 3):
            cells = R.random_board(3 * W + H, H, W, 0.45)
            buf = B.pack(cells)
            for t in range(3):
                cells = R.step(cells, b, s)
                assert step(H, W, b, s, buf.ctypes.data, buf.ctypes.data, Ww) == 0
                assert np.array_equal(buf, B.pack(cells)), (H, W, t)
