"""Every step-kernel instantiation of csrc/gol_kernels.hip at its column-group and row edges.

bits_step_kernel<K, DW>, band_step_kernel<K, DW, CONTIG> and their TableRule forms, through
gol_dev_bits_step / gol_dev_band_step / gol_dev_rule_step on caller-owned memory, against the numpy
torus stepper (tests/rule_ref.py), bit for bit.  The case table is tests/step_ref.py's (its coverage
is asserted in tests/test_step_ref_cpu.py): per instantiation the widths of one lane, one lane
under a column group, exactly one group and one lane over; ghost rows as the torus wrap, contiguous
with the shard and in buffers of their own; R == k; sub-ranges; strips of 1..6 rows as full strips
and as tails; pitch > Wd throughout.  Inputs are built in the kernel's layout by numpy (no
gol_dev_band_convert: these widths are not multiples of 32 words).  Everything that is not board
data -- pitch padding, guard rows around every allocation, all of dst -- holds a sentinel, so a
read or a write one word out of place shows: the rule with birth on 0 neighbours turns anything
read in place of a dead cell into live cells.
"""
import numpy as np
import pytest

import step_ref as S
from testlib import error_word, gpu_lib as G  # noqa: F401 (the fixture)

pytestmark = pytest.mark.gpu


def _dev(words):
    import torch
    return torch.from_numpy(np.ascontiguousarray(words).view(np.int32)).cuda()


def _host(t):
    return t.cpu().numpy().view(np.uint32)


def _slots(G):
    import torch
    s = torch.zeros(G._lib.GOL_COUNT_SLOTS * 8, dtype=torch.int64, device="cuda")
    s[S.COUNT_SEED[0]] = S.COUNT_SEED[1]
    return s


def _call(G, kind, k, dw, ptr, R, Wd, pitch, row0, rows, strip, rule, slots, stream):
    """The instantiation's entry; ptr: name -> device address."""
    lib = G.lib()
    head = (ptr["top"], ptr["mid"], ptr["bot"], ptr["dst"], R, Wd, pitch, row0, rows, k)
    if kind == "bits":
        return lib.gol_dev_bits_step(*head, 32 * dw, strip, slots, stream)
    if kind == "band":
        return lib.gol_dev_band_step(*head, 32 * dw, strip, slots, stream)
    import rule_ref as RR
    birth, survive = RR.masks(rule)
    layout = G._lib.GOL_LAYOUT_BAND if kind == "rule_band" else G._lib.GOL_LAYOUT_STANDARD
    return lib.gol_dev_rule_step(*head, layout, birth, survive, 32 * dw, strip, slots, stream)


def _launch(G, c, count=True):
    """One launch of case c on fresh buffers; returns (host buffers before, device buffers after, slots)."""
    import torch
    before = c.buffers()
    dev = {n: _dev(b) for n, b in before.items()}
    for t in dev.values():
        assert t.data_ptr() % 16 == 0
    ptr = {n: dev[al].data_ptr() + 4 * off for n, (al, off) in c.pointers().items()}
    if c.band:  # the kernel under test is the one the table says
        assert c.contiguous({al: t.data_ptr() // 4 for al, t in dev.items()}) == (c.form == "contig")
    slots = _slots(G) if count else None
    st = torch.cuda.current_stream().cuda_stream
    rc = _call(G, c.kind, c.k, c.dw, ptr, c.R, c.Wd, c.pitch, c.row0, c.rows, c.strip, c.rule,
               slots.data_ptr() if count else None, st)
    assert rc == 0, (c.id, G.lib().gol_last_error())
    torch.cuda.synchronize()
    assert error_word(G) == (0, 0), c.id
    return before, {n: _host(t) for n, t in dev.items()}, slots


def _check(c, before, after, slots):
    want = c.want_words()
    g = S.GUARD
    dst = after["dst"]
    got = dst[g + c.row0: g + c.row0 + c.rows, :c.Wd]
    bad = np.argwhere(got != want)
    assert bad.size == 0, f"{c.id}: {len(bad)} wrong words of {want.size}, first (row, word) {bad[:6].tolist()}"
    # nothing else of dst: the padding of the written rows, the other rows, the guard rows
    rest = dst.copy()
    rest[g + c.row0: g + c.row0 + c.rows, :c.Wd] = S.SENT
    bad = np.argwhere(rest != S.SENT)
    assert bad.size == 0, f"{c.id}: wrote outside its rows at (row, word) {(bad[:6] - [g, 0]).tolist()}"
    for name in before:
        if name != "dst":
            assert np.array_equal(after[name], before[name]), f"{c.id}: input buffer {name} changed"
    if slots is not None:
        assert int(slots.sum().item()) == S.COUNT_SEED[1] + S.popcount(want), c.id


@pytest.mark.parametrize("inst", S.PUBLIC, ids=S.inst_id)
def test_instantiation_at_its_edges(G, inst):
    cases = S.cases_of(inst)
    assert cases
    for c in cases:
        _check(c, *_launch(G, c))
    # once: without count_slots the same rows are written
    c = next(c for c in cases if c.tag == "sub" and c.form == "separate" and c.wclass == "one-lane-over"
             and c.rule == cases[-1].rule)
    before, after, _ = _launch(G, c, count=False)
    _check(c, before, after, None)


# ------------------------------------------------------------------ two launches on one stream
@pytest.mark.parametrize("kind,k,dw", [("bits", 4, 2), ("band", 4, 4), ("rule_std", 2, 2), ("rule_band", 2, 2)])
def test_chained_launches_see_each_other(G, kind, k, dw):
    """a -> b -> a over sub-ranges with no host synchronisation between: the second launch's ghost
    reads are rows the first one wrote (b held the sentinel before), and it overwrites rows of the
    buffer the first one read."""
    import torch
    inst = (kind, k, dw)
    rule = S.RULES[2] if kind.startswith("rule") else S.CONWAY
    Wd, R, g = S.useful_words(inst) + dw, 24, S.GUARD
    pitch = (Wd // 4 + 2) * 4
    pack = S.band_pack if S.is_band(kind) else S.std_pack
    seed = 77 + k
    t0 = S.torus(seed, R, Wd)
    a_host = np.full((R + 2 * g, pitch), S.SENT, dtype=np.uint32)
    a_host[g:g + R, :Wd] = pack(t0)
    a = _dev(a_host)
    b = _dev(np.full_like(a_host, S.SENT))
    st = torch.cuda.current_stream().cuda_stream
    slots = _slots(G)

    def ptrs(src, dst):
        mid = src.data_ptr() + 4 * g * pitch
        return {"top": mid + 4 * (R - k) * pitch, "mid": mid, "bot": mid, "dst": dst.data_ptr() + 4 * g * pitch}
    r1, n1 = 2, R - 5           # launch 1 writes b rows [2, 21) from a (the wrap)
    r2, n2 = r1 + k, n1 - 2 * k  # launch 2 writes a rows that depend on exactly those rows of b
    assert _call(G, kind, k, dw, ptrs(a, b), R, Wd, pitch, r1, n1, 3, rule, None, st) == 0
    assert _call(G, kind, k, dw, ptrs(b, a), R, Wd, pitch, r2, n2, 4, rule, slots.data_ptr(), st) == 0
    torch.cuda.synchronize()
    assert error_word(G) == (0, 0)
    t1, t2 = S.stepped(seed, R, Wd, rule, k), S.expected(t0, 0, R, 2 * k, rule)
    want_b = np.full_like(a_host, S.SENT)
    want_b[g + r1:g + r1 + n1, :Wd] = pack(t1[r1:r1 + n1])
    want_a = a_host.copy()
    want_a[g + r2:g + r2 + n2, :Wd] = pack(t2[r2:r2 + n2])
    assert np.array_equal(_host(b), want_b)
    assert np.array_equal(_host(a), want_a)
    assert int(slots.sum().item()) == S.COUNT_SEED[1] + int(t2[r2:r2 + n2].sum())


# ------------------------------------------------------------------ refusals
def _call_entry(G, kind, ptr, a, slots, stream):
    """The entry of `kind` with the arguments a (S.refusal_args: cells_per_lane, layout and masks as given)."""
    lib = G.lib()
    p = [None if a[n] == 0 else ptr[n] + (a[n] - S.P) for n in ("top", "mid", "bot", "dst")]
    head = (*p, a["R"], a["Wd"], a["pitch"], a["row0"], a["rows"], a["k"])
    if kind in ("bits", "band"):
        return getattr(lib, f"gol_dev_{kind}_step")(*head, a["cells_per_lane"], 0, slots, stream)
    return lib.gol_dev_rule_step(*head, a["layout"], a["birth"], a["survive"], a["cells_per_lane"], 0, slots, stream)


@pytest.mark.parametrize("kind", ["bits", "band", "rule_std", "rule_band"])
def test_refusals_launch_nothing(G, kind):
    import torch
    good = S.refusal_args(kind, {})
    k, R, Wd, pitch, g = good["k"], good["R"], good["Wd"], good["pitch"], S.GUARD
    assert (k, R, Wd, pitch) == (4, 20, 8, 16)
    src = _dev(np.full((R + 2 * g, pitch), 0xFFFFFFFF, dtype=np.uint32))  # all alive: a launch would write zeros
    dst = _dev(np.full((R + 2 * g, pitch), S.SENT, dtype=np.uint32))
    slots = _slots(G)
    mid = src.data_ptr() + 4 * g * pitch
    ptr = {"top": mid + 4 * (R - k) * pitch, "mid": mid, "bot": mid, "dst": dst.data_ptr() + 4 * g * pitch}
    st = torch.cuda.current_stream().cuda_stream
    bad = [b for name, b, _, via in S.refusals() if name == kind and via == "entry"]
    assert len(bad) >= 12
    for b in bad:
        rc = _call_entry(G, kind, ptr, S.refusal_args(kind, b), slots.data_ptr(), st)
        assert rc == G._lib.GOL_EINVAL, (kind, b)
    torch.cuda.synchronize()
    assert error_word(G) == (0, 0)
    assert bool((_host(dst) == S.SENT).all()) and int(slots.sum().item()) == S.COUNT_SEED[1]
    # and the call they were derived from is a good one
    assert _call_entry(G, kind, ptr, good, slots.data_ptr(), st) == 0
    torch.cuda.synchronize()
    assert error_word(G) == (0, 0)
    out = _host(dst)
    assert bool((out[g:g + R, :Wd] == 0).all()) and bool((out[:, Wd:] == S.SENT).all())
    assert int(slots.sum().item()) == S.COUNT_SEED[1]
