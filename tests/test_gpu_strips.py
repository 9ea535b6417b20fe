"""The pipeline kernels' strip schedules on hardware, one case per mode.

band_pipe_kernel (k = 12) and bytes_pipe_kernel (k = 32) take their rows from a schedule that
depends on the board's shape and on the device (CUs, resident workgroups): small tiles,
explicit strips, round-tiled strips, strips with a tail, and one ranked round, static or
paired (csrc/gol_strips.h; tests/test_strip_plan_cpu.py checks the row arithmetic on the CPU).
gol_dev_band_step_on / gol_dev_bytes_step_k_on schedule a launch as for a smaller device, so
every mode is reached at the smallest board that has it: each case asks gol_strip_plan for
the smallest row count with the mode it is named for, ASSERTS that mode, runs the launch on
a genuinely random board and compares every written row with the oracle, bit for bit.

The shard under test is rows [k, k + R) of a random torus of R + 2k rows, so its ghost rows
are the true neighbour rows of a larger board (k turns of the shard's rows depend on nothing
else): passed in one buffer (contiguous ghost rows) or as separate top / mid / bot buffers,
where a read of `mid` in place of a ghost row would show.  Every case reads the device's
error word afterwards.

Band `plain` (many rounds, no tail) needs >= 512 resident workgroups and a board of several GB
and is left to the CPU test.
"""
import numpy as np
import pytest

from oracle import oracle as O
from testlib import error_word, gpu_lib as G  # noqa: F401 (the fixture)

pytestmark = pytest.mark.gpu

SENT = 0x5A  # every byte of the sentinel
KERNELS = {"band": 12, "bytes": 32}


def _units(kernel, W, pad):
    """(width, pitch) as the kernel's launcher takes them: words (band), cells and bytes (bytes)."""
    return (W // 32, W // 32 + pad) if kernel == "band" else (W, W + pad)


def first_rows(G, kernel, mode, W, cus, slots, lo, hi, step=1, pad=0, row0=0, strip=0, also=lambda info: True):
    """The smallest row count in [lo, hi) (by `step`) whose plan on the pretended device has `mode`."""
    width, pitch = _units(kernel, W, pad)
    for rows in range(lo, hi, step):
        info, _ = G.strip_plan(kernel, rows, row0, width, pitch, cus, slots, strip, records=False)
        if info["mode"] == mode and also(info):
            return rows
    raise AssertionError(f"no {kernel} launch of [{lo}, {hi}) rows x {W} has mode {mode} on {cus} CUs / {slots} slots")


def run_case(G, kernel, mode, W, cus, slots, rows, *, row0=0, below=0, pad=0, separate=False, count=False, strip=0,
             seed=3, real_device=False):
    """One launch of rows [row0, row0 + rows) of a shard of R = row0 + rows + below rows, scheduled
    as for (cus, slots) -- or, real_device, by the plain device with (cus, slots) its own values --
    after asserting that its plan has `mode`; returns the plan's info."""
    import torch
    L, lib = G._lib, G.lib()
    k = KERNELS[kernel]
    R = row0 + rows + below
    H = R + 2 * k
    width, pitch = _units(kernel, W, pad)
    info, recs = G.strip_plan(kernel, rows, row0, width, pitch, cus, slots, strip)
    assert info["mode"] == mode, info
    words = O.mt_random_words(seed, H, W // 64, 16)
    ref = words.copy()
    O.mt_bits_run(ref, k, k, 16)
    want = ref[k + row0:k + row0 + rows]
    st = torch.cuda.current_stream().cuda_stream
    if kernel == "band":
        std = torch.from_numpy(words.view(np.int32).reshape(H, width)).cuda()
        src = torch.full((H, pitch), SENT * 0x01010101, dtype=torch.int32, device="cuda")
        L.check(lib.gol_dev_band_convert(1, std.data_ptr(), src.data_ptr(), H, width, width, pitch, st))
        dst = torch.full((R, pitch), SENT * 0x01010101, dtype=torch.int32, device="cuda")
    else:
        src = torch.full((H, pitch), SENT, dtype=torch.uint8, device="cuda")
        src[:, :W] = torch.from_numpy(O.unpack(words)).cuda()
        dst = torch.full((R, pitch), SENT, dtype=torch.uint8, device="cuda")
    if separate:
        top, mid, bot = src[:k].clone(), src[k:k + R].clone(), src[k + R:].clone()
        del src
    else:
        top, mid, bot = src[:k], src[k:k + R], src[k + R:]
    slots_t = torch.zeros(L.GOL_COUNT_SLOTS * 8, dtype=torch.int64, device="cuda") if count else None
    cptr = slots_t.data_ptr() if count else None
    as_dev = (0, 0) if real_device else (cus, slots)
    if kernel == "band":
        L.check(lib.gol_dev_band_step_on(top.data_ptr(), mid.data_ptr(), bot.data_ptr(), dst.data_ptr(), R, width, pitch,
                                         row0, rows, k, 128, strip, cptr, st, *as_dev))
    else:
        L.check(lib.gol_dev_bytes_step_k_on(top.data_ptr(), mid.data_ptr(), bot.data_ptr(), dst.data_ptr(), R, width,
                                            pitch, row0, rows, k, strip, cptr, st, *as_dev))
    torch.cuda.synchronize()
    assert error_word(G) == (0, 0)
    # the written rows, bit for bit
    out = dst[row0:row0 + rows]
    if kernel == "band":
        got = torch.empty((rows, width), dtype=torch.int32, device="cuda")
        L.check(lib.gol_dev_band_convert(0, out.data_ptr(), got.data_ptr(), rows, width, pitch, width, st))
        torch.cuda.synchronize()
        got = got.cpu().numpy().view(np.uint64)
    else:
        assert bool(((out[:, :W] == 0) | (out[:, :W] == 255)).all())
        got = O.pack(out[:, :W].cpu().numpy())
    bad = np.flatnonzero((got != want).any(axis=1))
    assert bad.size == 0, f"{bad.size} wrong rows of {rows}, first {bad[:8] + row0} (plan {info})"
    # nothing else: the padding of every row and every row outside [row0, row0 + rows)
    fill = SENT * 0x01010101 if kernel == "band" else SENT
    assert bool((dst[:, width if kernel == "band" else W:] == fill).all()), "a row's padding was written"
    assert bool((dst[:row0] == fill).all()) and bool((dst[row0 + rows:] == fill).all()), "rows outside the launch were written"
    if count:
        assert int(slots_t.sum().item()) == O.popcount_words(want)
    return info


# ------------------------------------------------------------------ band pipeline, k = 12
# (mode, W, cus, slots, first row count tried, step): W = 1024 is one column group, 8192 two, 16384 three
BAND_MODES = {
    "small": ("small", 1024, 8, 32, 601, 1),
    "explicit": ("explicit", 1024, 8, 32, 1001, 1),
    "round_tiled": ("round_tiled", 1024, 8, 40, 24577, 1),  # 5 per CU: no ranked round
    "tail": ("tail", 1024, 8, 40, 163841, 1),
    "static_1": ("ranked_static", 1024, 8, 8, 24577, 1),
    "paired_4": ("ranked_paired", 1024, 8, 32, 24577, 1),
    "paired_3": ("ranked_paired", 1024, 8, 24, 24577, 1),
    "paired_2": ("ranked_paired", 1024, 8, 16, 24577, 1),
    "paired_2groups": ("ranked_paired", 8192, 8, 32, 12301, 1),
}
BYTES_MODES = {
    "explicit": ("explicit", 1024, 8, 24, 1001, 1),
    "round_tiled": ("round_tiled", 1024, 8, 24, 301, 1),
    "plain": ("plain", 1024, 8, 8, 16385, 1),
    "static_1": ("ranked_static", 1024, 8, 8, 301, 1),
    "paired_3": ("ranked_paired", 1024, 8, 24, 301, 1),
    "paired_2": ("ranked_paired", 1024, 8, 16, 301, 1),
    "paired_2groups": ("ranked_paired", 3968, 8, 24, 301, 1),
}
VARIANTS = {
    "contiguous": dict(),
    "separate": dict(separate=True),
    "padded": dict(pad=16, separate=True),
    "offset": dict(row0=37, below=29),
    "counted": dict(count=True),
    "all": dict(pad=16, separate=True, row0=37, below=29, count=True),
}


def _case(G, kernel, name, **kw):
    mode, W, cus, slots, lo, step = (BAND_MODES if kernel == "band" else BYTES_MODES)[name]
    strip = 100 if mode == "explicit" else 0
    per_cu = slots // cus

    def also(info):
        if not mode.startswith("ranked"):
            return True
        return info["per_cu"] == min(per_cu, 3 if kernel == "bytes" else 4)
    rows = first_rows(G, kernel, mode, W, cus, slots, lo, lo + (1 << 20), step, pad=kw.get("pad", 0),
                      row0=kw.get("row0", 0), strip=strip, also=also)
    return rows, run_case(G, kernel, mode, W, cus, slots, rows, strip=strip, **kw)


@pytest.mark.parametrize("name", sorted(BAND_MODES))
def test_band_mode(G, name):
    """Every schedule of the band pipeline (128 cells per lane) at the smallest board that has it on
    a pretended 8-CU device: paired at 4, 3 and 2 workgroups per CU (3: the (0, 2) pair and a lone
    rank), the static split at 1, two column groups; contiguous ghost rows, fused count."""
    rows, info = _case(G, "band", name, count=True)
    if name == "paired_3":
        assert info["per_cu"] == 3
    if name == "paired_2groups":
        assert info["ngroups"] == 2


def test_band_ranked_with_idle_cus(G):
    """Three column groups on 64 CUs: 21 ranges per group, one CU has no rows (t * ngroups < cus);
    its workgroups must leave without touching their counters."""
    W, cus, slots = 16384, 64, 256
    rows = first_rows(G, "band", "ranked_paired", W, cus, slots, 4097, 1 << 20)
    info = run_case(G, "band", "ranked_paired", W, cus, slots, rows, count=True)
    assert info["ngroups"] == 3 and (cus // 3) * 3 < cus
    _, recs = G.strip_plan("band", rows, 0, W // 32, W // 32, cus, slots)
    assert int((recs["s0"] >= recs["s1"]).sum()) == info["per_cu"] * (cus - (cus // 3) * 3)


def test_band_tail_with_short_strips(G):
    """The tail whose strips are shorter than the launch's (a quarter of >= 388 rows): a few hundred
    thousand rows at one column group, ~100 MB, so once, with the fused count."""
    W, cus, slots = 1024, 8, 40
    rows = first_rows(G, "band", "tail", W, cus, slots, 163841, 1 << 21, 4099,
                      also=lambda i: 96 < i["tail_strip"] < i["strip"] and (i["tail_row"] % i["strip"]) != 0)
    info = run_case(G, "band", "tail", W, cus, slots, rows, count=True)
    assert 96 < info["tail_strip"] == info["strip"] // 4


@pytest.mark.parametrize("variant", sorted(VARIANTS))
@pytest.mark.parametrize("name", ["paired_4", "static_1", "round_tiled"])
def test_band_variants(G, name, variant):
    """Ghost rows in one buffer or in buffers of their own, a padded pitch (padding and every row
    outside the launch keep their sentinel), row0 > 0 with rows that are no multiple of the period
    or strip, and the fused count: on a paired and on two unpaired schedules."""
    rows, info = _case(G, "band", name, **VARIANTS[variant])
    unit = info["period"] if info["mode"].startswith("ranked") else info["strip"]
    assert rows % unit != 0


# ------------------------------------------------------------------ byte pipeline, k = 32
@pytest.mark.parametrize("name", sorted(BYTES_MODES))
def test_bytes_mode(G, name):
    """Every schedule of the byte pipeline on a pretended 8-CU device: paired at 3 (the (0, 2) pair
    and a lone rank) and 2 workgroups per CU, the static split at 1, two column groups."""
    rows, info = _case(G, "bytes", name, count=True)
    if name == "paired_2groups":
        assert info["ngroups"] == 2


@pytest.mark.parametrize("variant", sorted(VARIANTS))
@pytest.mark.parametrize("name", ["paired_3", "static_1", "round_tiled"])
def test_bytes_variants(G, name, variant):
    rows, info = _case(G, "bytes", name, **VARIANTS[variant])
    unit = info["period"] if info["mode"].startswith("ranked") else info["strip"]
    assert rows % unit != 0


# ------------------------------------------------------------------ both
@pytest.mark.parametrize("kernel", ["band", "bytes"])
def test_real_device_paired(G, kernel):
    """cus = slots = 0: the device's own schedule, at the smallest shape whose plan (from the
    device's CU count and the kernel's resident workgroups, gol_dev_pipe_limits) is paired -- so the
    map the device really runs stays under test when the kernel's occupancy changes."""
    cus, slots = G._lib.pipe_limits(kernel, contiguous=True, counted=True)
    assert cus % 8 == 0 and slots >= cus
    rows = first_rows(G, kernel, "ranked_paired", 1024, cus, slots, 301, 1 << 20, 7)
    info = run_case(G, kernel, "ranked_paired", 1024, cus, slots, rows, count=True, real_device=True)
    assert info["per_cu"] == min(slots // cus, 4 if kernel == "band" else 3)


@pytest.mark.parametrize("kernel,k,count", [("band", 12, False), ("band", 12, True), ("band", 8, False), ("band", 8, True),
                                            ("bytes", 32, False), ("bytes", 8, False)])
def test_plain_entry_is_the_on_entry_with_this_device(G, kernel, k, count):
    """gol_dev_band_step and gol_dev_bytes_step_k write what their _on twins write with cus = slots
    = 0, bit for bit, through the pipeline (band k = 12, bytes k = 32) and through the step kernel
    (k = 8), with the fused count and without: a shard of R rows between k true ghost rows, at the
    smallest shapes the kernels take (band: 24 rows x 4096 cells, 128 cells per lane; bytes: 32
    rows x 64 cells)."""
    import torch
    L, lib = G._lib, G.lib()
    R, W = (24, 4096) if kernel == "band" else (32, 64)
    width, pitch = _units(kernel, W, 0)
    words = O.random_words(5, 0, R + 2 * k, W // 64)
    if kernel == "band":  # (any words are a band board)
        src = torch.from_numpy(words.view(np.int32).reshape(R + 2 * k, width)).cuda()
    else:
        src = torch.from_numpy(O.unpack(words)).cuda()
    st = torch.cuda.current_stream().cuda_stream
    outs = []
    for on in (False, True):
        dst = torch.full((R, pitch), SENT, dtype=src.dtype, device="cuda")
        slots_t = torch.zeros(L.GOL_COUNT_SLOTS * 8, dtype=torch.int64, device="cuda") if count else None
        args = [src[:k].data_ptr(), src[k:k + R].data_ptr(), src[k + R:].data_ptr(), dst.data_ptr(), R, width, pitch, 0, R, k]
        args += ([128] if kernel == "band" else []) + [0, slots_t.data_ptr() if count else None, st] + ([0, 0] if on else [])
        name = ("gol_dev_band_step" if kernel == "band" else "gol_dev_bytes_step_k") + ("_on" if on else "")
        L.check(getattr(lib, name)(*args))
        torch.cuda.synchronize()
        assert error_word(G) == (0, 0)
        outs.append((dst, int(slots_t.sum().item()) if count else None))
    (plain, plain_n), (on, on_n) = outs
    assert bool((plain != SENT).any()), "nothing was written"
    assert torch.equal(plain, on) and plain_n == on_n
    if count:
        assert plain_n > 0


@pytest.mark.parametrize("kernel", ["band", "bytes"])
def test_counter_hand_over(G, kernel):
    """Two paired launches back to back on one stream (ping-pong), then a third paired launch of
    another shape on that stream: each finds the counters its predecessor's pairs zeroed (the
    second finisher of a pair resets them), so all three match the oracle."""
    import torch
    L, lib = G._lib, G.lib()
    k = KERNELS[kernel]
    mode, W, cus, slots, lo, step = (BAND_MODES if kernel == "band" else BYTES_MODES)["paired_3"]
    width, pitch = _units(kernel, W, 0)
    H = first_rows(G, kernel, mode, W, cus, slots, lo, 1 << 20) + 1000
    row0 = 129
    rows3 = first_rows(G, kernel, mode, W, cus, slots, lo, H - row0, row0=row0) + 17
    for rows, r0 in ((H, 0), (rows3, row0)):
        info, _ = G.strip_plan(kernel, rows, r0, width, pitch, cus, slots, records=False)
        assert info["mode"] == "ranked_paired", info
    words = O.random_words(11, 0, H, W // 64)
    if kernel == "band":
        std = torch.from_numpy(words.view(np.int32).reshape(H, width)).cuda()
        a = torch.empty_like(std)
        L.check(lib.gol_dev_band_convert(1, std.data_ptr(), a.data_ptr(), H, width, width, pitch, 0))
    else:
        a = torch.from_numpy(O.unpack(words)).cuda()
    torch.cuda.synchronize()
    b, c = torch.zeros_like(a), torch.zeros_like(a)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        for src, dst, r0, rows in ((a, b, 0, H), (b, c, 0, H), (c, a, row0, rows3)):
            args = (src[H - k:].data_ptr(), src.data_ptr(), src.data_ptr(), dst.data_ptr(), H, width, pitch, r0, rows, k)
            if kernel == "band":
                L.check(lib.gol_dev_band_step_on(*args, 128, 0, None, s.cuda_stream, cus, slots))
            else:
                L.check(lib.gol_dev_bytes_step_k_on(*args, 0, None, s.cuda_stream, cus, slots))
    s.synchronize()
    assert error_word(G) == (0, 0)

    def cells(t, r0, rows):
        t = t[r0:r0 + rows]
        if kernel == "bytes":
            return O.pack(t.cpu().numpy())
        out = torch.empty_like(t)
        L.check(lib.gol_dev_band_convert(0, t.data_ptr(), out.data_ptr(), rows, width, pitch, width, 0))
        torch.cuda.synchronize()
        return out.cpu().numpy().view(np.uint64)
    r1 = O.bits_run(words, k)
    r2 = O.bits_run(r1, k)
    r3 = O.bits_run(r2, k)
    assert np.array_equal(cells(b, 0, H), r1), "first launch"
    assert np.array_equal(cells(c, 0, H), r2), "second launch (the first one's counters)"
    assert np.array_equal(cells(a, row0, rows3), r3[row0:row0 + rows3]), "third launch, another shape"


@pytest.mark.parametrize("kernel", ["band", "bytes"])
def test_pretended_device_arguments(G, kernel):
    """cus % 8 != 0, more CUs than the device has, more resident workgroups than the kernel has
    there, one of the two left 0, and a k that is not the pipeline's: GOL_EINVAL, nothing launched."""
    import torch
    L, lib = G._lib, G.lib()
    k = KERNELS[kernel]
    dcus, dslots = L.pipe_limits(kernel, contiguous=False, counted=False)
    H, W = 2000, 1024
    width, pitch = _units(kernel, W, 0)
    a = torch.zeros((H, pitch), dtype=torch.int32 if kernel == "band" else torch.uint8, device="cuda")
    a[::3] = 255 if kernel == "bytes" else 0x01010101
    dst = torch.full_like(a, SENT)

    def launch(cus, slots, kk=k):
        args = (a[H - kk:].data_ptr(), a.data_ptr(), a.data_ptr(), dst.data_ptr(), H, width, pitch, 0, H, kk)
        st = torch.cuda.current_stream().cuda_stream
        if kernel == "band":
            return lib.gol_dev_band_step_on(*args, 128, 0, None, st, cus, slots)
        return lib.gol_dev_bytes_step_k_on(*args, 0, None, st, cus, slots)
    for cus, slots in ((12, 12), (dcus + 8, dcus + 8), (8, dslots + 1), (8, 0), (0, 8), (-8, 8)):
        assert launch(cus, slots) == L.GOL_EINVAL, (cus, slots)
    assert launch(8, 8, 8) == L.GOL_EINVAL  # not the pipelined k
    torch.cuda.synchronize()
    assert bool((dst == SENT).all()), "a refused call launched"
    assert launch(8, 8) == L.GOL_OK and launch(0, 0) == L.GOL_OK and launch(0, 0, 8) == L.GOL_OK
    torch.cuda.synchronize()
    assert error_word(G) == (0, 0)
