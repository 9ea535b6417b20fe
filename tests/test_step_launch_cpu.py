"""The check of every step launch (gol_step_launch_ok, csrc/gol_step_launch.h) through its export
gol_step_check_host, without a launch: it accepts the launch of every case of tests/step_ref.py's
table, refuses the shared refusal list (which tests/test_gpu_step_kernels.py and
tests/test_abi_cpu.py run through the gol_dev_* entries), reports the geometry step_ref states, and
has exactly step_ref's kernel table; the same two sets run through the stand-alone program under
ASan/UBSan (build/asan/step_check launch)."""
import ctypes
import subprocess

import pytest

import step_ref as S
from testlib import GOL_EINVAL, check_program, cpu_lib as G  # noqa: F401 (the fixture)

ALLOCS = ("src", "top", "mid", "bot", "dst")


def fake_ptr(alloc):
    """A 16-byte aligned base per allocation, far apart: the check reads no memory."""
    return (1 + ALLOCS.index(alloc)) << 24


def case_args(c, as_entry=1):
    """The arguments of gol_step_check_host (without the geometry) for the launch of case c."""
    ptr = {n: fake_ptr(al) + 4 * off for n, (al, off) in c.pointers().items()}
    birth, survive = S.RR.masks(c.rule)
    return [S.FAMILIES.index(c.kind), ptr["top"], ptr["mid"], ptr["bot"], ptr["dst"], c.R, c.Wd, c.pitch, c.row0, c.rows, c.k,
            c.dw, birth, survive, 0, 0, as_entry]


def named_args(a, as_entry):
    family = 7 if a["family"] is None else S.FAMILIES.index(a["family"])  # (7: no family)
    return [family, a["top"], a["mid"], a["bot"], a["dst"], a["R"], a["Wd"], a["pitch"], a["row0"], a["rows"], a["k"],
            a["words_per_lane"], a["birth"], a["survive"], a["cus"], a["slots"], as_entry]


def check_sets():
    """(accept, refuse): every case's launch, the good calls of the refusal list, the engine-only
    kernel as the engine is checked and a misaligned pointer of the bits family (which has no
    alignment clause); the refusal list and the engine-only kernel as a C entry."""
    accept = [case_args(c) for c in S.CASES]
    accept += [named_args(S.refusal_args(g, {}), e) for g in S.GOOD for e in (0, 1)]
    engine_only = dict(k=12, cells_per_lane=64)
    accept += [named_args(S.refusal_args("twin_band", engine_only), 0)]
    accept += [named_args(S.refusal_args("bits", dict(mid=S.P + 4, dst=S.P + 4)), 1)]
    accept += [named_args(S.refusal_args(g, dict(cus=8, slots=16)), 1) for g in ("twin_band", "twin_bytes")]
    refuse = [named_args(S.refusal_args(g, ch), e) for g, ch, _, _ in S.refusals() for e in (0, 1)
              if not (e == 0 and ch == engine_only)]
    return accept, refuse


def test_the_refusal_list_reaches_every_clause():
    S.check_refusal_coverage()
    with pytest.raises(AssertionError):
        S.check_refusal_coverage([r for r in S.refusals() if r[2] != "mask"])
    # each entry is one change away from a call that is good
    assert all(set(ch) <= set(S.refusal_args(g, {})) for g, ch, _, _ in S.refusals())


def test_the_check_accepts_every_case_and_refuses_the_list(G):
    check = G.lib().gol_step_check_host
    accept, refuse = check_sets()
    assert len(S.CASES) == 1504 and len(accept) == 1504 + 12 + 4 and len(refuse) == 2 * len(S.refusals()) - 1 == 197
    for a in accept:
        assert check(*a, None) == 0, a
    geo = (ctypes.c_int32 * 4)(-1, -1, -1, -1)
    for a in refuse:
        assert check(*a, geo) == GOL_EINVAL, a
    assert list(geo) == [-1] * 4  # a refusal writes nothing


def test_the_geometry_is_step_refs(G):
    check = G.lib().gol_step_check_host
    geo = (ctypes.c_int32 * 4)()
    for c in S.CASES:
        assert check(*case_args(c), geo) == 0
        U = S.useful_words(c.inst)
        contig = c.contiguous({al: fake_ptr(al) // 4 for al in ALLOCS})
        assert list(geo) == [U, -(-c.Wd // U), int(contig), 0], c.id
        if c.band:
            assert contig == (c.form == "contig")
    for g, pipelined in (("twin_band", 1), ("twin_bytes", 1), ("bits", 0)):
        a = S.refusal_args(g, {})
        assert check(*named_args(a, 1), geo) == 0
        family, k, dw = a["family"], a["k"], a["words_per_lane"]
        U = S.useful_words((family, k, dw))
        words = a["Wd"] // 32 if family == "bytes" else a["Wd"]
        assert list(geo) == [U, -(-words // U), 0, pipelined]
    assert S.useful_words(("band", 12, 4)) == 232 and S.useful_words(("bytes", 32, 1)) == 62


def test_the_table_is_step_refs(G):
    """k in 1..33 and 1..4 words per lane of every family: the check accepts exactly step_ref's
    table (as the engine is checked) less the engine-only kernel (as a C entry), and gol_band_max_k
    is the largest k the band entry offers."""
    check, lib = G.lib().gol_step_check_host, G.lib()
    for fi, f in enumerate(S.FAMILIES):
        for dw in (1, 2, 3, 4):
            W = 32 * 12 if f == "bytes" else 12  # whole lanes at every dw
            for k in range(1, 34):
                flags = S.TABLE.get((f, k, dw))
                got = [check(fi, S.P, S.P, S.P, S.P, 40, W, W, 0, 40, k, dw, 0, 0, 0, 0, e, None) == 0 for e in (0, 1)]
                assert got == [flags is not None, flags is not None and "engine_only" not in flags], (f, k, dw)
    for cpl, dw in ((0, 4), (64, 2), (128, 4), (32, 0), (96, 0), (256, 0)):
        assert S.words_per_lane("band", cpl) == dw
        offered = [k for (f, k, d), fl in S.TABLE.items() if f == "band" and d == dw and "engine_only" not in fl]
        assert lib.gol_band_max_k(cpl) == max(offered, default=0)
    assert lib.gol_band_max_k(64) == 16 and lib.gol_band_max_k(128) == 12


def test_the_check_under_sanitizers(tmp_path):
    """The same two sets through gol_step_launch_ok and the export in the stand-alone program:
    a line per launch, the expected answer first, NULL as 0."""
    accept, refuse = check_sets()
    path = tmp_path / "launches.txt"
    path.write_text("".join(" ".join(str(int(v)) for v in [ok] + a) + "\n"
                            for ok, group in ((1, accept), (0, refuse)) for a in group))
    r = subprocess.run([check_program("step_check"), "launch", str(path)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert f"step_check launch: {len(accept)} accepted, {len(refuse)} refused, 0 bad" in r.stdout
