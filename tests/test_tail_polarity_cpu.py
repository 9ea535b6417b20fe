"""Data polarity of the rule circuits: every gate output sparse on a settled board.

The truth tables of gol_device.h are read from the source (the `constexpr unsigned TT_... = 0x..;`
form) and evaluated in the wiring of gol_pipe.h pair_tail / pstage and of gol_device.h rule():
both pair outputs on all 4096 4 x 3 neighbourhoods, the one-row rule on all 512 3 x 3 ones.  Each
gate's output is then weighted by the histogram of a settled soup (tests/golden/nbhd_hist_4x3.json,
written by tools/nbhd_hist.py) and its share of ones must be below one half: a gate that answers 1
on an all-dead neighbourhood puts a nearly all-ones word between nearly all-zero ones in the
VALU's result stream; complements belong in the tables of the gates that read it.  The bound is the
condition itself (the sparser of a signal and its complement), not a tuned figure.  The
plain-operator twin of the one-row circuit (gol_batch.h, the batch's host code) is parsed from its
source and compared gate for gate.
"""
import json
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gol-distributed-final_amd", "csrc")
HIST = os.path.join(ROOT, "tests", "golden", "nbhd_hist_4x3.json")


def _tables():
    text = open(os.path.join(CSRC, "gol_device.h")).read()
    tt = {m.group(1): int(m.group(2), 16) for m in re.finditer(r"constexpr unsigned (TT_\w+) = 0x([0-9A-Fa-f]+);", text)}
    for name in ("TT_XOR3", "TT_MAJ", "TT_G1", "TT_G2", "TT_OUT", "TT_PG1", "TT_PG2", "TT_PG3", "TT_POUT"):
        assert name in tt, name
    return tt


def _gate(tt, a, b, c):
    # v_bitop3_b32 convention: operand 0 -> 0xF0, operand 1 -> 0xCC, operand 2 -> 0xAA
    return (tt >> ((a << 2) | (b << 1) | c)) & 1


def _rows(idx, n):
    """Neighbourhood index -> n rows of 3 cells (bit 3 r + c = row r, column c)."""
    return [[(idx >> (3 * r + c)) & 1 for c in range(3)] for r in range(n)]


def _life(rows):
    n = sum(sum(r) for r in rows) - rows[1][1]
    return 1 if (n == 3 or (rows[1][1] == 1 and n == 2)) else 0


def _pair_signals(T, rows):
    """gol_pipe.h pstage on one column (rows x_2m-2 .. x_2m+1): every gate output by name; the
    tails' gates carry the suffix of their output row (a: row 2m-1, d: row 2m)."""
    h = [sum(r) for r in rows]
    a, b, c, d = [(x & 1, x >> 1) for x in h]
    s = {"h0": c[0], "h1": c[1]}                    # the new row's horizontal sums (xor3 / maj)
    s["k"] = k = b[0] & c[0]
    s["p0"] = p0 = b[0] ^ c[0]
    s["p1"] = p1 = _gate(T["TT_XOR3"], b[1], c[1], k)
    s["p2"] = p2 = _gate(T["TT_MAJ"], b[1], c[1], k)
    for tag, (x0, x1), cell in (("a", a, rows[1][1]), ("d", d, rows[2][1])):
        g1 = _gate(T["TT_PG1"], p0, x0, cell)
        g2 = _gate(T["TT_PG2"], p1, p2, x1)
        g3 = _gate(T["TT_PG3"], p2, cell, g1)
        s["g1_" + tag], s["g2_" + tag], s["g3_" + tag] = g1, g2, g3
        s["out_" + tag] = _gate(T["TT_POUT"], g3, g1, g2)
    return s


def _row_signals(T, rows):
    """gol_device.h rule() on one column (three rows, the centre row's sum includes the cell)."""
    h = [sum(r) for r in rows]
    lo, hi = [x & 1 for x in h], [x >> 1 for x in h]
    s = {"t0": _gate(T["TT_XOR3"], *lo), "k0": _gate(T["TT_MAJ"], *lo),
         "u": _gate(T["TT_XOR3"], *hi), "v": _gate(T["TT_MAJ"], *hi)}
    s["G1"] = _gate(T["TT_G1"], s["t0"], s["k0"], s["v"])
    s["G2"] = _gate(T["TT_G2"], s["u"], s["v"], s["G1"])
    s["out"] = _gate(T["TT_OUT"], s["t0"], rows[1][1], s["G2"])
    return s


@pytest.fixture(scope="module")
def hist():
    with open(HIST) as f:
        return json.load(f)


def test_histogram_file_is_a_settled_soup(hist):
    counts = hist["counts"]
    assert len(counts) == 4096 and all(isinstance(c, int) and c >= 0 for c in counts)
    assert hist["cells"] == hist["height"] * hist["width"] == sum(counts)
    # every position counts its own cell once: bit 4 (row 1, column 1) gives the alive cells
    alive = sum(c for i, c in enumerate(counts) if (i >> 4) & 1)
    assert alive == hist["alive"]
    assert abs(alive / hist["cells"] - hist["density"]) < 1e-6
    assert 0.03 <= hist["density"] <= 0.07
    # a torus: each of the 12 positions of the window sees every cell once
    for bit in range(12):
        assert sum(c for i, c in enumerate(counts) if (i >> bit) & 1) == alive, bit


def test_pair_outputs_on_every_neighbourhood():
    T = _tables()
    for idx in range(4096):
        rows = _rows(idx, 4)
        s = _pair_signals(T, rows)
        assert s["p0"] + 2 * s["p1"] + 4 * s["p2"] == sum(rows[1]) + sum(rows[2])
        assert s["out_a"] == _life(rows[0:3]), idx
        assert s["out_d"] == _life(rows[1:4]), idx


def test_row_rule_on_every_neighbourhood():
    T = _tables()
    for idx in range(512):
        rows = _rows(idx, 3)
        assert _row_signals(T, rows)["out"] == _life(rows), idx


def _fractions(signals, weights):
    total = float(sum(weights))
    frac = {}
    for s, w in zip(signals, weights):
        for name, bit in s.items():
            frac[name] = frac.get(name, 0.0) + bit * w / total
    return frac


def test_every_pair_gate_is_sparse_on_a_settled_board(hist):
    T = _tables()
    frac = _fractions([_pair_signals(T, _rows(i, 4)) for i in range(4096)], hist["counts"])
    print({k: round(v, 3) for k, v in frac.items()})
    dense = {k: round(v, 3) for k, v in frac.items() if not v < 0.5}
    assert not dense, dense


def test_every_row_rule_gate_is_sparse_on_a_settled_board(hist):
    T = _tables()
    w = [0] * 512
    for i, c in enumerate(hist["counts"]):  # the 3 x 3 margin: rows y-1 .. y+1
        w[i & 511] += c
    frac = _fractions([_row_signals(T, _rows(i, 3)) for i in range(512)], w)
    print({k: round(v, 3) for k, v in frac.items()})
    dense = {k: round(v, 3) for k, v in frac.items() if not v < 0.5}
    assert not dense, dense


def test_search_tool_ranks_the_shipped_tables():
    """tools/rule_search_pair.c --hist reports where its SHIPPED tables stand among all assignments
    of the wiring: they are the header's."""
    T = _tables()
    text = open(os.path.join(ROOT, "tools", "rule_search_pair.c")).read()
    m = re.search(r"SHIPPED\[4\] = \{0x(\w+), 0x(\w+), 0x(\w+), 0x(\w+)\}", text)
    assert m and [int(x, 16) for x in m.groups()] == [T["TT_PG1"], T["TT_PG2"], T["TT_PG3"], T["TT_POUT"]]


def _twin_gates(inputs, mask):
    """The plain-operator branch of gol_batch_conway_next (gol_batch.h), evaluated statement by
    statement on Python integers (bit-parallel: one bit per input combination) -> its variables."""
    text = open(os.path.join(CSRC, "gol_batch.h")).read()
    m = re.search(r"gol_batch_conway_next\(.*?#else[^\n]*\n(.*?)#endif", text, re.S)
    assert m, "gol_batch_conway_next's plain-operator branch not found"
    env = dict(inputs)
    for stmt in m.group(1).split(";"):
        stmt = re.sub(r"//[^\n]*", "", stmt).strip()
        if not stmt:
            continue
        stmt = re.sub(r"^const uint32_t\s+", "", stmt)
        stmt = re.sub(r"^return\s+", "ret = ", stmt)
        parts, depth = [""], 0
        for ch in stmt:  # a declaration list: split at the commas outside parentheses
            depth += (ch == "(") - (ch == ")")
            if ch == "," and depth == 0:
                parts.append("")
            else:
                parts[-1] += ch
        for part in parts:
            name, expr = part.split("=", 1)
            assert re.fullmatch(r"[\w\s~&|^()]+", expr), expr
            env[name.strip()] = eval(expr, {"__builtins__": {}}, env) & mask  # noqa: S307 (operators and names only)
    return env


def test_batch_host_twin_equals_the_table_circuit_gate_for_gate():
    """All 2^7 values of (a0, a1, b0, b1, c0, c1, cell), one bit each, don't-cares included."""
    T = _tables()
    names = ("a0", "a1", "b0", "b1", "c0", "c1", "cell")
    n = 1 << len(names)
    mask = (1 << n) - 1
    inputs = {nm: sum(((p >> i) & 1) << p for p in range(n)) for i, nm in enumerate(names)}
    twin = _twin_gates(inputs, mask)

    def g(tt, a, b, c):
        r = 0
        for i in range(8):
            if (tt >> i) & 1:
                r |= (a if i & 4 else ~a) & (b if i & 2 else ~b) & (c if i & 1 else ~c)
        return r & mask
    t0 = g(T["TT_XOR3"], inputs["a0"], inputs["b0"], inputs["c0"])
    k0 = g(T["TT_MAJ"], inputs["a0"], inputs["b0"], inputs["c0"])
    u = g(T["TT_XOR3"], inputs["a1"], inputs["b1"], inputs["c1"])
    v = g(T["TT_MAJ"], inputs["a1"], inputs["b1"], inputs["c1"])
    g1 = g(T["TT_G1"], t0, k0, v)
    g2 = g(T["TT_G2"], u, v, g1)
    out = g(T["TT_OUT"], t0, inputs["cell"], g2)
    for name, want in (("t0", t0), ("k0", k0), ("u", u), ("v", v), ("g1", g1), ("g2", g2), ("ret", out)):
        assert twin[name] == want, name
