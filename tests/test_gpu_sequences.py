"""The board engine against its model, call by call (tests/engine_model.py): seeded random sequences
of public calls run on a real engine and on the numpy model, every returned value compared exactly
and the whole board compared in place (check_board: a full view at scale 1, the alive count, the
turn; never store_bytes, which would convert the layout) after half of the calls.  What is under
test is the state the calls leave for one another -- layout, halo, pending counts, the exact first
turn -- not any one kernel: every shape here is exercised singly elsewhere.

| id    | engine                                      | board     | what it reaches |
| band1 | layout="band"                               | 48 x 1024 | one shard reading its own wrap rows, k = 12 pipeline, band <-> standard |
| band3 | layout="band", shards=3, same_device=True   | 80 x 2048 | uneven shards, loopback halo, edge / interior plans, edits across seams |
| std2  | layout="standard", shards=2, same_device    | 50 x 192  | standard rows, funnel-shift reads, k up to 16 |
| bytes | layout="bytes"                              | 40 x 128  | byte pipeline k = 32 with a blocked-kernel tail, 0/255 tracking |
| w32   | default                                     | 36 x 96   | W % 64 == 32: byte board, k-turn blocked kernel |
| odd   | default                                     | 33 x 48   | W % 32 != 0: the one-turn scalar kernel only |

The seeds and the length are engine_model.SEEDS and LENGTH; tests/test_engine_model_cpu.py asserts
what they cover.  A failure's message holds config, seed, index, ops and checks as Python: paste them
before `replay(factory(G), config, ops, checks)` to run it again.  GOLHIP_SEQUENCE_LIBRARY names
another build of the library to run the same sequences on (a host-side change under study)."""
import os

import pytest

import engine_model as M
from testlib import gpu_lib as G  # noqa: F401 (the fixture)

pytestmark = pytest.mark.gpu


def factory(G):
    path = os.environ.get("GOLHIP_SEQUENCE_LIBRARY")
    library = G._lib.load(path) if path else None
    return lambda c: G.Engine(c["H"], c["W"], device=0, library=library, **c["engine"])


@pytest.mark.parametrize("cid,seed", [(cid, seed) for cid in M.CONFIGS for seed in M.SEEDS[cid]])
def test_random_sequence(G, cid, seed):
    config = M.CONFIGS[cid]
    M.replay(factory(G), config, M.generate(config, seed, M.LENGTH), M.check_points(seed, M.LENGTH), seed)


# The two orders named when this test was written, as the likeliest to be wrong.
COUNTED_EDIT_COUNT_COUNTED = [
    ("load_random", (7,)),
    ("step_counted", (36, 12)),                   # three fused count points left for one batched reduce
    ("paste", (2030, 20, 60, 14, "xor", 11)),     # rows 20..33 across the seam at row 27, wraps in x
    ("alive_count", ()),                          # slot array 0 and counts[0], which the points shared
    ("step_counted", (25, 12)),                   # the halo is made again; 25 = 12 + 12 + 1
    ("hash", ()),
]
ODD_LOAD_THEN_MIXED_CALLS = [
    ("load_bytes", (5, .4, True)),                # odd bytes: the exact first turn is pending
    ("view", (0, 0, 1, 192, 50)),
    ("load_words", (10, 10, 3)),                  # rows 10..19 only: the rest keeps its 255-cells
    ("step_flips", (None,)),
    ("set_rule", ("B36/S23", False)),
    ("step", (9,)),
    ("copy", (180, 20, 40, 12)),                  # wraps in x, across the seam at row 25
    ("set_rule", ("B3/S23", False)),
    ("step", (13,)),
]


@pytest.mark.parametrize("checks", [False, True])
@pytest.mark.parametrize("cid,ops", [("band3", COUNTED_EDIT_COUNT_COUNTED), ("std2", ODD_LOAD_THEN_MIXED_CALLS)],
                         ids=["counted_edit_count_counted", "odd_load_then_mixed_calls"])
def test_directed_sequence(G, cid, ops, checks):
    """Each once with every call meeting the state exactly as the one before left it, once with the
    board compared in place after every call."""
    M.replay(factory(G), M.CONFIGS[cid], ops, [checks] * len(ops))
