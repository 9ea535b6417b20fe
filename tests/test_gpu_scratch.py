"""The region queries' scratch (csrc/gol_frames.cpp: one grow-on-demand device and pinned buffer per
shard for the views, one for the paste, one for the reads): each query small, then past the scratch's
first capacity of 4096 words, then small again, a cut that has the read and the edit scratch live on
one stream, and a step of the board they leave.  Every comparison is exact, against the numpy
references of tests/region_ref.py."""
import numpy as np
import pytest

from oracle import oracle as O
from region_ref import apply_cuts, apply_edits, check_reads, check_view, random_cells, words_of
from testlib import gpu_lib as G  # noqa: F401 (the fixture)

pytestmark = pytest.mark.gpu


def grow_and_shrink(e, cells, layout, small, turn):
    """The queries on engine e, whose board is `cells`; returns the cells they leave."""
    H, W = cells.shape
    (sx, sy, sw, sh), large = small, (5 % W, 3 % H, W, H)
    board = cells.astype(np.uint8) * 255
    for view in [(0, 0, 1, 1, 1), (0, 0, 1, W, min(H, 300)), (W - 1, H - 1, 1, 3, 1)]:
        check_view(e, board, view, layout)
    cells = apply_edits(e, cells, [(sx, sy, sw, sh, "xor", 1), large + ("xor", 2), (sx, sy, sw, sh, "copy", 3)], layout, turn)
    check_reads(e, cells, [small, large, small], layout)
    cells = apply_cuts(e, cells, [large], layout)  # the whole board read and cleared
    assert not cells.any() and e.bounds() == (0, 0, 0, 0, 0)
    return apply_edits(e, cells, [(sx, sy, sw, sh, "or", 4)], layout, turn)


def test_band_scratch_grows_and_is_reused(G):
    """512 x 1024 band: 1024 x 300 pixels are 192000 words of view scratch, 1024 x 512 cells 8192 words
    of staged pattern rows; the small rectangle wraps both axes."""
    H, W = 512, 1024
    cells = random_cells(H, W, 24)
    with G.Engine(H, W, layout="band", device=0) as e:
        e.load_random(11)
        e.step(24)
        cells = grow_and_shrink(e, cells, "band", (1000, 508, 36, 9), 24)
        assert e.info()["layout"] == "band"
        e.step(12)
        assert e.turn == 36 and e.hash() == O.hash_words(O.bits_run(words_of(cells), 12))


@pytest.mark.parametrize("H,W", [(50, 50), (50, 100)])  # one byte per lane; aligned 4-byte words (W % 4 == 0)
def test_bytes_scratch_with_the_largest_rectangle(G, H, W):
    start = (np.random.default_rng(5).random((H, W)) < 0.4).astype(np.uint8) * 255
    with G.Engine(H, W, device=0) as e:
        e.load_bytes(start)
        e.step(5)
        cells = grow_and_shrink(e, O.run(start, 5) != 0, "bytes", (W - 6, H - 4, 36, 9), 5)
        board = cells.astype(np.uint8) * 255
        assert np.array_equal(e.store_bytes(), board)
        e.step(5)
        assert np.array_equal(e.store_bytes(), O.run(board, 5))
