"""golhip -- MI355X-native Game-of-Life hot path behind the reference's broker/worker API.

* ``Engine``               one GPU, board resident in HBM (gol_engine_*)
* ``Operations``           broker RPC service mirror (broker.go:62-277)
* ``GameOfLifeOperations`` worker RPC service mirror (worker.go:73-86)
* ``ShardedBoard``         torch.distributed mirror of the sharded step (runs the library's plans)
* ``halo_plan`` / ``step_plan``  the sharded step's schedule as data (gol_halo_plan, gol_step_plan)
* ``strip_plan``           which workgroup of a pipelined launch computes which rows (gol_strip_plan)
* ``Engine.view`` / ``Operations.view``  viewport frames of the running board (gol_engine_view; ``view_plan``)
* ``Engine(rule=)`` / ``Engine.set_rule`` / ``parse_rule`` / ``format_rule``  life-like rules (B/S masks, gol_engine_set_rule)
* ``Engine.paste`` / ``Engine.fill`` / ``Operations.paste`` / ``parse_rle`` / ``format_rle``  edits of the running board in place (gol_engine_paste) and the RLE pattern codec
* ``Engine.copy`` / ``Engine.cut`` / ``Engine.bounds`` / ``Engine.to_rle`` / ``Operations.copy`` / ``Operations.bounds``  exact reads of a region of the running board in place (gol_engine_copy, gol_engine_bounds)
* ``Batch``                many small boards (<= 512 x 512) stepped in one launch, resident in their workgroups, with a settle scan (gol_batch_*)
* ``Batch.islands`` / ``island`` / ``ISLAND_DTYPE``  the island census of every board of a batch, labelled on the GPU: per island a translation-invariant record (gol_batch_islands), and the record of a lone pattern to name it by
* ``symmetry=ISLAND_FREE`` (``ISLAND_FIXED`` the default) on ``Batch.islands``, ``Batch.islands_tally``, ``Batch.census`` and ``island``  the free hash: the smallest of an island's hashes in the eight orientations of the square, computed in the kernel, so a tally holds one line per object however it is turned or mirrored (the _sym entries)
* ``Batch.census`` / ``Batch.islands_tally`` / ``ISLAND_KIND_DTYPE``  the tally of island kinds (kind -> occurrences, with an example soup) of a streamed soup search or of the boards as they stand, built on the GPU inside the search's harvest (gol_batch_census, gol_batch_islands_tally)
* ``Batch(rule="MAP...")`` / ``Batch.set_map`` / ``Batch.set_maps`` / ``Batch.maps`` / ``parse_map`` / ``format_map`` / ``map_from_rule``  MAP rules: any two-state rule of the 3x3 block as a 512-bit table, one for the batch or one per board, under every stepping call of a batch (gol_batch_set_map, gol_batch_set_maps)
* ``distributor``          controller mirror (gol/gol.go + gol/distributor.go) over the broker API
* ``next_state_slab`` / ``partition_rows``  worker.go:15-70 / broker.go:135-206

Everything runs through libgolhip.so (hipcc, gfx950); there is no CPU fallback.
"""
from ._lib import (GolError, device_count, format_map, format_rle, format_rule, halo_plan, lib, map_from_rule,  # noqa: F401
                   parse_map, parse_rle, parse_rule, step_plan, strip_plan, view_plan)
from .batch import ISLAND_DTYPE, ISLAND_FIXED, ISLAND_FREE, ISLAND_KIND_DTYPE, Batch, island  # noqa: F401
from .broker import Operations  # noqa: F401
from .engine import Engine, next_state_slab, partition_rows  # noqa: F401
from .pgm import read_pgm, write_pgm_bytes  # noqa: F401
from .stubs import Cell, CellList, Parameters, Request, Response  # noqa: F401
from .worker import GameOfLifeOperations  # noqa: F401


def sharded_board(*args, **kwargs):
    """Construct a ShardedBoard (imports torch lazily)."""
    from .sharded import ShardedBoard
    return ShardedBoard(*args, **kwargs)
