"""ctypes binding of libgolhip.so (include/golhip.h).

The library is the product: it is built in-tree by ``__graft_entry__.build()``
(hipcc, gfx950) next to this file.  There is no fallback -- if the shared
object is missing or fails to load, every entry point raises.
"""
from __future__ import annotations

import ctypes
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libgolhip.so")

GOL_OK = 0
GOL_EINVAL = -1
GOL_EHIP = -2
GOL_ENOMEM = -3
GOL_EIO = -4
GOL_EFORMAT = -5
GOL_ESTATE = -6
GOL_EQUIT = -7
GOL_ECOMM = -8
GOL_COUNT_SLOTS = 256
GOL_RCCL_ID_BYTES = 128
GOL_TIMING_EXCHANGE = 2
GOL_IPC_ID_BYTES = 128
GOL_IPC_MAX_RANKS = 16
GOL_LAYOUT_AUTO, GOL_LAYOUT_STANDARD, GOL_LAYOUT_BAND, GOL_LAYOUT_BYTES = 0, 1, 2, 3
LAYOUTS = {"auto": GOL_LAYOUT_AUTO, "standard": GOL_LAYOUT_STANDARD, "band": GOL_LAYOUT_BAND,
           "bytes": GOL_LAYOUT_BYTES}
GOL_TRANSPORT_AUTO, GOL_TRANSPORT_LOOPBACK, GOL_TRANSPORT_RCCL, GOL_TRANSPORT_LOCAL, GOL_TRANSPORT_IPC = 0, 1, 2, 3, 4
TRANSPORTS = {"auto": GOL_TRANSPORT_AUTO, "loopback": GOL_TRANSPORT_LOOPBACK, "rccl": GOL_TRANSPORT_RCCL,
              "ipc": GOL_TRANSPORT_IPC}
TRANSPORT_NAMES = {GOL_TRANSPORT_LOOPBACK: "loopback", GOL_TRANSPORT_RCCL: "rccl", GOL_TRANSPORT_LOCAL: "local",
                   GOL_TRANSPORT_IPC: "ipc"}
GOL_SHARDS_SAME_DEVICE = 1
GOL_STEP_SERIAL, GOL_STEP_EDGE_FIRST, GOL_STEP_OVERLAP = 2, 4, 8
STEP_MODES = {"auto": 0, "serial": GOL_STEP_SERIAL, "edge_first": GOL_STEP_EDGE_FIRST, "overlap": GOL_STEP_OVERLAP}
GOL_HALO_SEND, GOL_HALO_RECV = 0, 1
GOL_LAUNCH_MAIN, GOL_LAUNCH_EDGE = 0, 1
VIEW_LAYOUTS = {0: "bytes", 1: "standard", 2: "band"}  # *src_layout of the view calls
GOL_RULE_GENERIC = 1  # gol_engine_set_rule flag: B3/S23 on the rule kernels too
GOL_PASTE_COPY, GOL_PASTE_OR, GOL_PASTE_XOR, GOL_PASTE_ANDNOT = 0, 1, 2, 3
GOL_STRIP_KERNEL_BAND, GOL_STRIP_KERNEL_BYTES = 0, 1
STRIP_KERNELS = {"band": GOL_STRIP_KERNEL_BAND, "bytes": GOL_STRIP_KERNEL_BYTES}
# GOL_FAMILY_*: the step kernels' families (gol_step_check_host)
STEP_FAMILIES = {"bits": 0, "band": 1, "rule_std": 2, "rule_band": 3, "bytes": 4}
# gol_strip_info.mode (GOL_STRIPS_*)
STRIP_MODES = {0: "small", 1: "explicit", 2: "plain", 3: "round_tiled", 4: "tail", 5: "ranked_static",
               6: "ranked_paired"}
GOL_COPY_CUT = 1  # flags of gol_engine_copy / gol_broker_copy
PASTE_OPS = {"copy": GOL_PASTE_COPY, "or": GOL_PASTE_OR, "xor": GOL_PASTE_XOR, "andnot": GOL_PASTE_ANDNOT}

_NAMES = {
    GOL_EINVAL: "EINVAL", GOL_EHIP: "EHIP", GOL_ENOMEM: "ENOMEM", GOL_EIO: "EIO",
    GOL_EFORMAT: "EFORMAT", GOL_ESTATE: "ESTATE", GOL_EQUIT: "EQUIT", GOL_ECOMM: "ECOMM",
}


class GolError(RuntimeError):
    def __init__(self, code: int, message: str):
        super().__init__(f"{_NAMES.get(code, code)}: {message}")
        self.code = code


class gol_config(ctypes.Structure):
    _fields_ = [("device", ctypes.c_int32), ("turns_per_launch", ctypes.c_int32),
                ("strip_rows", ctypes.c_int32), ("cells_per_lane", ctypes.c_int32),
                ("layout", ctypes.c_int32), ("shards", ctypes.c_int32), ("transport", ctypes.c_int32),
                ("flags", ctypes.c_int32)]


class gol_request(ctypes.Structure):
    _fields_ = [("World", ctypes.c_void_p), ("world_stride", ctypes.c_int64),
                ("Turns", ctypes.c_int64), ("ImageHeight", ctypes.c_int64),
                ("ImageWidth", ctypes.c_int64), ("Threads", ctypes.c_int64),
                ("EndY", ctypes.c_int64), ("StartY", ctypes.c_int64), ("Worker", ctypes.c_int64)]


class gol_response(ctypes.Structure):
    _fields_ = [("Alive", ctypes.c_void_p), ("alive_cap", ctypes.c_int64),
                ("alive_len", ctypes.c_int64), ("AliveCount", ctypes.c_int64),
                ("TurnsCompleted", ctypes.c_int64), ("World", ctypes.c_void_p),
                ("world_stride", ctypes.c_int64), ("WorkSlice", ctypes.c_void_p),
                ("work_stride", ctypes.c_int64), ("Worker", ctypes.c_int64)]


# int (*gol_write_fn)(void *user, int64_t offset, const uint8_t *data, int64_t len)
GOL_WRITE_FN = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_int64)


class gol_halo_op(ctypes.Structure):
    _fields_ = [("kind", ctypes.c_int32), ("peer", ctypes.c_int32), ("row", ctypes.c_int64), ("rows", ctypes.c_int64)]


class gol_launch(ctypes.Structure):
    _fields_ = [("stream", ctypes.c_int32), ("needs_halo", ctypes.c_int32), ("row0", ctypes.c_int64),
                ("rows", ctypes.c_int64)]


class gol_view_run(ctypes.Structure):
    _fields_ = [("row", ctypes.c_int64), ("rows", ctypes.c_int64), ("vrow", ctypes.c_int64)]


class gol_strip_info(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int32) for n in ("mode", "ngroups", "strip", "K", "RPB", "NS", "per_cu", "period",
                                               "tail_first", "tail_row", "tail_strip", "reserved")]


class gol_strip_rec(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int32) for n in ("group", "s0", "s1", "dir", "claim", "s1e", "nclaim")]


_i64 = ctypes.c_int64
_i32 = ctypes.c_int32
_u64 = ctypes.c_uint64
_vp = ctypes.c_void_p
_P = ctypes.POINTER

# (name, restype, argtypes) -- one row per declaration in include/golhip.h
SIGNATURES = [
    ("gol_abi_version", ctypes.c_int, []),
    ("gol_last_error", ctypes.c_char_p, []),
    ("gol_device_count", ctypes.c_int, [_P(ctypes.c_int)]),
    ("gol_next_state_slab", ctypes.c_int, [_vp, _i64, _i64, _i64, _i64, _i64, _vp, _i64]),
    ("gol_partition_rows", ctypes.c_int, [_i64, _i64, _i64, _P(_i64), _P(_i64)]),
    ("gol_engine_create", ctypes.c_int, [_i64, _i64, _P(gol_config), _P(_vp)]),
    ("gol_rccl_unique_id", ctypes.c_int, [_vp, _i64]),
    ("gol_ipc_unique_id", ctypes.c_int, [_vp, _i64]),
    ("gol_engine_create_rank", ctypes.c_int, [_i64, _i64, _i32, _i32, _vp, _P(gol_config), _P(_vp)]),
    ("gol_engine_destroy", None, [_vp]),
    ("gol_engine_topology", ctypes.c_int, [_vp, _P(_i32), _P(_i32), _P(_i32), _P(_i32)]),
    ("gol_engine_shard", ctypes.c_int, [_vp, _i32, _P(_i32), _P(_i64), _P(_i64)]),
    ("gol_engine_load_bytes", ctypes.c_int, [_vp, _vp, _i64]),
    ("gol_engine_load_pgm", ctypes.c_int, [_vp, ctypes.c_char_p]),
    ("gol_engine_load_random", ctypes.c_int, [_vp, _u64]),
    ("gol_engine_step", ctypes.c_int, [_vp, _i64]),
    ("gol_engine_step_counted", ctypes.c_int, [_vp, _i64, _i64, _vp, _i64]),
    ("gol_engine_turn", ctypes.c_int, [_vp, _P(_i64)]),
    ("gol_engine_alive_count", ctypes.c_int, [_vp, _P(_u64)]),
    ("gol_engine_store_bytes", ctypes.c_int, [_vp, _vp, _i64]),
    ("gol_engine_store_rows", ctypes.c_int, [_vp, _i64, _i64, _vp, _i64]),
    ("gol_engine_alive_cells", ctypes.c_int, [_vp, _vp, _i64, _P(_i64)]),
    ("gol_engine_step_flips", ctypes.c_int, [_vp, _vp, _i64, _P(_i64)]),
    ("gol_engine_write_pgm", ctypes.c_int, [_vp, ctypes.c_char_p]),
    ("gol_engine_write_pgm_to", ctypes.c_int, [_vp, _vp, _vp]),
    ("gol_engine_load_words", ctypes.c_int, [_vp, _i64, _i64, _vp, _i64]),
    ("gol_engine_store_words", ctypes.c_int, [_vp, _i64, _i64, _vp, _i64]),
    ("gol_engine_hash", ctypes.c_int, [_vp, _P(_u64)]),
    ("gol_engine_info", ctypes.c_int, [_vp, _P(_i32), _P(_i32), _P(_i32), _P(_i32)]),
    ("gol_engine_device_bits", ctypes.c_int, [_vp, _P(_vp), _P(_i64)]),
    ("gol_engine_set_timing", ctypes.c_int, [_vp, _i32]),
    ("gol_engine_timing", ctypes.c_int, [_vp, _P(_i64), _P(ctypes.c_double), _P(ctypes.c_double)]),
    ("gol_engine_exchange_timing", ctypes.c_int, [_vp, _P(_i64), _P(ctypes.c_double)]),
    ("gol_engine_exchange_split", ctypes.c_int, [_vp, _P(_i64), _P(ctypes.c_double), _P(ctypes.c_double)]),
    ("gol_engine_view_counts", ctypes.c_int, [_vp, _i64, _i64, _i32, _i32, _i32, _vp, _i64, _P(_i32)]),
    ("gol_engine_view", ctypes.c_int, [_vp, _i64, _i64, _i32, _i32, _i32, _vp, _i64, _P(_i32)]),
    ("gol_rule_parse", ctypes.c_int, [ctypes.c_char_p, _P(ctypes.c_uint32), _P(ctypes.c_uint32)]),
    ("gol_rule_format", ctypes.c_int, [ctypes.c_uint32, ctypes.c_uint32, ctypes.c_char_p, _i64]),
    ("gol_rule_eval_host", ctypes.c_int, [ctypes.c_uint32, ctypes.c_uint32, _P(ctypes.c_uint32), ctypes.c_uint32,
                                          _P(ctypes.c_uint32)]),
    ("gol_engine_set_rule", ctypes.c_int, [_vp, ctypes.c_uint32, ctypes.c_uint32, _i32]),
    ("gol_engine_rule", ctypes.c_int, [_vp, _P(ctypes.c_uint32), _P(ctypes.c_uint32), _P(_i32)]),
    ("gol_engine_paste", ctypes.c_int, [_vp, _i64, _i64, _i64, _i64, _vp, _i64, _i32, _P(_i64), _P(_i32)]),
    ("gol_paste_host", ctypes.c_int, [_i32, _vp, _i64, _i64, _i64, _i64, _i64, _i64, _i64, _vp, _i64, _i32, _P(_i64)]),
    ("gol_engine_copy", ctypes.c_int, [_vp, _i64, _i64, _i64, _i64, _vp, _i64, _i32, _P(_i64), _P(_i32)]),
    ("gol_engine_bounds", ctypes.c_int, [_vp, _i64, _i64, _i64, _i64, _P(_i64), _P(_i64), _P(_i64), _P(_i64), _P(_i64), _P(_i32)]),
    ("gol_copy_host", ctypes.c_int, [_i32, _vp, _i64, _i64, _i64, _i64, _i64, _i64, _i64, _vp, _i64, _P(_i64)]),
    ("gol_bounds_host", ctypes.c_int, [_i32, _vp, _i64, _i64, _i64, _i64, _i64, _i64, _P(_i64), _P(_i64), _P(_i64), _P(_i64), _P(_i64)]),
    ("gol_rle_parse", ctypes.c_int, [ctypes.c_char_p, _i64, _P(_i64), _P(_i64), _vp, _i64, _i64, ctypes.c_char_p, _i64]),
    ("gol_rle_format", ctypes.c_int, [_vp, _i64, _i64, _i64, ctypes.c_char_p, ctypes.c_char_p, _i64, _P(_i64)]),
    ("gol_batch_create", ctypes.c_int, [_i64, _i64, _i64, _i32, _i32, _P(_vp)]),
    ("gol_batch_destroy", None, [_vp]),
    ("gol_batch_info", ctypes.c_int, [_vp, _P(_i64), _P(_i64), _P(_i64), _P(_i32), _P(_i32), _P(_i32), _P(_i32)]),
    ("gol_batch_set_rule", ctypes.c_int, [_vp, ctypes.c_uint32, ctypes.c_uint32]),
    ("gol_batch_rule", ctypes.c_int, [_vp, _P(ctypes.c_uint32), _P(ctypes.c_uint32)]),
    ("gol_batch_set_rules", ctypes.c_int, [_vp, _i64, _i64, _vp, _vp]),
    ("gol_batch_rules", ctypes.c_int, [_vp, _i64, _i64, _vp, _vp]),
    ("gol_batch_load_words", ctypes.c_int, [_vp, _i64, _i64, _vp, _i64, _i64]),
    ("gol_batch_store_words", ctypes.c_int, [_vp, _i64, _i64, _vp, _i64, _i64]),
    ("gol_batch_load_random", ctypes.c_int, [_vp, _u64]),
    ("gol_batch_load_soups", ctypes.c_int, [_vp, _u64, _i64]),
    ("gol_batch_search", ctypes.c_int, [_vp, _u64, _i64, _i64, _i64, _vp, _vp, _vp, _vp, _vp]),
    ("gol_batch_step", ctypes.c_int, [_vp, _i64, _vp]),
    ("gol_batch_step_cycles", ctypes.c_int, [_vp, _i64, _vp, _vp]),
    ("gol_batch_run_cycles", ctypes.c_int, [_vp, _i64, _vp, _vp, _vp]),
    ("gol_batch_turn", ctypes.c_int, [_vp, _P(_i64)]),
    ("gol_batch_alive_counts", ctypes.c_int, [_vp, _vp, _i64]),
    ("gol_batch_hashes", ctypes.c_int, [_vp, _vp, _i64]),
    ("gol_batch_step_host", ctypes.c_int, [_i64, _i64, ctypes.c_uint32, ctypes.c_uint32, _vp, _vp, _i64]),
    ("gol_batch_cycles_host", ctypes.c_int, [_i64, _i64, ctypes.c_uint32, ctypes.c_uint32, _vp, _vp, _i64, _i64, _P(_i64), _P(_i64)]),
    ("gol_batch_run_cycles_host", ctypes.c_int, [_i64, _i64, ctypes.c_uint32, ctypes.c_uint32, _vp, _vp, _i64, _i64, _i64, _P(_i64),
                                                 _P(_i64), _P(_i64)]),
    ("gol_batch_soup_host", ctypes.c_int, [_i64, _i64, _u64, _i64, _vp, _i64]),
    ("gol_batch_search_host", ctypes.c_int, [_i64, _i64, ctypes.c_uint32, ctypes.c_uint32, _u64, _i64, _i64, _i64, _i64, _i64, _vp,
                                             _vp, _vp, _vp]),
    ("gol_batch_verdict_host", ctypes.c_int, [_i64, _i64, _i64]),
    ("gol_batch_step_check_host", ctypes.c_int, [_vp, _vp, _vp, _i64, _i64, _i64, _i32, _i64, _i32, _i32, ctypes.c_uint32,
                                                 ctypes.c_uint32, _vp, _i32, _i64, _vp, _vp, _i64, _vp, _vp]),
    # MAP rules of a batch (probed by symbol: a library without them still binds with strict=False)
    ("gol_map_parse", ctypes.c_int, [ctypes.c_char_p, _vp]),
    ("gol_map_format", ctypes.c_int, [_vp, ctypes.c_char_p, _i64]),
    ("gol_map_from_rule_host", ctypes.c_int, [ctypes.c_uint32, ctypes.c_uint32, _vp]),
    ("gol_map_eval_host", ctypes.c_int, [_vp, _vp, _P(ctypes.c_uint32)]),
    ("gol_batch_step_map_host", ctypes.c_int, [_i64, _i64, _vp, _vp, _vp, _i64, _i64]),
    ("gol_batch_set_map", ctypes.c_int, [_vp, _vp]),
    ("gol_batch_set_maps", ctypes.c_int, [_vp, _i64, _i64, _vp]),
    ("gol_batch_maps", ctypes.c_int, [_vp, _i64, _i64, _vp]),
    ("gol_batch_step_map_check_host", ctypes.c_int, [_vp, _vp, _vp, _i64, _i64, _i64, _i32, _i64, _i32, _i32, _vp, _i32, _i32, _i64,
                                                     _vp, _vp, _i64, _vp, _vp]),
    ("gol_batch_islands", ctypes.c_int, [_vp, _i64, _i64, _i32, _i64, _vp, _vp, _vp]),
    ("gol_batch_islands_host", ctypes.c_int, [_i64, _i64, _i32, _vp, _i64, _i64, _vp, _vp, _vp]),
    ("gol_batch_islands_check_host", ctypes.c_int, [_vp, _i64, _i64, _i64, _i32, _i64, _vp, _vp, _vp]),
    ("gol_batch_census", ctypes.c_int, [_vp, _u64, _i64, _i64, _i64, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _vp, _vp]),
    ("gol_batch_islands_tally", ctypes.c_int, [_vp, _i64, _i64, _i32, _vp, _vp, _vp, _i64, _vp]),
    ("gol_island_tally_host", ctypes.c_int, [_vp, _vp, _i64, _vp, _i64, _vp]),
    ("gol_batch_census_host", ctypes.c_int, [_i64, _i64, ctypes.c_uint32, ctypes.c_uint32, _u64, _i64, _i64, _i64, _i64, _i64, _i32,
                                             _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _vp]),
    ("gol_island_tally_home_host", _i64, [_u64, _i32]),
    ("gol_batch_islands_tally_check_host", ctypes.c_int, [_vp, _i64, _i64, _i64, _i32, _vp, _vp, _i64, _vp, _i64, _vp, _vp, _vp, _i32,
                                                          _vp]),
    # the _sym siblings: symmetry (GOL_ISLAND_FIXED / GOL_ISLAND_FREE) after reach
    ("gol_batch_islands_sym", ctypes.c_int, [_vp, _i64, _i64, _i32, _i32, _i64, _vp, _vp, _vp]),
    ("gol_batch_islands_tally_sym", ctypes.c_int, [_vp, _i64, _i64, _i32, _i32, _vp, _vp, _vp, _i64, _vp]),
    ("gol_batch_census_sym", ctypes.c_int, [_vp, _u64, _i64, _i64, _i64, _i32, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _vp,
                                            _vp]),
    ("gol_batch_islands_sym_host", ctypes.c_int, [_i64, _i64, _i32, _i32, _vp, _i64, _i64, _vp, _vp, _vp]),
    ("gol_batch_census_sym_host", ctypes.c_int, [_i64, _i64, ctypes.c_uint32, ctypes.c_uint32, _u64, _i64, _i64, _i64, _i64, _i64,
                                                 _i32, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _vp]),
    ("gol_batch_islands_sym_check_host", ctypes.c_int, [_vp, _i64, _i64, _i64, _i32, _i32, _i64, _vp, _vp, _vp]),
    ("gol_batch_islands_tally_sym_check_host", ctypes.c_int, [_vp, _i64, _i64, _i64, _i32, _i32, _vp, _vp, _i64, _vp, _i64, _vp, _vp,
                                                              _vp, _i32, _vp]),
    ("gol_island_orient_host", _u64, [_u64, _i32, _i32]),
    ("gol_step_check_host", ctypes.c_int, [_i32, _vp, _vp, _vp, _vp, _i64, _i64, _i64, _i64, _i64, _i32, _i32, ctypes.c_uint32,
                                           ctypes.c_uint32, _i32, _i32, _i32, _vp]),
    ("gol_halo_plan", ctypes.c_int, [_i64, _i32, _i32, _i32, _P(gol_halo_op), _i32, _P(_i32)]),
    ("gol_step_plan", ctypes.c_int, [_i64, _i32, _i32, _i32, _P(gol_launch), _i32, _P(_i32)]),
    ("gol_view_plan", ctypes.c_int, [_i64, _i32, _i32, _i64, _i64, _P(gol_view_run), _i32, _P(_i32)]),
    ("gol_strip_plan", ctypes.c_int,
     [_i32, _i64, _i64, _i64, _i64, _i32, _i32, _i32, _i32, _P(gol_strip_info), _vp, _i64, _P(_i64)]),
    ("gol_dev_bits_step", ctypes.c_int,
     [_vp, _vp, _vp, _vp, _i64, _i64, _i64, _i64, _i64, _i32, _i32, _i32, _vp, _vp]),
    ("gol_dev_random_fill", ctypes.c_int, [_vp, _i64, _i64, _i64, _i64, _u64, _vp]),
    ("gol_dev_popcount", ctypes.c_int, [_vp, _i64, _i64, _i64, _vp, _vp]),
    ("gol_dev_hash", ctypes.c_int, [_vp, _i64, _i64, _i64, _i64, _vp, _vp]),
    ("gol_dev_pack", ctypes.c_int, [_vp, _i64, _i64, _i64, _vp, _i64, _vp, _vp]),
    ("gol_dev_unpack", ctypes.c_int, [_vp, _i64, _i64, _i64, _vp, _i64, _vp]),
    ("gol_dev_bytes_step", ctypes.c_int, [_vp, _i64, _i64, _i64, _i64, _i64, _vp, _i64, _vp]),
    ("gol_dev_bytes_step_k", ctypes.c_int,
     [_vp, _vp, _vp, _vp, _i64, _i64, _i64, _i64, _i64, _i32, _i32, _vp, _vp]),
    ("gol_dev_band_step", ctypes.c_int,
     [_vp, _vp, _vp, _vp, _i64, _i64, _i64, _i64, _i64, _i32, _i32, _i32, _vp, _vp]),
    ("gol_dev_band_step_on", ctypes.c_int,
     [_vp, _vp, _vp, _vp, _i64, _i64, _i64, _i64, _i64, _i32, _i32, _i32, _vp, _vp, _i32, _i32]),
    ("gol_dev_bytes_step_k_on", ctypes.c_int,
     [_vp, _vp, _vp, _vp, _i64, _i64, _i64, _i64, _i64, _i32, _i32, _vp, _vp, _i32, _i32]),
    ("gol_dev_pipe_limits", ctypes.c_int, [_i32, _i32, _i32, _P(_i32), _P(_i32)]),
    ("gol_dev_rule_step", ctypes.c_int,
     [_vp, _vp, _vp, _vp, _i64, _i64, _i64, _i64, _i64, _i32, _i32, ctypes.c_uint32, ctypes.c_uint32, _i32, _i32, _vp,
      _vp]),
    ("gol_band_max_k", ctypes.c_int, [_i32]),
    ("gol_dev_band_convert", ctypes.c_int, [_i32, _vp, _vp, _i64, _i64, _i64, _i64, _vp]),
    ("gol_dev_batch_retire", ctypes.c_int, [_vp, _vp, _vp, _i64, _i64, _i64, _i64, _vp, _vp, _vp, _vp]),
    ("gol_dev_batch_restock", ctypes.c_int, [_vp, _vp, _vp, _vp, _vp, _i64, _i64, _i64, _i64, _vp, _vp, _vp, _vp]),
    ("gol_dev_batch_step", ctypes.c_int, [_vp, _vp, _vp, _i64, _i64, _i64, _i32, _i64, _i32, _i32, ctypes.c_uint32,
                                          ctypes.c_uint32, _vp, _i32, _i64, _vp, _vp, _i64, _vp, _vp, _vp]),
    ("gol_dev_batch_step_map", ctypes.c_int, [_vp, _vp, _vp, _i64, _i64, _i64, _i32, _i64, _i32, _i32, _vp, _i32, _i32, _i64, _vp,
                                              _vp, _i64, _vp, _vp, _vp]),
    ("gol_dev_batch_islands", ctypes.c_int, [_vp, _i64, _i64, _i64, _i32, _i64, _vp, _vp, _vp, _vp]),
    ("gol_dev_batch_islands_tally", ctypes.c_int, [_vp, _i64, _i64, _i64, _i32, _vp, _vp, _i64, _vp, _i64, _vp, _vp, _vp, _i32, _vp,
                                                   _vp]),
    ("gol_dev_island_table_clear", ctypes.c_int, [_vp, _i32, _vp, _vp]),
    ("gol_dev_batch_islands_sym", ctypes.c_int, [_vp, _i64, _i64, _i64, _i32, _i32, _i64, _vp, _vp, _vp, _vp]),
    ("gol_dev_batch_islands_tally_sym", ctypes.c_int, [_vp, _i64, _i64, _i64, _i32, _i32, _vp, _vp, _i64, _vp, _i64, _vp, _vp, _vp,
                                                       _i32, _vp, _vp]),
    ("gol_dev_error", ctypes.c_int, [_i32, _P(ctypes.c_uint32)]),
    ("gol_broker_create", ctypes.c_int, [_P(gol_config), _P(_vp)]),
    ("gol_broker_destroy", None, [_vp]),
    ("gol_broker_run", ctypes.c_int, [_vp, _P(gol_request), _P(gol_response)]),
    ("gol_broker_retrieve", ctypes.c_int, [_vp, _P(gol_request), _P(gol_response)]),
    ("gol_broker_pause", ctypes.c_int, [_vp]),
    ("gol_broker_quit", ctypes.c_int, [_vp]),
    ("gol_broker_superquit", ctypes.c_int, [_vp]),
    ("gol_broker_paused", ctypes.c_int, [_vp, _P(_i32)]),
    ("gol_broker_view", ctypes.c_int, [_vp, _i64, _i64, _i32, _i32, _i32, _vp, _i64, _P(_i64), _P(_i32)]),
    ("gol_broker_paste", ctypes.c_int, [_vp, _i64, _i64, _i64, _i64, _vp, _i64, _i32, _P(_i64), _P(_i64)]),
    ("gol_broker_copy", ctypes.c_int, [_vp, _i64, _i64, _i64, _i64, _vp, _i64, _i32, _P(_i64), _P(_i64)]),
    ("gol_broker_bounds", ctypes.c_int, [_vp, _i64, _i64, _i64, _i64, _P(_i64), _P(_i64), _P(_i64), _P(_i64), _P(_i64), _P(_i64)]),
    ("gol_worker_update", ctypes.c_int, [_P(gol_request), _P(gol_response)]),
]

_lib = None


def _one_hip_runtime():
    """libgolhip.so links ROCm's libamdhip64.so.7; PyTorch ships its own copy with the same soname.
    The first one loaded serves the whole process, and torch's GPU initialisation fails on the
    other one, so torch (when installed) is loaded first: then both use torch's runtime (the two
    are ABI-compatible: every GPU test passes torch tensors to the library)."""
    try:
        import torch  # noqa: F401
    except ImportError:
        pass


def load(path: str, strict: bool = True):
    """Bind the C ABI of the shared object at `path` (raises if it is missing).  strict=False
    (same-box A/B builds of older revisions, tools/ab.py) skips entry points it lacks."""
    _one_hip_runtime()
    if not os.path.exists(path):
        raise GolError(GOL_ESTATE, f"{path} is missing: run __graft_entry__.build() "
                                   "(hipcc --offload-arch=gfx950); there is no CPU fallback")
    L = ctypes.CDLL(path)
    for name, res, args in SIGNATURES:
        if not strict and not hasattr(L, name):
            continue
        fn = getattr(L, name)
        fn.restype = res
        fn.argtypes = args
    return L


def lib():
    """libgolhip.so, the product library (built in-tree next to this file)."""
    global _lib
    if _lib is None:
        _lib = load(LIB_PATH)
    return _lib


def check(rc: int) -> None:
    if rc != GOL_OK:
        raise GolError(rc, lib().gol_last_error().decode(errors="replace"))


def halo_plan(H: int, nranks: int, rank: int, k: int) -> list[tuple[str, int, int, int]]:
    """gol_halo_plan: the halo exchange of `rank` in issue order, as (kind "send"/"recv", peer,
    first shard-local row, rows).  Host code: no GPU needed."""
    ops = (gol_halo_op * 4)()
    n = ctypes.c_int32()
    check(lib().gol_halo_plan(H, nranks, rank, k, ops, 4, ctypes.byref(n)))
    return [("send" if o.kind == GOL_HALO_SEND else "recv", o.peer, o.row, o.rows) for o in ops[:n.value]]


def step_plan(R: int, k: int, kx: int, mode: str = "overlap") -> list[tuple[str, bool, int, int]]:
    """gol_step_plan: the launches of one k-turn step of an R-row shard in launch order, as
    (stream "main"/"edge", needs_halo, first output row, rows); mode "overlap", "edge_first" or
    "serial"."""
    out = (gol_launch * 3)()
    n = ctypes.c_int32()
    check(lib().gol_step_plan(R, k, kx, STEP_MODES[mode], out, 3, ctypes.byref(n)))
    return [("edge" if L.stream == GOL_LAUNCH_EDGE else "main", bool(L.needs_halo), L.row0, L.rows)
            for L in out[:n.value]]


def view_plan(H: int, nranks: int, rank: int, y0: int, vrows: int) -> list[tuple[int, int, int]]:
    """gol_view_plan: the runs of viewport rows (viewport row v = global row (y0 + v) mod H, v < vrows)
    that shard `rank` holds, as (first shard-local row, rows, first viewport row), in viewport order
    (at most 2: the torus wrap).  Host code: no GPU needed."""
    runs = (gol_view_run * 2)()
    n = ctypes.c_int32()
    check(lib().gol_view_plan(H, nranks, rank, y0, vrows, runs, 2, ctypes.byref(n)))
    return [(r.row, r.rows, r.vrow) for r in runs[:n.value]]


def strip_plan(kernel: str, rows: int, row0: int, width: int, pitch: int, cus: int, slots: int, strip_rows: int = 0,
               k: int | None = None, records: bool = True):
    """gol_strip_plan: the schedule of a pipelined launch (kernel "band": k = 12, width and pitch in
    words; "bytes": k = 32, in cells and bytes) on a device of `cus` CUs holding `slots` resident
    workgroups, as (info, recs): info a dict of gol_strip_info with the mode by name and the
    workgroup count `nwg`, recs a numpy record array (group, s0, s1, dir, claim, s1e, nclaim), one
    record per workgroup id (None with records=False).  Host code: no GPU needed."""
    import numpy as np
    kid = STRIP_KERNELS[kernel]
    k = (12 if kernel == "band" else 32) if k is None else k
    info = gol_strip_info()
    n = ctypes.c_int64()
    check(lib().gol_strip_plan(kid, rows, row0, width, pitch, k, strip_rows, cus, slots, ctypes.byref(info), None, 0,
                               ctypes.byref(n)))
    recs = None
    if records:
        recs = np.zeros(n.value, dtype=np.dtype([(f, "<i4") for f, _ in gol_strip_rec._fields_]))
        check(lib().gol_strip_plan(kid, rows, row0, width, pitch, k, strip_rows, cus, slots, ctypes.byref(info),
                                   recs.ctypes.data, n.value, ctypes.byref(n)))
    d = {f: getattr(info, f) for f, _ in gol_strip_info._fields_ if f != "reserved"}
    d["mode"] = STRIP_MODES[info.mode]
    d["nwg"] = int(n.value)
    return d, recs


def pipe_limits(kernel: str, contiguous: bool = True, counted: bool = False) -> tuple[int, int]:
    """gol_dev_pipe_limits: (CUs, resident workgroups of the pipeline kernel) of the current device."""
    c, n = ctypes.c_int32(), ctypes.c_int32()
    check(lib().gol_dev_pipe_limits(STRIP_KERNELS[kernel], int(contiguous), int(counted), ctypes.byref(c), ctypes.byref(n)))
    return c.value, n.value


def _lib_check(L, rc: int) -> None:
    if rc != GOL_OK:
        raise GolError(rc, L.gol_last_error().decode(errors="replace"))


def parse_rule(text: str, library=None) -> tuple[int, int]:
    """gol_rule_parse: "B36/S23" -> (birth, survive), two 9-bit masks over the neighbour count
    (bit n: exactly n alive neighbours).  Host code: no GPU needed."""
    L = library or lib()
    b, s = ctypes.c_uint32(), ctypes.c_uint32()
    _lib_check(L, L.gol_rule_parse(str(text).encode(), ctypes.byref(b), ctypes.byref(s)))
    return b.value, s.value


def format_rule(birth: int, survive: int, library=None) -> str:
    """gol_rule_format: the canonical text of a rule (upper case, ascending digits)."""
    L = library or lib()
    if not (0 <= birth < 1 << 32 and 0 <= survive < 1 << 32):
        raise GolError(GOL_EINVAL, f"rule masks out of range ({birth}, {survive})")
    buf = ctypes.create_string_buffer(24)
    _lib_check(L, L.gol_rule_format(birth, survive, buf, len(buf)))
    return buf.value.decode()


def _as_map(table) -> "np.ndarray":
    import numpy as np
    a = np.asarray(table)
    if a.shape != (16,) or a.dtype.kind not in "ui" or np.any(a < 0) or np.any(a.astype(np.uint64) >= 1 << 32):
        raise GolError(GOL_EINVAL, f"a map is 16 uint32 words (512 bits), got {a.dtype} {a.shape}")
    return np.ascontiguousarray(a, dtype=np.uint32)


def parse_map(text: str, library=None) -> "np.ndarray":
    """gol_map_parse: "MAP" and 86 base64 characters (with or without "=="), or "B36/S23", -> uint32[16], the
    512-bit table whose bit i = 256 NW + 128 N + 64 NE + 32 W + 16 C + 8 E + 4 SW + 2 S + SE says whether the cell is
    alive next turn.  Host code: no GPU needed."""
    import numpy as np
    L = library or lib()
    m = np.zeros(16, dtype=np.uint32)
    _lib_check(L, L.gol_map_parse(str(text).encode(), m.ctypes.data))
    return m


def format_map(table, library=None) -> str:
    """gol_map_format: the text of a map, "MAP" and 86 base64 characters."""
    L = library or lib()
    m = _as_map(table)
    buf = ctypes.create_string_buffer(90)
    _lib_check(L, L.gol_map_format(m.ctypes.data, buf, len(buf)))
    return buf.value.decode()


def map_from_rule(rule, library=None) -> "np.ndarray":
    """gol_map_from_rule_host: a life-like rule ("B36/S23" or a (birth, survive) pair of 9-bit masks) as a map."""
    import numpy as np
    L = library or lib()
    birth, survive = parse_rule(rule, L) if isinstance(rule, str) else (int(rule[0]), int(rule[1]))
    if not (0 <= birth < 1 << 32 and 0 <= survive < 1 << 32):
        raise GolError(GOL_EINVAL, f"rule masks out of range ({birth}, {survive})")
    m = np.zeros(16, dtype=np.uint32)
    _lib_check(L, L.gol_map_from_rule_host(birth, survive, m.ctypes.data))
    return m


def pack_pattern(cells) -> "np.ndarray":
    """A 2-D array of cells (non-zero = alive) as the uint64 rows of the paste calls: bit c % 64 of
    word c // 64 of a row = cell c (the bit order of load_words)."""
    import numpy as np
    a = np.asarray(cells)
    if a.ndim != 2 or a.shape[0] < 1 or a.shape[1] < 1:
        raise GolError(GOL_EINVAL, f"a pattern is a 2-D array of at least one cell, got shape {a.shape}")
    h, w = a.shape
    bits = np.zeros((h, (w + 63) // 64 * 64), dtype=np.uint8)
    bits[:, :w] = a != 0
    return np.ascontiguousarray(np.packbits(bits, axis=1, bitorder="little")).view("<u8")


def unpack_pattern(words, w: int) -> "np.ndarray":
    """The inverse of pack_pattern: (h, w) bool cells of uint64 pattern rows."""
    import numpy as np
    rows = np.ascontiguousarray(words, dtype="<u8")
    return np.unpackbits(rows.view(np.uint8), axis=1, bitorder="little")[:, :w].astype(bool)


def parse_rle(text, library=None):
    """gol_rle_parse: RLE text ("x = 3, y = 3, rule = B3/S23\\nbob$2bo$3o!") -> ((h, w) bool array,
    rule text, "" if the header names none).  Two-state patterns only; malformed text is
    GolError EFORMAT with the offset.  Host code: no GPU needed."""
    import numpy as np
    L = library or lib()
    raw = text if isinstance(text, (bytes, bytearray)) else str(text).encode()
    w, h = ctypes.c_int64(), ctypes.c_int64()
    rule = ctypes.create_string_buffer(max(len(raw), 1) + 1)
    _lib_check(L, L.gol_rle_parse(raw, len(raw), ctypes.byref(w), ctypes.byref(h), None, 0, 0, rule, len(rule)))
    words = np.zeros((h.value, (w.value + 63) // 64), dtype=np.uint64)
    _lib_check(L, L.gol_rle_parse(raw, len(raw), ctypes.byref(w), ctypes.byref(h), words.ctypes.data, words.shape[1],
                                  words.shape[0], None, 0))
    return unpack_pattern(words, w.value), rule.value.decode(errors="replace")


def format_rle(cells, rule=None, library=None) -> str:
    """gol_rle_format: a 2-D array of cells (non-zero = alive) as RLE text, with `rule` in the
    header when given; lines of at most 70 characters, ending in "!\\n"."""
    import numpy as np
    cells = np.asarray(cells)
    return format_rle_words(pack_pattern(cells), cells.shape[1], rule, library)


def format_rle_words(words, w: int, rule=None, library=None) -> str:
    """format_rle of a pattern that is already bit-packed: (h, >= ceil(w / 64)) uint64 rows as
    pack_pattern and Engine.copy_words give them."""
    import numpy as np
    L = library or lib()
    words = np.ascontiguousarray(words, dtype=np.uint64)
    h = words.shape[0]
    r = None if rule is None else str(rule).encode()
    need = ctypes.c_int64()
    _lib_check(L, L.gol_rle_format(words.ctypes.data, words.shape[1], w, h, r, None, 0, ctypes.byref(need)))
    buf = ctypes.create_string_buffer(need.value)
    _lib_check(L, L.gol_rle_format(words.ctypes.data, words.shape[1], w, h, r, buf, need.value, None))
    return buf.value.decode()


def device_count() -> int:
    n = ctypes.c_int()
    check(lib().gol_device_count(ctypes.byref(n)))
    return n.value
