// gol_kernels.h -- internal launcher interface of the kernel units (each unit holds its own
// launchers, gol_launch.cpp the state they share; not part of the C ABI).  The step kernels and
// the batch kernel each have one launcher that takes a descriptor: golk_step (gol_step_launch.h)
// and golk_batch_step (gol_batch.h); the region kernels share one, gol_region (gol_edit.h); the
// headers that hold a descriptor also hold its check.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gol_edit.h"  // gol_region; GOL_EDIT_BYTES / _STANDARD / _BAND: how a board's rows are stored
#include "gol_step_launch.h"

#ifndef GOL_COUNT_SLOTS
#define GOL_COUNT_SLOTS 256
#endif

// Flags of a launch's device error word (ORed by the failing waves).
#define GOLK_ERR_SPIN 1u  // a pipeline wave gave up waiting for an LDS flag (protocol fault)
#define GOLK_ERR_IPC 2u   // an IPC rank gave up waiting for a neighbour's flag (gol_comm.h)

// Per-device error word for launches made without one (lazily allocated, zeroed).
uint32_t *golk_device_err_word(int device);
// Per-device CU slot masks of the band pipeline's role placement (indexed by XCC, SE, SH, CU).
#define GOL_CU_SLOT_WORDS 2048
uint32_t *golk_cu_slots(int device);
// Zero them again on `s` (after a faulted launch whose workgroups may not have freed their slots).
hipError_t golk_reset_cu_slots(int device, hipStream_t s);
// Paired-rank claim counters (one buffer per launch stream; gol_strips.h StripMap).
// golk_reset_claims: zero the buffer of stream s, ordered on s (after a faulted launch).
// golk_release_claims: free it (the caller has synchronised s; an engine destroying its streams).
// golk_own_stream: mark s as an engine's stream; golk_reset_claims_device (gol_dev_error, after a
// fault in a launcher call on a caller's stream) then leaves its buffer alone.
hipError_t golk_reset_claims(hipStream_t s);
void golk_release_claims(hipStream_t s);
void golk_own_stream(hipStream_t s);
hipError_t golk_reset_claims_device(int device);

// One launch of a step kernel -- bits_step_kernel, band_step_kernel, their TableRule forms,
// bytes_blocked_kernel or one of the two split pipelines behind them -- of what the descriptor says
// (gol_step_launch.h, where the kernel table, every field and the check are).  hipErrorInvalidValue,
// nothing launched, unless gol_step_launch_ok accepts the descriptor and, for a pretended device
// (as_cus, as_slots), neither value exceeds this device's; hipSuccess at once for rows == 0.
hipError_t golk_step(const gol_step_launch &launch, hipStream_t s);
// This device's CU count and resident workgroups of a pipeline kernel (band: band_pipe_kernel with
// contiguous ghost rows or not; else bytes_pipe_kernel), with the fused count or not.
bool golk_pipe_limits(bool band, bool contig, bool count, int *cus, int64_t *slots);
// The pipeline kernels' host handles (gol_band_pipe.hip, gol_bytes_pipe.hip): for occupancy
// queries, and what the units' _launch launches (gol_device.h).
const void *golk_band_pipe_fn(bool contig, bool count);
const void *golk_bytes_pipe_fn(bool count);
// Rounds of resident workgroups a step launch of (family, k, dw) over `rows` rows makes (the band
// pipeline: 1 for its one-round rank-weighted launch; other kernels: 1e9, i.e. many); for the
// engine's choice of step plan.
double golk_step_rounds(int family, int64_t rows, int64_t Wd, int64_t pitch, int k, int dw, int strip);
// Standard <-> band rows (Wd % 32 == 0), out of place.
hipError_t golk_band_convert(bool to_band, const uint32_t *src, uint32_t *dst, int64_t rows, int64_t Wd,
                             int64_t spitch, int64_t dpitch, hipStream_t s);
hipError_t golk_bytes_step(const uint8_t *world, int64_t H, int64_t W, int64_t stride, int64_t y0, int64_t y1,
                           uint8_t *out, int64_t out_stride, hipStream_t s);
hipError_t golk_nonbinary(const uint8_t *bytes, int64_t rows, int64_t W, int64_t stride, uint32_t *flag, hipStream_t s);
hipError_t golk_random_fill(uint32_t *dst, int64_t rows, int64_t grow0, int64_t W, int64_t pitch, uint64_t seed,
                            hipStream_t s);
hipError_t golk_popcount(const uint32_t *src, int64_t rows, int64_t Wd, int64_t pitch, uint64_t *slots,
                         hipStream_t s);
// out[i] = sum of the GOL_COUNT_SLOTS slots of slot array i (arrays of GOL_COUNT_SLOTS*8 uint64);
// the slots are left zeroed.
hipError_t golk_slots_reduce(uint64_t *slots, int64_t n, uint64_t *out, hipStream_t s);
hipError_t golk_hash(const uint32_t *src, int64_t rows, int64_t grow0, int64_t Wd, int64_t pitch, uint64_t *slots,
                     hipStream_t s);
hipError_t golk_count_bytes(const uint8_t *src, int64_t rows, int64_t W, int64_t stride, uint64_t *slots,
                            hipStream_t s);
hipError_t golk_pack(const uint8_t *bytes, int64_t rows, int64_t W, int64_t stride, uint32_t *bits, int64_t pitch,
                     uint32_t *nonbinary, hipStream_t s);
hipError_t golk_unpack(const uint32_t *bits, int64_t rows, int64_t W, int64_t pitch, uint8_t *bytes, int64_t stride,
                       hipStream_t s);
// Per-row counts and the row-major (x, y) list of alive cells; with prev != NULL of the cells
// whose alive state differs between board and prev (same layout and pitch).  y0 is added to
// the listed y (global row of the first row).
hipError_t golk_row_counts(bool bits_mode, const void *board, const void *prev, int64_t rows, int64_t width_units,
                           int64_t pitch, int64_t *out, hipStream_t s);
hipError_t golk_alive_list(bool bits_mode, const void *board, const void *prev, int64_t rows, int64_t width_units,
                           int64_t pitch, const int64_t *offs, int32_t *xy, int64_t cap, int64_t y0, hipStream_t s);

// The region kernels: a rectangle of the running board read or edited in place.  Every launcher takes
// a gol_region (gol_edit.h, where its fields, its one check gol_region_ok and the column mapping
// are): hipErrorInvalidValue, nothing launched, unless the check accepts it; hipSuccess at once for
// rows == 0.  Counters and headers are device words the caller zeroes.
// gol_view.hip: adds to `frame` (w / scale uint32 per pixel row, dense) the alive cells of the
// region's rows, which are viewport rows [at, at + rows); viewport cell (c, v) belongs to pixel
// (c / scale, v / scale), 1 <= scale <= 4096, w a multiple of scale.
hipError_t golk_view_counts(const gol_region &r, int32_t scale, uint32_t *frame, hipStream_t s);
// pixels[i] = ceil(255 * frame[i] / scale^2) for i < n; both buffers hold n rounded up to 4
// elements, 16-byte aligned.
hipError_t golk_view_pixels(const uint32_t *frame, int64_t n, int32_t scale, uint8_t *pixels, hipStream_t s);
// gol_edit.hip: pattern rows [at, at + rows) (pstride uint64 words per row; pattern NULL: all ones)
// applied to the region under op (GOL_PASTE_*); *changed += the cells whose state changed.
hipError_t golk_paste(const gol_region &r, const uint64_t *pattern, int64_t pstride, int32_t op, uint64_t *changed,
                      hipStream_t s);
// gol_copy.hip (nothing is written to the board).  golk_copy gathers the region into pattern rows
// [at, at + rows): it writes every 32-bit half that holds a cell c < w, bits at c >= w zero, and no
// other half -- the caller clears the pattern first; *alive += the alive cells gathered.
hipError_t golk_copy(const gol_region &r, uint64_t *pattern, int64_t pstride, uint64_t *alive, hipStream_t s);
// The bounding box of the region's alive cells.  hdr, 5 words: [0] += alive cells, [1] = max of ~v and
// [2] = max of v over the rectangle rows v (at + the row's offset from `row`) that hold one, [3] = max
// of ~c and [4] = max of c over the columns that hold one.  golk_bounds_rows (once per run of rows)
// fills [0 .. 2] and ORs the columns seen into occ: T uint32 words, T the geom.T of gol_region_ok(r,
// GOL_EDIT_COPY, true, .); golk_bounds_cols (once, after them, on a region of the same rows) turns
// occ into [3] and [4].
hipError_t golk_bounds_rows(const gol_region &r, uint32_t *occ, uint64_t *hdr, hipStream_t s);
hipError_t golk_bounds_cols(const gol_region &r, const uint32_t *occ, uint64_t *hdr, hipStream_t s);

// Batches of small boards: n tori of H x W cells (1 <= H, W <= 512, n <= 2^20), board i at boards + i*H*Ww, Ww =
// ceil(W / 64) uint64 words per row, the bits at c >= W of a row zero.
// The step kernel (gol_batch.hip).  golk_batch_shape: waves per board, boards per workgroup and 32-bit words per lane.
// golk_batch_step: one launch, `turns` >= 1 turns in place, of what the descriptor says (gol_batch.h; the modes and every
// field are those of gol_dev_batch_step, include/golhip.h): every board, or with a list the boards list[0 .. *count)
// alone, *count <= slots <= n, where slots sizes the grid (without a list slots is 0 and n sizes it).
// hipErrorInvalidValue, nothing launched, unless gol_batch_launch_ok accepts the descriptor.
struct gol_batch_launch;
void golk_batch_shape(int64_t H, int64_t W, int *waves_per_board, int *boards_per_wg, int *words_per_lane);
hipError_t golk_batch_step(const gol_batch_launch &launch, hipStream_t s);
// The step kernel of MAP rules (gol_batch_map.hip): a launch whose descriptor has maps, which golk_batch_step hands over.
hipError_t golk_batch_map_step(const gol_batch_launch &launch, hipStream_t s);
// The island census (gol_island.hip): one launch of what the descriptor says (gol_island.h; every field is that of
// gol_dev_batch_islands, include/golhip.h).  hipErrorInvalidValue, nothing launched, unless gol_island_launch_ok accepts it.
struct gol_island_launch;
hipError_t golk_batch_islands(const gol_island_launch &launch, hipStream_t s);
// Every slot of a kind table of 2^table_log2 slots empty, *dropped = 0 (gol_dev_island_table_clear).
struct gol_island_kind;
hipError_t golk_island_table_clear(gol_island_kind *table, int32_t table_log2, int64_t *dropped, hipStream_t s);
// The small kernels (gol_batch_pass.hip).
// list[i] = i for i < n, counts = {n, 0}
hipError_t golk_batch_iota(int32_t *list, int32_t *counts, int64_t n, hipStream_t s);
// The retire pass (one workgroup, stable): counts[0] entries of list_in, counts[1] of finish.  finish loses the
// boards with left[] == 0; a listed board with found[] < 0 goes to active (which may be list_in), one found gets left[] =
// gol_batch_turns_left(found - t0, t_end - t_now) and, unless that is 0, goes to the end of finish.  counts receives
// the two new counts.
hipError_t golk_batch_retire(const int32_t *list_in, int32_t *counts, const int64_t *found, int64_t n, int64_t t0,
                             int64_t t_now, int64_t t_end, int32_t *active, int32_t *finish, int64_t *left, hipStream_t s);
// out[i] = alive cells of board i, or (hash) its oracle_hash_words
hipError_t golk_batch_reduce(bool hash, const uint64_t *boards, int64_t n, int64_t H, int64_t W, uint64_t *out, hipStream_t s);
// gol_batch_search (a slot is a board of the batch; a soup's number counts from the search's `first`).
// golk_batch_soups: board j = soup first + j (gol_batch_soup_word, gol_batch.h), j < n; first = 0: gol_batch_load_random.
// golk_batch_search_init: slots 0 .. m - 1 active with soups 0 .. m - 1, born at 0, not found; counts = {m, 0, 0, m}.
// golk_batch_restock: the pass between the launches (include/golhip.h, gol_dev_batch_restock).  golk_batch_harvest: alive
// and hash of prev[slot] into the tables for the counts[1] pairs (slot, soup) of the harvest list, 0, 0 where found[soup] <
// 0.  golk_batch_refill: the soup words of the slots of its first counts[2] pairs.  slots: an upper bound of those counts
// (the active slots before the pass), which sizes the grids.
hipError_t golk_batch_soups(uint64_t *boards, int64_t n, int64_t H, int64_t W, uint64_t seed, int64_t first, hipStream_t s);
hipError_t golk_batch_search_init(int32_t *active, int32_t *counts, int32_t *soup, int64_t *born, int64_t *found, int64_t m,
                                  hipStream_t s);
hipError_t golk_batch_restock(int32_t *active, int32_t *counts, int64_t *found, int64_t *born, int32_t *soup, int64_t n,
                              int64_t now, int64_t horizon, int64_t total, int64_t *out_found, int64_t *out_period,
                              int32_t *harvest, hipStream_t s);
hipError_t golk_batch_harvest(const uint64_t *prev, const int32_t *harvest, const int32_t *counts, int64_t n, int64_t H,
                              int64_t W, int64_t total, const int64_t *found, uint64_t *alive, uint64_t *hash, int64_t slots,
                              hipStream_t s);
hipError_t golk_batch_refill(uint64_t *boards, const int32_t *harvest, const int32_t *counts, const int32_t *soup, int64_t n,
                             int64_t H, int64_t W, uint64_t seed, int64_t first, int64_t total, int64_t slots, hipStream_t s);

// IPC transport (gol_comm.h): set *flag = value with release ordering at system scope after the
// stream's earlier work; wait (one wave on the stream) until every flags[i] (i < n <= 4, other
// processes' flag words mapped through IPC) has reached `want` (wrap-safe sequence compare),
// then acquire; after timeout_ticks of s_memrealtime (100 MHz) without it, OR GOLK_ERR_IPC into err.
#define GOLK_IPC_MAX_WAIT 4
hipError_t golk_ipc_signal(uint32_t *flag, uint32_t value, hipStream_t s);
hipError_t golk_ipc_wait(const uint32_t *const *flags, int n, uint32_t want, uint64_t timeout_ticks, uint32_t *err,
                         hipStream_t s);
