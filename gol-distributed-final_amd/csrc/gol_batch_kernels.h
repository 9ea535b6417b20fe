// gol_batch_kernels.h -- the launchers of the batch's kernel units (gol_batch.hip, gol_batch_map.hip,
// gol_batch_pass.hip, gol_island.hip); internal, not part of the C ABI.  The step kernels and the
// island census each have one launcher that takes a descriptor (gol_batch.h, gol_island.h, which
// also hold its check); a caller that fills one includes that header itself.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

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
