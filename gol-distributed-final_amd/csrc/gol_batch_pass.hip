// gol_batch_pass.hip -- the small kernels round the batch's step kernel (gol_batch.hip; include/golhip.h, "batches of
// small boards"): the soup fill, the census (one wave per board for the alive count and the hash), and the passes between
// the launches of a call: for gol_batch_run_cycles the identity list and the retire pass (one workgroup), for
// gol_batch_search the start of the search, the restock pass (one workgroup), the harvest and the refill.  The formulas they
// share with the host twins (the soup word, the census terms, the marks, the verdict) are gol_batch.h's.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "gol_device.h"
#include "gol_batch.h"
#include "gol_batch_kernels.h"

namespace {

// boards[i] = word i0 + i of the supply (seed): gol_batch_load_random (i0 = 0), gol_batch_load_soups and the search's first
// fill, soup first + j in slot j
__global__ __launch_bounds__(256) void batch_soups_kernel(uint64_t *boards, int64_t words, int32_t Ww, uint64_t tail,
                                                          uint64_t seed, uint64_t i0)
{
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < words; i += (int64_t)gridDim.x * 256)
        boards[i] = gol_batch_soup_word(seed, i0 + (uint64_t)i, Ww, tail);
}

// The census of the board at p by one wave (gol_batch.h: the alive cells, the hash terms), the sums in every lane
template <bool ALIVE, bool HASH>
__device__ __forceinline__ void wave_census(const uint64_t *p, int32_t words, uint64_t &alive, uint64_t &hash)
{
    uint64_t a = 0, h = 0;
    for (int i = threadIdx.x & 63; i < words; i += 64) {
        if (ALIVE) a += (uint64_t)__popcll(p[i]);
        if (HASH) h += gol_batch_hash_term(p[i], (uint64_t)i);
    }
    alive = ALIVE ? golk::wave_sum_u64(a) : 0;
    hash = HASH ? golk::wave_sum_u64(h) : 0;
}

// out[board] = its alive cells (HASH: its hash); a wave per board
template <bool HASH>
__global__ __launch_bounds__(256) void batch_reduce_kernel(const uint64_t *boards, int64_t n, int32_t words, uint64_t *out)
{
    for (int64_t b = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); b < n; b += (int64_t)gridDim.x * 4) {
        uint64_t a, h;
        wave_census<!HASH, HASH>(boards + b * words, words, a, h);
        if ((threadIdx.x & 63) == 0) out[b] = HASH ? h : a;
    }
}

// The boards 0 .. n - 1 as a list, and the two counts of a retiring call's start: n active, none to finish.
__global__ __launch_bounds__(256) void batch_iota_kernel(int32_t *list, int32_t *counts, int32_t n)
{
    for (int32_t i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) list[i] = i;
    if (blockIdx.x == 0 && threadIdx.x == 0) counts[0] = n, counts[1] = 0;
}

// The retire pass between the launches of gol_batch_run_cycles: one workgroup walks the lists in tiles of
// RETIRE_TILE entries, in order.  First the finish list, in place: a board with left[] == 0 has made its
// remainder and leaves.  Then the active list: a board still at found == -1 stays (active may be list_in: an
// entry is written at or before the place it was read from, and a tile is read before a barrier and written
// after it); a board found gets left[board] = gol_batch_turns_left and, unless that is 0, goes to the end of
// the finish list.  The places come from a ballot per wave and a scan of the RETIRE_COUNTS wave counts of a
// tile by wave 0 through LDS: stable, and the same on every run.  An entry outside 0 .. n - 1 is dropped.
// counts[0]: in the entries of list_in, out those of active; counts[1]: the finish list's, in and out.
#define RETIRE_ITEMS 16
#define RETIRE_TILE (1024 * RETIRE_ITEMS)
#define RETIRE_COUNTS (16 * RETIRE_ITEMS)  // wave counts of a tile, RETIRE_COUNTS / 64 per lane of wave 0
__global__ __launch_bounds__(1024) void batch_retire_kernel(const int32_t *list_in, int32_t *counts, const int64_t *found,
                                                            int64_t n, int64_t t0, int64_t rest, int32_t *active,
                                                            int32_t *finish, int64_t *left)
{
    __shared__ int32_t cnt[2][RETIRE_COUNTS], off[2][RETIRE_COUNTS], total[2];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t cap = n < ((int64_t)1 << 20) ? n : (int64_t)1 << 20;
    const int32_t n_in = (int32_t)max((int64_t)0, min((int64_t)counts[0], cap));
    const int32_t f_in = (int32_t)max((int64_t)0, min((int64_t)counts[1], cap));
    int32_t n_act = 0, n_fin = 0;  // (uniform) entries written so far
    for (int pass = 0; pass < 2; ++pass) {
        const int32_t *src = pass == 0 ? finish : list_in;
        const int64_t *val = pass == 0 ? left : found;
        const int32_t m = pass == 0 ? f_in : n_in;
        for (int32_t base = 0; base < m; base += RETIRE_TILE) {
            int32_t board[RETIRE_ITEMS], place[RETIRE_ITEMS];
            int64_t v[RETIRE_ITEMS];
            int kind[RETIRE_ITEMS];  // -1: leaves, 0: to (or stays in) the active list, 1: to (stays in) the finish list
            // the tile's loads first, each kind together: RETIRE_ITEMS of them in flight, none behind a store
#pragma unroll
            for (int k = 0; k < RETIRE_ITEMS; ++k) {
                const int32_t i = base + k * 1024 + (int32_t)threadIdx.x;
                board[k] = i < m ? src[i] : -1;
            }
#pragma unroll
            for (int k = 0; k < RETIRE_ITEMS; ++k) v[k] = board[k] >= 0 && board[k] < n ? val[board[k]] : 0;
#pragma unroll
            for (int k = 0; k < RETIRE_ITEMS; ++k) {
                kind[k] = -1;
                if (board[k] >= 0 && board[k] < n) {
                    if (pass == 0) {
                        kind[k] = v[k] > 0 ? 1 : -1;
                    } else if (v[k] < 0) {
                        kind[k] = 0;
                    } else {
                        const int64_t l = v[k] > t0 ? gol_batch_turns_left(v[k] - t0, rest) : 0;
                        left[board[k]] = l;
                        kind[k] = l > 0 ? 1 : -1;
                    }
                }
                const uint64_t b0 = __ballot(kind[k] == 0), b1 = __ballot(kind[k] == 1);
                const uint64_t below = ((uint64_t)1 << lane) - 1;
                place[k] = __popcll((kind[k] == 0 ? b0 : b1) & below);
                if (lane == 0) cnt[0][k * 16 + wave] = __popcll(b0), cnt[1][k * 16 + wave] = __popcll(b1);
            }
            __syncthreads();  // every entry of the tile is read
            if (wave == 0) {
#pragma unroll
                for (int q = 0; q < 2; ++q) {
                    int32_t c[RETIRE_COUNTS / 64], sum = 0;
#pragma unroll
                    for (int j = 0; j < RETIRE_COUNTS / 64; ++j) sum += c[j] = cnt[q][lane * (RETIRE_COUNTS / 64) + j];
                    int32_t incl = sum;
                    for (int d = 1; d < 64; d *= 2) {
                        const int32_t up = __shfl_up(incl, d);
                        if (lane >= d) incl += up;
                    }
                    int32_t at = incl - sum;
#pragma unroll
                    for (int j = 0; j < RETIRE_COUNTS / 64; ++j) {
                        off[q][lane * (RETIRE_COUNTS / 64) + j] = at;
                        at += c[j];
                    }
                    if (lane == 63) total[q] = incl;
                }
            }
            __syncthreads();
#pragma unroll
            for (int k = 0; k < RETIRE_ITEMS; ++k) {
                if (kind[k] == 0) active[n_act + off[0][k * 16 + wave] + place[k]] = board[k];
                if (kind[k] == 1 && n_fin + off[1][k * 16 + wave] + place[k] < cap)
                    finish[n_fin + off[1][k * 16 + wave] + place[k]] = board[k];
            }
            n_act += total[0];
            n_fin += total[1];
            __syncthreads();  // the tile is written, the counts are read
        }
    }
    if (threadIdx.x == 0) counts[0] = n_act, counts[1] = n_fin;
}

// ---- gol_batch_search: soups streamed through the batch's slots (a slot is a board of the batch)

// The search's start: slot i < m active with soup i, born at 0 and not found.  counts: [0] the active slots, [1] the slots
// the last pass harvested, [2] those of them it refilled, [3] the soups handed out so far.
__global__ __launch_bounds__(256) void batch_search_init_kernel(int32_t *active, int32_t *counts, int32_t *soup, int64_t *born,
                                                                int64_t *found, int32_t m)
{
    for (int32_t i = blockIdx.x * 256 + threadIdx.x; i < m; i += gridDim.x * 256) {
        active[i] = i;
        soup[i] = i;
        born[i] = 0;
        found[i] = -1;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) counts[0] = m, counts[1] = 0, counts[2] = 0, counts[3] = m;
}

// (The retire pass keeps its inline scan of two lists at once: folded into one function of this shape over one or two flag
// sets it took 8.7 us instead of 6.9 over 4096 entries, 631 instead of 576 over 2^20 on an MI355X.  DESIGN.md §4.20.)
// The places of a tile's flagged entries, in the tile's order (as the retire pass has them: a ballot per wave and item, the
// tile's RETIRE_COUNTS wave counts scanned by wave 0 through LDS); returns how many are flagged.  Every thread calls it.
__device__ __forceinline__ int32_t tile_places(const bool (&flag)[RETIRE_ITEMS], int32_t (&place)[RETIRE_ITEMS], int32_t *cnt,
                                               int32_t *off, int32_t *total)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < RETIRE_ITEMS; ++k) {
        const uint64_t b = __ballot(flag[k]);
        place[k] = __popcll(b & (((uint64_t)1 << lane) - 1));
        if (lane == 0) cnt[k * 16 + wave] = __popcll(b);
    }
    __syncthreads();
    if (wave == 0) {
        int32_t c[RETIRE_COUNTS / 64], sum = 0;
#pragma unroll
        for (int j = 0; j < RETIRE_COUNTS / 64; ++j) sum += c[j] = cnt[lane * (RETIRE_COUNTS / 64) + j];
        int32_t incl = sum;
        for (int d = 1; d < 64; d *= 2) {
            const int32_t up = __shfl_up(incl, d);
            if (lane >= d) incl += up;
        }
        int32_t at = incl - sum;
#pragma unroll
        for (int j = 0; j < RETIRE_COUNTS / 64; ++j) {
            off[lane * (RETIRE_COUNTS / 64) + j] = at;
            at += c[j];
        }
        if (lane == 63) *total = incl;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < RETIRE_ITEMS; ++k) place[k] += off[k * 16 + wave];
    const int32_t t = *total;
    __syncthreads();  // cnt, off and total are free again
    return t;
}

// The restock pass between the launches of gol_batch_search: one workgroup walks the active list in tiles of RETIRE_TILE
// slots, in order.  gol_batch_verdict decides from a slot's found age, its age now - born[slot] and the horizon.  A slot that
// is done (found or expired) writes found and period of its soup (-1, -1 when expired) and goes on the harvest list as the
// pair (slot, soup), in the list's order; the r-th done slot of the pass takes soup next + r while that is below total
// (born = now, found = -1, it stays active), else it leaves the active list.  So the slots refilled are the first counts[2]
// entries of the harvest list, which is the fill list too.  The active list is compacted in place (an entry is written at
// or before the place it was read from; a tile is read before a barrier and written after it); stable, the same on every
// run.  A slot outside 0 .. n - 1 is dropped, a soup outside 0 .. total - 1 writes no result.
__global__ __launch_bounds__(1024) void batch_restock_kernel(int32_t *active, int32_t *counts, int64_t *found, int64_t *born,
                                                             int32_t *soup, int64_t n, int64_t now, int64_t horizon,
                                                             int32_t total, int64_t *out_found, int64_t *out_period,
                                                             int32_t *harvest)
{
    __shared__ int32_t cnt[RETIRE_COUNTS], off[RETIRE_COUNTS], sum;
    const int64_t cap = n < ((int64_t)1 << 20) ? n : (int64_t)1 << 20;
    const int32_t n_in = (int32_t)max((int64_t)0, min((int64_t)counts[0], cap));
    const int32_t next = max(0, min(counts[3], total));  // the soups handed out before this pass
    int32_t n_act = 0, n_done = 0;                       // (uniform) entries written so far
    for (int32_t base = 0; base < n_in; base += RETIRE_TILE) {
        int32_t slot[RETIRE_ITEMS], place[RETIRE_ITEMS];
        int64_t f[RETIRE_ITEMS], b[RETIRE_ITEMS];
        bool hit[RETIRE_ITEMS], done[RETIRE_ITEMS], kept[RETIRE_ITEMS];
        // the tile's loads first, each kind together, none behind a store
#pragma unroll
        for (int k = 0; k < RETIRE_ITEMS; ++k) {
            const int32_t i = base + k * 1024 + (int32_t)threadIdx.x;
            slot[k] = i < n_in ? active[i] : -1;
            if (slot[k] >= n) slot[k] = -1;
        }
#pragma unroll
        for (int k = 0; k < RETIRE_ITEMS; ++k) f[k] = slot[k] >= 0 ? found[slot[k]] : -1;
#pragma unroll
        for (int k = 0; k < RETIRE_ITEMS; ++k) b[k] = slot[k] >= 0 ? born[slot[k]] : 0;
#pragma unroll
        for (int k = 0; k < RETIRE_ITEMS; ++k) {
            const int v = slot[k] >= 0 ? gol_batch_verdict(f[k], now - b[k], horizon) : GOL_BATCH_STAY;
            hit[k] = v == GOL_BATCH_FOUND;
            done[k] = v != GOL_BATCH_STAY;
        }
        const int32_t tile_done = tile_places(done, place, cnt, off, &sum);
#pragma unroll
        for (int k = 0; k < RETIRE_ITEMS; ++k) {
            kept[k] = slot[k] >= 0 && !done[k];
            if (!done[k]) continue;
            const int32_t r = n_done + place[k];  // < n_in <= n: the harvest list holds n pairs
            int32_t g = soup[slot[k]];
            if (g < 0 || g >= total) g = -1;
            if (g >= 0) {
                out_found[g] = hit[k] ? f[k] : -1;
                out_period[g] = hit[k] ? gol_batch_period(f[k]) : -1;
            }
            harvest[2 * r] = slot[k];
            harvest[2 * r + 1] = g;
            if (r < total - next) {
                soup[slot[k]] = next + r;
                born[slot[k]] = now;
                found[slot[k]] = -1;
                kept[k] = true;
            }
        }
        const int32_t tile_kept = tile_places(kept, place, cnt, off, &sum);
#pragma unroll
        for (int k = 0; k < RETIRE_ITEMS; ++k)
            if (kept[k]) active[n_act + place[k]] = slot[k];
        n_act += tile_kept;
        n_done += tile_done;
        __syncthreads();  // the tile is written before the next one is read
    }
    if (threadIdx.x == 0) {
        const int32_t refilled = min(n_done, total - next);
        counts[0] = n_act, counts[1] = n_done, counts[2] = refilled, counts[3] = next + refilled;
    }
}

// The census of the slots the pass harvested, a wave per slot: prev[slot] holds s(found) of the soup the slot ran (the aged
// step kernel keeps the snapshot once a board is found), and alive[soup], hash[soup] become its alive cells and its hash;
// 0, 0 for a soup that expired.
__global__ __launch_bounds__(256) void batch_harvest_kernel(const uint64_t *prev, const int32_t *harvest, const int32_t *counts,
                                                            int64_t n, int32_t words, int32_t total, const int64_t *found,
                                                            uint64_t *alive, uint64_t *hash)
{
    const int32_t m = (int32_t)max((int64_t)0, min((int64_t)counts[1], n));
    for (int32_t r = blockIdx.x * 4 + (threadIdx.x >> 6); r < m; r += gridDim.x * 4) {
        const int32_t slot = harvest[2 * r], g = harvest[2 * r + 1];
        if (slot < 0 || slot >= n || g < 0 || g >= total) continue;
        uint64_t a = 0, h = 0;
        if (found[g] >= 0) wave_census<true, true>(prev + (int64_t)slot * words, words, a, h);
        if ((threadIdx.x & 63) == 0) alive[g] = a, hash[g] = h;
    }
}

// The new soups of the slots the pass refilled (the first counts[2] pairs of the harvest list), soup[slot] the soup's number
// from `first`: the words of batch_soups_kernel.
__global__ __launch_bounds__(256) void batch_refill_kernel(uint64_t *boards, const int32_t *harvest, const int32_t *counts,
                                                           const int32_t *soup, int64_t n, int32_t words, int32_t Ww,
                                                           uint64_t tail, uint64_t seed, uint64_t first, int32_t total)
{
    const int64_t m = max((int64_t)0, min((int64_t)counts[2], n));
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < m * words; i += (int64_t)gridDim.x * 256) {
        const int64_t r = i / words, k = i - r * words;
        const int32_t slot = harvest[2 * r];
        if (slot < 0 || slot >= n) continue;
        const int32_t g = soup[slot];
        if (g < 0 || g >= total) continue;
        boards[(int64_t)slot * words + k] = gol_batch_soup_word(seed, (first + (uint64_t)g) * (uint64_t)words + (uint64_t)k, Ww, tail);
    }
}

// soups [first, first + total) of a search: at most 2^26 of the supply's 2^40
bool soups_ok(int64_t first, int64_t total)
{
    return first >= 0 && total >= 0 && total <= ((int64_t)1 << 26) && first + total <= ((int64_t)1 << 40);
}

}  // namespace

hipError_t golk_batch_iota(int32_t *list, int32_t *counts, int64_t n, hipStream_t s)
{
    if (!list || !counts || !gol_batch_shape_ok(n, 1, 1)) return hipErrorInvalidValue;
    batch_iota_kernel<<<(unsigned)std::min<int64_t>((n + 255) / 256, 1024), 256, 0, s>>>(list, counts, (int32_t)n);
    return hipGetLastError();
}

hipError_t golk_batch_retire(const int32_t *list_in, int32_t *counts, const int64_t *found, int64_t n, int64_t t0,
                             int64_t t_now, int64_t t_end, int32_t *active, int32_t *finish, int64_t *left, hipStream_t s)
{
    if (!list_in || !counts || !found || !active || !finish || !left || !gol_batch_shape_ok(n, 1, 1) || t0 > t_now || t_now > t_end)
        return hipErrorInvalidValue;
    batch_retire_kernel<<<1, 1024, 0, s>>>(list_in, counts, found, n, t0, t_end - t_now, active, finish, left);
    return hipGetLastError();
}

hipError_t golk_batch_reduce(bool hash, const uint64_t *boards, int64_t n, int64_t H, int64_t W, uint64_t *out, hipStream_t s)
{
    if (!boards || !out || !gol_batch_shape_ok(n, H, W)) return hipErrorInvalidValue;
    const int32_t words = (int32_t)(H * ((W + 63) / 64));
    const unsigned grid = (unsigned)std::min<int64_t>((n + 3) / 4, 8192);
    if (hash) batch_reduce_kernel<true><<<grid, 256, 0, s>>>(boards, n, words, out);
    else batch_reduce_kernel<false><<<grid, 256, 0, s>>>(boards, n, words, out);
    return hipGetLastError();
}

hipError_t golk_batch_soups(uint64_t *boards, int64_t n, int64_t H, int64_t W, uint64_t seed, int64_t first, hipStream_t s)
{
    if (!boards || !gol_batch_shape_ok(n, H, W) || first < 0 || first > ((int64_t)1 << 40)) return hipErrorInvalidValue;
    const int64_t Ww = (W + 63) / 64, words = n * H * Ww;
    const unsigned grid = (unsigned)std::min<int64_t>((words + 255) / 256, 8192);
    batch_soups_kernel<<<grid, 256, 0, s>>>(boards, words, (int32_t)Ww, gol_batch_tail64(W), seed, (uint64_t)(first * H * Ww));
    return hipGetLastError();
}

hipError_t golk_batch_search_init(int32_t *active, int32_t *counts, int32_t *soup, int64_t *born, int64_t *found, int64_t m,
                                  hipStream_t s)
{
    if (!active || !counts || !soup || !born || !found || !gol_batch_shape_ok(m, 1, 1)) return hipErrorInvalidValue;
    batch_search_init_kernel<<<(unsigned)std::min<int64_t>((m + 255) / 256, 1024), 256, 0, s>>>(active, counts, soup, born, found,
                                                                                               (int32_t)m);
    return hipGetLastError();
}

hipError_t golk_batch_restock(int32_t *active, int32_t *counts, int64_t *found, int64_t *born, int32_t *soup, int64_t n,
                              int64_t now, int64_t horizon, int64_t total, int64_t *out_found, int64_t *out_period,
                              int32_t *harvest, hipStream_t s)
{
    if (!active || !counts || !found || !born || !soup || !out_found || !out_period || !harvest || !gol_batch_shape_ok(n, 1, 1) ||
        now < 0 || horizon < 0 || !soups_ok(0, total))
        return hipErrorInvalidValue;
    batch_restock_kernel<<<1, 1024, 0, s>>>(active, counts, found, born, soup, n, now, horizon, (int32_t)total, out_found,
                                            out_period, harvest);
    return hipGetLastError();
}

hipError_t golk_batch_harvest(const uint64_t *prev, const int32_t *harvest, const int32_t *counts, int64_t n, int64_t H,
                              int64_t W, int64_t total, const int64_t *found, uint64_t *alive, uint64_t *hash, int64_t slots,
                              hipStream_t s)
{
    if (!prev || !harvest || !counts || !found || !alive || !hash || !gol_batch_shape_ok(n, H, W) || !soups_ok(0, total) ||
        slots < 1 || slots > n)
        return hipErrorInvalidValue;
    const unsigned grid = (unsigned)std::min<int64_t>((slots + 3) / 4, 8192);
    batch_harvest_kernel<<<grid, 256, 0, s>>>(prev, harvest, counts, n, (int32_t)(H * ((W + 63) / 64)), (int32_t)total, found,
                                              alive, hash);
    return hipGetLastError();
}

hipError_t golk_batch_refill(uint64_t *boards, const int32_t *harvest, const int32_t *counts, const int32_t *soup, int64_t n,
                             int64_t H, int64_t W, uint64_t seed, int64_t first, int64_t total, int64_t slots, hipStream_t s)
{
    if (!boards || !harvest || !counts || !soup || !gol_batch_shape_ok(n, H, W) || !soups_ok(first, total) || slots < 1 ||
        slots > n)
        return hipErrorInvalidValue;
    const int64_t Ww = (W + 63) / 64, words = H * Ww;
    const unsigned grid = (unsigned)std::min<int64_t>((slots * words + 255) / 256, 8192);
    batch_refill_kernel<<<grid, 256, 0, s>>>(boards, harvest, counts, soup, n, (int32_t)words, (int32_t)Ww, gol_batch_tail64(W),
                                             seed, (uint64_t)first, (int32_t)total);
    return hipGetLastError();
}
