// gol_batch.hip -- many small tori (1 <= H, W <= 512) stepped in one launch (include/golhip.h,
// "batches of small boards"; the row function is gol_batch.h).
//
// batch_step_kernel<NW, RULE, SCAN, LIST, AGED>: a board never leaves its workgroup during a launch.  One
// row per lane, NW = 1, 2, 4, 8 or 16 words of it in registers, ceil(H / 64) waves per board; boards
// of up to 128 rows share a workgroup (4 boards of one wave, 2 of two).  The board is read from HBM
// once, stepped `turns` times and written once, in place: no HBM traffic between the turns.
// Per turn a lane computes the horizontal sums of its own row (gol_batch_hsum) and takes those of the
// rows above and below from the neighbouring lanes by DPP (wave_shr:1 / wave_shl:1); only a wave's
// first and last row cross a wave (or wrap round the torus: rows (y +- 1) mod H) and go through LDS,
// double-buffered, so a turn has one __syncthreads() and the LDS of a workgroup is 256 NW + 64 bytes.
// H = 1, 2 and a partly filled last wave are the same code: a lane without a row keeps zero words.
// SCAN: the cells of the turn before stay in registers too, every lane compares its new row with
// the row two turns back, one ballot per wave and turn says whether any word differs, and the
// waves of a board exchange that bit through LDS under the next turn's barrier.  The first turn t
// with state(t) == state(t - 2) goes to settled[board] unless an earlier launch of the call set it;
// state(start - 1) of a launch comes from, and state(end - 1) goes to, a second device buffer.
// SCAN = GOL_BATCH_SCAN_CYCLES: the same registers hold a snapshot instead, state(m) of the last
// mark m = 2^j - 1 of the call's own turn count (gol_batch.h), every turn is compared with it, and after
// the comparison at a turn that is a mark the snapshot becomes that turn's state: the first turn t with
// state(t) == state(last mark before t) goes to settled[board] (any period: Brent's cycle detection);
// the snapshot goes through the same second buffer between the launches of a call.
// RULE: B3/S23 on 7 gates, the table circuit with the masks of the arguments, or the table circuit
// with the masks of the wave's own board (rules[2 board], rules[2 board + 1]), read once per launch
// by a scalar load, so the expanded tables are wave-uniform as in the one-rule kernel.
// LIST (gol_batch_run_cycles): a workgroup's board slots index a device list of board numbers with a device
// count; a slot past the count has no board, like a board past n.  With the cycle scan it is the search over the
// boards not found yet (prev, settled and the rules stay indexed by the board's own number).  Without a scan it is
// the finish: every listed board has its own number of turns still to make (left[board]), the workgroup's loop
// makes the most any of its boards needs (at most the launch's turns; uniform, since every wave runs every
// barrier), a wave whose board has made its turns keeps its cells, and the turns made are taken off left[].
// AGED (gol_batch_search; LIST + cycles, B3/S23 or the one-rule table): the listed boards are slots that hold soups of
// different ages.  born[board] is the call's turn count at the launch boundary where the slot was filled, read by a scalar
// load like the list entry; with age = done - born the mark test is per board (gol_batch_is_mark(age + it + 1)), age 0 is the
// board's first launch (the loaded state is the snapshot, prev is not read), and settled[board] receives the age at which
// the board is found.  Once found is known -- uniform over the board's waves, before the iteration's snapshot update --
// the snapshot is no longer replaced, so prev[board] holds s(found) after the launch for the harvest.
// Synchronisation is __syncthreads() alone: no workgroup waits for another one, there is no flag
// between workgroups, no spin loop and no atomic.  Every wave of a workgroup runs every barrier (a
// wave whose board is past the batch's end computes on zeros and stores nothing).
//
// The small kernels: random fill, one wave per board for the alive count and the hash, and for
// gol_batch_run_cycles the identity list and the retire pass between its launches (one workgroup); for gol_batch_search
// the soup fills, the restock pass (one workgroup) and the harvest.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "gol_device.h"
#define GOL_BATCH_CONWAY golk::rule  // B3/S23 on the step kernels' 7 gates
#include "gol_batch.h"

namespace {

struct BatchArgs {
    uint64_t *boards;  // n boards of H rows of Ww uint64 words, dense; stepped in place
    uint64_t *prev;    // SCAN: state(start - 1) in (have_prev), state(end - 1) out (write_prev); same shape
    int64_t *settled;  // SCAN: n turns, -1 = not settled yet
    int64_t n, turn0;  // boards; the turn of the loaded state
    gol_batch_row g;
    int32_t H, Ww, wpb, bpw;  // rows, uint64 words per row, waves per board, boards per workgroup
    int32_t turns;            // >= 1
    int32_t have_prev, write_prev;
    uint32_t birth, survive;
    const uint32_t *rules;  // GOL_BATCH_RULE_EACH: n pairs (birth, survive)
    int64_t done;           // GOL_BATCH_SCAN_CYCLES: the turns of the call before this launch
    // LIST: the board of slot i of the grid is list[i], i < *count (a slot past the count has no board)
    const int32_t *list, *count;
    int64_t *left;  // LIST without a scan (the finish): per board the turns it still has to make, taken off here
    // AGED (gol_batch_search): per board the call's turn count `done` of the launch before which it was filled
    const int64_t *born;
};

template <int NW>
__device__ __forceinline__ void load_row(const uint64_t *row, int32_t Ww, bool on, uint32_t (&c)[NW])
{
    const uint32_t *p = (const uint32_t *)row;
#pragma unroll
    for (int j = 0; j < NW; ++j) c[j] = on && j < 2 * Ww ? p[j] : 0u;
}

// (a row is 2 Ww words in memory; with NW = 1 the second one is padding)
template <int NW>
__device__ __forceinline__ void store_row(uint64_t *row, int32_t Ww, const uint32_t (&c)[NW])
{
    uint32_t *p = (uint32_t *)row;
#pragma unroll
    for (int j = 0; j < (NW < 2 ? 2 : NW); ++j)
        if (j < 2 * Ww) p[j] = j < NW ? c[j < NW ? j : 0] : 0u;
}

template <int NW, int RULE, int SCAN, bool LIST, bool AGED>
__global__ __launch_bounds__(512) void batch_step_kernel(const BatchArgs a)
{
    // [buffer][wave][first / last row of the wave][h0 / h1][word]
    __shared__ uint32_t edge[2][GOL_BATCH_MAX_WAVES][2][2][NW];
    __shared__ uint32_t differs[2][GOL_BATCH_MAX_WAVES];

    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int lb = wave / a.wpb, w = wave - lb * a.wpb;  // the board's slot in the workgroup, the wave's in the board
    // LIST: the slot's board from the list, the finish's trip count and this board's own turns -- all wave-uniform,
    // the slot made scalar like the per-board rule read below, so the reads are scalar loads
    int64_t board = (int64_t)blockIdx.x * a.bpw + lb;
    bool has = board < a.n;
    int trips = a.turns, my = a.turns;  // the turns of the workgroup's loop; of them, those this wave's board makes
    int64_t left = 0;
    int64_t age = a.done;  // (uniform) the turns of the scan before this launch: the call's, AGED the board's own
    if (LIST) {
        const uint32_t count = (uint32_t)*a.count;
        const uint32_t slot = __builtin_amdgcn_readfirstlane((uint32_t)(blockIdx.x * a.bpw + lb));
        has = slot < count;
        board = has ? a.list[slot] : 0;
        if (!SCAN) {  // every wave runs every barrier: the workgroup makes the most turns any of its boards needs
            trips = 0;
            for (uint32_t i = blockIdx.x * a.bpw; i < (blockIdx.x + 1) * a.bpw && i < count; ++i)
                trips = max(trips, (int)min((int64_t)a.turns, a.left[a.list[i]]));
            left = has ? a.left[board] : 0;
            my = (int)min((int64_t)a.turns, left);
        }
        if (AGED) age = a.done - (has ? a.born[board] : 0);
    }
    const bool have_prev = AGED ? age > 0 : a.have_prev != 0;  // AGED: a board's first launch has no snapshot to read
    const int y = w * 64 + lane;
    const int last = min(63, a.H - 1 - w * 64);  // the wave's last lane with a row
    const bool on = has && y < a.H;
    const uint32_t msk = on ? ~0u : 0u;
    const int wup = lb * a.wpb + (w == 0 ? a.wpb - 1 : w - 1), wdn = lb * a.wpb + (w == a.wpb - 1 ? 0 : w + 1);
    const gol_batch_row g = a.g;
    // the board's own rule: the board's index is wave-uniform, and made scalar it turns the read into a scalar
    // load (a wave past the batch's end reads the last board's rule, and computes on zeros)
    uint32_t birth = a.birth, survive = a.survive;
    if (RULE == GOL_BATCH_RULE_EACH) {
        const uint32_t i = __builtin_amdgcn_readfirstlane((uint32_t)(board < a.n ? board : a.n - 1));
        birth = __builtin_amdgcn_readfirstlane(a.rules[2 * (size_t)i]);
        survive = __builtin_amdgcn_readfirstlane(a.rules[2 * (size_t)i + 1]);
    }
    gol_rule_tab tab;
    gol_rule_expand(birth, survive, tab);

    const int64_t off = (board * a.H + y) * a.Ww;
    uint32_t cur[NW], old[NW];  // state(t - 1) and, SCAN, state(t - 2) or the snapshot
    load_row<NW>(a.boards + (on ? off : 0), a.Ww, on, cur);
    if (SCAN) load_row<NW>(a.prev + (on && have_prev ? off : 0), a.Ww, on && have_prev, old);
    if (SCAN == GOL_BATCH_SCAN_CYCLES && !have_prev) {  // the call's first launch: the mark d = 0
#pragma unroll
        for (int j = 0; j < NW; ++j) old[j] = cur[j];
    }

    int64_t found = -1;  // uniform over the board's waves
    bool mine = false;   // this wave's "a word differs" of the turn just computed
    int buf = 0;
    for (int it = 0; it < trips; ++it, buf ^= 1) {
        uint32_t b0[NW], b1[NW], a0[NW], a1[NW], d0[NW], d1[NW], next[NW];
        gol_batch_hsum<NW>(cur, g.nwr, g.tb, b0, b1);
        if (lane == 0) {
#pragma unroll
            for (int j = 0; j < NW; ++j) { edge[buf][wave][0][0][j] = b0[j]; edge[buf][wave][0][1][j] = b1[j]; }
        }
        if (lane == last) {
#pragma unroll
            for (int j = 0; j < NW; ++j) { edge[buf][wave][1][0][j] = b0[j]; edge[buf][wave][1][1][j] = b1[j]; }
        }
        // the turn before compared its state with the one two turns back (none before the first loaded state),
        // or with the snapshot
        const bool posted = SCAN == GOL_BATCH_SCAN_CYCLES ? it >= 1 : SCAN && it >= (a.have_prev ? 1 : 2);
        if (posted && lane == 0) differs[buf][wave] = mine;
        __syncthreads();
        if (posted && found < 0) {
            bool any = false;
            for (int i = 0; i < a.wpb; ++i) any |= differs[buf][lb * a.wpb + i] != 0;
            if (!any) found = (AGED ? age : a.turn0) + it;
        }
#pragma unroll
        for (int j = 0; j < NW; ++j) {
            a0[j] = golk::from_lower_lane(b0[j]);
            a1[j] = golk::from_lower_lane(b1[j]);
            d0[j] = golk::from_upper_lane(b0[j]);
            d1[j] = golk::from_upper_lane(b1[j]);
        }
        if (lane == 0) {
#pragma unroll
            for (int j = 0; j < NW; ++j) { a0[j] = edge[buf][wup][1][0][j]; a1[j] = edge[buf][wup][1][1][j]; }
        }
        if (lane == last) {
#pragma unroll
            for (int j = 0; j < NW; ++j) { d0[j] = edge[buf][wdn][0][0][j]; d1[j] = edge[buf][wdn][0][1][j]; }
        }
        gol_batch_next<NW, RULE != GOL_BATCH_RULE_CONWAY>(tab, g, a0, a1, b0, b1, d0, d1, cur, msk, next);
        if (SCAN) {
            // (uniform) cycles: the turn just computed is a mark, its state the snapshot from now on
            // AGED: the board's own age counts, and once it is found its snapshot stays: s(found) for the harvest
            const bool keep = SCAN == GOL_BATCH_SCAN_CYCLES && (!gol_batch_is_mark(age + it + 1) || (AGED && found >= 0));
            uint32_t d = 0;
#pragma unroll
            for (int j = 0; j < NW; ++j) {
                d |= next[j] ^ old[j];
                old[j] = SCAN == GOL_BATCH_SCAN_CYCLES ? (keep ? old[j] : next[j]) : cur[j];
            }
            mine = __ballot(d != 0) != 0;
        }
        const bool go = !LIST || SCAN || it < my;  // (uniform) the finish: a board that has made its turns keeps cur
#pragma unroll
        for (int j = 0; j < NW; ++j) cur[j] = go ? next[j] : cur[j];
    }
    // the last turn's comparison (buf: the buffer no wave reads any more)
    if (SCAN == GOL_BATCH_SCAN_CYCLES || (SCAN && (a.turns > 1 || a.have_prev))) {
        if (lane == 0) differs[buf][wave] = mine;
        __syncthreads();
        if (found < 0) {
            bool any = false;
            for (int i = 0; i < a.wpb; ++i) any |= differs[buf][lb * a.wpb + i] != 0;
            if (!any) found = (AGED ? age : a.turn0) + a.turns;
        }
    }
    if (on) {
        store_row<NW>(a.boards + off, a.Ww, cur);
        if (SCAN && a.write_prev) store_row<NW>(a.prev + off, a.Ww, old);
        if (SCAN && y == 0 && found >= 0 && a.settled[board] < 0) a.settled[board] = found;
        // (read before the loop's first barrier by every wave of the workgroup, written after its last one)
        if (LIST && !SCAN && y == 0 && my > 0) a.left[board] = left - my;
    }
}

// word(i, y, w) = splitmix64(seed ^ ((i H + y) Ww + w)), the padding of a row's last word cleared
__global__ __launch_bounds__(256) void batch_random_kernel(uint64_t *boards, int64_t words, int32_t Ww, uint64_t tail,
                                                           uint64_t seed)
{
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < words; i += (int64_t)gridDim.x * 256) {
        const uint64_t v = golk::splitmix64(seed ^ (uint64_t)i);
        boards[i] = i % Ww == Ww - 1 ? v & tail : v;
    }
}

// out[board] = its alive cells (HASH: sum of splitmix64(word ^ splitmix64(index in the board))); a wave per board
template <bool HASH>
__global__ __launch_bounds__(256) void batch_reduce_kernel(const uint64_t *boards, int64_t n, int32_t words, uint64_t *out)
{
    const int lane = threadIdx.x & 63;
    for (int64_t b = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); b < n; b += (int64_t)gridDim.x * 4) {
        const uint64_t *p = boards + b * words;
        uint64_t s = 0;
        for (int i = lane; i < words; i += 64)
            s += HASH ? golk::splitmix64(p[i] ^ golk::splitmix64((uint64_t)i)) : (uint64_t)__popcll(p[i]);
        s = golk::wave_sum_u64(s);
        if (lane == 0) out[b] = s;
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

// boards[i] = word i0 + i of the supply (seed): gol_batch_load_soups and the search's first fill, soup first + j in slot j
__global__ __launch_bounds__(256) void batch_soups_kernel(uint64_t *boards, int64_t words, int32_t Ww, uint64_t tail,
                                                          uint64_t seed, uint64_t i0)
{
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < words; i += (int64_t)gridDim.x * 256)
        boards[i] = gol_batch_soup_word(seed, i0 + (uint64_t)i, Ww, tail);
}

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
                out_period[g] = hit[k] ? f[k] - gol_batch_last_mark(f[k]) : -1;
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
// step kernel keeps the snapshot once a board is found), and alive[soup], hash[soup] become its alive cells and its
// oracle_hash_words (batch_reduce_kernel's sums); 0, 0 for a soup that expired.
__global__ __launch_bounds__(256) void batch_harvest_kernel(const uint64_t *prev, const int32_t *harvest, const int32_t *counts,
                                                            int64_t n, int32_t words, int32_t total, const int64_t *found,
                                                            uint64_t *alive, uint64_t *hash)
{
    const int lane = threadIdx.x & 63;
    const int32_t m = (int32_t)max((int64_t)0, min((int64_t)counts[1], n));
    for (int32_t r = blockIdx.x * 4 + (threadIdx.x >> 6); r < m; r += gridDim.x * 4) {
        const int32_t slot = harvest[2 * r], g = harvest[2 * r + 1];
        if (slot < 0 || slot >= n || g < 0 || g >= total) continue;
        uint64_t a = 0, h = 0;
        if (found[g] >= 0) {
            const uint64_t *p = prev + (int64_t)slot * words;
            for (int i = lane; i < words; i += 64) {
                a += (uint64_t)__popcll(p[i]);
                h += golk::splitmix64(p[i] ^ golk::splitmix64((uint64_t)i));
            }
            a = golk::wave_sum_u64(a);
            h = golk::wave_sum_u64(h);
        }
        if (lane == 0) alive[g] = a, hash[g] = h;
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

template <int NW, int RULE>
hipError_t launch_scan(int scan, bool list, const BatchArgs &a, dim3 grid, dim3 block, hipStream_t s)
{
    if (list && scan == GOL_BATCH_SCAN_CYCLES)
        batch_step_kernel<NW, RULE, GOL_BATCH_SCAN_CYCLES, true, false><<<grid, block, 0, s>>>(a);
    else if (list)
        batch_step_kernel<NW, RULE, GOL_BATCH_SCAN_NONE, true, false><<<grid, block, 0, s>>>(a);
    else if (scan == GOL_BATCH_SCAN_CYCLES)
        batch_step_kernel<NW, RULE, GOL_BATCH_SCAN_CYCLES, false, false><<<grid, block, 0, s>>>(a);
    else if (scan == GOL_BATCH_SCAN_SETTLE)
        batch_step_kernel<NW, RULE, GOL_BATCH_SCAN_SETTLE, false, false><<<grid, block, 0, s>>>(a);
    else
        batch_step_kernel<NW, RULE, GOL_BATCH_SCAN_NONE, false, false><<<grid, block, 0, s>>>(a);
    return hipGetLastError();
}

// the aged search of gol_batch_search: one rule for the batch (a rule per soup is not built)
template <int NW>
hipError_t launch_aged(int rule, const BatchArgs &a, dim3 grid, dim3 block, hipStream_t s)
{
    if (rule == GOL_BATCH_RULE_TABLE)
        batch_step_kernel<NW, GOL_BATCH_RULE_TABLE, GOL_BATCH_SCAN_CYCLES, true, true><<<grid, block, 0, s>>>(a);
    else
        batch_step_kernel<NW, GOL_BATCH_RULE_CONWAY, GOL_BATCH_SCAN_CYCLES, true, true><<<grid, block, 0, s>>>(a);
    return hipGetLastError();
}

template <int NW>
hipError_t launch_rule(int rule, int scan, bool list, const BatchArgs &a, dim3 grid, dim3 block, hipStream_t s)
{
    if (a.born) return rule == GOL_BATCH_RULE_EACH ? hipErrorInvalidValue : launch_aged<NW>(rule, a, grid, block, s);
    if (rule == GOL_BATCH_RULE_EACH) return launch_scan<NW, GOL_BATCH_RULE_EACH>(scan, list, a, grid, block, s);
    if (rule == GOL_BATCH_RULE_TABLE) return launch_scan<NW, GOL_BATCH_RULE_TABLE>(scan, list, a, grid, block, s);
    return launch_scan<NW, GOL_BATCH_RULE_CONWAY>(scan, list, a, grid, block, s);
}

}  // namespace

void golk_batch_shape(int64_t H, int64_t W, int *waves_per_board, int *boards_per_wg, int *words_per_lane)
{
    const int wpb = (int)((H + 63) / 64);
    *waves_per_board = wpb;
    *boards_per_wg = std::max(1, 4 / wpb);
    *words_per_lane = gol_batch_row_init(W).nw;
}

// list == NULL: every board, slots = n; else the boards list[0 .. *count), *count <= slots
static hipError_t batch_launch(uint64_t *boards, uint64_t *prev, int64_t *settled, int64_t n, int64_t H, int64_t W, int turns,
                               int64_t turn0, bool have_prev, bool write_prev, uint32_t birth, uint32_t survive,
                               const uint32_t *rules, int scan, int64_t done, const int32_t *list, const int32_t *count,
                               int64_t slots, int64_t *left, const int64_t *born, hipStream_t s)
{
    if (!boards || n < 1 || n > ((int64_t)1 << 20) || H < 1 || H > GOL_BATCH_MAX_SIDE || W < 1 || W > GOL_BATCH_MAX_SIDE ||
        turns < 1 || birth >= 512 || survive >= 512 || (settled && !prev) || ((have_prev || write_prev) && !settled) ||
        scan < GOL_BATCH_SCAN_NONE || scan > GOL_BATCH_SCAN_CYCLES || (scan != GOL_BATCH_SCAN_NONE) != (settled != nullptr) ||
        done < 0 || (scan == GOL_BATCH_SCAN_CYCLES && have_prev != (done > 0)))
        return hipErrorInvalidValue;
    BatchArgs a{};
    int nw;
    golk_batch_shape(H, W, &a.wpb, &a.bpw, &nw);
    a.boards = boards;
    a.prev = prev;
    a.settled = settled;
    a.n = n;
    a.turn0 = turn0;
    a.g = gol_batch_row_init(W);
    a.H = (int32_t)H;
    a.Ww = (int32_t)((W + 63) / 64);
    a.turns = turns;
    a.have_prev = have_prev;
    a.write_prev = write_prev;
    a.birth = birth;
    a.survive = survive;
    a.rules = rules;
    a.done = done;
    a.list = list;
    a.count = count;
    a.left = left;
    a.born = born;
    const dim3 grid((unsigned)((slots + a.bpw - 1) / a.bpw)), block((unsigned)(a.bpw * a.wpb * 64));
    const int rule = rules                             ? GOL_BATCH_RULE_EACH
                     : gol_batch_conway(birth, survive) ? GOL_BATCH_RULE_CONWAY
                                                        : GOL_BATCH_RULE_TABLE;
    switch (nw) {
    case 1: return launch_rule<1>(rule, scan, list != nullptr, a, grid, block, s);
    case 2: return launch_rule<2>(rule, scan, list != nullptr, a, grid, block, s);
    case 4: return launch_rule<4>(rule, scan, list != nullptr, a, grid, block, s);
    case 8: return launch_rule<8>(rule, scan, list != nullptr, a, grid, block, s);
    default: return launch_rule<16>(rule, scan, list != nullptr, a, grid, block, s);
    }
}

hipError_t golk_batch_step(uint64_t *boards, uint64_t *prev, int64_t *settled, int64_t n, int64_t H, int64_t W, int turns,
                           int64_t turn0, bool have_prev, bool write_prev, uint32_t birth, uint32_t survive,
                           const uint32_t *rules, int scan, int64_t done, hipStream_t s)
{
    return batch_launch(boards, prev, settled, n, H, W, turns, turn0, have_prev, write_prev, birth, survive, rules, scan, done,
                        nullptr, nullptr, n, nullptr, nullptr, s);
}

hipError_t golk_batch_step_list(uint64_t *boards, uint64_t *prev, int64_t *settled, int64_t n, int64_t H, int64_t W, int turns,
                                int64_t turn0, bool have_prev, bool write_prev, uint32_t birth, uint32_t survive,
                                const uint32_t *rules, int64_t done, const int32_t *list, const int32_t *count, int64_t slots,
                                int64_t *left, hipStream_t s)
{
    // the search (settled: the cycle scan of the listed boards) or the finish (left: each listed board's own turns)
    if (!list || !count || slots < 1 || slots > n || (settled != nullptr) == (left != nullptr)) return hipErrorInvalidValue;
    return batch_launch(boards, prev, settled, n, H, W, turns, turn0, have_prev, write_prev, birth, survive, rules,
                        settled ? GOL_BATCH_SCAN_CYCLES : GOL_BATCH_SCAN_NONE, done, list, count, slots, left, nullptr, s);
}

hipError_t golk_batch_step_aged(uint64_t *boards, uint64_t *prev, int64_t *found, const int64_t *born, int64_t n, int64_t H,
                                int64_t W, int turns, uint32_t birth, uint32_t survive, int64_t done, const int32_t *list,
                                const int32_t *count, int64_t slots, hipStream_t s)
{
    if (!list || !count || !found || !born || slots < 1 || slots > n) return hipErrorInvalidValue;
    return batch_launch(boards, prev, found, n, H, W, turns, 0, done > 0, true, birth, survive, nullptr, GOL_BATCH_SCAN_CYCLES,
                        done, list, count, slots, nullptr, born, s);
}

hipError_t golk_batch_iota(int32_t *list, int32_t *counts, int64_t n, hipStream_t s)
{
    if (!list || !counts || n < 1 || n > ((int64_t)1 << 20)) return hipErrorInvalidValue;
    batch_iota_kernel<<<(unsigned)std::min<int64_t>((n + 255) / 256, 1024), 256, 0, s>>>(list, counts, (int32_t)n);
    return hipGetLastError();
}

hipError_t golk_batch_retire(const int32_t *list_in, int32_t *counts, const int64_t *found, int64_t n, int64_t t0,
                             int64_t t_now, int64_t t_end, int32_t *active, int32_t *finish, int64_t *left, hipStream_t s)
{
    if (!list_in || !counts || !found || !active || !finish || !left || n < 1 || n > ((int64_t)1 << 20) || t0 > t_now ||
        t_now > t_end)
        return hipErrorInvalidValue;
    batch_retire_kernel<<<1, 1024, 0, s>>>(list_in, counts, found, n, t0, t_end - t_now, active, finish, left);
    return hipGetLastError();
}

hipError_t golk_batch_random(uint64_t *boards, int64_t n, int64_t H, int64_t W, uint64_t seed, hipStream_t s)
{
    if (!boards || n < 1 || H < 1 || H > GOL_BATCH_MAX_SIDE || W < 1 || W > GOL_BATCH_MAX_SIDE) return hipErrorInvalidValue;
    const int64_t Ww = (W + 63) / 64, words = n * H * Ww;
    const uint64_t tail = W % 64 ? ((uint64_t)1 << (W % 64)) - 1 : ~(uint64_t)0;
    const unsigned grid = (unsigned)std::min<int64_t>((words + 255) / 256, 8192);
    batch_random_kernel<<<grid, 256, 0, s>>>(boards, words, (int32_t)Ww, tail, seed);
    return hipGetLastError();
}

hipError_t golk_batch_reduce(bool hash, const uint64_t *boards, int64_t n, int64_t H, int64_t W, uint64_t *out, hipStream_t s)
{
    if (!boards || !out || n < 1 || H < 1 || H > GOL_BATCH_MAX_SIDE || W < 1 || W > GOL_BATCH_MAX_SIDE) return hipErrorInvalidValue;
    const int32_t words = (int32_t)(H * ((W + 63) / 64));
    const unsigned grid = (unsigned)std::min<int64_t>((n + 3) / 4, 8192);
    if (hash) batch_reduce_kernel<true><<<grid, 256, 0, s>>>(boards, n, words, out);
    else batch_reduce_kernel<false><<<grid, 256, 0, s>>>(boards, n, words, out);
    return hipGetLastError();
}

hipError_t golk_batch_soups(uint64_t *boards, int64_t n, int64_t H, int64_t W, uint64_t seed, int64_t first, hipStream_t s)
{
    if (!boards || n < 1 || H < 1 || H > GOL_BATCH_MAX_SIDE || W < 1 || W > GOL_BATCH_MAX_SIDE || first < 0 ||
        first > ((int64_t)1 << 40))
        return hipErrorInvalidValue;
    const int64_t Ww = (W + 63) / 64, words = n * H * Ww;
    const uint64_t tail = W % 64 ? ((uint64_t)1 << (W % 64)) - 1 : ~(uint64_t)0;
    const unsigned grid = (unsigned)std::min<int64_t>((words + 255) / 256, 8192);
    batch_soups_kernel<<<grid, 256, 0, s>>>(boards, words, (int32_t)Ww, tail, seed, (uint64_t)(first * H * Ww));
    return hipGetLastError();
}

hipError_t golk_batch_search_init(int32_t *active, int32_t *counts, int32_t *soup, int64_t *born, int64_t *found, int64_t m,
                                  hipStream_t s)
{
    if (!active || !counts || !soup || !born || !found || m < 1 || m > ((int64_t)1 << 20)) return hipErrorInvalidValue;
    batch_search_init_kernel<<<(unsigned)std::min<int64_t>((m + 255) / 256, 1024), 256, 0, s>>>(active, counts, soup, born, found,
                                                                                               (int32_t)m);
    return hipGetLastError();
}

hipError_t golk_batch_restock(int32_t *active, int32_t *counts, int64_t *found, int64_t *born, int32_t *soup, int64_t n,
                              int64_t now, int64_t horizon, int64_t total, int64_t *out_found, int64_t *out_period,
                              int32_t *harvest, hipStream_t s)
{
    if (!active || !counts || !found || !born || !soup || !out_found || !out_period || !harvest || n < 1 ||
        n > ((int64_t)1 << 20) || now < 0 || horizon < 0 || total < 0 || total > ((int64_t)1 << 26))
        return hipErrorInvalidValue;
    batch_restock_kernel<<<1, 1024, 0, s>>>(active, counts, found, born, soup, n, now, horizon, (int32_t)total, out_found,
                                            out_period, harvest);
    return hipGetLastError();
}

hipError_t golk_batch_harvest(const uint64_t *prev, const int32_t *harvest, const int32_t *counts, int64_t n, int64_t H,
                              int64_t W, int64_t total, const int64_t *found, uint64_t *alive, uint64_t *hash, int64_t slots,
                              hipStream_t s)
{
    if (!prev || !harvest || !counts || !found || !alive || !hash || n < 1 || n > ((int64_t)1 << 20) || H < 1 ||
        H > GOL_BATCH_MAX_SIDE || W < 1 || W > GOL_BATCH_MAX_SIDE || total < 0 || total > ((int64_t)1 << 26) || slots < 1 ||
        slots > n)
        return hipErrorInvalidValue;
    const unsigned grid = (unsigned)std::min<int64_t>((slots + 3) / 4, 8192);
    batch_harvest_kernel<<<grid, 256, 0, s>>>(prev, harvest, counts, n, (int32_t)(H * ((W + 63) / 64)), (int32_t)total, found,
                                              alive, hash);
    return hipGetLastError();
}

hipError_t golk_batch_refill(uint64_t *boards, const int32_t *harvest, const int32_t *counts, const int32_t *soup, int64_t n,
                             int64_t H, int64_t W, uint64_t seed, int64_t first, int64_t total, int64_t slots, hipStream_t s)
{
    if (!boards || !harvest || !counts || !soup || n < 1 || n > ((int64_t)1 << 20) || H < 1 || H > GOL_BATCH_MAX_SIDE || W < 1 ||
        W > GOL_BATCH_MAX_SIDE || first < 0 || total < 0 || total > ((int64_t)1 << 26) || first + total > ((int64_t)1 << 40) ||
        slots < 1 || slots > n)
        return hipErrorInvalidValue;
    const int64_t Ww = (W + 63) / 64, words = H * Ww;
    const uint64_t tail = W % 64 ? ((uint64_t)1 << (W % 64)) - 1 : ~(uint64_t)0;
    const unsigned grid = (unsigned)std::min<int64_t>((slots * words + 255) / 256, 8192);
    batch_refill_kernel<<<grid, 256, 0, s>>>(boards, harvest, counts, soup, n, (int32_t)words, (int32_t)Ww, tail, seed,
                                             (uint64_t)first, (int32_t)total);
    return hipGetLastError();
}
