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
// This unit holds the step kernel, the dispatch over its 85 instantiations and its one entry, golk_batch_step, which
// launches what a gol_batch_launch describes once gol_batch_launch_ok (gol_batch.h) accepts it.  The small kernels round
// it (fills, census, the passes between the launches of a call) are gol_batch_pass.hip.  What the kernel shares with the
// MAP kernel (gol_batch_map.hip) outside its body -- the arguments, a lane's row load and store, the launch code -- is
// gol_batch_args.h.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <cstddef>

#define GOL_BATCH_CONWAY golk::rule  // B3/S23 on the step kernels' 7 gates
#include "gol_batch_args.h"

namespace {

using golk::load_row;
using golk::store_row;

// (aligned to 4 bytes, so that the masks stand right after write_prev as they always did; pad puts the pointer at a
// multiple of 8 in the arguments)
struct __attribute__((packed, aligned(4))) RuleParams {
    uint32_t birth, survive, pad;
    const uint32_t *rules;  // GOL_BATCH_RULE_EACH: n pairs (birth, survive)
};
using BatchArgs = golk::BatchArgs<RuleParams>;
static_assert((offsetof(BatchArgs, rule) + offsetof(RuleParams, rules)) % 8 == 0, "rules is aligned in the kernel's arguments");

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
    uint32_t birth = a.rule.birth, survive = a.rule.survive;
    if (RULE == GOL_BATCH_RULE_EACH) {
        const uint32_t i = __builtin_amdgcn_readfirstlane((uint32_t)(board < a.n ? board : a.n - 1));
        birth = __builtin_amdgcn_readfirstlane(a.rule.rules[2 * (size_t)i]);
        survive = __builtin_amdgcn_readfirstlane(a.rule.rules[2 * (size_t)i + 1]);
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

// The 17 modes of a launch, (RULE, SCAN, LIST, AGED): per rule plain, settle, cycles, list + cycles and the finish; the
// aged search under one rule for the batch (a rule per soup is not built).  With the five NW: 85 instantiations.
template <int NW>
hipError_t launch(int rule, int scan, bool list, bool aged, const BatchArgs &a, dim3 grid, dim3 block, hipStream_t s)
{
#define MODE(RULE, SCAN, LIST, AGED)                                                                                    \
    if (rule == GOL_BATCH_RULE_##RULE && scan == GOL_BATCH_SCAN_##SCAN && list == LIST && aged == AGED) {               \
        batch_step_kernel<NW, GOL_BATCH_RULE_##RULE, GOL_BATCH_SCAN_##SCAN, LIST, AGED><<<grid, block, 0, s>>>(a);      \
        return hipGetLastError();                                                                                       \
    }
#define MODES_OF(RULE) \
    MODE(RULE, NONE, false, false) MODE(RULE, SETTLE, false, false) MODE(RULE, CYCLES, false, false) \
    MODE(RULE, CYCLES, true, false) MODE(RULE, NONE, true, false)
    MODES_OF(CONWAY) MODES_OF(TABLE) MODES_OF(EACH)
    MODE(CONWAY, CYCLES, true, true) MODE(TABLE, CYCLES, true, true)
#undef MODES_OF
#undef MODE
    return hipErrorInvalidValue;
}

}  // namespace

void golk_batch_shape(int64_t H, int64_t W, int *waves_per_board, int *boards_per_wg, int *words_per_lane)
{
    const int wpb = (int)((H + 63) / 64);
    *waves_per_board = wpb;
    *boards_per_wg = std::max(1, 4 / wpb);
    *words_per_lane = gol_batch_row_init(W).nw;
}

hipError_t golk_batch_step(const gol_batch_launch &l, hipStream_t s)
{
    if (!gol_batch_launch_ok(l)) return hipErrorInvalidValue;
    if (l.maps) return golk_batch_map_step(l, s);  // MAP rules: the kernel unit of their own (gol_batch_map.hip)
    const BatchArgs a = golk::batch_args(l, RuleParams{l.birth, l.survive, 0, l.rules});
    dim3 grid, block;
    golk::batch_grid(l, a.wpb, a.bpw, &grid, &block);
    const int rule = l.rules                               ? GOL_BATCH_RULE_EACH
                     : gol_batch_conway(l.birth, l.survive) ? GOL_BATCH_RULE_CONWAY
                                                            : GOL_BATCH_RULE_TABLE;
    return golk::with_nw(a.g.nw, [&](auto nw) {
        return launch<decltype(nw)::value>(rule, l.scan, l.list != nullptr, l.born != nullptr, a, grid, block, s);
    });
}
