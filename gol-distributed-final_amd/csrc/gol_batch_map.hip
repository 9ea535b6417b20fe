// gol_batch_map.hip -- the batch's step kernel for MAP rules (include/golhip.h, "MAP rules of a batch"; the row
// function and the circuit are gol_map.h): any two-state rule of the 3x3 block as a table of 512 bits, one for the
// batch or one per board.
//
// batch_map_kernel<NW, SCAN, LIST, AGED> has the layout and the modes of batch_step_kernel (gol_batch.hip, whose header
// describes them): one row per lane in NW = 1, 2, 4, 8 or 16 words, ceil(H / 64) waves per board, boards of up to 128
// rows share a workgroup; the board is read once, stepped `turns` times in registers and written once, in place.
// What differs is what a turn passes round.  A map sees the nine cells and not their count, so a lane takes the raw
// words of the rows above and below from the neighbouring lanes by DPP (NW moves each way, where the step kernel moves
// 2 NW sums) and forms their left and right planes itself; a wave's first and last row cross a wave, or wrap round the
// torus, through LDS ([2][waves][2][NW], double-buffered), so a turn has one __syncthreads(), which also carries the
// scan's "differs" bits.  The scans (settle, cycles with the Brent marks), the list, the finish with left[] and the
// aged mode are batch_step_kernel's, statement by statement: a change to one is a change to both.  (One body under a
// rule policy was built and left out: as a function inlined into two kernels of these names it did not compile to the
// instructions of either)  The arguments, a lane's row load and store and the launch code are shared:
// gol_batch_args.h.
// The board's map is read once per launch by scalar loads, 16 dwords from maps + (map_each ? 16 board : 0), the board's
// number made uniform as for the per-board rule read, so the table bits that select the circuit's leaves are
// wave-uniform.
// Synchronisation is __syncthreads() alone: no workgroup waits for another one, there is no flag between workgroups,
// no spin loop and no atomic.  Every wave of a workgroup runs every barrier (a wave whose board is past the batch's
// end computes on zeros and stores nothing).
//
// This unit holds the kernel, the dispatch over its 30 instantiations (five NW x plain, settle, cycles, list + cycles,
// the finish, aged) and its entry, golk_batch_map_step, to which golk_batch_step (gol_batch.hip) hands a launch
// that has maps.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gol_batch_args.h"
#include "gol_map.h"

namespace {

using golk::load_row;
using golk::store_row;

struct MapParams {
    const uint32_t *maps;  // 16 words, or map_each: n times 16
    int32_t map_each;
};
using MapArgs = golk::BatchArgs<MapParams>;

template <int NW, int SCAN, bool LIST, bool AGED>
__global__ __launch_bounds__(512) void batch_map_kernel(const MapArgs a)
{
    // [buffer][wave][first / last row of the wave][word]
    __shared__ uint32_t edge[2][GOL_BATCH_MAX_WAVES][2][NW];
    __shared__ uint32_t differs[2][GOL_BATCH_MAX_WAVES];

    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int lb = wave / a.wpb, w = wave - lb * a.wpb;  // the board's slot in the workgroup, the wave's in the board
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
    // the board's own map: the board's index is wave-uniform, and made scalar it turns the reads into scalar loads
    // (a wave past the batch's end, or without a board, reads a map that exists and computes on zeros)
    uint32_t map[GOL_MAP_WORDS];
    {
        const uint32_t i = __builtin_amdgcn_readfirstlane((uint32_t)(a.rule.map_each ? (has && board < a.n ? board : 0) : 0));
        const uint32_t *mp = a.rule.maps + GOL_MAP_WORDS * (size_t)i;
#pragma unroll
        for (int j = 0; j < GOL_MAP_WORDS; ++j) map[j] = __builtin_amdgcn_readfirstlane(mp[j]);
    }

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
        uint32_t up[NW], dn[NW], next[NW];
        if (lane == 0) {
#pragma unroll
            for (int j = 0; j < NW; ++j) edge[buf][wave][0][j] = cur[j];
        }
        if (lane == last) {
#pragma unroll
            for (int j = 0; j < NW; ++j) edge[buf][wave][1][j] = cur[j];
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
            up[j] = golk::from_lower_lane(cur[j]);
            dn[j] = golk::from_upper_lane(cur[j]);
        }
        if (lane == 0) {
#pragma unroll
            for (int j = 0; j < NW; ++j) up[j] = edge[buf][wup][1][j];
        }
        if (lane == last) {
#pragma unroll
            for (int j = 0; j < NW; ++j) dn[j] = edge[buf][wdn][0][j];
        }
        gol_batch_map_next<NW>(map, g, up, cur, dn, msk, next);
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

// The six modes of a launch, (SCAN, LIST, AGED): plain, settle, cycles, list + cycles, the finish and the aged search.
// With the five NW: 30 instantiations.
template <int NW>
hipError_t launch(int scan, bool list, bool aged, const MapArgs &a, dim3 grid, dim3 block, hipStream_t s)
{
#define MODE(SCAN, LIST, AGED)                                                                  \
    if (scan == GOL_BATCH_SCAN_##SCAN && list == LIST && aged == AGED) {                        \
        batch_map_kernel<NW, GOL_BATCH_SCAN_##SCAN, LIST, AGED><<<grid, block, 0, s>>>(a);      \
        return hipGetLastError();                                                               \
    }
    MODE(NONE, false, false) MODE(SETTLE, false, false) MODE(CYCLES, false, false)
    MODE(CYCLES, true, false) MODE(NONE, true, false) MODE(CYCLES, true, true)
#undef MODE
    return hipErrorInvalidValue;
}

}  // namespace

hipError_t golk_batch_map_step(const gol_batch_launch &l, hipStream_t s)
{
    if (!gol_batch_launch_ok(l) || !l.maps) return hipErrorInvalidValue;
    const MapArgs a = golk::batch_args(l, MapParams{l.maps, l.map_each});
    dim3 grid, block;
    golk::batch_grid(l, a.wpb, a.bpw, &grid, &block);
    return golk::with_nw(a.g.nw, [&](auto nw) {
        return launch<decltype(nw)::value>(l.scan, l.list != nullptr, l.born != nullptr, a, grid, block, s);
    });
}
