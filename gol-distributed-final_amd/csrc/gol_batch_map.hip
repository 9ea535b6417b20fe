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
// aged mode are batch_step_kernel's, statement by statement.
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

#include <algorithm>

#include "gol_device.h"
#include "gol_kernels.h"
#include "gol_map.h"

namespace {

struct MapArgs {
    uint64_t *boards;  // n boards of H rows of Ww uint64 words, dense; stepped in place
    uint64_t *prev;    // SCAN: state(start - 1) or the snapshot in (have_prev) and out (write_prev); same shape
    int64_t *settled;  // SCAN: n turns, -1 = not found yet
    int64_t n, turn0;  // boards; the turn of the loaded state
    gol_batch_row g;
    int32_t H, Ww, wpb, bpw;  // rows, uint64 words per row, waves per board, boards per workgroup
    int32_t turns;            // >= 1
    int32_t have_prev, write_prev;
    const uint32_t *maps;  // 16 words, or map_each: n times 16
    int32_t map_each;
    int64_t done;  // GOL_BATCH_SCAN_CYCLES: the turns of the call before this launch
    const int32_t *list, *count;
    int64_t *left;
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
        const uint32_t i = __builtin_amdgcn_readfirstlane((uint32_t)(a.map_each ? (has && board < a.n ? board : 0) : 0));
        const uint32_t *mp = a.maps + GOL_MAP_WORDS * (size_t)i;
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
    int wpb, bpw, nw;
    golk_batch_shape(l.H, l.W, &wpb, &bpw, &nw);
    const MapArgs a = {l.boards, l.prev, l.settled, l.n, l.turn0, gol_batch_row_init(l.W), (int32_t)l.H, (int32_t)((l.W + 63) / 64),
                       wpb, bpw, l.turns, l.have_prev, l.write_prev, l.maps, l.map_each, l.done, l.list, l.count, l.left, l.born};
    const int64_t slots = l.list ? l.slots : l.n;  // without a list every board has its slot
    const dim3 grid((unsigned)((slots + a.bpw - 1) / a.bpw)), block((unsigned)(a.bpw * a.wpb * 64));
    switch (nw) {
    case 1: return launch<1>(l.scan, l.list != nullptr, l.born != nullptr, a, grid, block, s);
    case 2: return launch<2>(l.scan, l.list != nullptr, l.born != nullptr, a, grid, block, s);
    case 4: return launch<4>(l.scan, l.list != nullptr, l.born != nullptr, a, grid, block, s);
    case 8: return launch<8>(l.scan, l.list != nullptr, l.born != nullptr, a, grid, block, s);
    default: return launch<16>(l.scan, l.list != nullptr, l.born != nullptr, a, grid, block, s);
    }
}
