// gol_batch_args.h -- what the batch's two step kernel units share outside their kernels' bodies (gol_batch.hip: the
// life-like rules, B/S; gol_batch_map.hip: the MAP rules): the kernel arguments, which differ in the rule's fields
// alone, a lane's row load and store, and the host side of a launch: the arguments of a launch descriptor, the grid and
// the dispatch over the words per lane.  The kernels themselves, whose layout and modes gol_batch.hip's header
// describes, are each in its unit.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "gol_device.h"
#include "gol_batch.h"
#include "gol_batch_kernels.h"

namespace golk {

template <class P>
struct BatchArgs {
    uint64_t *boards;  // n boards of H rows of Ww uint64 words, dense; stepped in place
    uint64_t *prev;    // SCAN: state(start - 1) or the snapshot in (have_prev) and out (write_prev); same shape
    int64_t *settled;  // SCAN: n turns, -1 = not found yet
    int64_t n, turn0;  // boards; the turn of the loaded state
    gol_batch_row g;
    int32_t H, Ww, wpb, bpw;  // rows, uint64 words per row, waves per board, boards per workgroup
    int32_t turns;            // >= 1
    int32_t have_prev, write_prev;
    P rule;        // the unit's own fields: the masks and the rules per board, or the maps
    int64_t done;  // GOL_BATCH_SCAN_CYCLES: the turns of the call before this launch
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

// The kernel arguments of a launch that gol_batch_launch_ok accepts, `rule` the unit's own fields of it.
template <class P>
BatchArgs<P> batch_args(const gol_batch_launch &l, const P &rule)
{
    int wpb, bpw, nw;
    golk_batch_shape(l.H, l.W, &wpb, &bpw, &nw);
    return {l.boards, l.prev, l.settled, l.n, l.turn0, gol_batch_row_init(l.W), (int32_t)l.H, (int32_t)((l.W + 63) / 64),
            wpb, bpw, l.turns, l.have_prev, l.write_prev, rule, l.done, l.list, l.count, l.left, l.born};
}

// The launch's grid: a workgroup per bpw board slots, a wave per 64 rows of each.
inline void batch_grid(const gol_batch_launch &l, int wpb, int bpw, dim3 *grid, dim3 *block)
{
    const int64_t slots = l.list ? l.slots : l.n;  // without a list every board has its slot
    *grid = dim3((unsigned)((slots + bpw - 1) / bpw));
    *block = dim3((unsigned)(bpw * wpb * 64));
}

// f(std::integral_constant<int, NW>()) for the words per lane of a row, nw = 1, 2, 4, 8 or 16.
template <class F>
hipError_t with_nw(int nw, F f)
{
    switch (nw) {
    case 1: return f(std::integral_constant<int, 1>());
    case 2: return f(std::integral_constant<int, 2>());
    case 4: return f(std::integral_constant<int, 4>());
    case 8: return f(std::integral_constant<int, 8>());
    default: return f(std::integral_constant<int, 16>());
    }
}

}  // namespace golk
