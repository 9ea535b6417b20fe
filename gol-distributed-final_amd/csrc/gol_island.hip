// gol_island.hip -- the island census of a batch of small tori in one launch (include/golhip.h, "the island census of
// a batch"; the row functions are gol_island.h).
//
// batch_islands_kernel<NW, REACH>: one board per workgroup of ceil(H / 64) waves, one row per lane, NW = 1, 2, 4, 8 or
// 16 words of it in registers, as in the step kernel (gol_batch.hip).  The board is read once and stays resident: a
// lane holds its row's remaining cells and the window rows (gol_island_window_row) of the 2 REACH + 1 board rows (y +
// dy) mod H round it, read straight from memory; they are constant, so the fingerprint needs no lane exchange.  (At
// NW = 16 and reach 2 the window rows do not fit the registers: there they are read again per island, by the lanes
// that hold cells of it.)
// Per island:
//   - the seed is the lowest remaining alive cell in row-major order: a ballot and a lane read per wave, the waves'
//     candidates through LDS, the minimum taken by every wave alike;
//   - the flood: M = {seed}, then M' = rem & dilation of M (gol_island_dilate) until no wave reports a change.  The
//     rows of M above and below come by DPP (wave_shr:1 / wave_shl:1, twice at reach 2); a lane whose neighbour row
//     lies outside its wave (or round the torus) reads it from LDS, where every wave posts the rows of its first two
//     and last two lanes, double-buffered, so a step has one __syncthreads().  A wave's "changed" bit of the step
//     before travels under the same barrier, so the flood ends one barrier after its last step, for every wave alike;
//   - the reduction: one uniform loop per wave over its lanes that hold cells of M (lane reads: the population, the OR
//     of the words for the columns, the sum of the lanes' hashes, gol_island_row_hash), the waves' parts and the next
//     seed's candidates through LDS under one barrier; thread 0 writes the record (if it is within cap) and sums the
//     fingerprint;
//   - M leaves the remaining cells.
// Synchronisation is __syncthreads() alone: no atomic, no flag between workgroups, no spin loop.  Every barrier is
// reached by every wave: every loop that holds one ends on a value all waves read from LDS after the same barrier.
// The DPP moves run with all lanes active, outside divergent branches; no register array is indexed by a variable.
// Both loops carry a hard trip bound of H W (an island has at most H W cells, a board at most H W islands, and every
// flood step but the last adds a cell): it cannot be reached, and a board that hit it would report count = -1.
//
// This unit holds the kernel, the dispatch over its ten instantiations and its one entry, golk_batch_islands, which
// launches what a gol_island_launch describes once gol_island_launch_ok accepts it.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gol_device.h"
#include "gol_island.h"

namespace {

struct IslandArgs {
    const uint64_t *boards;  // n boards of H rows of Ww uint64 words, dense; only read
    gol_batch_row g;
    int32_t H, W, Ww, wpb;  // rows, cells and uint64 words per row, waves per board
    int64_t cap;
    int64_t *count;
    gol_island *islands;
    uint64_t *fingerprint;
};

constexpr uint32_t NO_SEED = ~0u;

template <int NW>
__device__ __forceinline__ void load_row(const uint64_t *row, int32_t Ww, bool on, const gol_batch_row &g, uint32_t (&c)[NW])
{
    const uint32_t *p = (const uint32_t *)row;
#pragma unroll
    for (int j = 0; j < NW; ++j) c[j] = (on && j < 2 * Ww ? p[j] : 0u) & gol_island_keep(g, j);
}

// A neighbour row of M that lies outside the wave: row yy of the board, from the rows the waves posted.
template <int NW>
__device__ __forceinline__ void posted_row(const uint32_t (&edge)[GOL_BATCH_MAX_WAVES][4][NW], int yy, int H, uint32_t (&t)[NW])
{
    const int ww = yy >> 6, ll = yy & 63, lw = min(63, H - 1 - ww * 64);
    const int slot = ll == 0 ? 0 : (ll == 1 ? 1 : (ll == lw ? 3 : 2));
#pragma unroll
    for (int j = 0; j < NW; ++j) t[j] = edge[ww][slot][j];
}

template <int NW, int REACH>
__global__ __launch_bounds__(512) void batch_islands_kernel(const IslandArgs a)
{
    // [buffer][wave][lane 0, lane 1, the last lane but one, the last lane][word]
    __shared__ uint32_t edge[2][GOL_BATCH_MAX_WAVES][4][NW];
    __shared__ uint32_t changed[2][GOL_BATCH_MAX_WAVES];
    __shared__ uint32_t cand[2][GOL_BATCH_MAX_WAVES];
    __shared__ uint32_t part_cells[2][GOL_BATCH_MAX_WAVES], part_rows[2][GOL_BATCH_MAX_WAVES];
    __shared__ uint32_t part_cols[2][GOL_BATCH_MAX_WAVES][NW];
    __shared__ uint64_t part_hash[2][GOL_BATCH_MAX_WAVES];
    __shared__ uint64_t fingerprint;  // the sum of the records' hashes so far

    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t board = blockIdx.x;
    const int H = a.H;
    const int y = wave * 64 + lane;
    const int last = min(63, H - 1 - wave * 64);  // the wave's last lane with a row (>= 0)
    const bool on = y < H;
    const gol_batch_row g = a.g;
    const uint64_t *rows = a.boards + board * H * a.Ww;

    uint32_t rem[NW];                      // the row's cells not yet in an island
    uint32_t win[2 * REACH + 1][NW + 1];  // the window rows of the board rows (y + dy) mod H
    load_row<NW>(rows + (on ? (int64_t)y * a.Ww : 0), a.Ww, on, g, rem);
    auto load_windows = [&](uint32_t (&e)[2 * REACH + 1][NW + 1]) {
#pragma unroll
        for (int d = 0; d < 2 * REACH + 1; ++d) {
            const int yy = on ? ((y + d - REACH) % H + H) % H : 0;
            uint32_t c[NW];
            load_row<NW>(rows + (int64_t)yy * a.Ww, a.Ww, on, g, c);
            gol_island_window_row<NW, REACH>(c, g, a.W, e[d]);
        }
    };
    // The window rows stay in registers for the whole launch, but at NW = 16 and reach 2, where the 85 of them do not
    // fit beside the flood's rows (the kernel would spill): there a lane that holds cells of an island reads them again
    // when it hashes them (the only second read of a board; it meets the cache).
    constexpr bool RESIDENT = (2 * REACH + 1) * (NW + 1) <= 64;
    if (RESIDENT) load_windows(win);

    // the wave's lowest remaining cell as y << 10 | x (all lanes active)
    auto candidate = [&]() -> uint32_t {
        uint32_t any = 0, x = 0;
#pragma unroll
        for (int j = NW - 1; j >= 0; --j) {
            any |= rem[j];
            x = rem[j] ? (uint32_t)(j * 32 + __builtin_ctz(rem[j])) : x;
        }
        const uint64_t has = __ballot(any != 0);
        if (!has) return NO_SEED;  // (uniform)
        const int first = __builtin_amdgcn_readfirstlane(__builtin_ctzll(has));
        return (uint32_t)(wave * 64 + first) << 10 | (uint32_t)__builtin_amdgcn_readlane((int)x, first);
    };
    auto lowest = [&](int par) -> uint32_t {
        uint32_t s = NO_SEED;
        for (int i = 0; i < a.wpb; ++i) s = min(s, cand[par][i]);
        return s;
    };

    const int bound = H * a.W;  // (at most 2^18)
    int buf = 0, par = 0;
    {
        const uint32_t c = candidate();
        if (lane == 0) cand[par][wave] = c;
    }
    __syncthreads();
    uint32_t seed = lowest(par);  // uniform over the workgroup, like everything the loops end on
    par ^= 1;
    int k = 0;
    if (threadIdx.x == 0) fingerprint = 0;  // (thread 0's alone, kept out of the registers, which are short at NW = 16)
    bool over = false;
    while (seed != NO_SEED) {
        if (k == bound) {
            over = true;
            break;
        }
        const int sy = (int)(seed >> 10), sx = (int)(seed & 1023u);
        uint32_t m[NW];
#pragma unroll
        for (int j = 0; j < NW; ++j) m[j] = y == sy && j == (sx >> 5) ? 1u << (sx & 31) : 0u;
        bool mine = false;  // this wave's "a word changed" of the step just made
        for (int s = 0;; ++s) {
            if (lane == 0) {
                changed[buf][wave] = mine;
#pragma unroll
                for (int j = 0; j < NW; ++j) edge[buf][wave][0][j] = m[j];
            }
            if (lane == 1) {
#pragma unroll
                for (int j = 0; j < NW; ++j) edge[buf][wave][1][j] = m[j];
            }
            if (lane == last - 1) {
#pragma unroll
                for (int j = 0; j < NW; ++j) edge[buf][wave][2][j] = m[j];
            }
            if (lane == last) {
#pragma unroll
                for (int j = 0; j < NW; ++j) edge[buf][wave][3][j] = m[j];
            }
            __syncthreads();
            if (s > 0) {
                bool any = false;
                for (int i = 0; i < a.wpb; ++i) any |= changed[buf][i] != 0;
                if (!any) break;
            }
            if (s == bound) {
                over = true;
                break;
            }
            // the OR of the rows (y + dy) mod H of M
            uint32_t v[NW], nb[NW];
#pragma unroll
            for (int j = 0; j < NW; ++j) v[j] = nb[j] = m[j];
#pragma unroll
            for (int r = 1; r <= REACH; ++r) {  // the rows y - r
                uint32_t t[NW];
#pragma unroll
                for (int j = 0; j < NW; ++j) t[j] = nb[j] = golk::from_lower_lane(nb[j]);
                if (on && lane - r < 0) posted_row<NW>(edge[buf], ((y - r) % H + H) % H, H, t);
#pragma unroll
                for (int j = 0; j < NW; ++j) v[j] |= t[j];
            }
#pragma unroll
            for (int j = 0; j < NW; ++j) nb[j] = m[j];
#pragma unroll
            for (int r = 1; r <= REACH; ++r) {  // the rows y + r
                uint32_t t[NW];
#pragma unroll
                for (int j = 0; j < NW; ++j) t[j] = nb[j] = golk::from_upper_lane(nb[j]);
                if (on && lane + r > last) posted_row<NW>(edge[buf], (y + r) % H, H, t);
#pragma unroll
                for (int j = 0; j < NW; ++j) v[j] |= t[j];
            }
            uint32_t next[NW], d = 0;
            gol_island_dilate<NW, REACH>(rem, v, g, next);  // (a lane without a row has no cells)
#pragma unroll
            for (int j = 0; j < NW; ++j) {
                d |= next[j] ^ m[j];
                m[j] = next[j];
            }
            mine = __ballot(d != 0) != 0;
            buf ^= 1;
        }
        if (over) break;
        buf ^= 1;

        // the island is M: off the remaining cells, and its parts from this wave's lanes that hold cells of it
        uint32_t any = 0, pop = 0;
#pragma unroll
        for (int j = 0; j < NW; ++j) {
            rem[j] &= ~m[j];
            any |= m[j];
            pop += (uint32_t)__popc(m[j]);
        }
        uint64_t h = 0;
        if (any) {
            if (!RESIDENT) load_windows(win);
            h = gol_island_row_hash<NW, REACH>(m, win);
        }
        const uint64_t holds = __ballot(any != 0);
        uint32_t cells = 0, cols[NW];
        uint64_t hash = 0;
#pragma unroll
        for (int j = 0; j < NW; ++j) cols[j] = 0u;
        for (uint64_t left = holds; left; left &= left - 1) {  // (uniform in the wave; at most 64 trips)
            const int l = __builtin_amdgcn_readfirstlane(__builtin_ctzll(left));
            cells += (uint32_t)__builtin_amdgcn_readlane((int)pop, l);
            hash += (uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)h, l) |
                    (uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(h >> 32), l) << 32;
#pragma unroll
            for (int j = 0; j < NW; ++j) cols[j] |= (uint32_t)__builtin_amdgcn_readlane((int)m[j], l);
        }
        const uint32_t c = candidate();
        if (lane == 0) {
            part_cells[par][wave] = cells;
            part_rows[par][wave] = (uint32_t)__popcll(holds);
            part_hash[par][wave] = hash;
#pragma unroll
            for (int j = 0; j < NW; ++j) part_cols[par][wave][j] = cols[j];
            cand[par][wave] = c;
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            gol_island r = {sy, sx, 0, 0, 0, 0};
            uint32_t nrows = 0, ncols = 0;
            for (int i = 0; i < a.wpb; ++i) {
                r.cells += (int32_t)part_cells[par][i];
                nrows += part_rows[par][i];
                r.hash += part_hash[par][i];
            }
#pragma unroll
            for (int j = 0; j < NW; ++j) {
                uint32_t w = 0;
                for (int i = 0; i < a.wpb; ++i) w |= part_cols[par][i][j];
                ncols += (uint32_t)__popc(w);
            }
            r.rows = (uint16_t)nrows;
            r.cols = (uint16_t)ncols;
            fingerprint += r.hash;
            if (k < a.cap) a.islands[board * a.cap + k] = r;
        }
        seed = lowest(par);
        par ^= 1;
        ++k;
    }
    if (threadIdx.x == 0) {
        a.count[board] = over ? -1 : k;
        if (a.fingerprint) a.fingerprint[board] = fingerprint;
    }
}

template <int NW>
hipError_t launch(int reach, const IslandArgs &a, dim3 grid, dim3 block, hipStream_t s)
{
    if (reach == 1) batch_islands_kernel<NW, 1><<<grid, block, 0, s>>>(a);
    else batch_islands_kernel<NW, 2><<<grid, block, 0, s>>>(a);
    return hipGetLastError();
}

}  // namespace

hipError_t golk_batch_islands(const gol_island_launch &l, hipStream_t s)
{
    if (!gol_island_launch_ok(l)) return hipErrorInvalidValue;
    const gol_batch_row g = gol_batch_row_init(l.W);
    const int wpb = (int)((l.H + 63) / 64);
    const IslandArgs a = {l.boards, g, (int32_t)l.H, (int32_t)l.W, (int32_t)((l.W + 63) / 64), wpb, l.cap, l.count, l.islands,
                          l.fingerprint};
    const dim3 grid((unsigned)l.n), block((unsigned)(wpb * 64));
    switch (g.nw) {
    case 1: return launch<1>(l.reach, a, grid, block, s);
    case 2: return launch<2>(l.reach, a, grid, block, s);
    case 4: return launch<4>(l.reach, a, grid, block, s);
    case 8: return launch<8>(l.reach, a, grid, block, s);
    default: return launch<16>(l.reach, a, grid, block, s);
    }
}
