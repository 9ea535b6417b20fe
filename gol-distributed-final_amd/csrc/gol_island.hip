// gol_island.hip -- the island census of a batch of small tori in one launch (include/golhip.h, "the island census of
// a batch"; the row functions are gol_island.h).
//
// batch_islands_kernel<NW, REACH, TALLY, FREE>: one board per workgroup of ceil(H / 64) waves, one row per lane, NW = 1, 2, 4, 8 or
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
// Synchronisation is __syncthreads() alone: no flag between workgroups, no spin loop, and in the plain instantiations
// (TALLY = false) no atomic.  Every barrier is reached by every wave: every loop that holds one ends on a value all waves
// read from LDS after the same barrier.
// The DPP moves run with all lanes active, outside divergent branches; no register array is indexed by a variable.
// Both loops carry a hard trip bound of H W (an island has at most H W cells, a board at most H W islands, and every
// flood step but the last adds a cell): it cannot be reached, and a board that hit it would report count = -1.
//
// TALLY = true (include/golhip.h, "the tally of island kinds"): no record array; every finished island goes into a
// table of kinds in global memory instead, under its owner.  The board is board blockIdx.x (dense), or the slot of pair
// blockIdx.x of a device list of (slot, soup) pairs whose length is in device memory (listed: one uniform scalar branch,
// not another instantiation); a workgroup past the length, or whose soup expired, leaves before its first barrier.
// Thread 0 gathers the records in LDS, GOL_ISLAND_TALLY_BUFFER of them; wave 0, in which thread 0 runs, inserts a full
// buffer, and the remainder at the board's end, one lane per record, the equal hashes of a buffer merged first so that
// one lane inserts for all of them (tally_flush; DESIGN.md 4.24 has what that bought): a probe from the kind's home
// slot with a 64-bit compare-and-swap on the tag where it reads 0, an atomic add on the count, an atomic minimum on
// the first owner and on the packed shape only where a load shows the new value is lower.  Every field is a
// commutative reduction, so no workgroup waits for another and the table's contents do not depend on the order; a
// full table is counted in `dropped`.  The buffer is wave 0's alone and an insertion holds no barrier, so the barriers
// are those of the plain form.
//
// FREE = true (include/golhip.h, "island kinds free of orientation"): the hash of an island is the smallest of its
// sums in the eight orientations of the square.  A lane that holds cells of M accumulates eight sums
// (gol_island_row_hash_free: per cell the code in its eight orientations, gol_island_orient_all, and eight terms), the
// uniform loop over the holding lanes reads all eight, the waves post eight parts each, and thread 0 adds them and
// takes the minimum (gol_island_free_hash) before it writes the record, the fingerprint and the gathered record.
// Nothing after that differs: no barrier, atomic or loop is added, and the table sees a hash as before.
//
// This unit holds the kernel, the dispatch over its forty instantiations, the kernel that empties a table, and its
// entries: golk_batch_islands, which launches what a gol_island_launch describes once gol_island_launch_ok accepts it,
// and golk_island_table_clear.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "gol_device.h"
#include "gol_batch_kernels.h"
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
    // TALLY
    gol_island_slot *table;
    int32_t log2;
    unsigned long long *dropped;
    int64_t owner0, n;
    const int32_t *pairs, *pair_count;
    const int64_t *found;
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

// `add` islands of one kind and one owner, `shape` their smallest, into the table (a lane of wave 0; the others run
// beside it or are masked off).
__device__ __forceinline__ void tally_insert(const IslandArgs &a, uint64_t hash, uint64_t shape, uint64_t owner, uint64_t add)
{
    typedef unsigned long long u64;
    const uint64_t tag = gol_island_tally_tag(hash), slots = (uint64_t)1 << a.log2;
    uint64_t at = gol_island_tally_home(tag, a.log2);
    for (uint64_t tries = 0; tries < slots; ++tries, at = gol_island_tally_next(at, a.log2)) {
        gol_island_slot *p = a.table + at;
        uint64_t seen = __hip_atomic_load(&p->hash, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (seen == 0) seen = atomicCAS((u64 *)&p->hash, (u64)0, (u64)tag);  // (the value before: 0 where this lane claimed it)
        if (seen != 0 && seen != tag) continue;
        atomicAdd((u64 *)&p->count, (u64)add);
        if (__hip_atomic_load(&p->first, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) > owner) atomicMin((u64 *)&p->first, (u64)owner);
        if (__hip_atomic_load(&p->shape, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) > shape) atomicMin((u64 *)&p->shape, (u64)shape);
        return;
    }
    atomicAdd(a.dropped, (u64)add);  // every slot holds another kind
}

// The n gathered records into the table, lane l < n holding record l (all of wave 0; n is uniform).  Equal hashes are
// merged first: every lane counts its hash among the n and takes their smallest shape (broadcast reads of LDS), and
// the first lane of a kind inserts for all of them.  A board's commonest kinds come several to a buffer, and every
// atomic on a kind goes to one slot's cache line, whatever the workgroup: the merge takes that many off it.
__device__ __forceinline__ void tally_flush(const IslandArgs &a, const uint64_t (*kept)[2], int lane, int n, uint64_t owner)
{
    const bool on = lane < n;
    const uint64_t hash = kept[on ? lane : 0][0];
    uint64_t shape = kept[on ? lane : 0][1], same = 0;
    bool leader = on;
    for (int j = 0; j < n; ++j) {
        const uint64_t h = kept[j][0], s = kept[j][1];
        if (h != hash) continue;
        same += 1;
        shape = min(shape, s);
        leader = leader && j >= lane;
    }
    if (leader) tally_insert(a, hash, shape, owner, same);
}

template <int NW, int REACH, bool TALLY, bool FREE>
__global__ __launch_bounds__(512) void batch_islands_kernel(const IslandArgs a)
{
    constexpr int NS = FREE ? 8 : 1;  // the sums of an island: one per orientation
    // [buffer][wave][lane 0, lane 1, the last lane but one, the last lane][word]
    __shared__ uint32_t edge[2][GOL_BATCH_MAX_WAVES][4][NW];
    __shared__ uint32_t changed[2][GOL_BATCH_MAX_WAVES];
    __shared__ uint32_t cand[2][GOL_BATCH_MAX_WAVES];
    __shared__ uint32_t part_cells[2][GOL_BATCH_MAX_WAVES], part_rows[2][GOL_BATCH_MAX_WAVES];
    __shared__ uint32_t part_cols[2][GOL_BATCH_MAX_WAVES][NW];
    __shared__ uint64_t part_hash[2][GOL_BATCH_MAX_WAVES][NS];
    __shared__ uint64_t fingerprint;  // the sum of the records' hashes so far

    uint64_t(*kept)[2] = nullptr;  // TALLY: the records gathered for wave 0, hash and packed shape
    if constexpr (TALLY) {
        __shared__ uint64_t kept_records[GOL_ISLAND_TALLY_BUFFER][2];
        kept = kept_records;
    }

    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int64_t board = blockIdx.x, out = blockIdx.x;  // the board read, and the place of its count and fingerprint
    if constexpr (TALLY) {
        if (a.pairs) {  // (uniform: every exit below is the whole workgroup's, before its first barrier)
            if ((int64_t)blockIdx.x >= (int64_t)*a.pair_count) return;
            const int32_t slot = a.pairs[2 * blockIdx.x], soup = a.pairs[2 * blockIdx.x + 1];
            if (slot < 0 || slot >= a.n || soup < 0) return;
            if (a.found[soup] < 0) {  // expired: the slot holds no s(found)
                if (threadIdx.x == 0) {
                    a.count[soup] = 0;
                    if (a.fingerprint) a.fingerprint[soup] = 0;
                }
                return;
            }
            board = slot, out = soup;
        }
    }
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
        uint64_t h[NS];
#pragma unroll
        for (int s = 0; s < NS; ++s) h[s] = 0;
        if (any) {
            if (!RESIDENT) load_windows(win);
            if constexpr (FREE) gol_island_row_hash_free<NW, REACH>(m, win, h);
            else h[0] = gol_island_row_hash<NW, REACH>(m, win);
        }
        const uint64_t holds = __ballot(any != 0);
        uint32_t cells = 0, cols[NW];
        uint64_t hash[NS];
#pragma unroll
        for (int s = 0; s < NS; ++s) hash[s] = 0;
#pragma unroll
        for (int j = 0; j < NW; ++j) cols[j] = 0u;
        for (uint64_t left = holds; left; left &= left - 1) {  // (uniform in the wave; at most 64 trips)
            const int l = __builtin_amdgcn_readfirstlane(__builtin_ctzll(left));
            cells += (uint32_t)__builtin_amdgcn_readlane((int)pop, l);
#pragma unroll
            for (int s = 0; s < NS; ++s)
                hash[s] += (uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)h[s], l) |
                           (uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(h[s] >> 32), l) << 32;
#pragma unroll
            for (int j = 0; j < NW; ++j) cols[j] |= (uint32_t)__builtin_amdgcn_readlane((int)m[j], l);
        }
        const uint32_t c = candidate();
        if (lane == 0) {
            part_cells[par][wave] = cells;
            part_rows[par][wave] = (uint32_t)__popcll(holds);
#pragma unroll
            for (int s = 0; s < NS; ++s) part_hash[par][wave][s] = hash[s];
#pragma unroll
            for (int j = 0; j < NW; ++j) part_cols[par][wave][j] = cols[j];
            cand[par][wave] = c;
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            gol_island r = {sy, sx, 0, 0, 0, 0};
            uint32_t nrows = 0, ncols = 0;
            uint64_t sums[NS];
#pragma unroll
            for (int s = 0; s < NS; ++s) sums[s] = 0;
            for (int i = 0; i < a.wpb; ++i) {
                r.cells += (int32_t)part_cells[par][i];
                nrows += part_rows[par][i];
#pragma unroll
                for (int s = 0; s < NS; ++s) sums[s] += part_hash[par][i][s];
            }
            if constexpr (FREE) r.hash = gol_island_free_hash(sums);  // the smallest of the eight orientations' sums
            else r.hash = sums[0];
#pragma unroll
            for (int j = 0; j < NW; ++j) {
                uint32_t w = 0;
                for (int i = 0; i < a.wpb; ++i) w |= part_cols[par][i][j];
                ncols += (uint32_t)__popc(w);
            }
            r.rows = (uint16_t)nrows;
            r.cols = (uint16_t)ncols;
            fingerprint += r.hash;
            if constexpr (TALLY) {
                kept[k % GOL_ISLAND_TALLY_BUFFER][0] = r.hash;
                kept[k % GOL_ISLAND_TALLY_BUFFER][1] = gol_island_shape_pack(r.cells, nrows, ncols);
            } else {
                if (k < a.cap) a.islands[board * a.cap + k] = r;
            }
        }
        if constexpr (TALLY) {
            if (wave == 0 && k % GOL_ISLAND_TALLY_BUFFER == GOL_ISLAND_TALLY_BUFFER - 1) {  // full: thread 0's writes, in this wave's order
                __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
                tally_flush(a, kept, lane, GOL_ISLAND_TALLY_BUFFER, (uint64_t)(a.owner0 + out));
            }
        }
        seed = lowest(par);
        par ^= 1;
        ++k;
    }
    if constexpr (TALLY) {
        if (wave == 0 && !over) {  // the remainder
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
            tally_flush(a, kept, lane, k % GOL_ISLAND_TALLY_BUFFER, (uint64_t)(a.owner0 + out));
        }
    }
    if (threadIdx.x == 0) {
        a.count[out] = over ? -1 : k;
        if (a.fingerprint) a.fingerprint[out] = fingerprint;
    }
}

__global__ __launch_bounds__(256) void island_table_clear_kernel(gol_island_slot *table, int64_t slots, unsigned long long *dropped)
{
    const gol_island_slot empty = GOL_ISLAND_SLOT_EMPTY;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < slots; i += (int64_t)gridDim.x * 256) table[i] = empty;
    if (blockIdx.x == 0 && threadIdx.x == 0) *dropped = 0;
}

template <int NW, bool FREE>
hipError_t launch_of(int reach, const IslandArgs &a, dim3 grid, dim3 block, hipStream_t s)
{
    if (a.table) {
        if (reach == 1) batch_islands_kernel<NW, 1, true, FREE><<<grid, block, 0, s>>>(a);
        else batch_islands_kernel<NW, 2, true, FREE><<<grid, block, 0, s>>>(a);
    } else {
        if (reach == 1) batch_islands_kernel<NW, 1, false, FREE><<<grid, block, 0, s>>>(a);
        else batch_islands_kernel<NW, 2, false, FREE><<<grid, block, 0, s>>>(a);
    }
    return hipGetLastError();
}

template <int NW>
hipError_t launch(int reach, int symmetry, const IslandArgs &a, dim3 grid, dim3 block, hipStream_t s)
{
    return symmetry == GOL_ISLAND_FREE ? launch_of<NW, true>(reach, a, grid, block, s) : launch_of<NW, false>(reach, a, grid, block, s);
}

}  // namespace

hipError_t golk_batch_islands(const gol_island_launch &l, hipStream_t s)
{
    if (!gol_island_launch_ok(l)) return hipErrorInvalidValue;
    const gol_batch_row g = gol_batch_row_init(l.W);
    const int wpb = (int)((l.H + 63) / 64);
    const IslandArgs a = {l.boards, g, (int32_t)l.H, (int32_t)l.W, (int32_t)((l.W + 63) / 64), wpb, l.cap, l.count, l.islands,
                          l.fingerprint, (gol_island_slot *)l.table, l.table_log2, (unsigned long long *)l.dropped, l.owner0, l.n,
                          l.pairs, l.pair_count, l.found};
    const dim3 grid((unsigned)(l.pairs ? l.max_pairs : l.n)), block((unsigned)(wpb * 64));
    switch (g.nw) {
    case 1: return launch<1>(l.reach, l.symmetry, a, grid, block, s);
    case 2: return launch<2>(l.reach, l.symmetry, a, grid, block, s);
    case 4: return launch<4>(l.reach, l.symmetry, a, grid, block, s);
    case 8: return launch<8>(l.reach, l.symmetry, a, grid, block, s);
    default: return launch<16>(l.reach, l.symmetry, a, grid, block, s);
    }
}

hipError_t golk_island_table_clear(gol_island_kind *table, int32_t table_log2, int64_t *dropped, hipStream_t s)
{
    if (!table || !dropped || table_log2 < GOL_ISLAND_TALLY_MIN_LOG2 || table_log2 > GOL_ISLAND_TALLY_MAX_LOG2)
        return hipErrorInvalidValue;
    const int64_t slots = (int64_t)1 << table_log2;
    island_table_clear_kernel<<<(unsigned)std::min<int64_t>((slots + 255) / 256, 4096), 256, 0, s>>>((gol_island_slot *)table, slots,
                                                                                                  (unsigned long long *)dropped);
    return hipGetLastError();
}
