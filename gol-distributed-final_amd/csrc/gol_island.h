// gol_island.h -- the island census of a small torus (include/golhip.h, "the island census of a batch", where link,
// island, window code, term, record, order and fingerprint are defined): what the kernel (gol_island.hip, one row per
// lane) and the host twin (gol_island_host.cpp) share, so the code the GPU runs is tested on the CPU.  No HIP header.
//
// A row is the NW words of gol_batch.h (gol_batch_row: nwr words in use, the last cell's bit tb, the tail mask; the
// padding zero).  Here:
//   - the record (gol_island, from golhip.h) and the term of a cell's window code;
//   - the rotations of a row on its W-cell ring by one cell either way, as words, on the L / R formulas of gol_batch.h
//     with the column wrap of a row that ends inside a word (two cells: the rotation twice, which is right on rings of
//     one and two cells as well);
//   - one dilation step of a row of the flood: M' = board & the OR of the (2 reach + 1)^2 shifted neighbours of M, from
//     the OR of the 2 reach + 1 rows of M round it;
//   - the window row: a board row turned so that the 2 reach + 1 cells round cell x are bits x .. x + 2 reach of NW + 1
//     words (the ring unrolled past its end), so a cell's part of the code is a shift and a mask;
//   - the hash of the cells of M in one row, and its FREE form: a code in the eight orientations of the square
//     (gol_island_orient), the eight sums of a row and their minimum, the free hash;
//   - the descriptor of one launch, plain or TALLY, with the one check of what makes it valid;
//   - the kind table of a tally: the packed shape and its unpacking, the empty slot, the home slot and the probe step;
//   - the check of a census's reach and symmetry (gol_island_mode_ok).
#pragma once
#include <stdint.h>

#include "gol_batch.h"
#include "golhip.h"

#define GOL_ISLAND_MAX_REACH 2

#define GOL_ISLAND_TALLY_MIN_LOG2 4
#define GOL_ISLAND_TALLY_MAX_LOG2 24
#define GOL_ISLAND_TALLY_BUFFER 64  // records a workgroup gathers before wave 0 inserts them, one lane each

static_assert(sizeof(gol_island) == 24, "the record is 24 bytes");
static_assert(sizeof(gol_island_kind) == 32, "a kind, and a slot of the device table, is 32 bytes");

// A slot of the device table as the kernel sees it: four 64-bit words, the last the packed shape.
struct gol_island_slot {
    uint64_t hash, count, first, shape;
};
static_assert(sizeof(gol_island_slot) == sizeof(gol_island_kind), "a slot has the bytes of a kind");
#define GOL_ISLAND_SLOT_EMPTY {0u, 0u, (uint64_t)INT64_MAX, ~(uint64_t)0}

GOL_BATCH_HD uint64_t gol_island_shape_pack(int32_t cells, uint32_t rows, uint32_t cols)
{
    return (uint64_t)(uint32_t)cells << 32 | (uint64_t)(rows & 0xffffu) << 16 | (uint64_t)(cols & 0xffffu);
}
// A filled slot as the kind a caller reads: the shape unpacked.
GOL_BATCH_HD gol_island_kind gol_island_slot_kind(const gol_island_slot &s)
{
    return {s.hash, (int64_t)s.count, (int64_t)s.first, (int32_t)(s.shape >> 32), (uint16_t)(s.shape >> 16), (uint16_t)s.shape};
}
// The tag a hash is tallied under: 0 is the empty slot's.
GOL_BATCH_HD uint64_t gol_island_tally_tag(uint64_t hash) { return hash ? hash : 1u; }
// The home slot of a tag in a table of 2^log2 slots, and the slot a probe visits after `slot`.
GOL_BATCH_HD uint64_t gol_island_tally_home(uint64_t tag, int32_t log2) { return gol_batch_splitmix64(tag) >> (64 - log2); }
// The order of a tally: count descending, then hash ascending.
GOL_BATCH_HD bool gol_island_kind_before(const gol_island_kind &a, const gol_island_kind &b)
{
    return a.count != b.count ? a.count > b.count : a.hash < b.hash;
}
GOL_BATCH_HD uint64_t gol_island_tally_next(uint64_t slot, int32_t log2) { return (slot + 1u) & (((uint64_t)1 << log2) - 1u); }

GOL_BATCH_HD uint64_t gol_island_term(uint64_t code, int32_t reach) { return gol_batch_splitmix64(code ^ ((uint64_t)reach << 32)); }

// The reach and the symmetry of a census: the one place they are checked, for launches, entries and twins alike.
GOL_BATCH_HD bool gol_island_mode_ok(int32_t reach, int32_t symmetry)
{
    return reach >= 1 && reach <= GOL_ISLAND_MAX_REACH && (symmetry == GOL_ISLAND_FIXED || symmetry == GOL_ISLAND_FREE);
}

// One launch of the census, as gol_dev_batch_islands (table NULL: plain, the fields after fingerprint 0) or
// gol_dev_batch_islands_tally (table not NULL: TALLY, cap 0) takes it; the pointers are device memory.
struct gol_island_launch {
    const uint64_t *boards;  // n boards of H rows of ceil(W / 64) words
    int64_t n, H, W;
    int32_t reach;
    int32_t symmetry;       // GOL_ISLAND_FIXED or GOL_ISLAND_FREE: the hash of the records, the fingerprint and the table's tag
    int64_t cap;            // records per board in `islands`
    int64_t *count;         // n (listed: indexed by soup)
    gol_island *islands;    // n cap, or NULL with cap == 0
    uint64_t *fingerprint;  // as count, or NULL
    // TALLY
    gol_island_kind *table;     // 2^table_log2 slots (gol_island_slot)
    int32_t table_log2;
    int64_t *dropped;           // one counter
    int64_t owner0;             // the owner of board 0 (listed: of soup 0)
    const int32_t *pairs;       // NULL: dense; else (slot, soup) pairs, the harvest list of the restock pass
    const int32_t *pair_count;  // the pairs in the list (device memory)
    int64_t max_pairs;          // the workgroups of a listed launch
    const int64_t *found;       // listed: by soup, < 0: the soup expired
};

// What makes a launch valid; everything else is refused and nothing is launched.
GOL_BATCH_HD bool gol_island_launch_ok(const gol_island_launch &l)
{
    if (!l.boards || !l.count || !gol_batch_shape_ok(l.n, l.H, l.W)) return false;
    if (!gol_island_mode_ok(l.reach, l.symmetry) || l.cap < 0) return false;
    if (!l.pairs && (l.pair_count || l.found || l.max_pairs != 0)) return false;
    if (!l.table)  // plain
        return (l.cap == 0 || l.islands != nullptr) && !l.dropped && !l.pairs && l.table_log2 == 0 && l.owner0 == 0;
    if (l.cap != 0 || l.islands || !l.dropped || l.owner0 < 0 || l.owner0 > ((int64_t)1 << 40)) return false;
    if (l.table_log2 < GOL_ISLAND_TALLY_MIN_LOG2 || l.table_log2 > GOL_ISLAND_TALLY_MAX_LOG2) return false;
    return !l.pairs || (l.pair_count && l.found && l.max_pairs >= 1 && l.max_pairs <= l.n);
}

// The mask of word j of a row (uniform in a kernel).
GOL_BATCH_HD uint32_t gol_island_keep(const gol_batch_row &g, int j) { return j < g.nwr - 1 ? ~0u : (j == g.nwr - 1 ? g.tail : 0u); }

// o[x] = c[(x - 1) mod W]: every cell moves one column up (L of gol_batch.h, masked).  o is not c.
template <int NW>
GOL_BATCH_HD void gol_island_rot_up(const uint32_t (&c)[NW], const gol_batch_row &g, uint32_t (&o)[NW])
{
    uint32_t last = c[0];  // word nwr - 1, picked without a variable register index
    GOL_BATCH_UNROLL
    for (int j = 1; j < NW; ++j) last = j == g.nwr - 1 ? c[j] : last;
    const uint32_t wl = (last >> g.tb) & 1u;  // cell W - 1, to the left of cell 0
    GOL_BATCH_UNROLL
    for (int j = 0; j < NW; ++j) o[j] = ((c[j] << 1) | (j > 0 ? c[j > 0 ? j - 1 : 0] >> 31 : wl)) & gol_island_keep(g, j);
}

// o[x] = c[(x + 1) mod W]: every cell moves one column down (R of gol_batch.h).  o is not c.
template <int NW>
GOL_BATCH_HD void gol_island_rot_down(const uint32_t (&c)[NW], const gol_batch_row &g, uint32_t (&o)[NW])
{
    const uint32_t wr = (c[0] & 1u) << g.tb;  // cell 0, to the right of cell W - 1
    GOL_BATCH_UNROLL
    for (int j = 0; j < NW; ++j)
        o[j] = (c[j] >> 1) | (j + 1 < NW ? c[j + 1 < NW ? j + 1 : j] << 31 : 0u) | (j == g.nwr - 1 ? wr : 0u);
}

// One dilation step of a row: v is the OR of the rows (y + dy) mod H, |dy| <= REACH, of M; out = board & the OR of v
// rotated by every |dx| <= REACH.
template <int NW, int REACH>
GOL_BATCH_HD void gol_island_dilate(const uint32_t (&board)[NW], const uint32_t (&v)[NW], const gol_batch_row &g,
                                    uint32_t (&out)[NW])
{
    uint32_t acc[NW], a[NW], t[NW];  // (one direction after the other: fewer rows alive at a time)
    GOL_BATCH_UNROLL
    for (int j = 0; j < NW; ++j) acc[j] = a[j] = v[j];
    GOL_BATCH_UNROLL
    for (int k = 0; k < REACH; ++k) {
        gol_island_rot_up<NW>(a, g, t);
        GOL_BATCH_UNROLL
        for (int j = 0; j < NW; ++j) acc[j] |= a[j] = t[j];
    }
    GOL_BATCH_UNROLL
    for (int j = 0; j < NW; ++j) a[j] = v[j];
    GOL_BATCH_UNROLL
    for (int k = 0; k < REACH; ++k) {
        gol_island_rot_down<NW>(a, g, t);
        GOL_BATCH_UNROLL
        for (int j = 0; j < NW; ++j) acc[j] |= a[j] = t[j];
    }
    GOL_BATCH_UNROLL
    for (int j = 0; j < NW; ++j) out[j] = board[j] & acc[j];
}

// The window row of a board row c: bit i of e, 0 <= i < W + 2 REACH, is cell (i - REACH) mod W, so the cells x - REACH
// .. x + REACH of the ring are bits x .. x + 2 REACH.  The row rotated up by REACH, and its first 2 REACH cells again
// from bit W on; a ring of fewer than 4 cells is repeated five times (W + 2 REACH <= 5 W), all in word 0.
template <int NW, int REACH>
GOL_BATCH_HD void gol_island_window_row(const uint32_t (&c)[NW], const gol_batch_row &g, int32_t W, uint32_t (&e)[NW + 1])
{
    uint32_t p[NW], t[NW];
    GOL_BATCH_UNROLL
    for (int j = 0; j < NW; ++j) p[j] = c[j];
    GOL_BATCH_UNROLL
    for (int k = 0; k < REACH; ++k) {
        gol_island_rot_up<NW>(p, g, t);
        GOL_BATCH_UNROLL
        for (int j = 0; j < NW; ++j) p[j] = t[j];
    }
    if (W < 4) {  // (uniform)
        e[0] = p[0] | p[0] << W | p[0] << 2 * W | p[0] << 3 * W | p[0] << 4 * W;
        GOL_BATCH_UNROLL
        for (int j = 1; j <= NW; ++j) e[j] = 0u;
        return;
    }
    const uint32_t low = p[0] & ((1u << 2 * REACH) - 1u);
    const int32_t ws = W / 32, bs = W % 32;  // where bit W lies
    GOL_BATCH_UNROLL
    for (int j = 0; j <= NW; ++j) {
        uint32_t v = j < NW ? p[j < NW ? j : 0] : 0u;
        v |= j == ws ? low << bs : 0u;
        v |= j == ws + 1 && bs > 0 ? low >> (32 - bs) : 0u;
        e[j] = v;
    }
}

// The 2 REACH + 1 cells of a window row from bit b < 32 of word lo on (hi: the word after it).  A funnel shift in 32-bit
// operations: written through a 64-bit word, the two words of a lane's register array are read as one, overlapping the
// next pair, and the array leaves the registers.
template <int REACH>
GOL_BATCH_HD uint32_t gol_island_field(uint32_t lo, uint32_t hi, uint32_t b)
{
    return ((lo >> b) | ((hi << 1) << (31u - b))) & ((1u << (2 * REACH + 1)) - 1u);
}

// The sum of the terms of the cells of m, one row of an island: e[dy + REACH] is the window row of board row (y + dy) mod H.
template <int NW, int REACH>
GOL_BATCH_HD uint64_t gol_island_row_hash(const uint32_t (&m)[NW], const uint32_t (&e)[2 * REACH + 1][NW + 1])
{
    uint64_t h = 0;
    GOL_BATCH_UNROLL
    for (int j = 0; j < NW; ++j) {
        for (uint32_t left = m[j]; left; left &= left - 1u) {  // (at most 32 trips)
            const uint32_t b = (uint32_t)__builtin_ctz(left);
            uint64_t code = 0;
            GOL_BATCH_UNROLL
            for (int d = 0; d < 2 * REACH + 1; ++d)
                code |= (uint64_t)gol_island_field<REACH>(e[d][j], e[d][j + 1], b) << (d * (2 * REACH + 1));
            h += gol_island_term(code, REACH);
        }
    }
    return h;
}

// ---------------------------------------------------------------------------------------------- the FREE form
// (include/golhip.h, "island kinds free of orientation": orientation s = t | fy << 1 | fx << 2.)
// A code is 2 REACH + 1 fields of 2 REACH + 1 bits, the bit of (dy, dx) at (dy + REACH) (2 REACH + 1) + (dx + REACH).  The
// three generators as delta swaps, their masks constants of REACH: the rows flipped (the fields reordered), the
// columns flipped (every field's bits reversed), the transpose (the bit of (i, i + d) and that of (i + d, i) lie d
// (K - 1) apart).
template <int REACH>
struct gol_island_sym {
    static constexpr int K = 2 * REACH + 1;
    static constexpr uint64_t row(int i) { return (((uint64_t)1 << K) - 1u) << (i * K); }
    static constexpr uint64_t col(int j)
    {
        uint64_t m = 0;
        for (int i = 0; i < K; ++i) m |= (uint64_t)1 << (i * K + j);
        return m;
    }
    static constexpr uint64_t diag(int d)  // the bits (i, i + d)
    {
        uint64_t m = 0;
        for (int i = 0; i + d < K; ++i) m |= (uint64_t)1 << (i * K + i + d);
        return m;
    }
};

template <int REACH>
GOL_BATCH_HD uint64_t gol_island_flip_rows(uint64_t c)
{
    typedef gol_island_sym<REACH> S;
    uint64_t r = c & S::row(REACH);
    GOL_BATCH_UNROLL
    for (int i = 0; i < REACH; ++i) {
        const int sh = (S::K - 1 - 2 * i) * S::K;
        r |= (c & S::row(i)) << sh | ((c >> sh) & S::row(i));
    }
    return r;
}

template <int REACH>
GOL_BATCH_HD uint64_t gol_island_flip_cols(uint64_t c)
{
    typedef gol_island_sym<REACH> S;
    uint64_t r = c & S::col(REACH);
    GOL_BATCH_UNROLL
    for (int j = 0; j < REACH; ++j) {
        const int sh = S::K - 1 - 2 * j;
        r |= (c & S::col(j)) << sh | ((c >> sh) & S::col(j));
    }
    return r;
}

template <int REACH>
GOL_BATCH_HD uint64_t gol_island_transpose(uint64_t c)
{
    typedef gol_island_sym<REACH> S;
    uint64_t r = c & S::diag(0);
    GOL_BATCH_UNROLL
    for (int d = 1; d < S::K; ++d) {
        const int sh = d * (S::K - 1);
        r |= (c & S::diag(d)) << sh | ((c >> sh) & S::diag(d));
    }
    return r;
}

// o[s] = orient(c, REACH, s), all eight: the flips first, then the transpose (one row flip, two column flips, four
// transposes).
template <int REACH>
GOL_BATCH_HD void gol_island_orient_all(uint64_t c, uint64_t (&o)[8])
{
    o[0] = c;
    o[2] = gol_island_flip_rows<REACH>(c);
    o[4] = gol_island_flip_cols<REACH>(c);
    o[6] = gol_island_flip_cols<REACH>(o[2]);
    GOL_BATCH_UNROLL
    for (int s = 0; s < 8; s += 2) o[s + 1] = gol_island_transpose<REACH>(o[s]);
}

// orient(code, reach, s) of golhip.h; 0 for an s outside 0..7 or a reach outside 1..GOL_ISLAND_MAX_REACH.
GOL_BATCH_HD uint64_t gol_island_orient(uint64_t code, int32_t reach, int32_t s)
{
    if (s < 0 || s > 7 || reach < 1 || reach > GOL_ISLAND_MAX_REACH) return 0;
    uint64_t o[8];
    if (reach == 1) gol_island_orient_all<1>(code, o);
    else gol_island_orient_all<2>(code, o);
    uint64_t r = o[0];
    GOL_BATCH_UNROLL
    for (int i = 1; i < 8; ++i) r = i == s ? o[i] : r;
    return r;
}

// gol_island_row_hash in the eight orientations: h[s] the sum of term(orient(code, REACH, s)) over the cells of m.
template <int NW, int REACH>
GOL_BATCH_HD void gol_island_row_hash_free(const uint32_t (&m)[NW], const uint32_t (&e)[2 * REACH + 1][NW + 1], uint64_t (&h)[8])
{
    GOL_BATCH_UNROLL
    for (int s = 0; s < 8; ++s) h[s] = 0;
    GOL_BATCH_UNROLL
    for (int j = 0; j < NW; ++j) {
        for (uint32_t left = m[j]; left; left &= left - 1u) {  // (at most 32 trips)
            const uint32_t b = (uint32_t)__builtin_ctz(left);
            uint64_t code = 0, o[8];
            GOL_BATCH_UNROLL
            for (int d = 0; d < 2 * REACH + 1; ++d)
                code |= (uint64_t)gol_island_field<REACH>(e[d][j], e[d][j + 1], b) << (d * (2 * REACH + 1));
            gol_island_orient_all<REACH>(code, o);
            GOL_BATCH_UNROLL
            for (int s = 0; s < 8; ++s) h[s] += gol_island_term(o[s], REACH);
        }
    }
}

// The free hash: the smallest of an island's eight sums.
GOL_BATCH_HD uint64_t gol_island_free_hash(const uint64_t (&h)[8])
{
    uint64_t r = h[0];
    GOL_BATCH_UNROLL
    for (int s = 1; s < 8; ++s) r = h[s] < r ? h[s] : r;
    return r;
}
