// gol_batch.h -- one row of a small torus (1 <= H, W <= 512, any width) as up to 16 32-bit words in
// one lane, and one turn of it: the horizontal sums of the row with the column wrap of a row that
// ends inside a word, the tail mask, and the choice between the two rule circuits.  Shared by the
// batch kernel (gol_batch.hip, one row per lane) and the host (gol_batch_step_host,
// include/golhip.h), so the code the GPU runs is tested on the CPU.
//
// A row of W cells is nwr = ceil(W / 32) words c[0 .. nwr) (bit c % 32 of word c / 32 = cell c), held
// in NW = nwr rounded up to 1, 2, 4, 8 or 16 words; the words from nwr on and the bits above tb =
// (W - 1) % 32 of word nwr - 1 are zero (the padding).  The left and right neighbours of every cell,
// as words:
//   L[j] = (c[j] << 1) | (j > 0 ? c[j-1] >> 31 : cell W - 1)
//   R[j] = (c[j] >> 1) | (j < nwr - 1 ? c[j+1] << 31 : cell 0 at bit tb)
// and the row's horizontal sums h0 + 2 h1 = L + c + R per cell (the cell included, as in every
// kernel here).  The three rows' sums go into the rule: B3/S23 the 7-gate circuit of the step
// kernels (golk::rule), any other rule gol_rule_sum3 + gol_rule_eval (gol_rule.h).  The padding of the
// result is cleared afterwards (a cell of the padding has neighbours, and B0 rules give birth there).
// Also here, for the same reason: the step kernel's modes and the marks of its cycle scan, the soup words and the
// census, the descriptor of one launch with the one check of what makes it valid, and the host twins' unpacking of a
// uint64 row into a lane's words and back (no HIP header is needed).
#pragma once
#include <stdint.h>

#include "gol_rule.h"

#define GOL_BATCH_HD GOL_RULE_HD
#if defined(__HIP_DEVICE_COMPILE__)
#define GOL_BATCH_UNROLL _Pragma("unroll")  // (a lane's words are registers: no loop may index them)
#else
#define GOL_BATCH_UNROLL
#endif

#define GOL_BATCH_MAX_SIDE 512  // cells: at most 16 words of a row, 8 waves of 64 rows
#define GOL_BATCH_MAX_WAVES 8
#define GOL_BATCH_MAX_BOARDS ((int64_t)1 << 20)

// A batch's shape: n boards of H x W cells.  The mask of a row's last uint64 word (the padding above cell W - 1 clear).
GOL_BATCH_HD bool gol_batch_shape_ok(int64_t n, int64_t H, int64_t W)
{
    return n >= 1 && n <= GOL_BATCH_MAX_BOARDS && H >= 1 && H <= GOL_BATCH_MAX_SIDE && W >= 1 && W <= GOL_BATCH_MAX_SIDE;
}

GOL_BATCH_HD uint64_t gol_batch_tail64(int64_t W) { return W % 64 ? ((uint64_t)1 << (W % 64)) - 1 : ~(uint64_t)0; }

// The step kernel's modes.  Rule: B3/S23 on 7 gates, one table rule for the batch, a table rule per
// board.  Scan: none, state(t) == state(t - 2) (periods 1 and 2, the exact settle turn), cycles of
// any period against a snapshot taken at the marks below.
enum { GOL_BATCH_RULE_CONWAY = 0, GOL_BATCH_RULE_TABLE = 1, GOL_BATCH_RULE_EACH = 2 };
enum { GOL_BATCH_SCAN_NONE = 0, GOL_BATCH_SCAN_SETTLE = 1, GOL_BATCH_SCAN_CYCLES = 2 };

// The cycle scan's marks (Brent's cycle detection), in turns d >= 0 since the call began: d = 2^j - 1,
// that is 0, 1, 3, 7, ...  A turn d >= 1 is compared with the state at the last mark before it, and
// the state of a turn that is a mark is the snapshot of the turns after it.
GOL_BATCH_HD bool gol_batch_is_mark(int64_t d) { return d >= 0 && ((d + 1) & d) == 0; }

GOL_BATCH_HD int64_t gol_batch_last_mark(int64_t d)  // d >= 1: the largest mark < d
{
    int64_t p = 1;
    while (p <= d / 2) p *= 2;  // the largest power of two <= d
    return p - 1;
}

// The period of a board found d >= 1 turns into its scan: state(d) == state(the last mark before d).
GOL_BATCH_HD int64_t gol_batch_period(int64_t d) { return d - gol_batch_last_mark(d); }

// Retirement (gol_batch_run_cycles): a board found d >= 1 turns after the call began, with period p = d - the last
// mark before d, has s(t + p) == s(t) from turn d - p on.  Seen at a turn >= d with `rest` >= 0 turns of the call still to
// come, its state at the call's end is its state now advanced by rest mod p turns: the turns it still has to make.
GOL_BATCH_HD int64_t gol_batch_turns_left(int64_t d, int64_t rest) { return rest % gol_batch_period(d); }

// Soups (gol_batch_load_soups, gol_batch_search): word (y, w) of soup g of (seed, H, Ww) is splitmix64(seed ^ ((g H + y) Ww
// + w)), the padding of a row's last word cleared with `tail`: board g of gol_batch_load_random on a batch that holds it.
// i = (g H + y) Ww + w is the word's index in the supply; the fill kernels and gol_batch_soup_host run this function.
GOL_BATCH_HD uint64_t gol_batch_splitmix64(uint64_t x)
{
    uint64_t z = x + 0x9E3779B97F4A7C15ULL;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
    return z ^ (z >> 31);
}

GOL_BATCH_HD uint64_t gol_batch_soup_word(uint64_t seed, uint64_t i, int64_t Ww, uint64_t tail)
{
    const uint64_t v = gol_batch_splitmix64(seed ^ i);
    return i % (uint64_t)Ww == (uint64_t)Ww - 1 ? v & tail : v;
}

// The census of a board: its alive cells, and its hash (oracle_hash_words) the sum over its H Ww words of this term of
// word i.  The kernels sum the terms over a wave's lanes (gol_batch_pass.hip), gol_batch_board_census over a dense host board.
GOL_BATCH_HD uint64_t gol_batch_hash_term(uint64_t word, uint64_t i) { return gol_batch_splitmix64(word ^ gol_batch_splitmix64(i)); }

GOL_BATCH_HD void gol_batch_board_census(const uint64_t *board, int64_t words, uint64_t *alive, uint64_t *hash)
{
    *alive = *hash = 0;
    for (int64_t i = 0; i < words; ++i) {
        *alive += (uint64_t)__builtin_popcountll(board[i]);
        *hash += gol_batch_hash_term(board[i], (uint64_t)i);
    }
}

// The results of a search before it has run: no soup found.  period, alive and hash may be NULL.
GOL_BATCH_HD void gol_batch_no_results(int64_t total, int64_t *found, int64_t *period, uint64_t *alive, uint64_t *hash)
{
    for (int64_t g = 0; g < total; ++g) {
        found[g] = -1;
        if (period) period[g] = -1;
        if (alive) alive[g] = 0;
        if (hash) hash[g] = 0;
    }
}

// The search's verdict on a slot at a launch boundary (the restock pass, gol_batch_search_host): its soup is `age` turns old,
// the scan found it at the age `found` (< 0: not yet), and the search looks `horizon` turns far.  A soup found after the
// horizon, in a launch that ran past it, is not a find.
enum { GOL_BATCH_STAY = 0, GOL_BATCH_FOUND = 1, GOL_BATCH_EXPIRED = 2 };
GOL_BATCH_HD int gol_batch_verdict(int64_t found, int64_t age, int64_t horizon)
{
    if (found >= 0) return found <= horizon ? GOL_BATCH_FOUND : GOL_BATCH_EXPIRED;
    return age >= horizon ? GOL_BATCH_EXPIRED : GOL_BATCH_STAY;
}

// One launch of the step kernel, as gol_dev_batch_step takes it (include/golhip.h, where every field is described);
// the pointers are device memory.  The drivers fill one per call and change per launch what differs.
struct gol_batch_launch {
    uint64_t *boards, *prev;  // n boards of H rows of ceil(W / 64) words; the scan's second buffer
    int64_t *settled;         // the scan's result per board
    int64_t n, H, W;
    int32_t turns;
    int64_t turn0;
    bool have_prev, write_prev;
    uint32_t birth, survive;
    const uint32_t *rules;  // a rule per board, or NULL
    int32_t scan;           // GOL_BATCH_SCAN_*
    int64_t done;
    const int32_t *list, *count;  // the boards of the launch, or NULL: every board
    int64_t slots;                // with a list: the grid's board slots, >= *count; else 0 (the grid is sized by n)
    int64_t *left;                // the finish
    const int64_t *born;          // the aged search
    // MAP rules (gol_map.h), or NULL: 16 words for every board, or map_each: n times 16, board b under maps + 16 b
    const uint32_t *maps;
    bool map_each;
};

// What makes a launch valid, per mode; everything else is refused and nothing is launched.
GOL_BATCH_HD bool gol_batch_launch_ok(const gol_batch_launch &l)
{
    if (!l.boards || !gol_batch_shape_ok(l.n, l.H, l.W) || l.turns < 1 || l.birth >= 512 || l.survive >= 512 || l.done < 0)
        return false;
    // maps take the place of the masks and of the rules per board; the aged search has one map; no maps, no flag
    if (l.maps ? l.rules || l.birth || l.survive || (l.born && l.map_each) : l.map_each) return false;
    // a scan has its result and its second buffer; without one there is no scan mode and neither prev flag
    const bool scans = l.settled != nullptr;
    if (scans ? !l.prev || (l.scan != GOL_BATCH_SCAN_SETTLE && l.scan != GOL_BATCH_SCAN_CYCLES)
              : l.scan != GOL_BATCH_SCAN_NONE || l.have_prev || l.write_prev)
        return false;
    // the cycle scan's snapshot comes from the launch before, which the call's first launch does not have
    if (l.scan == GOL_BATCH_SCAN_CYCLES && l.have_prev != (l.done > 0)) return false;
    // plain, settle, cycles: every board, nothing of a list
    if (!l.list && !l.count && !l.left && !l.born) return l.slots == 0;
    // a list has its count and its slots, and no settle scan
    if (!l.list || !l.count || l.slots < 1 || l.slots > l.n || l.scan == GOL_BATCH_SCAN_SETTLE) return false;
    // aged: the cycle scan in the boards' own ages, one rule, the snapshot always written
    if (l.born) return scans && !l.left && !l.rules && l.turn0 == 0 && l.write_prev;
    // list + cycles, or the finish with its turns left and no scan
    return scans != (l.left != nullptr);
}

// The shape of a row: nwr words in use of nw held, the last cell's bit and the mask of the last word.
struct gol_batch_row {
    int32_t nwr, nw;
    uint32_t tb, tail;
};

GOL_BATCH_HD gol_batch_row gol_batch_row_init(int64_t W)  // 1 <= W <= GOL_BATCH_MAX_SIDE
{
    gol_batch_row r;
    r.nwr = (int32_t)((W + 31) / 32);
    r.nw = 1;
    while (r.nw < r.nwr) r.nw *= 2;
    r.tb = (uint32_t)((W - 1) % 32);
    r.tail = r.tb == 31 ? ~0u : (1u << (r.tb + 1)) - 1u;
    return r;
}

GOL_BATCH_HD bool gol_batch_conway(uint32_t birth, uint32_t survive)
{
    return birth == GOL_RULE_BIRTH_CONWAY && survive == GOL_RULE_SURVIVE_CONWAY;
}

// A host row of ceil(W / 64) uint64 words as the g.nw words a lane holds (the padding of the input masked off), and back
// (an odd nwr: the upper half of the last uint64 word is padding).
GOL_BATCH_HD void gol_batch_unpack_row(const gol_batch_row &g, const uint64_t *row, uint32_t *c)
{
    for (int j = 0; j < g.nw; ++j) {
        c[j] = j < g.nwr ? (uint32_t)(row[j / 2] >> (32 * (j & 1))) : 0u;
        if (j == g.nwr - 1) c[j] &= g.tail;
    }
}

GOL_BATCH_HD void gol_batch_pack_row(const gol_batch_row &g, const uint32_t *c, uint64_t *row)
{
    for (int w = 0; w < (g.nwr + 1) / 2; ++w)
        row[w] = (uint64_t)c[2 * w] | (uint64_t)(2 * w + 1 < g.nw ? c[2 * w + 1] : 0u) << 32;
}

// The horizontal sums of a row (padding zero).  nwr and tb are wave-uniform in a kernel.
template <int NW>
GOL_BATCH_HD void gol_batch_hsum(const uint32_t (&c)[NW], int32_t nwr, uint32_t tb, uint32_t (&h0)[NW], uint32_t (&h1)[NW])
{
    uint32_t last = c[0];  // word nwr - 1, picked without a variable register index
    GOL_BATCH_UNROLL
    for (int j = 1; j < NW; ++j) last = j == nwr - 1 ? c[j] : last;
    const uint32_t wl = (last >> tb) & 1u;  // cell W - 1, to the left of cell 0
    const uint32_t wr = (c[0] & 1u) << tb;  // cell 0, to the right of cell W - 1
    GOL_BATCH_UNROLL
    for (int j = 0; j < NW; ++j) {
        const uint32_t l = (c[j] << 1) | (j > 0 ? c[j > 0 ? j - 1 : 0] >> 31 : wl);
        const uint32_t r = (c[j] >> 1) | (j + 1 < NW ? c[j + 1 < NW ? j + 1 : j] << 31 : 0u) | (j == nwr - 1 ? wr : 0u);
        h0[j] = gol_rule_xor3(l, c[j], r);
        h1[j] = gol_rule_maj(l, c[j], r);
    }
}

// B3/S23 from the three rows' sums (a above, b the cell's own row, c below) and the cell.
GOL_BATCH_HD uint32_t gol_batch_conway_next(uint32_t a0, uint32_t a1, uint32_t b0, uint32_t b1, uint32_t c0, uint32_t c1,
                                            uint32_t cell)
{
#if defined(__HIP_DEVICE_COMPILE__) && defined(GOL_BATCH_CONWAY)  // (the kernel unit: golk::rule of gol_device.h)
    return GOL_BATCH_CONWAY(a0, a1, b0, b1, c0, c1, cell);
#else  // the same circuit in plain operators (gol_device.h: TT_G1, TT_G2, TT_OUT)
    const uint32_t t0 = a0 ^ b0 ^ c0, k0 = (a0 & b0) | (c0 & (a0 | b0));
    const uint32_t u = a1 ^ b1 ^ c1, v = (a1 & b1) | (c1 & (a1 | b1));
    const uint32_t g1 = (t0 ^ k0 ^ v) & ~(t0 & k0 & v);  // exactly one of t0, k0, v
    const uint32_t g2 = (u & v) | ((u ^ v ^ g1) & ~(u & v & g1));  // (u & v) | exactly one of u, v, g1
    return (t0 | cell) & ~g2;
#endif
}

// One turn of a row: its next cells from the sums of the row above (a), its own (b) and the one
// below (d).  GENERIC: the table circuit with t (gol_rule_expand), else B3/S23.  msk: all ones for a
// row of the board, 0 for a lane without one.
template <int NW, bool GENERIC>
GOL_BATCH_HD void gol_batch_next(const gol_rule_tab &t, const gol_batch_row &g, const uint32_t (&a0)[NW],
                                 const uint32_t (&a1)[NW], const uint32_t (&b0)[NW], const uint32_t (&b1)[NW],
                                 const uint32_t (&d0)[NW], const uint32_t (&d1)[NW], const uint32_t (&cell)[NW], uint32_t msk,
                                 uint32_t (&out)[NW])
{
    GOL_BATCH_UNROLL
    for (int j = 0; j < NW; ++j) {
        uint32_t v;
        if (GENERIC) {
            uint32_t t0, t1, t2, t3;
            gol_rule_sum3(a0[j], a1[j], b0[j], b1[j], d0[j], d1[j], t0, t1, t2, t3);
            v = gol_rule_eval(t, t0, t1, t2, t3, cell[j]);
        } else {
            v = gol_batch_conway_next(a0[j], a1[j], b0[j], b1[j], d0[j], d1[j], cell[j]);
        }
        const uint32_t keep = j < g.nwr - 1 ? ~0u : (j == g.nwr - 1 ? g.tail : 0u);  // (uniform)
        out[j] = v & keep & msk;
    }
}
