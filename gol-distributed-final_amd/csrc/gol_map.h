// gol_map.h -- a MAP rule (any two-state rule of the 3x3 block) as data, and the one circuit that evaluates it on
// bit-sliced words.  Shared by the batch's map kernel (gol_batch_map.hip, one row per lane) and the host
// (gol_map_eval_host, gol_batch_step_map_host, include/golhip.h: "MAP rules of a batch"), so the circuit the GPU runs
// is tested on the CPU.
//
// A map is uint32_t map[16], a truth table of 512 bits: bit i is (map[i >> 5] >> (i & 31)) & 1, and for a cell
//   i = 256 NW + 128 N + 64 NE + 32 W + 16 C + 8 E + 4 SW + 2 S + SE
// of its 3x3 block on the torus; the cell is alive next turn iff bit i is set (i = 0 included).  The nine planes of 32
// cells are x[0 .. 9) in that order, x[k] the plane of weight 2^(8 - k): NW, N, NE, W, C, E, SW, S, SE.
//
// The circuit is a Shannon mux tree over the nine planes with wave-uniform leaves.  The two lowest variables are not
// muxed: the 16 functions of (S, SE) are computed once per word into F[16], F[s] the function whose truth table over
// 2 S + SE is the nibble s, and each of the 128 nodes above them is F[sel], sel the four consecutive table bits
// 4 k .. 4 k + 3 -- an aligned nibble of a table word, which is why the index order is the one above.  127 muxes over
// SW, E, C, W, NE, N, NW follow, written depth first so that few nodes are alive at a time.
#pragma once
#include <stdint.h>

#include "gol_batch.h"

#define GOL_MAP_WORDS 16  // uint32 words of a map: 512 bits

GOL_BATCH_HD uint32_t gol_map_bit(const uint32_t *map, uint32_t i) { return (map[i >> 5] >> (i & 31u)) & 1u; }

// The life-like rule (two 9-bit masks, gol_rule.h) as a map: bit i = the mask of the centre's state at the count of the
// other eight.
GOL_BATCH_HD void gol_map_from_rule(uint32_t birth, uint32_t survive, uint32_t *map)
{
    for (int w = 0; w < GOL_MAP_WORDS; ++w) map[w] = 0;
    for (uint32_t i = 0; i < 512; ++i) {
        const uint32_t n = (uint32_t)__builtin_popcount(i & ~16u);
        if (((i & 16u ? survive : birth) >> n) & 1u) map[i >> 5] |= 1u << (i & 31u);
    }
}

// The left and right neighbour words of a row held as c[NW] (padding zero), with the column wrap of a row that ends
// inside a word: the l and r of gol_batch_hsum (gol_batch.h), which keeps its own copy.  nwr and tb are wave-uniform.
template <int NW>
GOL_BATCH_HD void gol_map_planes(const uint32_t (&c)[NW], int32_t nwr, uint32_t tb, uint32_t (&l)[NW], uint32_t (&r)[NW])
{
    uint32_t last = c[0];  // word nwr - 1, picked without a variable register index
    GOL_BATCH_UNROLL
    for (int j = 1; j < NW; ++j) last = j == nwr - 1 ? c[j] : last;
    const uint32_t wl = (last >> tb) & 1u;  // cell W - 1, to the left of cell 0
    const uint32_t wr = (c[0] & 1u) << tb;  // cell 0, to the right of cell W - 1
    GOL_BATCH_UNROLL
    for (int j = 0; j < NW; ++j) {
        l[j] = (c[j] << 1) | (j > 0 ? c[j > 0 ? j - 1 : 0] >> 31 : wl);
        r[j] = (c[j] >> 1) | (j + 1 < NW ? c[j + 1 < NW ? j + 1 : j] << 31 : 0u) | (j == nwr - 1 ? wr : 0u);
    }
}

// Node k of level LEVEL: the function of the planes below the level's own that the table bits [k << (LEVEL + 2),
// (k + 1) << (LEVEL + 2)) give.  Level 0 is a leaf, F[the nibble k of the table]; level L >= 1 muxes on the plane of
// weight 2 << L, x[7 - L].
template <int LEVEL>
GOL_BATCH_HD uint32_t gol_map_node(const uint32_t *map, const uint32_t (&F)[16], const uint32_t *x, int k)
{
    if constexpr (LEVEL == 0) {
        return F[(map[k >> 3] >> (4 * (k & 7))) & 15u];
    } else {
        const uint32_t lo = gol_map_node<LEVEL - 1>(map, F, x, 2 * k);
        const uint32_t hi = gol_map_node<LEVEL - 1>(map, F, x, 2 * k + 1);
        return gol_rule_mux(x[7 - LEVEL], hi, lo);
    }
}

// next = map[i] for 32 cells, x the nine planes of i (above).
GOL_BATCH_HD uint32_t gol_map_eval(const uint32_t *map, const uint32_t *x)
{
    const uint32_t s = x[7], e = x[8];
    const uint32_t m[4] = {~s & ~e, ~s & e, s & ~e, s & e};  // the cells with 2 S + SE = 0, 1, 2, 3
    uint32_t F[16];
    GOL_BATCH_UNROLL
    for (int f = 0; f < 16; ++f) F[f] = (f & 1 ? m[0] : 0u) | (f & 2 ? m[1] : 0u) | (f & 4 ? m[2] : 0u) | (f & 8 ? m[3] : 0u);
    return gol_map_node<7>(map, F, x, 0);
}

// One turn of a row under a map: its next cells from its own words c and the raw words of the row above (up) and the
// row below (dn), every padding zero.  The padding of the result is cleared (a map may give birth on empty ground);
// msk: all ones for a row of the board, 0 for a lane without one.
template <int NW>
GOL_BATCH_HD void gol_batch_map_next(const uint32_t *map, const gol_batch_row &g, const uint32_t (&up)[NW], const uint32_t (&c)[NW],
                                     const uint32_t (&dn)[NW], uint32_t msk, uint32_t (&out)[NW])
{
    uint32_t ul[NW], ur[NW], cl[NW], cr[NW], dl[NW], dr[NW];
    gol_map_planes<NW>(up, g.nwr, g.tb, ul, ur);
    gol_map_planes<NW>(c, g.nwr, g.tb, cl, cr);
    gol_map_planes<NW>(dn, g.nwr, g.tb, dl, dr);
    GOL_BATCH_UNROLL
    for (int j = 0; j < NW; ++j) {
        const uint32_t x[9] = {ul[j], up[j], ur[j], cl[j], c[j], cr[j], dl[j], dn[j], dr[j]};
        const uint32_t keep = j < g.nwr - 1 ? ~0u : (j == g.nwr - 1 ? g.tail : 0u);  // (uniform)
        out[j] = gol_map_eval(map, x) & keep & msk;
    }
}
