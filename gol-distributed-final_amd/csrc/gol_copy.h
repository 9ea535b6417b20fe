// gol_copy.h -- a rectangle of cells read from a row of the board, in the layout the row is
// stepped in: the read-side twin of gol_edit.h, whose geometry (gol_edit_geom: the lanes T, the unit
// of lane t, bit0, wrap_c) it reuses.  Shared by the region-read kernels (gol_copy.hip) and the host
// (gol_copy_host, gol_bounds_host, include/golhip.h), so the mapping the GPU runs is tested on the CPU.
//
// Copy (gather).  Pattern cell c of a row (0 <= c < w; bit c % 64 of word c / 64) is board column
// (x0 + c) mod W.  The pattern is written as 32-bit halves, and every half has exactly one writer:
//  - band rows: lane t < T = min(w, Wd) reads its one word (gol_edit_unit); bit gol_copy_band_bit(g,
//    t, m) of it is pattern cell t + m*Wd, slot m < gol_copy_band_slots(g).  The 32 lanes 32q .. 32q +
//    31 of slot m hold the 32 consecutive cells of half q + m*Wd/32 (Wd % 32 == 0), q < ceil(T / 32);
//  - standard rows: half j < ceil(w / 32) is a funnel shift of board words gol_copy_std_unit(g, j, 0)
//    and (g, j, 1) (the second only if gol_copy_std_hi(g, j)), masked to [0, w): gol_copy_std_half;
//  - byte rows: cell c is byte gol_edit_unit(g, c) of the one-byte form (alive = non-zero), 64
//    consecutive cells make a pattern word.
// Bounds.  Lane t < T of the paste's geometry (the 4-byte form of byte rows included) masks its unit
// to the rectangle -- gol_copy_mask: gol_edit_word / gol_edit_bytes4 without a pattern under COPY --
// and ORs gol_copy_occ of it into a column-occupancy word per lane (gol_copy_occ_unit, one lane and
// row of it, is what kernel and host both call); gol_copy_cols turns the set bits of that word back
// into the smallest and largest rectangle column among them.
#pragma once
#include "gol_edit.h"

GOL_EDIT_HD uint32_t gol_copy_band_slots(const gol_edit_geom &g) { return (uint32_t)((g.w + g.units - 1) / g.units); }

GOL_EDIT_HD uint32_t gol_copy_band_bit(const gol_edit_geom &g, int64_t t, uint32_t m)
{
    const uint32_t carry = g.first + t >= g.units;
    return (g.bit0 + carry + m) & 31u;
}

// Standard rows: the board word that holds the first (k = 0) or the last (k = 1) cells of pattern half j.
GOL_EDIT_HD int64_t gol_copy_std_unit(const gol_edit_geom &g, int64_t j, int k)
{
    const int64_t u = g.first + j + k;  // < 2 * units
    return u >= g.units ? u - g.units : u;
}

// Whether half j takes cells of a second word at all.
GOL_EDIT_HD bool gol_copy_std_hi(const gol_edit_geom &g, int64_t j)
{
    return g.bit0 != 0 && j * 32 + 32 - (int64_t)g.bit0 < g.w;
}

// Pattern half j (cells 32j .. 32j + 31, the bits at c >= w zero) of board words lo and hi.
GOL_EDIT_HD uint32_t gol_copy_std_half(const gol_edit_geom &g, int64_t j, uint32_t lo, uint32_t hi)
{
    uint32_t v = g.bit0 ? (lo >> g.bit0) | (hi << (32 - g.bit0)) : lo;
    const int64_t rem = g.w - j * 32;  // >= 1
    if (rem < 32) v &= (1u << rem) - 1u;
    return v;
}

// The bits (bytes of the 4-byte form: 0xff each) of lane t's unit that lie in the rectangle.
GOL_EDIT_HD uint32_t gol_copy_mask(const gol_edit_geom &g, int64_t t)
{
    if (g.layout == GOL_EDIT_BYTES) return 0xffu;
    return g.layout == GOL_EDIT_BYTES4 ? gol_edit_bytes4(g, t, nullptr, 0) : gol_edit_word(g, t, nullptr, 0);
}

// Occupancy bits of a masked unit: the word itself (bit layouts), bit i = byte i != 0 (bytes).
GOL_EDIT_HD uint32_t gol_copy_occ(const gol_edit_geom &g, uint32_t v)
{
    if (g.layout == GOL_EDIT_BAND || g.layout == GOL_EDIT_STANDARD) return v;
    uint32_t o = 0;
    for (int i = 0; i < 4; ++i) o |= (uint32_t)(((v >> (8 * i)) & 0xffu) != 0) << i;
    return o;
}

// Pass 1 of the bounds for one lane and row, as the kernels and gol_bounds_host both run it: unit u
// (gol_edit_unit of the lane) of the board row at `brow` (gol_edit_row) loaded, masked to the
// rectangle (mask: gol_copy_mask of the lane) and turned into occupancy bits.
GOL_EDIT_HD uint32_t gol_copy_occ_unit(int32_t form, const gol_edit_geom &g, int64_t u, uint32_t mask, const void *brow)
{
    if (form == GOL_EDIT_BYTES) return ((const uint8_t *)brow)[u] != 0;
    return gol_copy_occ(g, ((const uint32_t *)brow)[u] & mask);
}

GOL_EDIT_HD int gol_copy_ctz(uint32_t v)  // v != 0
{
    return __builtin_ctz(v);
}
GOL_EDIT_HD int gol_copy_top(uint32_t v)  // v != 0: its highest set bit
{
    return 31 - __builtin_clz(v);
}

// The smallest and the largest rectangle column among the set bits of lane t's occupancy word
// occ != 0 (only bits of the rectangle are ever set).
GOL_EDIT_HD void gol_copy_cols(const gol_edit_geom &g, int64_t t, uint32_t occ, int64_t *cmin, int64_t *cmax)
{
    if (g.layout == GOL_EDIT_BYTES) {
        *cmin = *cmax = t;
    } else if (g.layout == GOL_EDIT_BAND) {  // slot m is bit (bit0 + carry + m) & 31: rotate slot 0 to bit 0
        const uint32_t s = gol_copy_band_bit(g, t, 0);
        const uint32_t rot = s ? (occ >> s) | (occ << (32 - s)) : occ;
        *cmin = t + (int64_t)gol_copy_ctz(rot) * g.units;
        *cmax = t + (int64_t)gol_copy_top(rot) * g.units;
    } else {  // standard / 4-byte words: cell = cells*t - bit0 + bit; lane 0's bits below bit0 wrapped
        const int64_t cells = g.layout == GOL_EDIT_STANDARD ? 32 : 4;
        const int64_t c0 = t * cells - (int64_t)g.bit0;
        const uint32_t low = t == 0 && g.wrap_c >= 0 ? occ & ((1u << g.bit0) - 1u) : 0u;
        const uint32_t main = occ & ~low;
        *cmin = main ? c0 + gol_copy_ctz(main) : g.wrap_c + gol_copy_ctz(low);
        *cmax = low ? g.wrap_c + gol_copy_top(low) : c0 + gol_copy_top(main);
    }
}
