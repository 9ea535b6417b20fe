// gol_edit.h -- a rectangle of cells pasted into a row of the board, in the layout the row is
// stepped in.  Shared by the paste kernels (gol_edit.hip) and the host (gol_paste_host,
// include/golhip.h), so the word function the GPU runs is tested on the CPU; the write-side twin of
// the viewport's mapping (gol_view.hip).
//
// Pattern cell c of a row (0 <= c < w <= W; bit c % 64 of word c / 64, all ones without a pattern)
// lands on board column (x0 + c) mod W.  A row of the rectangle covers T distinct units of the
// board row (words; bytes of a byte board), and unit-lane t (0 <= t < T) owns exactly one of them,
// so a plain read-modify-write per lane is race-free:
//  - band rows (bit b of word u = cell b*Wd + u): T = min(w, Wd); lane t owns word (x0 % Wd + t) mod
//    Wd and gathers pattern cells c = t + m*Wd, m = 0, 1, .., into bit (x0 / Wd + carry + m) & 31
//    (carry: the word index wrapped past Wd, i.e. the next band);
//  - standard rows (word s = cells 32s .. 32s+31): the rectangle spans n = ceil((x0 % 32 + w) / 32)
//    words from word x0 / 32; lane t takes the 32 pattern cells from c = 32t - x0 % 32 (a funnel
//    shift of two pattern words, masked to [0, w)).  n = Wd + 1 (the full width from the middle of
//    a word) would name the first word twice, so T = min(n, Wd) and lane 0 also applies the cells
//    that wrapped, from c = W - x0 % 32;
//  - byte rows: T = w, lane t owns byte (x0 + t) mod W; or, where the rows are 4-byte aligned (W % 4
//    == 0, pitch % 4 == 0, an aligned buffer: GOL_EDIT_BYTES4, chosen by gol_region_ok), the standard
//    form with 4 cells per aligned 4-byte word.
// Below the mapping: gol_region, what a launch of any region kernel or a call of a host twin is
// given, its one check, and the paste's step of one unit, which kernel and twin both call.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define GOL_EDIT_HD __host__ __device__ inline __attribute__((always_inline))  // (no HIP header needed)
#else
#define GOL_EDIT_HD inline
#endif

// (GOL_PASTE_* of include/golhip.h)
#define GOL_EDIT_COPY 0
#define GOL_EDIT_OR 1
#define GOL_EDIT_XOR 2
#define GOL_EDIT_ANDNOT 3
// layouts: gol_engine_info's bit_mode values (the views' src_layout)
#define GOL_EDIT_BYTES 0
#define GOL_EDIT_STANDARD 1
#define GOL_EDIT_BAND 2
#define GOL_EDIT_BYTES4 3  // (internal) byte rows as aligned 4-byte words, 4 cells each
// GOL_EDIT_BYTES4 for byte rows that allow it, else the layout itself (for gol_region_ok alone).
#define GOL_EDIT_FORM(layout, W, pitch, base) \
    ((layout) == GOL_EDIT_BYTES && (W) % 4 == 0 && (pitch) % 4 == 0 && (uintptr_t)(base) % 4 == 0 ? GOL_EDIT_BYTES4 : (layout))

struct gol_edit_geom {
    int64_t units;   // units per board row: Wd words, W bytes, or W / 4 words of 4 bytes
    int64_t first;   // unit of lane 0: band x0 % Wd, standard x0 / 32, bytes x0, byte words x0 / 4
    int64_t T;       // lanes: distinct units a row of the rectangle covers
    int64_t w;       // cells per pattern row
    int64_t wrap_c;  // standard, byte words: lane 0 also takes the pattern cells from here (-1: none)
    uint32_t bit0;   // band: x0 / Wd; standard: x0 % 32; byte words: x0 % 4
    int32_t layout, op;
};

// false: arguments outside 1 <= w <= W, 0 <= x0 < W, the layout's width rule, op 0..3.
GOL_EDIT_HD bool gol_edit_geom_init(gol_edit_geom &g, int32_t layout, int64_t W, int64_t x0, int64_t w, int32_t op)
{
    if (W < 1 || w < 1 || w > W || x0 < 0 || x0 >= W || op < GOL_EDIT_COPY || op > GOL_EDIT_ANDNOT) return false;
    g.layout = layout;
    g.op = op;
    g.w = w;
    g.wrap_c = -1;
    g.bit0 = 0;
    if (layout == GOL_EDIT_BYTES) {
        g.units = W;
        g.first = x0;
        g.T = w;
    } else if (layout == GOL_EDIT_STANDARD || layout == GOL_EDIT_BYTES4) {
        const int64_t cells = layout == GOL_EDIT_STANDARD ? 32 : 4;  // per unit
        if (W % cells != 0) return false;
        g.units = W / cells;
        g.first = x0 / cells;
        g.bit0 = (uint32_t)(x0 % cells);
        const int64_t n = ((int64_t)g.bit0 + w + cells - 1) / cells;  // <= units + 1
        g.T = n < g.units ? n : g.units;
        if (n > g.units) g.wrap_c = W - (int64_t)g.bit0;
    } else if (layout == GOL_EDIT_BAND) {
        if (W % 1024 != 0) return false;
        g.units = W / 32;
        g.first = x0 % g.units;
        g.bit0 = (uint32_t)(x0 / g.units);
        g.T = w < g.units ? w : g.units;
    } else {
        return false;
    }
    return true;
}

// The unit lane t owns (0 <= t < T <= units).
GOL_EDIT_HD int64_t gol_edit_unit(const gol_edit_geom &g, int64_t t)
{
    const int64_t u = g.first + t;  // < 2 * units
    return u >= g.units ? u - g.units : u;
}

// Pattern cell c (0 <= c < w) of the row at prow (NULL: 1).
GOL_EDIT_HD uint32_t gol_edit_pbit(const uint64_t *prow, int64_t c)
{
    return prow ? (uint32_t)(prow[c >> 6] >> (c & 63)) & 1u : 1u;
}

// Pattern cells c .. c + 31 (-32 < c < w) as a word, *mask = the bits with 0 <= cell < w; reads
// only the ceil(w / 64) words of the row, whatever their bits past w hold.
GOL_EDIT_HD uint32_t gol_edit_p32(const uint64_t *prow, int64_t w, int64_t c, uint32_t *mask)
{
    const uint32_t lo = c < 0 ? (uint32_t)-c : 0u;                // first valid bit, < 32
    const uint32_t hi = w - c < 32 ? (uint32_t)(w - c) : 32u;     // one past the last, 1 .. 32
    const uint32_t m = (hi >= 32 ? 0xffffffffu : (1u << hi) - 1u) & ~((1u << lo) - 1u);
    *mask = m;
    if (!prow) return m;
    const int64_t cc = c < 0 ? 0 : c;
    const int64_t i = cc >> 6, nw = (w + 63) >> 6;
    const uint32_t sh = (uint32_t)(cc & 63);
    uint64_t v = prow[i] >> sh;
    if (sh > 32 && i + 1 < nw) v |= prow[i + 1] << (64 - sh);
    return ((uint32_t)v << lo) & m;
}

// old with the pattern bits p applied under mask (p & ~mask == 0).
GOL_EDIT_HD uint32_t gol_edit_apply(uint32_t old, uint32_t p, uint32_t mask, int32_t op)
{
    switch (op) {
    case GOL_EDIT_COPY: return (old & ~mask) | p;
    case GOL_EDIT_OR: return old | p;
    case GOL_EDIT_XOR: return old ^ p;
    default: return old & ~p;
    }
}

// The new value of the word lane t owns (bit layouts); prow: the pattern row, or NULL.
GOL_EDIT_HD uint32_t gol_edit_word(const gol_edit_geom &g, int64_t t, const uint64_t *prow, uint32_t old)
{
    uint32_t p = 0, mask = 0;
    if (g.layout == GOL_EDIT_BAND) {
        const uint32_t carry = g.first + t >= g.units;
        uint32_t b = g.bit0 + carry;
        for (int64_t c = t; c < g.w; c += g.units, ++b) {  // at most 32 cells: w <= 32 units
            const uint32_t bit = 1u << (b & 31);
            mask |= bit;
            if (gol_edit_pbit(prow, c)) p |= bit;
        }
        return gol_edit_apply(old, p, mask, g.op);
    }
    p = gol_edit_p32(prow, g.w, t * 32 - (int64_t)g.bit0, &mask);
    uint32_t v = gol_edit_apply(old, p, mask, g.op);
    if (t == 0 && g.wrap_c >= 0) {  // the cells that wrapped into the first word (its bits below bit0)
        p = gol_edit_p32(prow, g.w, g.wrap_c, &mask);
        v = gol_edit_apply(v, p, mask, g.op);
    }
    return v;
}

// A byte cell (alive = non-zero) under pattern bit p: COPY writes 0 / 255, the other operations
// write only where p is set; a cell that is not written keeps its byte.
GOL_EDIT_HD uint8_t gol_edit_byte(uint8_t old, uint32_t p, int32_t op)
{
    if (op == GOL_EDIT_COPY) return p ? 255 : 0;
    if (!p) return old;
    if (op == GOL_EDIT_OR) return 255;
    if (op == GOL_EDIT_XOR) return old ? 0 : 255;
    return 0;
}

// The new value of the aligned 4-byte word lane t owns (GOL_EDIT_BYTES4: byte i = cell 4u + i).
GOL_EDIT_HD uint32_t gol_edit_bytes4(const gol_edit_geom &g, int64_t t, const uint64_t *prow, uint32_t old)
{
    uint32_t v = old;
    int64_t c0 = t * 4 - (int64_t)g.bit0;
    for (int pass = 0; pass < 2; ++pass) {
        for (int i = 0; i < 4; ++i) {
            const int64_t c = c0 + i;
            if (c < 0 || c >= g.w) continue;
            const uint32_t b = gol_edit_byte((uint8_t)(v >> (8 * i)), gol_edit_pbit(prow, c), g.op);
            v = (v & ~(0xffu << (8 * i))) | (b << (8 * i));
        }
        if (t != 0 || g.wrap_c < 0) break;  // lane 0: then the cells that wrapped into its first bytes
        c0 = g.wrap_c;
    }
    return v;
}

// Cells of a 4-byte word whose alive state (byte != 0) differs between a and b.
GOL_EDIT_HD int gol_edit_flips4(uint32_t a, uint32_t b)
{
    int n = 0;
    for (int i = 0; i < 4; ++i) n += (((a >> (8 * i)) & 0xffu) != 0) != (((b >> (8 * i)) & 0xffu) != 0);
    return n;
}

// ------------------------------------------------------------------ a region launch and its check
// What every region kernel (view, paste, copy, bounds: gol_region_kernels.h) and every host twin
// (gol_paste_host, gol_copy_host, gol_bounds_host) is given: a rectangle of a run of board rows.
struct gol_region {
    int32_t layout;     // how the rows are stored: GOL_EDIT_BYTES / _STANDARD / _BAND
    void *base;         // row 0 of the rows (a shard's rows; only the paste writes through it)
    int64_t pitch;      // units from a row to the next: words, bytes of a byte board
    int64_t W;          // cells per board row
    int64_t x0, w;      // cell c of a rectangle row, 0 <= c < w <= W, is board column (x0 + c) mod W
    int64_t row, rows;  // board rows [row, row + rows) ..
    int64_t at;         // .. are the pattern's, the rectangle's or the viewport's rows [at, at + rows)
};

// The one rule of a valid region: the layout 0..2, a base, row, rows, at >= 0, the geometry
// (gol_edit_geom_init: the columns, the layout's width rule, op) and a pitch of at least the
// layout's units per row.  words4: byte rows take their 4-byte form where GOL_EDIT_FORM allows it;
// g->layout is the form chosen.  false: *g holds nothing of use.
GOL_EDIT_HD bool gol_region_ok(const gol_region &r, int32_t op, bool words4, gol_edit_geom *g)
{
    if (r.layout < GOL_EDIT_BYTES || r.layout > GOL_EDIT_BAND || !r.base || r.row < 0 || r.rows < 0 || r.at < 0) return false;
    const int32_t form = words4 ? GOL_EDIT_FORM(r.layout, r.W, r.pitch, r.base) : r.layout;
    return gol_edit_geom_init(*g, form, r.W, r.x0, r.w, op) && r.pitch >= (r.layout == GOL_EDIT_BYTES ? r.W : g->units);
}

// A pattern buffer of `stride` words per row holds rows of w cells.
GOL_EDIT_HD bool gol_region_stride_ok(int64_t w, int64_t stride) { return stride >= (w + 63) / 64; }

// Row r of the rows at `base` in form `form` (a pitch counts bytes for both byte forms, else words).
GOL_EDIT_HD void *gol_edit_row(int32_t form, const void *base, int64_t pitch, int64_t r)
{
    if (form == GOL_EDIT_BYTES || form == GOL_EDIT_BYTES4) return (uint8_t *)base + r * pitch;
    return (uint32_t *)base + r * pitch;
}

// One lane's step of a paste, as the kernels and gol_paste_host both run it: the unit lane t owns
// (t < g.T; u = gol_edit_unit(g, t), which a kernel lane keeps over its rows) of the board row at
// `brow` (gol_edit_row) read, the pattern row `prow` (NULL: ones) applied, the unit stored if it
// changed.  Returns the cells whose alive state flipped.
GOL_EDIT_HD uint32_t gol_edit_paste_unit(int32_t form, const gol_edit_geom &g, int64_t t, int64_t u, void *brow, const uint64_t *prow)
{
    if (form == GOL_EDIT_BYTES4) {
        uint32_t *p = (uint32_t *)brow + u;
        const uint32_t old = *p, v = gol_edit_bytes4(g, t, prow, old);
        if (v != old) *p = v;
        return (uint32_t)gol_edit_flips4(old, v);
    }
    if (form == GOL_EDIT_BYTES) {
        uint8_t *p = (uint8_t *)brow + u;
        const uint8_t old = *p, v = gol_edit_byte(old, gol_edit_pbit(prow, t), g.op);
        if (v != old) *p = v;
        return (old != 0) != (v != 0);
    }
    uint32_t *p = (uint32_t *)brow + u;
    const uint32_t old = *p, v = gol_edit_word(g, t, prow, old);
    if (v != old) *p = v;
    return (uint32_t)__builtin_popcount(old ^ v);
}

#if defined(__HIPCC__)
// ------------------------------------------------------------------ device side (gol_edit.hip, gol_copy.hip)
#include <hip/hip_runtime.h>

#include <algorithm>

// Threads of a workgroup of the region kernels (paste, copy, bounds): lanes run along the units of a row.
constexpr int GOL_EDIT_BLOCK = 256;

// The wave's sum of n added to the device counter *sum by one lane (every lane of the wave takes
// part in the shuffles).
__device__ __forceinline__ void gol_edit_wave_add(uint32_t n, unsigned long long *sum)
{
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) n += __shfl_down(n, d, 64);
    if ((threadIdx.x & 63) == 0 && n) atomicAdd(sum, (unsigned long long)n);
}

// The grid of a region kernel over `lanes` lanes and `rows` rows: about 2048 workgroups at most; a
// workgroup strides over the rows that are left.  false: more lanes than a grid holds.
inline bool gol_edit_grid(int64_t lanes, int64_t rows, dim3 *grid)
{
    const int64_t nxb = (lanes + GOL_EDIT_BLOCK - 1) / GOL_EDIT_BLOCK;
    if (nxb > INT32_MAX) return false;
    const int64_t ny = std::min<int64_t>(rows, std::max<int64_t>(1, 2048 / nxb));
    *grid = dim3((unsigned)nxb, (unsigned)ny);
    return true;
}
#endif
