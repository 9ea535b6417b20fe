// gol_step_launch.h -- one launch of a step kernel as data: the table of the step kernels, the
// descriptor of a launch, the one check of what makes it valid and the geometry that follows from
// it.  The launcher (golk_step, gol_kernels.hip), the C entries (gol_abi.cpp), the engine
// (gol_step.cpp) and the export gol_step_check_host (gol_step_host.cpp) all read this file and
// nothing else for these questions.  No HIP header: a plain C++ program can include it
// (step_check.cpp); the launch twin of gol_batch.h.
#pragma once
#include <stdint.h>

#include "gol_strips.h"  // band_useful_words, GOL_MAX_STRIP; golhip.h: GOL_FAMILY_*

// ------------------------------------------------------------------ the kernel table
// Words per lane: of the life-like rule kernels (both layouts), and the defaults of
// cells_per_lane <= 0 (standard layout: 64 cells per lane; band: 128).
#define GOLK_RULE_DW 2
#define GOL_DEFAULT_DW 2
#ifndef GOL_BAND_DEFAULT_DW
#define GOL_BAND_DEFAULT_DW 4
#endif

#define GOL_STEP_PIPELINED 1    // a split pipeline (gol_band_pipe.hip, gol_bytes_pipe.hip): one workgroup
                                // per (column group, range of rows), strips from a plan (gol_strips.h)
#define GOL_STEP_ENGINE_ONLY 2  // the engine launches it (band layout, cells_per_lane=64,
                                // turns_per_launch=12), the C entry gol_dev_band_step refuses it
#define GOL_STEP_MAX_K 32

// Every step kernel, once: X(family, k turns per launch, words per lane, flags).  The dispatch of
// gol_kernels.hip expands this list, so an instantiation is added or removed by one line here.
// BITS, BAND: bits_step_kernel<K, DW>, band_step_kernel<K, DW, CONTIG> (B3/S23); RULE_STD,
// RULE_BAND: their TableRule forms; BYTES: bytes_blocked_kernel<K> (a lane holds one word of 32
// cells).  k = 16 keeps its whole pipeline in registers up to 2 words per lane only.
#define GOL_STEP_KERNELS(X)                                                                        \
    X(BITS, 1, 1, 0) X(BITS, 2, 1, 0) X(BITS, 4, 1, 0) X(BITS, 8, 1, 0) X(BITS, 16, 1, 0)          \
    X(BITS, 1, 2, 0) X(BITS, 2, 2, 0) X(BITS, 4, 2, 0) X(BITS, 8, 2, 0) X(BITS, 16, 2, 0)          \
    X(BITS, 1, 4, 0) X(BITS, 2, 4, 0) X(BITS, 4, 4, 0) X(BITS, 8, 4, 0)                            \
    X(BAND, 1, 2, 0) X(BAND, 2, 2, 0) X(BAND, 4, 2, 0) X(BAND, 8, 2, 0) X(BAND, 16, 2, 0)          \
    X(BAND, 12, 2, GOL_STEP_ENGINE_ONLY)                                                           \
    X(BAND, 1, 4, 0) X(BAND, 2, 4, 0) X(BAND, 4, 4, 0) X(BAND, 8, 4, 0)                            \
    X(BAND, 12, 4, GOL_STEP_PIPELINED)                                                             \
    X(RULE_STD, 1, 2, 0) X(RULE_STD, 2, 2, 0) X(RULE_STD, 4, 2, 0) X(RULE_STD, 8, 2, 0)            \
    X(RULE_BAND, 1, 2, 0) X(RULE_BAND, 2, 2, 0) X(RULE_BAND, 4, 2, 0) X(RULE_BAND, 8, 2, 0)        \
    X(BYTES, 1, 1, 0) X(BYTES, 2, 1, 0) X(BYTES, 4, 1, 0) X(BYTES, 8, 1, 0) X(BYTES, 16, 1, 0)     \
    X(BYTES, 32, 1, GOL_STEP_PIPELINED)

constexpr int gol_step_key(int family, int k, int dw) { return (family * 64 + k) * 8 + dw; }
constexpr bool gol_step_band(int family) { return family == GOL_FAMILY_BAND || family == GOL_FAMILY_RULE_BAND; }
constexpr bool gol_step_rule(int family) { return family == GOL_FAMILY_RULE_STD || family == GOL_FAMILY_RULE_BAND; }

// Is (family, k, dw) a kernel, is it pipelined, do the C entries offer it, and how many output
// words does a wave produce (its column group): 62 lanes of dw words, the band layout's 64 lanes
// less ceil(k / dw) halo lanes a side, 62 words of 32 byte cells.
struct gol_step_kernel {
    bool exists, pipelined, offered;
    int useful;
};

inline gol_step_kernel gol_step_kernel_of(int family, int k, int dw)
{
    if (family < GOL_FAMILY_BITS || family > GOL_FAMILY_BYTES || k < 1 || k > GOL_STEP_MAX_K || dw < 1 || dw > 4) return {};
    int flags;
    switch (gol_step_key(family, k, dw)) {
#define GOL_STEP_CASE(F, K, DW, FLAGS) case gol_step_key(GOL_FAMILY_##F, K, DW): flags = (FLAGS); break;
    GOL_STEP_KERNELS(GOL_STEP_CASE)
#undef GOL_STEP_CASE
    default: return {};
    }
    const int useful = family == GOL_FAMILY_BYTES ? 62 : (gol_step_band(family) ? golk::band_useful_words(k, dw) : 62 * dw);
    return {true, (flags & GOL_STEP_PIPELINED) != 0, !(flags & GOL_STEP_ENGINE_ONLY), useful};
}

// The largest k <= limit that is a kernel of (family, dw) -- offered: that the C entries offer --
// or 0.
inline int gol_step_max_k(int family, int dw, int64_t limit, bool offered = false)
{
    for (int k = (int)(limit < GOL_STEP_MAX_K ? limit : GOL_STEP_MAX_K); k >= 1; --k) {
        const gol_step_kernel kn = gol_step_kernel_of(family, k, dw);
        if (kn.exists && (kn.offered || !offered)) return k;
    }
    return 0;
}

// Words per lane of a C entry's cells_per_lane (<= 0: the family's default); 0, or a value the
// table does not have: not one of the family's.
inline int gol_step_dw(int family, int32_t cells_per_lane)
{
    switch (family) {
    case GOL_FAMILY_BITS: return cells_per_lane > 0 ? cells_per_lane / 32 : GOL_DEFAULT_DW;
    case GOL_FAMILY_BAND: return cells_per_lane == 64 ? 2 : (cells_per_lane == 128 ? 4 : (cells_per_lane <= 0 ? GOL_BAND_DEFAULT_DW : 0));
    case GOL_FAMILY_BYTES: return 1;
    default: return cells_per_lane <= 0 || cells_per_lane == 32 * GOLK_RULE_DW ? GOLK_RULE_DW : 0;
    }
}

// ------------------------------------------------------------------ one launch
// The pointers are device memory; a row is `width` units wide and `pitch` units from the next:
// uint32 words of 32 cells for the bit families, bytes (one per cell) for BYTES.
struct gol_step_launch {
    int32_t family;              // GOL_FAMILY_*
    const void *top, *mid, *bot; // input row y of the shard (-k <= y < R + k): top + (y + k) pitch for y < 0,
                                 // mid + y pitch for 0 <= y < R, bot + (y - R) pitch for y >= R
    void *dst;                   // row y of the output at dst + y pitch
    int64_t R;                   // rows of the shard
    int64_t width, pitch;        // Wd words (bytes: W cells) of a row; units from a row to the next
    int64_t row0, rows;          // the launch writes rows [row0, row0 + rows) of dst; rows == 0: nothing
    int32_t k, dw;               // turns per launch and words per lane: a kernel of the table
    int32_t strip_rows;          // output rows per strip; <= 0: gol_step_auto_strip (a pipeline: its plan's)
    uint32_t birth, survive;     // the rule families' 9-bit masks over the neighbour count (gol_rule.h)
    uint64_t *slots;             // GOL_COUNT_SLOTS * 8 counters the alive cells written are added to, or NULL
    uint32_t *err;               // the launch's error word (BAND, BYTES); NULL: the device's default word
    int32_t as_cus;              // a pipelined kernel: schedule as for a device of as_cus CUs holding
    int64_t as_slots;            // as_slots resident workgroups of the kernel; 0, 0: this device
};

// What makes a launch valid; everything else is refused and nothing is launched.  offered: as a C
// entry, which does not offer the engine-only kernel.  What needs the device -- as_cus and
// as_slots not above what it has -- is checked where it is known (gol_launch.cpp pipe_device).
inline bool gol_step_launch_ok(const gol_step_launch &l, bool offered = false)
{
    const bool bytes = l.family == GOL_FAMILY_BYTES;
    const gol_step_kernel kn = gol_step_kernel_of(l.family, l.k, l.dw);
    // the four segments
    if (!l.top || !l.mid || !l.bot || !l.dst) return false;
    // a kernel of the table, and a shard that holds the k rows its neighbours read
    if (!kn.exists || (offered && !kn.offered) || l.k > l.R) return false;
    // a board, and rows that do not overlap
    if (l.R <= 0 || l.width <= 0 || l.pitch < l.width) return false;
    // whole lanes: dw words of a bit row in width and pitch; a byte row 32 cells in width, 16 bytes in pitch
    if (l.width % (bytes ? 32 : l.dw) || l.pitch % (bytes ? 16 : l.dw)) return false;
    // the rows written lie in the shard
    if (l.row0 < 0 || l.rows < 0 || l.row0 + l.rows > l.R) return false;
    // a lane's load is aligned: 4 dw bytes (BAND, RULE_*), 16 bytes (BYTES).  BITS has no such
    // clause: gol_dev_bits_step never had one, and it is kept that way (a 4-byte uint32 pointer).
    const uintptr_t align = l.family == GOL_FAMILY_BITS ? 1 : (bytes ? 16 : 4 * (uintptr_t)l.dw);
    if (((uintptr_t)l.top | (uintptr_t)l.mid | (uintptr_t)l.bot | (uintptr_t)l.dst) & (align - 1)) return false;
    // the rule families' masks are 9 bits (the others do not read them)
    if (gol_step_rule(l.family) && (l.birth >= 512 || l.survive >= 512)) return false;
    // a pretended device: none, or for a pipelined kernel both values, the CUs in whole groups of 8
    if ((l.as_cus || l.as_slots) && (!kn.pipelined || l.as_cus <= 0 || l.as_slots <= 0 || l.as_cus % 8)) return false;
    return true;
}

// ------------------------------------------------------------------ the geometry of a valid launch
// Strip length of the one-wave kernels without a strip_rows: `rows` output rows, ngroups column groups.
inline int gol_step_auto_strip(int64_t rows, int64_t ngroups, int k)
{
    // aim for >= ~8192 waves (32 per CU) but no longer than 64*k rows: the 2k halo rows then
    // cost <= 1/32 (measured best on the 2^17 x 2^20 torus: 512 rows at k = 8, 1024 at k = 16)
    int64_t strip = rows * ngroups / 8192;
    const int64_t hi = 64 * (int64_t)k;
    if (strip > hi) strip = hi;
    int64_t lo = 8 * (int64_t)k;
    if (lo < 32) lo = 32;
    // a board too small for ~512 strips of lo rows (the reference's images: 512^2 is one column
    // group) is latency-bound: a launch lasts one wave's serial walk over strip + 2k rows, so
    // ~512 short strips win (512^2, k = 8: strip 1-2 -> 2.3 us per turn, 64 -> 5.8;
    // profiles/r03/r03q_small.jsonl)
    if (rows * ngroups < lo * 512) lo = rows * ngroups / 512 > 1 ? rows * ngroups / 512 : 1;
    if (strip < lo) strip = lo;
    if (strip > rows) strip = rows;
    if (strip < 1) strip = 1;
    return (int)strip;
}

struct gol_step_geometry {
    bool pipelined;
    bool contig;     // the ghost rows lie right above and below the shard: top + k pitch == mid, bot == mid + R pitch
    int32_t useful;  // output words of a wave
    int64_t words;   // words of 32 cells in a row
    int32_t ngroups; // column groups: ceil(words / useful)
    int32_t strip;   // rows per strip of a one-wave kernel (a pipeline's come from its plan)
};

// ngroups and strip of a kernel over rows of `words` words, `rows` of them per launch
inline void gol_step_strips(const gol_step_kernel &kn, int64_t words, int64_t rows, int k, int strip_rows, gol_step_geometry &g)
{
    g.pipelined = kn.pipelined;
    g.useful = kn.useful;
    g.words = words;
    g.ngroups = (int32_t)((words + kn.useful - 1) / kn.useful);
    g.strip = strip_rows > 0 ? (strip_rows < golk::GOL_MAX_STRIP ? strip_rows : golk::GOL_MAX_STRIP)
                             : gol_step_auto_strip(rows, g.ngroups, k);
}

inline gol_step_geometry gol_step_geometry_of(const gol_step_launch &l)  // gol_step_launch_ok(l)
{
    gol_step_geometry g;
    const int64_t unit = l.family == GOL_FAMILY_BYTES ? 1 : 4;  // bytes of a unit of width and pitch
    const uintptr_t mid = (uintptr_t)l.mid;
    g.contig = (uintptr_t)l.top + (uintptr_t)(l.k * l.pitch * unit) == mid && (uintptr_t)l.bot == mid + (uintptr_t)(l.R * l.pitch * unit);
    gol_step_strips(gol_step_kernel_of(l.family, l.k, l.dw), l.family == GOL_FAMILY_BYTES ? l.width / 32 : l.width, l.rows, l.k,
                    l.strip_rows, g);
    return g;
}
