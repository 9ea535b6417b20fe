// gol_strips.h -- which workgroup of a pipelined launch computes which output rows.  Shared by the
// two pipeline kernels (band_pipe_kernel, gol_band_pipe.hip; bytes_pipe_kernel, gol_bytes_pipe.hip),
// the launch code that picks a schedule (gol_kernels.hip), and the host (gol_strip_plan,
// include/golhip.h), so the row-range arithmetic the GPU runs is tested on the CPU; the strip-level
// twin of gol_edit.h.
//
// Two halves:
//  - StripMap, work_item, work_dir, pair_extent: the map a launch carries and the functions that
//    turn it and a workgroup id into (column group, rows [s0, s1), direction, claim counter).
//    Host and device compile them; the kernels call nothing else for their rows.
//  - band_strip_plan, bytes_strip_plan: the choice of a schedule (a StripPlan: strip length, map,
//    workgroup count, mode) as a pure function of the launch's shape and of two device
//    properties, the CU count and the workgroups of the kernel resident on the device at once.
//    Host only.  The launchers call them with the device's values; gol_strip_plan and the
//    pretended-device launchers (gol_dev_*_on) with the caller's.
#pragma once
#include <stdint.h>

#include "golhip.h"  // GOL_STRIPS_* (the mode names)

#if defined(__HIPCC__) || defined(__CUDACC__)
#define GOL_STRIPS_HD __host__ __device__ inline __attribute__((always_inline))  // (no HIP header needed)
#else
#define GOL_STRIPS_HD inline
#endif

// ------------------------------------------------------------------ pipeline shapes
// Band pipeline, k = KW * P = 12: KW stages in each of P waves; blocks of GOL_BAND_RPB rows (one
// pair step), rings of GOL_BAND_NS slots (the role loops are unrolled over the slots).
#ifndef GOL_BAND_KW
#define GOL_BAND_KW 3
#endif
#define GOL_BAND_P 4
#define GOL_BAND_RPB 2
#define GOL_BAND_NS 4
// Byte pipeline, k = KW * P = 32: blocks of GOL_BYTES_RPB rows (two pair steps); NS hand-off slots
// between the waves, NSI input slots of the first wave (2 blocks in flight); the role loops are
// unrolled over NS (NSI divides it).
#ifndef GOL_BYTES_PIPE_KW
#define GOL_BYTES_PIPE_KW 4
#define GOL_BYTES_PIPE_P 8
#endif
#define GOL_BYTES_RPB 4
#ifndef GOL_BYTES_NS
#define GOL_BYTES_NS 3
#endif
#ifndef GOL_BYTES_NSI
#define GOL_BYTES_NSI 3
#endif
#ifndef GOL_BYTES_PER_CU
#define GOL_BYTES_PER_CU 3  // workgroups per CU of a one-round launch
#endif

namespace golk {

GOL_STRIPS_HD constexpr int band_halo_lanes(int k, int dw) { return (k + dw - 1) / dw; }
GOL_STRIPS_HD constexpr int band_useful_words(int k, int dw) { return (64 - 2 * band_halo_lanes(k, dw)) * dw; }

// Rows per wave strip are capped so a lane's 32-bit alive count cannot overflow.
constexpr int GOL_MAX_STRIP = 1 << 24;

// ------------------------------------------------------------------ the map of a launch
// Work items of the pipelined kernels (one workgroup = one column group x one strip of rows).
// ranked = 0: equal strips of `strip` rows, workgroup l -> XCD-remapped item.  ranked = 1 (a
// launch of exactly one round, cus x per_cu workgroups): the dispatcher deals workgroup l to CU
// l % cus as the (l / cus)-th arrival there, and a SIMD issues to its oldest ready wave first,
// so the CU's workgroups run at different speeds (one round of equal strips ended them at 247 /
// 298 / 388 / 482 us, tools/timeline.py); each CU then takes one column group x `period` rows
// and splits the rows by arrival rank: rank r gets len[r] rows at off[r].
// Paired ranks (dir != 0): two workgroups of a CU share one row range [off, off + len) and
// walk it from both ends (dir +1 down from its top, dir -1 up from its bottom), claiming input
// blocks from a counter of the pair (claims: 16 words per (CU, pair slot): [0] blocks claimed,
// [1] pipelines done; the second to finish zeroes both for the next launch).  The range [s0, s1)
// is stretched to s1e (pair_extent) so that RPB * (claimed blocks of both) = s1e - s0 + 4K
// exactly: a walker that claimed n blocks read RPB * n rows and, 2K rows behind its input,
// stored RPB * n - 2K of them, so the two stored RPB * nclaim - 4K = s1e - s0 rows, which meet
// without overlap wherever the faster one got to: no rank waits for a slower one at the end of
// the launch.
// Tail (ranked = 0, launches of many rounds): workgroups l >= tail_l, the last dispatched,
// take strips of tail_strip rows from row tail_row on, so the launch ends on short strips
// instead of a partial round of full ones.
struct StripMap {
    int32_t ranked, cus, per_cu, period;
    int32_t len[4], off[4];
    int32_t dir[4], pslot[4];
    uint32_t *claims;
    int32_t chunk;  // blocks per claim
    int32_t tail_l, tail_row, tail_strip;
};

GOL_STRIPS_HD int strips_min(int a, int b) { return a < b ? a : b; }

// Column group, strip [s0, s1) and a per-CU rotation index of workgroup l (1-D grid); false: the
// workgroup has no rows.  nwg() is the launch's workgroup count, asked for only by the map that
// needs it (the kernels pass a read of gridDim.x: as a plain value it was loaded at every kernel's
// start and the pipe kernels came out with other code).
template <class Count>
GOL_STRIPS_HD bool work_item(const StripMap &sm, int ngroups, int64_t row0, int64_t rows, int strip, int l, Count nwg,
                             int &group, int &s0, int &s1, int &rot)
{
    const int end = (int)(row0 + rows);
    if (!sm.ranked && sm.tail_l && l >= sm.tail_l) {
        const int i = l - sm.tail_l;
        group = i % ngroups;
        const int t = i / ngroups;
        s0 = (int)row0 + sm.tail_row + t * sm.tail_strip;
        s1 = strips_min(s0 + sm.tail_strip, end);
        rot = group + t;
    } else if (!sm.ranked) {
        // XCD-aware order: workgroups are dispatched round-robin over the 8 XCDs (L2 per XCD), so
        // consecutive ids are remapped to let each XCD walk its own contiguous run of column groups
        // of a strip: the lateral halo columns two neighbouring groups both read then meet in one L2.
        const int n = sm.tail_l ? sm.tail_l : (int)nwg(), per = n / 8;
        const int m = l < per * 8 ? (l % 8) * per + l / 8 : l;
        group = m % ngroups;
        const int by = m / ngroups;
        s0 = (int)row0 + by * strip;
        s1 = strips_min(s0 + strip, sm.tail_l ? (int)row0 + sm.tail_row : end);
        rot = group + by;
    } else {
        const int rank = l / sm.cus, c = l % sm.cus;
        const int c2 = (c % 8) * (sm.cus / 8) + c / 8;  // contiguous CUs per XCD (cus % 8 == 0)
        group = c2 % ngroups;
        const int t = c2 / ngroups;
        s0 = (int)row0 + t * sm.period + sm.off[rank];
        s1 = strips_min(s0 + sm.len[rank], end);
        rot = rank;
    }
    return s0 < s1;
}
// Direction and claim counter of workgroup l (0 / nullptr: a static strip).
GOL_STRIPS_HD int work_dir(const StripMap &sm, int l, uint32_t *&ctr)
{
    ctr = nullptr;
    if (!sm.ranked) return 0;
    const int rank = l / sm.cus, c = l % sm.cus;
    if (!sm.dir[rank]) return 0;
    ctr = sm.claims + ((int64_t)c * 2 + sm.pslot[rank]) * 16;
    return sm.dir[rank];
}
// A pair's range [s0, s1), stretched to s1e so that a loop trip (TRIP = RPB * NS rows) divides
// its len + 4K (whole loop trips; rows past s1 are read clamped and never stored), and the blocks
// of the pair, a multiple of NS.  dir 0 (a static strip): s1e = s1.  The two expressions are
// macros, and the kernels expand them in place: as an inlined function of the same text, with the
// constants as arguments or as template arguments, both pipe kernels came out with other scalar
// code (the compiler reassociates the sums together with the kernel's own uses of s1 - s0, and
// did so differently), and a change of the schedule's arithmetic must not be a change of the hot
// loops.  pair_extent is the same pair of expressions for the host.
#define GOL_PAIR_S1E(dir, s0, s1, K, TRIP) \
    ((dir) ? (s0) + (((s1) - (s0) + 4 * (K) + (TRIP) - 1) / (TRIP)) * (TRIP) - 4 * (K) : (s1))
#define GOL_PAIR_NCLAIM(s0, s1e, K, RPB) (((s1e) - (s0) + 4 * (K)) / (RPB))
template <int K, int RPB, int NS>
GOL_STRIPS_HD void pair_extent(int dir, int s0, int s1, int &s1e, int &nclaim)
{
    constexpr int TRIP = RPB * NS;  // rows per loop trip
    s1e = GOL_PAIR_S1E(dir, s0, s1, K, TRIP);
    nclaim = GOL_PAIR_NCLAIM(s0, s1e, K, RPB);
}

// ------------------------------------------------------------------ the choice of a schedule
// Rows per arrival rank, from measurements (tools/timeline.py, same-box A/B with tools/ab.py):
// one round of equal strips ended the ranks' workgroups at T_r (band 247 / 298 / 388 / 482 us,
// bytes 96 / 136 / 174 us), so the static split gives rank r a share ~ 1 / T_r, refined by
// re-measuring (w_r <- w_r T_mean / T_r).  With paired ranks (StripMap) only the sum over a
// pair matters: band pairs (0, 3) and (1, 2) ran at equal speed (65536^2: 0.54 / 0.46 ended
// them at 425 / 360 us; 50 / 50: 110.3 TCUPS vs 106.2 for the static split, same box); bytes
// pair (0, 2) with rank 1 alone on 0.31 of the rows.
#ifndef GOL_BAND_RANK_W
#define GOL_BAND_RANK_W 0.25, 0.25, 0.25, 0.25
#endif
#ifndef GOL_BYTES_RANK_W
#define GOL_BYTES_RANK_W 0.4457, 0.33, 0.2449, 0.0  // lone rank 1: 0.31 -> 0.33 after the fill skip (+1.3 %)
#endif
// Rounds of short tail strips (StripMap.tail_*), 1 / GOL_BAND_TAIL_DIV of a strip's rows each.
// Round 3, half-length strips, same box, 2^17 x 2^20: none 137.2 TCUPS, 0.5 round 138.8, 1.0
// 138.8, 1.5 138.6; 262144^2: 132.2 / 133.6 / 133.2 / 133.0.  Round 6, weak board, two boxes, 3 + 4
// reps against half-length strips for 0.5 round: quarter-length strips for 1 round +0.5 / +0.6 %,
// for 0.5 round +0.1 %, 0.25 round -1.1 %, 1.5 rounds -0.4 %; third-length -0.3 %, eighth-length
// -0.1 % (profiles/r06/r06_ab_tail.log).
#ifndef GOL_BAND_TAIL
#define GOL_BAND_TAIL 1.0
#endif
#ifndef GOL_BAND_TAIL_DIV
#define GOL_BAND_TAIL_DIV 4
#endif
#ifndef GOL_BAND_PAIRED
#define GOL_BAND_PAIRED 1
#endif
#ifndef GOL_BYTES_PAIRED
#define GOL_BYTES_PAIRED 1
#endif
// Rows per strip of the band pipeline's launches of many rounds (same box, weak board, 3 reps:
// 1024 148.4 TCUPS, 2048 148.3, 4096 147.0; profiles/r04/r04d_ab_rounds.jsonl)
#ifndef GOL_BAND_STRIP
#define GOL_BAND_STRIP 1024
#endif
// Band launches of up to this many rounds of strips run as one round of rank-weighted, paired
// ranges instead, when their column groups spread over the CUs (rank_split).  Same box, 3 reps
// each: config 4's N = 4 share 65536 x 262144 (2.95 rounds of 781-row strips) 134.2 -> 148.3
// TCUPS at 4 rounds; at 16 rounds the N = 2 share 131072 x 262144 (4.5 rounds) 142.0 -> 150.2
// and the whole 262144^2 board (9 rounds) 145.3 -> 149.4 (profiles/r04/r04d_ab_*.jsonl).  The
// weak board's 133 column groups spread over 256 CUs only one per CU (52 %): strips.
#ifndef GOL_BAND_RANK_ROUNDS
#define GOL_BAND_RANK_ROUNDS 16
#endif

// The schedule of one launch: strips of `strip` rows (ranked maps: unused), nwg workgroups, mode
// GOL_STRIPS_* (include/golhip.h).  sm.claims is left null: the launcher sets it.
struct StripPlan {
    int32_t mode, strip, ngroups;
    int64_t nwg;
    StripMap sm;
};

inline int64_t strips_min64(int64_t a, int64_t b) { return a < b ? a : b; }
inline int64_t strips_max64(int64_t a, int64_t b) { return a > b ? a : b; }

// Strip length for a one-workgroup-per-(column group, strip) kernel on a board that fills the
// device only a few times over: the strip count is a multiple of the strips that fit in one
// round of resident workgroups, so the last round is not a small remainder (e.g. 65536^2 at
// k = 12: 9 groups x 228 strips = 2052 workgroups was 2 rounds + 4 workgroups).  Boards of
// many rounds (more than 4) keep their strip: false (their tail is a small fraction already).
inline bool round_tiled_strip(int64_t rows, int64_t ngroups, int64_t slots, int64_t min_rows, int64_t cap, int32_t &strip)
{
    if (slots <= 0 || rows <= 0) return false;
    const int64_t per_round = strips_max64(1, slots / ngroups);
    const int64_t rounds = (rows + per_round * cap - 1) / (per_round * cap);
    if (rounds > 4) return false;
    const int64_t nstrips = per_round * rounds;
    const int64_t st = (rows + nstrips - 1) / nstrips;
    strip = (int32_t)strips_min64(rows, strips_max64(st, min_rows));
    return true;
}

// Rank-weighted strips for a launch of exactly one round (StripMap): every CU takes one column
// group x `period` rows and its per_cu workgroups split them in proportion to `weight[rank]`,
// the measured relative speed of the rank-th arrival on a CU.  Used when the strips of one
// column group can be spread over the CUs with little waste (ngroups x strips per group >= 94 %
// of the CUs) and every rank still gets >= min_rows rows; else false (equal strips).
inline bool rank_split(int64_t rows, int64_t ngroups, int cus, int per_cu, const double *weight, int64_t min_rows,
                       int64_t max_strip, StripMap &sm, bool paired, int chunk = 0, int max_rounds = 2)
{
    if (cus <= 0 || cus % 8 || per_cu < 1 || per_cu > 4 || ngroups > cus || rows <= 0) return false;
    // only boards that fill the device at most max_rounds times with strips of max_strip rows: on
    // bigger boards workgroups refill the CUs as they finish, and only the last round has the tail
    if (ngroups * ((rows + max_strip - 1) / max_strip) > max_rounds * (int64_t)cus * per_cu) return false;
    const int64_t t = cus / ngroups;  // strips per column group, one CU each
    if (t * ngroups * 100 < (int64_t)cus * 94) return false;
    const int64_t period = (rows + t - 1) / t;
    double wsum = 0;
    for (int r = 0; r < per_cu; ++r) wsum += weight[r];
    StripMap m{};
    m.ranked = 1;
    m.cus = cus;
    m.per_cu = per_cu;
    m.period = (int32_t)period;
    if (paired && per_cu >= 2) {
        // pairs walking one range from both ends: per_cu 2: (0, 1); 3: (0, 2) + rank 1 alone;
        // 4: (0, 3) + (1, 2).  A pair's range gets the sum of its ranks' weights.
        static const int pa[4][2] = {{0, 0}, {0, 0}, {0, 1}, {0, 2}};
        int ga[2][2];
        int ng = 0;
        if (per_cu == 4) { ga[0][0] = 0; ga[0][1] = 3; ga[1][0] = 1; ga[1][1] = 2; ng = 2; }
        else { ga[0][0] = pa[per_cu][0]; ga[0][1] = pa[per_cu][1]; ng = 1; }
        m.chunk = chunk;
        int64_t off = 0;
        double wused = 0;
        for (int g = 0; g < ng; ++g) {
            const double w = weight[ga[g][0]] + weight[ga[g][1]];
            wused += w;
            const int64_t len = (g == ng - 1 && per_cu != 3) ? period - off : (int64_t)(period * wused / wsum + 0.5) - off;
            if (len < min_rows) return false;
            for (int j = 0; j < 2; ++j) {
                const int r = ga[g][j];
                m.off[r] = (int32_t)off;
                m.len[r] = (int32_t)len;
                m.dir[r] = j == 0 ? 1 : -1;
                m.pslot[r] = g;
            }
            off += len;
        }
        if (per_cu == 3) {  // rank 1: the rest, a static strip
            if (period - off < min_rows) return false;
            m.off[1] = (int32_t)off;
            m.len[1] = (int32_t)(period - off);
        }
        sm = m;
        return true;
    }
    int64_t off = 0;
    for (int r = 0; r < per_cu; ++r) {
        const int64_t len = r == per_cu - 1 ? period - off : (int64_t)(period * weight[r] / wsum + 0.5);
        if (len < min_rows) return false;
        m.len[r] = (int32_t)len;
        m.off[r] = (int32_t)off;
        off += len;
    }
    sm = m;
    return true;
}

inline int32_t ranked_mode(const StripMap &sm)
{
    for (int r = 0; r < sm.per_cu; ++r)
        if (sm.dir[r]) return GOL_STRIPS_RANKED_PAIRED;
    return GOL_STRIPS_RANKED_STATIC;
}

// The band pipeline's launch (k = 12, 4 words per lane) of `rows` rows of a board Wd words wide,
// pitch words apart, on a device of `cus` CUs holding `slots` resident workgroups of the kernel.
// strip_rows > 0: the caller's strips.  can_pair: the launch has claim counters.
inline StripPlan band_strip_plan(int64_t rows, int64_t Wd, int64_t pitch, int k, int strip_rows, int cus, int64_t slots,
                                 bool can_pair = true)
{
    constexpr int KW = GOL_BAND_KW, P = GOL_BAND_P;
    static const double weight[4] = {GOL_BAND_RANK_W};
    const int U = band_useful_words(k, 4);
    StripPlan p{};
    p.ngroups = (int32_t)((Wd + U - 1) / U);
    // one workgroup per (column group, strip): strips up to 1024 rows (measured best at k = 12)
    // Boards with fewer than ~256 tiles of 8k rows are latency-bound (a launch lasts one
    // pipeline's walk over strip + 2k rows): ~512 tiles of >= 2 rows instead, without the
    // one-round rank split (1024^2: 2.6 us per turn vs 5.1 at 96 rows; 4096^2: 3.0 vs 5.2;
    // 8192^2: 4.1 vs 5.3; 16384^2 keeps the rank split: 6.0 vs 6.4 with 96-row tiles;
    // profiles/r03/r03q_small.jsonl)
    const int64_t work = rows * p.ngroups;
    const bool small = strip_rows <= 0 && work < (int64_t)8 * k * 256;
    int64_t st;
    if (small)
        st = strips_min64(rows, strips_max64(2, work / 512));
    else
        st = strip_rows > 0 ? strips_min64(strip_rows, GOL_MAX_STRIP)
                            : strips_min64(rows, strips_max64(8 * k, strips_min64(GOL_BAND_STRIP, work / 2048)));
    // the pipe kernel's stores address a strip as one buffer (32-bit range)
    p.strip = (int32_t)strips_max64(1, strips_min64(st, (int64_t(1) << 30) / (pitch * 4)));
    p.mode = small ? GOL_STRIPS_SMALL : (strip_rows > 0 ? GOL_STRIPS_EXPLICIT : GOL_STRIPS_PLAIN);
    const bool auto_strip = strip_rows <= 0 && !small;
    if (!auto_strip) {
        p.nwg = (int64_t)p.ngroups * ((rows + p.strip - 1) / p.strip);
        return p;
    }
    // one round of rank-weighted ranges, when it applies; a range's stores: one 32-bit buffer
    StripMap m{};
    if ((can_pair || !GOL_BAND_PAIRED) && cus > 0 && slots > 0 &&
        rank_split(rows, p.ngroups, cus, (int)(slots / cus), weight, 8 * KW * P, 1024, m, GOL_BAND_PAIRED, GOL_BAND_NS,
                   GOL_BAND_RANK_ROUNDS) &&
        (int64_t)m.period * pitch * 4 < (int64_t(1) << 31)) {
        p.sm = m;
        p.nwg = (int64_t)cus * m.per_cu;
        p.mode = ranked_mode(m);
        return p;
    }
    if (round_tiled_strip(rows, p.ngroups, slots, 8 * KW * P, 1024, p.strip)) p.mode = GOL_STRIPS_ROUND_TILED;
    p.nwg = (int64_t)p.ngroups * ((rows + p.strip - 1) / p.strip);
    if (GOL_BAND_TAIL > 0 && slots > 0 && p.nwg > 4 * slots) {
        // the last ~GOL_BAND_TAIL rounds of workgroups run strips of 1 / GOL_BAND_TAIL_DIV of the rows
        const int64_t ts = strips_max64(8 * KW * P, p.strip / GOL_BAND_TAIL_DIV);
        const int64_t nt = (int64_t)(GOL_BAND_TAIL * (double)slots / p.ngroups + 0.999);  // tail strips per group
        const int64_t tail_rows = strips_min64(rows / 2, nt * ts);
        const int64_t big = rows - tail_rows;
        const int64_t nbig = (big + p.strip - 1) / p.strip;
        p.sm.tail_l = (int32_t)(p.ngroups * nbig);
        p.sm.tail_row = (int32_t)big;
        p.sm.tail_strip = (int32_t)ts;
        p.nwg = p.sm.tail_l + p.ngroups * ((tail_rows + ts - 1) / ts);
        p.mode = GOL_STRIPS_TAIL;
    }
    return p;
}

// The byte pipeline's largest strip: the last wave stores a strip through one buffer descriptor
// (strip rows x pitch bytes < 2^31).
inline int64_t bytes_max_rows(int64_t pitch) { return strips_max64(1, ((int64_t(1) << 31) - 1) / pitch - 1); }

// The byte pipeline's launch (k = 32) of `rows` rows of a board W cells wide, pitch bytes apart:
// one workgroup of GOL_BYTES_PIPE_P waves per (column group, strip): rank-weighted strips in one
// round, else round-tiled strips >= 4k rows.  can_pair: the launch has claim counters (without:
// the static split).
inline StripPlan bytes_strip_plan(int64_t rows, int64_t W, int64_t pitch, int k, int strip_rows, int cus, int64_t slots,
                                  bool can_pair = true)
{
    static const double weight[4] = {GOL_BYTES_RANK_W};
    StripPlan p{};
    p.ngroups = (int32_t)((W / 32 + 61) / 62);
    const int64_t max_rows = bytes_max_rows(pitch);
    StripMap m{};
    if (strip_rows <= 0 && cus > 0 &&
        rank_split(rows, p.ngroups, cus, (int)strips_min64(GOL_BYTES_PER_CU, slots / cus), weight, 2 * k, 1024, m,
                   GOL_BYTES_PAIRED && can_pair, GOL_BYTES_NS) &&
        m.period <= max_rows) {
        p.sm = m;
        p.nwg = (int64_t)cus * m.per_cu;
        p.mode = ranked_mode(m);
        return p;
    }
    if (strip_rows > 0) {
        p.strip = (int32_t)strips_min64(strip_rows, GOL_MAX_STRIP);
        p.mode = GOL_STRIPS_EXPLICIT;
    } else {
        p.strip = (int32_t)strips_min64(rows, strips_max64(8 * k, rows * p.ngroups / 1024));
        p.mode = round_tiled_strip(rows, p.ngroups, slots, 4 * k, 1024, p.strip) ? GOL_STRIPS_ROUND_TILED : GOL_STRIPS_PLAIN;
    }
    p.strip = (int32_t)strips_min64(p.strip, max_rows);
    p.nwg = (int64_t)p.ngroups * ((rows + p.strip - 1) / p.strip);
    return p;
}

}  // namespace golk
