// gol_rule.hip -- life-like rules (B/S masks as data) on the bit board: the register pipeline of
// bits_step_kernel / band_step_kernel (gol_kernels.hip: one wave runs all K stages over a 3-row
// wavefront, same row addressing, strips, writer lanes and fused count) with the hard-wired
// B3/S23 tail replaced by the full 4-bit neighbourhood count and a mux tree over the rule's two
// tables (gol_rule.h).  Per word and generation: 2 ops of horizontal sums (band; the standard
// layout's shifted frame adds its 2 v_alignbit), 7 for the count, 19 for the rule.
#define GOL_TU_RULE 1
#include "gol_kernels.hip"
#include "gol_rule.h"

namespace golk {

struct RuleArgs {
    BitsArgs b;
    uint32_t birth, survive;
};

// One stage (generation g+1) of one row step S, in place on `cur`: band layout (centred sums, the
// centre is the word itself) or the standard layout's shifted frame (hsum_left).
template <int K, int DW, int S, bool BAND>
__device__ __forceinline__ void rstage(Pipe<K, DW> &p, const int g, uint32_t (&cur)[DW], const gol_rule_tab &tab)
{
    constexpr int SA = (S + 1) % 3, SM = (S + 2) % 3;
    if constexpr (BAND) {
#pragma unroll
        for (int j = 0; j < DW; ++j) p.cc[g][S][j] = cur[j];
        hsum_band<DW>(p.cc[g][S], p.h0[g][S], p.h1[g][S]);
    } else {
        hsum_left<DW>(cur, p.h0[g][S], p.h1[g][S], p.cc[g][S]);
    }
#pragma unroll
    for (int j = 0; j < DW; ++j) {
        uint32_t t0, t1, t2, t3;
        gol_rule_sum3(p.h0[g][SA][j], p.h1[g][SA][j], p.h0[g][SM][j], p.h1[g][SM][j], p.h0[g][S][j], p.h1[g][S][j],
                      t0, t1, t2, t3);
        cur[j] = gol_rule_eval(tab, t0, t1, t2, t3, p.cc[g][SM][j]);
    }
}

// The three rows of a block through the K stages as a wavefront (row S at stage w - S).
template <int K, int DW, bool BAND>
__device__ __forceinline__ void rblock(Pipe<K, DW> &p, uint32_t (&cur)[3][DW], const gol_rule_tab &tab)
{
#pragma unroll
    for (int w = 0; w < K + 2; ++w) {
        if (w < K) rstage<K, DW, 0, BAND>(p, w, cur[0], tab);
        if (w >= 1 && w - 1 < K) rstage<K, DW, 1, BAND>(p, w - 1, cur[1], tab);
        if (w >= 2 && w - 2 < K) rstage<K, DW, 2, BAND>(p, w - 2, cur[2], tab);
    }
}

// ------------------------------------------------------------------ standard layout
// bits_step_kernel with rstage: grid.x groups of 4 waves along the row, grid.y strips of output
// rows; a wave = one column group of 62*DW output words (+1 halo lane each side).
template <int K, int DW>
__global__ void __launch_bounds__(256) rule_bits_step_kernel(RuleArgs ra)
{
    const BitsArgs &a = ra.b;
    const int lane = threadIdx.x & 63;
    const int group = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (group >= a.ngroups) return;

    const int64_t col_raw = (int64_t)group * (62 * DW) + (int64_t)(lane - 1) * DW;
    const int64_t col = ((col_raw % a.Wd) + a.Wd) % a.Wd;
    const bool writer = lane >= 1 && lane <= 62 && col_raw < a.Wd;

    const int R = (int)a.R;
    const int s0 = (int)a.row0 + (int)blockIdx.y * a.strip;
    const int s1 = min(s0 + a.strip, (int)(a.row0 + a.rows));
    const int first_in = s0 - K;
    const int last_in = s1 + K - 1;
    const int nblk = ((s1 - s0) + 2 * K + 2) / 3;

    const uint32_t *top_adj = a.top + K * a.pitch;
    const uint32_t *bot_adj = a.bot - a.R * a.pitch;
    const uint32_t lane_off = (uint32_t)col * 4u;
    auto row_ptr = [&](int y) -> const uint32_t * {
        y = y > last_in ? last_in : y;  // steps past the end re-read the last row; never stored
        const uint32_t *base = y < 0 ? top_adj : (y >= R ? bot_adj : a.mid);
        const char *rb = reinterpret_cast<const char *>(base + (int64_t)y * a.pitch);
        return reinterpret_cast<const uint32_t *>(rb + lane_off);
    };

    gol_rule_tab tab;
    gol_rule_expand(ra.birth, ra.survive, tab);
    Pipe<K, DW> p;
    pipe_init(p);

    uint32_t buf[3][DW];
#pragma unroll
    for (int s = 0; s < 3; ++s) load_words<DW>(row_ptr(first_in + s), buf[s]);

    uint32_t alive = 0;
    for (int blk = 0; blk < nblk; ++blk) {
        const int t0 = blk * 3;
        uint32_t nxt[3][DW];
#pragma unroll
        for (int s = 0; s < 3; ++s) load_words<DW>(row_ptr(first_in + t0 + 3 + s), nxt[s]);
        uint32_t cur[3][DW];
#pragma unroll
        for (int s = 0; s < 3; ++s)
#pragma unroll
            for (int j = 0; j < DW; ++j) cur[s][j] = buf[s][j];
        rblock<K, DW, false>(p, cur, tab);
#pragma unroll
        for (int S = 0; S < 3; ++S) {
            uint32_t (&out)[DW] = cur[S];
            const int t = t0 + S;
            const int y = s0 + t - 2 * K;  // row emitted by the last stage
            if (t >= 2 * K && y < s1) {
                const uint32_t nx0 = from_upper_lane(out[0]);  // undo the K-bit frame shift
#pragma unroll
                for (int j = 0; j < DW; ++j) out[j] = __builtin_amdgcn_alignbit(j == DW - 1 ? nx0 : out[j + 1], out[j], K);
                if (writer) {
                    char *rb = reinterpret_cast<char *>(a.dst + (int64_t)y * a.pitch);
                    store_words<DW>(reinterpret_cast<uint32_t *>(rb + lane_off), out);
                    if (a.slots) {
#pragma unroll
                        for (int j = 0; j < DW; ++j) alive += __popc(out[j]);
                    }
                }
            }
        }
#pragma unroll
        for (int s = 0; s < 3; ++s)
#pragma unroll
            for (int j = 0; j < DW; ++j) buf[s][j] = nxt[s][j];
    }
    if (a.slots) slot_add(a.slots, alive);
}

// ------------------------------------------------------------------ band layout
// band_step_kernel (its general row addressing: a segment displacement per row) with rstage.
template <int K, int DW>
__global__ void __launch_bounds__(256) rule_band_step_kernel(RuleArgs ra)
{
    const BitsArgs &a = ra.b;
    constexpr int HL = band_halo_lanes(K, DW);
    constexpr int U = band_useful_words(K, DW);
    const int lane = threadIdx.x & 63;
    const int group = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (group >= a.ngroups) return;

    const int64_t col_raw = (int64_t)group * U + (int64_t)(lane - HL) * DW;
    const int64_t q = col_raw >= 0 ? col_raw / a.Wd : -((-col_raw + a.Wd - 1) / a.Wd);  // floor
    const int64_t col = col_raw - q * a.Wd;
    const uint32_t rot = (uint32_t)q & 31u;
    const bool wrap = __ballot(rot != 0) != 0;  // wave-uniform: any lane outside [0, Wd)
    const bool writer = lane >= HL && lane < 64 - HL && col_raw < a.Wd;

    const int R = (int)a.R;
    const int s0 = (int)a.row0 + (int)blockIdx.y * a.strip;
    const int s1 = min(s0 + a.strip, (int)(a.row0 + a.rows));
    const int first_in = s0 - K;
    const int last_in = s1 + K - 1;
    constexpr int NB = 2;  // blocks per loop trip: a ring of row blocks, one loaded ahead
    const int nblk = ((s1 - s0) + 2 * K + 2) / 3;
    const int nblk_r = (nblk + NB - 1) / NB * NB;  // trailing blocks re-read the last row, store nothing

    const int pitch_b = (int)a.pitch * 4;
    const char *mid_b = reinterpret_cast<const char *>(a.mid);
    const int64_t top_d = (reinterpret_cast<const char *>(a.top) - mid_b) + (int64_t)K * pitch_b;
    const int64_t bot_d = (reinterpret_cast<const char *>(a.bot) - mid_b) - (int64_t)R * pitch_b;
    const uint32_t lane_off = (uint32_t)col * 4u;
    // buffer stores with the row as the range: unwritten rows and halo lanes are dropped by the
    // range check (band_step_kernel)
    char *dst_b = reinterpret_cast<char *>(a.dst);
    const uint32_t row_bytes = (uint32_t)a.Wd * 4u;
    const uint32_t st_off = writer ? lane_off : 0x80000000u;
    const uint32_t st_mask = writer ? 0xFFFFFFFFu : 0u;
    auto load_row = [&](int y, uint32_t (&w)[DW]) {
        y = y > last_in ? last_in : y;
        const int64_t d = y < 0 ? top_d : (y >= R ? bot_d : 0);
        const char *rb = mid_b + (d + (int64_t)y * pitch_b);
        load_words<DW>(reinterpret_cast<const uint32_t *>(rb + lane_off), w);
    };
    auto unwrap = [&](uint32_t (&w)[DW]) {
        if (wrap) {
#pragma unroll
            for (int j = 0; j < DW; ++j) w[j] = __builtin_amdgcn_alignbit(w[j], w[j], rot);
        }
    };

    gol_rule_tab tab;
    gol_rule_expand(ra.birth, ra.survive, tab);
    Pipe<K, DW> p;
    pipe_init(p);

    uint32_t ring[NB][3][DW];
#pragma unroll
    for (int s = 0; s < 3; ++s) load_row(first_in + s, ring[0][s]);

    uint32_t alive = 0;
    for (int blk0 = 0; blk0 < nblk_r; blk0 += NB) {
#pragma unroll
        for (int u = 0; u < NB; ++u) {
            const int t0 = (blk0 + u) * 3;
#pragma unroll
            for (int s = 0; s < 3; ++s) load_row(first_in + t0 + 3 + s, ring[(u + 1) % NB][s]);
            uint32_t (&cur)[3][DW] = ring[u];
#pragma unroll
            for (int s = 0; s < 3; ++s) unwrap(cur[s]);
            rblock<K, DW, true>(p, cur, tab);
#pragma unroll
            for (int S = 0; S < 3; ++S) {
                const int t = t0 + S;
                const int y = s0 + t - 2 * K;
                const bool row_ok = t >= 2 * K && y < s1;  // wave-uniform
                store_row_masked<DW>(dst_b + (int64_t)(row_ok ? y : s0) * pitch_b, row_ok ? row_bytes : 0u, st_off,
                                     cur[S]);
                if (a.slots) {
                    uint32_t c = 0;
#pragma unroll
                    for (int j = 0; j < DW; ++j) c += __popc(cur[S][j]);
                    alive += c & (row_ok ? st_mask : 0u);
                }
            }
        }
    }
    if (a.slots) slot_add(a.slots, alive);
}

}  // namespace golk

// ------------------------------------------------------------------ launcher
using namespace golk;

template <int K>
static hipError_t launch_rule(bool band, dim3 grid, const RuleArgs &ra, hipStream_t s)
{
    constexpr int DW = GOLK_RULE_DW;
    if (band) hipLaunchKernelGGL((rule_band_step_kernel<K, DW>), grid, dim3(256), 0, s, ra);
    else hipLaunchKernelGGL((rule_bits_step_kernel<K, DW>), grid, dim3(256), 0, s, ra);
    return hipGetLastError();
}

int golk_rule_useful_words(bool band, int k) { return band ? band_useful_words(k, GOLK_RULE_DW) : 62 * GOLK_RULE_DW; }

hipError_t golk_rule_step(const uint32_t *top, const uint32_t *mid, const uint32_t *bot, uint32_t *dst, int64_t R,
                          int64_t Wd, int64_t pitch, int64_t row0, int64_t rows, int k, bool band, uint32_t birth,
                          uint32_t survive, int strip, uint64_t *slots, hipStream_t s)
{
    if (rows <= 0) return hipSuccess;
    if (birth >= 512 || survive >= 512 || Wd % GOLK_RULE_DW || pitch % GOLK_RULE_DW) return hipErrorInvalidValue;
    RuleArgs ra;
    BitsArgs &a = ra.b;
    a.top = top; a.mid = mid; a.bot = bot; a.dst = dst;
    a.R = R; a.Wd = Wd; a.pitch = pitch; a.row0 = row0; a.rows = rows;
    const int U = golk_rule_useful_words(band, k);
    a.ngroups = (int)((Wd + U - 1) / U);
    a.strip = strip > 0 ? std::min(strip, 1 << 24) : golk_auto_strip(rows, a.ngroups, k);  // (32-bit lane counts)
    a.slots = slots;
    a.sm = StripMap{};
    a.err = nullptr;  // no flag waits in these kernels
    a.cu_slots = nullptr;
    ra.birth = birth;
    ra.survive = survive;
    const dim3 grid((a.ngroups + 3) / 4, (unsigned)((rows + a.strip - 1) / a.strip));
    switch (k) {
    case 1: return launch_rule<1>(band, grid, ra, s);
    case 2: return launch_rule<2>(band, grid, ra, s);
    case 4: return launch_rule<4>(band, grid, ra, s);
    case 8: return launch_rule<8>(band, grid, ra, s);
    default: return hipErrorInvalidValue;
    }
}
