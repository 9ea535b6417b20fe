// gol_kernels.hip -- gfx950 (MI355X) kernels of the Game-of-Life hot path.
//
// Replaces the reference's per-cell Go loops:
//   worker.go:15-42 calculateNextState, worker.go:44-70 calculateSurroundings
//   broker.go:47-58 calculateAliveCells (count part)
// with two board representations:
//   * bit board  : 32 cells per uint32 (64 per uint64, LSB = lowest x).  A lane
//                  owns DW consecutive words of a row and slides down a strip
//                  of rows; K generations are pipelined in registers (temporal
//                  blocking), so a launch reads and writes the board once for K
//                  turns.  Stepped in the column-band layout (bit b of word w =
//                  cell b*Wd + w, shift-free generations) when W % 1024 == 0.
//   * byte board : one byte per cell (exact reference semantics incl. bytes
//                  that are neither 0 nor 255), SWAR on 4 cells per VGPR.
// One compiled path per kernel family; the variants measured and dropped in
// round 1 (vertical-first stages, barrier-synchronised split pipeline, centred
// standard-layout stages, per-role profiling builds) are recorded in DESIGN.md
// and live in git history (commit 297b13e).
//
// This unit: the step kernels (bits_step_kernel, band_step_kernel) with their rules, the layout
// conversion, the blocked and exact byte kernels, and their launchers: golk_step, the one launcher
// of every step kernel, takes a descriptor (gol_step_launch.h: the kernel table, the check, the
// geometry) and expands the table into its dispatch.  The two split pipelines are
// units of their own (gol_band_pipe.hip, gol_bytes_pipe.hip; launched through gol_step_device.h), the
// board utilities gol_util.hip; the launch state (error word, CU slots, claim counters, the strips
// of a pipelined launch) is host code, gol_launch.cpp.
// gol_device.h holds the lane helpers every kernel unit shares, gol_step_device.h the step kernels'
// machinery, gol_pipe.h what only the pipelines share.
#include <stdlib.h>

#include <type_traits>

#include "gol_launch.h"
#include "gol_rule.h"
#include "gol_step_device.h"
#include "gol_step_kernels.h"
#include "gol_step_launch.h"

namespace golk {

// Truth tables, lane helpers, rule(): gol_device.h.  Pipe, the band stage (hsum_band, bstage), BitsArgs,
// BytesKArgs, pack32 / unpack32: gol_step_device.h

// Standard layout, shifted frame: the horizontal 3-sum is formed from the cell and its two
// LEFT neighbours, S'[p] = c[p] + c[p-1] + c[p-2] = the 3-sum centred on p-1, so a stage
// needs one DPP (left word) instead of two and the centre cell is c << 1.  Every
// generation moves the frame one bit to the left; after K generations one funnel shift
// with the right neighbour word realigns the row.
template <int DW>
__device__ __forceinline__ void hsum_left(const uint32_t (&c)[DW], uint32_t (&h0)[DW], uint32_t (&h1)[DW],
                                          uint32_t (&ctr)[DW])
{
    const uint32_t left_in = from_lower_lane(c[DW - 1]);
#pragma unroll
    for (int j = 0; j < DW; ++j) {
        const uint32_t wl = (j == 0) ? left_in : c[j - 1];
        const uint32_t L1 = __builtin_amdgcn_alignbit(c[j], wl, 31);  // c[p-1] at bit p
        const uint32_t L2 = __builtin_amdgcn_alignbit(c[j], wl, 30);  // c[p-2] at bit p
        h0[j] = bitop3<TT_XOR3>(L1, c[j], L2);
        h1[j] = bitop3<TT_MAJ>(L1, c[j], L2);
        ctr[j] = L1;
    }
}

// One shifted-frame stage (generation g+1) of one row step S, in place on `cur`.
template <int K, int DW, int S>
__device__ __forceinline__ void sstage(Pipe<K, DW> &p, const int g, uint32_t (&cur)[DW])
{
    constexpr int SA = (S + 1) % 3, SM = (S + 2) % 3;
    hsum_left<DW>(cur, p.h0[g][S], p.h1[g][S], p.cc[g][S]);
#pragma unroll
    for (int j = 0; j < DW; ++j)
        cur[j] = rule(p.h0[g][SA][j], p.h1[g][SA][j], p.h0[g][SM][j], p.h1[g][SM][j], p.h0[g][S][j],
                      p.h1[g][S][j], p.cc[g][SM][j]);
}

// ------------------------------------------------------------------ the rule of a step kernel
// bits_step_kernel and band_step_kernel are generic over the rule (B3S23 and TableRule, below
// the band stages).  Rule::Args is the kernel's argument block: BitsArgs, plus the rule's data if
// it has any.  Rule::tab(args) is the rule's wave-uniform state, formed once per wave;
// Rule::stage<K, DW, S, BAND>(tab, p, g, cur) is one stage (generation g+1) of one row step S, in
// place on `cur`.
struct B3S23;

// The three rows of a block run through the K stages as a wavefront (row S is at stage w - S),
// so every instruction has two independent neighbours to issue beside it and the DPP
// read-after-write hazards are covered without s_nop.  (K, DW, Rule: template parameters where
// it is expanded.)
#define GOL_STAGE_BLOCK(BAND, tab, p, cur)                                                        \
    _Pragma("unroll") for (int w = 0; w < K + 2; ++w) {                                           \
        if (w < K) Rule::template stage<K, DW, 0, BAND>(tab, p, w, cur[0]);                       \
        if (w >= 1 && w - 1 < K) Rule::template stage<K, DW, 1, BAND>(tab, p, w - 1, cur[1]);     \
        if (w >= 2 && w - 2 < K) Rule::template stage<K, DW, 2, BAND>(tab, p, w - 2, cur[2]);     \
    }
// Where the wavefront is expanded is a matter of instruction scheduling only: as a function the
// compiler unrolls and simplifies it on its own before it inlines it, in the kernel's body
// together with the loads and stores around it, and the same operations come out in another
// order.  Each rule keeps the form it was measured with (Rule::BLOCK_INLINE): B3/S23 in the
// kernel's body (as a function e.g. bits_step_kernel<4, 2> has 1432 instructions instead of
// 1014), the table rule as a function (in the body its k = 8 standard kernel has the same 2329
// instructions in another order and ran 2.6 % slower).
template <class Rule, bool BAND, int K, int DW>
__device__ __forceinline__ void stage_block(const typename Rule::Tab &tab, Pipe<K, DW> &p, uint32_t (&cur)[3][DW])
{
    GOL_STAGE_BLOCK(BAND, tab, p, cur)
}

// ------------------------------------------------------------------ bit-board step, standard layout
// grid.x: groups of 4 waves along the row; grid.y: strips of output rows.
// Wave = one column group of 62*DW output words (+1 halo lane each side).
template <int K, int DW, class Rule = B3S23>
__global__ void __launch_bounds__(256) bits_step_kernel(typename Rule::Args a)
{
    const int lane = threadIdx.x & 63;
    const int group = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (group >= a.ngroups) return;  // whole wave exits; no barriers in this kernel

    // column (in words) of this lane's first word, torus-wrapped
    const int64_t col_raw = (int64_t)group * (62 * DW) + (int64_t)(lane - 1) * DW;
    const int64_t col = ((col_raw % a.Wd) + a.Wd) % a.Wd;
    const bool writer = lane >= 1 && lane <= 62 && col_raw < a.Wd;

    // Row indices are wave-uniform 32-bit values (rows < 2^31), kept in SGPRs.
    const int R = (int)a.R;
    const int s0 = (int)a.row0 + (int)blockIdx.y * a.strip;  // first output row
    const int s1 = min(s0 + a.strip, (int)(a.row0 + a.rows)); // end output row
    const int first_in = s0 - K;                              // first input row
    const int last_in = s1 + K - 1;                           // last input row
    const int nblk = ((s1 - s0) + 2 * K + 2) / 3;

    // Input row y lives at base(y) + y*pitch with base = top + k*pitch (y < 0), mid
    // (0 <= y < R) or bot - R*pitch (y >= R): a scalar row pointer plus a 32-bit per-lane
    // byte offset (global_load ... saddr form).
    const uint32_t *top_adj = a.top + K * a.pitch;
    const uint32_t *bot_adj = a.bot - a.R * a.pitch;
    const uint32_t lane_off = (uint32_t)col * 4u;  // bytes
    auto row_ptr = [&](int y) -> const uint32_t * {
        y = y > last_in ? last_in : y;  // steps past the end re-read the last row; never stored
        const uint32_t *base = y < 0 ? top_adj : (y >= R ? bot_adj : a.mid);
        const char *rb = reinterpret_cast<const char *>(base + (int64_t)y * a.pitch);
        return reinterpret_cast<const uint32_t *>(rb + lane_off);
    };

    const typename Rule::Tab tab = Rule::tab(a);
    Pipe<K, DW> p;
    pipe_init(p);

    uint32_t buf[3][DW];
#pragma unroll
    for (int s = 0; s < 3; ++s) load_words<DW>(row_ptr(first_in + s), buf[s]);

    uint32_t alive = 0;  // < 2^32: strips are capped at 2^24 rows x 128 cells per lane
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
        if constexpr (Rule::BLOCK_INLINE) { GOL_STAGE_BLOCK(false, tab, p, cur) }
        else stage_block<Rule, false>(tab, p, cur);
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

// Store DW words at byte offset voff of a buffer [row, row + nbytes): out-of-range offsets
// (and nbytes = 0) are dropped by the hardware range check.  aux 2 = nt (streaming) stores.
template <int DW>
__device__ __forceinline__ void store_row_masked(char *row, uint32_t nbytes, uint32_t voff, const uint32_t (&w)[DW])
{
    const __amdgpu_buffer_rsrc_t r = __builtin_amdgcn_make_buffer_rsrc(row, (short)0, (int)nbytes, 0x00020000);
    if constexpr (DW == 4) {
        typedef __attribute__((ext_vector_type(4))) uint32_t v4u;
        __builtin_amdgcn_raw_buffer_store_b128(v4u{w[0], w[1], w[2], w[3]}, r, voff, 0, 2);
    } else if constexpr (DW == 2) {
        typedef __attribute__((ext_vector_type(2))) uint32_t v2u;
        __builtin_amdgcn_raw_buffer_store_b64(v2u{w[0], w[1]}, r, voff, 0, 0);
    } else {
        static_assert(DW == 4 || DW == 2, "band lanes hold 2 or 4 words");
    }
}

// The same stage for a life-like rule as data (gol_rule.h): the full 4-bit count of the 3x3 block
// and a mux tree over the rule's two tables instead of the hard-wired B3/S23 tail.  Per word and
// generation: 2 ops of horizontal sums (band; the standard layout's shifted frame adds its 2
// v_alignbit), 7 for the count, 19 for the rule.
template <int K, int DW, int S, bool BAND>
__device__ __forceinline__ void rstage(const gol_rule_tab &tab, Pipe<K, DW> &p, const int g, uint32_t (&cur)[DW])
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

// The two rules of the step kernels (GOL_STAGE_BLOCK).  B3/S23 hard-wired: no data, so the kernel's
// argument block is BitsArgs itself.
struct B3S23 {
    typedef BitsArgs Args;
    static constexpr bool BLOCK_INLINE = true;
    struct Tab {};
    static __device__ __forceinline__ Tab tab(const Args &) { return {}; }
    template <int K, int DW, int S, bool BAND>
    static __device__ __forceinline__ void stage(const Tab &, Pipe<K, DW> &p, const int g, uint32_t (&cur)[DW])
    {
        if constexpr (BAND) bstage<K, DW, S>(p, g, cur);
        else sstage<K, DW, S>(p, g, cur);
    }
};
// Any life-like rule: the two 9-bit masks, expanded into the circuit's tables once per wave.
struct TableRule {
    struct Args : BitsArgs {
        uint32_t birth, survive;
    };
    typedef gol_rule_tab Tab;
    static constexpr bool BLOCK_INLINE = false;
    static __device__ __forceinline__ Tab tab(const Args &a)
    {
        Tab t;
        gol_rule_expand(a.birth, a.survive, t);
        return t;
    }
    template <int K, int DW, int S, bool BAND>
    static __device__ __forceinline__ void stage(const Tab &t, Pipe<K, DW> &p, const int g, uint32_t (&cur)[DW])
    {
        rstage<K, DW, S, BAND>(t, p, g, cur);
    }
};

// One wave = all K stages (k = 1, 2, 4, 8; 16 with 2 words per lane).  Same row addressing,
// strips and fused count as bits_step_kernel; grid.x: groups of 4 waves along the row,
// grid.y: strips of output rows.
// CONTIG: top == mid - K*pitch and bot == mid + R*pitch (halo rows stored right above and
// below the shard), so input row y is simply mid + y*pitch: no per-row segment select.
template <int K, int DW, bool CONTIG, class Rule = B3S23>
__global__ void __launch_bounds__(256) band_step_kernel(typename Rule::Args a)
{
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
    constexpr int NB = 2;  // blocks per loop trip: the ring below (one block loaded ahead)
    const int nblk = ((s1 - s0) + 2 * K + 2) / 3;
    const int nblk_r = (nblk + NB - 1) / NB * NB;  // trailing blocks re-read the last row, store nothing

    // Every row address is a.mid + (segment displacement + y * pitch): one pointer (the
    // compiler keeps it in the global address space, so the loads are global_load with exact
    // vmcnt waits) plus an integer select.  A select between pointer locals can become an
    // indexed private array (scratch loads in the loop); an integer-to-pointer cast becomes a
    // flat load (vmcnt(0) + lgkmcnt waits).
    const int pitch_b = (int)a.pitch * 4;
    const char *mid_b = reinterpret_cast<const char *>(a.mid);
    const int64_t top_d = (reinterpret_cast<const char *>(a.top) - mid_b) + (int64_t)K * pitch_b;
    const int64_t bot_d = (reinterpret_cast<const char *>(a.bot) - mid_b) - (int64_t)R * pitch_b;
    const uint32_t lane_off = (uint32_t)col * 4u;
    // Stores: buffer stores with the row as the buffer range, so rows that must not be
    // written (pipeline fill, past the strip) and halo lanes are dropped by the range check
    // instead of a branch (stores under a branch make the compiler's vmcnt waits for the NEXT
    // block's rows also wait for these stores).
    char *dst_b = reinterpret_cast<char *>(a.dst);
    const uint32_t row_bytes = (uint32_t)a.Wd * 4u;
    const uint32_t st_off = writer ? lane_off : 0x80000000u;
    const uint32_t st_mask = writer ? 0xFFFFFFFFu : 0u;
    auto load_row = [&](int y, uint32_t (&w)[DW]) {
        y = y > last_in ? last_in : y;
        const int64_t d = CONTIG ? 0 : (y < 0 ? top_d : (y >= R ? bot_d : 0));
        const char *rb = mid_b + (d + (int64_t)y * pitch_b);
        load_words<DW>(reinterpret_cast<const uint32_t *>(rb + lane_off), w);
    };
    auto unwrap = [&](uint32_t (&w)[DW]) {
        if (wrap) {
#pragma unroll
            for (int j = 0; j < DW; ++j) w[j] = __builtin_amdgcn_alignbit(w[j], w[j], rot);
        }
    };

    const typename Rule::Tab tab = Rule::tab(a);
    Pipe<K, DW> p;
    pipe_init(p);

    // Row blocks in flight: a ring of NB three-row buffers; block b lives in ring[b % NB] and
    // is loaded one block ahead of use.  The block loop is unrolled by NB so the ring index is
    // static: no register copies, and the loads are waited for just before their first use (a
    // copy at the loop end would also wait for that block's stores: gfx9 has one in-order
    // vmcnt for loads and stores).
    uint32_t ring[NB][3][DW];
#pragma unroll
    for (int s = 0; s < 3; ++s) load_row(first_in + s, ring[0][s]);
    // Three empty-range stores (dropped) so that the loop is entered with the same memory-
    // counter history as its back edge (loads, then a block's 3 stores): the compiler then
    // waits for the block's rows with vmcnt(6), not vmcnt(3).
#pragma unroll
    for (int s = 0; s < 3; ++s) store_row_masked<DW>(dst_b, 0u, st_off, ring[0][s]);

    uint32_t alive = 0;  // < 2^32: strips are capped at 2^24 rows x 128 cells per lane
    for (int blk0 = 0; blk0 < nblk_r; blk0 += NB) {
#pragma unroll
        for (int u = 0; u < NB; ++u) {
            const int t0 = (blk0 + u) * 3;
#pragma unroll
            for (int s = 0; s < 3; ++s) load_row(first_in + t0 + 3 + s, ring[(u + 1) % NB][s]);
            uint32_t (&cur)[3][DW] = ring[u];
#pragma unroll
            for (int s = 0; s < 3; ++s) unwrap(cur[s]);
            if constexpr (Rule::BLOCK_INLINE) { GOL_STAGE_BLOCK(true, tab, p, cur) }
            else stage_block<Rule, true>(tab, p, cur);
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
#undef GOL_STAGE_BLOCK

// 32 x 32 bit-matrix transpose in registers: afterwards x[i] bit b = (before) x[b] bit i.
__device__ __forceinline__ void transpose32(uint32_t (&x)[32])
{
    uint32_t m = 0x0000FFFFu;
#pragma unroll
    for (int j = 16; j != 0; j >>= 1) {
#pragma unroll
        for (int k = 0; k < 32; ++k) {
            if (k & j) continue;
            const uint32_t t = ((x[k] >> j) ^ x[k + j]) & m;
            x[k + j] ^= t;
            x[k] ^= t << j;
        }
        m ^= m << (j >> 1);
    }
}

// Standard bit rows (word s bit i = cell 32s + i) -> band rows, or back.  One lane per
// (row, m): the 32 standard words m, m + Wm, ..., m + 31*Wm (Wm = Wd/32) hold exactly the
// cells of band words 32m .. 32m+31, so the conversion is one 32x32 transpose.
template <bool TO_BAND>
__global__ void band_convert_kernel(const uint32_t *src, uint32_t *dst, int64_t rows, int64_t Wm, int64_t spitch,
                                    int64_t dpitch)
{
    const int64_t n = rows * Wm;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t y = i / Wm, m = i % Wm;
        uint32_t x[32];
        if (TO_BAND) {
            const uint32_t *s = src + y * spitch + m;
#pragma unroll
            for (int b = 0; b < 32; ++b) x[b] = s[b * Wm];
        } else {
            const uint4 *s = reinterpret_cast<const uint4 *>(src + y * spitch + 32 * m);
#pragma unroll
            for (int v = 0; v < 8; ++v) {
                const uint4 q = s[v];
                x[4 * v] = q.x; x[4 * v + 1] = q.y; x[4 * v + 2] = q.z; x[4 * v + 3] = q.w;
            }
        }
        transpose32(x);
        if (TO_BAND) {
            uint4 *d = reinterpret_cast<uint4 *>(dst + y * dpitch + 32 * m);
#pragma unroll
            for (int v = 0; v < 8; ++v) d[v] = make_uint4(x[4 * v], x[4 * v + 1], x[4 * v + 2], x[4 * v + 3]);
        } else {
            uint32_t *d = dst + y * dpitch + m;
#pragma unroll
            for (int b = 0; b < 32; ++b) d[b * Wm] = x[b];
        }
    }
}

// ------------------------------------------------------------------ byte-board step, k turns per launch
// For boards whose bytes are all 0 or 255 (every board after its first turn): each lane
// packs 32 bytes of a row into one 32-cell word (bit i = byte i & 1), runs the same K-stage
// shifted-frame register pipeline as the standard bit board and unpacks the result to 0/255
// bytes.  HBM traffic: 2 bytes per cell per K turns.
// One wave = all K stages (k = 1..16), 62 column words per wave.
template <int K>
__global__ void __launch_bounds__(256) bytes_blocked_kernel(BytesKArgs a)
{
    const int lane = threadIdx.x & 63;
    const int group = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (group >= a.ngroups) return;
    const int64_t col_raw = (int64_t)group * 62 + (lane - 1);
    const int64_t col = ((col_raw % a.Wd) + a.Wd) % a.Wd;
    const bool writer = lane >= 1 && lane <= 62 && col_raw < a.Wd;
    const int R = (int)a.R;
    const int s0 = (int)a.row0 + (int)blockIdx.y * a.strip;
    const int s1 = min(s0 + a.strip, (int)(a.row0 + a.rows));
    const int first_in = s0 - K, last_in = s1 + K - 1;
    constexpr int NB = 2;  // blocks per loop trip: one block loaded ahead
    const int nblk = ((s1 - s0) + 2 * K + 2) / 3;
    const int nblk_r = (nblk + NB - 1) / NB * NB;  // trailing blocks store nothing
    // row addresses: a.mid + (segment displacement + y * pitch) (see band_step_kernel)
    const int pitch = (int)a.pitch;
    const char *mid_b = reinterpret_cast<const char *>(a.mid);
    const int64_t top_d = (reinterpret_cast<const char *>(a.top) - mid_b) + (int64_t)K * pitch;
    const int64_t bot_d = (reinterpret_cast<const char *>(a.bot) - mid_b) - (int64_t)R * pitch;
    const uint32_t lane_off = (uint32_t)(col * 32);
    auto load = [&](int y, Raw32 &r) {
        y = y > last_in ? last_in : y;
        const int64_t d = y < 0 ? top_d : (y >= R ? bot_d : 0);
        const uint4 *q = reinterpret_cast<const uint4 *>(mid_b + (d + (int64_t)y * pitch) + lane_off);
        r.lo = q[0];
        r.hi = q[1];
    };
    // range-checked stores (dropped for halo lanes and rows outside the strip)
    char *dst_b = reinterpret_cast<char *>(a.dst);
    const uint32_t row_bytes = (uint32_t)a.Wd * 32u;
    const uint32_t st_off = writer ? lane_off : 0x80000000u;
    const uint32_t st_mask = writer ? 0xFFFFFFFFu : 0u;
    auto store = [&](char *row, uint32_t nbytes, const uint32_t w) {
        uint4 lo, hi;
        unpack32(w, lo, hi);
        const __amdgpu_buffer_rsrc_t r = __builtin_amdgcn_make_buffer_rsrc(row, (short)0, (int)nbytes, 0x00020000);
        typedef __attribute__((ext_vector_type(4))) uint32_t v4u;
        __builtin_amdgcn_raw_buffer_store_b128(v4u{lo.x, lo.y, lo.z, lo.w}, r, st_off, 0, 0);
        __builtin_amdgcn_raw_buffer_store_b128(v4u{hi.x, hi.y, hi.z, hi.w}, r, st_off + 16u, 0, 0);
    };
    Pipe<K, 1> p;
    pipe_init(p);
    Raw32 ring[NB][3];
#pragma unroll
    for (int s = 0; s < 3; ++s) load(first_in + s, ring[0][s]);
    // same memory-counter history on loop entry as on the back edge (3 rows x 2 stores)
#pragma unroll
    for (int s = 0; s < 3; ++s) store(dst_b, 0u, 0u);
    uint32_t alive = 0;  // strips are capped at 2^24 rows x 32 cells per lane
    for (int blk0 = 0; blk0 < nblk_r; blk0 += NB) {
#pragma unroll
        for (int u = 0; u < NB; ++u) {
            const int t0 = (blk0 + u) * 3;
#pragma unroll
            for (int s = 0; s < 3; ++s) load(first_in + t0 + 3 + s, ring[(u + 1) % NB][s]);
            uint32_t cur[3][1];
#pragma unroll
            for (int s = 0; s < 3; ++s) cur[s][0] = pack32(ring[u][s].lo, ring[u][s].hi);
#pragma unroll
            for (int w = 0; w < K + 2; ++w) {
                if (w < K) sstage<K, 1, 0>(p, w, cur[0]);
                if (w >= 1 && w - 1 < K) sstage<K, 1, 1>(p, w - 1, cur[1]);
                if (w >= 2 && w - 2 < K) sstage<K, 1, 2>(p, w - 2, cur[2]);
            }
#pragma unroll
            for (int S = 0; S < 3; ++S) {
                const int t = t0 + S;
                const int y = s0 + t - 2 * K;
                const bool row_ok = t >= 2 * K && y < s1;  // wave-uniform
                const uint32_t o = __builtin_amdgcn_alignbit(from_upper_lane(cur[S][0]), cur[S][0], K);
                store(dst_b + (int64_t)(row_ok ? y : s0) * pitch, row_ok ? row_bytes : 0u, o);
                if (a.slots) alive += (uint32_t)__popc(o) & (row_ok ? st_mask : 0u);
            }
        }
    }
    if (a.slots) slot_add(a.slots, alive);
}

// ------------------------------------------------------------------ byte-board step (exact semantics)
// SWAR on 4 cells per uint32.  A = (byte == 255), Z = (byte == 0), as 0x01 per byte.
__device__ __forceinline__ uint32_t bytes_eq_ff(uint32_t d)
{
    const uint32_t x = ~d;
    const uint32_t nz = ((x & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | x;  // bit7 set where x byte != 0
    return (~nz >> 7) & 0x01010101u;
}
__device__ __forceinline__ uint32_t bytes_eq_00(uint32_t d)
{
    const uint32_t nz = ((d & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | d;
    return (~nz >> 7) & 0x01010101u;
}

struct ByteRow {
    uint32_t a[4];  // (byte == 255) flags
    uint32_t z[4];  // (byte == 0) flags
    uint32_t hs[4]; // horizontal 3-sums of the a flags (0..3 per byte)
};

__device__ __forceinline__ void byte_row(const uint4 v, ByteRow &r)
{
    const uint32_t d[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int j = 0; j < 4; ++j) { r.a[j] = bytes_eq_ff(d[j]); r.z[j] = bytes_eq_00(d[j]); }
    const uint32_t left_in = from_lower_lane(r.a[3]);
    const uint32_t right_in = from_upper_lane(r.a[0]);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const uint32_t wl = j == 0 ? left_in : r.a[j - 1];
        const uint32_t wr = j == 3 ? right_in : r.a[j + 1];
        const uint32_t L = __builtin_amdgcn_alignbyte(r.a[j], wl, 3);  // byte x-1 at byte x
        const uint32_t R = __builtin_amdgcn_alignbyte(wr, r.a[j], 1);  // byte x+1 at byte x
        r.hs[j] = L + r.a[j] + R;
    }
}

__device__ __forceinline__ uint32_t byte_rule(uint32_t hs_up, uint32_t hs_mid, uint32_t hs_dn, uint32_t a,
                                              uint32_t z)
{
    const uint32_t n = hs_up + hs_mid + hs_dn - a;                                   // neighbours, 0..8
    const uint32_t ne3 = ((n ^ 0x03030303u) + 0x7F7F7F7Fu) & 0x80808080u;           // n != 3
    const uint32_t ne23 = (((n | 0x01010101u) ^ 0x03030303u) + 0x7F7F7F7Fu) & 0x80808080u;  // n not in {2,3}
    const uint32_t born = z & ~(ne3 >> 7);
    const uint32_t surv = a & ~(ne23 >> 7);
    const uint32_t r = born | surv;  // 0x01 per byte
    return (r << 8) - r;             // 0xFF per byte
}

struct BytesArgs {
    const uint8_t *world;
    uint8_t *out;
    int64_t H, W, stride, out_stride, y0, y1;
    int32_t strip, ngroups;
};

// Wave = 62 lanes x 16 bytes of output per row; lanes 0/63 are halo.
__global__ void __launch_bounds__(256) bytes_step_kernel(BytesArgs a)
{
    const int lane = threadIdx.x & 63;
    const int group = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (group >= a.ngroups) return;
    const int64_t col_raw = (int64_t)group * (62 * 16) + (int64_t)(lane - 1) * 16;
    const int64_t col = ((col_raw % a.W) + a.W) % a.W;
    const bool writer = lane >= 1 && lane <= 62 && col_raw < a.W;

    const int64_t s0 = a.y0 + (int64_t)blockIdx.y * a.strip;
    const int64_t s1 = min(s0 + (int64_t)a.strip, a.y1);
    auto load = [&](int64_t y) -> uint4 {
        y = ((y % a.H) + a.H) % a.H;
        return *reinterpret_cast<const uint4 *>(a.world + y * a.stride + col);
    };
    ByteRow up, mid, dn;
    byte_row(load(s0 - 1), up);
    byte_row(load(s0), mid);
    uint4 nxt = load(s0 + 1);
    for (int64_t y = s0; y < s1; ++y) {
        byte_row(nxt, dn);
        nxt = load(y + 2);  // prefetch (wraps harmlessly past the strip)
        if (writer) {
            uint4 o;
            o.x = byte_rule(up.hs[0], mid.hs[0], dn.hs[0], mid.a[0], mid.z[0]);
            o.y = byte_rule(up.hs[1], mid.hs[1], dn.hs[1], mid.a[1], mid.z[1]);
            o.z = byte_rule(up.hs[2], mid.hs[2], dn.hs[2], mid.a[2], mid.z[2]);
            o.w = byte_rule(up.hs[3], mid.hs[3], dn.hs[3], mid.a[3], mid.z[3]);
            *reinterpret_cast<uint4 *>(a.out + (y - a.y0) * a.out_stride + col) = o;
        }
        up = mid;
        mid = dn;
    }
}

// Widths that are not a multiple of 16 (one thread per cell), a literal restatement of
// worker.go:26-37 / 44-70.
__global__ void bytes_step_scalar_kernel(BytesArgs a)
{
    const int64_t n = (a.y1 - a.y0) * a.W;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t y = a.y0 + i / a.W, x = i % a.W;
        const int64_t ya = (y + a.H - 1) % a.H, yb = (y + 1) % a.H;
        const int64_t xl = (x + a.W - 1) % a.W, xr = (x + 1) % a.W;
        const uint8_t *w = a.world;
        const int64_t s = a.stride;
        int cnt = (w[ya * s + xl] == 255) + (w[ya * s + x] == 255) + (w[ya * s + xr] == 255) +
                  (w[y * s + xl] == 255) + (w[y * s + xr] == 255) + (w[yb * s + xl] == 255) +
                  (w[yb * s + x] == 255) + (w[yb * s + xr] == 255);
        const uint8_t c = w[y * s + x];
        uint8_t o = 0;
        if (c == 0 && cnt == 3) o = 255;
        if (c == 255 && (cnt == 2 || cnt == 3)) o = 255;
        a.out[(y - a.y0) * a.out_stride + x] = o;
    }
}

}  // namespace golk

// ------------------------------------------------------------------ launchers
using namespace golk;

// The kernel arguments of a step launch, filled in one place: column groups and strips from the
// launch's geometry (a pipeline's strips come from its plan afterwards), no strip map; the error
// word and the CU slot masks for the families that have a pipeline (the one-wave kernels wait for
// no flag and read neither).  A: TableRule::Args (BitsArgs and the masks) or BytesKArgs.
template <class A>
static hipError_t fill_args(A &a, const gol_step_launch &l, const gol_step_geometry &g)
{
    a.top = static_cast<decltype(a.top)>(l.top); a.mid = static_cast<decltype(a.mid)>(l.mid);
    a.bot = static_cast<decltype(a.bot)>(l.bot); a.dst = static_cast<decltype(a.dst)>(l.dst);
    a.R = l.R; a.Wd = g.words; a.pitch = l.pitch; a.row0 = l.row0; a.rows = l.rows;
    a.ngroups = g.ngroups;
    a.strip = g.strip;
    a.slots = l.slots;
    a.sm = StripMap{};
    a.err = nullptr;
    if (l.family == GOL_FAMILY_BAND || l.family == GOL_FAMILY_BYTES) {
        a.err = err_or_default(l.err);
        if (!a.err) return hipErrorOutOfMemory;
    }
    if constexpr (std::is_same<A, TableRule::Args>::value) {
        a.birth = l.birth; a.survive = l.survive;
        a.cu_slots = nullptr;
        int dev = 0;
        if (GOL_BAND_PLACE && l.family == GOL_FAMILY_BAND && hipGetDevice(&dev) == hipSuccess) a.cu_slots = golk_cu_slots(dev);
    }
    return hipSuccess;
}

// One entry of the kernel table (gol_step_launch.h) on `grid`; a pipelined entry is not launched here.
template <int F, int K, int DW, bool PIPE>
static void launch_kernel(dim3 grid, bool contig, const TableRule::Args &a, const BytesKArgs &b, hipStream_t s)
{
    const BitsArgs &c = a;  // (the B3/S23 kernels take the arguments without the masks)
    if constexpr (PIPE) return;
    else if constexpr (F == GOL_FAMILY_BITS) hipLaunchKernelGGL((bits_step_kernel<K, DW>), grid, dim3(256), 0, s, c);
    else if constexpr (F == GOL_FAMILY_BAND) {
        if (contig) hipLaunchKernelGGL((band_step_kernel<K, DW, true>), grid, dim3(256), 0, s, c);
        else hipLaunchKernelGGL((band_step_kernel<K, DW, false>), grid, dim3(256), 0, s, c);
    } else if constexpr (F == GOL_FAMILY_RULE_STD) hipLaunchKernelGGL((bits_step_kernel<K, DW, TableRule>), grid, dim3(256), 0, s, a);
    else if constexpr (F == GOL_FAMILY_RULE_BAND) hipLaunchKernelGGL((band_step_kernel<K, DW, false, TableRule>), grid, dim3(256), 0, s, a);
    else hipLaunchKernelGGL(bytes_blocked_kernel<K>, grid, dim3(256), 0, s, b);
}

hipError_t golk_step(const gol_step_launch &l, hipStream_t s)
{
    if (!gol_step_launch_ok(l)) return hipErrorInvalidValue;
    if (l.rows == 0) return hipSuccess;
    const gol_step_geometry g = gol_step_geometry_of(l);
    const bool bytes = l.family == GOL_FAMILY_BYTES, count = l.slots != nullptr;
    TableRule::Args a;
    BytesKArgs b;
    const hipError_t e = bytes ? fill_args(b, l, g) : fill_args(a, l, g);
    if (e != hipSuccess) return e;
    if (g.pipelined) {
        // one workgroup of the pipeline's waves per (column group, range of rows): band_strip_plan
        // (k = 12: 4 waves x 3 stages), bytes_strip_plan (k = 32: 8 waves x 4)
        unsigned nwg = 0;
        if (bytes) {
            if (!pipe_plan(bytes_strip_plan, golk_bytes_pipe_fn(count), 64 * GOL_BYTES_PIPE_P, l.rows, l.width, l.pitch, l.k,
                           l.strip_rows, l.as_cus, l.as_slots, s, b.strip, b.sm, nwg))
                return hipErrorInvalidValue;
            return golk_bytes_pipe_launch(count, nwg, b, s);
        }
        if (!pipe_plan(band_strip_plan, golk_band_pipe_fn(g.contig, count), 64 * GOL_BAND_P, l.rows, l.width, l.pitch, l.k,
                       l.strip_rows, l.as_cus, l.as_slots, s, a.strip, a.sm, nwg))
            return hipErrorInvalidValue;
        return golk_band_pipe_launch(g.contig, count, nwg, a, s);
    }
    const dim3 grid((g.ngroups + 3) / 4, (unsigned)((l.rows + g.strip - 1) / g.strip));
    switch (gol_step_key(l.family, l.k, l.dw)) {
#define GOL_STEP_CASE(F, K, DW, FLAGS) \
    case gol_step_key(GOL_FAMILY_##F, K, DW): launch_kernel<GOL_FAMILY_##F, K, DW, ((FLAGS) & GOL_STEP_PIPELINED) != 0>(grid, g.contig, a, b, s); break;
    GOL_STEP_KERNELS(GOL_STEP_CASE)
#undef GOL_STEP_CASE
    }
    return hipGetLastError();
}

hipError_t golk_band_convert(bool to_band, const uint32_t *src, uint32_t *dst, int64_t rows, int64_t Wd,
                             int64_t spitch, int64_t dpitch, hipStream_t s)
{
    const int64_t Wm = Wd / 32;
    if (rows <= 0) return hipSuccess;
    const dim3 g(grid_for(rows * Wm, 256, 256 * 64));
    if (to_band)
        hipLaunchKernelGGL(band_convert_kernel<true>, g, dim3(256), 0, s, src, dst, rows, Wm, spitch, dpitch);
    else
        hipLaunchKernelGGL(band_convert_kernel<false>, g, dim3(256), 0, s, src, dst, rows, Wm, spitch, dpitch);
    return hipGetLastError();
}

hipError_t golk_bytes_step(const uint8_t *world, int64_t H, int64_t W, int64_t stride, int64_t y0, int64_t y1,
                           uint8_t *out, int64_t out_stride, hipStream_t s)
{
    BytesArgs a;
    a.world = world; a.out = out; a.H = H; a.W = W; a.stride = stride; a.out_stride = out_stride;
    a.y0 = y0; a.y1 = y1;
    if (y1 <= y0) return hipSuccess;
    const bool vec = (W % 16 == 0) && (stride % 16 == 0) && (out_stride % 16 == 0) &&
                     (((uintptr_t)world & 15) == 0) && (((uintptr_t)out & 15) == 0);
    if (vec) {
        a.ngroups = (int)((W + 62 * 16 - 1) / (62 * 16));
        const int64_t rows = y1 - y0;
        int64_t strip = rows * a.ngroups / 8192;
        if (strip < 16) strip = 16;
        if (strip > 256) strip = 256;
        if (strip > rows) strip = rows;
        a.strip = (int)strip;
        dim3 grid((a.ngroups + 3) / 4, (int)((rows + strip - 1) / strip));
        hipLaunchKernelGGL(bytes_step_kernel, grid, dim3(256), 0, s, a);
    } else {
        a.ngroups = 0; a.strip = 0;
        hipLaunchKernelGGL(bytes_step_scalar_kernel, dim3(grid_for((y1 - y0) * W)), dim3(256), 0, s, a);
    }
    return hipGetLastError();
}
