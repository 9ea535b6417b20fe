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
// conversion, the blocked and exact byte kernels, the board utilities, the list kernels, the IPC
// flag kernels, and every launcher with its host state.  The two split pipelines are units of
// their own (gol_band_pipe.hip, gol_bytes_pipe.hip; entry points declared in gol_device.h).
// gol_device.h holds what the units share, gol_pipe.h what only the pipelines share.
#include <stdlib.h>

#include <algorithm>
#include <map>
#include <mutex>
#include <set>
#include <utility>

#include "gol_device.h"
#include "gol_rule.h"

namespace golk {

// Truth tables, lane helpers, rule(), Pipe, the band stage (hsum_band, bstage), BitsArgs,
// BytesKArgs, pack32 / unpack32: gol_device.h

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

// ------------------------------------------------------------------ board utilities
// Synthetic board: 64-bit word (y, w) = splitmix64(seed ^ (y*Ww + w)).
__global__ void random_fill_kernel(uint32_t *dst, int64_t rows, int64_t grow0, int64_t Ww, int64_t pitch,
                                   uint64_t seed)
{
    const int64_t n = rows * Ww;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t y = i / Ww, w = i % Ww;
        const uint64_t v = splitmix64(seed ^ (uint64_t)((grow0 + y) * Ww + w));
        *reinterpret_cast<uint2 *>(dst + y * pitch + 2 * w) = make_uint2((uint32_t)v, (uint32_t)(v >> 32));
    }
}

__global__ void popcount_kernel(const uint32_t *src, int64_t rows, int64_t Wd, int64_t pitch, uint64_t *slots)
{
    uint64_t c = 0;
    const int64_t n = rows * Wd;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t y = i / Wd, w = i % Wd;
        c += __popc(src[y * pitch + w]);
    }
    slot_add(slots, c);
}

// Sum the GOL_COUNT_SLOTS slots of `n` consecutive slot arrays into out[0..n) (one wave each).
__global__ void slots_reduce_kernel(uint64_t *slots, int64_t n, uint64_t *out)
{
    const int lane = threadIdx.x & 63;
    const int64_t i = blockIdx.x * (int64_t)(blockDim.x >> 6) + (threadIdx.x >> 6);
    if (i >= n) return;
    uint64_t s = 0;
    for (int j = lane; j < GOL_COUNT_SLOTS; j += 64) {
        uint64_t *p = &slots[(i * GOL_COUNT_SLOTS + j) * 8];
        s += *p;
        *p = 0;  // left zeroed: the next counted launch needs no memset (gol_engine.cpp slots_zero)
    }
    s = wave_sum_u64(s);
    if (lane == 0) out[i] = s;
}

__global__ void hash_kernel(const uint32_t *src, int64_t rows, int64_t grow0, int64_t Ww, int64_t pitch,
                            uint64_t *slots)
{
    uint64_t h = 0;
    const int64_t n = rows * Ww;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t y = i / Ww, w = i % Ww;
        const uint2 v = *reinterpret_cast<const uint2 *>(src + y * pitch + 2 * w);
        const uint64_t word = (uint64_t)v.x | ((uint64_t)v.y << 32);
        h += splitmix64(word ^ splitmix64((uint64_t)((grow0 + y) * Ww + w)));
    }
    slot_add(slots, h);
}

__global__ void count_nonzero_bytes_kernel(const uint8_t *src, int64_t rows, int64_t W, int64_t stride,
                                           uint64_t *slots)
{
    uint64_t c = 0;
    const int64_t n = rows * W;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t y = i / W, x = i % W;
        c += src[y * stride + x] != 0;
    }
    slot_add(slots, c);
}

// flag |= 1 if any byte of the rows x W board is neither 0 nor 255
__global__ void nonbinary_kernel(const uint8_t *bytes, int64_t rows, int64_t W, int64_t stride, uint32_t *flag)
{
    const int64_t n = rows * W;
    uint32_t bad = 0;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const uint8_t c = bytes[(i / W) * stride + i % W];
        bad |= (c != 0 && c != 255);
    }
    if (__ballot(bad) && (threadIdx.x & 63) == 0) atomicOr(flag, 1u);
}

// bytes -> bits: one thread per 32-cell word
__global__ void pack_kernel(const uint8_t *bytes, int64_t rows, int64_t W, int64_t stride, uint32_t *bits,
                            int64_t pitch, uint32_t *nonbinary)
{
    const int64_t Wd = W / 32;
    const int64_t n = rows * Wd;
    uint32_t bad = 0;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t y = i / Wd, w = i % Wd;
        const uint8_t *p = bytes + y * stride + 32 * w;
        uint32_t v = 0;
#pragma unroll 8
        for (int b = 0; b < 32; ++b) {
            const uint8_t c = p[b];
            v |= (uint32_t)(c == 255) << b;
            bad |= (c != 0 && c != 255);
        }
        bits[y * pitch + w] = v;
    }
    if (nonbinary && bad) atomicOr(nonbinary, 1u);
}

// bits -> bytes (0/255): one thread per 32-cell word, two 16-byte stores
__global__ void unpack_kernel(const uint32_t *bits, int64_t rows, int64_t W, int64_t pitch, uint8_t *bytes,
                              int64_t stride)
{
    const int64_t Wd = W / 32;
    const int64_t n = rows * Wd;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t y = i / Wd, w = i % Wd;
        const uint32_t v = bits[y * pitch + w];
        uint32_t o[8];
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            const uint32_t nib = (v >> (4 * q)) & 0xF;
            // spread 4 bits to 4 bytes, then 0x01 -> 0xFF
            const uint32_t s = (nib & 1) | ((nib & 2) << 7) | ((nib & 4) << 14) | ((nib & 8) << 21);
            o[q] = (s << 8) - s;
        }
        uint8_t *dst = bytes + y * stride + 32 * w;
        if (((uintptr_t)dst & 15) == 0) {
            reinterpret_cast<uint4 *>(dst)[0] = make_uint4(o[0], o[1], o[2], o[3]);
            reinterpret_cast<uint4 *>(dst)[1] = make_uint4(o[4], o[5], o[6], o[7]);
        } else {
            for (int q = 0; q < 8; ++q)
                for (int b = 0; b < 4; ++b) dst[4 * q + b] = (uint8_t)(o[q] >> (8 * b));
        }
    }
}

// Alive-cell list, row-major (broker.go:47-58): one wave per row, ballot + mbcnt prefix over
// 64 cells at a time.  offs[y] = first output index of row y.  With `prev` the listed cells
// are those that differ from `prev` (the CellFlipped events of one turn,
// gol/event.go:50-60): the same kernels over bits ^ prev.  y0 is the global row of row 0.
__global__ void alive_list_bits_kernel(const uint32_t *bits, const uint32_t *prev, int64_t rows, int64_t Wd,
                                       int64_t pitch, const int64_t *offs, int32_t *xy, int64_t cap, int64_t y0)
{
    const int lane = threadIdx.x & 63;
    const int64_t y = blockIdx.x * (int64_t)(blockDim.x >> 6) + (threadIdx.x >> 6);
    if (y >= rows) return;
    int64_t base = offs[y];
    for (int64_t w0 = 0; w0 < Wd; w0 += 64) {
        const int64_t w = w0 + lane;
        const uint32_t v = w < Wd ? bits[y * pitch + w] ^ (prev ? prev[y * pitch + w] : 0u) : 0u;
        const uint32_t c = __popc(v);
        // exclusive prefix of c over the wave
        uint32_t incl = c;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const uint32_t t = __shfl_up(incl, off, 64);
            if (lane >= off) incl += t;
        }
        int64_t o = base + (incl - c);
        uint32_t m = v;
        while (m) {
            const int b = __ffs(m) - 1;
            m &= m - 1;
            if (o < cap) { xy[2 * o] = (int32_t)(32 * w + b); xy[2 * o + 1] = (int32_t)(y0 + y); }
            ++o;
        }
        base += __shfl(incl, 63, 64);
    }
}

// bytes: a cell is alive when != 0 (broker.go:50-55); with `prev`, listed when its alive state
// differs from prev's.
__device__ __forceinline__ bool byte_listed(const uint8_t *bytes, const uint8_t *prev, int64_t i)
{
    return (bytes[i] != 0) != (prev ? prev[i] != 0 : false);
}

__global__ void alive_list_bytes_kernel(const uint8_t *bytes, const uint8_t *prev, int64_t rows, int64_t W,
                                        int64_t stride, const int64_t *offs, int32_t *xy, int64_t cap, int64_t y0)
{
    const int lane = threadIdx.x & 63;
    const int64_t y = blockIdx.x * (int64_t)(blockDim.x >> 6) + (threadIdx.x >> 6);
    if (y >= rows) return;
    int64_t base = offs[y];
    for (int64_t x0 = 0; x0 < W; x0 += 64) {
        const int64_t x = x0 + lane;
        const bool alive = x < W && byte_listed(bytes, prev, y * stride + x);
        const uint64_t m = __ballot(alive);
        if (alive) {
            const int64_t o = base + __popcll(m & ((1ULL << lane) - 1));
            if (o < cap) { xy[2 * o] = (int32_t)x; xy[2 * o + 1] = (int32_t)(y0 + y); }
        }
        base += __popcll(m);
    }
}

__global__ void row_counts_bits_kernel(const uint32_t *bits, const uint32_t *prev, int64_t rows, int64_t Wd,
                                       int64_t pitch, int64_t *out)
{
    const int lane = threadIdx.x & 63;
    const int64_t y = blockIdx.x * (int64_t)(blockDim.x >> 6) + (threadIdx.x >> 6);
    if (y >= rows) return;
    uint64_t c = 0;
    for (int64_t w = lane; w < Wd; w += 64) c += __popc(bits[y * pitch + w] ^ (prev ? prev[y * pitch + w] : 0u));
    c = wave_sum_u64(c);
    if (lane == 0) out[y] = (int64_t)c;
}

__global__ void row_counts_bytes_kernel(const uint8_t *bytes, const uint8_t *prev, int64_t rows, int64_t W,
                                        int64_t stride, int64_t *out)
{
    const int lane = threadIdx.x & 63;
    const int64_t y = blockIdx.x * (int64_t)(blockDim.x >> 6) + (threadIdx.x >> 6);
    if (y >= rows) return;
    uint64_t c = 0;
    for (int64_t x = lane; x < W; x += 64) c += byte_listed(bytes, prev, y * stride + x);
    c = wave_sum_u64(c);
    if (lane == 0) out[y] = (int64_t)c;
}

}  // namespace golk

// ------------------------------------------------------------------ IPC sequence flags
// The IPC halo transport (gol_ipc.cpp): a rank's flag words live in its own HBM and are polled by
// its ring neighbours' kernels through IPC mappings (other processes, the same or another GPU).
// Stream order puts a signal after the launches whose rows it announces (their end-of-kernel
// release has written them back), and the copy after the wait that acquired the flag.
__global__ void ipc_signal_kernel(uint32_t *flag, uint32_t value)
{
    if (threadIdx.x == 0) __hip_atomic_store(flag, value, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}

struct IpcWaitArgs {
    const uint32_t *f0, *f1, *f2, *f3;
    int32_t n;
    uint32_t want;
    uint64_t timeout;
    uint32_t *err;
};

// Lane i < n polls flag i (a bounded wait: every lane leaves, with or without the flag).
__global__ void ipc_wait_kernel(IpcWaitArgs a)
{
    const int lane = threadIdx.x;
    bool ok = true;
    if (lane < a.n) {
        const uint32_t *f = lane == 0 ? a.f0 : (lane == 1 ? a.f1 : (lane == 2 ? a.f2 : a.f3));
        const uint64_t t0 = __builtin_amdgcn_s_memrealtime();
        for (;;) {
            const uint32_t v = __hip_atomic_load(f, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_SYSTEM);
            if ((int32_t)(v - a.want) >= 0) break;
            if (__builtin_amdgcn_s_memrealtime() - t0 > a.timeout) {
                ok = false;
                break;
            }
            __builtin_amdgcn_s_sleep(8);
        }
    }
    if (!ok) atomicOr(a.err, GOLK_ERR_IPC);
}

// ------------------------------------------------------------------ launchers
using namespace golk;

static inline int grid_for(int64_t n, int block = 256, int64_t cap = 256 * 16)
{
    int64_t g = (n + block - 1) / block;
    if (g < 1) g = 1;
    if (g > cap) g = cap;
    return (int)g;
}

// A per-device buffer of `words` zeroed words, allocated at its first use and kept in `bufs`.
// Zeroed and synchronised: launches on non-blocking streams are not ordered after the null stream.
static uint32_t *device_words(std::map<int, uint32_t *> &bufs, int device, size_t words)
{
    static std::mutex mu;
    std::lock_guard<std::mutex> lock(mu);
    auto it = bufs.find(device);
    if (it != bufs.end()) return it->second;
    int prev = 0;
    uint32_t *w = nullptr;
    if (hipGetDevice(&prev) != hipSuccess || hipSetDevice(device) != hipSuccess) return nullptr;
    if (hipMalloc(&w, words * sizeof(uint32_t)) != hipSuccess || hipMemset(w, 0, words * sizeof(uint32_t)) != hipSuccess ||
        hipDeviceSynchronize() != hipSuccess)
        w = nullptr;
    (void)hipSetDevice(prev);
    if (w) bufs[device] = w;
    return w;
}

// Per-device error word used when a launcher is called without one (gol_dev_* launchers).
uint32_t *golk_device_err_word(int device)
{
    static std::map<int, uint32_t *> words;
    return device_words(words, device, 1);
}

// Per-device CU slot masks of the band pipeline (GOL_BAND_PLACE; zeroed once, every workgroup
// frees its slot on exit).
uint32_t *golk_cu_slots(int device)
{
    static std::map<int, uint32_t *> tabs;
    return device_words(tabs, device, GOL_CU_SLOT_WORDS);
}

hipError_t golk_reset_cu_slots(int device, hipStream_t s)
{
    uint32_t *w = golk_cu_slots(device);
    return w ? hipMemsetAsync(w, 0, GOL_CU_SLOT_WORDS * sizeof(uint32_t), s) : hipErrorOutOfMemory;
}

static uint32_t *err_or_default(uint32_t *err)
{
    if (err) return err;
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return nullptr;
    return golk_device_err_word(dev);
}

template <int K, int DW>
static hipError_t launch_bits(const BitsArgs &a, hipStream_t s)
{
    const int nstrips = (int)((a.rows + a.strip - 1) / a.strip);
    dim3 grid((a.ngroups + 3) / 4, nstrips);
    hipLaunchKernelGGL((bits_step_kernel<K, DW>), grid, dim3(256), 0, s, a);
    return hipGetLastError();
}

template <int DW>
static hipError_t launch_bits_k(int k, const BitsArgs &a, hipStream_t s)
{
    switch (k) {
    case 1: return launch_bits<1, DW>(a, s);
    case 2: return launch_bits<2, DW>(a, s);
    case 4: return launch_bits<4, DW>(a, s);
    case 8: return launch_bits<8, DW>(a, s);
    case 16: if constexpr (DW <= 2) return launch_bits<16, DW>(a, s);
             return hipErrorInvalidValue;
    default: return hipErrorInvalidValue;
    }
}

int golk_auto_strip(int64_t rows, int64_t ngroups, int k)
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
    if (rows * ngroups < lo * 512) lo = std::max<int64_t>(1, rows * ngroups / 512);
    if (strip < lo) strip = lo;
    if (strip > rows) strip = rows;
    if (strip < 1) strip = 1;
    return (int)strip;
}

// Workgroups of `kernel` (block threads) resident on the whole device at once (cached).
static int64_t resident_workgroups(const void *kernel, int block)
{
    static std::mutex mu;
    static std::map<std::pair<const void *, int>, int64_t> cache;
    int dev = 0, cus = 0, per_cu = 0;
    if (hipGetDevice(&dev) != hipSuccess) return 0;
    std::lock_guard<std::mutex> lock(mu);
    auto it = cache.find({kernel, dev});
    if (it != cache.end()) return it->second;
    int64_t n = 0;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess &&
        hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel, block, 0) == hipSuccess)
        n = (int64_t)cus * per_cu;
    cache[{kernel, dev}] = n;
    return n;
}

// Arguments of a step launch (golk_bits_step, golk_band_step, golk_rule_step): waves of U output
// words, strips of `strip` rows (<= 0: golk_auto_strip), no strip map, error word or CU slots.
static BitsArgs step_args(const uint32_t *top, const uint32_t *mid, const uint32_t *bot, uint32_t *dst, int64_t R,
                          int64_t Wd, int64_t pitch, int64_t row0, int64_t rows, int U, int k, int strip,
                          uint64_t *slots)
{
    BitsArgs a;
    a.top = top; a.mid = mid; a.bot = bot; a.dst = dst;
    a.R = R; a.Wd = Wd; a.pitch = pitch; a.row0 = row0; a.rows = rows;
    a.ngroups = (int)((Wd + U - 1) / U);
    a.strip = strip > 0 ? std::min(strip, GOL_MAX_STRIP) : golk_auto_strip(rows, a.ngroups, k);
    a.slots = slots;
    a.sm = StripMap{};
    a.err = nullptr;  // no flag waits in the step kernels
    a.cu_slots = nullptr;
    return a;
}

hipError_t golk_bits_step(const uint32_t *top, const uint32_t *mid, const uint32_t *bot, uint32_t *dst,
                          int64_t R, int64_t Wd, int64_t pitch, int64_t row0, int64_t rows, int k, int dw,
                          int strip, uint64_t *slots, hipStream_t s)
{
    if (rows <= 0) return hipSuccess;
    const BitsArgs a = step_args(top, mid, bot, dst, R, Wd, pitch, row0, rows, 62 * dw, k, strip, slots);
    switch (dw) {
    case 1: return launch_bits_k<1>(k, a, s);
    case 2: return launch_bits_k<2>(k, a, s);
    case 4: return launch_bits_k<4>(k, a, s);
    default: return hipErrorInvalidValue;
    }
}

template <int DW, bool C>
static hipError_t launch_band(int k, dim3 grid, const BitsArgs &a, hipStream_t s)
{
    switch (k) {
    case 1: hipLaunchKernelGGL((band_step_kernel<1, DW, C>), grid, dim3(256), 0, s, a); break;
    case 2: hipLaunchKernelGGL((band_step_kernel<2, DW, C>), grid, dim3(256), 0, s, a); break;
    case 4: hipLaunchKernelGGL((band_step_kernel<4, DW, C>), grid, dim3(256), 0, s, a); break;
    case 8: hipLaunchKernelGGL((band_step_kernel<8, DW, C>), grid, dim3(256), 0, s, a); break;
    case 12: if constexpr (DW <= 2) { hipLaunchKernelGGL((band_step_kernel<12, DW, C>), grid, dim3(256), 0, s, a); break; }
             return hipErrorInvalidValue;
    case 16: if constexpr (DW <= 2) { hipLaunchKernelGGL((band_step_kernel<16, DW, C>), grid, dim3(256), 0, s, a); break; }
             return hipErrorInvalidValue;
    default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

static int device_cus()
{
    int dev = 0, cus = 0;
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess)
        return 0;
    return cus;
}

// Claim counters of the paired ranks (StripMap), one zeroed buffer per stream: launches on one
// stream run in order and leave their counters zeroed; launches on different streams may run
// at once and must not share counters.  The buffer is zeroed ON that stream (stream-ordered
// before the launch that asks for it): a null-stream hipMemset is not ordered before work on a
// non-blocking stream, and a first launch that raced it counted rows twice (overlapping claims;
// tests/test_gpu_engine.py::test_band_paired_narrow_board).  A launch that faults (a pipeline
// wave timed out) can leave counters set: golk_reset_claims zeroes a device's buffers again.
static std::mutex claims_mu;
static std::map<std::pair<hipStream_t, int>, uint32_t *> claims_bufs;
static size_t claims_bytes(int cus) { return (size_t)cus * 2 * 16 * sizeof(uint32_t); }
static uint32_t *claim_counters(hipStream_t s, int cus)
{
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return nullptr;
    std::lock_guard<std::mutex> lock(claims_mu);
    auto it = claims_bufs.find({s, dev});
    if (it != claims_bufs.end()) return it->second;
    uint32_t *c = nullptr;
    if (hipMalloc(&c, claims_bytes(cus)) != hipSuccess) return nullptr;
    if (hipMemsetAsync(c, 0, claims_bytes(cus), s) != hipSuccess) {
        (void)hipFree(c);
        return nullptr;
    }
    claims_bufs[{s, dev}] = c;
    return c;
}

static std::set<hipStream_t> engine_streams;  // streams owned by an engine (golk_own_stream)

hipError_t golk_reset_claims(hipStream_t s)
{
    std::lock_guard<std::mutex> lock(claims_mu);
    hipError_t e = hipSuccess;
    for (auto &kv : claims_bufs) {
        if (kv.first.first != s) continue;
        int cus = 0;
        e = hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, kv.first.second);
        if (e == hipSuccess) e = hipMemsetAsync(kv.second, 0, claims_bytes(cus), s);  // before any later launch on s
        if (e != hipSuccess) break;
    }
    return e;
}

void golk_release_claims(hipStream_t s)
{
    std::lock_guard<std::mutex> lock(claims_mu);
    for (auto it = claims_bufs.begin(); it != claims_bufs.end();) {
        if (it->first.first == s) {
            (void)hipFree(it->second);
            it = claims_bufs.erase(it);
        } else {
            ++it;
        }
    }
    engine_streams.erase(s);
}

void golk_own_stream(hipStream_t s)
{
    std::lock_guard<std::mutex> lock(claims_mu);
    engine_streams.insert(s);
}

hipError_t golk_reset_claims_device(int device)
{
    // Synchronous, on the null stream between two device-wide synchronisations: a caller's stream
    // that owns a buffer here may have been destroyed since (its handle is not used), and the
    // second synchronisation orders the zeroing before any later launch on a non-blocking stream.
    std::lock_guard<std::mutex> lock(claims_mu);
    int cus = 0, prev = 0;
    hipError_t e = hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device);
    if (e == hipSuccess) e = hipGetDevice(&prev);
    if (e == hipSuccess) e = hipSetDevice(device);
    if (e != hipSuccess) return e;
    e = hipDeviceSynchronize();
    for (auto &kv : claims_bufs) {
        if (e != hipSuccess) break;
        if (kv.first.second != device || engine_streams.count(kv.first.first)) continue;
        e = hipMemset(kv.second, 0, claims_bytes(cus));
    }
    if (e == hipSuccess) {
        uint32_t *w = golk_cu_slots(device);  // (placement only: a timed-out workgroup kept its slot)
        if (w) e = hipMemset(w, 0, GOL_CU_SLOT_WORDS * sizeof(uint32_t));
    }
    if (e == hipSuccess) e = hipDeviceSynchronize();
    (void)hipSetDevice(prev);
    return e;
}

// The device a pipelined launch is scheduled for: this one (as_cus = as_slots = 0), or a
// pretended smaller one of as_cus CUs (a multiple of 8) holding as_slots resident workgroups of
// `kernel`; false: it asks for more than this device has.
static bool pipe_device(const void *kernel, int block, int as_cus, int64_t as_slots, int &cus, int64_t &slots)
{
    cus = device_cus();
    slots = resident_workgroups(kernel, block);
    if (!as_cus && !as_slots) return true;
    if (as_cus <= 0 || as_cus % 8 || as_cus > cus || as_slots <= 0 || as_slots > slots) return false;
    cus = as_cus;
    slots = as_slots;
    return true;
}

// The strips of a pipelined launch: the device it is scheduled for (pipe_device; false: no such
// device), `plan`'s StripPlan for it (band_strip_plan / bytes_strip_plan) and, for a paired plan,
// the stream's claim counters -- sized by the device itself, whichever device the launch is
// scheduled for; without them the plan is made again unpaired.
typedef StripPlan (*StripPlanFn)(int64_t, int64_t, int64_t, int, int, int, int64_t, bool);
static bool pipe_plan(StripPlanFn plan, const void *kernel, int block, int64_t rows, int64_t width, int64_t pitch, int k,
                      int strip_rows, int as_cus, int64_t as_slots, hipStream_t s, int32_t &strip, StripMap &sm,
                      unsigned &nwg)
{
    int cus = 0;
    int64_t resident = 0;
    if (!pipe_device(kernel, block, as_cus, as_slots, cus, resident)) return false;
    StripPlan p = plan(rows, width, pitch, k, strip_rows, cus, resident, true);
    uint32_t *claims = p.mode == GOL_STRIPS_RANKED_PAIRED ? claim_counters(s, device_cus()) : nullptr;
    if (p.mode == GOL_STRIPS_RANKED_PAIRED && !claims) p = plan(rows, width, pitch, k, strip_rows, cus, resident, false);
    strip = p.strip;
    sm = p.sm;
    sm.claims = claims;
    nwg = (unsigned)p.nwg;
    return true;
}

bool golk_pipe_limits(bool band, bool contig, bool count, int *cus, int64_t *slots)
{
    *cus = device_cus();
    *slots = band ? resident_workgroups(golk_band_pipe_fn(contig, count), 64 * GOL_BAND_P)
                  : resident_workgroups(golk_bytes_pipe_fn(count), 64 * GOL_BYTES_PIPE_P);
    return *cus > 0 && *slots > 0;
}

hipError_t golk_band_step(const uint32_t *top, const uint32_t *mid, const uint32_t *bot, uint32_t *dst, int64_t R,
                          int64_t Wd, int64_t pitch, int64_t row0, int64_t rows, int k, int dw, int strip,
                          uint64_t *slots, uint32_t *err, hipStream_t s, int as_cus, int64_t as_slots)
{
    if (rows <= 0) return hipSuccess;
    BitsArgs a = step_args(top, mid, bot, dst, R, Wd, pitch, row0, rows, band_useful_words(k, dw), k, strip, slots);
    a.err = err_or_default(err);
    if (!a.err) return hipErrorOutOfMemory;
    if (GOL_BAND_PLACE) {
        int dev = 0;
        if (hipGetDevice(&dev) == hipSuccess) a.cu_slots = golk_cu_slots(dev);
    }
    const bool contig = top + (int64_t)k * pitch == mid && bot == mid + R * pitch;
    if (dw == 4 && k == GOL_BAND_KW * GOL_BAND_P) {
        // k = 12 on the band layout: 4 waves x 3 stages (band_pipe_kernel), one workgroup per
        // (column group, range of rows): band_strip_plan.
        const bool count = a.slots != nullptr;
        unsigned nwg = 0;
        if (!pipe_plan(band_strip_plan, golk_band_pipe_fn(contig, count), 64 * GOL_BAND_P, rows, Wd, pitch, k, strip,
                       as_cus, as_slots, s, a.strip, a.sm, nwg))
            return hipErrorInvalidValue;
        return golk_band_pipe_launch(contig, count, nwg, a, s);
    }
    if (as_cus || as_slots) return hipErrorInvalidValue;
    dim3 grid((a.ngroups + 3) / 4, (int)((rows + a.strip - 1) / a.strip));
    if (dw == 2) return contig ? launch_band<2, true>(k, grid, a, s) : launch_band<2, false>(k, grid, a, s);
    if (dw == 4) return contig ? launch_band<4, true>(k, grid, a, s) : launch_band<4, false>(k, grid, a, s);
    return hipErrorInvalidValue;
}

int golk_band_useful_words(int k, int dw) { return band_useful_words(k, dw); }

// Life-like rules: the step kernels with the rule as data, general row addressing.
template <int K>
static hipError_t launch_rule(bool band, dim3 grid, const TableRule::Args &a, hipStream_t s)
{
    constexpr int DW = GOLK_RULE_DW;
    if (band) hipLaunchKernelGGL((band_step_kernel<K, DW, false, TableRule>), grid, dim3(256), 0, s, a);
    else hipLaunchKernelGGL((bits_step_kernel<K, DW, TableRule>), grid, dim3(256), 0, s, a);
    return hipGetLastError();
}

int golk_rule_useful_words(bool band, int k) { return band ? band_useful_words(k, GOLK_RULE_DW) : 62 * GOLK_RULE_DW; }

hipError_t golk_rule_step(const uint32_t *top, const uint32_t *mid, const uint32_t *bot, uint32_t *dst, int64_t R,
                          int64_t Wd, int64_t pitch, int64_t row0, int64_t rows, int k, bool band, uint32_t birth,
                          uint32_t survive, int strip, uint64_t *slots, hipStream_t s)
{
    if (rows <= 0) return hipSuccess;
    if (birth >= 512 || survive >= 512 || Wd % GOLK_RULE_DW || pitch % GOLK_RULE_DW) return hipErrorInvalidValue;
    const TableRule::Args a{step_args(top, mid, bot, dst, R, Wd, pitch, row0, rows, golk_rule_useful_words(band, k), k,
                                      strip, slots),
                            birth, survive};
    const dim3 grid((a.ngroups + 3) / 4, (unsigned)((rows + a.strip - 1) / a.strip));
    switch (k) {
    case 1: return launch_rule<1>(band, grid, a, s);
    case 2: return launch_rule<2>(band, grid, a, s);
    case 4: return launch_rule<4>(band, grid, a, s);
    case 8: return launch_rule<8>(band, grid, a, s);
    default: return hipErrorInvalidValue;
    }
}

double golk_step_rounds(bool band, int64_t rows, int64_t Wd, int64_t pitch, int k, int dw, int strip)
{
    if (!band || dw != 4 || k != GOL_BAND_KW * GOL_BAND_P || rows <= 0) return 1e9;
    const int64_t slots = resident_workgroups(golk_band_pipe_fn(true, true), 64 * GOL_BAND_P);
    if (slots <= 0) return 1e9;
    const StripPlan p = band_strip_plan(rows, Wd, pitch, k, strip, device_cus(), slots);  // the launch's own plan
    return p.sm.ranked ? 1.0 : (double)p.nwg / (double)slots;
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

hipError_t golk_bytes_blocked(const uint8_t *top, const uint8_t *mid, const uint8_t *bot, uint8_t *dst, int64_t R,
                              int64_t W, int64_t pitch, int64_t row0, int64_t rows, int k, int strip, uint64_t *slots,
                              uint32_t *err, hipStream_t s, int as_cus, int64_t as_slots)
{
    BytesKArgs a;
    a.top = top; a.mid = mid; a.bot = bot; a.dst = dst;
    a.R = R; a.Wd = W / 32; a.pitch = pitch; a.row0 = row0; a.rows = rows;
    a.ngroups = (int)((a.Wd + 61) / 62);
    a.strip = strip > 0 ? std::min(strip, GOL_MAX_STRIP) : golk_auto_strip(rows, a.ngroups, k);
    a.slots = slots;
    a.err = err_or_default(err);
    if (rows <= 0) return hipSuccess;
    if (!a.err) return hipErrorOutOfMemory;
    a.sm = StripMap{};
    if (k == 32) {
        // one workgroup of GOL_BYTES_PIPE_P waves per (column group, strip): bytes_strip_plan
        const bool count = a.slots != nullptr;
        unsigned nwg = 0;
        if (!pipe_plan(bytes_strip_plan, golk_bytes_pipe_fn(count), 64 * GOL_BYTES_PIPE_P, rows, W, pitch, k, strip,
                       as_cus, as_slots, s, a.strip, a.sm, nwg))
            return hipErrorInvalidValue;
        return golk_bytes_pipe_launch(count, nwg, a, s);
    }
    if (as_cus || as_slots) return hipErrorInvalidValue;
    const int nstrips = (int)((rows + a.strip - 1) / a.strip);
    dim3 grid((a.ngroups + 3) / 4, nstrips);
    switch (k) {
    case 1: hipLaunchKernelGGL(bytes_blocked_kernel<1>, grid, dim3(256), 0, s, a); break;
    case 2: hipLaunchKernelGGL(bytes_blocked_kernel<2>, grid, dim3(256), 0, s, a); break;
    case 4: hipLaunchKernelGGL(bytes_blocked_kernel<4>, grid, dim3(256), 0, s, a); break;
    case 8: hipLaunchKernelGGL(bytes_blocked_kernel<8>, grid, dim3(256), 0, s, a); break;
    case 16: hipLaunchKernelGGL(bytes_blocked_kernel<16>, grid, dim3(256), 0, s, a); break;
    default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

hipError_t golk_nonbinary(const uint8_t *bytes, int64_t rows, int64_t W, int64_t stride, uint32_t *flag, hipStream_t s)
{
    if (rows <= 0) return hipSuccess;
    hipLaunchKernelGGL(nonbinary_kernel, dim3(grid_for(rows * W, 256, 256 * 16)), dim3(256), 0, s, bytes, rows, W, stride,
                       flag);
    return hipGetLastError();
}

hipError_t golk_random_fill(uint32_t *dst, int64_t rows, int64_t grow0, int64_t W, int64_t pitch, uint64_t seed,
                            hipStream_t s)
{
    const int64_t Ww = W / 64;
    if (rows <= 0) return hipSuccess;
    hipLaunchKernelGGL(random_fill_kernel, dim3(grid_for(rows * Ww, 256, 256 * 64)), dim3(256), 0, s, dst, rows,
                       grow0, Ww, pitch, seed);
    return hipGetLastError();
}

hipError_t golk_popcount(const uint32_t *src, int64_t rows, int64_t Wd, int64_t pitch, uint64_t *slots, hipStream_t s)
{
    hipLaunchKernelGGL(popcount_kernel, dim3(grid_for(rows * Wd, 256, 256 * 16)), dim3(256), 0, s, src, rows, Wd,
                       pitch, slots);
    return hipGetLastError();
}

hipError_t golk_slots_reduce(uint64_t *slots, int64_t n, uint64_t *out, hipStream_t s)
{
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(slots_reduce_kernel, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, s, slots, n, out);
    return hipGetLastError();
}

hipError_t golk_hash(const uint32_t *src, int64_t rows, int64_t grow0, int64_t Wd, int64_t pitch, uint64_t *slots,
                     hipStream_t s)
{
    hipLaunchKernelGGL(hash_kernel, dim3(grid_for(rows * (Wd / 2), 256, 256 * 16)), dim3(256), 0, s, src, rows,
                       grow0, Wd / 2, pitch, slots);
    return hipGetLastError();
}

hipError_t golk_count_bytes(const uint8_t *src, int64_t rows, int64_t W, int64_t stride, uint64_t *slots,
                            hipStream_t s)
{
    hipLaunchKernelGGL(count_nonzero_bytes_kernel, dim3(grid_for(rows * W, 256, 256 * 16)), dim3(256), 0, s, src,
                       rows, W, stride, slots);
    return hipGetLastError();
}

hipError_t golk_pack(const uint8_t *bytes, int64_t rows, int64_t W, int64_t stride, uint32_t *bits, int64_t pitch,
                     uint32_t *nonbinary, hipStream_t s)
{
    if (rows <= 0) return hipSuccess;
    hipLaunchKernelGGL(pack_kernel, dim3(grid_for(rows * (W / 32), 256, 256 * 64)), dim3(256), 0, s, bytes, rows, W,
                       stride, bits, pitch, nonbinary);
    return hipGetLastError();
}

hipError_t golk_unpack(const uint32_t *bits, int64_t rows, int64_t W, int64_t pitch, uint8_t *bytes, int64_t stride,
                       hipStream_t s)
{
    if (rows <= 0) return hipSuccess;
    hipLaunchKernelGGL(unpack_kernel, dim3(grid_for(rows * (W / 32), 256, 256 * 64)), dim3(256), 0, s, bits, rows, W,
                       pitch, bytes, stride);
    return hipGetLastError();
}

hipError_t golk_row_counts(bool bits_mode, const void *board, const void *prev, int64_t rows, int64_t width_units,
                           int64_t pitch, int64_t *out, hipStream_t s)
{
    const int wpb = 4;
    if (rows <= 0) return hipSuccess;
    dim3 grid((unsigned)((rows + wpb - 1) / wpb));
    if (bits_mode)
        hipLaunchKernelGGL(row_counts_bits_kernel, grid, dim3(64 * wpb), 0, s, (const uint32_t *)board,
                           (const uint32_t *)prev, rows, width_units, pitch, out);
    else
        hipLaunchKernelGGL(row_counts_bytes_kernel, grid, dim3(64 * wpb), 0, s, (const uint8_t *)board,
                           (const uint8_t *)prev, rows, width_units, pitch, out);
    return hipGetLastError();
}

hipError_t golk_alive_list(bool bits_mode, const void *board, const void *prev, int64_t rows, int64_t width_units,
                           int64_t pitch, const int64_t *offs, int32_t *xy, int64_t cap, int64_t y0, hipStream_t s)
{
    const int wpb = 4;
    if (rows <= 0) return hipSuccess;
    dim3 grid((unsigned)((rows + wpb - 1) / wpb));
    if (bits_mode)
        hipLaunchKernelGGL(alive_list_bits_kernel, grid, dim3(64 * wpb), 0, s, (const uint32_t *)board,
                           (const uint32_t *)prev, rows, width_units, pitch, offs, xy, cap, y0);
    else
        hipLaunchKernelGGL(alive_list_bytes_kernel, grid, dim3(64 * wpb), 0, s, (const uint8_t *)board,
                           (const uint8_t *)prev, rows, width_units, pitch, offs, xy, cap, y0);
    return hipGetLastError();
}

hipError_t golk_ipc_signal(uint32_t *flag, uint32_t value, hipStream_t s)
{
    hipLaunchKernelGGL(ipc_signal_kernel, dim3(1), dim3(64), 0, s, flag, value);
    return hipGetLastError();
}

hipError_t golk_ipc_wait(const uint32_t *const *flags, int n, uint32_t want, uint64_t timeout_ticks, uint32_t *err,
                         hipStream_t s)
{
    if (n <= 0) return hipSuccess;
    if (n > GOLK_IPC_MAX_WAIT || !err) return hipErrorInvalidValue;
    IpcWaitArgs a;
    a.f0 = flags[0];
    a.f1 = n > 1 ? flags[1] : flags[0];
    a.f2 = n > 2 ? flags[2] : flags[0];
    a.f3 = n > 3 ? flags[3] : flags[0];
    a.n = n;
    a.want = want;
    a.timeout = timeout_ticks;
    a.err = err;
    hipLaunchKernelGGL(ipc_wait_kernel, dim3(1), dim3(64), 0, s, a);
    return hipGetLastError();
}
