// gol_band_pipe.hip -- the band layout's split pipeline (k = 12 per launch): band_pipe_kernel,
// its CU-slot role placement and its launch, in a translation unit of its own so that it is
// compiled under the machine scheduler that runs it fastest (Makefile BANDFLAGS).
#include <type_traits>

#include "gol_pipe.h"
#include "gol_step_kernels.h"

namespace golk {

// The K = KW*P stages split over the P waves of one workgroup: wave w runs stages
// [w*KW, (w+1)*KW) and hands every block of RPB = 2 rows (one pair step) to wave w+1 through an
// LDS ring of NS = 4 slots.  A wave then holds 5*KW*4 pipeline VGPRs instead of 5*K*4, which fits
// 4 waves per SIMD.  Wave 0 stages its input rows HBM -> LDS with global_load_lds (no VGPRs),
// wave P-1 stores to HBM.  Synchronisation is per ring, by LDS flags: ready[e] = blocks
// published into ring e, consumed[e] = blocks taken out of it; a producer fills slot b % NS
// once block b-NS is consumed.  Every spin is bounded (spin_until_ge).  1-D grid of work items
// (work_item).
// COUNT: the last wave adds the alive cells of the rows it stores to a.slots (branch-free: a
// per-row uniform select, no branch around the count as a null-slots check made it).
// Role placement (GOL_BAND_PLACE): a workgroup of the band pipeline claims a free slot q (0..3) in
// its CU's mask and each wave takes pipeline role (its SIMD + q) % 4, so that the (up to) four
// workgroups resident on a CU put one wave of every role on every SIMD.  (Roles by wave index +
// a per-workgroup rotation put two waves of one role on a SIMD for 64-75 % of the waves,
// tools/timeline.py, profiles/r03/r03h_tl_roles.jsonl.)  Vector atomics of lane 0.
// (The knob's default, 1, is in gol_step_device.h: the launcher reads it too.)
__device__ __forceinline__ uint32_t cu_slot_index()
{
    const uint32_t hw = __builtin_amdgcn_s_getreg((31 << 11) | 4);  // HW_ID
    const uint32_t xcc = __builtin_amdgcn_s_getreg((31 << 11) | 20) & 7u;  // XCC_ID
    return (xcc << 8) | (((hw >> 13) & 7u) << 5) | (((hw >> 12) & 1u) << 4) | ((hw >> 8) & 0xFu);
}
__device__ __forceinline__ int claim_cu_slot(uint32_t *m)
{
    uint32_t cur = __hip_atomic_load(m, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    for (int i = 0; i < 8; ++i) {
        const uint32_t fr = ~cur & 0xFu;
        if (!fr) return -1;
        const int b = __ffs(fr) - 1;
        const uint32_t old = atomicCAS(m, cur, cur | (1u << b));
        if (old == cur) return b;
        cur = old;
    }
    return -1;
}

// Cache policy bits of the band pipeline's output stores (2 = nt, streaming) and input loads.
#ifndef GOL_BAND_STORE_AUX
#define GOL_BAND_STORE_AUX 2
#endif
#ifndef GOL_BAND_LOAD_AUX
#define GOL_BAND_LOAD_AUX 0
#endif
// (Pipeline shape of k = 12, GOL_BAND_KW / _P / _RPB / _NS: gol_strips.h.)
// The loader issues block b + GOL_BAND_PREFETCH at block b (its in_ring slot was read at the start
// of block b + GOL_BAND_PREFETCH - NS, so up to NS) and waits for block b + 1 only.  Same box, 3
// reps: 3 against 2 weak 163.6-164.1 vs 163.1-163.7 TCUPS, 262144^2 +0.6 %, 65536^2 +1.2 %; 4 as 3
// (profiles/r05/r05d_ab_prefetch.jsonl).
#ifndef GOL_BAND_PREFETCH
#define GOL_BAND_PREFETCH 3
#endif
template <int KW, int P, bool CONTIG, bool COUNT>
__global__ void __launch_bounds__(64 * P)
__attribute__((amdgpu_waves_per_eu(KW >= 4 ? 3 : 4, 8)))  // 5 KW DW pipeline VGPRs
band_pipe_kernel(BitsArgs a)
{
    constexpr int DW = 4;
    constexpr int K = KW * P;
    constexpr int HL = band_halo_lanes(K, DW);
    constexpr int U = band_useful_words(K, DW);
    constexpr int ROW = 64 * DW;
    constexpr int RPB = GOL_BAND_RPB;  // rows per block: one pair step
    constexpr int NS = GOL_BAND_NS;    // (the loops below are unrolled over the NS slots)
    static_assert(RPB == 2, "a block is one pair step");
    __shared__ uint32_t in_ring[NS][RPB][ROW];
    __shared__ uint32_t ring_[P - 1][NS][RPB][ROW];  // ring e+1 in the text = ring[e] here
    __shared__ int ready_[P], consumed_[P];
    __shared__ int flag_scratch[64];  // dummy target of lanes 1..63's flag writes (never read; all waves share it)
    __shared__ int place_[P + 2];  // GOL_BAND_PLACE: SIMD of each wave, the CU slot, the mask index

    const int lane = threadIdx.x & 63;
    const int litem = (int)blockIdx.x;
    int group, s0, s1, rotv;
    const bool has_rows = work_item(a.sm, a.ngroups, a.row0, a.rows, a.strip, litem, [] { return gridDim.x; }, group, s0, s1, rotv);
    uint32_t *ctr;
    const int dir = work_dir(a.sm, litem, ctr);  // 0: static strip, +1 / -1: paired (StripMap)
    // Pipeline position of this wave, rotated per workgroup (role placement below refines it)
    int wv = __builtin_amdgcn_readfirstlane(((threadIdx.x >> 6) + rotv) % P);
    constexpr bool PLACE = GOL_BAND_PLACE && P == 4;

    const int64_t col_raw = (int64_t)group * U + (int64_t)(lane - HL) * DW;
    const int64_t band_q = col_raw >= 0 ? col_raw / a.Wd : -((-col_raw + a.Wd - 1) / a.Wd);
    const int64_t col = col_raw - band_q * a.Wd;
    const uint32_t rot = (uint32_t)band_q & 31u;
    const bool wrap = __ballot(rot != 0) != 0;
    const bool writer = lane >= HL && lane < 64 - HL && col_raw < a.Wd;

    const int R = (int)a.R;
    const int first_in = s0 - K;
    const int last_in = s1 + K - 1;
    // the stream: input row first_in + t at stream step t (walking up, dir -1: s1e + K - 1 - t);
    // output row first_in + t - K (s1e - 1 + 2K - t), valid from step 2K on
    const int nblk = ((s1 - s0) + 2 * K + RPB - 1) / RPB;
    // a pair's range, stretched to s1e so that TRIP divides its len + 4K (whole loop trips); rows
    // past s1 are read clamped and never stored; nclaim: blocks of the pair, a multiple of NS
    // (gol_strips.h: the expressions the host's pair_extent evaluates)
    constexpr int TRIP = RPB * NS;  // rows per loop trip
    const int s1e = GOL_PAIR_S1E(dir, s0, s1, K, TRIP);
    const int nclaim = GOL_PAIR_NCLAIM(s0, s1e, K, RPB);

    const int pitch_b = (int)a.pitch * 4;
    const char *mid_b = reinterpret_cast<const char *>(a.mid);
    const int64_t top_d = (reinterpret_cast<const char *>(a.top) - mid_b) + (int64_t)K * pitch_b;
    const int64_t bot_d = (reinterpret_cast<const char *>(a.bot) - mid_b) - (int64_t)R * pitch_b;
    const uint32_t lane_off = (uint32_t)col * 4u;
    char *dst_b = reinterpret_cast<char *>(a.dst);
    const uint32_t st_off = writer ? lane_off : 0x80000000u;

    // wave 0: block b -> in_ring[b % NS] (global_load_lds).  The slot is an argument: a lambda
    // that captures a __shared__ array silently loses the kernel's host-side stub.
    // Interior blocks (both rows inside [first_in, last_in] and, unless CONTIG, inside the shard's
    // own rows: every block but the first and last few of a strip) take the row address carried
    // from the previous block (uniform) plus the lane's offset; the others clamp and pick the row's
    // segment per row.  stage_in is called for blocks 0, 1, 2, ... in order.
    // The slot is an LDS-typed pointer (a generic one costs a null check per load: 4 SALU).  The
    // interior blocks are one range [ib_lo, ib_lo + ib_n) of block numbers, found here once.
    const int in_lo = CONTIG ? first_in : max(first_in, 0), in_hi = CONTIG ? last_in : min(last_in, R - 1);
    const int64_t row_step = dir >= 0 ? (int64_t)pitch_b : -(int64_t)pitch_b;
    const int y_first = dir >= 0 ? first_in : s1e + K - 1;  // first row of block 0
    const int ib_lo = dir >= 0 ? div_ceil_nn(in_lo - y_first, RPB) : div_ceil_nn(y_first - in_hi, RPB);
    const int ib_hi = dir >= 0 ? div_floor(in_hi - (RPB - 1) - y_first, RPB) : div_floor(y_first - (RPB - 1) - in_lo, RPB);
    const uint32_t ib_n = ib_hi >= ib_lo ? (uint32_t)(ib_hi - ib_lo + 1) : 0u;
    const char *st_row = mid_b + (int64_t)y_first * pitch_b;  // the next block's first row (used when interior)
    auto stage_in = [&](int b, lds_u32 *slot) {
        const char *g0 = st_row;
        st_row += RPB * row_step;
        if ((uint32_t)(b - ib_lo) < ib_n) {
            // The block's two rows as two LDS-DMA loads in the SGPR-base form (the row address in
            // an SGPR pair, the lane's 32-bit offset in a VGPR): the builtin's address computation
            // made the compiler use the 64-bit VGPR-address form here, one v_lshl_add_u64 and a
            // VGPR pair read per load.  Same box, 3 reps: weak +0.6-1.0 %, 262144^2 +-0
            // (profiles/r06/r06_ab_saddr.jsonl).  M0 (the LDS destination) is written and
            // restored inside the statement, one wait state before each load (the hazard scan of
            // tools/check_lds_wait.py checks it); s_nop 4 first covers an SGPR base that a VALU
            // (readfirstlane) may have written.
            static_assert(RPB == 2 && GOL_BAND_LOAD_AUX == 0, "two rows per block, default cache policy");
            uint32_t keep;
            const char *g1 = g0 + row_step;
            asm volatile("s_nop 4\n\ts_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\t"
                         "global_load_lds_dwordx4 %1, %3\n\ts_mov_b32 m0, %4\n\ts_nop 0\n\t"
                         "global_load_lds_dwordx4 %1, %5\n\ts_mov_b32 m0, %0"
                         : "=&s"(keep)
                         : "v"(lane_off), "s"(slot), "s"(g0), "s"(slot + ROW), "s"(g1)
                         : "memory");
            return;
        }
#pragma unroll
        for (int s = 0; s < RPB; ++s) {
            const int t = RPB * b + s;  // stream position
            int y = dir >= 0 ? first_in + t : s1e + K - 1 - t;
            y = y > last_in ? last_in : (y < first_in ? first_in : y);
            const int64_t d = CONTIG ? 0 : (y < 0 ? top_d : (y >= R ? bot_d : 0));
            const char *g = mid_b + (d + (int64_t)y * pitch_b) + lane_off;
            __builtin_amdgcn_global_load_lds(reinterpret_cast<const void *>(g), slot + s * ROW, 16, 0, GOL_BAND_LOAD_AUX);
        }
    };

    if (!has_rows) return;  // whole workgroup (no barrier after this point)
    if (threadIdx.x < P) { ready_[threadIdx.x] = 0; consumed_[threadIdx.x] = 0; }
    if constexpr (PLACE) {
        if (lane == 0) place_[threadIdx.x >> 6] = (int)((__builtin_amdgcn_s_getreg((31 << 11) | 4) >> 4) & 3u);
        if (threadIdx.x == 0) {
            const uint32_t idx = cu_slot_index();
            place_[P] = a.cu_slots ? claim_cu_slot(a.cu_slots + idx) : -1;
            place_[P + 1] = (int)idx;
        }
    }
    __syncthreads();
    if constexpr (PLACE) {
        const int q = place_[P];
        const int m = (1 << place_[0]) | (1 << place_[1]) | (1 << place_[2]) | (1 << place_[3]);
        if (q >= 0 && m == 0xF) wv = __builtin_amdgcn_readfirstlane((place_[threadIdx.x >> 6] + q) & 3);
    }
    lds_u32 *const ring_l = (lds_u32 *)&ring_[0][0][0][0];
    lds_u32 *const in_l = (lds_u32 *)&in_ring[0][0][0];
    lds_u32 *const ready_l = (lds_u32 *)&ready_[0];
    lds_u32 *const consumed_l = (lds_u32 *)&consumed_[0];
    constexpr int SLOT = RPB * ROW;  // uint32 per slot (one block)

    PairState<DW> st[KW];
#pragma unroll
    for (int g = 0; g < KW; ++g)
#pragma unroll
        for (int j = 0; j < DW; ++j) { st[g].a0[j] = 0; st[g].a1[j] = 0; st[g].b0[j] = 0; st[g].b1[j] = 0; st[g].cb[j] = 0; }
    uint32_t alive = 0;
    const uint32_t st_mask = writer ? 0xFFFFFFFFu : 0u;
    int seen_ready = 0, seen_free = 0;  // cached flag values (ring wv ready, ring wv+1 consumed)
    const uint32_t nrows = (uint32_t)(s1 - s0);
    // One loop per role (0 = loader, 1 = middle, 2 = last), unrolled over the NS ring slots so
    // every LDS address is a per-lane register plus an immediate offset and every wait count is
    // a constant.  Per block b (LDS operations of a wave complete in order):
    //  * wait for block b's two rows (read at the end of block b-1, the wave's youngest LDS
    //    operations: lgkmcnt(0), which also completes block b-1's row writes);
    //  * readers: write "block b consumed"; writers: publish "blocks < b ready";
    //  * compute the pair through the wave's KW stages;
    //  * writers: make sure slot b % NS is free, write the two rows; the last wave stores them
    //    to HBM;
    //  * readers: make sure block b+1 is published; the loader instead refills block b-2's slot
    //    with block b+2 (global_load_lds) and waits (vmcnt) for block b+1's; read block b+1's rows;
    //  * the block count is padded to a multiple of NS: padding blocks read clamped rows and
    //    their stores fall outside the strip's buffer range.
    //  (Reading the next rows before the compute instead holds 8 more VGPRs across it: the kernel
    //  then spills at 128.)
    const int nblkT = (nblk + NS - 1) / NS * NS;
    constexpr int SB = SLOT * 4, RB = ROW * 4;  // slot and row strides in bytes
    lds_u32 *const scratch = (lds_u32 *)&flag_scratch[0] + lane;
    lds_u32 *const rdy_addr = lane == 0 ? ready_l + wv + 1 : scratch;  // writer: ring wv+1 ready
    lds_u32 *const cns_addr = lane == 0 ? consumed_l + wv : scratch;   // reader: ring wv consumed
    lds_u32 *const in_base = in_l + lane * 4;
    lds_u32 *const rd_base = ring_l + (wv - 1) * NS * SLOT + lane * 4;  // ring wv (wv >= 1)
    lds_u32 *const wr_base = ring_l + wv * NS * SLOT + lane * 4;        // ring wv+1 (wv < P-1)
    auto unpack = [&](const v4u32 v, uint32_t (&cur)[DW]) { cur[0] = v.x; cur[1] = v.y; cur[2] = v.z; cur[3] = v.w; };
    auto pack = [&](const uint32_t (&cur)[DW]) { return v4u32{cur[0], cur[1], cur[2], cur[3]}; };
    // last wave: output row y = s0 + 2b + S - 2K, stored at voffset lane_off + (y - s0) * pitch
    // of a buffer spanning the strip's rows: rows before s0 (negative offsets, as unsigned
    // >= 2^32 - 2K * pitch) and from s1 on fall outside it, and so does a halo lane's 2^31.
    const __amdgpu_buffer_rsrc_t strip_rs = __builtin_amdgcn_make_buffer_rsrc(
        dst_b + (int64_t)s0 * pitch_b, (short)0, (int)(nrows * (uint32_t)pitch_b), 0x00020000);
    // (walking up, dir -1: output row y = s1e - 1 + 2K - 2b - S, offsets decreasing)
    // (readfirstlane: the compiler otherwise keeps this uniform row index in a VGPR and compares it
    // with a vector compare per row)
    int rrel = __builtin_amdgcn_readfirstlane(dir >= 0 ? -2 * K : s1e - 1 + 2 * K - s0);  // output row - s0
    const int rstep = dir >= 0 ? 1 : -1;
    uint32_t voff = st_off + (uint32_t)rrel * (uint32_t)pitch_b;
    const uint32_t vstep = (uint32_t)rstep * (uint32_t)pitch_b;
    // a row's cells onto the count: one accumulating v_bcnt per word, as one asm statement (the
    // compiler turns the same chain in C into bcnt pairs + v_add3).  Plain VALU reading VALU
    // results: no wait states inside (tools/check_lds_wait.py checks the pipeline kernels' asm for
    // the VALU hazards the compiler cannot see).
    auto count_row = [&](const uint32_t (&cur)[DW]) {
        uint32_t c = 0;
        asm("v_bcnt_u32_b32 %0, %1, 0\n\tv_bcnt_u32_b32 %0, %2, %0\n\tv_bcnt_u32_b32 %0, %3, %0\n\t"
            "v_bcnt_u32_b32 %0, %4, %0"
            : "=&v"(c)
            : "v"(cur[0]), "v"(cur[1]), "v"(cur[2]), "v"(cur[3]));
        return c;
    };
    auto count_rows2 = [&](const uint32_t (&x0)[DW], const uint32_t (&x1)[DW]) {
        asm("v_bcnt_u32_b32 %0, %1, %0\n\tv_bcnt_u32_b32 %0, %2, %0\n\tv_bcnt_u32_b32 %0, %3, %0\n\t"
            "v_bcnt_u32_b32 %0, %4, %0\n\tv_bcnt_u32_b32 %0, %5, %0\n\tv_bcnt_u32_b32 %0, %6, %0\n\t"
            "v_bcnt_u32_b32 %0, %7, %0\n\tv_bcnt_u32_b32 %0, %8, %0"
            : "+v"(alive)
            : "v"(x0[0]), "v"(x0[1]), "v"(x0[2]), "v"(x0[3]), "v"(x1[0]), "v"(x1[1]), "v"(x1[2]), "v"(x1[3]));
    };
    // the block's two output rows to HBM, and the fused count of the rows this strip stores (halo
    // lanes are masked once at the end): one v_bcnt chain of 8 words onto the count, and a block at
    // a strip's end (a row outside it: a uniform branch) takes the count of that row off again.
    // (Round 5's per-row select cost 15 VALU per block instead of 8: the count in bcnt pairs +
    // v_add3, a vector compare and a select per row.)
    auto emit2 = [&](const uint32_t (&x0)[DW], const uint32_t (&x1)[DW]) {
        __builtin_amdgcn_raw_buffer_store_b128(pack(x0), strip_rs, voff, 0, GOL_BAND_STORE_AUX);
        __builtin_amdgcn_raw_buffer_store_b128(pack(x1), strip_rs, voff + vstep, 0, GOL_BAND_STORE_AUX);
        if constexpr (COUNT) {
            count_rows2(x0, x1);
            const bool in0 = (uint32_t)rrel < nrows, in1 = (uint32_t)(rrel + rstep) < nrows;  // wave-uniform
            if (!(in0 && in1)) alive -= (in0 ? 0u : count_row(x0)) + (in1 ? 0u : count_row(x1));
        }
        voff += 2 * vstep;
        rrel += 2 * rstep;
    };
    lds_u32 *const src_base = wv == 0 ? in_base : rd_base;
    // paired: the loader's claims, NS blocks (one loop trip) each, one in flight (issued at a
    // trip's first block, used at the next trip's start); the first before block 0's loads
    constexpr int FINAL = 1 << 30;  // ready flag = FINAL + blocks: the stream has ended
    // (lane 0 claims; the kernels are built without the atomic optimizer, which broadcast the
    // claim's return at once and so waited for it right there: an atomic round trip per trip)
    uint32_t pending = 0;
    if (wv == 0 && dir && lane == 0) pending = atomicAdd(ctr, (uint32_t)NS);
    // block 0's rows, read to completion here (the compiler copies the loop-carried registers
    // on loop entry, which must not happen while a read is in flight)
    constexpr int PF = GOL_BAND_PREFETCH;
    static_assert(PF >= 2 && PF <= NS, "blocks b+1 .. b+PF in flight in NS slots");
    if (wv == 0) {
        stage_in(0, in_l);
        stage_in(1, in_l + SLOT);
        if constexpr (PF > 2) stage_in(2, in_l + (2 % NS) * SLOT);
        if constexpr (PF > 3) stage_in(3, in_l + (3 % NS) * SLOT);
        asm volatile("s_waitcnt vmcnt(%0)" ::"n"(RPB * (PF - 1)) : "memory");  // block 0 (and the claim)
    } else if (seen_ready < 1) {
        seen_ready = spin_until_ge(ready_l + wv, 1);
        if (seen_ready < 0) {
            raise_error(a.err, GOLK_ERR_SPIN);
            return;
        }
    }
    v4u32 nx0 = lds_rd128_issue_o<0>(src_base);
    v4u32 nx1 = lds_rd128_issue_o<RB>(src_base);
    lds_wait_n<0>(nx0);
    lds_wait_n<0>(nx1);
    // readers: the block the loop is about to run exists (an empty paired stream ends at once)
    bool more = !(seen_ready >= FINAL && seen_ready - FINAL == 0);
    auto step = [&](int b, auto u_c, auto role_c, auto dyn_c, auto skip_c) -> bool {
        constexpr int US = decltype(u_c)::value;
        constexpr int ROLE = decltype(role_c)::value;
        constexpr bool DYN = decltype(dyn_c)::value;
        constexpr bool SKIP = decltype(skip_c)::value;  // a fill block: no rule (see run)
        constexpr bool LAST = ROLE == 2;
        constexpr int NXT = (US + 1) % NS;
        uint32_t r0[DW], r1[DW];
        // block b's rows, the youngest LDS operations of this wave: once they are in, so are
        // block b-1's row writes, and both flags can go out at once
        lds_settle2(nx0, nx1);
        unpack(nx0, r0);
        unpack(nx1, r1);
        if constexpr (ROLE == 1) lds_flag_wr2(cns_addr, b + 1, rdy_addr, b);
        else if constexpr (ROLE != 0) lds_flag_wr(cns_addr, b + 1);  // block b's slot is free
        else lds_flag_wr(rdy_addr, b);          // blocks < b are in ring wv+1
        if constexpr (ROLE == 0) {
            if (wrap) {
#pragma unroll
                for (int j = 0; j < DW; ++j) {
                    r0[j] = __builtin_amdgcn_alignbit(r0[j], r0[j], rot);
                    r1[j] = __builtin_amdgcn_alignbit(r1[j], r1[j], rot);
                }
            }
        }
        if constexpr (!SKIP) {
#pragma unroll
            for (int g = 0; g < KW; ++g) pstage<DW>(st[g], r0, r1);
        }
        if constexpr (LAST) {
            emit2(r0, r1);
        } else {
            if (seen_free < b + 1 - NS) {  // slot b % NS: block b - NS consumed
                seen_free = spin_until_ge(consumed_l + wv + 1, b + 1 - NS);
                if (seen_free < 0) return false;
            }
            lds_wr128x2_o<US * SB, US * SB + RB>(wr_base, pack(r0), pack(r1));
        }
        // block b+1's rows: read now, waited for at the next block's start (the compute of the
        // other waves of the SIMD covers the LDS latency)
        if constexpr (ROLE == 0) {
            stage_in(b + PF, in_l + ((US + PF) % NS) * SLOT);  // refills block b+PF-NS's slot (clamped past the end)
            // block b+1 landed, b+2 .. b+PF in flight (and, paired, at US 1 the claim issued at US 0)
            asm volatile("s_waitcnt vmcnt(%0)" ::"n"(RPB * (PF - 1) + (DYN && US == 1 ? 1 : 0)) : "memory");
            if constexpr (DYN && US == 0) {
                if (lane == 0) pending = atomicAdd(ctr, (uint32_t)NS);
            }
        } else {
            // the next block exists unless the writer's flag says the stream ended before it
            if (seen_ready < b + 2) {
                seen_ready = spin_until_ge(ready_l + wv, b + 2);
                if (seen_ready < 0) return false;
            }
            more = seen_ready < FINAL || b + 1 < seen_ready - FINAL;
        }
        lds_rd128x2_issue_o<NXT * SB, NXT * SB + RB>(src_base, nx0, nx1);  // (past the stream's end: a stale slot, unused)
        return true;
    };
    // blocks the loader has: nblkT, or (paired) the claims granted so far
    auto grant = [&](uint32_t c) { return c >= (uint32_t)nclaim ? 0 : NS; };
    auto trip = [&](int b, auto role_c, auto dyn_c, auto skip_c) -> bool {
        return step(b, std::integral_constant<int, 0>(), role_c, dyn_c, skip_c) &&
               step(b + 1, std::integral_constant<int, 1>(), role_c, dyn_c, skip_c) &&
               step(b + 2, std::integral_constant<int, 2>(), role_c, dyn_c, skip_c) &&
               step(b + 3, std::integral_constant<int, 3>(), role_c, dyn_c, skip_c);
    };
    static_assert(NS == 4, "trip() runs NS steps");
    auto run = [&](auto role_c, auto dyn_c) -> bool {
        constexpr int ROLE = decltype(role_c)::value;
        constexpr bool DYN = decltype(dyn_c)::value;
        int nb = DYN ? 0 : nblkT;
        int b = 0;
        // Fill blocks: stage g's input is valid from stream step 2g on, and a stage whose state
        // missed the steps before S emits garbage only up to step S + 1, which no later stage uses
        // if S <= 2g (stage g's outputs are read from step 2g + 2 on; the last stage's rows before
        // step 2K fall outside the strip).  A wave whose first stage is g0 = KW * wv therefore
        // passes the blocks before step 2 g0 (2b + 1 < 2 g0: b < g0) on without the rule -- whole
        // loop trips of them, in a loop of their own (a branch per block inside the main loop made
        // the compiler spill).
        if constexpr (ROLE != 0) {
            const int nskip = KW * wv;
            for (; b + NS <= nskip; b += NS) {
                if (!more) break;
                if (!trip(b, role_c, dyn_c, std::true_type())) return false;
            }
        }
        for (;; b += NS) {
            if constexpr (ROLE == 0) {
                if constexpr (DYN) nb += grant(__builtin_amdgcn_readfirstlane(pending));
                if (b >= nb) break;
            } else {
                if (!more) break;
            }
            if (!trip(b, role_c, dyn_c, std::false_type())) return false;
        }
        // the last block's reads of the next slot are still in flight: land them before their
        // registers are used for anything else
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        if constexpr (ROLE != 2) {
            asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
            lds_flag_wr(rdy_addr, FINAL + b);
        }
        if constexpr (ROLE == 0 && DYN) {
            if (lane == 0 && atomicAdd(ctr + 1, 1u) == 1u) {  // both loaders' claims are over
                atomicExch(ctr, 0u);
                atomicExch(ctr + 1, 0u);
            }
        }
        return true;
    };
    // (paired or not changes only the loader's loop: the readers' loops are one instantiation,
    // 65 -> 44 KB of code per kernel; measured equal, same box: weak -0.5 %, 262144^2 +0.8 %,
    // 65536^2 -0.6 %, profiles/r05/r05b_ab_dedupe_bytes.jsonl)
    auto run_role = [&](auto role_c) -> bool {
        if constexpr (decltype(role_c)::value != 0) return run(role_c, std::false_type());
        else return dir ? run(role_c, std::true_type()) : run(role_c, std::false_type());
    };
    bool ok;
    if (wv == 0) ok = run_role(std::integral_constant<int, 0>());
    else if (wv == P - 1) ok = run_role(std::integral_constant<int, 2>());
    else ok = run_role(std::integral_constant<int, 1>());
    if (!ok) raise_error(a.err, GOLK_ERR_SPIN);
    alive &= st_mask;  // halo lanes' rows are not this group's
    if (wv == 0) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    if (COUNT && wv == P - 1) slot_add(a.slots, alive);
    if constexpr (PLACE) {  // the last wave of the pipeline frees the workgroup's CU slot
        if (wv == P - 1 && lane == 0 && place_[P] >= 0) atomicAnd(a.cu_slots + place_[P + 1], ~(1u << place_[P]));
    }
}

}  // namespace golk

// band_pipe_kernel's instantiations, their host stubs and launch, under the max-ILP machine
// scheduler (Makefile BANDFLAGS).
// The scheduler choice is per translation unit, and it is a per-kernel one: same box, 2 reps,
// max-ILP ran the band boards 1.0-1.9 % faster (weak 148.3 vs 146.8, 262144^2 151.5 vs 148.9,
// 65536^2 139.8 vs 137.2) and the byte pipeline 4.5 % slower (56.8 vs 59.4);
// profiles/r04/r04h_sched.jsonl.
using namespace golk;
const void *golk_band_pipe_fn(bool contig, bool count)
{
    constexpr int KW = GOL_BAND_KW, P = GOL_BAND_P;
    return contig ? (count ? (const void *)band_pipe_kernel<KW, P, true, true> : (const void *)band_pipe_kernel<KW, P, true, false>)
                  : (count ? (const void *)band_pipe_kernel<KW, P, false, true> : (const void *)band_pipe_kernel<KW, P, false, false>);
}
hipError_t golk_band_pipe_launch(bool contig, bool count, unsigned nwg, const BitsArgs &a, hipStream_t s)
{
    void *args[] = {const_cast<BitsArgs *>(&a)};  // the kernel's one parameter, by value
    (void)hipLaunchKernel(golk_band_pipe_fn(contig, count), dim3(nwg), dim3(64 * GOL_BAND_P), args, 0, s);
    return hipGetLastError();
}
