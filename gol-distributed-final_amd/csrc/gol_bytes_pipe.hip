// gol_bytes_pipe.hip -- the byte board's split pipeline (k = 32 per launch): bytes_pipe_kernel and
// its launch, in a translation unit of its own so that it is compiled under the machine
// scheduler that runs it fastest (Makefile BYTEFLAGS).
#include <type_traits>

#include "gol_pipe.h"
#include "gol_step_kernels.h"

namespace golk {

// f(integral_constant<0>), .., f(integral_constant<N-1>), unrolled
template <int N, int I = 0, typename F>
__device__ __forceinline__ void static_for(F &&f)
{
    if constexpr (I < N) {
        f(std::integral_constant<int, I>());
        static_for<N, I + 1>(f);
    }
}

// Byte board, split pipeline: K = KW * P turns per launch, P waves per workgroup on one
// column group of 62 words (32 cells per lane, standard bit layout in registers, shifted
// frame), KW stages per wave, blocks of 4 rows (two pair steps, as band_pipe_kernel's, run as a
// wavefront: the second pair one stage behind the first, two independent pair steps in flight
// per stage step -- one 32-cell word per lane is otherwise one dependent chain) handed on
// through LDS rings of NS slots (256 B per row) with band_pipe_kernel's flag protocol and loop
// shape: one loop per role, unrolled over the NS slots (every LDS address a register plus an
// immediate, no slot arithmetic, no per-block branch for the fill blocks).  Wave 0 stages its
// input blocks HBM -> LDS with global_load_lds and packs 32 bytes per lane into one word with
// v_dot4_i32_i8; wave P-1 realigns (after 32 stages the frame shift is exactly one word),
// unpacks through a 2 KiB LDS table (byte -> 8 bytes of 0x00 / 0xFF) and stores the strip
// through one buffer descriptor with a running offset.  One 32-cell word per lane covers K <= 32
// columns of halo, so K = 32 costs no more lanes than K = 16.
// (Round 4's form -- 3-row blocks, one block per loop trip with running slot indices and a
// per-block fill branch -- spent 0.44 scalar instructions per VALU: DESIGN.md §4.4.)
//
// Shifted-frame pair step: pstage's circuit on this frame.  A row's 3-sum at bit p is
// c[p] + c[p-1] + c[p-2] (centred on p-1: the neighbour from the lower lane by one DPP, two
// v_alignbit), the cell is c[p-1]; every stage moves the frame one bit to the left.
__device__ __forceinline__ void spstage(PairState<1> &s, uint32_t &r0, uint32_t &r1)
{
    const uint32_t w0 = from_lower_lane(r0), w1 = from_lower_lane(r1);
    const uint32_t l0 = __builtin_amdgcn_alignbit(r0, w0, 31), m0 = __builtin_amdgcn_alignbit(r0, w0, 30);
    const uint32_t l1 = __builtin_amdgcn_alignbit(r1, w1, 31), m1 = __builtin_amdgcn_alignbit(r1, w1, 30);
    const uint32_t c0 = bitop3<TT_XOR3>(l0, r0, m0), c1 = bitop3<TT_MAJ>(l0, r0, m0);
    const uint32_t d0 = bitop3<TT_XOR3>(l1, r1, m1), d1 = bitop3<TT_MAJ>(l1, r1, m1);
    const uint32_t k = s.b0[0] & c0;
    const uint32_t p0 = s.b0[0] ^ c0;
    const uint32_t p1 = bitop3<TT_XOR3>(s.b1[0], c1, k);
    const uint32_t p2 = bitop3<TT_MAJ>(s.b1[0], c1, k);
    r0 = pair_tail(p0, p1, p2, s.a0[0], s.a1[0], s.cb[0]);  // row 2m-1: its cell = c[p-1] of x_2m-1
    r1 = pair_tail(p0, p1, p2, d0, d1, l0);                 // row 2m: its cell = c[p-1] of x_2m
    s.a0[0] = c0;
    s.a1[0] = c1;
    s.b0[0] = d0;
    s.b1[0] = d1;
    s.cb[0] = l1;
}

// (Ring slots of the byte pipeline, GOL_BYTES_NS / _NSI, and GOL_BYTES_PER_CU: gol_strips.h.)
// Cache policy bits of the byte pipeline's output stores (0: default)
#ifndef GOL_BYTES_STORE_AUX
#define GOL_BYTES_STORE_AUX 0
#endif
template <int KW, int P, bool COUNT>
__global__ void __launch_bounds__(64 * P) __attribute__((amdgpu_waves_per_eu(6, 8))) bytes_pipe_kernel(BytesKArgs a)
{
    constexpr int K = KW * P;
    static_assert(K <= 32, "one 32-cell halo word per side");
    constexpr int RPB = GOL_BYTES_RPB;  // rows per block: two pair steps
    static_assert(RPB == 4, "a block is two pair steps");
    constexpr int NS = GOL_BYTES_NS;  // (the loops below are unrolled over the NS slots)
    constexpr int NSI = GOL_BYTES_NSI;
    static_assert(NS % NSI == 0 && NSI >= 3, "input slots: 2 blocks in flight, one being read");
    constexpr int ROW = 64;  // uint32 per ring row
    __shared__ uint32_t ring[P - 1][NS][RPB][ROW];
    __shared__ uint32_t in_ring[NSI][RPB][2][256];  // byte rows: [half][lane][16 bytes]
    __shared__ uint2 lut[256];
    __shared__ int ready[P], consumed[P];
    __shared__ int flag_scratch[64];  // dummy target of lanes 1..63's flag writes (lds_flag_wr; never read)

    const int lane = threadIdx.x & 63;
    const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    int group, s0, s1, rotv;
    if (!work_item(a.sm, a.ngroups, a.row0, a.rows, a.strip, blockIdx.x, [] { return gridDim.x; }, group, s0, s1, rotv)) return;
    uint32_t *ctr;
    const int dir = work_dir(a.sm, blockIdx.x, ctr);  // 0: static strip, +1 / -1: paired
    const int64_t col_raw = (int64_t)group * 62 + (lane - 1);
    const int64_t col = ((col_raw % a.Wd) + a.Wd) % a.Wd;
    const bool writer = lane >= 1 && lane <= 62 && col_raw < a.Wd;
    const int R = (int)a.R;
    const int first_in = s0 - K, last_in = s1 + K - 1;
    const int nblk = ((s1 - s0) + 2 * K + RPB - 1) / RPB;
    // a pair's range, stretched to s1e so that TRIP divides its len + 4K (rows past s1 are read
    // clamped and never stored: they only feed outputs past s1); nclaim: blocks of the pair, a
    // multiple of NS (gol_strips.h: the expressions the host's pair_extent evaluates)
    constexpr int TRIP = RPB * NS;  // rows per loop trip
    const int s1e = GOL_PAIR_S1E(dir, s0, s1, K, TRIP);
    const int nclaim = GOL_PAIR_NCLAIM(s0, s1e, K, RPB);
    const int pitch = (int)a.pitch;
    const char *mid_b = reinterpret_cast<const char *>(a.mid);
    const int64_t top_d = (reinterpret_cast<const char *>(a.top) - mid_b) + (int64_t)K * pitch;
    const int64_t bot_d = (reinterpret_cast<const char *>(a.bot) - mid_b) - (int64_t)R * pitch;
    const uint32_t lane_off = (uint32_t)(col * 32);
    char *dst_b = reinterpret_cast<char *>(a.dst);
    const uint32_t st_off = writer ? lane_off : 0x80000000u;
    const uint32_t st_mask = writer ? 0xFFFFFFFFu : 0u;

    // stream position t -> input row (walking up, dir -1: from s1e + K - 1)
    auto in_row = [&](int t) { return dir >= 0 ? first_in + t : s1e + K - 1 - t; };
    // wave 0: block b -> an in_ring slot (the slot is an argument: a lambda that captures a
    // __shared__ array loses the kernel's host-side stub).  Interior blocks (both rows inside the
    // shard and inside [first_in, last_in]: every block but the first and last few of a strip) take
    // one row address, carried from block to block and stepped by a pitch; the others clamp and
    // pick the row's segment per row (round 4: +2.4 % on 16384^2 bytes over per-row addresses).
    // The slot is an LDS-typed pointer (a generic one costs a null check per load: 4 SALU) and the
    // interior blocks are one range [ib_lo, ib_lo + ib_n) of block numbers, found here once.  (The
    // load's immediate offset moves its LDS destination too: the second 16 bytes of a lane's 32
    // take their own address.)
    const int in_lo = max(first_in, 0), in_hi = min(last_in, R - 1);
    const int64_t row_step = dir >= 0 ? (int64_t)pitch : -(int64_t)pitch;
    const int y_first = in_row(0);
    const int ib_lo = dir >= 0 ? div_ceil_nn(in_lo - y_first, RPB) : div_ceil_nn(y_first - in_hi, RPB);
    const int ib_hi = dir >= 0 ? div_floor(in_hi - (RPB - 1) - y_first, RPB) : div_floor(y_first - (RPB - 1) - in_lo, RPB);
    const uint32_t ib_n = ib_hi >= ib_lo ? (uint32_t)(ib_hi - ib_lo + 1) : 0u;
    const char *st_u = mid_b + (int64_t)y_first * pitch;  // the next block's first row (wave-uniform)
    constexpr int IROW = 2 * 256;  // uint32 per input row in LDS (two 16-byte halves of 64 lanes)
    auto stage_in = [&](int b, lds_u32 *slot) {
        const char *gu = st_u;
        st_u += RPB * row_step;
        if ((uint32_t)(b - ib_lo) < ib_n) {
            // The block's 8 LDS-DMA loads in the SGPR-base form, as the band loader's (row address
            // in an SGPR pair, the lane's 32-bit offset -- and +16 for a row's second half -- in a
            // VGPR; M0 set and restored inside, a wait state before each load): the builtin made
            // the compiler compute a 64-bit VGPR address per load.  Same box, 3 reps: 16384^2
            // bytes 63.0 -> 63.7 TCUPS (profiles/r06/r06_ab_bsaddr.jsonl).
            static_assert(RPB == 4, "four rows per block");
            // row bases, wave-uniform: readfirstlane makes that explicit for builds whose control
            // flow hides it (GOL_SPIN_LIMIT=0: the "s" operands below would get VGPRs); it folds
            // away where the compiler already keeps them in SGPRs
            auto uni = [](const char *q) {
                const uint64_t v = reinterpret_cast<uint64_t>(q);
                const uint64_t lo = (uint32_t)__builtin_amdgcn_readfirstlane((uint32_t)v);
                const uint64_t hi = (uint32_t)__builtin_amdgcn_readfirstlane((uint32_t)(v >> 32));
                return reinterpret_cast<const char *>(lo | (hi << 32));
            };
            const char *r0 = uni(gu), *r1 = uni(r0 + row_step), *r2 = uni(r1 + row_step), *r3 = uni(r2 + row_step);
            uint32_t keep;
            asm volatile("s_nop 4\n\ts_mov_b32 %0, m0\n\t"
                         "s_mov_b32 m0, %3\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %7\n\t"
                         "s_add_u32 m0, %3, 0x400\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %2, %7\n\t"
                         "s_mov_b32 m0, %4\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %8\n\t"
                         "s_add_u32 m0, %4, 0x400\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %2, %8\n\t"
                         "s_mov_b32 m0, %5\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %9\n\t"
                         "s_add_u32 m0, %5, 0x400\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %2, %9\n\t"
                         "s_mov_b32 m0, %6\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %10\n\t"
                         "s_add_u32 m0, %6, 0x400\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %2, %10\n\t"
                         "s_mov_b32 m0, %0"
                         : "=&s"(keep)
                         : "v"(lane_off), "v"(lane_off + 16u), "s"(slot), "s"(slot + IROW), "s"(slot + 2 * IROW),
                           "s"(slot + 3 * IROW), "s"(r0), "s"(r1), "s"(r2), "s"(r3)
                         : "memory", "scc");
            return;
        }
#pragma unroll
        for (int S = 0; S < RPB; ++S) {
            int y = in_row(RPB * b + S);
            y = y > last_in ? last_in : (y < first_in ? first_in : y);  // past the end: clamped, never stored
            const int64_t d = y < 0 ? top_d : (y >= R ? bot_d : 0);
            const char *gg = mid_b + (d + (int64_t)y * pitch) + lane_off;
            __builtin_amdgcn_global_load_lds(reinterpret_cast<const void *>(gg), slot + S * IROW, 16, 0, 0);
            __builtin_amdgcn_global_load_lds(reinterpret_cast<const void *>(gg + 16), slot + S * IROW + 256, 16, 0, 0);
        }
    };
    __builtin_amdgcn_s_setprio(1);  // polls drop to 0 (spin_until_ge<true>)
    for (int i = threadIdx.x; i < 256; i += 64 * P) {
        uint32_t o[2];
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const uint32_t sp = __umul24((i >> (4 * h)) & 0xF, 0x00204081u) & 0x01010101u;
            o[h] = (sp << 8) - sp;
        }
        lut[i] = make_uint2(o[0], o[1]);
    }
    if (threadIdx.x < P) { ready[threadIdx.x] = 0; consumed[threadIdx.x] = 0; }
    __syncthreads();
    lds_u32 *const ring_l = (lds_u32 *)&ring[0][0][0][0];
    lds_u32 *const in_l = (lds_u32 *)&in_ring[0][0][0][0];
    lds_u32 *const ready_l = (lds_u32 *)&ready[0];
    lds_u32 *const consumed_l = (lds_u32 *)&consumed[0];
    constexpr int SLOT = RPB * ROW;        // uint32 per hand-off slot
    constexpr int ISLOT = RPB * 2 * 256;   // uint32 per input slot
    constexpr int SB = SLOT * 4, RB = ROW * 4, ISB = ISLOT * 4;
    lds_u32 *const scratch = (lds_u32 *)&flag_scratch[0] + lane;
    lds_u32 *const rdy_addr = lane == 0 ? ready_l + wv + 1 : scratch;  // ring wv+1 ready
    lds_u32 *const cns_addr = lane == 0 ? consumed_l + wv : scratch;   // ring wv consumed
    lds_u32 *const in_base = in_l + lane * 4;
    lds_u32 *const rd_base = ring_l + (wv - 1) * NS * SLOT + lane;  // ring wv (wv >= 1)
    lds_u32 *const wr_base = ring_l + wv * NS * SLOT + lane;        // ring wv+1 (wv < P-1)

    PairState<1> st[KW];
#pragma unroll
    for (int g = 0; g < KW; ++g) { st[g].a0[0] = 0; st[g].a1[0] = 0; st[g].b0[0] = 0; st[g].b1[0] = 0; st[g].cb[0] = 0; }
    uint32_t alive = 0;
    const uint32_t nrows = (uint32_t)(s1 - s0);
    // last wave: output row y stored at voffset st_off + (y - s0) * pitch of ONE buffer spanning
    // the strip's rows (the host keeps rows x pitch < 2^31): rows before s0 (negative offsets, as
    // unsigned >= 2^32 - 2K * pitch), from s1 on, and a halo lane's 2^31 fall outside it
    const __amdgpu_buffer_rsrc_t strip_rs = __builtin_amdgcn_make_buffer_rsrc(
        dst_b + (int64_t)s0 * pitch, (short)0, (int)(nrows * (uint32_t)pitch), 0x00020000);
    int rrel = dir >= 0 ? -2 * K : s1e - 1 + 2 * K - s0;  // output row - s0 of the next row (wave-uniform)
    const int rstep = dir >= 0 ? 1 : -1;
    uint32_t voff = st_off + (uint32_t)rrel * (uint32_t)pitch;
    const uint32_t vstep = (uint32_t)rstep * (uint32_t)pitch;
    // undo the K-bit frame shift (K = 32: exactly the next lane's word; alignbit takes its shift
    // mod 32), unpack through the LUT, store, count
    auto emit = [&](uint32_t w) {
        const uint32_t nxw = from_upper_lane(w);
        const uint32_t o = K % 32 ? __builtin_amdgcn_alignbit(nxw, w, K % 32) : nxw;
        uint2 e[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) e[q] = lut[(o >> (8 * q)) & 0xFF];
        __builtin_amdgcn_raw_buffer_store_b128(v4u32{e[0].x, e[0].y, e[1].x, e[1].y}, strip_rs, voff, 0, GOL_BYTES_STORE_AUX);
        __builtin_amdgcn_raw_buffer_store_b128(v4u32{e[2].x, e[2].y, e[3].x, e[3].y}, strip_rs, voff + 16u, 0, GOL_BYTES_STORE_AUX);
        if constexpr (COUNT) {
            const uint32_t c = __popc(o) + alive;
            alive = (uint32_t)rrel < nrows ? c : alive;
        }
        voff += vstep;
        rrel += rstep;
    };
    constexpr int FINAL = 1 << 30;  // ready flag = FINAL + blocks: the stream has ended
    uint32_t pending = 0;  // the loader's claim in flight (paired)
    if (wv == 0 && dir && lane == 0) pending = atomicAdd(ctr, (uint32_t)NS);
    // block 0's rows read to completion here (the compiler copies loop-carried registers on loop
    // entry, which must not happen while a read is in flight).  A reader's next block (RPB words)
    // is read at the end of a block; the loader reads its block's 2 RPB 16-byte halves at the
    // block's start (32 VGPRs held across the compute would spill at 6 waves per SIMD).
    v4u32 nb[2 * RPB];  // loader
    uint32_t nw[RPB];   // readers
    int seen_ready = 0, seen_free = 0;
    auto read_in = [&](auto off_c) {  // the loader's reads of one input slot
        constexpr int OFF = decltype(off_c)::value;
        static_assert(RPB == 4, "eight half-row reads");
        nb[0] = lds_rd128_issue_o<OFF>(in_base);
        nb[1] = lds_rd128_issue_o<OFF + 1024>(in_base);
        nb[2] = lds_rd128_issue_o<OFF + 2048>(in_base);
        nb[3] = lds_rd128_issue_o<OFF + 3072>(in_base);
        nb[4] = lds_rd128_issue_o<OFF + 4096>(in_base);
        nb[5] = lds_rd128_issue_o<OFF + 5120>(in_base);
        nb[6] = lds_rd128_issue_o<OFF + 6144>(in_base);
        nb[7] = lds_rd128_issue_o<OFF + 7168>(in_base);
    };
    auto read_ring = [&](auto off_c) {  // a reader's reads of one ring slot
        constexpr int OFF = decltype(off_c)::value;
        static_assert(RPB == 4, "four row reads");
        nw[0] = lds_rd32_issue_o<OFF>(rd_base);
        nw[1] = lds_rd32_issue_o<OFF + 256>(rd_base);
        nw[2] = lds_rd32_issue_o<OFF + 512>(rd_base);
        nw[3] = lds_rd32_issue_o<OFF + 768>(rd_base);
    };
    auto settle_in = [&]() {
#pragma unroll
        for (int h = 0; h < 2 * RPB; ++h) lds_settle<0>(nb[h]);
    };
    if (wv == 0) {
        stage_in(0, in_l);
        stage_in(1, in_l + ISLOT);
        asm volatile("s_waitcnt vmcnt(%0)" ::"n"(2 * RPB) : "memory");  // block 0 landed (the claim before it too)
#pragma unroll
        for (int S = 0; S < RPB; ++S) nw[S] = 0;
    } else {
        seen_ready = spin_until_ge<true>(ready_l + wv, 1);
        if (seen_ready < 0) {
            raise_error(a.err, GOLK_ERR_SPIN);
            return;
        }
        read_ring(std::integral_constant<int, 0>());
        asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(nw[0]), "+v"(nw[1]), "+v"(nw[2]), "+v"(nw[3])::"memory");
    }
    bool more = !(seen_ready >= FINAL && seen_ready - FINAL == 0);
    // Fill blocks (band_pipe_kernel's rule): a wave whose first stage is g0 = KW * wv passes the
    // blocks that end before step 2 g0 (RPB b + RPB <= 2 g0) on without the rule -- a uniform
    // branch per block here (the byte pipeline has registers to spare; a loop of its own per role
    // doubled the role's code)
    const int nskip = 2 * KW * wv / RPB;
    auto step = [&](int b, auto u_c, auto role_c, auto dyn_c) -> bool {
        constexpr int US = decltype(u_c)::value;
        constexpr int ROLE = decltype(role_c)::value;
        constexpr bool DYN = decltype(dyn_c)::value;
        constexpr bool LAST = ROLE == 2;
        constexpr int NXT = (US + 1) % NS;
        uint32_t r[RPB];
        // block b's rows, the youngest LDS operations of this wave: once they are in, so are
        // block b-1's row writes, and both flags can go out at once
        if constexpr (ROLE == 0) {
            read_in(std::integral_constant<int, US % NSI * ISB>());
            settle_in();
#pragma unroll
            for (int S = 0; S < RPB; ++S)
                r[S] = pack32_ff(uint4{nb[2 * S].x, nb[2 * S].y, nb[2 * S].z, nb[2 * S].w},
                                 uint4{nb[2 * S + 1].x, nb[2 * S + 1].y, nb[2 * S + 1].z, nb[2 * S + 1].w});
        } else {
            asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(nw[0]), "+v"(nw[1]), "+v"(nw[2]), "+v"(nw[3])::"memory");
#pragma unroll
            for (int S = 0; S < RPB; ++S) r[S] = nw[S];
            lds_flag_wr(cns_addr, b + 1);  // block b's slot is free
        }
        if constexpr (!LAST) lds_flag_wr(rdy_addr, b);  // blocks < b are in ring wv+1
        if (ROLE == 0 || b >= nskip) {
            // stage step w: the first pair at stage w, the second at stage w-1 (each stage takes
            // its pairs in stream order)
#pragma unroll
            for (int w = 0; w <= KW; ++w) {
                if (w < KW) spstage(st[w], r[0], r[1]);
                if (w >= 1) spstage(st[w - 1], r[2], r[3]);
            }
        }
        if constexpr (LAST) {
#pragma unroll
            for (int S = 0; S < RPB; ++S) emit(r[S]);
        } else {
            if (seen_free < b + 1 - NS) {  // slot b % NS: block b - NS consumed
                seen_free = spin_until_ge<true>(consumed_l + wv + 1, b + 1 - NS);
                if (seen_free < 0) return false;
            }
            static_assert(RPB == 4, "four row writes");
            lds_wr32_o<US * SB>(wr_base, r[0]);
            lds_wr32_o<US * SB + RB>(wr_base, r[1]);
            lds_wr32_o<US * SB + 2 * RB>(wr_base, r[2]);
            lds_wr32_o<US * SB + 3 * RB>(wr_base, r[3]);
        }
        // block b+1's rows: read now, waited for at the next block's start
        if constexpr (ROLE == 0) {
            stage_in(b + 2, in_l + ((US + 2) % NSI) * ISLOT);  // refills block b+2-NSI's slot (clamped past the end)
            // block b+1 landed, b+2 in flight (2 RPB loads; and, paired, at US 1 the claim issued at US 0)
            if constexpr (DYN && US == 1) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(2 * RPB + 1) : "memory");
            else asm volatile("s_waitcnt vmcnt(%0)" ::"n"(2 * RPB) : "memory");
            if constexpr (DYN && US == 0) {
                if (lane == 0) pending = atomicAdd(ctr, (uint32_t)NS);
            }
        } else {
            // the next block exists unless the writer's flag says the stream ended before it
            if (seen_ready < b + 2) {
                seen_ready = spin_until_ge<true>(ready_l + wv, b + 2);
                if (seen_ready < 0) return false;
            }
            more = seen_ready < FINAL || b + 1 < seen_ready - FINAL;
            read_ring(std::integral_constant<int, NXT * SB>());
        }
        return true;
    };
    auto grant = [&](uint32_t c) { return c >= (uint32_t)nclaim ? 0 : NS; };

    auto trip = [&](int b, auto role_c, auto dyn_c) -> bool {
        bool ok = true;
        static_for<NS>([&](auto u_c) {
            if (ok) ok = step(b + decltype(u_c)::value, u_c, role_c, dyn_c);
        });
        return ok;
    };
    auto run = [&](auto role_c, auto dyn_c) -> bool {
        constexpr int ROLE = decltype(role_c)::value;
        constexpr bool DYN = decltype(dyn_c)::value;
        int nb = DYN ? 0 : (nblk + NS - 1) / NS * NS;
        int b = 0;
        for (;; b += NS) {
            if constexpr (ROLE == 0) {
                if constexpr (DYN) nb += grant(__builtin_amdgcn_readfirstlane(pending));
                if (b >= nb) break;
            } else {
                if (!more) break;
            }
            if (!trip(b, role_c, dyn_c)) return false;
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // the last block's reads of the next slot
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
    // which halves their code -- the I-cache holds 64 KiB for two CUs)
    auto run_role = [&](auto role_c) -> bool {
        if constexpr (decltype(role_c)::value != 0) return run(role_c, std::false_type());
        else return dir ? run(role_c, std::true_type()) : run(role_c, std::false_type());
    };
    bool ok;
    if (wv == 0) ok = run_role(std::integral_constant<int, 0>());
    else if (wv == P - 1) ok = run_role(std::integral_constant<int, 2>());
    else ok = run_role(std::integral_constant<int, 1>());
    if (wv == 0) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // input blocks staged past the end
    if (!ok) raise_error(a.err, GOLK_ERR_SPIN);
    alive &= st_mask;  // halo lanes' rows are not this group's
    if (COUNT && wv == P - 1) slot_add(a.slots, alive);
}

}  // namespace golk

// bytes_pipe_kernel's instantiations and launch, under the max-memory-clause machine scheduler,
// bottom-up, and no post-RA scheduler (Makefile BYTEFLAGS).  Same box, 3 reps each: 59.4 -> 60.4
// TCUPS on 16384^2 bytes, then 60.2 -> 60.6 without the post-RA pass, 60.7 -> 61.2 bottom-up; under
// max-ILP (the band pipeline's) 56.8 (profiles/r04/r04h_sched.jsonl).
using namespace golk;
const void *golk_bytes_pipe_fn(bool count)
{
    constexpr int KW = GOL_BYTES_PIPE_KW, P = GOL_BYTES_PIPE_P;
    return count ? (const void *)bytes_pipe_kernel<KW, P, true> : (const void *)bytes_pipe_kernel<KW, P, false>;
}
hipError_t golk_bytes_pipe_launch(bool count, unsigned nwg, const BytesKArgs &a, hipStream_t s)
{
    void *args[] = {const_cast<BytesKArgs *>(&a)};  // the kernel's one parameter, by value
    (void)hipLaunchKernel(golk_bytes_pipe_fn(count), dim3(nwg), dim3(64 * GOL_BYTES_PIPE_P), args, 0, s);
    return hipGetLastError();
}
