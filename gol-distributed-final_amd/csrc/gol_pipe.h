// gol_pipe.h -- what only the two pipeline kernels share (band_pipe_kernel, gol_band_pipe.hip;
// bytes_pipe_kernel, gol_bytes_pipe.hip): the inline-asm LDS accesses, the bounded flag wait,
// the loaders' interior-block arithmetic and the pair step.  Device code: included by .hip
// units only.
#pragma once
#include "gol_step_device.h"

namespace golk {

// ------------------------------------------------------------------ LDS helpers of the pipelines
// LDS accesses of the pipelines are inline asm: the compiler treats a global_load_lds in
// flight as a pending LDS write and would put vmcnt(0) before every LDS access it can see
// (which, on the storing wave, also waits for its HBM stores).
typedef __attribute__((address_space(3))) uint32_t lds_u32;
// ceil(a / d) for a >= 0 (else 0) and floor(a / d) for any a (d > 0)
__device__ __forceinline__ int div_ceil_nn(int a, int d) { return a > 0 ? (a + d - 1) / d : 0; }
__device__ __forceinline__ int div_floor(int a, int d) { return a >= 0 ? a / d : -((-a + d - 1) / d); }
typedef __attribute__((ext_vector_type(4))) uint32_t v4u32;
// Wait for a read with N younger LDS operations allowed in flight (LDS operations of a wave
// complete in order, and these kernels issue no scalar loads in the loop; the assembly check
// tools/check_lds_wait.py confirms the latter).  The value is an in-out operand, so every
// use of it is ordered after the wait.
template <int N>
__device__ __forceinline__ void lds_wait_n(v4u32 &r)
{
    if constexpr (N == 0) asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(r)::"memory");
    else asm volatile("s_waitcnt lgkmcnt(1)" : "+v"(r)::"memory");
}

// Wait until `r` (an issued read) has landed, N younger LDS operations left in flight: at a loop
// back edge, so that the compiler's copies of the loop-carried register read the landed value.
template <int N>
__device__ __forceinline__ void lds_settle(v4u32 &r) { asm volatile("s_waitcnt lgkmcnt(%1)" : "+v"(r) : "i"(N) : "memory"); }
// Immediate-offset forms (byte offsets < 64 KiB): ring slots and rows at compile-time offsets
// from one per-lane address register.
template <int OFF>
__device__ __forceinline__ v4u32 lds_rd128_issue_o(const lds_u32 *p)
{
    v4u32 r;
    asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(r) : "v"(p), "i"(OFF) : "memory");
    return r;
}
template <int OFF>
__device__ __forceinline__ void lds_wr32_o(lds_u32 *p, uint32_t v)
{
    asm volatile("ds_write_b32 %0, %1 offset:%2" ::"v"(p), "v"(v), "i"(OFF) : "memory");
}
template <int OFF>
__device__ __forceinline__ uint32_t lds_rd32_issue_o(const lds_u32 *p)
{
    uint32_t r;
    asm volatile("ds_read_b32 %0, %1 offset:%2" : "=v"(r) : "v"(p), "i"(OFF) : "memory");
    return r;
}
// Two-instruction forms (one asm statement: one conservative hazard s_nop after it, not two):
// the band pipeline's block reads, writes, settle and middle-wave flags through these measured
// weak 163.3 -> 165.2 TCUPS, 262144^2 +0.2 % (same box, profiles/r05/r05g_ab_lds_pairs.jsonl).
template <int OFF0, int OFF1>
__device__ __forceinline__ void lds_rd128x2_issue_o(const lds_u32 *p, v4u32 &a, v4u32 &b)
{
    asm volatile("ds_read_b128 %0, %2 offset:%3\n\tds_read_b128 %1, %2 offset:%4" : "=&v"(a), "=&v"(b) : "v"(p), "i"(OFF0), "i"(OFF1) : "memory");
}
template <int OFF0, int OFF1>
__device__ __forceinline__ void lds_wr128x2_o(lds_u32 *p, v4u32 a, v4u32 b)
{
    asm volatile("ds_write_b128 %0, %1 offset:%3\n\tds_write_b128 %0, %2 offset:%4" ::"v"(p), "v"(a), "v"(b), "i"(OFF0), "i"(OFF1) : "memory");
}
__device__ __forceinline__ void lds_settle2(v4u32 &a, v4u32 &b) { asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(a), "+v"(b)::"memory"); }
__device__ __forceinline__ void lds_flag_wr2(lds_u32 *p, int v, lds_u32 *q, int w)
{
    asm volatile("ds_write_b32 %0, %1\n\tds_write_b32 %2, %3" ::"v"(p), "v"(v), "v"(q), "v"(w) : "memory");
}
// Flag write without an exec mask: lane 0's address is the flag, the other lanes write their
// own scratch word (one ds_write, no saveexec / branch around it).
__device__ __forceinline__ void lds_flag_wr(lds_u32 *p, int v) { asm volatile("ds_write_b32 %0, %1" ::"v"(p), "v"(v) : "memory"); }
__device__ __forceinline__ int lds_rd32(const lds_u32 *p)
{
    int r;
    asm volatile("ds_read_b32 %0, %1\n\ts_waitcnt lgkmcnt(0)" : "=v"(r) : "v"(p) : "memory");
    return r;
}
// Wait until flag f >= v; returns the value seen (callers cache it: a producer is usually
// several blocks ahead, so most blocks need no flag read), or -1 after GOL_SPIN_LIMIT polls.
// A wave that sees -1 leaves its loop, every wave waiting on it times out the same way, and
// each records GOLK_ERR_SPIN in the launch's error word on its way out (once, after the loop:
// an atomic inside the loop costs the pipeline registers), so the host reports the launch as
// failed (GOL_EHIP) instead of returning a board with unwritten strips.
// YIELD (the byte pipeline, whose waves run at priority 1): the polling wave drops to priority 0,
// so the computing waves of its SIMD win the issue arbitration (+1.5 % on 16384^2 bytes; the band
// pipeline measured 0 / -1 %, same box).
template <bool YIELD = false>
__device__ __forceinline__ int spin_until_ge(const lds_u32 *f, int v)
{
    if constexpr (YIELD) __builtin_amdgcn_s_setprio(0);
#pragma clang loop unroll(disable)
    for (int n = 0; n < GOL_SPIN_LIMIT; ++n) {
        const int x = __builtin_amdgcn_readfirstlane(lds_rd32(f));
        if (x >= v) {
            if constexpr (YIELD) __builtin_amdgcn_s_setprio(1);
            return x;
        }
        __builtin_amdgcn_s_sleep(YIELD ? GOL_BYTES_SPIN_SLEEP : GOL_SPIN_SLEEP);
    }
    if constexpr (YIELD) __builtin_amdgcn_s_setprio(1);
    return -1;
}

// ------------------------------------------------------------------ band layout, split pipeline
// Pair step of one stage.  The stage's input stream x_0, x_1, ... arrives in
// pairs (x_2m, x_2m+1) = (r0, r1); its state holds the horizontal 3-sums of x_2m-2 (a) and
// x_2m-1 (b) and the cells of x_2m-1 (cb).  It emits the next state of rows 2m-1 and 2m in
// place of r0, r1 (one row of delay per stage, as a row-by-row stage) and moves its state on by
// two rows.  The two outputs share the sum of their common rows P = b + c = p0 + 2 p1 + 4 p2
// (c = x_2m's 3-sums; 4 gates), then each takes a 4-gate tail over (P, the third row's sums, its
// cell) found by exhaustive search (tools/rule_search_pair.c; tests/test_rule_circuit_cpu.py
// checks it on every 4 x 3 neighbourhood): with the 2 gates of each row's horizontal sum a
// generation is 8 ops per 32 cells instead of 9.  The tail relies on the cell's row being one of
// the pair (the pair sum of a live cell is >= 1, of a dead one <= 5), which holds for both outputs.
__device__ __forceinline__ uint32_t pair_tail(uint32_t p0, uint32_t p1, uint32_t p2, uint32_t x0, uint32_t x1,
                                              uint32_t cell)
{
    const uint32_t g1 = bitop3<TT_PG1>(p0, x0, cell);
    const uint32_t g2 = bitop3<TT_PG2>(p1, p2, x1);
    const uint32_t g3 = bitop3<TT_PG3>(p2, cell, g1);
    return bitop3<TT_POUT>(g3, g1, g2);
}
template <int DW>
struct PairState {
    uint32_t a0[DW], a1[DW], b0[DW], b1[DW], cb[DW];
};
template <int DW>
__device__ __forceinline__ void pstage(PairState<DW> &s, uint32_t (&r0)[DW], uint32_t (&r1)[DW])
{
    // word by word, so that few temporaries are live at once (the pipeline holds 5 KW DW state
    // registers beside this); the outputs go to o0 / o1 because a word's 3-sums need its
    // neighbour words' old values.  (Writing the lane's edge words first -- the next stage's DPP
    // moves read them, and a DPP move right after the VALU op that wrote its source waits on an
    // s_nop -- cut the s_nops per trip from 43 to 15 and measured equal, same box.)
    const uint32_t l0 = from_lower_lane(r0[DW - 1]), u0 = from_upper_lane(r0[0]);
    const uint32_t l1 = from_lower_lane(r1[DW - 1]), u1 = from_upper_lane(r1[0]);
    uint32_t o0[DW], o1[DW];
#pragma unroll
    for (int j = 0; j < DW; ++j) {
        const uint32_t x0 = r0[j], x1 = r1[j];
        const uint32_t w0 = j == 0 ? l0 : r0[j - 1], w1 = j == 0 ? l1 : r1[j - 1];
        const uint32_t n0 = j == DW - 1 ? u0 : r0[j + 1], n1 = j == DW - 1 ? u1 : r1[j + 1];
        const uint32_t c0 = bitop3<TT_XOR3>(w0, x0, n0), c1 = bitop3<TT_MAJ>(w0, x0, n0);
        const uint32_t d0 = bitop3<TT_XOR3>(w1, x1, n1), d1 = bitop3<TT_MAJ>(w1, x1, n1);
        const uint32_t k = s.b0[j] & c0;
        const uint32_t p0 = s.b0[j] ^ c0;
        const uint32_t p1 = bitop3<TT_XOR3>(s.b1[j], c1, k);
        const uint32_t p2 = bitop3<TT_MAJ>(s.b1[j], c1, k);
        o0[j] = pair_tail(p0, p1, p2, s.a0[j], s.a1[j], s.cb[j]);  // row 2m-1: above = x_2m-2
        o1[j] = pair_tail(p0, p1, p2, d0, d1, x0);                 // row 2m: below = x_2m+1
        s.a0[j] = c0;
        s.a1[j] = c1;
        s.b0[j] = d0;
        s.b1[j] = d1;
        s.cb[j] = x1;
    }
#pragma unroll
    for (int j = 0; j < DW; ++j) {
        r0[j] = o0[j];
        r1[j] = o1[j];
    }
}

}  // namespace golk
