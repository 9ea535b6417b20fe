// old_stages.h -- stages and LDS helpers of pipeline shapes the product dropped in rounds 2-5, kept
// beside the micro-benchmarks that still time them (pipe_compute, pipe_map, byte_stage): the
// 3-row one-word wavefront (sstage_wave3 / sstage_waves3), the word-by-word band stage
// (bstage_seq) and the blocking, unindexed or single-write LDS accesses.  No product kernel calls any of them.
#pragma once
#include <utility>

#include "gol_pipe.h"

namespace golk {

// Step W of a 3-row wavefront over K shifted-frame stages, one word per lane: row r (ring slot
// r) is at stage W - r.  The three rows' stages are independent within a step, and each op is
// written for all active rows before the next (a one-word stage is a dependent chain of 13
// ops; row after row, the compiler kept the chains apart and one wave issued at the
// dependent-op latency).
template <int K, int NSTG, int W>
__device__ __forceinline__ void sstage_wave3(Pipe<K, 1> &p, uint32_t (&c)[3])
{
    static_assert(NSTG <= K, "stages of the pipe state");
    constexpr bool on[3] = {W < NSTG, W >= 1 && W - 1 < NSTG, W >= 2 && W - 2 < NSTG};
    constexpr int g[3] = {on[0] ? W : 0, on[1] ? W - 1 : 0, on[2] ? W - 2 : 0};
    uint32_t wl[3], L1[3], L2[3], t0[3], k0[3], u[3], v[3], e1[3], e2[3];
#pragma unroll
    for (int r = 0; r < 3; ++r) if (on[r]) wl[r] = from_lower_lane(c[r]);
#pragma unroll
    for (int r = 0; r < 3; ++r) if (on[r]) L1[r] = __builtin_amdgcn_alignbit(c[r], wl[r], 31);
#pragma unroll
    for (int r = 0; r < 3; ++r) if (on[r]) L2[r] = __builtin_amdgcn_alignbit(c[r], wl[r], 30);
#pragma unroll
    for (int r = 0; r < 3; ++r) if (on[r]) p.h0[g[r]][r][0] = bitop3<TT_XOR3>(L1[r], c[r], L2[r]);
#pragma unroll
    for (int r = 0; r < 3; ++r) if (on[r]) p.h1[g[r]][r][0] = bitop3<TT_MAJ>(L1[r], c[r], L2[r]);
#pragma unroll
    for (int r = 0; r < 3; ++r) if (on[r]) p.cc[g[r]][r][0] = L1[r];
#define GOL_ROWS3(expr) _Pragma("unroll") for (int r = 0; r < 3; ++r) if (on[r]) { const int A = (r + 1) % 3, M = (r + 2) % 3; (void)A; (void)M; expr; }
    GOL_ROWS3(k0[r] = bitop3<TT_MAJ>(p.h0[g[r]][A][0], p.h0[g[r]][M][0], p.h0[g[r]][r][0]))
    GOL_ROWS3(u[r] = bitop3<TT_XOR3>(p.h1[g[r]][A][0], p.h1[g[r]][M][0], p.h1[g[r]][r][0]))
    GOL_ROWS3(v[r] = bitop3<TT_MAJ>(p.h1[g[r]][A][0], p.h1[g[r]][M][0], p.h1[g[r]][r][0]))
    GOL_ROWS3(t0[r] = bitop3<TT_XOR3>(p.h0[g[r]][A][0], p.h0[g[r]][M][0], p.h0[g[r]][r][0]))
    GOL_ROWS3(e1[r] = bitop3<TT_G1>(t0[r], k0[r], v[r]))
    GOL_ROWS3(e2[r] = bitop3<TT_G2>(u[r], v[r], e1[r]))
    GOL_ROWS3(c[r] = bitop3<TT_OUT>(t0[r], p.cc[g[r]][M][0], e2[r]))
#undef GOL_ROWS3
}
// All NSTG stages of one 3-row block (steps 0 .. NSTG + 1).
template <int K, int NSTG, int... W>
__device__ __forceinline__ void sstage_waves3(Pipe<K, 1> &p, uint32_t (&c)[3], std::integer_sequence<int, W...>)
{
    (sstage_wave3<K, NSTG, W>(p, c), ...);
}

// Same stage with the rule evaluated word by word (fewer live temporaries than bstage; at
// 4 waves per SIMD a dependent op issues as fast as an independent one).
template <int K, int DW, int S>
__device__ __forceinline__ void bstage_seq(Pipe<K, DW> &p, const int g, uint32_t (&cur)[DW])
{
    constexpr int SA = (S + 1) % 3, SM = (S + 2) % 3;
#pragma unroll
    for (int j = 0; j < DW; ++j) p.cc[g][S][j] = cur[j];
    hsum_band<DW>(p.cc[g][S], p.h0[g][S], p.h1[g][S]);
#pragma unroll
    for (int j = 0; j < DW; ++j)
        cur[j] = rule(p.h0[g][SA][j], p.h1[g][SA][j], p.h0[g][SM][j], p.h1[g][SM][j], p.h0[g][S][j],
                      p.h1[g][S][j], p.cc[g][SM][j]);
}

__device__ __forceinline__ v4u32 lds_rd128(const lds_u32 *p)
{
    v4u32 r;
    asm volatile("ds_read_b128 %0, %1\n\ts_waitcnt lgkmcnt(0)" : "=v"(r) : "v"(p) : "memory");
    return r;
}
__device__ __forceinline__ void lds_wait1() { asm volatile("s_waitcnt lgkmcnt(1)" ::: "memory"); }
template <int OFF>
__device__ __forceinline__ void lds_wr128_o(lds_u32 *p, v4u32 v)
{
    asm volatile("ds_write_b128 %0, %1 offset:%2" ::"v"(p), "v"(v), "i"(OFF) : "memory");
}
__device__ __forceinline__ void lds_wr32(lds_u32 *p, int v) { asm volatile("ds_write_b32 %0, %1" ::"v"(p), "v"(v) : "memory"); }
// Rows S = 0, 1, 2 of one ring slot (ROW = 64 uint32 apart), read and waited for together (the
// byte pipeline's 3-row blocks, dropped with commit 2a68ef7; byte_stage.hip still times them).
__device__ __forceinline__ void lds_rd32x3(const lds_u32 *p, uint32_t (&r)[3])
{
    asm volatile(
        "ds_read_b32 %0, %3\n\t"
        "ds_read_b32 %1, %3 offset:256\n\t"
        "ds_read_b32 %2, %3 offset:512\n\t"
        "s_waitcnt lgkmcnt(0)"
        : "=&v"(r[0]), "=&v"(r[1]), "=&v"(r[2])
        : "v"(p)
        : "memory");
}

}  // namespace golk
