// gol_step_device.h -- the step kernels' machinery, for the units that hold them (gol_kernels.hip;
// gol_band_pipe.hip and gol_bytes_pipe.hip through gol_pipe.h) and the micro-benchmarks of
// tools/ubench: the pipeline build knobs, word loads and stores, the register-pipeline state with
// the band stage, the byte packing, the argument blocks of the step and pipeline kernels and the
// pipeline units' entry points.  The lane helpers under it are
// gol_device.h.  Device code: included by .hip units only.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gol_device.h"
#include "gol_strips.h"

// Polls of a pipeline flag before a wave gives up (sets GOLK_ERR_SPIN in the launch's error
// word and leaves; the host turns that into GOL_EHIP).  A test build sets 0 to force the path.
#ifndef GOL_SPIN_LIMIT
#define GOL_SPIN_LIMIT (1 << 22)
#endif
// s_sleep argument between two polls of a pipeline flag (units of 64 shader cycles): 0 (the
// poll's own LDS round trip paces it) measured +1 % on 65536^2, +0.3 % on 16384^2 bytes, equal on
// the weak board, over 1; 2 was slower (same box, tools/ab.py)
#ifndef GOL_BYTES_SPIN_SLEEP
#define GOL_BYTES_SPIN_SLEEP 0  // (the byte pipeline's polls, spin_until_ge<true>)
#endif
#ifndef GOL_SPIN_SLEEP
#define GOL_SPIN_SLEEP 0
#endif
// Role placement of the band pipeline (gol_band_pipe.hip, band_pipe_kernel); its launcher hands
// the kernel the CU slot masks only when it is on.
#ifndef GOL_BAND_PLACE
#define GOL_BAND_PLACE 1
#endif

namespace golk {

template <int DW> struct VecT;
template <> struct VecT<1> { typedef uint32_t type; };
template <> struct VecT<2> { typedef uint2 type; };
template <> struct VecT<4> { typedef uint4 type; };

template <int DW>
__device__ __forceinline__ void load_words(const uint32_t *p, uint32_t (&w)[DW])
{
    typedef typename VecT<DW>::type V;
    V v = *reinterpret_cast<const V *>(p);
    if constexpr (DW == 1) { w[0] = v; }
    if constexpr (DW == 2) { w[0] = v.x; w[1] = v.y; }
    if constexpr (DW == 4) { w[0] = v.x; w[1] = v.y; w[2] = v.z; w[3] = v.w; }
}
template <int DW>
__device__ __forceinline__ void store_words(uint32_t *p, const uint32_t (&w)[DW])
{
    typedef typename VecT<DW>::type V;
    V v;
    if constexpr (DW == 1) { v = w[0]; }
    if constexpr (DW == 2) { v.x = w[0]; v.y = w[1]; }
    if constexpr (DW == 4) { v.x = w[0]; v.y = w[1]; v.z = w[2]; v.w = w[3]; }
    *reinterpret_cast<V *>(p) = v;
}

// ------------------------------------------------------------------ register pipeline
// State of stage g (generation g+1): a ring of 3 rows of horizontal sums plus the cells of
// those rows.  Slot s = step % 3 holds the row received at this step; the stage emits the
// next state of the row received one step ago.
template <int K, int DW>
struct Pipe {
    uint32_t h0[K][3][DW];
    uint32_t h1[K][3][DW];
    uint32_t cc[K][3][DW];
};

template <int K, int DW>
__device__ __forceinline__ void pipe_init(Pipe<K, DW> &p)
{
#pragma unroll
    for (int g = 0; g < K; ++g)
#pragma unroll
        for (int s = 0; s < 3; ++s)
#pragma unroll
            for (int j = 0; j < DW; ++j) { p.h0[g][s][j] = 0; p.h1[g][s][j] = 0; p.cc[g][s][j] = 0; }
}

// ------------------------------------------------------------------ band-layout bit board
// Column-band layout: a row is Wd = W/32 words and bit b of word w is cell x = b*Wd + w (32
// bands of Wd columns, one per bit).  The horizontal neighbours of a cell are the SAME bit
// of the neighbouring words, so a generation is pure bitwise logic: no v_alignbit (which
// issues at half the rate of v_bitop3 on gfx950) and the centre cell is the
// word itself.  The column torus wraps band b's last column onto band b+1's first:
// band-space column c = q*Wd + r reads word r rotated right by q (one v_alignbit per word
// per LOAD, only in the waves that straddle the wrap).  Cost: the horizontal halo is k words
// (k columns) instead of one 32-cell word, so a wave of 64 lanes x DW words keeps
// 64 - 2*ceil(k/DW) lanes of output.
template <int DW>
__device__ __forceinline__ void hsum_band(const uint32_t (&c)[DW], uint32_t (&h0)[DW], uint32_t (&h1)[DW])
{
    const uint32_t left_in = from_lower_lane(c[DW - 1]);
    const uint32_t right_in = from_upper_lane(c[0]);
#pragma unroll
    for (int j = 0; j < DW; ++j) {
        const uint32_t L = (j == 0) ? left_in : c[j - 1];
        const uint32_t R = (j == DW - 1) ? right_in : c[j + 1];
        h0[j] = bitop3<TT_XOR3>(L, c[j], R);
        h1[j] = bitop3<TT_MAJ>(L, c[j], R);
    }
}

// The rule written op by op across the DW words (each op has DW-1 independent neighbours):
// per word the 8 ops form a dependent chain, and one wave issues a dependent VALU op ~1.7x
// slower than an independent one (MI355X_MICROARCH.md, constants table).
template <int K, int DW, int S>
__device__ __forceinline__ void bstage(Pipe<K, DW> &p, const int g, uint32_t (&cur)[DW])
{
    constexpr int SA = (S + 1) % 3, SM = (S + 2) % 3;
#pragma unroll
    for (int j = 0; j < DW; ++j) p.cc[g][S][j] = cur[j];
    hsum_band<DW>(p.cc[g][S], p.h0[g][S], p.h1[g][S]);
    const uint32_t (&a0)[DW] = p.h0[g][SA], (&a1)[DW] = p.h1[g][SA];
    const uint32_t (&b0)[DW] = p.h0[g][SM], (&b1)[DW] = p.h1[g][SM];
    const uint32_t (&c0)[DW] = p.h0[g][S], (&c1)[DW] = p.h1[g][S];
    uint32_t t0[DW], k0[DW], u[DW], v[DW], e1[DW], e2[DW];
#pragma unroll
    for (int j = 0; j < DW; ++j) k0[j] = bitop3<TT_MAJ>(a0[j], b0[j], c0[j]);
#pragma unroll
    for (int j = 0; j < DW; ++j) u[j] = bitop3<TT_XOR3>(a1[j], b1[j], c1[j]);
#pragma unroll
    for (int j = 0; j < DW; ++j) v[j] = bitop3<TT_MAJ>(a1[j], b1[j], c1[j]);
#pragma unroll
    for (int j = 0; j < DW; ++j) t0[j] = bitop3<TT_XOR3>(a0[j], b0[j], c0[j]);
#pragma unroll
    for (int j = 0; j < DW; ++j) e1[j] = bitop3<TT_G1>(t0[j], k0[j], v[j]);
#pragma unroll
    for (int j = 0; j < DW; ++j) e2[j] = bitop3<TT_G2>(u[j], v[j], e1[j]);
#pragma unroll
    for (int j = 0; j < DW; ++j) cur[j] = bitop3<TT_OUT>(t0[j], p.cc[g][SM][j], e2[j]);
}

// StripMap, work_item, work_dir, pair_extent: gol_strips.h (shared with the host)

struct BitsArgs {
    const uint32_t *top, *mid, *bot;
    uint32_t *dst;
    int64_t R, Wd, pitch, row0, rows;
    int32_t strip, ngroups;
    uint64_t *slots;
    uint32_t *err;
    uint32_t *cu_slots;  // band pipeline: per-CU masks of the workgroup slots in use (GOL_CU_SLOT_WORDS)
    StripMap sm;
};

// ------------------------------------------------------------------ byte rows <-> 32-cell words
// 32 bytes of a row -> one word (bit i = byte i & 1)
__device__ __forceinline__ uint32_t pack32(const uint4 lo, const uint4 hi)
{
    const uint32_t d[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
    uint32_t b[4];
#pragma unroll
    for (int q = 0; q < 4; ++q)  // byte q of the word = cells 8q..8q+7
        b[q] = __builtin_amdgcn_udot4(d[2 * q] & 0x01010101u, 0x08040201u,
                                      __builtin_amdgcn_udot4(d[2 * q + 1] & 0x01010101u, 0x80402010u, 0u, false),
                                      false);
    return b[0] | (b[1] << 8) | (b[2] << 16) | (b[3] << 24);
}
// Same for bytes that are exactly 0x00 or 0xFF (-1 as int8): weights -2^i give +2^i per set byte.
// (Builtins, not inline asm: a v_dot4 result read by another VALU needs 3 wait states, which the
// compiler's hazard recognizer inserts only for instructions it can see.  The inline-asm VOP3P
// form measured +1.5 % and then +-0 on another box, and under the post-RA scheduler it read
// stale sums: profiles/r05/r05y_ab_bytes_sched.jsonl.)
__device__ __forceinline__ uint32_t pack32_ff(const uint4 lo, const uint4 hi)
{
    const uint32_t d[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
    uint32_t b[4];
#pragma unroll
    for (int q = 0; q < 4; ++q)
        b[q] = (uint32_t)__builtin_amdgcn_sdot4((int)d[2 * q], (int)0xF8FCFEFFu,
                                               __builtin_amdgcn_sdot4((int)d[2 * q + 1], (int)0x80C0E0F0u, 0, false), false);
    return b[0] | (b[1] << 8) | (b[2] << 16) | (b[3] << 24);
}

__device__ __forceinline__ void unpack32(const uint32_t w, uint4 &lo, uint4 &hi)
{
    uint32_t o[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) {
        const uint32_t n = (w >> (4 * q)) & 0xFu;
        const uint32_t sp = __umul24(n, 0x00204081u) & 0x01010101u;  // bit i -> byte i
        o[q] = (sp << 8) - sp;                                       // 0x01 -> 0xFF
    }
    lo = make_uint4(o[0], o[1], o[2], o[3]);
    hi = make_uint4(o[4], o[5], o[6], o[7]);
}

struct BytesKArgs {
    const uint8_t *top, *mid, *bot;
    uint8_t *dst;
    int64_t R, Wd, pitch, row0, rows;  // Wd = W / 32 words, pitch in bytes
    int32_t strip, ngroups;
    uint64_t *slots;
    uint32_t *err;
    StripMap sm;
};

// Byte rows of one lane: 32 bytes = two 16-byte loads, packed to a word at use.
struct Raw32 {
    uint4 lo, hi;
};

}  // namespace golk

// The pipeline kernels live in translation units of their own (gol_band_pipe.hip,
// gol_bytes_pipe.hip: each under its own machine scheduler, Makefile).  _launch: nwg workgroups of
// the kernel golk_*_pipe_fn names (gol_step_kernels.h) on stream s.
hipError_t golk_band_pipe_launch(bool contig, bool count, unsigned nwg, const golk::BitsArgs &a, hipStream_t s);
hipError_t golk_bytes_pipe_launch(bool count, unsigned nwg, const golk::BytesKArgs &a, hipStream_t s);
