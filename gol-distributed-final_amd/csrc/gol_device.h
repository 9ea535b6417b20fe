// gol_device.h -- the lane and wave helpers any kernel unit may use (the step units through
// gol_step_device.h, gol_util.hip, the batch's units and the micro-benchmarks of tools/ubench): the
// v_bitop3 truth tables, the DPP lane moves, splitmix64, the wave sum, the count slots' add, the
// error word's raise and the B3/S23 rule on seven gates (the step kernels' and the batch's).  No
// launcher and no strip map: of the project's headers it includes gol_launch.h alone, for
// GOL_COUNT_SLOTS.  Device code: included by .hip units only.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gol_launch.h"

namespace golk {

// ------------------------------------------------------------------ helpers
// v_bitop3_b32 truth tables: operand 0 -> 0xF0, operand 1 -> 0xCC, operand 2 -> 0xAA.
constexpr unsigned TT_XOR3 = 0x96;  // a ^ b ^ c
constexpr unsigned TT_MAJ = 0xE8;   // majority(a, b, c)
// The rule tail (tools/rule_search.c, tests/test_rule_circuit_cpu.py): with T = t0 + 2(k0 + u +
// 2v) the 3x3 sum including the cell, alive' = (T == 3) | (cell & T == 4)
//   = (t0 | cell) & ~G2,  G2 = TT_G2(u, v, G1),  G1 = TT_G1(t0, k0, v)  (exactly one of t0, k0, v).
// Three gates instead of the four of t0 ? [S == 1] : cell & [S == 2]: an exhaustive search over
// 3-gate circuits finds them only when it may use that the centre row's horizontal sum includes
// the cell (a centre sum of 0 means a dead cell, 3 a live one), which holds in every kernel here.
// Polarity (here and in the pair tails): every gate answers 0 on a dead neighbourhood, so that no
// nearly all-ones word sits between the nearly all-zero ones of a settled board; the complements
// live in the tables of the gates that read them (tools/rule_search_pair.c --hist
// ranks the choice, tests/test_tail_polarity_cpu.py holds it).
constexpr unsigned TT_G1 = 0x16;    // exactly one of a, b, c
constexpr unsigned TT_G2 = 0xD6;    // (a & b) | exactly one of a, b, c
constexpr unsigned TT_OUT = 0x54;   // (a | b) & ~c

// The pair step's tails (gol_pipe.h pair_tail; tools/rule_search_pair.c)
constexpr unsigned TT_PG1 = 0xBC;   // (p0, x0, cell)
constexpr unsigned TT_PG2 = 0xDA;   // (p1, p2, x1)
constexpr unsigned TT_PG3 = 0xE4;   // (p2, cell, g1)
constexpr unsigned TT_POUT = 0x18;  // (g3, g1, g2)

template <unsigned TT>
__device__ __forceinline__ uint32_t bitop3(uint32_t a, uint32_t b, uint32_t c)
{
    return __builtin_amdgcn_bitop3_b32(a, b, c, TT);
}
// lane i receives lane i-1's value (lane 0 receives 0)
__device__ __forceinline__ uint32_t from_lower_lane(uint32_t v)
{
    return __builtin_amdgcn_mov_dpp(v, 0x138 /* wave_shr:1 */, 0xf, 0xf, true);
}
// lane i receives lane i+1's value (lane 63 receives 0)
__device__ __forceinline__ uint32_t from_upper_lane(uint32_t v)
{
    return __builtin_amdgcn_mov_dpp(v, 0x130 /* wave_shl:1 */, 0xf, 0xf, true);
}

__device__ __forceinline__ uint64_t splitmix64(uint64_t x)
{
    uint64_t z = x + 0x9E3779B97F4A7C15ULL;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
    return z ^ (z >> 31);
}

__device__ __forceinline__ uint64_t wave_sum_u64(uint64_t v)
{
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

// One atomic per wave into one of GOL_COUNT_SLOTS slots (64 B apart).
__device__ __forceinline__ void slot_add(uint64_t *slots, uint64_t v)
{
    v = wave_sum_u64(v);
    if ((threadIdx.x & 63) == 0 && v) {
        unsigned wave = (blockIdx.x + blockIdx.y * gridDim.x) * (blockDim.x >> 6) + (threadIdx.x >> 6);
        atomicAdd((unsigned long long *)&slots[(wave % GOL_COUNT_SLOTS) * 8], (unsigned long long)v);
    }
}

// Error word of a launch: flags ORed by lane 0 of a failing wave (a vector global atomic).
__device__ __forceinline__ void raise_error(uint32_t *err, uint32_t flag)
{
    if ((threadIdx.x & 63) == 0) atomicOr(err, flag);
}

// B3/S23 from three horizontal sums (rows above/middle/below, value = h0 + 2*h1 in 0..3 per
// cell; the middle one includes the cell) and the middle cell.  T = sum of the 3x3 block
// including the cell = t0 + 2*(k0 + u + 2v); alive' = (T == 3) | (cell & T == 4): 7 gates.
__device__ __forceinline__ uint32_t rule(uint32_t a0, uint32_t a1, uint32_t b0, uint32_t b1,
                                         uint32_t c0, uint32_t c1, uint32_t cell)
{
    const uint32_t t0 = bitop3<TT_XOR3>(a0, b0, c0);
    const uint32_t k0 = bitop3<TT_MAJ>(a0, b0, c0);
    const uint32_t u = bitop3<TT_XOR3>(a1, b1, c1);
    const uint32_t v = bitop3<TT_MAJ>(a1, b1, c1);
    const uint32_t g1 = bitop3<TT_G1>(t0, k0, v);
    const uint32_t g2 = bitop3<TT_G2>(u, v, g1);
    return bitop3<TT_OUT>(t0, cell, g2);
}

}  // namespace golk
