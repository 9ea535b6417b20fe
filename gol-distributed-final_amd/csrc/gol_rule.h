// gol_rule.h -- a life-like rule (B/S, radius 1, outer-totalistic) as data, and the one circuit
// that evaluates it on bit-sliced words.  Shared by the rule kernels (gol_kernels.hip, TableRule) and the host
// (gol_rule_eval_host, include/golhip.h), so the circuit the GPU runs is tested on the CPU.
//
// A rule is two 9-bit masks: birth bit n / survive bit n = a dead / an alive cell with exactly n
// alive neighbours of its 8 is alive next turn.  The kernels count the 3x3 block INCLUDING the
// centre, T = 0..9 (the horizontal sums of the register pipeline include the cell), so the rule
// becomes two tables over T: dead cells look up D[T] = birth bit T, alive cells A[T] = survive
// bit T - 1 (A[0] and D[9] cannot occur).  Expanded once per wave into 0 / ~0 words, the tables
// are the leaves of a 2:1 mux tree: on the centre cell first (10 ops, each one word with two
// wave-uniform constants), then on the count bits t0 (5), t1 (2), t2 (1), t3 (1): 19 ops per word.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define GOL_RULE_HD __host__ __device__ inline __attribute__((always_inline))  // (no HIP header needed)
#else
#define GOL_RULE_HD inline
#endif

#define GOL_RULE_BIRTH_CONWAY 0x008u
#define GOL_RULE_SURVIVE_CONWAY 0x00Cu

// The two tables over the centre-inclusive count, as 0 / ~0 words.
struct gol_rule_tab {
    uint32_t a[10];  // alive centre, T alive cells in the 3x3 block
    uint32_t d[10];  // dead centre
};

GOL_RULE_HD void gol_rule_expand(uint32_t birth, uint32_t survive, gol_rule_tab &t)
{
    for (int n = 0; n < 10; ++n) {
        t.d[n] = n <= 8 ? 0u - ((birth >> n) & 1u) : 0u;
        t.a[n] = n >= 1 ? 0u - ((survive >> (n - 1)) & 1u) : 0u;
    }
}

// The circuit's five 3-input gates.  On the GPU each is one v_bitop3_b32 (truth tables: operand 0
// -> 0xF0, operand 1 -> 0xCC, operand 2 -> 0xAA); left to the compiler, the plain forms became
// chains of 2-input ops (49 VALU ops per word instead of 28).
#if defined(__HIP_DEVICE_COMPILE__)
#define GOL_RULE_GATE(tt, plain) return __builtin_amdgcn_bitop3_b32(a, b, c, tt)
#else
#define GOL_RULE_GATE(tt, plain) return plain
#endif
GOL_RULE_HD uint32_t gol_rule_mux(uint32_t a, uint32_t b, uint32_t c) { GOL_RULE_GATE(0xCA, (a & b) | (~a & c)); }  // a ? b : c
GOL_RULE_HD uint32_t gol_rule_xor3(uint32_t a, uint32_t b, uint32_t c) { GOL_RULE_GATE(0x96, a ^ b ^ c); }
GOL_RULE_HD uint32_t gol_rule_maj(uint32_t a, uint32_t b, uint32_t c) { GOL_RULE_GATE(0xE8, (a & b) | (c & (a | b))); }
GOL_RULE_HD uint32_t gol_rule_xa(uint32_t a, uint32_t b, uint32_t c) { GOL_RULE_GATE(0x78, a ^ (b & c)); }
GOL_RULE_HD uint32_t gol_rule_and3(uint32_t a, uint32_t b, uint32_t c) { GOL_RULE_GATE(0x80, a & b & c); }
#undef GOL_RULE_GATE

// next = f(centre, T) for 32 cells: t0..t3 are the bit planes of T (centre included), cell the
// centre word.
GOL_RULE_HD uint32_t gol_rule_eval(const gol_rule_tab &t, uint32_t t0, uint32_t t1, uint32_t t2, uint32_t t3,
                                   uint32_t cell)
{
    uint32_t l[10];
    for (int n = 0; n < 10; ++n) l[n] = gol_rule_mux(cell, t.a[n], t.d[n]);
    const uint32_t m01 = gol_rule_mux(t0, l[1], l[0]), m23 = gol_rule_mux(t0, l[3], l[2]);
    const uint32_t m45 = gol_rule_mux(t0, l[5], l[4]), m67 = gol_rule_mux(t0, l[7], l[6]);
    const uint32_t m89 = gol_rule_mux(t0, l[9], l[8]);
    const uint32_t m03 = gol_rule_mux(t1, m23, m01), m47 = gol_rule_mux(t1, m67, m45);
    const uint32_t m07 = gol_rule_mux(t2, m47, m03);
    return gol_rule_mux(t3, m89, m07);
}

// The same from the masks (the expansion is loop-invariant and wave-uniform in a kernel).
GOL_RULE_HD uint32_t gol_rule_next(uint32_t birth, uint32_t survive, uint32_t t0, uint32_t t1, uint32_t t2,
                                   uint32_t t3, uint32_t cell)
{
    gol_rule_tab t;
    gol_rule_expand(birth, survive, t);
    return gol_rule_eval(t, t0, t1, t2, t3, cell);
}

// Bit planes of T = the sum of three rows' horizontal sums (each h0 + 2 h1 in 0..3): 7 ops.
GOL_RULE_HD void gol_rule_sum3(uint32_t a0, uint32_t a1, uint32_t b0, uint32_t b1, uint32_t c0, uint32_t c1,
                               uint32_t &t0, uint32_t &t1, uint32_t &t2, uint32_t &t3)
{
    t0 = gol_rule_xor3(a0, b0, c0);
    const uint32_t k0 = gol_rule_maj(a0, b0, c0);  // carry of the ones, weight 2
    const uint32_t u = gol_rule_xor3(a1, b1, c1);  // weight 2
    const uint32_t v = gol_rule_maj(a1, b1, c1);   // weight 4
    t1 = k0 ^ u;
    t2 = gol_rule_xa(v, k0, u);
    t3 = gol_rule_and3(v, k0, u);
}
