// Data polarity of the pair step: does the VALU run faster, or at a higher clock, when
// every gate output of the tail is sparse?  The kernel's pair step (gol_pipe.h pstage, KW = 3 stages per
// 2-row block as in band_pipe_kernel) at 4 waves per SIMD, with no memory traffic and no waits in the
// loop, in a 2 x 3 grid: the tail's truth tables before the polarity change (g1, g2 answer 1 on a dead
// neighbourhood: ~90 % ones on a settled board) and the shipped ones (the same gates complemented, their
// readers' tables adjusted: every output sparse), on three kinds of operand words:
//   zero    an all-dead board
//   soup    settled soups: per wave one of 16 slabs of 6 rows x 256 band-layout words (32 bit planes of 256
//           columns), cut from a board of 48 wrapping rows stepped 700 turns from a 50 % random fill on the
//           host (the alive share is printed; ~5 %).  6 rows is what fits beside the stages' state in 128
//           VGPRs.  The wave streams its 6 rows round and round, so stage g sees generation g of that cyclic
//           slab: settled but for the seam between its last and first row
//   rand50  independent random words, 50 % ones, entering stage 0 (stages 1, 2 see their successors)
// pstage_tt below is pstage with the four tail tables as template arguments and nothing else changed; the
// program first checks on the device that with the shipped tables it equals golk::pstage bit for bit and
// that the old tables give the same rows.  The instruction stream of the two table sets differs in the
// bitop3 immediates only (compare with --save-temps).
// Per run: one launch of >= 2 s (the shader clock settles within the first ~0.2 s), per wave the deltas
// of s_memtime (shader cycles) and s_memrealtime (100 MHz) over the loop -> SIMD cycles per block, VALU
// issue rate (661 VALU per trip of 3 blocks, counted in the loop's ISA: 3 x 3 x (64 logic + 4 DPP) + 49 for the
// loop-variant inputs and the checksum; no scratch), shader clock; median and 5-95 % band
// over waves.  The six cells run interleaved, REPS times; one JSON line per run.
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -mllvm -amdgpu-sched-strategy=max-ilp -mllvm -disable-post-ra \
//     -I include -I gol-distributed-final_amd/csrc tools/ubench/pair_polarity.hip -o tools/variants/pair_polarity
//   tools/variants/pair_polarity [REPS=3] [SECONDS=2.2]
#include <algorithm>
#include <stdio.h>
#include <stdlib.h>
#include <vector>

#include "gol_pipe.h"

namespace {
using namespace golk;

struct OldTables { static constexpr unsigned G1 = 0x43, G2 = 0x25, G3 = 0x8D, OUT = 0x90; };
struct NewTables { static constexpr unsigned G1 = TT_PG1, G2 = TT_PG2, G3 = TT_PG3, OUT = TT_POUT; };

template <class T>
__device__ __forceinline__ uint32_t pair_tail_tt(uint32_t p0, uint32_t p1, uint32_t p2, uint32_t x0, uint32_t x1, uint32_t cell)
{
    const uint32_t g1 = bitop3<T::G1>(p0, x0, cell);
    const uint32_t g2 = bitop3<T::G2>(p1, p2, x1);
    const uint32_t g3 = bitop3<T::G3>(p2, cell, g1);
    return bitop3<T::OUT>(g3, g1, g2);
}
template <class T, int DW>
__device__ __forceinline__ void pstage_tt(PairState<DW> &s, uint32_t (&r0)[DW], uint32_t (&r1)[DW])
{
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
        o0[j] = pair_tail_tt<T>(p0, p1, p2, s.a0[j], s.a1[j], s.cb[j]);
        o1[j] = pair_tail_tt<T>(p0, p1, p2, d0, d1, x0);
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

constexpr int DW = 4, KW = 3, ROWS = 6, SLABS = 16, SLAB_WORDS = ROWS * 64 * DW, HOST_ROWS = 48;

// stamps: per wave (shader cycles, 100 MHz ticks) of the loop.  in: SLABS slabs of ROWS rows of 256 words.
template <class T>
__global__ void __launch_bounds__(256, 4) pp_kernel(const uint32_t *in, uint32_t *out, uint64_t *stamps, int iters, uint32_t zmask)
{
    const int lane = threadIdx.x & 63, wave = blockIdx.x * 4 + (threadIdx.x >> 6);
    const uint32_t *src = in + (size_t)(wave % SLABS) * SLAB_WORDS + lane * DW;
    uint32_t x[ROWS][DW];
#pragma unroll
    for (int r = 0; r < ROWS; ++r)
#pragma unroll
        for (int j = 0; j < DW; ++j) x[r][j] = src[r * 64 * DW + j];
    PairState<DW> st[KW];
#pragma unroll
    for (int g = 0; g < KW; ++g)
#pragma unroll
        for (int j = 0; j < DW; ++j) st[g].a0[j] = st[g].a1[j] = st[g].b0[j] = st[g].b1[j] = st[g].cb[j] = 0;
    uint32_t acc = 0;
    const uint64_t c0 = __builtin_amdgcn_s_memtime(), t0 = __builtin_amdgcn_s_memrealtime();
    for (int it = 0; it < iters; ++it) {
#pragma unroll
        for (int u = 0; u < ROWS / 2; ++u) {
            uint32_t r0[DW], r1[DW];
            const uint32_t z = acc & zmask;  // 0 (zmask is 0), but loop-variant: stage 0's row sums stay in the loop
#pragma unroll
            for (int j = 0; j < DW; ++j) {
                r0[j] = x[2 * u][j] ^ z;
                r1[j] = x[2 * u + 1][j] ^ z;
            }
#pragma unroll
            for (int g = 0; g < KW; ++g) pstage_tt<T, DW>(st[g], r0, r1);
#pragma unroll
            for (int j = 0; j < DW; ++j) acc ^= r0[j] ^ r1[j];
        }
    }
    const uint64_t c1 = __builtin_amdgcn_s_memtime(), t1 = __builtin_amdgcn_s_memrealtime();
    if (lane == 0) {
        stamps[2 * wave] = c1 - c0;
        stamps[2 * wave + 1] = t1 - t0;
    }
    if (acc == 0x12345678u && iters < 0) out[threadIdx.x] = acc;  // (never: iters > 0)
}

// pstage_tt against the kernel's pstage, and the old tables against the shipped: mismatching words
__global__ void __launch_bounds__(64) check_kernel(const uint32_t *in, uint32_t *bad)
{
    const int lane = threadIdx.x;
    PairState<DW> a[KW], b[KW], c[KW];
    for (int g = 0; g < KW; ++g)
        for (int j = 0; j < DW; ++j) {
            a[g].a0[j] = a[g].a1[j] = a[g].b0[j] = a[g].b1[j] = a[g].cb[j] = 0;
            b[g] = a[g];
            c[g] = a[g];
        }
    uint32_t n = 0;
    for (int s = 0; s < SLABS; ++s)
        for (int u = 0; u < ROWS / 2; ++u) {
            uint32_t r[3][2][DW];
            for (int v = 0; v < 3; ++v)
                for (int j = 0; j < DW; ++j) {
                    r[v][0][j] = in[(size_t)s * SLAB_WORDS + (2 * u) * 64 * DW + lane * DW + j];
                    r[v][1][j] = in[(size_t)s * SLAB_WORDS + (2 * u + 1) * 64 * DW + lane * DW + j];
                }
            for (int g = 0; g < KW; ++g) {
                pstage<DW>(a[g], r[0][0], r[0][1]);
                pstage_tt<NewTables, DW>(b[g], r[1][0], r[1][1]);
                pstage_tt<OldTables, DW>(c[g], r[2][0], r[2][1]);
            }
            for (int j = 0; j < DW; ++j)
                n += (r[0][0][j] != r[1][0][j]) + (r[0][1][j] != r[1][1][j]) + (r[0][0][j] != r[2][0][j]) + (r[0][1][j] != r[2][1][j]);
        }
    if (n) atomicAdd(bad, n);
}

uint64_t rng_state = 0x9E3779B97F4A7C15ULL;
uint32_t rnd32()
{
    rng_state ^= rng_state << 13;
    rng_state ^= rng_state >> 7;
    rng_state ^= rng_state << 17;
    return (uint32_t)(rng_state >> 16);
}

// one turn of B3/S23 on a board of HOST_ROWS rows (wrapping) of NW band-layout words (host; bit-sliced counting in plain operators:
// T = the 3 x 3 sum including the cell, alive' = [T == 3] | (cell & [T == 4]))
void life_turn(std::vector<uint32_t> &w)
{
    constexpr int NW = 64 * DW;
    std::vector<uint32_t> h0(w.size()), h1(w.size()), o(w.size());
    for (int y = 0; y < HOST_ROWS; ++y)
        for (int j = 0; j < NW; ++j) {
            const uint32_t c = w[y * NW + j];
            // band layout: a cell's horizontal neighbours are the same bit of the adjacent words; dead beyond
            // the wave's 256 words, as lane 0 and lane 63 see it
            const uint32_t l = j > 0 ? w[y * NW + j - 1] : 0u, r = j + 1 < NW ? w[y * NW + j + 1] : 0u;
            h0[y * NW + j] = l ^ c ^ r;
            h1[y * NW + j] = (l & c) | (r & (l | c));
        }
    for (int y = 0; y < HOST_ROWS; ++y)
        for (int j = 0; j < NW; ++j) {
            const int a = ((y + HOST_ROWS - 1) % HOST_ROWS) * NW + j, b = y * NW + j, c = ((y + 1) % HOST_ROWS) * NW + j;
            const uint32_t t0 = h0[a] ^ h0[b] ^ h0[c], k0 = (h0[a] & h0[b]) | (h0[c] & (h0[a] | h0[b]));
            const uint32_t u = h1[a] ^ h1[b] ^ h1[c], v = (h1[a] & h1[b]) | (h1[c] & (h1[a] | h1[b]));
            const uint32_t b1 = k0 ^ u, cy = k0 & u, b2 = v ^ cy, b3 = v & cy;  // T = t0 + 2 b1 + 4 b2 + 8 b3
            o[b] = (t0 & b1 & ~b2 & ~b3) | (w[b] & ~t0 & ~b1 & b2 & ~b3);
        }
    w.swap(o);
}

double ones_share(const std::vector<uint32_t> &v)
{
    uint64_t n = 0;
    for (uint32_t x : v) n += __builtin_popcount(x);
    return (double)n / (32.0 * v.size());
}

#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_)); exit(1); } } while (0)

template <class T>
void run(const char *tables, const char *data, double ones, const uint32_t *in, uint32_t *out, uint64_t *stamps, int iters, int rep)
{
    const int blocks = 256 * 4, waves = blocks * 4;  // 4 workgroups of 4 waves per CU: 4 waves per SIMD
    CK(hipMemset(stamps, 0, (size_t)waves * 16));
    hipLaunchKernelGGL((pp_kernel<T>), dim3(blocks), dim3(256), 0, 0, in, out, stamps, iters, 0u);
    CK(hipGetLastError());
    CK(hipDeviceSynchronize());
    std::vector<uint64_t> h(2 * waves);
    CK(hipMemcpy(h.data(), stamps, (size_t)waves * 16, hipMemcpyDeviceToHost));
    std::vector<double> ghz, cyc;
    for (int i = 0; i < waves; ++i)
        if (h[2 * i] && h[2 * i + 1]) {
            ghz.push_back((double)h[2 * i] / ((double)h[2 * i + 1] * 10.0));  // cycles per 10 ns tick
            cyc.push_back((double)h[2 * i] / ((double)iters * (ROWS / 2)) / 4.0);  // SIMD cycles per block per wave
        }
    std::sort(ghz.begin(), ghz.end());
    std::sort(cyc.begin(), cyc.end());
    auto pct = [](const std::vector<double> &v, double q) { return v[(size_t)(q * (v.size() - 1) + 0.5)]; };
    const double valu = 661.0 / 3;  // per block (the loop's ISA, see above)
    double secs = 0;
    for (int i = 0; i < waves; ++i) secs = std::max(secs, (double)h[2 * i + 1] * 1e-8);
    printf("{\"rep\": %d, \"tables\": \"%s\", \"data\": \"%s\", \"ones\": %.4f, \"waves\": %zu, \"launch_s\": %.3f, "
           "\"simd_cycles_per_block\": %.2f, \"valu_issue\": %.4f, \"clock_GHz\": %.4f, \"clock_GHz_p5_p95\": [%.4f, %.4f], "
           "\"blocks_per_us_per_simd\": %.4f}\n",
           rep, tables, data, ones, ghz.size(), secs, pct(cyc, 0.5), valu * 2.0 / pct(cyc, 0.5), pct(ghz, 0.5), pct(ghz, 0.05),
           pct(ghz, 0.95), pct(ghz, 0.5) * 1e3 / (pct(cyc, 0.5) * 4.0));
    fflush(stdout);
}
}  // namespace

int main(int argc, char **argv)
{
    const int reps = argc > 1 ? atoi(argv[1]) : 3;
    const double seconds = argc > 2 ? atof(argv[2]) : 2.2;
    const size_t words = (size_t)SLABS * SLAB_WORDS;
    std::vector<uint32_t> zero(words, 0), soup(words), r50(words);
    for (auto &x : r50) x = rnd32();
    for (int s = 0; s < SLABS; ++s) {
        std::vector<uint32_t> w((size_t)HOST_ROWS * 64 * DW);
        for (auto &x : w) x = rnd32();
        for (int t = 0; t < 700; ++t) life_turn(w);
        std::copy(w.begin(), w.begin() + SLAB_WORDS, soup.begin() + (size_t)s * SLAB_WORDS);
    }
    uint32_t *in[3], *out, *bad;
    uint64_t *stamps;
    const std::vector<uint32_t> *host[3] = {&zero, &soup, &r50};
    const char *names[3] = {"zero", "soup", "rand50"};
    for (int d = 0; d < 3; ++d) {
        CK(hipMalloc(&in[d], words * 4));
        CK(hipMemcpy(in[d], host[d]->data(), words * 4, hipMemcpyHostToDevice));
    }
    CK(hipMalloc(&out, 4096));
    CK(hipMalloc(&bad, 4));
    CK(hipMalloc(&stamps, (size_t)256 * 4 * 4 * 16));
    CK(hipMemset(bad, 0, 4));
    for (int d = 0; d < 3; ++d) hipLaunchKernelGGL(check_kernel, dim3(1), dim3(64), 0, 0, (const uint32_t *)in[d], bad);
    uint32_t nbad = 1;
    CK(hipMemcpy(&nbad, bad, 4, hipMemcpyDeviceToHost));
    if (nbad) {
        fprintf(stderr, "pstage_tt differs from pstage, or the old tables from the shipped ones: %u words\n", nbad);
        return 1;
    }
    // iterations for `seconds`: from a short launch of the soup cell
    run<NewTables>("calibrate", "soup", ones_share(soup), in[1], out, stamps, 20000, -1);
    std::vector<uint64_t> h(2);
    CK(hipMemcpy(h.data(), stamps, 16, hipMemcpyDeviceToHost));  // wave 0: shader cycles (the ticks of a short launch mislead)
    const int iters = (int)(20000.0 * seconds / ((double)h[0] / 2.35e9)) + 1;
    for (int rep = 0; rep < reps; ++rep)
        for (int d = 0; d < 3; ++d) {
            run<OldTables>("old", names[d], ones_share(*host[d]), in[d], out, stamps, iters, rep);
            run<NewTables>("new", names[d], ones_share(*host[d]), in[d], out, stamps, iters, rep);
        }
    return 0;
}
