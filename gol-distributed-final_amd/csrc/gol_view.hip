// gol_view.hip -- viewport frames (include/golhip.h, gol_engine_view): the alive cells of every
// scale x scale box of a torus rectangle, counted from the board in the layout it is stepped in.
//
// A view is (x0, y0, scale, out_w, out_h); viewport cell (c, v), 0 <= c < C = out_w * scale,
// 0 <= v < out_h * scale, is board cell ((x0 + c) mod W, (y0 + v) mod H) and belongs to pixel
// (c / scale, v / scale).  One launch adds a run of source rows (gol_view_plan) to the frame, so the
// rows of one box may come from several shards, ranks or launches: the frame is only ever added to.
//
// Lanes run along the words of a row.  A workgroup takes 256 consecutive words (bytes of a byte
// board) and at most VIEW_ROWS rows of one pixel row, and
//  1. adds those rows bit-sliced: a ripple-carry counter of NP bit planes per word gives the
//     column counts of its 32 cells at once (one coalesced 4-byte load per lane and row);
//  2. walks the pixels a word contributes to ("slots"): the count of a pixel's cells in the word is
//     sum_k popcount(plane_k & mask) << k.
//       band rows (bit b of word w = cell b*Wd + w): slot m is the one bit (b0 + m) mod 32, viewport
//         cell c = t + m*Wd for lane t -- along the lanes c is consecutive, so `scale` neighbouring
//         lanes share a pixel; a box that straddles a band boundary (word Wd-1 bit b, then word 0
//         bit b+1) simply continues in another lane's next slot;
//       standard rows (word s = cells 32s .. 32s+31): slot n is the n-th pixel the word overlaps,
//         its mask the run of bits inside it;
//       byte rows: the same with 4 cells per aligned 4-byte word and packed 8-bit counters (W % 4
//         == 0; else one byte per lane);
//  3. sums each slot over the neighbouring lanes of the same pixel (a segmented wave scan through
//     lane shuffles: the pixel index never decreases along the lanes) and adds one total per
//     pixel and wave to the frame.
// Only the words the viewport covers are read, and only the rows of the run.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gol_edit.h"
#include "gol_region_kernels.h"

namespace {

constexpr int VIEW_BLOCK = 256;
constexpr int VIEW_ROWS = 128;  // rows per workgroup: a count <= 128 fits 8 planes
constexpr uint32_t VIEW_NOKEY = 0xffffffffu;

struct ViewArgs {
    const void *src;   // row 0 of the shard's rows
    int64_t pitch;     // row pitch in words (bytes of a byte board)
    int64_t units;     // words per row (Wd); bytes: W / 4 words, or W bytes
    int64_t first;     // unit of viewport cell 0: band x0 % Wd, standard x0 / 32, bytes x0 / 4 or x0
    int64_t T;         // units along the viewport
    int64_t C;         // viewport cells along x (out_w * scale)
    int64_t row, rows, vrow;  // the run: source rows [row, row + rows) are viewport rows vrow ..
    uint32_t *frame;   // out_h x out_w counts, dense
    uint32_t scale, out_w;
    uint32_t nsub;     // workgroups per pixel row (ceil(scale / VIEW_ROWS))
    uint32_t nslots;   // slots per word
    uint32_t bit0;     // band: x0 / Wd; standard: x0 % 32; byte words: x0 % 4
    uint32_t qW, rW;   // band: Wd / scale, Wd % scale
};

// v summed over the neighbouring lanes with the same key (keys never decrease along the lanes;
// VIEW_NOKEY lanes carry 0); the last lane of each run adds its total to frow[key].
__device__ __forceinline__ void seg_emit(uint32_t v, uint32_t key, uint32_t *frow, int lane)
{
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t ov = __shfl_up(v, d, 64);
        const uint32_t ok = __shfl_up(key, d, 64);
        if (lane >= d && ok == key) v += ov;
    }
    const uint32_t nk = __shfl_down(key, 1, 64);
    if ((lane == 63 || nk != key) && key != VIEW_NOKEY && v != 0) atomicAdd(frow + key, v);
}

// The rows this workgroup adds: viewport rows [lo, hi) of pixel row *j (empty: nothing to do).
__device__ __forceinline__ bool view_rows(const ViewArgs &a, int64_t *j, int64_t *lo, int64_t *hi)
{
    const int64_t g = blockIdx.x;
    *j = a.vrow / a.scale + g / a.nsub;
    const int64_t box = *j * (int64_t)a.scale, sub = box + (g % a.nsub) * (int64_t)VIEW_ROWS;
    int64_t e = sub + VIEW_ROWS;
    if (e > box + a.scale) e = box + a.scale;
    if (e > a.vrow + a.rows) e = a.vrow + a.rows;
    *lo = sub > a.vrow ? sub : a.vrow;
    *hi = e;
    return *lo < *hi;
}

template <int NP, bool BAND>
__global__ __launch_bounds__(VIEW_BLOCK) void view_bits_kernel(const ViewArgs a)
{
    int64_t j, lo, hi;
    if (!view_rows(a, &j, &lo, &hi)) return;  // (the same in every lane)
    const int lane = threadIdx.x & 63;
    uint32_t *frow = a.frame + j * (int64_t)a.out_w;
    const int64_t nxb = (a.T + VIEW_BLOCK - 1) / VIEW_BLOCK;
    for (int64_t xb = blockIdx.y; xb < nxb; xb += gridDim.y) {
        const int64_t t = xb * VIEW_BLOCK + threadIdx.x;
        const bool active = t < a.T;
        int64_t w = a.first + t;  // < 2 * units
        const uint32_t carry = w >= a.units;
        if (carry) w -= a.units;
        // 1. the column counts of the word's 32 cells over rows [lo, hi), bit-sliced
        uint32_t p[NP];
#pragma unroll
        for (int k = 0; k < NP; ++k) p[k] = 0;
        if (active) {
            const uint32_t *ptr = (const uint32_t *)a.src + (a.row + (lo - a.vrow)) * a.pitch + w;
            if (NP == 1) {
                p[0] = *ptr;
            } else {
#pragma unroll 4
                for (int64_t r = lo; r < hi; ++r, ptr += a.pitch) {
                    uint32_t c = *ptr;
#pragma unroll
                    for (int k = 0; k < NP; ++k) {
                        const uint32_t n = p[k] & c;
                        p[k] ^= c;
                        c = n;
                    }
                }
            }
        }
        // 2., 3. the pixels of the word, slot by slot (every lane takes part in the shuffles)
        if (BAND) {
            uint32_t q = (uint32_t)t / a.scale, r = (uint32_t)t % a.scale;  // t < Wd < 2^31
            int64_t c = t;
            for (uint32_t m = 0; m < a.nslots; ++m) {
                const bool ok = active && c < a.C;
                const uint32_t mask = 1u << ((a.bit0 + carry + m) & 31);
                uint32_t v = 0;
#pragma unroll
                for (int k = 0; k < NP; ++k) v += (uint32_t)__popc(p[k] & mask) << k;
                seg_emit(ok ? v : 0u, ok ? q : VIEW_NOKEY, frow, lane);
                c += a.units;
                q += a.qW;
                r += a.rW;
                if (r >= a.scale) {
                    r -= a.scale;
                    ++q;
                }
            }
        } else {
            // the word's cells are viewport cells [c0, c0 + 32), clipped to [0, C)
            const int64_t c0 = t * 32 - (int64_t)a.bit0;
            const int64_t clo = c0 > 0 ? c0 : 0, chi = c0 + 32 < a.C ? c0 + 32 : a.C;
            const bool some = active && clo < chi;
            const uint64_t i0 = some ? (uint64_t)clo / a.scale : 0;
            for (uint32_t n = 0; n < a.nslots; ++n) {
                const int64_t i = (int64_t)i0 + n;
                int64_t blo = i * (int64_t)a.scale, bhi = blo + a.scale;
                if (blo < clo) blo = clo;
                if (bhi > chi) bhi = chi;
                const bool ok = some && blo < bhi;
                const uint32_t b0 = ok ? (uint32_t)(blo - c0) : 0u, b1 = ok ? (uint32_t)(bhi - c0) : 0u;  // 0 <= b0 < b1 <= 32
                const uint32_t mask = (b1 >= 32 ? 0xffffffffu : (1u << b1) - 1u) & ~((1u << b0) - 1u);
                uint32_t v = 0;
#pragma unroll
                for (int k = 0; k < NP; ++k) v += (uint32_t)__popc(p[k] & mask) << k;
                seg_emit(ok ? v : 0u, ok ? (uint32_t)i : VIEW_NOKEY, frow, lane);
            }
        }
    }
}

// Byte rows with W % 4 == 0 (4-byte aligned rows): the standard form with 4 cells per word.  A
// lane adds the rows of its aligned word as four packed 8-bit counters of bytes != 0 (at most
// VIEW_ROWS = 128 each), then walks the pixels the word's 4 cells overlap.
__global__ __launch_bounds__(VIEW_BLOCK) void view_bytes4_kernel(const ViewArgs a)
{
    int64_t j, lo, hi;
    if (!view_rows(a, &j, &lo, &hi)) return;
    const int lane = threadIdx.x & 63;
    uint32_t *frow = a.frame + j * (int64_t)a.out_w;
    const int64_t nxb = (a.T + VIEW_BLOCK - 1) / VIEW_BLOCK;
    const int64_t wpitch = a.pitch / 4;
    for (int64_t xb = blockIdx.y; xb < nxb; xb += gridDim.y) {
        const int64_t t = xb * VIEW_BLOCK + threadIdx.x;
        const bool active = t < a.T;
        int64_t w = a.first + t;  // < 2 * units
        if (w >= a.units) w -= a.units;
        uint32_t acc = 0;
        if (active) {
            const uint32_t *ptr = (const uint32_t *)a.src + (a.row + (lo - a.vrow)) * wpitch + w;
#pragma unroll 4
            for (int64_t r = lo; r < hi; ++r, ptr += wpitch) {
                uint32_t u = *ptr;  // bit 0 of every byte = the byte != 0
                u |= u >> 4;
                u |= u >> 2;
                u |= u >> 1;
                acc += u & 0x01010101u;
            }
        }
        const int64_t c0 = t * 4 - (int64_t)a.bit0;
        const int64_t clo = c0 > 0 ? c0 : 0, chi = c0 + 4 < a.C ? c0 + 4 : a.C;
        const bool some = active && clo < chi;
        const uint64_t i0 = some ? (uint64_t)clo / a.scale : 0;
        for (uint32_t n = 0; n < a.nslots; ++n) {
            const int64_t i = (int64_t)i0 + n;
            int64_t blo = i * (int64_t)a.scale, bhi = blo + a.scale;
            if (blo < clo) blo = clo;
            if (bhi > chi) bhi = chi;
            const bool ok = some && blo < bhi;
            const uint32_t b0 = ok ? (uint32_t)(blo - c0) : 0u, nb = ok ? (uint32_t)(bhi - blo) : 0u;  // b0 + nb <= 4
            uint32_t m = acc >> (8 * b0);
            if (nb < 4) m &= (1u << (8 * nb)) - 1u;
            const uint32_t v = (m & 0xff) + ((m >> 8) & 0xff) + ((m >> 16) & 0xff) + (m >> 24);
            seg_emit(ok ? v : 0u, ok ? (uint32_t)i : VIEW_NOKEY, frow, lane);
        }
    }
}

// Byte rows of any width: one cell per lane, consecutive lanes read consecutive bytes.
__global__ __launch_bounds__(VIEW_BLOCK) void view_bytes_kernel(const ViewArgs a)
{
    int64_t j, lo, hi;
    if (!view_rows(a, &j, &lo, &hi)) return;
    const int lane = threadIdx.x & 63;
    uint32_t *frow = a.frame + j * (int64_t)a.out_w;
    const int64_t nxb = (a.T + VIEW_BLOCK - 1) / VIEW_BLOCK;
    for (int64_t xb = blockIdx.y; xb < nxb; xb += gridDim.y) {
        const int64_t c = xb * VIEW_BLOCK + threadIdx.x;
        const bool active = c < a.T;
        int64_t x = a.first + c;
        if (x >= a.units) x -= a.units;
        uint32_t v = 0;
        if (active) {
            const uint8_t *ptr = (const uint8_t *)a.src + (a.row + (lo - a.vrow)) * a.pitch + x;
#pragma unroll 4
            for (int64_t r = lo; r < hi; ++r, ptr += a.pitch) v += *ptr != 0;
        }
        const uint32_t key = a.scale == 1 ? (uint32_t)c : (uint32_t)((uint64_t)c / a.scale);
        seg_emit(active ? v : 0u, active ? key : VIEW_NOKEY, frow, lane);
    }
}

// 4 pixels per lane: ceil(255 n / scale^2) (n <= scale^2 <= 2^24: 255 n + scale^2 - 1 < 2^32).
__global__ __launch_bounds__(VIEW_BLOCK) void view_pixels_kernel(const uint32_t *frame, int64_t n4, uint32_t s2,
                                                                 uint32_t *pixels)
{
    const int64_t i = (int64_t)blockIdx.x * VIEW_BLOCK + threadIdx.x;
    if (i >= n4) return;
    const uint4 c = ((const uint4 *)frame)[i];
    const uint32_t a = (255u * c.x + s2 - 1) / s2, b = (255u * c.y + s2 - 1) / s2, d = (255u * c.z + s2 - 1) / s2,
                   e = (255u * c.w + s2 - 1) / s2;
    pixels[i] = a | (b << 8) | (d << 16) | (e << 24);
}

template <bool BAND>
hipError_t launch_bits(const ViewArgs &a, int np, dim3 grid, hipStream_t s)
{
    if (np == 1) view_bits_kernel<1, BAND><<<grid, VIEW_BLOCK, 0, s>>>(a);
    else if (np == 4) view_bits_kernel<4, BAND><<<grid, VIEW_BLOCK, 0, s>>>(a);
    else view_bits_kernel<8, BAND><<<grid, VIEW_BLOCK, 0, s>>>(a);
    return hipGetLastError();
}

}  // namespace

hipError_t golk_view_counts(const gol_region &r, int32_t scale, uint32_t *frame, hipStream_t s)
{
    gol_edit_geom g;  // of the viewport's cells: r.w = out_w * scale of them from column r.x0
    if (!frame || scale < 1 || scale > 4096 || r.w % scale != 0 || !gol_region_ok(r, GOL_EDIT_COPY, true, &g))
        return hipErrorInvalidValue;
    if (r.rows == 0) return hipSuccess;
    ViewArgs a{};
    a.src = r.base;
    a.pitch = r.pitch;
    a.units = g.units;
    a.first = g.first;
    a.bit0 = g.bit0;
    a.C = r.w;
    a.row = r.row;
    a.rows = r.rows;
    a.vrow = r.at;
    a.frame = frame;
    a.scale = (uint32_t)scale;
    a.out_w = (uint32_t)(r.w / scale);
    a.nsub = (uint32_t)((scale + VIEW_ROWS - 1) / VIEW_ROWS);
    // the view's own: a lane per unit the viewport touches -- past the geometry's clamp to the units of a
    // row, the first word again for the cells that wrapped (g.wrap_c) -- and the pixels (slots) of a unit
    a.T = g.T + (g.wrap_c >= 0);
    if (g.layout == GOL_EDIT_BYTES) {
        a.nslots = 1;
    } else if (g.layout == GOL_EDIT_BAND) {
        a.nslots = (uint32_t)((a.C + a.units - 1) / a.units);  // <= 32 bits of a word
        a.qW = (uint32_t)(a.units / scale);
        a.rW = (uint32_t)(a.units % scale);
    } else {
        const uint32_t cells = g.layout == GOL_EDIT_STANDARD ? 32 : 4;
        a.nslots = (cells - 2 + a.scale) / a.scale + 1;  // pixels `cells` consecutive cells can touch
    }
    // one workgroup per pixel row of the run and VIEW_ROWS rows of its boxes
    const int64_t j0 = r.at / scale, j1 = (r.at + r.rows - 1) / scale;
    const int64_t groups = (j1 - j0 + 1) * a.nsub;
    const int64_t nxb = (a.T + VIEW_BLOCK - 1) / VIEW_BLOCK;
    if (groups > INT32_MAX) return hipErrorInvalidValue;
    const dim3 grid((unsigned)groups, (unsigned)(nxb < 65535 ? nxb : 65535));
    const int most = scale < VIEW_ROWS ? scale : VIEW_ROWS;  // rows a workgroup adds at most
    if (r.layout == GOL_EDIT_BYTES) {
        if (g.layout == GOL_EDIT_BYTES4) view_bytes4_kernel<<<grid, VIEW_BLOCK, 0, s>>>(a);
        else view_bytes_kernel<<<grid, VIEW_BLOCK, 0, s>>>(a);
        return hipGetLastError();
    }
    const int np = most == 1 ? 1 : (most <= 15 ? 4 : 8);
    return r.layout == GOL_EDIT_BAND ? launch_bits<true>(a, np, grid, s) : launch_bits<false>(a, np, grid, s);
}

hipError_t golk_view_pixels(const uint32_t *frame, int64_t n, int32_t scale, uint8_t *pixels, hipStream_t s)
{
    if (!frame || !pixels || n < 0 || scale < 1 || scale > 4096) return hipErrorInvalidValue;
    const int64_t n4 = (n + 3) / 4;
    if (n4 == 0) return hipSuccess;
    const int64_t blocks = (n4 + VIEW_BLOCK - 1) / VIEW_BLOCK;
    if (blocks > INT32_MAX) return hipErrorInvalidValue;
    view_pixels_kernel<<<(unsigned)blocks, VIEW_BLOCK, 0, s>>>(frame, n4, (uint32_t)scale * (uint32_t)scale,
                                                               (uint32_t *)pixels);
    return hipGetLastError();
}
