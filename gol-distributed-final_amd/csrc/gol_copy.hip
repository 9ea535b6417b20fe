// gol_copy.hip -- read a rectangle of cells from the board in place (include/golhip.h,
// gol_engine_copy, gol_engine_bounds): the mapping of gol_copy.h.  Lanes run along the units of a
// row, so a wave reads consecutive words; a workgroup strides over the rows.
//  - copy: the rectangle gathered into bit-packed pattern rows.  Every 32-bit half of a pattern
//    word has one writer (gol_copy.h), so the staged pattern takes plain vector stores, no atomics:
//    band rows one wave ballot per slot (two finished halves), standard rows a funnel shift per
//    half, byte rows one ballot of byte != 0 per 64 cells.  The writers add the popcount of what
//    they emit to a wave sum, and one lane per wave adds that to the device counter.
//  - bounds: pass 1 masks every unit to the rectangle, ORs it into a per-lane column word (one
//    atomicOr per lane and workgroup into the occupancy array), counts the alive cells and keeps the
//    first and the last non-empty row of the wave (ballots of masked != 0; one atomicMax each per
//    wave, the minimum as the maximum of the complement); pass 2 turns the occupancy words back into
//    rectangle columns, again one atomicMax each per wave.
// No LDS, no scratch; every store is a vector store or a plain atomic.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gol_copy.h"
#include "gol_region_kernels.h"

namespace {

constexpr int COPY_BLOCK = GOL_EDIT_BLOCK;
typedef unsigned long long u64;

struct CopyArgs {
    gol_edit_geom g;
    const void *src;          // row 0 of the shard's rows
    int64_t pitch;            // words (bytes of a byte board)
    int64_t row, rows, prow;  // board rows [row, row + rows) go to pattern rows [prow, prow + rows)
    int64_t lanes;            // band: T; standard: halves ceil(w / 32); bytes: w
    uint32_t *pattern;        // as 32-bit halves, 2 * pstride per row
    int64_t pstride;          // uint64 words per pattern row
    u64 *alive;
};

// FORM: GOL_EDIT_BAND, GOL_EDIT_STANDARD or GOL_EDIT_BYTES
template <int FORM>
__global__ __launch_bounds__(COPY_BLOCK) void copy_kernel(const CopyArgs a)
{
    const int64_t t = (int64_t)blockIdx.x * COPY_BLOCK + threadIdx.x;  // (a wave's first t is a multiple of 64)
    const bool active = t < a.lanes;
    const int lane = threadIdx.x & 63;
    uint32_t n = 0;
    if (FORM == GOL_EDIT_BAND) {
        const int64_t u = active ? gol_edit_unit(a.g, t) : 0;
        const uint32_t slots = gol_copy_band_slots(a.g), b0 = active ? gol_copy_band_bit(a.g, t, 0) : 0;
        const int64_t q = t >> 5, hstep = a.g.units >> 5;  // this lane's group of 32; halves per slot
        const bool writer = (lane & 31) == 0 && active;    // (T > 32q: the group holds a cell of the rectangle)
        for (int64_t r = blockIdx.y; r < a.rows; r += gridDim.y) {
            const uint32_t v = active ? ((const uint32_t *)a.src)[(a.row + r) * a.pitch + u] : 0u;
            uint32_t *prow = a.pattern + (a.prow + r) * a.pstride * 2;
            for (uint32_t m = 0; m < slots; ++m) {  // (wave-uniform: every lane takes part in the ballot)
                const bool bit = active && t + (int64_t)m * a.g.units < a.g.w && ((v >> ((b0 + m) & 31u)) & 1u);
                const u64 bal = __ballot(bit);
                const int64_t hw = q + m * hstep;
                if (writer && hw * 32 < a.g.w) {  // (a half past the last cell stays as the staging was cleared: zero)
                    const uint32_t half = (uint32_t)(bal >> (lane & 32));
                    prow[hw] = half;
                    n += (uint32_t)__popc(half);
                }
            }
        }
    } else if (FORM == GOL_EDIT_STANDARD) {
        if (active) {
            const int64_t ulo = gol_copy_std_unit(a.g, t, 0), uhi = gol_copy_std_unit(a.g, t, 1);
            const bool hi = gol_copy_std_hi(a.g, t);
            for (int64_t r = blockIdx.y; r < a.rows; r += gridDim.y) {
                const uint32_t *srow = (const uint32_t *)a.src + (a.row + r) * a.pitch;
                const uint32_t half = gol_copy_std_half(a.g, t, srow[ulo], hi ? srow[uhi] : 0u);
                a.pattern[(a.prow + r) * a.pstride * 2 + t] = half;
                n += (uint32_t)__popc(half);
            }
        }
    } else {
        const int64_t u = active ? gol_edit_unit(a.g, t) : 0;
        for (int64_t r = blockIdx.y; r < a.rows; r += gridDim.y) {
            const bool bit = active && ((const uint8_t *)a.src)[(a.row + r) * a.pitch + u] != 0;
            const u64 bal = __ballot(bit);
            if (lane == 0 && active) {  // one writer of both halves of word t / 64
                uint32_t *p = a.pattern + (a.prow + r) * a.pstride * 2 + (t >> 6) * 2;
                p[0] = (uint32_t)bal;
                p[1] = (uint32_t)(bal >> 32);
                n += (uint32_t)__popcll(bal);
            }
        }
    }
    gol_edit_wave_add(n, a.alive);  // (every lane of the wave takes part in the shuffles)
}

// hdr: [0] alive, [1] max of ~row, [2] max of row, [3] max of ~column, [4] max of column (rows and
// columns of the rectangle; zeroed before the first launch, [1 .. 4] meaningful where alive != 0)
struct BoundsArgs {
    gol_edit_geom g;
    const void *src;
    int64_t pitch;
    int64_t row, rows, vrow;  // board rows [row, row + rows) are rectangle rows [vrow, vrow + rows)
    uint32_t *occ;            // T column-occupancy words
    u64 *hdr;
};

// FORM: GOL_EDIT_BYTES (one cell per lane), GOL_EDIT_BYTES4 (an aligned 4-byte word), else the bit layouts
template <int FORM>
__global__ __launch_bounds__(COPY_BLOCK) void bounds_rows_kernel(const BoundsArgs a)
{
    const int64_t t = (int64_t)blockIdx.x * COPY_BLOCK + threadIdx.x;
    const bool active = t < a.g.T;
    const int64_t u = active ? gol_edit_unit(a.g, t) : 0;
    const uint32_t mask = active ? gol_copy_mask(a.g, t) : 0u;
    uint32_t n = 0, col = 0;
    int64_t first = -1, last = -1;  // wave-uniform: the wave's first and last row with an alive cell
    for (int64_t r = blockIdx.y; r < a.rows; r += gridDim.y) {
        const uint32_t o = active ? gol_copy_occ_unit(FORM, a.g, u, mask, gol_edit_row(FORM, a.src, a.pitch, a.row + r)) : 0u;
        col |= o;
        n += (uint32_t)__popc(o);
        if (__ballot(o != 0)) {  // (every lane of the wave takes part)
            if (first < 0) first = r;
            last = r;
        }
    }
    if (col) atomicOr(a.occ + t, col);
    if ((threadIdx.x & 63) == 0 && first >= 0) {
        atomicMax(a.hdr + 1, ~(u64)(a.vrow + first));
        atomicMax(a.hdr + 2, (u64)(a.vrow + last));
    }
    gol_edit_wave_add(n, a.hdr);
}

__global__ __launch_bounds__(COPY_BLOCK) void bounds_cols_kernel(const gol_edit_geom g, const uint32_t *occ, u64 *hdr)
{
    const int64_t t = (int64_t)blockIdx.x * COPY_BLOCK + threadIdx.x;
    const uint32_t o = t < g.T ? occ[t] : 0u;
    u64 lo = 0, hi = 0;  // max of ~cmin, max of cmax; 0: none
    if (o) {
        int64_t cmin, cmax;
        gol_copy_cols(g, t, o, &cmin, &cmax);
        lo = ~(u64)cmin;
        hi = (u64)cmax;
    }
    const bool any = __ballot(o != 0) != 0;
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        lo = max(lo, (u64)__shfl_down(lo, d, 64));
        hi = max(hi, (u64)__shfl_down(hi, d, 64));
    }
    if ((threadIdx.x & 63) == 0 && any) {
        atomicMax(hdr + 3, lo);
        atomicMax(hdr + 4, hi);
    }
}

}  // namespace

hipError_t golk_copy(const gol_region &r, uint64_t *pattern, int64_t pstride, uint64_t *alive, hipStream_t s)
{
    CopyArgs a{};
    if (!pattern || !alive || !gol_region_ok(r, GOL_EDIT_COPY, false, &a.g) || !gol_region_stride_ok(r.w, pstride))
        return hipErrorInvalidValue;
    if (r.rows == 0) return hipSuccess;
    a.src = r.base;
    a.pitch = r.pitch;
    a.row = r.row;
    a.rows = r.rows;
    a.prow = r.at;
    a.lanes = r.layout == GOL_EDIT_BAND ? a.g.T : r.layout == GOL_EDIT_STANDARD ? (r.w + 31) / 32 : r.w;
    a.pattern = (uint32_t *)pattern;
    a.pstride = pstride;
    a.alive = (u64 *)alive;
    dim3 grid;
    if (!gol_edit_grid(a.lanes, r.rows, &grid)) return hipErrorInvalidValue;
    if (r.layout == GOL_EDIT_BAND) copy_kernel<GOL_EDIT_BAND><<<grid, COPY_BLOCK, 0, s>>>(a);
    else if (r.layout == GOL_EDIT_STANDARD) copy_kernel<GOL_EDIT_STANDARD><<<grid, COPY_BLOCK, 0, s>>>(a);
    else copy_kernel<GOL_EDIT_BYTES><<<grid, COPY_BLOCK, 0, s>>>(a);
    return hipGetLastError();
}

hipError_t golk_bounds_rows(const gol_region &r, uint32_t *occ, uint64_t *hdr, hipStream_t s)
{
    BoundsArgs a{};
    if (!occ || !hdr || !gol_region_ok(r, GOL_EDIT_COPY, true, &a.g)) return hipErrorInvalidValue;
    if (r.rows == 0) return hipSuccess;
    a.src = r.base;
    a.pitch = r.pitch;
    a.row = r.row;
    a.rows = r.rows;
    a.vrow = r.at;
    a.occ = occ;
    a.hdr = (u64 *)hdr;
    dim3 grid;
    if (!gol_edit_grid(a.g.T, r.rows, &grid)) return hipErrorInvalidValue;
    if (a.g.layout == GOL_EDIT_BYTES4) bounds_rows_kernel<GOL_EDIT_BYTES4><<<grid, COPY_BLOCK, 0, s>>>(a);
    else if (a.g.layout == GOL_EDIT_BYTES) bounds_rows_kernel<GOL_EDIT_BYTES><<<grid, COPY_BLOCK, 0, s>>>(a);
    else bounds_rows_kernel<GOL_EDIT_STANDARD><<<grid, COPY_BLOCK, 0, s>>>(a);
    return hipGetLastError();
}

hipError_t golk_bounds_cols(const gol_region &r, const uint32_t *occ, uint64_t *hdr, hipStream_t s)
{
    gol_edit_geom g;
    if (!occ || !hdr || !gol_region_ok(r, GOL_EDIT_COPY, true, &g)) return hipErrorInvalidValue;
    dim3 grid;
    if (!gol_edit_grid(g.T, 1, &grid)) return hipErrorInvalidValue;
    bounds_cols_kernel<<<grid, COPY_BLOCK, 0, s>>>(g, occ, (u64 *)hdr);
    return hipGetLastError();
}
