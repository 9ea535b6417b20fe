// gol_copy_host.cpp -- gol_copy_host and gol_bounds_host (include/golhip.h): the region-read
// kernels' check (gol_region_ok, gol_edit.h) and mapping (gol_copy.h; the bounds' pass 1 is
// gol_copy_occ_unit itself) applied to a host buffer, lane by lane and row by row as the kernels
// do.  No HIP header: a stand-alone program links this file and gol_edit_host.cpp alone
// (copy_check.cpp).
#include <stdint.h>
#include <string.h>

#include <vector>

#include "gol_copy.h"
#include "golhip.h"

int gol_set_error(int code, const char *fmt, ...);

extern "C" int gol_copy_host(int32_t layout, const void *board, int64_t pitch, int64_t W, int64_t row, int64_t rows,
                             int64_t prow, int64_t x0, int64_t w, uint64_t *pattern, int64_t stride, int64_t *alive)
{
    const gol_region reg{layout, const_cast<void *>(board), pitch, W, x0, w, row, rows, prow};
    gol_edit_geom g;
    if (!pattern || !gol_region_ok(reg, GOL_EDIT_COPY, false, &g) || !gol_region_stride_ok(w, stride))
        return gol_set_error(GOL_EINVAL, "bad host copy (layout %d, W %lld, pitch %lld, x0 %lld, w %lld, rows %lld, stride %lld)",
                             layout, (long long)W, (long long)pitch, (long long)x0, (long long)w, (long long)rows,
                             (long long)stride);
    const int64_t pw = (w + 63) / 64;
    int64_t n = 0;
    for (int64_t r = 0; r < rows; ++r) {
        uint64_t *pr = pattern + (prow + r) * stride;
        memset(pr, 0, pw * sizeof(uint64_t));  // (the kernels' cleared staging)
        auto put_half = [&](int64_t hw, uint32_t half) {  // (one writer per half: |= of a cleared half is a store)
            pr[hw >> 1] |= (uint64_t)half << (32 * (hw & 1));
            n += __builtin_popcount(half);
        };
        if (layout == GOL_EDIT_BAND) {
            const uint32_t *src = (const uint32_t *)board + (row + r) * pitch;
            const uint32_t slots = gol_copy_band_slots(g);
            for (int64_t q = 0; q * 32 < g.T; ++q)  // the ballot of lanes 32q .. 32q + 31, slot by slot
                for (uint32_t m = 0; m < slots; ++m) {
                    const int64_t hw = q + (int64_t)m * (g.units >> 5);
                    if (hw * 32 >= w) continue;
                    uint32_t half = 0;
                    for (int64_t t = q * 32; t < q * 32 + 32 && t < g.T; ++t)
                        if (t + (int64_t)m * g.units < w && ((src[gol_edit_unit(g, t)] >> gol_copy_band_bit(g, t, m)) & 1u))
                            half |= 1u << (t & 31);
                    put_half(hw, half);
                }
        } else if (layout == GOL_EDIT_STANDARD) {
            const uint32_t *src = (const uint32_t *)board + (row + r) * pitch;
            for (int64_t j = 0; j * 32 < w; ++j)
                put_half(j, gol_copy_std_half(g, j, src[gol_copy_std_unit(g, j, 0)],
                                              gol_copy_std_hi(g, j) ? src[gol_copy_std_unit(g, j, 1)] : 0u));
        } else {
            const uint8_t *src = (const uint8_t *)board + (row + r) * pitch;
            for (int64_t c = 0; c < w; ++c)
                if (src[gol_edit_unit(g, c)]) {
                    pr[c >> 6] |= (uint64_t)1 << (c & 63);
                    ++n;
                }
        }
    }
    if (alive) *alive = n;
    return GOL_OK;
}

extern "C" int gol_bounds_host(int32_t layout, const void *board, int64_t pitch, int64_t W, int64_t row, int64_t rows,
                               int64_t x0, int64_t w, int64_t *cmin, int64_t *cmax, int64_t *rmin, int64_t *rmax,
                               int64_t *alive)
{
    const gol_region reg{layout, const_cast<void *>(board), pitch, W, x0, w, row, rows, 0};
    gol_edit_geom g;
    if (!gol_region_ok(reg, GOL_EDIT_COPY, true, &g))
        return gol_set_error(GOL_EINVAL, "bad host bounds (layout %d, W %lld, pitch %lld, x0 %lld, w %lld, rows %lld)", layout,
                             (long long)W, (long long)pitch, (long long)x0, (long long)w, (long long)rows);
    std::vector<uint32_t> occ((size_t)g.T, 0u);
    int64_t n = 0, r0 = rows, r1 = -1, c0 = w, c1 = -1;
    for (int64_t t = 0; t < g.T; ++t) {  // pass 1: a lane keeps its unit and mask over the rows, as in the kernel
        const int64_t u = gol_edit_unit(g, t);
        const uint32_t mask = gol_copy_mask(g, t);
        for (int64_t r = 0; r < rows; ++r) {
            const uint32_t o = gol_copy_occ_unit(g.layout, g, u, mask, gol_edit_row(g.layout, board, pitch, row + r));
            if (!o) continue;
            occ[(size_t)t] |= o;
            n += __builtin_popcount(o);
            if (r < r0) r0 = r;
            if (r > r1) r1 = r;
        }
    }
    for (int64_t t = 0; t < g.T; ++t) {  // pass 2
        if (!occ[(size_t)t]) continue;
        int64_t a, b;
        gol_copy_cols(g, t, occ[(size_t)t], &a, &b);
        if (a < c0) c0 = a;
        if (b > c1) c1 = b;
    }
    if (cmin) *cmin = c0;
    if (cmax) *cmax = c1;
    if (rmin) *rmin = r0;
    if (rmax) *rmax = r1;
    if (alive) *alive = n;
    return GOL_OK;
}
