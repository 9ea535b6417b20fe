// gol_edit_host.cpp -- gol_paste_host (include/golhip.h): the paste kernels' check and unit step
// (gol_edit.h: gol_region_ok, gol_edit_paste_unit) on a host buffer, lane by lane and row by row as
// the kernels do.  No HIP header: a stand-alone program links this file and gol_rle.cpp alone
// (rle_check.cpp).
#include <stdint.h>

#include "gol_edit.h"
#include "golhip.h"

int gol_set_error(int code, const char *fmt, ...);

extern "C" int gol_paste_host(int32_t layout, void *board, int64_t pitch, int64_t W, int64_t row, int64_t rows,
                              int64_t prow, int64_t x0, int64_t w, const uint64_t *pattern, int64_t stride, int32_t op,
                              int64_t *changed)
{
    const gol_region reg{layout, board, pitch, W, x0, w, row, rows, prow};
    gol_edit_geom g;
    if (!gol_region_ok(reg, op, true, &g) || (pattern && !gol_region_stride_ok(w, stride)))
        return gol_set_error(GOL_EINVAL,
                             "bad host paste (layout %d, W %lld, pitch %lld, x0 %lld, w %lld, rows %lld, stride %lld, op %d)",
                             layout, (long long)W, (long long)pitch, (long long)x0, (long long)w, (long long)rows,
                             (long long)stride, op);
    int64_t n = 0;
    for (int64_t r = 0; r < rows; ++r) {
        const uint64_t *pr = pattern ? pattern + (prow + r) * stride : nullptr;
        void *brow = gol_edit_row(g.layout, board, pitch, row + r);
        for (int64_t t = 0; t < g.T; ++t) n += gol_edit_paste_unit(g.layout, g, t, gol_edit_unit(g, t), brow, pr);
    }
    if (changed) *changed = n;
    return GOL_OK;
}
