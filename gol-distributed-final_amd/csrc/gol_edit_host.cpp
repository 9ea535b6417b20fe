// gol_edit_host.cpp -- gol_paste_host (include/golhip.h): the paste kernels' word function
// (gol_edit.h) applied to a host buffer, lane by lane and row by row as the kernels do.  No HIP
// header: a stand-alone program links this file and gol_rle.cpp alone (rle_check.cpp).
#include <stdint.h>

#include "gol_edit.h"
#include "golhip.h"

int gol_set_error(int code, const char *fmt, ...);

extern "C" int gol_paste_host(int32_t layout, void *board, int64_t pitch, int64_t W, int64_t row, int64_t rows,
                              int64_t prow, int64_t x0, int64_t w, const uint64_t *pattern, int64_t stride, int32_t op,
                              int64_t *changed)
{
    gol_edit_geom g;
    const int32_t form = layout < GOL_EDIT_BYTES || layout > GOL_EDIT_BAND ? -1 : GOL_EDIT_FORM(layout, W, pitch, board);
    if (!board || row < 0 || rows < 0 || prow < 0 || !gol_edit_geom_init(g, form, W, x0, w, op) ||
        pitch < (layout == GOL_EDIT_BYTES ? W : g.units) || (pattern && stride < (w + 63) / 64))
        return gol_set_error(GOL_EINVAL,
                             "bad host paste (layout %d, W %lld, pitch %lld, x0 %lld, w %lld, rows %lld, stride %lld, op %d)",
                             layout, (long long)W, (long long)pitch, (long long)x0, (long long)w, (long long)rows,
                             (long long)stride, op);
    int64_t n = 0;
    for (int64_t r = 0; r < rows; ++r) {
        const uint64_t *pr = pattern ? pattern + (prow + r) * stride : nullptr;
        for (int64_t t = 0; t < g.T; ++t) {
            const int64_t u = gol_edit_unit(g, t);
            if (form == GOL_EDIT_BYTES4) {
                uint32_t *p = (uint32_t *)((uint8_t *)board + (row + r) * pitch) + u;
                const uint32_t old = *p, v = gol_edit_bytes4(g, t, pr, old);
                if (v != old) *p = v;
                n += gol_edit_flips4(old, v);
            } else if (form == GOL_EDIT_BYTES) {
                uint8_t *p = (uint8_t *)board + (row + r) * pitch + u;
                const uint8_t old = *p, v = gol_edit_byte(old, gol_edit_pbit(pr, t), op);
                if (v != old) *p = v;
                n += (old != 0) != (v != 0);
            } else {
                uint32_t *p = (uint32_t *)board + (row + r) * pitch + u;
                const uint32_t old = *p, v = gol_edit_word(g, t, pr, old);
                if (v != old) *p = v;
                n += __builtin_popcount(old ^ v);
            }
        }
    }
    if (changed) *changed = n;
    return GOL_OK;
}
