// gol_edit.hip -- paste a rectangle of cells into the board in place (include/golhip.h,
// gol_engine_paste): the word function of gol_edit.h, one lane per distinct destination unit (word;
// byte of a byte board, or 4 of them where its rows are 4-byte aligned) and row.  Lanes run along
// the units of a row, so a wave reads and writes consecutive words; a unit belongs to exactly one
// lane of a launch (gol_edit.h), so the board is updated with a plain read-modify-write.  Every lane adds popcount(old ^ new) (bytes: the cell's
// alive state changed) to a wave sum, and one lane per wave adds that to the device counter.
// No LDS, no scratch.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gol_edit.h"
#include "gol_kernels.h"

namespace {

constexpr int EDIT_BLOCK = GOL_EDIT_BLOCK;

struct EditArgs {
    gol_edit_geom g;
    void *dst;                // row 0 of the shard's rows
    int64_t pitch;            // words (bytes of a byte board)
    int64_t row, rows, prow;  // pattern rows [prow, prow + rows) go to board rows [row, row + rows)
    const uint64_t *pattern;  // NULL: all ones
    int64_t pstride;
    unsigned long long *changed;
};

// FORM: GOL_EDIT_BYTES (one cell per lane), GOL_EDIT_BYTES4 (an aligned 4-byte word), else the bit layouts
template <int FORM>
__global__ __launch_bounds__(EDIT_BLOCK) void paste_kernel(const EditArgs a)
{
    const int64_t t = (int64_t)blockIdx.x * EDIT_BLOCK + threadIdx.x;
    const bool active = t < a.g.T;
    const int64_t u = active ? gol_edit_unit(a.g, t) : 0;
    uint32_t n = 0;
    for (int64_t r = blockIdx.y; r < a.rows; r += gridDim.y) {
        if (!active) continue;
        const uint64_t *prow = a.pattern ? a.pattern + (a.prow + r) * a.pstride : nullptr;
        if (FORM == GOL_EDIT_BYTES4) {
            uint32_t *p = (uint32_t *)((uint8_t *)a.dst + (a.row + r) * a.pitch) + u;
            const uint32_t old = *p, v = gol_edit_bytes4(a.g, t, prow, old);
            if (v != old) *p = v;
            n += (uint32_t)gol_edit_flips4(old, v);
        } else if (FORM == GOL_EDIT_BYTES) {
            uint8_t *p = (uint8_t *)a.dst + (a.row + r) * a.pitch + u;
            const uint8_t old = *p, v = gol_edit_byte(old, gol_edit_pbit(prow, t), a.g.op);
            if (v != old) *p = v;
            n += (old != 0) != (v != 0);
        } else {
            uint32_t *p = (uint32_t *)a.dst + (a.row + r) * a.pitch + u;
            const uint32_t old = *p, v = gol_edit_word(a.g, t, prow, old);
            if (v != old) *p = v;
            n += (uint32_t)__popc(old ^ v);
        }
    }
    gol_edit_wave_add(n, a.changed);  // (every lane of the wave takes part in the shuffles)
}

}  // namespace

hipError_t golk_paste(int form, void *dst, int64_t pitch, int64_t W, int64_t x0, int64_t w, int64_t row, int64_t rows,
                      int64_t prow, const uint64_t *pattern, int64_t pstride, int32_t op, uint64_t *changed,
                      hipStream_t s)
{
    EditArgs a{};
    if (form < GOL_EDIT_BYTES || form > GOL_EDIT_BAND) return hipErrorInvalidValue;
    const int f = GOL_EDIT_FORM(form, W, pitch, dst);  // byte rows as aligned 4-byte words where the board allows it
    if (!dst || !changed || row < 0 || rows < 0 || prow < 0 || !gol_edit_geom_init(a.g, f, W, x0, w, op))
        return hipErrorInvalidValue;
    if (pitch < (form == GOL_EDIT_BYTES ? W : W / 32) || (pattern && pstride < (w + 63) / 64)) return hipErrorInvalidValue;
    if (rows == 0) return hipSuccess;
    a.dst = dst;
    a.pitch = pitch;
    a.row = row;
    a.rows = rows;
    a.prow = prow;
    a.pattern = pattern;
    a.pstride = pstride;
    a.changed = (unsigned long long *)changed;
    dim3 grid;
    if (!gol_edit_grid(a.g.T, rows, &grid)) return hipErrorInvalidValue;
    if (f == GOL_EDIT_BYTES4) paste_kernel<GOL_EDIT_BYTES4><<<grid, EDIT_BLOCK, 0, s>>>(a);
    else if (f == GOL_EDIT_BYTES) paste_kernel<GOL_EDIT_BYTES><<<grid, EDIT_BLOCK, 0, s>>>(a);
    else paste_kernel<GOL_EDIT_STANDARD><<<grid, EDIT_BLOCK, 0, s>>>(a);
    return hipGetLastError();
}
