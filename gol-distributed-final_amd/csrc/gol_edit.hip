// gol_edit.hip -- paste a rectangle of cells into the board in place (include/golhip.h,
// gol_engine_paste): the unit step of gol_edit.h (gol_edit_paste_unit, which gol_paste_host runs
// too), one lane per distinct destination unit (word; byte of a byte board, or 4 of them where its
// rows are 4-byte aligned) and row.  Lanes run along the units of a row, so a wave reads and writes
// consecutive words; a unit belongs to exactly one lane of a launch (gol_edit.h), so the board is
// updated with a plain read-modify-write.  Every lane adds the cells it flipped to a wave sum, and
// one lane per wave adds that to the device counter.
// No LDS, no scratch.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gol_edit.h"
#include "gol_region_kernels.h"

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
        n += gol_edit_paste_unit(FORM, a.g, t, u, gol_edit_row(FORM, a.dst, a.pitch, a.row + r), prow);
    }
    gol_edit_wave_add(n, a.changed);  // (every lane of the wave takes part in the shuffles)
}

}  // namespace

hipError_t golk_paste(const gol_region &r, const uint64_t *pattern, int64_t pstride, int32_t op, uint64_t *changed,
                      hipStream_t s)
{
    EditArgs a{};
    if (!changed || !gol_region_ok(r, op, true, &a.g) || (pattern && !gol_region_stride_ok(r.w, pstride)))
        return hipErrorInvalidValue;
    if (r.rows == 0) return hipSuccess;
    a.dst = r.base;
    a.pitch = r.pitch;
    a.row = r.row;
    a.rows = r.rows;
    a.prow = r.at;
    a.pattern = pattern;
    a.pstride = pstride;
    a.changed = (unsigned long long *)changed;
    dim3 grid;
    if (!gol_edit_grid(a.g.T, r.rows, &grid)) return hipErrorInvalidValue;
    if (a.g.layout == GOL_EDIT_BYTES4) paste_kernel<GOL_EDIT_BYTES4><<<grid, EDIT_BLOCK, 0, s>>>(a);
    else if (a.g.layout == GOL_EDIT_BYTES) paste_kernel<GOL_EDIT_BYTES><<<grid, EDIT_BLOCK, 0, s>>>(a);
    else paste_kernel<GOL_EDIT_STANDARD><<<grid, EDIT_BLOCK, 0, s>>>(a);
    return hipGetLastError();
}
