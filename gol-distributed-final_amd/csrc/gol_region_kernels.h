// gol_region_kernels.h -- the launchers of the region kernels' units (gol_view.hip, gol_edit.hip,
// gol_copy.hip); internal, not part of the C ABI.  They share one descriptor, gol_region (gol_edit.h,
// which also holds its check and GOL_EDIT_BYTES / _STANDARD / _BAND: how a board's rows are stored);
// a caller that fills one includes that header itself.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

struct gol_region;

// The region kernels: a rectangle of the running board read or edited in place.  Every launcher takes
// a gol_region (gol_edit.h, where its fields, its one check gol_region_ok and the column mapping
// are): hipErrorInvalidValue, nothing launched, unless the check accepts it; hipSuccess at once for
// rows == 0.  Counters and headers are device words the caller zeroes.
// gol_view.hip: adds to `frame` (w / scale uint32 per pixel row, dense) the alive cells of the
// region's rows, which are viewport rows [at, at + rows); viewport cell (c, v) belongs to pixel
// (c / scale, v / scale), 1 <= scale <= 4096, w a multiple of scale.
hipError_t golk_view_counts(const gol_region &r, int32_t scale, uint32_t *frame, hipStream_t s);
// pixels[i] = ceil(255 * frame[i] / scale^2) for i < n; both buffers hold n rounded up to 4
// elements, 16-byte aligned.
hipError_t golk_view_pixels(const uint32_t *frame, int64_t n, int32_t scale, uint8_t *pixels, hipStream_t s);
// gol_edit.hip: pattern rows [at, at + rows) (pstride uint64 words per row; pattern NULL: all ones)
// applied to the region under op (GOL_PASTE_*); *changed += the cells whose state changed.
hipError_t golk_paste(const gol_region &r, const uint64_t *pattern, int64_t pstride, int32_t op, uint64_t *changed,
                      hipStream_t s);
// gol_copy.hip (nothing is written to the board).  golk_copy gathers the region into pattern rows
// [at, at + rows): it writes every 32-bit half that holds a cell c < w, bits at c >= w zero, and no
// other half -- the caller clears the pattern first; *alive += the alive cells gathered.
hipError_t golk_copy(const gol_region &r, uint64_t *pattern, int64_t pstride, uint64_t *alive, hipStream_t s);
// The bounding box of the region's alive cells.  hdr, 5 words: [0] += alive cells, [1] = max of ~v and
// [2] = max of v over the rectangle rows v (at + the row's offset from `row`) that hold one, [3] = max
// of ~c and [4] = max of c over the columns that hold one.  golk_bounds_rows (once per run of rows)
// fills [0 .. 2] and ORs the columns seen into occ: T uint32 words, T the geom.T of gol_region_ok(r,
// GOL_EDIT_COPY, true, .); golk_bounds_cols (once, after them, on a region of the same rows) turns
// occ into [3] and [4].
hipError_t golk_bounds_rows(const gol_region &r, uint32_t *occ, uint64_t *hdr, hipStream_t s);
hipError_t golk_bounds_cols(const gol_region &r, const uint32_t *occ, uint64_t *hdr, hipStream_t s);
