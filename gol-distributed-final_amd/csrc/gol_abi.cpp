// gol_abi.cpp -- C ABI of libgolhip.so: library entry points, the worker's slab
// step, the row partition and the device launchers (include/golhip.h).  The
// board engine (one GPU or row shards) is gol_engine.cpp and the files it names.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "gol_batch.h"
#include "gol_batch_kernels.h"
#include "gol_engine_int.h"
#include "gol_island.h"
#include "gol_rule.h"
#include "gol_step_kernels.h"
#include "gol_util_kernels.h"

// ------------------------------------------------------------------ errors
static thread_local std::string g_err;

int gol_set_error(int code, const char *fmt, ...)
{
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_err = buf;
    return code;
}

extern "C" int gol_abi_version(void) { return GOL_ABI_VERSION; }
extern "C" const char *gol_last_error(void) { return g_err.c_str(); }

extern "C" int gol_device_count(int *n)
{
    if (!n) return gol_set_error(GOL_EINVAL, "n is NULL");
    int c = 0;
    HIPCHK(hipGetDeviceCount(&c));
    *n = c;
    return GOL_OK;
}

extern "C" int gol_partition_rows(int64_t H, int64_t parts, int64_t i, int64_t *y0, int64_t *y1)
{
    if (!y0 || !y1 || parts <= 0 || i < 0 || i >= parts || H < 0)
        return gol_set_error(GOL_EINVAL, "bad partition arguments H=%lld parts=%lld i=%lld", (long long)H,
                             (long long)parts, (long long)i);
    // broker.go:135-139 (even) and broker.go:172-206 (first H%T slabs get one extra row)
    const int64_t base = H / parts, rem = H % parts;
    *y0 = i * base + std::min(i, rem);
    *y1 = *y0 + base + (i < rem ? 1 : 0);
    return GOL_OK;
}

// ------------------------------------------------------------------ worker path
extern "C" int gol_next_state_slab(const uint8_t *world, int64_t H, int64_t W, int64_t stride, int64_t y0,
                                   int64_t y1, uint8_t *out, int64_t out_stride)
{
    if (!world || !out || H <= 0 || W <= 0 || stride < W || out_stride < W || y0 < 0 || y1 > H || y0 > y1)
        return gol_set_error(GOL_EINVAL, "bad slab arguments H=%lld W=%lld y0=%lld y1=%lld", (long long)H,
                             (long long)W, (long long)y0, (long long)y1);
    if (y0 == y1) return GOL_OK;
    const int64_t ds = (W + 15) / 16 * 16;
    uint8_t *dworld = nullptr, *dout = nullptr;
    hipStream_t s = nullptr;
    int rc = GOL_OK;
    auto fail = [&](hipError_t e, const char *what) {
        rc = gol_set_error(GOL_EHIP, "%s: %s", what, hipGetErrorString(e));
    };
    hipError_t e;
    if ((e = hipStreamCreateWithFlags(&s, hipStreamNonBlocking)) != hipSuccess) { fail(e, "stream"); return rc; }
    if ((e = hipMalloc(&dworld, H * ds)) != hipSuccess) fail(e, "hipMalloc world");
    else if ((e = hipMalloc(&dout, (y1 - y0) * ds)) != hipSuccess) fail(e, "hipMalloc slab");
    else if ((e = hipMemcpy2DAsync(dworld, ds, world, stride, W, H, hipMemcpyHostToDevice, s)) != hipSuccess)
        fail(e, "copy in");
    else if ((e = golk_bytes_step(dworld, H, W, ds, y0, y1, dout, ds, s)) != hipSuccess) fail(e, "launch");
    else if ((e = hipMemcpy2DAsync(out, out_stride, dout, ds, W, y1 - y0, hipMemcpyDeviceToHost, s)) != hipSuccess)
        fail(e, "copy out");
    else if ((e = hipStreamSynchronize(s)) != hipSuccess) fail(e, "sync");
    if (dworld) (void)hipFree(dworld);
    if (dout) (void)hipFree(dout);
    (void)hipStreamDestroy(s);
    return rc;
}

// ------------------------------------------------------------------ device launchers
#define LAUNCH(expr)                                                                                      \
    do {                                                                                                  \
        hipError_t e_ = (expr);                                                                           \
        if (e_ != hipSuccess) return gol_set_error(GOL_EHIP, "%s: %s", #expr, hipGetErrorString(e_));     \
        return GOL_OK;                                                                                    \
    } while (0)

// The step entries: each resolves cells_per_lane to words per lane, fills a descriptor
// (gol_step_launch.h) and answers as gol_step_launch_ok does for a C entry, with its own text.
// step_launch: the part they share, a pretended device (cus, slots; 0, 0: this one) and the launch.
static int step_launch(gol_step_launch l, void *stream, int32_t cus, int32_t slots)
{
    l.as_cus = cus;
    l.as_slots = slots;
    if ((cus || slots) && !gol_step_launch_ok(l, true))
        return gol_set_error(GOL_EINVAL, "a pretended device (%d CUs, %d resident workgroups) needs the pipelined k, cus %% 8 == 0 and both > 0", cus, slots);
    const hipError_t e = golk_step(l, (hipStream_t)stream);
    if (e == hipErrorInvalidValue && cus) {  // the device has less (gol_launch.cpp pipe_device): nothing was launched
        int dcus = 0;
        int64_t dslots = 0;
        const gol_step_geometry g = gol_step_geometry_of(l);
        if (!golk_pipe_limits(l.family == GOL_FAMILY_BAND, g.contig, l.slots != nullptr, &dcus, &dslots))
            return gol_set_error(GOL_EHIP, "no device properties");
        return gol_set_error(GOL_EINVAL, "a pretended device of %d CUs and %d resident workgroups exceeds this one (%d, %lld)", cus,
                             slots, dcus, (long long)dslots);
    }
    if (e != hipSuccess) return gol_set_error(GOL_EHIP, "step launch: %s", hipGetErrorString(e));
    return GOL_OK;
}

extern "C" int gol_dev_bits_step(const uint32_t *top, const uint32_t *mid, const uint32_t *bot, uint32_t *dst,
                                 int64_t R, int64_t Wd, int64_t pitch, int64_t row0, int64_t rows, int32_t k,
                                 int32_t cells_per_lane, int32_t strip_rows, uint64_t *count_slots, void *stream)
{
    const int dw = gol_step_dw(GOL_FAMILY_BITS, cells_per_lane);
    const gol_step_launch l = {GOL_FAMILY_BITS, top, mid, bot, dst, R, Wd, pitch, row0, rows, k, dw, strip_rows, 0, 0, count_slots};
    if (!gol_step_launch_ok(l, true))
        return gol_set_error(GOL_EINVAL, "bad bits_step arguments (R=%lld Wd=%lld pitch=%lld k=%d dw=%d)",
                             (long long)R, (long long)Wd, (long long)pitch, k, dw);
    return step_launch(l, stream, 0, 0);
}

extern "C" int gol_dev_band_step_on(const uint32_t *top, const uint32_t *mid, const uint32_t *bot, uint32_t *dst,
                                    int64_t R, int64_t Wd, int64_t pitch, int64_t row0, int64_t rows, int32_t k,
                                    int32_t cells_per_lane, int32_t strip_rows, uint64_t *count_slots, void *stream,
                                    int32_t cus, int32_t slots)
{
    const gol_step_launch l = {GOL_FAMILY_BAND, top, mid, bot, dst, R, Wd, pitch, row0, rows, k,
                               gol_step_dw(GOL_FAMILY_BAND, cells_per_lane), strip_rows, 0, 0, count_slots};
    if (!gol_step_launch_ok(l, true))
        return gol_set_error(GOL_EINVAL, "bad band_step arguments (R=%lld Wd=%lld pitch=%lld k=%d cells_per_lane=%d)",
                             (long long)R, (long long)Wd, (long long)pitch, k, cells_per_lane);
    return step_launch(l, stream, cus, slots);
}

extern "C" int gol_dev_band_step(const uint32_t *top, const uint32_t *mid, const uint32_t *bot, uint32_t *dst,
                                 int64_t R, int64_t Wd, int64_t pitch, int64_t row0, int64_t rows, int32_t k,
                                 int32_t cells_per_lane, int32_t strip_rows, uint64_t *count_slots, void *stream)
{
    return gol_dev_band_step_on(top, mid, bot, dst, R, Wd, pitch, row0, rows, k, cells_per_lane, strip_rows, count_slots,
                                stream, 0, 0);
}

extern "C" int gol_dev_rule_step(const uint32_t *top, const uint32_t *mid, const uint32_t *bot, uint32_t *dst,
                                 int64_t R, int64_t Wd, int64_t pitch, int64_t row0, int64_t rows, int32_t k,
                                 int32_t layout, uint32_t birth, uint32_t survive, int32_t cells_per_lane,
                                 int32_t strip_rows, uint64_t *count_slots, void *stream)
{
    // (a layout that is neither: no family, which the check refuses)
    const int family = layout == GOL_LAYOUT_STANDARD ? GOL_FAMILY_RULE_STD : (layout == GOL_LAYOUT_BAND ? GOL_FAMILY_RULE_BAND : -1);
    const gol_step_launch l = {family, top, mid, bot, dst, R, Wd, pitch, row0, rows, k, gol_step_dw(family, cells_per_lane),
                               strip_rows, birth, survive, count_slots};
    if (!gol_step_launch_ok(l, true))
        return gol_set_error(GOL_EINVAL,
                             "bad rule_step arguments (R=%lld Wd=%lld pitch=%lld k=%d layout=%d B=0x%x S=0x%x cells_per_lane=%d)",
                             (long long)R, (long long)Wd, (long long)pitch, k, layout, birth, survive, cells_per_lane);
    return step_launch(l, stream, 0, 0);
}

extern "C" int gol_band_max_k(int32_t cells_per_lane)
{
    return gol_step_max_k(GOL_FAMILY_BAND, gol_step_dw(GOL_FAMILY_BAND, cells_per_lane), GOL_STEP_MAX_K, true);
}

extern "C" int gol_dev_band_convert(int32_t to_band, const uint32_t *src, uint32_t *dst, int64_t rows, int64_t Wd,
                                    int64_t src_pitch, int64_t dst_pitch, void *stream)
{
    if (!src || !dst || src == dst || rows < 0 || Wd <= 0 || Wd % 32 || src_pitch < Wd || dst_pitch < Wd ||
        (to_band ? dst_pitch : src_pitch) % 4 || (((uintptr_t)(to_band ? dst : src)) & 15))
        return gol_set_error(GOL_EINVAL, "bad band_convert arguments (Wd=%lld)", (long long)Wd);
    LAUNCH(golk_band_convert(to_band != 0, src, dst, rows, Wd, src_pitch, dst_pitch, (hipStream_t)stream));
}

extern "C" int gol_dev_random_fill(uint32_t *dst, int64_t rows, int64_t grow0, int64_t W, int64_t pitch,
                                   uint64_t seed, void *stream)
{
    if (!dst || rows < 0 || grow0 < 0 || W <= 0 || W % 64 || pitch < W / 32 || pitch % 2)
        return gol_set_error(GOL_EINVAL, "bad random_fill arguments");
    LAUNCH(golk_random_fill(dst, rows, grow0, W, pitch, seed, (hipStream_t)stream));
}

extern "C" int gol_dev_popcount(const uint32_t *src, int64_t rows, int64_t Wd, int64_t pitch, uint64_t *slots,
                                void *stream)
{
    if (!src || !slots || rows < 0 || Wd <= 0 || pitch < Wd) return gol_set_error(GOL_EINVAL, "bad popcount arguments");
    LAUNCH(golk_popcount(src, rows, Wd, pitch, slots, (hipStream_t)stream));
}

extern "C" int gol_dev_hash(const uint32_t *src, int64_t rows, int64_t grow0, int64_t Wd, int64_t pitch,
                            uint64_t *slots, void *stream)
{
    if (!src || !slots || rows < 0 || grow0 < 0 || Wd <= 0 || Wd % 2 || pitch < Wd || pitch % 2)
        return gol_set_error(GOL_EINVAL, "bad hash arguments");
    LAUNCH(golk_hash(src, rows, grow0, Wd, pitch, slots, (hipStream_t)stream));
}

extern "C" int gol_dev_pack(const uint8_t *bytes, int64_t rows, int64_t W, int64_t stride, uint32_t *bits,
                            int64_t pitch, uint32_t *nonbinary, void *stream)
{
    if (!bytes || !bits || rows < 0 || W <= 0 || W % 32 || stride < W || pitch < W / 32)
        return gol_set_error(GOL_EINVAL, "bad pack arguments");
    LAUNCH(golk_pack(bytes, rows, W, stride, bits, pitch, nonbinary, (hipStream_t)stream));
}

extern "C" int gol_dev_unpack(const uint32_t *bits, int64_t rows, int64_t W, int64_t pitch, uint8_t *bytes,
                              int64_t stride, void *stream)
{
    if (!bytes || !bits || rows < 0 || W <= 0 || W % 32 || stride < W || pitch < W / 32)
        return gol_set_error(GOL_EINVAL, "bad unpack arguments");
    LAUNCH(golk_unpack(bits, rows, W, pitch, bytes, stride, (hipStream_t)stream));
}

extern "C" int gol_dev_bytes_step_k_on(const uint8_t *top, const uint8_t *mid, const uint8_t *bot, uint8_t *dst,
                                       int64_t R, int64_t W, int64_t stride, int64_t row0, int64_t rows, int32_t k,
                                       int32_t strip_rows, uint64_t *count_slots, void *stream, int32_t cus,
                                       int32_t slots)
{
    const gol_step_launch l = {GOL_FAMILY_BYTES, top, mid, bot, dst, R, W, stride, row0, rows, k, 1, strip_rows, 0, 0, count_slots};
    if (!gol_step_launch_ok(l, true))
        return gol_set_error(GOL_EINVAL, "bad bytes_step_k arguments (R=%lld W=%lld stride=%lld k=%d)",
                             (long long)R, (long long)W, (long long)stride, k);
    return step_launch(l, stream, cus, slots);
}

extern "C" int gol_dev_bytes_step_k(const uint8_t *top, const uint8_t *mid, const uint8_t *bot, uint8_t *dst,
                                    int64_t R, int64_t W, int64_t stride, int64_t row0, int64_t rows, int32_t k,
                                    int32_t strip_rows, uint64_t *count_slots, void *stream)
{
    return gol_dev_bytes_step_k_on(top, mid, bot, dst, R, W, stride, row0, rows, k, strip_rows, count_slots, stream, 0, 0);
}

extern "C" int gol_dev_pipe_limits(int32_t kernel, int32_t contiguous, int32_t counted, int32_t *cus, int32_t *slots)
{
    if (!cus || !slots || (kernel != GOL_STRIP_KERNEL_BAND && kernel != GOL_STRIP_KERNEL_BYTES))
        return gol_set_error(GOL_EINVAL, "bad pipe_limits arguments (kernel %d)", kernel);
    int c = 0;
    int64_t n = 0;
    if (!golk_pipe_limits(kernel == GOL_STRIP_KERNEL_BAND, contiguous != 0, counted != 0, &c, &n))
        return gol_set_error(GOL_EHIP, "no device properties");
    *cus = c;
    *slots = (int32_t)n;
    return GOL_OK;
}

extern "C" int gol_dev_bytes_step(const uint8_t *world, int64_t H, int64_t W, int64_t stride, int64_t y0,
                                  int64_t y1, uint8_t *out, int64_t out_stride, void *stream)
{
    if (!world || !out || H <= 0 || W <= 0 || stride < W || out_stride < W || y0 < 0 || y1 > H || y0 > y1)
        return gol_set_error(GOL_EINVAL, "bad bytes_step arguments");
    LAUNCH(golk_bytes_step(world, H, W, stride, y0, y1, out, out_stride, (hipStream_t)stream));
}

extern "C" int gol_dev_batch_retire(const int32_t *list_in, int32_t *counts, const int64_t *found, int64_t n, int64_t t0,
                                    int64_t t_now, int64_t t_end, int32_t *active, int32_t *finish, int64_t *left, void *stream)
{
    if (!list_in || !counts || !found || !active || !finish || !left || !gol_batch_shape_ok(n, 1, 1) || t0 < 0 || t0 > t_now ||
        t_now > t_end)
        return gol_set_error(GOL_EINVAL, "bad batch_retire arguments (n %lld, turns %lld <= %lld <= %lld, or NULL)", (long long)n,
                             (long long)t0, (long long)t_now, (long long)t_end);
    LAUNCH(golk_batch_retire(list_in, counts, found, n, t0, t_now, t_end, active, finish, left, (hipStream_t)stream));
}

extern "C" int gol_dev_batch_restock(int32_t *active, int32_t *counts, int64_t *found_age, int64_t *born, int32_t *soup, int64_t n,
                                     int64_t now, int64_t horizon, int64_t total, int64_t *out_found, int64_t *out_period,
                                     int32_t *harvest, void *stream)
{
    if (!active || !counts || !found_age || !born || !soup || !out_found || !out_period || !harvest ||
        !gol_batch_shape_ok(n, 1, 1) || now < 0 || horizon < 0 || total < 0 || total > ((int64_t)1 << 26))
        return gol_set_error(GOL_EINVAL, "bad batch_restock arguments (n %lld, now %lld, horizon %lld, total %lld, or NULL)",
                             (long long)n, (long long)now, (long long)horizon, (long long)total);
    LAUNCH(golk_batch_restock(active, counts, found_age, born, soup, n, now, horizon, total, out_found, out_period, harvest,
                              (hipStream_t)stream));
}

extern "C" int gol_dev_batch_step(uint64_t *boards, uint64_t *prev, int64_t *settled, int64_t n, int64_t H, int64_t W, int32_t turns,
                                  int64_t turn0, int32_t have_prev, int32_t write_prev, uint32_t birth, uint32_t survive,
                                  const uint32_t *rules, int32_t scan, int64_t done, const int32_t *list, const int32_t *count,
                                  int64_t slots, int64_t *left, const int64_t *born, void *stream)
{
    const gol_batch_launch l = {boards, prev, settled, n, H, W, turns, turn0, have_prev != 0, write_prev != 0, birth, survive,
                                rules, scan, done, list, count, slots, left, born};
    const hipError_t e = golk_batch_step(l, (hipStream_t)stream);
    if (e == hipErrorInvalidValue)  // gol_batch_launch_ok said no: nothing was launched
        return gol_set_error(GOL_EINVAL, "bad batch_step arguments (n %lld, %lld x %lld, %d turns, scan %d, done %lld, slots %lld, or a pointer)",
                             (long long)n, (long long)H, (long long)W, turns, scan, (long long)done, (long long)slots);
    if (e != hipSuccess) return gol_set_error(GOL_EHIP, "batch_step: %s", hipGetErrorString(e));
    return GOL_OK;
}

extern "C" int gol_dev_batch_step_map(uint64_t *boards, uint64_t *prev, int64_t *settled, int64_t n, int64_t H, int64_t W,
                                      int32_t turns, int64_t turn0, int32_t have_prev, int32_t write_prev, const uint32_t *maps,
                                      int32_t map_each, int32_t scan, int64_t done, const int32_t *list, const int32_t *count,
                                      int64_t slots, int64_t *left, const int64_t *born, void *stream)
{
    const gol_batch_launch l = {boards, prev, settled, n, H, W, turns, turn0, have_prev != 0, write_prev != 0, 0, 0,
                                nullptr, scan, done, list, count, slots, left, born, maps, map_each != 0};
    // (without maps it would be the launch of gol_dev_batch_step under B/S, which is not this entry's)
    const hipError_t e = maps ? golk_batch_step(l, (hipStream_t)stream) : hipErrorInvalidValue;
    if (e == hipErrorInvalidValue)  // gol_batch_launch_ok said no: nothing was launched
        return gol_set_error(GOL_EINVAL,
                             "bad batch_step_map arguments (n %lld, %lld x %lld, %d turns, scan %d, done %lld, slots %lld, map_each %d, or a "
                             "pointer)",
                             (long long)n, (long long)H, (long long)W, turns, scan, (long long)done, (long long)slots, map_each);
    if (e != hipSuccess) return gol_set_error(GOL_EHIP, "batch_step_map: %s", hipGetErrorString(e));
    return GOL_OK;
}

extern "C" int gol_dev_batch_islands_sym(const uint64_t *boards, int64_t n, int64_t H, int64_t W, int32_t reach, int32_t symmetry,
                                         int64_t cap, int64_t *count, gol_island *islands, uint64_t *fingerprint, void *stream)
{
    const gol_island_launch l = {boards, n, H, W, reach, symmetry, cap, count, islands, fingerprint};
    const hipError_t e = golk_batch_islands(l, (hipStream_t)stream);
    if (e == hipErrorInvalidValue)  // gol_island_launch_ok said no: nothing was launched
        return gol_set_error(GOL_EINVAL,
                             "bad batch_islands arguments (n %lld, %lld x %lld, reach %d, symmetry %d, cap %lld, or a pointer)",
                             (long long)n, (long long)H, (long long)W, reach, symmetry, (long long)cap);
    if (e != hipSuccess) return gol_set_error(GOL_EHIP, "batch_islands: %s", hipGetErrorString(e));
    return GOL_OK;
}

extern "C" int gol_dev_batch_islands(const uint64_t *boards, int64_t n, int64_t H, int64_t W, int32_t reach, int64_t cap,
                                     int64_t *count, gol_island *islands, uint64_t *fingerprint, void *stream)
{
    return gol_dev_batch_islands_sym(boards, n, H, W, reach, GOL_ISLAND_FIXED, cap, count, islands, fingerprint, stream);
}

extern "C" int gol_dev_batch_islands_tally_sym(const uint64_t *boards, int64_t n, int64_t H, int64_t W, int32_t reach,
                                               int32_t symmetry, const int32_t *pairs, const int32_t *pair_count, int64_t max_pairs,
                                               const int64_t *found, int64_t owner0, int64_t *count, uint64_t *fingerprint,
                                               gol_island_kind *table, int32_t table_log2, int64_t *dropped, void *stream)
{
    const gol_island_launch l = {boards, n, H, W, reach, symmetry, 0, count, nullptr, fingerprint, table, table_log2, dropped, owner0,
                                 pairs, pair_count, max_pairs, found};
    // (a NULL table would be the plain launch, which is not this entry's)
    const hipError_t e = table ? golk_batch_islands(l, (hipStream_t)stream) : hipErrorInvalidValue;
    if (e == hipErrorInvalidValue)  // gol_island_launch_ok said no: nothing was launched
        return gol_set_error(GOL_EINVAL,
                             "bad batch_islands_tally arguments (n %lld, %lld x %lld, reach %d, symmetry %d, table 2^%d, owner0 %lld, %lld "
                             "pairs, or a pointer)",
                             (long long)n, (long long)H, (long long)W, reach, symmetry, table_log2, (long long)owner0,
                             (long long)max_pairs);
    if (e != hipSuccess) return gol_set_error(GOL_EHIP, "batch_islands_tally: %s", hipGetErrorString(e));
    return GOL_OK;
}

extern "C" int gol_dev_batch_islands_tally(const uint64_t *boards, int64_t n, int64_t H, int64_t W, int32_t reach,
                                           const int32_t *pairs, const int32_t *pair_count, int64_t max_pairs, const int64_t *found,
                                           int64_t owner0, int64_t *count, uint64_t *fingerprint, gol_island_kind *table,
                                           int32_t table_log2, int64_t *dropped, void *stream)
{
    return gol_dev_batch_islands_tally_sym(boards, n, H, W, reach, GOL_ISLAND_FIXED, pairs, pair_count, max_pairs, found, owner0, count,
                                           fingerprint, table, table_log2, dropped, stream);
}

extern "C" int gol_dev_island_table_clear(gol_island_kind *table, int32_t table_log2, int64_t *dropped, void *stream)
{
    const hipError_t e = golk_island_table_clear(table, table_log2, dropped, (hipStream_t)stream);
    if (e == hipErrorInvalidValue)
        return gol_set_error(GOL_EINVAL, "bad island_table_clear arguments (table 2^%d in 4..24, or a pointer)", table_log2);
    if (e != hipSuccess) return gol_set_error(GOL_EHIP, "island_table_clear: %s", hipGetErrorString(e));
    return GOL_OK;
}

extern "C" int gol_dev_error(int32_t device, uint32_t *flags)
{
    if (!flags) return gol_set_error(GOL_EINVAL, "flags is NULL");
    int dev = device;
    if (dev < 0) HIPCHK(hipGetDevice(&dev));
    int prev = 0;
    HIPCHK(hipGetDevice(&prev));
    uint32_t *w = golk_device_err_word(dev);
    if (!w) return gol_set_error(GOL_EHIP, "no error word on device %d", dev);
    HIPCHK(hipSetDevice(dev));
    uint32_t v = 0;
    hipError_t he = hipMemcpy(&v, w, sizeof v, hipMemcpyDeviceToHost);
    if (he == hipSuccess && v) he = hipMemset(w, 0, sizeof v);
    if (he == hipSuccess && v) he = golk_reset_claims_device(dev);  // a timed-out pair may have left its claims set
    (void)hipSetDevice(prev);
    if (he != hipSuccess) return gol_set_error(GOL_EHIP, "error word: %s", hipGetErrorString(he));
    *flags = v;
    if (v) return gol_set_error(GOL_EHIP, "device fault in a launch on device %d (error flags 0x%x)", dev, v);
    return GOL_OK;
}

// ------------------------------------------------------------------ rules (host only)
extern "C" int gol_rule_parse(const char *text, uint32_t *birth, uint32_t *survive)
{
    if (!text || !birth || !survive) return gol_set_error(GOL_EINVAL, "bad rule_parse arguments (NULL)");
    const char *p = text;
    uint32_t m[2] = {0, 0};
    for (int half = 0; half < 2; ++half) {
        const char want = half == 0 ? 'B' : 'S';
        if (*p != want && *p != want + ('a' - 'A'))
            return gol_set_error(GOL_EINVAL, "rule \"%s\": expected B<digits>/S<digits>", text);
        for (++p; *p >= '0' && *p <= '8'; ++p) {
            const uint32_t bit = 1u << (*p - '0');
            if (m[half] & bit) return gol_set_error(GOL_EINVAL, "rule \"%s\": digit %c repeated", text, *p);
            m[half] |= bit;
        }
        if (half == 0 && *p++ != '/') return gol_set_error(GOL_EINVAL, "rule \"%s\": expected B<digits>/S<digits>, digits 0-8", text);
    }
    if (*p) return gol_set_error(GOL_EINVAL, "rule \"%s\": expected B<digits>/S<digits>, digits 0-8, nothing after", text);
    *birth = m[0];
    *survive = m[1];
    return GOL_OK;
}

extern "C" int gol_rule_format(uint32_t birth, uint32_t survive, char *buf, int64_t len)
{
    if (!buf || birth >= 512 || survive >= 512) return gol_set_error(GOL_EINVAL, "bad rule_format arguments (masks are 9 bits)");
    char out[24];
    int n = 0;
    out[n++] = 'B';
    for (int d = 0; d <= 8; ++d)
        if (birth >> d & 1u) out[n++] = (char)('0' + d);
    out[n++] = '/';
    out[n++] = 'S';
    for (int d = 0; d <= 8; ++d)
        if (survive >> d & 1u) out[n++] = (char)('0' + d);
    out[n++] = 0;
    if (len < n) return gol_set_error(GOL_EINVAL, "rule_format: the buffer holds %lld bytes, the text needs %d", (long long)len, n);
    memcpy(buf, out, n);
    return GOL_OK;
}

extern "C" int gol_rule_eval_host(uint32_t birth, uint32_t survive, const uint32_t nb[8], uint32_t centre, uint32_t *next)
{
    if (!nb || !next || birth >= 512 || survive >= 512) return gol_set_error(GOL_EINVAL, "bad rule_eval_host arguments");
    // the kernels' count: the 3x3 block as three rows' horizontal sums, the centre in the middle one
    const uint32_t in[3][3] = {{nb[0], nb[1], nb[2]}, {nb[3], centre, nb[4]}, {nb[5], nb[6], nb[7]}};
    uint32_t h0[3], h1[3], t0, t1, t2, t3;
    for (int r = 0; r < 3; ++r) {
        h0[r] = gol_rule_xor3(in[r][0], in[r][1], in[r][2]);
        h1[r] = gol_rule_maj(in[r][0], in[r][1], in[r][2]);
    }
    gol_rule_sum3(h0[0], h1[0], h0[1], h1[1], h0[2], h1[2], t0, t1, t2, t3);
    *next = gol_rule_next(birth, survive, t0, t1, t2, t3, centre);
    return GOL_OK;
}
