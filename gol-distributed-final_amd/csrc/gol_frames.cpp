// gol_frames.cpp -- reading and editing the board engine's (gol_engine.cpp) board between steps,
// where it is and as it is: the viewport frames (gol_engine_view, _view_counts), their write-side
// twin, the paste (gol_engine_paste), and the reads at cell precision (gol_engine_copy, _bounds).
// All four run the region kernels (gol_region_kernels.h) on rows [0, R) of the current buffer -- never the
// ghost rows, which an exchange for the next step may be writing -- with no layout conversion and
// no change to cur / band / mode / the turn, through one per-shard driver (query_shards).
#include "gol_edit.h"
#include "gol_engine_int.h"
#include "gol_region_kernels.h"

// A shard's runs of a query's rows (gol_view_plan); n == 0: it holds none and takes no part.
struct shard_runs {
    gol_view_run runs[2];
    int32_t n = 0;
    int64_t rows() const { return (n > 0 ? runs[0].rows : 0) + (n > 1 ? runs[1].rows : 0); }
};

// The tail of a query whose work is queued on the compute streams of the shards in `plan`: read
// back their error words, wait for them, and report (and clear) a pending device fault as the other
// queries do.
static int finish_query(gol_engine *e, const std::vector<shard_runs> &plan)
{
    uint32_t flags = 0;
    for (size_t i = 0; i < e->sh.size(); ++i) {
        if (!plan[i].n) continue;
        gol_shard &s = e->sh[i];
        RCCHK(set_dev(s.device));
        HIPCHK(hipMemcpyAsync(s.host_word, s.err, sizeof(uint32_t), hipMemcpyDeviceToHost, s.stream));
        HIPCHK(hipStreamSynchronize(s.stream));
        flags |= s.host_word[0];
    }
    return flags ? sync_all(e, false) : GOL_OK;
}

// A call that failed after it queued copies from or to the pinned buffers of the shards in `plan`:
// they end before the call does.  Returns rc.
static int drain_queued(gol_engine *e, const std::vector<shard_runs> &plan, int rc)
{
    for (size_t i = 0; i < e->sh.size(); ++i)
        if (plan[i].n && hipSetDevice(e->sh[i].device) == hipSuccess) (void)hipStreamSynchronize(e->sh[i].stream);
    return rc;
}

// One query over the local shards: every shard that holds rows of [y0, y0 + h) (mod H) gets
// enqueue(shard, its runs) with its device set, which queues the shard's part on its compute stream
// behind the last step (join_last_step: invalidate_halo has queued the waits for an exchange in
// flight; this covers a step whose exchange was not issued); then the streams are waited for.  A
// failure on the way drains what was queued.  plan[i]: shard i's runs.
template <class Enqueue>
static int query_shards(gol_engine *e, int64_t y0, int64_t h, std::vector<shard_runs> &plan, Enqueue enqueue)
{
    plan.assign(e->sh.size(), shard_runs());
    int rc = GOL_OK;
    for (size_t i = 0; i < e->sh.size() && rc == GOL_OK; ++i) {
        shard_runs &rr = plan[i];
        rc = gol_view_plan(e->H, e->nranks, e->rank + (int32_t)i, y0, h, rr.runs, 2, &rr.n);
        if (rc != GOL_OK) rr.n = 0;
        if (rr.n == 0) continue;
        rc = set_dev(e->sh[i].device);
        if (rc == GOL_OK) rc = join_last_step(e->sh[i]);
        if (rc == GOL_OK) rc = enqueue(e->sh[i], rr);
    }
    return rc != GOL_OK ? drain_queued(e, plan, rc) : finish_query(e, plan);
}

// Room for `words` words in a shard's scratch (the device of the shard set).
static int ensure_scratch(gol_scratch &b, int64_t words)
{
    if (b.cap >= words && b.dev && b.host) return GOL_OK;  // (both: one allocation may have failed)
    if (b.dev) (void)hipFree(b.dev);
    if (b.host) (void)hipHostFree(b.host);
    b = gol_scratch();
    const int64_t cap = std::max<int64_t>(words, 1 << 12);
    HIPCHK(hipMalloc(&b.dev, cap * sizeof(uint64_t)));
    HIPCHK(hipHostMalloc((void **)&b.host, cap * sizeof(uint64_t), hipHostMallocDefault));
    b.cap = cap;
    return GOL_OK;
}

// How the board's rows are stored now: the region kernels' layout, and what the queries report
// through *src_layout (the numbers include/golhip.h documents there).
static_assert(GOL_EDIT_BYTES == 0 && GOL_EDIT_STANDARD == 1 && GOL_EDIT_BAND == 2, "*src_layout: 0 bytes, 1 standard, 2 band");
static int board_form(const gol_engine *e)
{
    return e->mode != GOL_MODE_BITS ? GOL_EDIT_BYTES : (e->band ? GOL_EDIT_BAND : GOL_EDIT_STANDARD);
}

// Columns [x0, x0 + w) of a run of shard s's rows, which are the query's rows from `at`.
static gol_region shard_region(const gol_engine *e, const gol_shard &s, int64_t x0, int64_t w, const gol_view_run &run,
                               int64_t at)
{
    const gol_rows b = board_rows(e, s);
    return {board_form(e), b.ptr, b.pitch, e->W, x0, w, run.row, run.rows, at};
}

// The rectangle of a paste or a read; staged: its cells go through a shard's scratch as pattern rows.
static int region_check(const gol_engine *e, const char *what, int64_t x0, int64_t y0, int64_t w, int64_t h, bool staged)
{
    if (!e) return gol_set_error(GOL_EINVAL, "engine is NULL");
    if (w < 1 || w > e->W || h < 1 || h > e->H || x0 < 0 || x0 >= e->W || y0 < 0 || y0 >= e->H ||
        (staged && w > (int64_t(1) << 26) / h))
        return gol_set_error(GOL_EINVAL, "bad %s (%lld x %lld cells at (%lld, %lld)) of a %lld x %lld board: the rectangle "
                             "within one turn of the torus%s", what, (long long)w, (long long)h, (long long)x0, (long long)y0,
                             (long long)e->W, (long long)e->H, staged ? ", at most 2^26 cells" : "");
    return GOL_OK;
}

// ------------------------------------------------------------------ viewport frames
// (include/golhip.h, "viewport frames")  The view scratch of a shard: the counts of its rows,
// n rounded up to 4 uint32, and behind them as many pixel bytes (golk_view_pixels: 4 pixels per
// lane, both 16-byte aligned); the pinned copy holds whichever of the two the call reads back.
static int view_check(gol_engine *e, int64_t x0, int64_t y0, int32_t scale, int32_t out_w, int32_t out_h, const void *out,
                      int64_t stride)
{
    if (!e || !out) return gol_set_error(GOL_EINVAL, "bad view arguments (NULL)");
    if (scale < 1 || scale > 4096 || out_w < 1 || out_h < 1 || (int64_t)out_w * scale > e->W ||
        (int64_t)out_h * scale > e->H || x0 < 0 || x0 >= e->W || y0 < 0 || y0 >= e->H ||
        (int64_t)out_w * out_h > (int64_t(1) << 26) || stride < out_w)
        return gol_set_error(GOL_EINVAL,
                             "bad view (x0 %lld, y0 %lld, scale %d, %d x %d pixels, stride %lld) of a %lld x %lld board: "
                             "1 <= scale <= 4096, the viewport within one turn of the torus, at most 2^26 pixels",
                             (long long)x0, (long long)y0, scale, out_w, out_h, (long long)stride, (long long)e->W,
                             (long long)e->H);
    return GOL_OK;
}

// Every local shard counts its runs of the viewport into its own frame and copies it to its pinned
// buffer: the counts, or with `pixels` (one shard holding every row) the pixels.
static int view_render(gol_engine *e, int64_t x0, int64_t y0, int32_t scale, int32_t out_w, int32_t out_h, bool pixels,
                       std::vector<shard_runs> &plan)
{
    const int64_t n = (int64_t)out_w * out_h, n4 = (n + 3) / 4 * 4;
    return query_shards(e, y0, (int64_t)out_h * scale, plan, [&](gol_shard &s, const shard_runs &rr) -> int {
        RCCHK(ensure_scratch(s.view, (n4 * 5 + 7) / 8));
        uint32_t *frame = (uint32_t *)s.view.dev;
        uint8_t *pix = (uint8_t *)(frame + n4);
        HIPCHK(hipMemsetAsync(frame, 0, n4 * sizeof(uint32_t), s.stream));
        for (int32_t r = 0; r < rr.n; ++r)
            HIPCHK(golk_view_counts(shard_region(e, s, x0, (int64_t)out_w * scale, rr.runs[r], rr.runs[r].vrow), scale, frame,
                                    s.stream));
        if (pixels) HIPCHK(golk_view_pixels(frame, n, scale, pix, s.stream));
        HIPCHK(hipMemcpyAsync(s.view.host, pixels ? (const void *)pix : frame, pixels ? n : n * sizeof(uint32_t),
                              hipMemcpyDeviceToHost, s.stream));
        return GOL_OK;
    });
}

extern "C" int gol_engine_view_counts(gol_engine *e, int64_t x0, int64_t y0, int32_t scale, int32_t out_w, int32_t out_h,
                                      uint32_t *counts, int64_t stride, int32_t *src_layout)
{
    RCCHK(view_check(e, x0, y0, scale, out_w, out_h, counts, stride));
    std::vector<shard_runs> plan;
    RCCHK(view_render(e, x0, y0, scale, out_w, out_h, false, plan));
    for (int64_t j = 0; j < out_h; ++j) {
        uint32_t *dst = counts + j * stride;
        bool first = true;
        for (size_t i = 0; i < e->sh.size(); ++i) {
            if (!plan[i].n) continue;
            const uint32_t *src = (const uint32_t *)e->sh[i].view.host + j * out_w;
            if (first) memcpy(dst, src, out_w * sizeof(uint32_t));
            else
                for (int32_t x = 0; x < out_w; ++x) dst[x] += src[x];
            first = false;
        }
        if (first) memset(dst, 0, out_w * sizeof(uint32_t));  // none of this process's rows are in view
    }
    if (src_layout) *src_layout = board_form(e);
    return GOL_OK;
}

extern "C" int gol_engine_view(gol_engine *e, int64_t x0, int64_t y0, int32_t scale, int32_t out_w, int32_t out_h,
                               uint8_t *pixels, int64_t stride, int32_t *src_layout)
{
    RCCHK(view_check(e, x0, y0, scale, out_w, out_h, pixels, stride));
    if (e->sh.front().y0 != 0 || e->sh.back().y1 != e->H)
        return gol_set_error(GOL_EINVAL, "view needs every row in this process (it holds rows [%lld, %lld)): add the "
                                         "ranks' view_counts frames", (long long)e->sh.front().y0, (long long)e->sh.back().y1);
    const bool one = e->sh.size() == 1;  // the pixels on the device; several shards: from the summed counts
    std::vector<shard_runs> plan;
    RCCHK(view_render(e, x0, y0, scale, out_w, out_h, one, plan));
    const uint32_t s2 = (uint32_t)scale * (uint32_t)scale;
    for (int64_t j = 0; j < out_h; ++j) {
        uint8_t *dst = pixels + j * stride;
        if (one) {
            memcpy(dst, (const uint8_t *)e->sh[0].view.host + j * out_w, out_w);
            continue;
        }
        for (int32_t x = 0; x < out_w; ++x) {
            uint32_t c = 0;
            for (size_t i = 0; i < e->sh.size(); ++i)
                if (plan[i].n) c += ((const uint32_t *)e->sh[i].view.host)[j * out_w + x];
            dst[x] = (uint8_t)((255u * c + s2 - 1) / s2);
        }
    }
    if (src_layout) *src_layout = board_form(e);
    return GOL_OK;
}

// ------------------------------------------------------------------ board edits
// (include/golhip.h, "board edits")  The write-side twin of the views; only the halo becomes stale.
// The edit scratch of a shard: word 0 the changed-cells counter, then the staged pattern rows (dense
// rows of ceil(w / 64) words, in run order).
// One shard's part of a paste, queued on its compute stream: its runs of the rectangle's rows, then
// the readback of the counter.
static int paste_enqueue(gol_engine *e, gol_shard &s, const shard_runs &rr, int64_t x0, int64_t w, const uint64_t *pattern,
                         int64_t stride, int32_t op)
{
    const int64_t pw = (w + 63) / 64, words = pattern ? rr.rows() * pw : 0;
    RCCHK(ensure_scratch(s.edit, 1 + words));
    HIPCHK(hipMemsetAsync(s.edit.dev, 0, sizeof(uint64_t), s.stream));
    if (pattern) {
        uint64_t *dst = s.edit.host + 1;
        for (int32_t r = 0; r < rr.n; ++r)
            for (int64_t j = 0; j < rr.runs[r].rows; ++j, dst += pw)
                memcpy(dst, pattern + (rr.runs[r].vrow + j) * stride, pw * sizeof(uint64_t));
        HIPCHK(hipMemcpyAsync(s.edit.dev + 1, s.edit.host + 1, words * sizeof(uint64_t), hipMemcpyHostToDevice, s.stream));
    }
    int64_t staged = 0;
    for (int32_t r = 0; r < rr.n; ++r) {
        HIPCHK(golk_paste(shard_region(e, s, x0, w, rr.runs[r], staged), pattern ? s.edit.dev + 1 : nullptr, pw, op, s.edit.dev,
                          s.stream));
        staged += rr.runs[r].rows;
    }
    HIPCHK(hipMemcpyAsync(s.edit.host, s.edit.dev, sizeof(uint64_t), hipMemcpyDeviceToHost, s.stream));
    return GOL_OK;
}

extern "C" int gol_engine_paste(gol_engine *e, int64_t x0, int64_t y0, int64_t w, int64_t h, const uint64_t *pattern,
                                int64_t stride, int32_t op, int64_t *changed, int32_t *dst_layout)
{
    RCCHK(region_check(e, "paste", x0, y0, w, h, true));
    if ((pattern && !gol_region_stride_ok(w, stride)) || op < GOL_PASTE_COPY || op > GOL_PASTE_ANDNOT)
        return gol_set_error(GOL_EINVAL, "bad paste (stride %lld of %lld cells, op %d): stride >= ceil(w / 64), op 0..3",
                             (long long)stride, (long long)w, op);
    if (e->mode == GOL_MODE_EXACT)
        return gol_set_error(GOL_ESTATE, "the board holds loaded bytes other than 0/255 until turn 1: step once before editing it");
    RCCHK(invalidate_halo(e));
    std::vector<shard_runs> plan;
    RCCHK(query_shards(e, y0, h, plan, [&](gol_shard &s, const shard_runs &rr) {
        return paste_enqueue(e, s, rr, x0, w, pattern, stride, op);
    }));
    int64_t n = 0;
    for (size_t i = 0; i < e->sh.size(); ++i)
        if (plan[i].n) n += (int64_t)e->sh[i].edit.host[0];
    if (changed) *changed = n;
    if (dst_layout) *dst_layout = board_form(e);
    return GOL_OK;
}

// ------------------------------------------------------------------ region reads
// (include/golhip.h, "region reads")  The read-side twin of the paste at cell precision.  A plain
// copy and the bounds change nothing, the halo included; a cut is the copy with the paste's clear
// (paste_enqueue, ANDNOT without a pattern) queued behind it on the same stream, so the read scratch
// is not the edit scratch.  The read scratch of a shard: READ_HDR header words (the alive counter;
// golk_bounds_rows' hdr in the first 5), then the copy's staged pattern rows (as the paste's) or the
// bounds' column-occupancy words.
static constexpr int64_t READ_HDR = 8;

extern "C" int gol_engine_copy(gol_engine *e, int64_t x0, int64_t y0, int64_t w, int64_t h, uint64_t *pattern, int64_t stride,
                               int32_t flags, int64_t *alive, int32_t *src_layout)
{
    RCCHK(region_check(e, "copy", x0, y0, w, h, true));
    if (!pattern || !gol_region_stride_ok(w, stride) || (flags & ~GOL_COPY_CUT))
        return gol_set_error(GOL_EINVAL, "bad copy (pattern %s, stride %lld of %lld cells, flags %d): stride >= ceil(w / 64), "
                             "flags 0 or GOL_COPY_CUT", pattern ? "given" : "NULL", (long long)stride, (long long)w, flags);
    const bool cut = flags & GOL_COPY_CUT;
    if (cut && e->mode == GOL_MODE_EXACT)
        return gol_set_error(GOL_ESTATE, "the board holds loaded bytes other than 0/255 until turn 1: step once before editing it");
    if (cut) RCCHK(invalidate_halo(e));
    const int64_t pw = (w + 63) / 64;
    std::vector<shard_runs> plan;
    RCCHK(query_shards(e, y0, h, plan, [&](gol_shard &s, const shard_runs &rr) -> int {
        const int64_t words = READ_HDR + rr.rows() * pw;
        RCCHK(ensure_scratch(s.read, words));
        HIPCHK(hipMemsetAsync(s.read.dev, 0, words * sizeof(uint64_t), s.stream));  // (the counter; the halves no lane writes)
        int64_t staged = 0;
        for (int32_t r = 0; r < rr.n; ++r) {
            HIPCHK(golk_copy(shard_region(e, s, x0, w, rr.runs[r], staged), s.read.dev + READ_HDR, pw, s.read.dev, s.stream));
            staged += rr.runs[r].rows;
        }
        HIPCHK(hipMemcpyAsync(s.read.host, s.read.dev, words * sizeof(uint64_t), hipMemcpyDeviceToHost, s.stream));
        return cut ? paste_enqueue(e, s, rr, x0, w, nullptr, 0, GOL_PASTE_ANDNOT) : GOL_OK;  // behind the read
    }));
    if ((int64_t)e->sh.size() < e->nranks)  // rows of other processes: zero
        for (int64_t r = 0; r < h; ++r) memset(pattern + r * stride, 0, pw * sizeof(uint64_t));
    int64_t n = 0;
    for (size_t i = 0; i < e->sh.size(); ++i) {
        if (!plan[i].n) continue;
        const uint64_t *src = e->sh[i].read.host + READ_HDR;
        for (int32_t r = 0; r < plan[i].n; ++r)
            for (int64_t j = 0; j < plan[i].runs[r].rows; ++j, src += pw)
                memcpy(pattern + (plan[i].runs[r].vrow + j) * stride, src, pw * sizeof(uint64_t));
        n += (int64_t)e->sh[i].read.host[0];  // (a cut: the cells its clear changed, edit.host[0], are these)
    }
    if (alive) *alive = n;
    if (src_layout) *src_layout = board_form(e);
    return GOL_OK;
}

extern "C" int gol_engine_bounds(gol_engine *e, int64_t x0, int64_t y0, int64_t w, int64_t h, int64_t *bx, int64_t *by,
                                 int64_t *bw, int64_t *bh, int64_t *alive, int32_t *src_layout)
{
    RCCHK(region_check(e, "bounds", x0, y0, w, h, false));
    std::vector<shard_runs> plan;
    RCCHK(query_shards(e, y0, h, plan, [&](gol_shard &s, const shard_runs &rr) -> int {
        gol_edit_geom g;  // g.T lanes: as many column-occupancy words behind the header
        const gol_region all = shard_region(e, s, x0, w, rr.runs[0], rr.runs[0].vrow);
        if (!gol_region_ok(all, GOL_EDIT_COPY, true, &g))
            return gol_set_error(GOL_EINVAL, "bounds: the board's rows do not take its layout's geometry");
        const int64_t words = READ_HDR + (g.T + 1) / 2;
        RCCHK(ensure_scratch(s.read, words));
        uint32_t *occ = (uint32_t *)(s.read.dev + READ_HDR);
        HIPCHK(hipMemsetAsync(s.read.dev, 0, words * sizeof(uint64_t), s.stream));
        for (int32_t r = 0; r < rr.n; ++r)
            HIPCHK(golk_bounds_rows(shard_region(e, s, x0, w, rr.runs[r], rr.runs[r].vrow), occ, s.read.dev, s.stream));
        HIPCHK(golk_bounds_cols(all, occ, s.read.dev, s.stream));
        HIPCHK(hipMemcpyAsync(s.read.host, s.read.dev, READ_HDR * sizeof(uint64_t), hipMemcpyDeviceToHost, s.stream));
        return GOL_OK;
    }));
    int64_t n = 0, r0 = h, r1 = -1, c0 = w, c1 = -1;
    for (size_t i = 0; i < e->sh.size(); ++i) {
        const uint64_t *hd = e->sh[i].read.host;
        if (!plan[i].n || hd[0] == 0) continue;
        n += (int64_t)hd[0];
        r0 = std::min(r0, (int64_t)~hd[1]);
        r1 = std::max(r1, (int64_t)hd[2]);
        c0 = std::min(c0, (int64_t)~hd[3]);
        c1 = std::max(c1, (int64_t)hd[4]);
    }
    if (bx) *bx = n ? c0 : 0;
    if (by) *by = n ? r0 : 0;
    if (bw) *bw = n ? c1 - c0 + 1 : 0;
    if (bh) *bh = n ? r1 - r0 + 1 : 0;
    if (alive) *alive = n;
    if (src_layout) *src_layout = board_form(e);
    return GOL_OK;
}
