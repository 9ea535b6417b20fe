// gol_frames.cpp -- reading and editing the board engine's (gol_engine.cpp) board between steps,
// where it is and as it is: the viewport frames (gol_engine_view, _view_counts), their write-side
// twin, the paste (gol_engine_paste), and the reads at cell precision (gol_engine_copy, _bounds).
#include "gol_engine_int.h"

// The tail of a query whose work is queued on the compute streams of the shards in `used`: read
// back their error words, wait for them, and report (and clear) a pending device fault as the other
// queries do.
static int finish_query(gol_engine *e, const std::vector<char> &used)
{
    uint32_t flags = 0;
    for (size_t i = 0; i < e->sh.size(); ++i) {
        if (!used[i]) continue;
        gol_shard &s = e->sh[i];
        RCCHK(set_dev(s.device));
        HIPCHK(hipMemcpyAsync(s.host_word, s.err, sizeof(uint32_t), hipMemcpyDeviceToHost, s.stream));
        HIPCHK(hipStreamSynchronize(s.stream));
        flags |= s.host_word[0];
    }
    return flags ? sync_all(e, false) : GOL_OK;
}

// ------------------------------------------------------------------ viewport frames
// (include/golhip.h, "viewport frames")  The board is read where it is and as it is: no layout
// conversion, no change to cur / band / the halo state, rows [0, R) of the current buffer only
// (never the ghost rows, which an exchange for the next step may be writing).
static int ensure_view(gol_shard &s, int64_t n)
{
    if (s.view_cap >= n) return GOL_OK;
    if (s.view_frame) (void)hipFree(s.view_frame);
    if (s.view_pix) (void)hipFree(s.view_pix);
    if (s.view_host) (void)hipHostFree(s.view_host);
    s.view_frame = nullptr;
    s.view_pix = nullptr;
    s.view_host = nullptr;
    s.view_cap = 0;
    const int64_t cap = std::max<int64_t>((n + 3) / 4 * 4, 1 << 16);  // (golk_view_pixels: 4 pixels per lane)
    HIPCHK(hipMalloc(&s.view_frame, cap * sizeof(uint32_t)));
    HIPCHK(hipMalloc(&s.view_pix, cap));
    HIPCHK(hipHostMalloc((void **)&s.view_host, cap * sizeof(uint32_t), hipHostMallocDefault));
    s.view_cap = cap;
    return GOL_OK;
}

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

// How the board's rows are stored now: what the view, edit and copy kernels take as `form`, and
// what the queries report through *src_layout (the numbers include/golhip.h documents there).
static_assert(GOL_EDIT_BYTES == 0 && GOL_EDIT_STANDARD == 1 && GOL_EDIT_BAND == 2, "*src_layout: 0 bytes, 1 standard, 2 band");
static int board_form(const gol_engine *e)
{
    return e->mode != GOL_MODE_BITS ? GOL_EDIT_BYTES : (e->band ? GOL_EDIT_BAND : GOL_EDIT_STANDARD);
}

// Every local shard counts its runs of the viewport (gol_view_plan) into its own frame and copies
// it to its pinned buffer: the counts, or with `pixels` (one shard holding every row) the pixels.
// used[i]: shard i holds viewport rows.
static int view_render(gol_engine *e, int64_t x0, int64_t y0, int32_t scale, int32_t out_w, int32_t out_h, bool pixels,
                       std::vector<char> &used)
{
    const int64_t n = (int64_t)out_w * out_h, vrows = (int64_t)out_h * scale;
    const int form = board_form(e);
    used.assign(e->sh.size(), 0);
    for (size_t i = 0; i < e->sh.size(); ++i) {
        gol_shard &s = e->sh[i];
        gol_view_run runs[2];
        int32_t nr = 0;
        RCCHK(gol_view_plan(e->H, e->nranks, e->rank + (int32_t)i, y0, vrows, runs, 2, &nr));
        if (nr == 0) continue;
        used[i] = 1;
        RCCHK(set_dev(s.device));
        RCCHK(ensure_view(s, n));
        RCCHK(join_last_step(s));
        HIPCHK(hipMemsetAsync(s.view_frame, 0, (n + 3) / 4 * 4 * sizeof(uint32_t), s.stream));
        const gol_rows b = board_rows(e, s);
        for (int32_t r = 0; r < nr; ++r)
            HIPCHK(golk_view_counts(form, b.ptr, b.pitch, e->W, x0, scale, out_w, runs[r].row, runs[r].rows, runs[r].vrow,
                                    s.view_frame, s.stream));
        if (pixels) {
            HIPCHK(golk_view_pixels(s.view_frame, n, scale, s.view_pix, s.stream));
            HIPCHK(hipMemcpyAsync(s.view_host, s.view_pix, n, hipMemcpyDeviceToHost, s.stream));
        } else {
            HIPCHK(hipMemcpyAsync(s.view_host, s.view_frame, n * sizeof(uint32_t), hipMemcpyDeviceToHost, s.stream));
        }
    }
    return finish_query(e, used);
}

extern "C" int gol_engine_view_counts(gol_engine *e, int64_t x0, int64_t y0, int32_t scale, int32_t out_w, int32_t out_h,
                                      uint32_t *counts, int64_t stride, int32_t *src_layout)
{
    RCCHK(view_check(e, x0, y0, scale, out_w, out_h, counts, stride));
    std::vector<char> used;
    RCCHK(view_render(e, x0, y0, scale, out_w, out_h, false, used));
    for (int64_t j = 0; j < out_h; ++j) {
        uint32_t *dst = counts + j * stride;
        bool first = true;
        for (size_t i = 0; i < e->sh.size(); ++i) {
            if (!used[i]) continue;
            const uint32_t *src = e->sh[i].view_host + j * out_w;
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
    std::vector<char> used;
    RCCHK(view_render(e, x0, y0, scale, out_w, out_h, one, used));
    const uint32_t s2 = (uint32_t)scale * (uint32_t)scale;
    for (int64_t j = 0; j < out_h; ++j) {
        uint8_t *dst = pixels + j * stride;
        if (one) {
            memcpy(dst, (const uint8_t *)e->sh[0].view_host + j * out_w, out_w);
            continue;
        }
        for (int32_t x = 0; x < out_w; ++x) {
            uint32_t c = 0;
            for (size_t i = 0; i < e->sh.size(); ++i)
                if (used[i]) c += e->sh[i].view_host[j * out_w + x];
            dst[x] = (uint8_t)((255u * c + s2 - 1) / s2);
        }
    }
    if (src_layout) *src_layout = board_form(e);
    return GOL_OK;
}

// ------------------------------------------------------------------ board edits
// (include/golhip.h, "board edits")  The write-side twin of the views: the rectangle goes into rows
// [0, R) of the current buffer where they are and as they are -- no layout conversion, no change to
// cur / band / mode / the turn; only the halo becomes stale.
static int ensure_edit(gol_shard &s, int64_t words)
{
    if (s.edit_cap >= words && s.edit_dev && s.edit_host) return GOL_OK;  // (both: one allocation may have failed)
    if (s.edit_dev) (void)hipFree(s.edit_dev);
    if (s.edit_host) (void)hipHostFree(s.edit_host);
    s.edit_dev = nullptr;
    s.edit_host = nullptr;
    s.edit_cap = 0;
    const int64_t cap = std::max<int64_t>(words, 1 << 12);
    HIPCHK(hipMalloc(&s.edit_dev, (1 + cap) * sizeof(uint64_t)));
    HIPCHK(hipHostMalloc((void **)&s.edit_host, (1 + cap) * sizeof(uint64_t), hipHostMallocDefault));
    s.edit_cap = cap;
    return GOL_OK;
}

// A call that failed after it queued copies from or to the pinned buffers of the shards in `used`:
// they end before the call does.  Returns rc.
static int drain_queued(gol_engine *e, const std::vector<char> &used, int rc)
{
    for (size_t i = 0; i < e->sh.size(); ++i)
        if (used[i] && hipSetDevice(e->sh[i].device) == hipSuccess) (void)hipStreamSynchronize(e->sh[i].stream);
    return rc;
}

// One shard's part of a paste, queued on its compute stream: its runs of the rectangle's rows
// (gol_view_plan), then the readback of the counter.
static int paste_enqueue(gol_engine *e, gol_shard &s, const gol_view_run *runs, int32_t nr, int form, int64_t x0, int64_t w,
                         const uint64_t *pattern, int64_t stride, int32_t op)
{
    const int64_t pw = (w + 63) / 64;  // the staged pattern rows are dense
    RCCHK(set_dev(s.device));
    int64_t rows = 0;
    for (int32_t r = 0; r < nr; ++r) rows += runs[r].rows;
    RCCHK(ensure_edit(s, pattern ? rows * pw : 0));
    // as the views (invalidate_halo has queued the waits for an exchange in flight; these cover a
    // step whose exchange was not issued)
    RCCHK(join_last_step(s));
    HIPCHK(hipMemsetAsync(s.edit_dev, 0, sizeof(uint64_t), s.stream));
    if (pattern) {
        uint64_t *dst = s.edit_host + 1;
        for (int32_t r = 0; r < nr; ++r)
            for (int64_t j = 0; j < runs[r].rows; ++j, dst += pw)
                memcpy(dst, pattern + (runs[r].vrow + j) * stride, pw * sizeof(uint64_t));
        HIPCHK(hipMemcpyAsync(s.edit_dev + 1, s.edit_host + 1, rows * pw * sizeof(uint64_t), hipMemcpyHostToDevice, s.stream));
    }
    const gol_rows b = board_rows(e, s);
    int64_t staged = 0;
    for (int32_t r = 0; r < nr; ++r) {
        HIPCHK(golk_paste(form, b.ptr, b.pitch, e->W, x0, w, runs[r].row, runs[r].rows, staged,
                          pattern ? s.edit_dev + 1 : nullptr, pw, op, s.edit_dev, s.stream));
        staged += runs[r].rows;
    }
    HIPCHK(hipMemcpyAsync(s.edit_host, s.edit_dev, sizeof(uint64_t), hipMemcpyDeviceToHost, s.stream));
    return GOL_OK;
}

extern "C" int gol_engine_paste(gol_engine *e, int64_t x0, int64_t y0, int64_t w, int64_t h, const uint64_t *pattern,
                                int64_t stride, int32_t op, int64_t *changed, int32_t *dst_layout)
{
    if (!e) return gol_set_error(GOL_EINVAL, "engine is NULL");
    if (w < 1 || w > e->W || h < 1 || h > e->H || x0 < 0 || x0 >= e->W || y0 < 0 || y0 >= e->H ||
        w > (int64_t(1) << 26) / h || (pattern && stride < (w + 63) / 64) || op < GOL_PASTE_COPY || op > GOL_PASTE_ANDNOT)
        return gol_set_error(GOL_EINVAL,
                             "bad paste (%lld x %lld cells at (%lld, %lld), stride %lld, op %d) into a %lld x %lld board: the "
                             "rectangle within one turn of the torus, at most 2^26 cells, stride >= ceil(w / 64), op 0..3",
                             (long long)w, (long long)h, (long long)x0, (long long)y0, (long long)stride, op, (long long)e->W,
                             (long long)e->H);
    if (e->mode == GOL_MODE_EXACT)
        return gol_set_error(GOL_ESTATE, "the board holds loaded bytes other than 0/255 until turn 1: step once before editing it");
    RCCHK(invalidate_halo(e));
    const int form = board_form(e);
    std::vector<char> used(e->sh.size(), 0);
    int rc = GOL_OK;
    for (size_t i = 0; i < e->sh.size() && rc == GOL_OK; ++i) {
        gol_view_run runs[2];
        int32_t nr = 0;
        rc = gol_view_plan(e->H, e->nranks, e->rank + (int32_t)i, y0, h, runs, 2, &nr);
        if (rc != GOL_OK || nr == 0) continue;
        used[i] = 1;
        rc = paste_enqueue(e, e->sh[i], runs, nr, form, x0, w, pattern, stride, op);
    }
    if (rc != GOL_OK) return drain_queued(e, used, rc);
    RCCHK(finish_query(e, used));
    int64_t n = 0;
    for (size_t i = 0; i < e->sh.size(); ++i)
        if (used[i]) n += (int64_t)e->sh[i].edit_host[0];
    if (changed) *changed = n;
    if (dst_layout) *dst_layout = form;
    return GOL_OK;
}

// ------------------------------------------------------------------ region reads
// (include/golhip.h, "region reads")  The read-side twin of the paste at cell precision: the
// rectangle is read from rows [0, R) of the current buffer where they are and as they are.  A plain
// copy and the bounds change nothing, the halo included; a cut is the copy with the paste's clear
// (paste_enqueue, ANDNOT without a pattern) queued behind it on the same stream.
static constexpr int64_t READ_HDR = 8;  // header words of read_dev / read_host (golk_bounds_rows' hdr in the first 5)

static int ensure_read(gol_shard &s, int64_t words)
{
    if (s.read_cap >= words && s.read_dev && s.read_host) return GOL_OK;  // (both: one allocation may have failed)
    if (s.read_dev) (void)hipFree(s.read_dev);
    if (s.read_host) (void)hipHostFree(s.read_host);
    s.read_dev = nullptr;
    s.read_host = nullptr;
    s.read_cap = 0;
    const int64_t cap = std::max<int64_t>(words, 1 << 12);
    HIPCHK(hipMalloc(&s.read_dev, (READ_HDR + cap) * sizeof(uint64_t)));
    HIPCHK(hipHostMalloc((void **)&s.read_host, (READ_HDR + cap) * sizeof(uint64_t), hipHostMallocDefault));
    s.read_cap = cap;
    return GOL_OK;
}

struct read_runs {
    gol_view_run runs[2];
    int32_t n = 0;
    int64_t rows() const { return (n > 0 ? runs[0].rows : 0) + (n > 1 ? runs[1].rows : 0); }
};

static int region_check(const gol_engine *e, const char *what, int64_t x0, int64_t y0, int64_t w, int64_t h)
{
    if (!e) return gol_set_error(GOL_EINVAL, "engine is NULL");
    if (w < 1 || w > e->W || h < 1 || h > e->H || x0 < 0 || x0 >= e->W || y0 < 0 || y0 >= e->H)
        return gol_set_error(GOL_EINVAL, "bad %s (%lld x %lld cells at (%lld, %lld)) of a %lld x %lld board: the rectangle "
                             "within one turn of the torus", what, (long long)w, (long long)h, (long long)x0, (long long)y0,
                             (long long)e->W, (long long)e->H);
    return GOL_OK;
}

// One shard's part of a copy, queued on its compute stream: the cleared staging (dense rows of
// ceil(w / 64) words, in run order), its runs gathered into it, then the readback of header and rows.
static int copy_enqueue(gol_engine *e, gol_shard &s, const read_runs &rr, int form, int64_t x0, int64_t w)
{
    const int64_t pw = (w + 63) / 64, words = READ_HDR + rr.rows() * pw;
    RCCHK(set_dev(s.device));
    RCCHK(ensure_read(s, rr.rows() * pw));
    RCCHK(join_last_step(s));
    HIPCHK(hipMemsetAsync(s.read_dev, 0, words * sizeof(uint64_t), s.stream));  // (the counter; the halves no lane writes)
    const gol_rows b = board_rows(e, s);
    int64_t staged = 0;
    for (int32_t r = 0; r < rr.n; ++r) {
        HIPCHK(golk_copy(form, b.ptr, b.pitch, e->W, x0, w, rr.runs[r].row, rr.runs[r].rows, staged, s.read_dev + READ_HDR, pw,
                         s.read_dev, s.stream));
        staged += rr.runs[r].rows;
    }
    HIPCHK(hipMemcpyAsync(s.read_host, s.read_dev, words * sizeof(uint64_t), hipMemcpyDeviceToHost, s.stream));
    return GOL_OK;
}

extern "C" int gol_engine_copy(gol_engine *e, int64_t x0, int64_t y0, int64_t w, int64_t h, uint64_t *pattern, int64_t stride,
                               int32_t flags, int64_t *alive, int32_t *src_layout)
{
    RCCHK(region_check(e, "copy", x0, y0, w, h));
    if (!pattern || w > (int64_t(1) << 26) / h || stride < (w + 63) / 64 || (flags & ~GOL_COPY_CUT))
        return gol_set_error(GOL_EINVAL, "bad copy (%lld x %lld cells, pattern %s, stride %lld, flags %d): at most 2^26 cells, "
                             "stride >= ceil(w / 64), flags 0 or GOL_COPY_CUT", (long long)w, (long long)h,
                             pattern ? "given" : "NULL", (long long)stride, flags);
    const bool cut = flags & GOL_COPY_CUT;
    if (cut && e->mode == GOL_MODE_EXACT)
        return gol_set_error(GOL_ESTATE, "the board holds loaded bytes other than 0/255 until turn 1: step once before editing it");
    if (cut) RCCHK(invalidate_halo(e));
    const int form = board_form(e);
    const int64_t pw = (w + 63) / 64;
    std::vector<char> used(e->sh.size(), 0);
    std::vector<read_runs> plan(e->sh.size());
    int rc = GOL_OK;
    for (size_t i = 0; i < e->sh.size() && rc == GOL_OK; ++i) {
        read_runs &rr = plan[i];
        rc = gol_view_plan(e->H, e->nranks, e->rank + (int32_t)i, y0, h, rr.runs, 2, &rr.n);
        if (rc != GOL_OK || rr.n == 0) continue;
        used[i] = 1;
        rc = copy_enqueue(e, e->sh[i], rr, form, x0, w);
        if (rc == GOL_OK && cut)  // behind the read, on the same stream
            rc = paste_enqueue(e, e->sh[i], rr.runs, rr.n, form, x0, w, nullptr, 0, GOL_PASTE_ANDNOT);
    }
    if (rc != GOL_OK) return drain_queued(e, used, rc);
    RCCHK(finish_query(e, used));
    if ((int64_t)e->sh.size() < e->nranks)  // rows of other processes: zero
        for (int64_t r = 0; r < h; ++r) memset(pattern + r * stride, 0, pw * sizeof(uint64_t));
    int64_t n = 0;
    for (size_t i = 0; i < e->sh.size(); ++i) {
        if (!used[i]) continue;
        const uint64_t *src = e->sh[i].read_host + READ_HDR;
        for (int32_t r = 0; r < plan[i].n; ++r)
            for (int64_t j = 0; j < plan[i].runs[r].rows; ++j, src += pw)
                memcpy(pattern + (plan[i].runs[r].vrow + j) * stride, src, pw * sizeof(uint64_t));
        n += (int64_t)e->sh[i].read_host[0];  // (a cut: the cells its clear changed, edit_host[0], are these)
    }
    if (alive) *alive = n;
    if (src_layout) *src_layout = form;
    return GOL_OK;
}

extern "C" int gol_engine_bounds(gol_engine *e, int64_t x0, int64_t y0, int64_t w, int64_t h, int64_t *bx, int64_t *by,
                                 int64_t *bw, int64_t *bh, int64_t *alive, int32_t *src_layout)
{
    RCCHK(region_check(e, "bounds", x0, y0, w, h));
    const int form = board_form(e);
    std::vector<char> used(e->sh.size(), 0);
    int rc = GOL_OK;
    for (size_t i = 0; i < e->sh.size() && rc == GOL_OK; ++i) {
        gol_shard &s = e->sh[i];
        read_runs rr;
        rc = gol_view_plan(e->H, e->nranks, e->rank + (int32_t)i, y0, h, rr.runs, 2, &rr.n);
        if (rc != GOL_OK || rr.n == 0) continue;
        used[i] = 1;
        rc = [&]() -> int {
            const gol_rows b = board_rows(e, s);
            const int64_t T = golk_bounds_lanes(form, b.ptr, b.pitch, e->W, x0, w);
            if (T < 1) return gol_set_error(GOL_EINVAL, "bounds: the board's rows do not take its layout's geometry");
            RCCHK(set_dev(s.device));
            RCCHK(ensure_read(s, (T + 1) / 2));
            RCCHK(join_last_step(s));
            uint32_t *occ = (uint32_t *)(s.read_dev + READ_HDR);  // T column-occupancy words behind the header
            HIPCHK(hipMemsetAsync(s.read_dev, 0, (READ_HDR + (T + 1) / 2) * sizeof(uint64_t), s.stream));
            for (int32_t r = 0; r < rr.n; ++r)
                HIPCHK(golk_bounds_rows(form, b.ptr, b.pitch, e->W, x0, w, rr.runs[r].row, rr.runs[r].rows, rr.runs[r].vrow, occ,
                                        s.read_dev, s.stream));
            HIPCHK(golk_bounds_cols(form, b.ptr, b.pitch, e->W, x0, w, occ, s.read_dev, s.stream));
            HIPCHK(hipMemcpyAsync(s.read_host, s.read_dev, READ_HDR * sizeof(uint64_t), hipMemcpyDeviceToHost, s.stream));
            return GOL_OK;
        }();
    }
    if (rc != GOL_OK) return drain_queued(e, used, rc);
    RCCHK(finish_query(e, used));
    int64_t n = 0, r0 = h, r1 = -1, c0 = w, c1 = -1;
    for (size_t i = 0; i < e->sh.size(); ++i) {
        const uint64_t *hd = e->sh[i].read_host;
        if (!used[i] || hd[0] == 0) continue;
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
    if (src_layout) *src_layout = form;
    return GOL_OK;
}
