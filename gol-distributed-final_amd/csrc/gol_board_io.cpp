// gol_board_io.cpp -- the board engine's (gol_engine.cpp) data in and out: loads from bytes, a
// seed, a PGM file or bit-packed words, stores to the same, the PGM stream, and the cell lists.
#include <fcntl.h>
#include <sys/stat.h>
#include <unistd.h>
#include <functional>

#include "gol_engine_int.h"
#include "gol_util_kernels.h"

// ------------------------------------------------------------------ load
// After the bit rows of every shard were packed with s.flag set on bytes other than 0/255:
// the global decision (every shard, every rank) whether turn 1 must run on the bytes.
static int any_nonbinary(gol_engine *e, bool *out)
{
    uint32_t f = 0;
    for (auto &s : e->sh) {
        RCCHK(set_dev(s.device));
        if (several(e)) RCCHK(e->comm->allreduce_max_u32(s.flag, 1, s.stream));
        HIPCHK(hipMemcpyAsync(s.host_word + 1, s.flag, sizeof(uint32_t), hipMemcpyDeviceToHost, s.stream));
    }
    for (auto &s : e->sh) {
        RCCHK(set_dev(s.device));
        HIPCHK(hipStreamSynchronize(s.stream));
        f |= s.host_word[1];
    }
    *out = f != 0;
    return GOL_OK;
}

static int reset_board_state(gol_engine *e)
{
    RCCHK(invalidate_halo(e));
    e->turn = 0;
    e->band = false;
    e->cur = 0;
    e->bcur = 0;
    return GOL_OK;
}

// A row source of a load: makes board rows [y, y + n) (no torus wrap, n <= s.stage_rows) readable
// by a copy on s.stream at *rows, *stride bytes apart.  `keep`: they are being kept as bytes for
// the exact first turn, not packed.
using row_source = std::function<int(gol_shard &s, int64_t y, int64_t n, bool keep, const uint8_t **rows, int64_t *stride)>;

// Load a bit-capable board from `src`: pack every shard's rows into its bit board, and if any
// byte of the board (every shard, every rank) is neither 0 nor 255 keep rows y0-1 .. y1 as bytes
// for the exact first turn (worker.go:26-37; e->mode says which).
static int load_rows(gol_engine *e, const row_source &src)
{
    const uint8_t *rows = nullptr;
    int64_t stride = 0;
    for (auto &s : e->sh) {
        RCCHK(set_dev(s.device));
        RCCHK(ensure_staging(e, s));
        HIPCHK(hipMemsetAsync(s.flag, 0, sizeof(uint32_t), s.stream));
        for (int64_t y = s.y0; y < s.y1; y += s.stage_rows) {
            const int64_t n = std::min(s.stage_rows, s.y1 - y);
            RCCHK(src(s, y, n, false, &rows, &stride));
            HIPCHK(hipMemcpy2DAsync(s.staging, e->bstride, rows, stride, e->W, n, hipMemcpyHostToDevice, s.stream));
            HIPCHK(golk_pack(s.staging, n, e->W, e->bstride, s.bits[0] + (y - s.y0) * e->pitch, e->pitch, s.flag, s.stream));
        }
    }
    bool nonbinary = false;
    RCCHK(any_nonbinary(e, &nonbinary));
    if (!nonbinary) {
        for (auto &s : e->sh) free_exact_bytes(s);
        e->mode = GOL_MODE_BITS;
        return GOL_OK;
    }
    for (auto &s : e->sh) {
        RCCHK(set_dev(s.device));
        free_exact_bytes(s);
        HIPCHK(hipMalloc(&s.bytes[0], (s.R + 2) * e->bstride));
        HIPCHK(hipMalloc(&s.bytes[1], s.R * e->bstride));
        // shard rows -1 .. R in runs that do not wrap: the row above, the shard's own, the row below
        for (int64_t i = -1, n; i < s.R + 1; i += n) {
            n = i < 0 || i == s.R ? 1 : std::min(s.stage_rows, s.R - i);
            RCCHK(src(s, (s.y0 + i + e->H) % e->H, n, true, &rows, &stride));
            HIPCHK(hipMemcpy2DAsync(s.bytes[0] + (i + 1) * e->bstride, e->bstride, rows, stride, e->W, n, hipMemcpyHostToDevice,
                                    s.stream));
        }
        HIPCHK(hipStreamSynchronize(s.stream));
    }
    e->mode = GOL_MODE_EXACT;
    return GOL_OK;
}

extern "C" int gol_engine_load_bytes(gol_engine *e, const uint8_t *world, int64_t stride)
{
    if (!e || !world || stride < e->W) return gol_set_error(GOL_EINVAL, "bad load arguments");
    RCCHK(reset_board_state(e));
    if (e->mode == GOL_MODE_BYTES || !e->bit_capable) {  // one shard, byte board
        gol_shard &s = e->sh[0];
        RCCHK(set_dev(s.device));
        HIPCHK(hipMemcpy2DAsync(s.bytes[0], e->bstride, world, stride, e->W, e->H, hipMemcpyHostToDevice, s.stream));
        HIPCHK(hipMemsetAsync(s.flag, 0, sizeof(uint32_t), s.stream));
        HIPCHK(golk_nonbinary(s.bytes[0], e->H, e->W, e->bstride, s.flag, s.stream));
        HIPCHK(hipMemcpyAsync(s.host_word + 1, s.flag, sizeof(uint32_t), hipMemcpyDeviceToHost, s.stream));
        HIPCHK(hipStreamSynchronize(s.stream));
        e->bytes_binary = s.host_word[1] == 0;
        e->mode = GOL_MODE_BYTES;
        return GOL_OK;
    }
    return load_rows(e, [&](gol_shard &, int64_t y, int64_t, bool, const uint8_t **rows, int64_t *rstride) -> int {
        *rows = world + y * stride;  // the caller's board, where it is
        *rstride = stride;
        return GOL_OK;
    });
}

extern "C" int gol_engine_load_random(gol_engine *e, uint64_t seed)
{
    if (!e) return gol_set_error(GOL_EINVAL, "engine is NULL");
    if (e->W % 64 != 0) return gol_set_error(GOL_EINVAL, "random boards need W %% 64 == 0");
    RCCHK(reset_board_state(e));
    if (!e->bit_capable) {  // GOL_LAYOUT_BYTES: the same cells as 0/255 bytes (fill bits, then unpack)
        gol_shard &s = e->sh[0];
        RCCHK(set_dev(s.device));
        uint32_t *bits = nullptr;
        HIPCHK(hipMalloc((void **)&bits, e->H * e->pitch * sizeof(uint32_t)));
        hipError_t err = golk_random_fill(bits, e->H, 0, e->W, e->pitch, seed, s.stream);
        if (err == hipSuccess) err = golk_unpack(bits, e->H, e->W, e->pitch, s.bytes[0], e->bstride, s.stream);
        if (err == hipSuccess) err = hipStreamSynchronize(s.stream);
        const hipError_t ferr = hipFree(bits);
        HIPCHK(err);
        HIPCHK(ferr);
        e->bytes_binary = true;
        e->mode = GOL_MODE_BYTES;
        return GOL_OK;
    }
    for (auto &s : e->sh) {
        RCCHK(set_dev(s.device));
        free_exact_bytes(s);
        HIPCHK(golk_random_fill(s.bits[0], s.R, s.y0, e->W, e->pitch, seed, s.stream));
    }
    e->mode = GOL_MODE_BITS;
    return sync_all(e);
}
static int pread_all(int fd, void *buf, size_t n, int64_t off)
{
    uint8_t *p = (uint8_t *)buf;
    while (n > 0) {
        const ssize_t r = pread(fd, p, n, off);
        if (r <= 0) return gol_set_error(GOL_EIO, "short read at offset %lld", (long long)off);
        p += r;
        n -= (size_t)r;
        off += r;
    }
    return GOL_OK;
}

// The raster at file offset `data` of fd (W*H bytes: checked), streamed through the pinned staging.
static int load_pgm_impl(gol_engine *e, int fd, int64_t data)
{
    const char *const short_raster = "pixel data shorter than W*H (a whitespace byte ends the field)";
    RCCHK(reset_board_state(e));
    if (e->mode == GOL_MODE_BYTES || !e->bit_capable) {  // one shard, small byte board
        std::vector<uint8_t> all(e->H * e->W);
        RCCHK(pread_all(fd, all.data(), all.size(), data));
        for (uint8_t c : all)
            if (gol_pgm_is_space(c)) return gol_set_error(GOL_EFORMAT, "%s", short_raster);
        return gol_engine_load_bytes(e, all.data(), e->W);
    }
    // a whitespace byte (the reference's strings.Fields split would end the raster there) is neither
    // 0 nor 255, so it can only be in a board whose rows are kept: looked for there
    uint32_t ws = 0;
    const gol_mode before = e->mode;
    RCCHK(load_rows(e, [&](gol_shard &s, int64_t y, int64_t n, bool keep, const uint8_t **rows, int64_t *stride) -> int {
        HIPCHK(hipStreamSynchronize(s.stream));  // the pinned rows are free again
        RCCHK(pread_all(fd, s.host_staging, (size_t)(n * e->W), data + y * e->W));
        if (keep)
            for (int64_t x = 0; x < n * e->W; ++x) ws |= gol_pgm_is_space(s.host_staging[x]);
        *rows = s.host_staging;
        *stride = e->W;
        return GOL_OK;
    }));
    if (e->mode != GOL_MODE_EXACT) return GOL_OK;
    if (several(e)) {  // agree on the verdict
        gol_shard &s = e->sh[0];
        s.host_word[2] = ws;
        HIPCHK(hipMemcpyAsync(s.flag, s.host_word + 2, sizeof(uint32_t), hipMemcpyHostToDevice, s.stream));
        RCCHK(e->comm->allreduce_max_u32(s.flag, 1, s.stream));
        HIPCHK(hipMemcpyAsync(s.host_word + 2, s.flag, sizeof(uint32_t), hipMemcpyDeviceToHost, s.stream));
        HIPCHK(hipStreamSynchronize(s.stream));
        ws = s.host_word[2];
    }
    if (ws) {
        for (auto &s : e->sh) free_exact_bytes(s);
        e->mode = before;
        return gol_set_error(GOL_EFORMAT, "%s", short_raster);
    }
    return GOL_OK;
}

extern "C" int gol_engine_load_pgm(gol_engine *e, const char *path)
{
    if (!e || !path) return gol_set_error(GOL_EINVAL, "bad arguments");
    const int fd = open(path, O_RDONLY);
    if (fd < 0) return gol_set_error(GOL_EIO, "cannot open %s", path);
    uint8_t head[4096];
    const ssize_t got = pread(fd, head, sizeof head, 0);
    struct stat st;
    int64_t off = 0;
    int rc = got > 0 ? gol_pgm_parse_header(head, (size_t)got, e->W, e->H, &off) : gol_set_error(GOL_EFORMAT, "Not a pgm file");
    if (rc == GOL_OK && (fstat(fd, &st) != 0 || st.st_size < off + e->H * e->W))
        rc = gol_set_error(GOL_EFORMAT, "pixel data shorter than W*H");
    if (rc == GOL_OK) rc = load_pgm_impl(e, fd, off);
    close(fd);
    return rc;
}

// ------------------------------------------------------------------ store / list / PGM
// Rows [a, b) (global) of shard s as bytes into host `out` (pitch stride), chunked.
static int shard_rows_to_host(gol_engine *e, gol_shard &s, int64_t a, int64_t b, uint8_t *out, int64_t stride)
{
    RCCHK(set_dev(s.device));
    const gol_rows br = board_rows(e, s);
    if (!br.bits) {
        HIPCHK(hipMemcpy2DAsync(out, stride, br.bytes() + (a - br.gy0) * br.pitch, br.pitch, e->W, b - a, hipMemcpyDeviceToHost,
                                s.stream));
    } else {
        RCCHK(ensure_staging(e, s));
        for (int64_t y = a; y < b; y += s.stage_rows) {
            const int64_t n = std::min(s.stage_rows, b - y);
            HIPCHK(golk_unpack(br.words() + (y - br.gy0) * br.pitch, n, e->W, br.pitch, s.staging, e->bstride, s.stream));
            HIPCHK(hipMemcpy2DAsync(out + (y - a) * stride, stride, s.staging, e->bstride, e->W, n, hipMemcpyDeviceToHost,
                                    s.stream));
        }
    }
    HIPCHK(hipStreamSynchronize(s.stream));
    return GOL_OK;
}

extern "C" int gol_engine_store_rows(gol_engine *e, int64_t y0, int64_t y1, uint8_t *out, int64_t stride)
{
    if (!e || !out || stride < e->W || y0 < 0 || y1 > e->H || y0 > y1) return gol_set_error(GOL_EINVAL, "bad store arguments");
    if (y0 < e->sh.front().y0 || y1 > e->sh.back().y1)
        return gol_set_error(GOL_EINVAL, "rows [%lld, %lld) are not held by this process (rows [%lld, %lld))", (long long)y0,
                             (long long)y1, (long long)e->sh.front().y0, (long long)e->sh.back().y1);
    RCCHK(ensure_standard(e));
    for (auto &s : e->sh) {
        const int64_t a = std::max(y0, s.y0), b = std::min(y1, s.y1);
        if (a < b) RCCHK(shard_rows_to_host(e, s, a, b, out + (a - y0) * stride, stride));
    }
    return GOL_OK;
}

extern "C" int gol_engine_store_bytes(gol_engine *e, uint8_t *out, int64_t stride)
{
    if (!e) return gol_set_error(GOL_EINVAL, "engine is NULL");
    return gol_engine_store_rows(e, 0, e->H, out, stride);
}

// Row-major (x, y) list of the cells of the rows `b` of shard s that are alive (prev == NULL) or
// whose alive state differs from `prev` (rows of the same form and pitch): per-row counts -> host
// exclusive scan -> one wave per row.  Writes min(total, cap) pairs, *n = total.
static int list_cells(gol_shard &s, const gol_rows &b, const void *prev, int32_t *xy, int64_t cap, int64_t *n)
{
    RCCHK(set_dev(s.device));
    int64_t *dcounts = nullptr;
    int32_t *dxy = nullptr;
    std::vector<int64_t> counts(std::max<int64_t>(b.rows, 1));
    HIPCHK(hipMalloc(&dcounts, counts.size() * sizeof(int64_t)));
    hipError_t he = golk_row_counts(b.bits, b.ptr, prev, b.rows, b.units, b.pitch, dcounts, s.stream);
    if (he == hipSuccess)
        he = hipMemcpyAsync(counts.data(), dcounts, b.rows * sizeof(int64_t), hipMemcpyDeviceToHost, s.stream);
    if (he == hipSuccess) he = hipStreamSynchronize(s.stream);
    int64_t total = 0;
    if (he == hipSuccess) {
        for (int64_t y = 0; y < b.rows; ++y) {  // exclusive prefix -> first index of each row
            const int64_t v = counts[y];
            counts[y] = total;
            total += v;
        }
        *n = total;
    }
    const int64_t m = std::min(total, cap);
    if (he == hipSuccess && m > 0) {
        he = hipMemcpyAsync(dcounts, counts.data(), b.rows * sizeof(int64_t), hipMemcpyHostToDevice, s.stream);
        if (he == hipSuccess) he = hipMalloc(&dxy, m * 2 * sizeof(int32_t));
        if (he == hipSuccess) he = golk_alive_list(b.bits, b.ptr, prev, b.rows, b.units, b.pitch, dcounts, dxy, m, b.gy0, s.stream);
        if (he == hipSuccess) he = hipMemcpyAsync(xy, dxy, m * 2 * sizeof(int32_t), hipMemcpyDeviceToHost, s.stream);
        if (he == hipSuccess) he = hipStreamSynchronize(s.stream);
    }
    (void)hipFree(dcounts);
    if (dxy) (void)hipFree(dxy);
    if (he != hipSuccess) return gol_set_error(GOL_EHIP, "cell list: %s", hipGetErrorString(he));
    return GOL_OK;
}

// The shards' lists (of rows(s) against prev(s)) one after the other in xy, under the running cap.
template <typename Rows, typename Prev>
static int list_shards(gol_engine *e, int32_t *xy, int64_t cap, int64_t *n, Rows rows, Prev prev)
{
    int64_t total = 0;
    for (auto &s : e->sh) {
        int64_t got = 0;
        const int64_t room = std::max<int64_t>(0, cap - total);
        RCCHK(list_cells(s, rows(s), prev(s), room > 0 ? xy + 2 * total : nullptr, room, &got));
        total += got;
    }
    *n = total;
    return GOL_OK;
}

extern "C" int gol_engine_alive_cells(gol_engine *e, int32_t *xy, int64_t cap, int64_t *n)
{
    if (!e || !n || cap < 0 || (cap > 0 && !xy)) return gol_set_error(GOL_EINVAL, "bad arguments");
    RCCHK(ensure_standard(e));
    return list_shards(e, xy, cap, n, [&](gol_shard &s) { return board_rows(e, s); }, [](gol_shard &) { return nullptr; });
}

extern "C" int gol_engine_step_flips(gol_engine *e, int32_t *xy, int64_t cap, int64_t *n)
{
    if (!e || !n || cap < 0 || (cap > 0 && !xy)) return gol_set_error(GOL_EINVAL, "bad arguments");
    RCCHK(rule_step_check(e));
    RCCHK(agree_step_state(e));
    RCCHK(ensure_standard(e));
    auto current = [&](gol_shard &s) { return board_rows(e, s); };
    if (e->mode == GOL_MODE_BITS) {
        // one standard-layout turn; the previous generation stays in the other buffer
        RCCHK(launch_k(e, 1, -1));
        e->turn += 1;
        RCCHK(sync_all(e));
        return list_shards(e, xy, cap, n, current, [&](gol_shard &s) { return s.bits[1 - e->cur]; });
    }
    if (e->mode == GOL_MODE_EXACT) {
        // turn 1 from the loaded bytes: compare the new state (unpacked) with the loaded bytes
        RCCHK(exact_turn(e));
        e->turn += 1;
        for (auto &s : e->sh) {
            RCCHK(set_dev(s.device));
            HIPCHK(golk_unpack(s.bits[e->cur], s.R, e->W, e->pitch, s.bytes[1], e->bstride, s.stream));
        }
        RCCHK(list_shards(
            e, xy, cap, n, [&](gol_shard &s) { return gol_rows{s.bytes[1], false, s.R, e->W, e->bstride, s.y0}; },
            [&](gol_shard &s) { return s.bytes[0] + e->bstride; }));
        return sync_all(e);  // frees the byte rows
    }
    // byte board (W % 64 != 0): one shard; the previous bytes stay in the other buffer
    RCCHK(advance(e, 1, -1));
    RCCHK(sync_all(e));
    return list_shards(e, xy, cap, n, current, [&](gol_shard &s) { return s.bytes[1 - e->bcur]; });
}

// writePgmImage's byte stream (gol/io.go:52-81): the header (rank 0) and this process's rows at
// their file offsets, chunk by chunk (device unpack -> pinned staging), into `sink`.
static int pgm_stream(gol_engine *e, gol_write_fn sink, void *user, int64_t *hlen_out)
{
    RCCHK(ensure_standard(e));
    char header[96];
    const int hlen = gol_pgm_format_header(header, sizeof header, e->W, e->H);
    *hlen_out = hlen;
    const bool coll = several(e);
    if (!coll || e->rank == 0) {
        if (sink(user, 0, (const uint8_t *)header, hlen) != 0) return gol_set_error(GOL_EIO, "the PGM sink failed (header)");
    }
    for (auto &s : e->sh) {
        RCCHK(set_dev(s.device));
        RCCHK(ensure_staging(e, s));
        const gol_rows b = board_rows(e, s);
        const int64_t r0 = b.gy0, r1 = b.gy0 + b.rows;
        if (!b.bits || s.stage_rows < 2) {
            for (int64_t y = r0; y < r1; y += s.stage_rows) {
                const int64_t n = std::min(s.stage_rows, r1 - y);
                RCCHK(shard_rows_to_host(e, s, y, y + n, s.host_staging, e->W));
                if (sink(user, hlen + y * e->W, s.host_staging, n * e->W) != 0)
                    return gol_set_error(GOL_EIO, "the PGM sink failed at row %lld", (long long)y);
            }
            continue;
        }
        // bit board: two halves of the staging buffers; chunk i+1 is unpacked and copied to the
        // host while the sink consumes chunk i
        const int64_t half = s.stage_rows / 2;
        hipEvent_t done[2] = {nullptr, nullptr};
        int rc = GOL_OK;
        for (auto &d : done)
            if (rc == GOL_OK && hipEventCreateWithFlags(&d, hipEventDisableTiming) != hipSuccess)
                rc = gol_set_error(GOL_EHIP, "event for the PGM stream");
        auto enqueue = [&](int64_t y, int h) -> int {
            const int64_t n = std::min(half, r1 - y);
            uint8_t *dst = s.staging + h * half * e->bstride;
            HIPCHK(golk_unpack(b.words() + (y - b.gy0) * b.pitch, n, e->W, b.pitch, dst, e->bstride, s.stream));
            HIPCHK(hipMemcpy2DAsync(s.host_staging + h * half * e->W, e->W, dst, e->bstride, e->W, n, hipMemcpyDeviceToHost,
                                    s.stream));
            HIPCHK(hipEventRecord(done[h], s.stream));
            return GOL_OK;
        };
        if (rc == GOL_OK) rc = enqueue(r0, 0);
        for (int64_t y = r0, i = 0; y < r1 && rc == GOL_OK; y += half, ++i) {
            const int h = (int)(i & 1);
            if (y + half < r1) rc = enqueue(y + half, 1 - h);  // the other half's sink call has returned
            if (rc == GOL_OK && hipEventSynchronize(done[h]) != hipSuccess) rc = gol_set_error(GOL_EHIP, "PGM stream copy");
            if (rc == GOL_OK && sink(user, hlen + y * e->W, s.host_staging + h * half * e->W, std::min(half, r1 - y) * e->W) != 0)
                rc = gol_set_error(GOL_EIO, "the PGM sink failed at row %lld", (long long)y);
        }
        (void)hipStreamSynchronize(s.stream);
        for (auto d : done)
            if (d) (void)hipEventDestroy(d);
        RCCHK(rc);
    }
    return GOL_OK;
}

static int fd_sink(void *user, int64_t off, const uint8_t *data, int64_t len)
{
    const int fd = *static_cast<int *>(user);
    while (len > 0) {
        const ssize_t w = pwrite(fd, data, (size_t)len, off);
        if (w <= 0) return -1;
        data += w;
        len -= w;
        off += w;
    }
    return 0;
}

extern "C" int gol_engine_write_pgm_to(gol_engine *e, gol_write_fn sink, void *user)
{
    if (!e || !sink) return gol_set_error(GOL_EINVAL, "bad arguments");
    int64_t hlen = 0;
    int rc = pgm_stream(e, sink, user, &hlen);
    if (e->rank_mode && e->nranks > 1) {
        const int rb = rank_barrier(e);  // every rank's rows are in its sink when any rank returns
        if (rc == GOL_OK) rc = rb;
    }
    return rc;
}

extern "C" int gol_engine_write_pgm(gol_engine *e, const char *path)
{
    if (!e || !path) return gol_set_error(GOL_EINVAL, "bad arguments");
    const bool coll = several(e);
    int rc = GOL_OK;
    if (!coll || e->rank == 0) {
        const int hlen = gol_pgm_format_header(nullptr, 0, e->W, e->H);
        const int fd = open(path, O_WRONLY | O_CREAT | O_TRUNC, 0644);
        if (fd < 0) rc = gol_set_error(GOL_EIO, "cannot create %s", path);
        else {
            if (ftruncate(fd, hlen + e->H * e->W) != 0) rc = gol_set_error(GOL_EIO, "cannot size %s", path);
            if (close(fd) != 0 && rc == GOL_OK) rc = gol_set_error(GOL_EIO, "close %s", path);
        }
    }
    if (coll) {
        const int rb = rank_barrier(e);  // the file exists and is sized before any rank writes
        if (rc == GOL_OK) rc = rb;
    }
    int fd = rc == GOL_OK ? open(path, O_WRONLY) : -1;
    if (rc == GOL_OK && fd < 0) rc = gol_set_error(GOL_EIO, "cannot open %s", path);
    int64_t hlen = 0;
    if (rc == GOL_OK) {
        rc = pgm_stream(e, fd_sink, &fd, &hlen);
        if (rc == GOL_EIO) gol_set_error(GOL_EIO, "short write to %s", path);
    }
    if (fd >= 0 && close(fd) != 0 && rc == GOL_OK) rc = gol_set_error(GOL_EIO, "close %s", path);
    if (coll) {
        const int rb = rank_barrier(e);  // every rank's rows are written when any rank returns
        if (rc == GOL_OK) rc = rb;
    }
    return rc;
}

// ------------------------------------------------------------------ bit-packed rows in / out
static int rows_check(gol_engine *e, int64_t y0, int64_t y1, const void *p, int64_t stride)
{
    if (!e || !p || y0 < 0 || y1 > e->H || y0 > y1 || stride < e->W / 64)
        return gol_set_error(GOL_EINVAL, "bad word-row arguments");
    if (!e->bit_capable) return gol_set_error(GOL_EINVAL, "bit-packed rows need a bit board (W %% 64 == 0, layout not BYTES)");
    if (y0 < e->sh.front().y0 || y1 > e->sh.back().y1)
        return gol_set_error(GOL_EINVAL, "rows [%lld, %lld) are not held by this process", (long long)y0, (long long)y1);
    return GOL_OK;
}

extern "C" int gol_engine_load_words(gol_engine *e, int64_t y0, int64_t y1, const uint64_t *words, int64_t stride)
{
    RCCHK(rows_check(e, y0, y1, words, stride));
    if (e->mode == GOL_MODE_EXACT) {  // the loaded bytes' turn 1 is void now: bits[0] holds their 255-cells
        for (auto &s : e->sh) free_exact_bytes(s);
        e->mode = GOL_MODE_BITS;
    }
    RCCHK(ensure_standard(e));
    RCCHK(invalidate_halo(e));
    e->turn = 0;
    for (auto &s : e->sh) {
        const int64_t a = std::max(y0, s.y0), b = std::min(y1, s.y1);
        if (a >= b) continue;
        RCCHK(set_dev(s.device));
        HIPCHK(hipMemcpy2DAsync(s.bits[e->cur] + (a - s.y0) * e->pitch, e->pitch * sizeof(uint32_t), words + (a - y0) * stride,
                                stride * sizeof(uint64_t), e->W / 8, b - a, hipMemcpyHostToDevice, s.stream));
        HIPCHK(hipStreamSynchronize(s.stream));  // the caller's buffer is only borrowed
    }
    return GOL_OK;
}

extern "C" int gol_engine_store_words(gol_engine *e, int64_t y0, int64_t y1, uint64_t *words, int64_t stride)
{
    RCCHK(rows_check(e, y0, y1, words, stride));
    if (e->mode == GOL_MODE_EXACT)
        return gol_set_error(GOL_ESTATE, "the board holds bytes other than 0/255 until turn 1: use store_bytes");
    RCCHK(ensure_standard(e));
    for (auto &s : e->sh) {
        const int64_t a = std::max(y0, s.y0), b = std::min(y1, s.y1);
        if (a >= b) continue;
        RCCHK(set_dev(s.device));
        HIPCHK(hipMemcpy2DAsync(words + (a - y0) * stride, stride * sizeof(uint64_t), s.bits[e->cur] + (a - s.y0) * e->pitch,
                                e->pitch * sizeof(uint32_t), e->W / 8, b - a, hipMemcpyDeviceToHost, s.stream));
        HIPCHK(hipStreamSynchronize(s.stream));
    }
    return GOL_OK;
}
