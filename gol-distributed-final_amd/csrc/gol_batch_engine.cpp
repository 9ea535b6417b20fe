// gol_batch_engine.cpp -- batches of small boards (include/golhip.h): the handle, the argument
// checks, the rules per board and the MAP rules (gol_map.h), the split of a stepping call into launches (one gol_batch_launch per call,
// gol_batch.h), the retiring call's lists and readbacks, the soup search's driver (with the census launch that
// gol_batch_census adds to its harvest) and the strided copies.  The handle itself is gol_batch_int.h's; the island
// census, the tally's kind table and their entries are gol_batch_census.cpp.
// The kernels are gol_batch.hip (the step kernel), gol_batch_pass.hip (the rest) and gol_island.hip (the census),
// the host twins gol_batch_host.cpp and gol_island_host.cpp.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <new>
#include <vector>

#include "gol_batch_int.h"

// A launch is bounded to about this many cell-updates (and GOL_BATCH_MAX_TURNS turns), as the
// broker's chunks are: no launch runs long, whatever the batch.
#define GOL_BATCH_LAUNCH_UPDATES ((int64_t)1 << 35)
#define GOL_BATCH_MAX_TURNS 4096
// Strided loads and stores are staged through a dense host block of at most this many bytes.
#define GOL_BATCH_STAGE_BYTES ((int64_t)64 << 20)

namespace {

int auto_turns(int64_t boards, int64_t H, int64_t W)
{
    return (int)std::min<int64_t>(GOL_BATCH_MAX_TURNS, std::max<int64_t>(1, GOL_BATCH_LAUNCH_UPDATES / (boards * H * W)));
}

int range_check(const gol_batch *b, const char *what, int64_t i0, int64_t i1, const void *words, int64_t row_stride,
                int64_t board_stride)
{
    if (!b || !words || i0 < 0 || i0 > i1 || i1 > b->n || row_stride < b->Ww || board_stride < (b->H - 1) * row_stride + b->Ww)
        return gol_set_error(GOL_EINVAL, "bad batch %s (boards [%lld, %lld) of %lld, row stride %lld, board stride %lld)", what,
                             (long long)i0, (long long)i1, b ? (long long)b->n : 0LL, (long long)row_stride,
                             (long long)board_stride);
    return GOL_OK;
}

// out[0 .. n) = the alive counts or the hashes
int reduce(gol_batch *b, bool hash, uint64_t *out, int64_t cap)
{
    if (!b || !out || cap < b->n)
        return gol_set_error(GOL_EINVAL, "bad batch %s (cap %lld for %lld boards)", hash ? "hashes" : "alive_counts",
                             (long long)cap, b ? (long long)b->n : 0LL);
    OnDevice dev(b->device);
    HIPCHK(dev.err);
    const int rc = need(b->aux, b->n);
    if (rc) return rc;
    HIPCHK(golk_batch_reduce(hash, b->boards, b->n, b->H, b->W, b->aux, b->stream));
    HIPCHK(hipMemcpyAsync(out, b->aux, (size_t)b->n * sizeof(uint64_t), hipMemcpyDeviceToHost, b->stream));
    HIPCHK(hipStreamSynchronize(b->stream));
    return GOL_OK;
}

// The device copy of a host vector of the batch (the rules per board, the maps) brought up to date: `count` words
// allocated at its first use, the vector copied while the copy is stale.
int upload(gol_batch *b, const std::vector<uint32_t> &host, uint32_t *&dev, int64_t count, bool &dirty)
{
    if (!dirty && dev) return GOL_OK;
    const int rc = need(dev, count);
    if (rc) return rc;
    HIPCHK(hipMemcpyAsync(dev, host.data(), host.size() * sizeof(uint32_t), hipMemcpyHostToDevice, b->stream));
    HIPCHK(hipStreamSynchronize(b->stream));  // (the host copy may change after the call)
    dirty = false;
    return GOL_OK;
}

// A batch under MAP rules: the descriptor's two map fields from the device copy of the maps, brought up to date, and no
// masks.  This is all a driver knows of maps.
int use_maps(gol_batch *b, gol_batch_launch *l)
{
    if (b->maps.empty()) return GOL_OK;
    const int rc = upload(b, b->maps, b->dmaps, GOL_MAP_WORDS * b->n, b->maps_dirty);
    if (rc) return rc;
    l->birth = l->survive = 0;
    l->maps = b->dmaps;
    l->map_each = b->maps.size() > GOL_MAP_WORDS;
    return GOL_OK;
}

// The start of a stepping call: the launch descriptor with what every launch of the call shares (the boards, the shape,
// the rule, or the device copy of the rules per board brought up to date), and for a scan (scan != GOL_BATCH_SCAN_NONE)
// its result per board (aux) at -1 and its second buffer.  The drivers set per launch the fields that differ.
int begin_call(gol_batch *b, int scan, int64_t turns, gol_batch_launch *l)
{
    *l = {b->boards, nullptr, nullptr, b->n, b->H, b->W, 0, 0, false, false, b->birth, b->survive, nullptr, scan};  // (the rest 0)
    if (scan != GOL_BATCH_SCAN_NONE) {  // (settle scan, turns < 2: nothing can be found, every board is -1)
        int rc = need(b->aux, b->n);
        if (!rc) rc = need(b->prev, b->n * b->H * b->Ww);
        if (rc) return rc;
        l->prev = b->prev;
        l->settled = (int64_t *)b->aux;
        HIPCHK(hipMemsetAsync(l->settled, 0xff, (size_t)b->n * sizeof(int64_t), b->stream));
    }
    if (turns == 0) return GOL_OK;
    if (!b->maps.empty()) return use_maps(b, l);
    if (b->rules.empty()) return GOL_OK;
    const int rc = upload(b, b->rules, b->drules, (int64_t)b->rules.size(), b->rules_dirty);
    if (rc) return rc;
    l->rules = b->drules;
    return GOL_OK;
}

// `turns` turns of every board in launches of at most tpl; scan != GOL_BATCH_SCAN_NONE: out[0 .. n) =
// the turn the scan found per board, else -1.  Blocks once, after the last launch.
int step(gol_batch *b, int64_t turns, int scan, int64_t *out)
{
    OnDevice dev(b->device);
    HIPCHK(dev.err);
    gol_batch_launch l;
    const int rc = begin_call(b, scan, turns, &l);
    if (rc) return rc;
    const bool scans = scan != GOL_BATCH_SCAN_NONE;
    for (int64_t done = 0; done < turns; done += l.turns) {
        l.turns = (int)std::min<int64_t>(b->tpl, turns - done);
        l.turn0 = b->turn + done, l.done = done;
        l.have_prev = scans && done > 0, l.write_prev = scans && done + l.turns < turns;
        HIPCHK(golk_batch_step(l, b->stream));
    }
    if (scans) HIPCHK(hipMemcpyAsync(out, l.settled, (size_t)b->n * sizeof(int64_t), hipMemcpyDeviceToHost, b->stream));
    const hipError_t e = hipStreamSynchronize(b->stream);
    if (e != hipSuccess) return gol_set_error(GOL_EHIP, "batch step: %s", hipGetErrorString(e));
    b->turn += turns;
    return GOL_OK;
}

// gol_batch_run_cycles: the search over the active list in launches, a retire pass and a readback of the two counts
// after each; then the finish list's remainders in launches of their own, each followed by the same pass (which
// drops the boards that are done).  ends: the call's turn count at the end of every search launch.
int run_cycles(gol_batch *b, int64_t turns, int64_t *out, std::vector<int64_t> &ends)
{
    OnDevice dev(b->device);
    HIPCHK(dev.err);
    gol_batch_launch l;
    int rc = begin_call(b, GOL_BATCH_SCAN_CYCLES, turns, &l);
    if (!rc) rc = need(b->lists, 2 * b->n + 2);
    if (!rc) rc = need(b->left, b->n);
    if (rc) return rc;
    if (!b->hcounts) HIPCHK(hipHostMalloc(&b->hcounts, 2 * sizeof(int32_t), hipHostMallocDefault));
    int64_t *found = l.settled;
    int32_t *active = b->lists, *finish = b->lists + b->n, *counts = b->lists + 2 * b->n;
    int32_t *host = b->hcounts;  // the boards in the two lists, as the device counts them
    host[0] = (int32_t)b->n;
    host[1] = 0;
    auto retire = [&](int64_t done) -> int {
        HIPCHK(golk_batch_retire(active, counts, found, b->n, b->turn, b->turn + done, b->turn + turns, active, finish, b->left,
                                 b->stream));
        HIPCHK(hipMemcpyAsync(host, counts, 2 * sizeof(int32_t), hipMemcpyDeviceToHost, b->stream));
        HIPCHK(hipStreamSynchronize(b->stream));
        if (host[0] < 0 || host[0] > b->n || host[1] < 0 || host[1] > b->n)
            return gol_set_error(GOL_EHIP, "batch run_cycles: list counts %d, %d of %lld boards", host[0], host[1], (long long)b->n);
        return GOL_OK;
    };
    if (turns > 0) HIPCHK(golk_batch_iota(active, counts, b->n, b->stream));
    int64_t done = 0;
    l.list = active, l.count = counts;
    while (done < turns && host[0] > 0) {
        l.turns = (int)std::min<int64_t>(b->auto_tpl ? auto_turns(host[0], b->H, b->W) : b->tpl, turns - done);
        l.turn0 = b->turn + done, l.done = done, l.slots = host[0];
        l.have_prev = done > 0, l.write_prev = done + l.turns < turns;
        HIPCHK(golk_batch_step(l, b->stream));
        done += l.turns;
        ends.push_back(done);
        rc = retire(done);
        if (rc) return rc;
    }
    // the finish: no scan, every listed board its own turns left
    l.prev = nullptr, l.settled = nullptr, l.scan = GOL_BATCH_SCAN_NONE, l.have_prev = l.write_prev = false, l.done = 0;
    l.list = finish, l.count = counts + 1, l.left = b->left, l.turn0 = b->turn + done;
    while (host[1] > 0) {
        l.turns = b->auto_tpl ? auto_turns(host[1], b->H, b->W) : b->tpl;
        l.slots = host[1];
        HIPCHK(golk_batch_step(l, b->stream));
        rc = retire(turns);  // (the active list: no board of it is found since the last pass, or none is left)
        if (rc) return rc;
    }
    HIPCHK(hipMemcpyAsync(out, found, (size_t)b->n * sizeof(int64_t), hipMemcpyDeviceToHost, b->stream));
    const hipError_t e = hipStreamSynchronize(b->stream);
    if (e != hipSuccess) return gol_set_error(GOL_EHIP, "batch run_cycles: %s", hipGetErrorString(e));
    b->turn += turns;
    return GOL_OK;
}

// gol_batch_search on st->slots = min(n, total) slots in launches of st->launch_turns turns: the first fill, then per
// launch the aged step over the active list, the restock pass, the harvest and the refill of the slots it names, and a
// blocking read of the counts, until no slot is active.  The tables live on the device and are copied out once.
// tally (gol_batch_census; else NULL): after the harvest, the listed TALLY census of the same harvest list, on the
// snapshots, into the tables islands and fingerprint and the kind table.
int search(gol_batch *b, uint64_t seed, int64_t first, int64_t total, int64_t horizon, const gol_batch_soup_out &out,
           gol_batch_search_stats *st, const gol_batch_tally *tally)
{
    const int64_t n = b->n, m = st->slots;
    const int L = (int)st->launch_turns;
    int rc = need(b->prev, n * b->H * b->Ww);
    if (!rc) rc = need(b->slists, 4 * n + 4);
    if (!rc) rc = need(b->sages, 2 * n);
    if (!rc) rc = grow(b->tab, b->tab_words, 6 * total);
    if (rc) return rc;
    if (!b->scounts) HIPCHK(hipHostMalloc(&b->scounts, 4 * sizeof(int32_t), hipHostMallocDefault));
    int32_t *active = b->slists, *harvest = b->slists + n, *soup = b->slists + 3 * n, *counts = b->slists + 4 * n;
    int64_t *born = b->sages, *age = b->sages + n;
    int64_t *tfound = b->tab, *tperiod = b->tab + total;
    uint64_t *talive = (uint64_t *)(b->tab + 2 * total), *thash = (uint64_t *)(b->tab + 3 * total);
    HIPCHK(hipMemsetAsync(tfound, 0xff, (size_t)(2 * total) * sizeof(int64_t), b->stream));
    int64_t *tislands = b->tab + 4 * total;
    uint64_t *tfp = (uint64_t *)(b->tab + 5 * total);
    HIPCHK(hipMemsetAsync(talive, 0, (size_t)((tally ? 4 : 2) * total) * sizeof(uint64_t), b->stream));
    HIPCHK(golk_batch_soups(b->boards, m, b->H, b->W, seed, first, b->stream));
    HIPCHK(golk_batch_search_init(active, counts, soup, born, age, m, b->stream));
    // the aged launch: the cycle scan of the listed slots in their own ages from turn 0, the snapshot always written
    gol_batch_launch l = {b->boards, b->prev, age, n, b->H, b->W, L, 0, false, true, b->birth, b->survive, nullptr,
                          GOL_BATCH_SCAN_CYCLES, 0, active, counts, 0, nullptr, born};
    rc = use_maps(b, &l);
    if (rc) return rc;
    int32_t *host = b->scounts;
    host[0] = (int32_t)m;
    for (int64_t done = 0; host[0] > 0;) {
        const int64_t in = host[0];
        l.have_prev = done > 0, l.done = done, l.slots = in;
        HIPCHK(golk_batch_step(l, b->stream));
        done += L;
        st->launches += 1;
        st->board_turns += in * L;
        HIPCHK(golk_batch_restock(active, counts, age, born, soup, n, done, horizon, total, tfound, tperiod, harvest, b->stream));
        HIPCHK(golk_batch_harvest(b->prev, harvest, counts, n, b->H, b->W, total, tfound, talive, thash, in, b->stream));
        if (tally) {
            const gol_island_launch il = {b->prev, n, b->H, b->W, tally->reach, tally->symmetry, 0, tislands, nullptr, tfp, tally->table,
                                          tally->log2, tally->dropped, first, harvest, counts + 1, in, tfound};
            HIPCHK(golk_batch_islands(il, b->stream));
        }
        HIPCHK(golk_batch_refill(b->boards, harvest, counts, soup, n, b->H, b->W, seed, first, total, in, b->stream));
        HIPCHK(hipMemcpyAsync(host, counts, 4 * sizeof(int32_t), hipMemcpyDeviceToHost, b->stream));
        HIPCHK(hipStreamSynchronize(b->stream));
        if (host[0] < 0 || host[0] > in || host[1] < 0 || host[1] > in || host[2] < 0 || host[2] > host[1] || host[3] < m ||
            host[3] > total)
            return gol_set_error(GOL_EHIP, "batch search: counts %d, %d, %d, %d of %lld slots, %lld soups", host[0], host[1],
                                 host[2], host[3], (long long)in, (long long)total);
    }
    st->full_turns = st->launches * m * L;
    const size_t bytes = (size_t)total * sizeof(int64_t);
    HIPCHK(hipMemcpyAsync(out.found, tfound, bytes, hipMemcpyDeviceToHost, b->stream));
    if (out.period) HIPCHK(hipMemcpyAsync(out.period, tperiod, bytes, hipMemcpyDeviceToHost, b->stream));
    if (out.alive) HIPCHK(hipMemcpyAsync(out.alive, talive, bytes, hipMemcpyDeviceToHost, b->stream));
    if (out.hash) HIPCHK(hipMemcpyAsync(out.hash, thash, bytes, hipMemcpyDeviceToHost, b->stream));
    if (tally && out.islands) HIPCHK(hipMemcpyAsync(out.islands, tislands, bytes, hipMemcpyDeviceToHost, b->stream));
    if (tally && out.fingerprint) HIPCHK(hipMemcpyAsync(out.fingerprint, tfp, bytes, hipMemcpyDeviceToHost, b->stream));
    HIPCHK(hipStreamSynchronize(b->stream));
    return GOL_OK;
}

// gol_batch_load_words (load) and gol_batch_store_words: boards [i0, i1) between the caller's rows, row_stride and
// board_stride words apart, and the device.  Dense rows go in one copy (a load only when no row has padding to mask);
// others through a dense host block of at most GOL_BATCH_STAGE_BYTES: a load masks every row's last word, a store writes
// the Ww words of a row and leaves what lies between rows and boards.
int copy_words(gol_batch *b, bool load, int64_t i0, int64_t i1, uint64_t *words, int64_t row_stride, int64_t board_stride)
{
    OnDevice dev(b->device);
    HIPCHK(dev.err);
    const int64_t bw = b->H * b->Ww;  // words of a board on the device
    const hipMemcpyKind kind = load ? hipMemcpyHostToDevice : hipMemcpyDeviceToHost;
    auto copy = [&](uint64_t *host, int64_t c0, int64_t c1) -> int {  // (blocks: the stage is reused)
        uint64_t *d = b->boards + c0 * bw;
        HIPCHK(hipMemcpyAsync(load ? d : host, load ? host : d, (size_t)((c1 - c0) * bw) * sizeof(uint64_t), kind, b->stream));
        HIPCHK(hipStreamSynchronize(b->stream));
        return GOL_OK;
    };
    if (row_stride == b->Ww && board_stride == bw && !(load && b->W % 64)) return copy(words, i0, i1);
    const int64_t per = std::max<int64_t>(1, GOL_BATCH_STAGE_BYTES / (bw * (int64_t)sizeof(uint64_t)));
    const uint64_t tail = gol_batch_tail64(b->W);
    std::vector<uint64_t> stage((size_t)(std::min(per, std::max<int64_t>(i1 - i0, 1)) * bw));
    for (int64_t c0 = i0; c0 < i1; c0 += per) {
        const int64_t c1 = std::min(i1, c0 + per);
        int rc = load ? GOL_OK : copy(stage.data(), c0, c1);
        if (rc) return rc;
        for (int64_t i = c0; i < c1; ++i)
            for (int64_t y = 0; y < b->H; ++y) {
                uint64_t *d = stage.data() + ((i - c0) * b->H + y) * b->Ww, *w = words + (i - i0) * board_stride + y * row_stride;
                memcpy(load ? d : w, load ? w : d, (size_t)b->Ww * sizeof(uint64_t));
                if (load) d[b->Ww - 1] &= tail;
            }
        rc = load ? copy(stage.data(), c0, c1) : GOL_OK;
        if (rc) return rc;
    }
    return GOL_OK;
}

}  // namespace

// gol_batch_search (ask NULL) and gol_batch_census_sym (gol_batch_census.cpp).
int gol_batch_search_call(gol_batch *b, uint64_t seed, int64_t first, int64_t total, int64_t horizon, const gol_batch_soup_out &out,
                          const gol_batch_census_ask *ask, gol_batch_search_stats *stats)
{
    const char *what = ask ? "census" : "search";
    if (!b || !out.found || first < 0 || total < 0 || horizon < 0 || first > ((int64_t)1 << 40) || total > ((int64_t)1 << 26) ||
        first + total > ((int64_t)1 << 40))
        return gol_set_error(GOL_EINVAL, "bad batch %s (soups [%lld, +%lld) in 0..2^40, at most 2^26, horizon %lld, or NULL)", what,
                             (long long)first, (long long)total, (long long)horizon);
    if (ask && !gol_batch_tally_args_ok(*ask))
        return gol_set_error(GOL_EINVAL, "bad batch census (reach %d in 1..2, symmetry %d in 0..1, kinds_cap %lld in 0..2^23, or NULL)",
                             ask->reach, ask->symmetry, (long long)ask->kinds_cap);
    if (!b->rules.empty()) return gol_set_error(GOL_ESTATE, "batch %s: the boards of the batch have different rules", what);
    if (b->maps.size() > GOL_MAP_WORDS) return gol_set_error(GOL_ESTATE, "batch %s: the boards of the batch have different maps", what);
    OnDevice dev(b->device);
    HIPCHK(dev.err);
    const int64_t m = std::min(b->n, total);
    // every launch makes L turns (no longer than the horizon), so ages are multiples of L
    const int64_t L = std::max<int64_t>(1, std::min<int64_t>(b->auto_tpl ? auto_turns(std::max<int64_t>(m, 1), b->H, b->W) : b->tpl,
                                                             horizon));
    gol_batch_search_stats st{};
    st.slots = m;
    st.launch_turns = L;
    gol_batch_tally tally;
    int tallied = GOL_OK;  // (a full table: the per-soup outputs stand, the call ends as after a search, and then says so)
    if (total > 0 && horizon > 0) {
        int rc = ask ? gol_batch_tally_begin(b, *ask, &tally) : GOL_OK;
        if (!rc) rc = search(b, seed, first, total, horizon, out, &st, ask ? &tally : nullptr);
        if (rc) return rc;
        if (ask) tallied = gol_batch_tally_end(b, tally, what, *ask);
    } else {  // nothing to run
        gol_batch_no_results(total, out.found, out.period, out.alive, out.hash);
        for (int64_t g = 0; ask && g < total; ++g) {
            if (out.islands) out.islands[g] = 0;
            if (out.fingerprint) out.fingerprint[g] = 0;
        }
        if (ask) *ask->n_kinds = 0;
    }
    HIPCHK(hipMemsetAsync(b->boards, 0, (size_t)(b->n * b->H * b->Ww) * sizeof(uint64_t), b->stream));
    HIPCHK(hipStreamSynchronize(b->stream));
    b->turn = 0;
    if (stats) *stats = st;
    return tallied;
}

extern "C" void gol_batch_destroy(gol_batch *b)
{
    if (!b) return;
    {
        OnDevice dev(b->device);
        if (b->stream) (void)hipStreamSynchronize(b->stream);
        void *const device[] = {b->boards, b->prev, b->aux, b->drules, b->dmaps, b->lists, b->left, b->slists, b->sages, b->tab, b->isl, b->kind};
        for (void *p : device)
            if (p) (void)hipFree(p);
        for (void *p : {(void *)b->hcounts, (void *)b->scounts})
            if (p) (void)hipHostFree(p);
        if (b->stream) (void)hipStreamDestroy(b->stream);
    }
    delete b;
}

extern "C" int gol_batch_create(int64_t n, int64_t H, int64_t W, int32_t device, int32_t turns_per_launch, gol_batch **out)
{
    if (!out || !gol_batch_shape_ok(n, H, W) || turns_per_launch < 0 || device < -1)
        return gol_set_error(GOL_EINVAL, "bad batch (n %lld in 1..2^20, H %lld and W %lld in 1..%d, turns per launch %d >= 0)",
                             (long long)n, (long long)H, (long long)W, GOL_BATCH_MAX_SIDE, turns_per_launch);
    *out = nullptr;
    int dev = device;
    if (dev < 0) HIPCHK(hipGetDevice(&dev));
    int count = 0;
    HIPCHK(hipGetDeviceCount(&count));
    if (dev >= count) return gol_set_error(GOL_EINVAL, "device %d of %d", dev, count);
    gol_batch *b = new (std::nothrow) gol_batch;
    if (!b) return gol_set_error(GOL_ENOMEM, "batch handle");
    b->n = n;
    b->H = H;
    b->W = W;
    b->Ww = (W + 63) / 64;
    b->device = dev;
    golk_batch_shape(H, W, &b->wpb, &b->bpw, &b->nw);
    b->auto_tpl = turns_per_launch == 0;
    b->tpl = turns_per_launch > 0 ? turns_per_launch : auto_turns(n, H, W);
    auto fail = [&](int rc) {
        gol_batch_destroy(b);
        return rc;
    };
    OnDevice on(dev);
    hipError_t e = on.err;
    if (e == hipSuccess) e = hipStreamCreateWithFlags(&b->stream, hipStreamNonBlocking);
    if (e == hipSuccess) e = hipMalloc(&b->boards, (size_t)(n * H * b->Ww) * sizeof(uint64_t));
    if (e == hipSuccess) e = hipMemsetAsync(b->boards, 0, (size_t)(n * H * b->Ww) * sizeof(uint64_t), b->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(b->stream);
    if (e != hipSuccess)
        return fail(gol_set_error(e == hipErrorOutOfMemory ? GOL_ENOMEM : GOL_EHIP, "batch of %lld boards: %s", (long long)n,
                                  hipGetErrorString(e)));
    *out = b;
    return GOL_OK;
}

extern "C" int gol_batch_info(gol_batch *b, int64_t *n, int64_t *H, int64_t *W, int32_t *waves_per_board,
                              int32_t *boards_per_workgroup, int32_t *words_per_lane, int32_t *turns_per_launch)
{
    if (!b) return gol_set_error(GOL_EINVAL, "batch is NULL");
    if (n) *n = b->n;
    if (H) *H = b->H;
    if (W) *W = b->W;
    if (waves_per_board) *waves_per_board = b->wpb;
    if (boards_per_workgroup) *boards_per_workgroup = b->bpw;
    if (words_per_lane) *words_per_lane = b->nw;
    if (turns_per_launch) *turns_per_launch = b->tpl;
    return GOL_OK;
}

extern "C" int gol_batch_set_rule(gol_batch *b, uint32_t birth, uint32_t survive)
{
    if (!b || birth >= 512 || survive >= 512)
        return gol_set_error(GOL_EINVAL, "bad batch rule (B 0x%x, S 0x%x: masks are 9 bits)", birth, survive);
    b->birth = birth;
    b->survive = survive;
    b->rules.clear();
    b->maps.clear();
    return GOL_OK;
}

extern "C" int gol_batch_rule(gol_batch *b, uint32_t *birth, uint32_t *survive)
{
    if (!b) return gol_set_error(GOL_EINVAL, "batch is NULL");
    if (!b->maps.empty()) return gol_set_error(GOL_ESTATE, "the batch runs under MAP rules (gol_batch_maps)");
    if (!b->rules.empty()) return gol_set_error(GOL_ESTATE, "the boards of the batch have different rules (gol_batch_rules)");
    if (birth) *birth = b->birth;
    if (survive) *survive = b->survive;
    return GOL_OK;
}

extern "C" int gol_batch_set_rules(gol_batch *b, int64_t i0, int64_t i1, const uint32_t *birth, const uint32_t *survive)
{
    if (!b || !birth || !survive || i0 < 0 || i0 > i1 || i1 > b->n)
        return gol_set_error(GOL_EINVAL, "bad batch set_rules (boards [%lld, %lld) of %lld, or NULL)", (long long)i0, (long long)i1,
                             b ? (long long)b->n : 0LL);
    for (int64_t i = i0; i < i1; ++i)
        if (birth[i - i0] >= 512 || survive[i - i0] >= 512)
            return gol_set_error(GOL_EINVAL, "bad batch rule of board %lld (B 0x%x, S 0x%x: masks are 9 bits)", (long long)i,
                                 birth[i - i0], survive[i - i0]);
    if (i0 == i1) return GOL_OK;
    b->maps.clear();  // (the boards outside [i0, i1) are under birth / survive again)
    if (b->rules.empty()) {  // one rule so far
        bool same = true;
        for (int64_t i = i0; i < i1 && same; ++i) same = birth[i - i0] == b->birth && survive[i - i0] == b->survive;
        if (same) return GOL_OK;
        try {
            b->rules.resize((size_t)(2 * b->n));
        } catch (const std::bad_alloc &) {
            return gol_set_error(GOL_ENOMEM, "rules of %lld boards", (long long)b->n);
        }
        for (int64_t i = 0; i < b->n; ++i) b->rules[2 * i] = b->birth, b->rules[2 * i + 1] = b->survive;
    }
    for (int64_t i = i0; i < i1; ++i) b->rules[2 * i] = birth[i - i0], b->rules[2 * i + 1] = survive[i - i0];
    bool same = true;
    for (int64_t i = 1; i < b->n && same; ++i) same = b->rules[2 * i] == b->rules[0] && b->rules[2 * i + 1] == b->rules[1];
    if (same) {  // one rule again: the launches of gol_batch_set_rule
        b->birth = b->rules[0];
        b->survive = b->rules[1];
        b->rules.clear();
    }
    b->rules_dirty = true;
    return GOL_OK;
}

extern "C" int gol_batch_rules(gol_batch *b, int64_t i0, int64_t i1, uint32_t *birth, uint32_t *survive)
{
    if (!b || !birth || !survive || i0 < 0 || i0 > i1 || i1 > b->n)
        return gol_set_error(GOL_EINVAL, "bad batch rules (boards [%lld, %lld) of %lld, or NULL)", (long long)i0, (long long)i1,
                             b ? (long long)b->n : 0LL);
    if (!b->maps.empty()) return gol_set_error(GOL_ESTATE, "the batch runs under MAP rules (gol_batch_maps)");
    for (int64_t i = i0; i < i1; ++i) {
        birth[i - i0] = b->rules.empty() ? b->birth : b->rules[2 * i];
        survive[i - i0] = b->rules.empty() ? b->survive : b->rules[2 * i + 1];
    }
    return GOL_OK;
}

// MAP rules (gol_map.h).  One map for the batch: the rules per board go, the masks stay unused until a rule is set again.
extern "C" int gol_batch_set_map(gol_batch *b, const uint32_t *map)
{
    if (!b || !map) return gol_set_error(GOL_EINVAL, "bad batch set_map arguments (NULL)");
    try {
        b->maps.assign(map, map + GOL_MAP_WORDS);
    } catch (const std::bad_alloc &) {
        return gol_set_error(GOL_ENOMEM, "the map of the batch");
    }
    b->rules.clear();
    b->maps_dirty = true;
    return GOL_OK;
}

// The board's map as the batch stands: its own, the batch's one map, or its life-like rule as a map.
static void map_of(const gol_batch *b, int64_t i, uint32_t *out)
{
    if (b->maps.size() > GOL_MAP_WORDS) memcpy(out, b->maps.data() + GOL_MAP_WORDS * i, GOL_MAP_WORDS * sizeof(uint32_t));
    else if (!b->maps.empty()) memcpy(out, b->maps.data(), GOL_MAP_WORDS * sizeof(uint32_t));
    else if (b->rules.empty()) gol_map_from_rule(b->birth, b->survive, out);
    else gol_map_from_rule(b->rules[2 * i], b->rules[2 * i + 1], out);
}

extern "C" int gol_batch_set_maps(gol_batch *b, int64_t i0, int64_t i1, const uint32_t *maps)
{
    if (!b || !maps || i0 < 0 || i0 > i1 || i1 > b->n)
        return gol_set_error(GOL_EINVAL, "bad batch set_maps (boards [%lld, %lld) of %lld, or NULL)", (long long)i0, (long long)i1,
                             b ? (long long)b->n : 0LL);
    if (i0 == i1) return GOL_OK;
    std::vector<uint32_t> all;  // every board's map: the other boards keep theirs, a life-like rule as its map
    try {
        all.resize((size_t)(GOL_MAP_WORDS * b->n));
    } catch (const std::bad_alloc &) {
        return gol_set_error(GOL_ENOMEM, "maps of %lld boards", (long long)b->n);
    }
    for (int64_t i = 0; i < b->n; ++i) map_of(b, i, all.data() + GOL_MAP_WORDS * i);
    memcpy(all.data() + GOL_MAP_WORDS * i0, maps, (size_t)(GOL_MAP_WORDS * (i1 - i0)) * sizeof(uint32_t));
    bool same = true;
    for (int64_t i = 1; i < b->n && same; ++i) same = !memcmp(all.data(), all.data() + GOL_MAP_WORDS * i, GOL_MAP_WORDS * sizeof(uint32_t));
    if (same) all.resize(GOL_MAP_WORDS);  // one map: the launches of gol_batch_set_map
    b->maps.swap(all);
    b->rules.clear();
    b->maps_dirty = true;
    return GOL_OK;
}

extern "C" int gol_batch_maps(gol_batch *b, int64_t i0, int64_t i1, uint32_t *maps)
{
    if (!b || !maps || i0 < 0 || i0 > i1 || i1 > b->n)
        return gol_set_error(GOL_EINVAL, "bad batch maps (boards [%lld, %lld) of %lld, or NULL)", (long long)i0, (long long)i1,
                             b ? (long long)b->n : 0LL);
    for (int64_t i = i0; i < i1; ++i) map_of(b, i, maps + GOL_MAP_WORDS * (i - i0));
    return GOL_OK;
}

extern "C" int gol_batch_turn(gol_batch *b, int64_t *turn)
{
    if (!b || !turn) return gol_set_error(GOL_EINVAL, "bad batch turn arguments (NULL)");
    *turn = b->turn;
    return GOL_OK;
}

extern "C" int gol_batch_load_words(gol_batch *b, int64_t i0, int64_t i1, const uint64_t *words, int64_t row_stride,
                                    int64_t board_stride)
{
    int rc = range_check(b, "load_words", i0, i1, words, row_stride, board_stride);
    if (!rc) rc = copy_words(b, true, i0, i1, const_cast<uint64_t *>(words), row_stride, board_stride);  // (only read)
    if (!rc) b->turn = 0;
    return rc;
}

extern "C" int gol_batch_store_words(gol_batch *b, int64_t i0, int64_t i1, uint64_t *words, int64_t row_stride,
                                     int64_t board_stride)
{
    const int rc = range_check(b, "store_words", i0, i1, words, row_stride, board_stride);
    return rc ? rc : copy_words(b, false, i0, i1, words, row_stride, board_stride);
}

// (the supply from its first word)
extern "C" int gol_batch_load_random(gol_batch *b, uint64_t seed) { return gol_batch_load_soups(b, seed, 0); }

extern "C" int gol_batch_load_soups(gol_batch *b, uint64_t seed, int64_t first)
{
    if (!b || first < 0 || first + b->n > ((int64_t)1 << 40))
        return gol_set_error(GOL_EINVAL, "bad batch load_soups (first %lld: soups in 0..2^40)", (long long)first);
    OnDevice dev(b->device);
    HIPCHK(dev.err);
    HIPCHK(golk_batch_soups(b->boards, b->n, b->H, b->W, seed, first, b->stream));
    HIPCHK(hipStreamSynchronize(b->stream));
    b->turn = 0;
    return GOL_OK;
}

extern "C" int gol_batch_search(gol_batch *b, uint64_t seed, int64_t first, int64_t total, int64_t horizon, int64_t *found,
                                int64_t *period, uint64_t *alive, uint64_t *hash, gol_batch_search_stats *stats)
{
    return gol_batch_search_call(b, seed, first, total, horizon, {found, period, alive, hash, nullptr, nullptr}, nullptr, stats);
}

extern "C" int gol_batch_step(gol_batch *b, int64_t turns, int64_t *settled)
{
    if (!b || turns < 0) return gol_set_error(GOL_EINVAL, "bad batch step (turns %lld)", (long long)turns);
    return step(b, turns, settled ? GOL_BATCH_SCAN_SETTLE : GOL_BATCH_SCAN_NONE, settled);
}

extern "C" int gol_batch_step_cycles(gol_batch *b, int64_t turns, int64_t *found, int64_t *period)
{
    if (!b || turns < 0 || !found)
        return gol_set_error(GOL_EINVAL, "bad batch step_cycles (turns %lld, or NULL)", (long long)turns);
    const int64_t t0 = b->turn;
    const int rc = step(b, turns, GOL_BATCH_SCAN_CYCLES, found);
    if (rc) return rc;
    if (period)  // found - the last mark before it, with the kernel's own mark function
        for (int64_t i = 0; i < b->n; ++i)
            period[i] = found[i] < 0 ? -1 : gol_batch_period(found[i] - t0);
    return GOL_OK;
}

extern "C" int gol_batch_run_cycles(gol_batch *b, int64_t turns, int64_t *found, int64_t *period, int64_t *made)
{
    if (!b || turns < 0 || !found)
        return gol_set_error(GOL_EINVAL, "bad batch run_cycles (turns %lld, or NULL)", (long long)turns);
    const int64_t t0 = b->turn;
    std::vector<int64_t> ends;
    try {  // before any GPU work (no search launch is shorter than tpl, but for the last one)
        ends.reserve((size_t)((turns + b->tpl - 1) / b->tpl));
    } catch (const std::exception &) {
        return gol_set_error(GOL_ENOMEM, "batch run_cycles: the launch ends of %lld turns", (long long)turns);
    }
    const int rc = run_cycles(b, turns, found, ends);
    if (rc) return rc;
    for (int64_t i = 0; i < b->n; ++i) {
        const int64_t d = found[i] < 0 ? 0 : found[i] - t0;
        if (period) period[i] = d ? gol_batch_period(d) : -1;
        if (made && !d) made[i] = turns;
        if (made && d) {  // the board left after the first launch that ended at or after d, and made its remainder
            const int64_t at = *std::lower_bound(ends.begin(), ends.end(), d);
            made[i] = at + gol_batch_turns_left(d, turns - at);
        }
    }
    return GOL_OK;
}

extern "C" int gol_batch_alive_counts(gol_batch *b, uint64_t *counts, int64_t cap) { return reduce(b, false, counts, cap); }

extern "C" int gol_batch_hashes(gol_batch *b, uint64_t *hashes, int64_t cap) { return reduce(b, true, hashes, cap); }
