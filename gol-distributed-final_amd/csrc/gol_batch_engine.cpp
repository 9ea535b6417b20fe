// gol_batch_engine.cpp -- batches of small boards (include/golhip.h): the handle, the argument
// checks, the rules per board, the split of a stepping call into launches, the retiring call's lists and
// readbacks, the soup search's driver, and the strided copies.  The kernels are
// gol_batch.hip (whose object takes the name gol_batch.o), the host twin gol_batch_host.cpp.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <new>
#include <vector>

#include "gol_batch.h"
#include "gol_engine_int.h"

// A launch is bounded to about this many cell-updates (and GOL_BATCH_MAX_TURNS turns), as the
// broker's chunks are: no launch runs long, whatever the batch.
#define GOL_BATCH_LAUNCH_UPDATES ((int64_t)1 << 35)
#define GOL_BATCH_MAX_TURNS 4096
#define GOL_BATCH_MAX_BOARDS ((int64_t)1 << 20)
// Strided loads and stores are staged through a dense host block of at most this many bytes.
#define GOL_BATCH_STAGE_BYTES ((int64_t)64 << 20)

struct gol_batch {
    int64_t n = 0, H = 0, W = 0, Ww = 0;
    int device = 0;
    int tpl = 1;  // turns per launch at most
    bool auto_tpl = false;  // the automatic length: run_cycles sizes each launch by the boards still in it
    int wpb = 1, bpw = 1, nw = 1;
    uint32_t birth = GOL_RULE_BIRTH_CONWAY, survive = GOL_RULE_SURVIVE_CONWAY;
    // empty: every board under birth / survive; else n pairs (birth, survive), not all equal
    std::vector<uint32_t> rules;
    uint32_t *drules = nullptr;  // the device copy of `rules` (on demand), stale while rules_dirty
    bool rules_dirty = false;
    int64_t turn = 0;
    hipStream_t stream = nullptr;
    uint64_t *boards = nullptr;
    uint64_t *prev = nullptr;  // state(start - 1) between the launches of a scanning call (on demand)
    uint64_t *aux = nullptr;   // n words: the settle turns, the counts, the hashes (on demand)
    // run_cycles (on demand): the active list, the finish list (n entries each) and the two counts; the turns left per board
    int32_t *lists = nullptr;
    int64_t *left = nullptr;
    int32_t *hcounts = nullptr;  // pinned host memory: the two counts read back after every launch
    // search (on demand): the active list (n), the harvest list (2 n), the soup per slot (n) and the four counts; born and
    // the found age per slot (2 n); the result tables found, period, alive, hash (4 tab_cap words); four pinned counts
    int32_t *slists = nullptr;
    int64_t *sages = nullptr;
    int64_t *tab = nullptr;
    int64_t tab_cap = 0;
    int32_t *scounts = nullptr;
};

namespace {

// The batch's device for the length of a call.
struct OnDevice {
    int before = -1;
    hipError_t err;
    explicit OnDevice(int device)
    {
        err = hipGetDevice(&before);
        if (err == hipSuccess && before != device) err = hipSetDevice(device);
    }
    ~OnDevice()
    {
        if (before >= 0) (void)hipSetDevice(before);
    }
};

int need_aux(gol_batch *b)
{
    if (!b->aux) HIPCHK(hipMalloc(&b->aux, (size_t)b->n * sizeof(uint64_t)));
    return GOL_OK;
}

int auto_turns(int64_t boards, int64_t H, int64_t W)
{
    return (int)std::min<int64_t>(GOL_BATCH_MAX_TURNS, std::max<int64_t>(1, GOL_BATCH_LAUNCH_UPDATES / (boards * H * W)));
}

uint64_t tail_mask(int64_t W) { return W % 64 ? ((uint64_t)1 << (W % 64)) - 1 : ~(uint64_t)0; }

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
    const int rc = need_aux(b);
    if (rc) return rc;
    HIPCHK(golk_batch_reduce(hash, b->boards, b->n, b->H, b->W, b->aux, b->stream));
    HIPCHK(hipMemcpyAsync(out, b->aux, (size_t)b->n * sizeof(uint64_t), hipMemcpyDeviceToHost, b->stream));
    HIPCHK(hipStreamSynchronize(b->stream));
    return GOL_OK;
}

// The device copy of the rules per board, brought up to date.
int upload_rules(gol_batch *b)
{
    if (!b->rules_dirty && b->drules) return GOL_OK;
    if (!b->drules) HIPCHK(hipMalloc(&b->drules, b->rules.size() * sizeof(uint32_t)));
    HIPCHK(hipMemcpyAsync(b->drules, b->rules.data(), b->rules.size() * sizeof(uint32_t), hipMemcpyHostToDevice, b->stream));
    HIPCHK(hipStreamSynchronize(b->stream));  // (the host copy may change after the call)
    b->rules_dirty = false;
    return GOL_OK;
}

// `turns` turns of every board in launches of at most tpl; scan != GOL_BATCH_SCAN_NONE: out[0 .. n) =
// the turn the scan found per board, else -1.  Blocks once, after the last launch.
int step(gol_batch *b, int64_t turns, int scan, int64_t *out)
{
    OnDevice dev(b->device);
    HIPCHK(dev.err);
    int64_t *found = nullptr;
    if (scan != GOL_BATCH_SCAN_NONE) {  // (settle scan, turns < 2: nothing can be found, every board is -1)
        const int rc = need_aux(b);
        if (rc) return rc;
        if (!b->prev) HIPCHK(hipMalloc(&b->prev, (size_t)(b->n * b->H * b->Ww) * sizeof(uint64_t)));
        found = (int64_t *)b->aux;
        HIPCHK(hipMemsetAsync(found, 0xff, (size_t)b->n * sizeof(int64_t), b->stream));
    }
    const bool each = !b->rules.empty();
    if (each && turns > 0) {
        const int rc = upload_rules(b);
        if (rc) return rc;
    }
    for (int64_t done = 0; done < turns;) {
        const int k = (int)std::min<int64_t>(b->tpl, turns - done);
        HIPCHK(golk_batch_step(b->boards, found ? b->prev : nullptr, found, b->n, b->H, b->W, k, b->turn + done, found && done > 0,
                               found && done + k < turns, b->birth, b->survive, each ? b->drules : nullptr, scan, done,
                               b->stream));
        done += k;
    }
    if (found) HIPCHK(hipMemcpyAsync(out, found, (size_t)b->n * sizeof(int64_t), hipMemcpyDeviceToHost, b->stream));
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
    const int rc = need_aux(b);
    if (rc) return rc;
    if (!b->prev) HIPCHK(hipMalloc(&b->prev, (size_t)(b->n * b->H * b->Ww) * sizeof(uint64_t)));
    if (!b->lists) HIPCHK(hipMalloc(&b->lists, (size_t)(2 * b->n + 2) * sizeof(int32_t)));
    if (!b->left) HIPCHK(hipMalloc(&b->left, (size_t)b->n * sizeof(int64_t)));
    if (!b->hcounts) HIPCHK(hipHostMalloc(&b->hcounts, 2 * sizeof(int32_t), hipHostMallocDefault));
    int64_t *found = (int64_t *)b->aux;
    int32_t *active = b->lists, *finish = b->lists + b->n, *counts = b->lists + 2 * b->n;
    HIPCHK(hipMemsetAsync(found, 0xff, (size_t)b->n * sizeof(int64_t), b->stream));
    const bool each = !b->rules.empty();
    if (each && turns > 0) {
        const int rc2 = upload_rules(b);
        if (rc2) return rc2;
    }
    const uint32_t *rules = each ? b->drules : nullptr;
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
    while (done < turns && host[0] > 0) {
        const int k = (int)std::min<int64_t>(b->auto_tpl ? auto_turns(host[0], b->H, b->W) : b->tpl, turns - done);
        HIPCHK(golk_batch_step_list(b->boards, b->prev, found, b->n, b->H, b->W, k, b->turn + done, done > 0, done + k < turns,
                                    b->birth, b->survive, rules, done, active, counts, host[0], nullptr, b->stream));
        done += k;
        ends.push_back(done);
        const int rc2 = retire(done);
        if (rc2) return rc2;
    }
    while (host[1] > 0) {
        const int k = b->auto_tpl ? auto_turns(host[1], b->H, b->W) : b->tpl;
        HIPCHK(golk_batch_step_list(b->boards, nullptr, nullptr, b->n, b->H, b->W, k, b->turn + done, false, false, b->birth,
                                    b->survive, rules, 0, finish, counts + 1, host[1], b->left, b->stream));
        const int rc2 = retire(turns);  // (the active list: no board of it is found since the last pass, or none is left)
        if (rc2) return rc2;
    }
    HIPCHK(hipMemcpyAsync(out, found, (size_t)b->n * sizeof(int64_t), hipMemcpyDeviceToHost, b->stream));
    const hipError_t e = hipStreamSynchronize(b->stream);
    if (e != hipSuccess) return gol_set_error(GOL_EHIP, "batch run_cycles: %s", hipGetErrorString(e));
    b->turn += turns;
    return GOL_OK;
}

// gol_batch_search on m = min(n, total) slots in launches of L turns: the first fill, then per launch the aged step over the
// active list, the restock pass, the harvest and the refill of the slots it names, and a blocking read of the counts, until
// no slot is active.  The tables live on the device and are copied out once.
int search(gol_batch *b, uint64_t seed, int64_t first, int64_t total, int64_t horizon, int64_t m, int L, int64_t *found,
           int64_t *period, uint64_t *alive, uint64_t *hash, gol_batch_search_stats *st)
{
    const int64_t n = b->n;
    if (!b->prev) HIPCHK(hipMalloc(&b->prev, (size_t)(n * b->H * b->Ww) * sizeof(uint64_t)));
    if (!b->slists) HIPCHK(hipMalloc(&b->slists, (size_t)(4 * n + 4) * sizeof(int32_t)));
    if (!b->sages) HIPCHK(hipMalloc(&b->sages, (size_t)(2 * n) * sizeof(int64_t)));
    if (!b->scounts) HIPCHK(hipHostMalloc(&b->scounts, 4 * sizeof(int32_t), hipHostMallocDefault));
    if (b->tab_cap < total) {
        if (b->tab) HIPCHK(hipFree(b->tab));
        b->tab = nullptr;
        b->tab_cap = 0;
        HIPCHK(hipMalloc(&b->tab, (size_t)(4 * total) * sizeof(int64_t)));
        b->tab_cap = total;
    }
    int32_t *active = b->slists, *harvest = b->slists + n, *soup = b->slists + 3 * n, *counts = b->slists + 4 * n;
    int64_t *born = b->sages, *age = b->sages + n;
    int64_t *tfound = b->tab, *tperiod = b->tab + total;
    uint64_t *talive = (uint64_t *)(b->tab + 2 * total), *thash = (uint64_t *)(b->tab + 3 * total);
    HIPCHK(hipMemsetAsync(tfound, 0xff, (size_t)(2 * total) * sizeof(int64_t), b->stream));
    HIPCHK(hipMemsetAsync(talive, 0, (size_t)(2 * total) * sizeof(uint64_t), b->stream));
    HIPCHK(golk_batch_soups(b->boards, m, b->H, b->W, seed, first, b->stream));
    HIPCHK(golk_batch_search_init(active, counts, soup, born, age, m, b->stream));
    int32_t *host = b->scounts;
    host[0] = (int32_t)m;
    for (int64_t done = 0; host[0] > 0;) {
        const int64_t in = host[0];
        HIPCHK(golk_batch_step_aged(b->boards, b->prev, age, born, n, b->H, b->W, L, b->birth, b->survive, done, active, counts,
                                    in, b->stream));
        done += L;
        st->launches += 1;
        st->board_turns += in * L;
        HIPCHK(golk_batch_restock(active, counts, age, born, soup, n, done, horizon, total, tfound, tperiod, harvest, b->stream));
        HIPCHK(golk_batch_harvest(b->prev, harvest, counts, n, b->H, b->W, total, tfound, talive, thash, in, b->stream));
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
    HIPCHK(hipMemcpyAsync(found, tfound, bytes, hipMemcpyDeviceToHost, b->stream));
    if (period) HIPCHK(hipMemcpyAsync(period, tperiod, bytes, hipMemcpyDeviceToHost, b->stream));
    if (alive) HIPCHK(hipMemcpyAsync(alive, talive, bytes, hipMemcpyDeviceToHost, b->stream));
    if (hash) HIPCHK(hipMemcpyAsync(hash, thash, bytes, hipMemcpyDeviceToHost, b->stream));
    HIPCHK(hipStreamSynchronize(b->stream));
    return GOL_OK;
}

}  // namespace

extern "C" void gol_batch_destroy(gol_batch *b)
{
    if (!b) return;
    {
        OnDevice dev(b->device);
        if (b->stream) (void)hipStreamSynchronize(b->stream);
        if (b->boards) (void)hipFree(b->boards);
        if (b->prev) (void)hipFree(b->prev);
        if (b->aux) (void)hipFree(b->aux);
        if (b->drules) (void)hipFree(b->drules);
        if (b->lists) (void)hipFree(b->lists);
        if (b->left) (void)hipFree(b->left);
        if (b->hcounts) (void)hipHostFree(b->hcounts);
        if (b->slists) (void)hipFree(b->slists);
        if (b->sages) (void)hipFree(b->sages);
        if (b->tab) (void)hipFree(b->tab);
        if (b->scounts) (void)hipHostFree(b->scounts);
        if (b->stream) (void)hipStreamDestroy(b->stream);
    }
    delete b;
}

extern "C" int gol_batch_create(int64_t n, int64_t H, int64_t W, int32_t device, int32_t turns_per_launch, gol_batch **out)
{
    if (!out || n < 1 || n > GOL_BATCH_MAX_BOARDS || H < 1 || H > GOL_BATCH_MAX_SIDE || W < 1 || W > GOL_BATCH_MAX_SIDE ||
        turns_per_launch < 0 || device < -1)
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
    return GOL_OK;
}

extern "C" int gol_batch_rule(gol_batch *b, uint32_t *birth, uint32_t *survive)
{
    if (!b) return gol_set_error(GOL_EINVAL, "batch is NULL");
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
    for (int64_t i = i0; i < i1; ++i) {
        birth[i - i0] = b->rules.empty() ? b->birth : b->rules[2 * i];
        survive[i - i0] = b->rules.empty() ? b->survive : b->rules[2 * i + 1];
    }
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
    const int rc = range_check(b, "load_words", i0, i1, words, row_stride, board_stride);
    if (rc) return rc;
    OnDevice dev(b->device);
    HIPCHK(dev.err);
    const int64_t bw = b->H * b->Ww;  // words of a board on the device
    if (row_stride == b->Ww && board_stride == bw && b->W % 64 == 0) {
        HIPCHK(hipMemcpyAsync(b->boards + i0 * bw, words, (size_t)((i1 - i0) * bw) * sizeof(uint64_t), hipMemcpyHostToDevice,
                              b->stream));
        HIPCHK(hipStreamSynchronize(b->stream));
    } else {  // dense and masked on the host first
        const int64_t per = std::max<int64_t>(1, GOL_BATCH_STAGE_BYTES / (bw * (int64_t)sizeof(uint64_t)));
        const uint64_t tail = tail_mask(b->W);
        std::vector<uint64_t> stage((size_t)(std::min(per, std::max<int64_t>(i1 - i0, 1)) * bw));
        for (int64_t c0 = i0; c0 < i1; c0 += per) {
            const int64_t c1 = std::min(i1, c0 + per);
            for (int64_t i = c0; i < c1; ++i)
                for (int64_t y = 0; y < b->H; ++y) {
                    uint64_t *d = stage.data() + ((i - c0) * b->H + y) * b->Ww;
                    memcpy(d, words + (i - i0) * board_stride + y * row_stride, (size_t)b->Ww * sizeof(uint64_t));
                    d[b->Ww - 1] &= tail;
                }
            HIPCHK(hipMemcpyAsync(b->boards + c0 * bw, stage.data(), (size_t)((c1 - c0) * bw) * sizeof(uint64_t),
                                  hipMemcpyHostToDevice, b->stream));
            HIPCHK(hipStreamSynchronize(b->stream));  // (the stage is reused)
        }
    }
    b->turn = 0;
    return GOL_OK;
}

extern "C" int gol_batch_store_words(gol_batch *b, int64_t i0, int64_t i1, uint64_t *words, int64_t row_stride,
                                     int64_t board_stride)
{
    const int rc = range_check(b, "store_words", i0, i1, words, row_stride, board_stride);
    if (rc) return rc;
    OnDevice dev(b->device);
    HIPCHK(dev.err);
    const int64_t bw = b->H * b->Ww;
    if (row_stride == b->Ww && board_stride == bw) {
        HIPCHK(hipMemcpyAsync(words, b->boards + i0 * bw, (size_t)((i1 - i0) * bw) * sizeof(uint64_t), hipMemcpyDeviceToHost,
                              b->stream));
        HIPCHK(hipStreamSynchronize(b->stream));
        return GOL_OK;
    }
    const int64_t per = std::max<int64_t>(1, GOL_BATCH_STAGE_BYTES / (bw * (int64_t)sizeof(uint64_t)));
    std::vector<uint64_t> stage((size_t)(std::min(per, std::max<int64_t>(i1 - i0, 1)) * bw));
    for (int64_t c0 = i0; c0 < i1; c0 += per) {
        const int64_t c1 = std::min(i1, c0 + per);
        HIPCHK(hipMemcpyAsync(stage.data(), b->boards + c0 * bw, (size_t)((c1 - c0) * bw) * sizeof(uint64_t),
                              hipMemcpyDeviceToHost, b->stream));
        HIPCHK(hipStreamSynchronize(b->stream));
        for (int64_t i = c0; i < c1; ++i)
            for (int64_t y = 0; y < b->H; ++y)  // Ww words of a row: the words between rows and boards stay
                memcpy(words + (i - i0) * board_stride + y * row_stride, stage.data() + ((i - c0) * b->H + y) * b->Ww,
                       (size_t)b->Ww * sizeof(uint64_t));
    }
    return GOL_OK;
}

extern "C" int gol_batch_load_random(gol_batch *b, uint64_t seed)
{
    if (!b) return gol_set_error(GOL_EINVAL, "batch is NULL");
    OnDevice dev(b->device);
    HIPCHK(dev.err);
    HIPCHK(golk_batch_random(b->boards, b->n, b->H, b->W, seed, b->stream));
    HIPCHK(hipStreamSynchronize(b->stream));
    b->turn = 0;
    return GOL_OK;
}

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
    if (!b || !found || first < 0 || total < 0 || horizon < 0 || first > ((int64_t)1 << 40) || total > ((int64_t)1 << 26) ||
        first + total > ((int64_t)1 << 40))
        return gol_set_error(GOL_EINVAL, "bad batch search (soups [%lld, +%lld) in 0..2^40, at most 2^26, horizon %lld, or NULL)",
                             (long long)first, (long long)total, (long long)horizon);
    if (!b->rules.empty()) return gol_set_error(GOL_ESTATE, "batch search: the boards of the batch have different rules");
    OnDevice dev(b->device);
    HIPCHK(dev.err);
    const int64_t m = std::min(b->n, total);
    // every launch makes L turns (no longer than the horizon), so ages are multiples of L
    const int64_t L = std::max<int64_t>(1, std::min<int64_t>(b->auto_tpl ? auto_turns(std::max<int64_t>(m, 1), b->H, b->W) : b->tpl,
                                                             horizon));
    gol_batch_search_stats st{};
    st.slots = m;
    st.launch_turns = L;
    if (total > 0 && horizon > 0) {
        const int rc = search(b, seed, first, total, horizon, m, (int)L, found, period, alive, hash, &st);
        if (rc) return rc;
    } else {  // nothing to run: every soup is at -1
        for (int64_t g = 0; g < total; ++g) {
            found[g] = -1;
            if (period) period[g] = -1;
            if (alive) alive[g] = 0;
            if (hash) hash[g] = 0;
        }
    }
    HIPCHK(hipMemsetAsync(b->boards, 0, (size_t)(b->n * b->H * b->Ww) * sizeof(uint64_t), b->stream));
    HIPCHK(hipStreamSynchronize(b->stream));
    b->turn = 0;
    if (stats) *stats = st;
    return GOL_OK;
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
            period[i] = found[i] < 0 ? -1 : found[i] - t0 - gol_batch_last_mark(found[i] - t0);
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
        if (period) period[i] = d ? d - gol_batch_last_mark(d) : -1;
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
