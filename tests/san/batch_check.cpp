// Sanitizer driver for the host twin of the batch kernel (gol_batch_host.cpp: gol_batch_step_host,
// the row function of gol_batch.h that the kernel runs).  A stand-alone program: built only by
// `make asan` from gol_batch_host.cpp with AddressSanitizer + UndefinedBehaviorSanitizer, linked
// without the GPU runtime, and run as a plain child process by tests/test_batch_cpu.py.  Every buffer
// is a heap block of its exact size -- (H - 1) * stride + ceil(W / 64) words -- so a read or write past
// a row is a sanitizer report.  Each shape runs four turns of each rule from a random board whose
// padding bits are set, out of place and in place, and every turn is compared with a cell-by-cell
// count of the eight neighbours.  Exit status 0: all equal; 1: a difference (printed).
// `batch_check cycles`: gol_batch_cycles_host instead, on the same kind of buffers: every call's found,
// period and final board against a scan written here (all states kept, the marks a list), and the mark
// functions of gol_batch.h against that list for every d <= 1100.
// `batch_check run`: gol_batch_run_cycles_host (the retiring scheme of gol_batch_run_cycles on one board) against
// gol_batch_cycles_host over a grid of shapes, turns and launch lengths, on the same kind of buffers: found, period and
// the final board equal, and made the formula of golhip.h written out here.
// `batch_check search`: gol_batch_soup_host and gol_batch_search_host (the scheme of gol_batch_search) on buffers of exact size
// against a scan of every soup written here, over shapes, rules, slot counts and launch lengths; its splitmix64 is its own.
// `batch_check launch FILE`: gol_batch_launch_ok (gol_batch.h) and its export gol_batch_step_check_host on the launches of
// a file that tests/test_batch_ref_cpu.py writes: the case table's launches and the refusal list, each with its answer.
#include "check_common.h"
#include "gol_batch.h"

static int cell(const uint64_t *b, int64_t stride, int64_t y, int64_t x) { return (int)(b[y * stride + x / 64] >> (x % 64) & 1); }

// the next state of the H x W cells of `in`, as a block like `in` with the padding zero
static void naive(int64_t H, int64_t W, uint32_t birth, uint32_t survive, const uint64_t *in, uint64_t *out, int64_t stride)
{
    const int64_t Ww = (W + 63) / 64;
    for (int64_t y = 0; y < H; ++y) {
        for (int64_t w = 0; w < Ww; ++w) out[y * stride + w] = 0;
        for (int64_t x = 0; x < W; ++x) {
            int n = 0;
            for (int dy = -1; dy <= 1; ++dy)
                for (int dx = -1; dx <= 1; ++dx)
                    if (dy || dx) n += cell(in, stride, (y + dy + H) % H, (x + dx + W) % W);
            const uint32_t mask = cell(in, stride, y, x) ? survive : birth;
            if (mask >> n & 1u) out[y * stride + x / 64] |= (uint64_t)1 << (x % 64);
        }
    }
}

static int check(int64_t H, int64_t W, int64_t pad, uint32_t birth, uint32_t survive)
{
    const int64_t Ww = (W + 63) / 64, stride = Ww + pad;
    const size_t words = (size_t)((H - 1) * stride + Ww);
    const uint64_t gap = GAP;
    uint64_t *a = new uint64_t[words], *b = new uint64_t[words], *want = new uint64_t[words];
    for (size_t i = 0; i < words; ++i) a[i] = rnd() & rnd();  // (the padding bits of a row set, too)
    int bad = 0;
    for (int turn = 1; turn <= 4 && !bad; ++turn) {
        for (size_t i = 0; i < words; ++i) want[i] = b[i] = gap;
        naive(H, W, birth, survive, a, want, stride);
        int rc;
        if (turn & 1) {  // out of place
            rc = gol_batch_step_host(H, W, birth, survive, a, b, stride);
        } else {  // in place: the words between the rows are the input's, not the gap pattern
            memcpy(b, a, words * sizeof(uint64_t));
            for (int64_t y = 0; y + 1 < H; ++y)
                for (int64_t w = Ww; w < stride; ++w) want[y * stride + w] = a[y * stride + w];
            rc = gol_batch_step_host(H, W, birth, survive, b, b, stride);
        }
        if (rc != GOL_OK || memcmp(b, want, words * sizeof(uint64_t))) {
            printf("%lldx%lld stride %lld B 0x%x S 0x%x turn %d: rc %d, differs\n", (long long)H, (long long)W, (long long)stride,
                   birth, survive, turn, rc);
            bad = 1;
        }
        memcpy(a, want, words * sizeof(uint64_t));
        for (int64_t y = 0; y + 1 < H; ++y)  // garbage between the rows again: it is never read
            for (int64_t w = Ww; w < stride; ++w) a[y * stride + w] = rnd();
    }
    delete[] a;
    delete[] b;
    delete[] want;
    return bad;
}

// A board of exact size for check_cycles and check_run (delete[]): row r of `rows` at (y0, x0), 'O' alive, or random
// cells when rows is NULL; the padding bits and the words between the rows GAP
static uint64_t *pattern_board(int64_t H, int64_t W, int64_t stride, const char *const *rows, int nrows, int64_t y0, int64_t x0)
{
    const int64_t Ww = (W + 63) / 64;
    const size_t words = (size_t)((H - 1) * stride + Ww);
    const uint64_t tail = tail_of(W);
    uint64_t *a = new uint64_t[words];
    for (size_t i = 0; i < words; ++i) a[i] = rows ? 0 : rnd() & rnd();
    for (int r = 0; r < nrows; ++r)
        for (int64_t c = 0; rows[r][c]; ++c)
            if (rows[r][c] == 'O') a[((y0 + r) % H) * stride + ((x0 + c) % W) / 64] |= (uint64_t)1 << (((x0 + c) % W) % 64);
    for (int64_t y = 0; y < H; ++y) {
        a[y * stride + Ww - 1] = (a[y * stride + Ww - 1] & tail) | (GAP & ~tail);  // padding bits set: never read
        for (int64_t w = Ww; w < stride && y + 1 < H; ++w) a[y * stride + w] = GAP;
    }
    return a;
}

// one call of gol_batch_cycles_host on a board of exact size (pattern_board), out of place or in place
static int check_cycles(int64_t H, int64_t W, int64_t pad, uint32_t birth, uint32_t survive, const char *const *rows, int nrows,
                        int64_t y0, int64_t x0, int64_t turns, bool in_place)
{
    const int64_t Ww = (W + 63) / 64, stride = Ww + pad;
    const size_t words = (size_t)((H - 1) * stride + Ww);
    const uint64_t gap = GAP, tail = tail_of(W);
    uint64_t *a = pattern_board(H, W, stride, rows, nrows, y0, x0), *b = new uint64_t[words];
    // the scan, naively: every state kept, the marks 0, 1, 3, 7, ... a list
    std::vector<std::vector<uint64_t>> st(1, std::vector<uint64_t>(a, a + words));
    for (int64_t y = 0; y < H; ++y) st[0][y * stride + Ww - 1] &= tail;
    std::vector<int64_t> marks;
    for (int64_t m = 0; m <= turns; m = 2 * m + 1) marks.push_back(m);
    int64_t want_found = -1, want_period = -1;
    for (int64_t d = 1; d <= turns; ++d) {
        st.push_back(st[0]);
        naive(H, W, birth, survive, st[(size_t)d - 1].data(), st[(size_t)d].data(), stride);
        int64_t m = 0;
        for (int64_t v : marks)
            if (v < d) m = v;
        if (want_found < 0 && st[(size_t)d] == st[(size_t)m]) want_found = d, want_period = d - m;
    }
    int64_t found = 77, period = 77;
    for (size_t i = 0; i < words; ++i) b[i] = gap;
    if (in_place) memcpy(b, a, words * sizeof(uint64_t));
    const int rc = gol_batch_cycles_host(H, W, birth, survive, in_place ? b : a, b, stride, turns, &found, &period);
    std::vector<uint64_t> want = st.back();
    for (int64_t y = 0; y + 1 < H; ++y)
        for (int64_t w = Ww; w < stride; ++w) want[y * stride + w] = gap;
    int bad = rc != GOL_OK || found != want_found || period != want_period || memcmp(b, want.data(), words * sizeof(uint64_t));
    if (bad)
        printf("cycles %lldx%lld stride %lld B 0x%x S 0x%x turns %lld%s: rc %d, found %lld (%lld), period %lld (%lld)\n",
               (long long)H, (long long)W, (long long)stride, birth, survive, (long long)turns, in_place ? " in place" : "", rc,
               (long long)found, (long long)want_found, (long long)period, (long long)want_period);
    delete[] a;
    delete[] b;
    return bad;
}

static int main_cycles()
{
    int bad = 0, n = 0;
    // the mark functions against the list
    std::vector<int64_t> marks;
    for (int64_t m = 0; m <= 1100; m = 2 * m + 1) marks.push_back(m);
    for (int64_t d = 0; d <= 1100; ++d) {
        bool is = false;
        int64_t last = -1;
        for (int64_t v : marks) {
            is = is || v == d;
            if (v < d) last = v;
        }
        if (gol_batch_is_mark(d) != is || (d >= 1 && gol_batch_last_mark(d) != last)) {
            printf("mark functions differ at d = %lld\n", (long long)d);
            ++bad;
        }
    }
    static const char *const glider[] = {".O.", "..O", "OOO"}, *const row10[] = {"OOOOOOOOOO"}, *const blinker[] = {"OOO"},
                             *const block[] = {"OO", "OO"};
    for (int pad = 0; pad <= 2; pad += 2)
        for (int in_place = 0; in_place <= 1; ++in_place, n += 8) {
            bad += check_cycles(5, 5, pad, 0x008, 0x00C, block, 0, 0, 0, 10, in_place);  // empty
            bad += check_cycles(5, 5, pad, 0x008, 0x00C, block, 2, 1, 1, 10, in_place);
            bad += check_cycles(5, 5, pad, 0x008, 0x00C, blinker, 1, 2, 1, 10, in_place);
            bad += check_cycles(20, 20, pad, 0x008, 0x00C, row10, 1, 10, 5, 100, in_place);
            bad += check_cycles(66, 33, pad, 0x008, 0x00C, row10, 1, 0, 28, 100, in_place);
            bad += check_cycles(8, 8, pad, 0x008, 0x00C, glider, 3, 0, 0, 200, in_place);
            bad += check_cycles(7, 9, pad, 0x008, 0x00C, glider, 3, 0, 0, 600, in_place);
            bad += check_cycles(3, 65, pad, 0x008, 0x00C, glider, 0, 0, 0, 0, in_place);  // no turn: the board, masked
        }
    static const int shapes[][2] = {{1, 1}, {2, 5}, {16, 16}, {7, 33}, {5, 65}, {65, 31}, {3, 481}};
    static const uint32_t rules[][2] = {{0x008, 0x00C}, {0x048, 0x00C}, {0x004, 0x000},
                                        {0x001, 0x100}, {0x0AA, 0x0AA}, {0x018, 0x018}};
    for (const auto &s : shapes)
        for (const auto &r : rules)
            for (int pad = 0; pad <= 2; pad += 2, ++n)
                bad += check_cycles(s[0], s[1], pad, r[0], r[1], nullptr, 0, 0, 0, 70, pad != 0);
    uint64_t w[8] = {0};
    int64_t f = 77, p = 77;
    const int einval[] = {gol_batch_cycles_host(0, 8, 8, 12, w, w, 1, 1, &f, &p),
                          gol_batch_cycles_host(8, 513, 8, 12, w, w, 9, 1, &f, &p),
                          gol_batch_cycles_host(8, 8, 512, 12, w, w, 1, 1, &f, &p),
                          gol_batch_cycles_host(8, 8, 8, 512, w, w, 1, 1, &f, &p),
                          gol_batch_cycles_host(8, 65, 8, 12, w, w, 1, 1, &f, &p),
                          gol_batch_cycles_host(8, 8, 8, 12, nullptr, w, 1, 1, &f, &p),
                          gol_batch_cycles_host(8, 8, 8, 12, w, nullptr, 1, 1, &f, &p),
                          gol_batch_cycles_host(8, 8, 8, 12, w, w, 1, -1, &f, &p),
                          gol_batch_cycles_host(8, 8, 8, 12, w, w, 1, 1, nullptr, &p)};
    for (int rc : einval)
        if (rc != GOL_EINVAL || f != 77 || p != 77) {
            printf("a bad argument returned %d\n", rc);
            ++bad;
        }
    if (gol_batch_cycles_host(8, 8, 8, 12, w, w, 1, 3, &f, nullptr) != GOL_OK || f != 1) {  // (period may be NULL)
        printf("a NULL period: found %lld\n", (long long)f);
        ++bad;
    }
    printf("batch_check cycles: %d cases, %d bad\n", n, bad);
    return bad ? 1 : 0;
}

// one call of gol_batch_run_cycles_host against gol_batch_cycles_host on boards of exact size
static int check_run(int64_t H, int64_t W, int64_t pad, uint32_t birth, uint32_t survive, const char *const *rows, int nrows,
                     int64_t turns, int64_t launch, bool in_place)
{
    const int64_t Ww = (W + 63) / 64, stride = Ww + pad;
    const size_t words = (size_t)((H - 1) * stride + Ww);
    const uint64_t gap = GAP;
    uint64_t *a = pattern_board(H, W, stride, rows, nrows, 0, 0), *b = new uint64_t[words], *want = new uint64_t[words];
    for (size_t i = 0; i < words; ++i) want[i] = b[i] = gap;
    int64_t wf = 77, wp = 77, found = 77, period = 77, made = 77;
    int rc = gol_batch_cycles_host(H, W, birth, survive, a, want, stride, turns, &wf, &wp);
    int64_t wm = turns;
    if (wf >= 0) {
        int64_t at = (wf + launch - 1) / launch * launch;
        if (at > turns) at = turns;
        wm = at + (turns - at) % wp;
    }
    if (in_place) {
        memcpy(b, a, words * sizeof(uint64_t));
        for (int64_t y = 0; y + 1 < H; ++y)
            for (int64_t w = Ww; w < stride; ++w) want[y * stride + w] = a[y * stride + w];
    }
    if (rc == GOL_OK)
        rc = gol_batch_run_cycles_host(H, W, birth, survive, in_place ? b : a, b, stride, turns, launch, &found, &period, &made);
    const int bad = rc != GOL_OK || found != wf || period != wp || made != wm || memcmp(b, want, words * sizeof(uint64_t));
    if (bad)
        printf("run %lldx%lld stride %lld B 0x%x S 0x%x turns %lld launch %lld%s: rc %d, found %lld (%lld), period %lld (%lld), "
               "made %lld (%lld)\n",
               (long long)H, (long long)W, (long long)stride, birth, survive, (long long)turns, (long long)launch,
               in_place ? " in place" : "", rc, (long long)found, (long long)wf, (long long)period, (long long)wp, (long long)made,
               (long long)wm);
    delete[] a;
    delete[] b;
    delete[] want;
    return bad;
}

static int main_run()
{
    int bad = 0, n = 0;
    static const char *const glider[] = {".O.", "..O", "OOO"}, *const row10[] = {"OOOOOOOOOO"};
    static const int shapes[][2] = {{1, 1}, {2, 5}, {16, 16}, {7, 33}, {5, 65}, {65, 31}, {3, 481}};
    static const uint32_t rules[][2] = {{0x008, 0x00C}, {0x048, 0x00C}, {0x004, 0x000}, {0x0AA, 0x0AA}};
    static const int64_t turns[] = {0, 1, 2, 70}, launches[] = {1, 5, 7, 64, 70, 1000};
    for (const auto &s : shapes)
        for (const auto &r : rules)
            for (int64_t t : turns)
                for (int64_t l : launches)
                    for (int pad = 0; pad <= 2; pad += 2, ++n) bad += check_run(s[0], s[1], pad, r[0], r[1], nullptr, 0, t, l, pad != 0);
    for (int64_t l : launches)
        for (int pad = 0; pad <= 2; pad += 2, n += 3) {
            bad += check_run(8, 8, pad, 0x008, 0x00C, glider, 3, 200, l, pad != 0);    // found 63, period 32
            bad += check_run(7, 9, pad, 0x008, 0x00C, glider, 3, 1100, l, pad == 0);   // found 507, period 252
            bad += check_run(20, 20, pad, 0x008, 0x00C, row10, 1, 100, l, pad != 0);  // found 30, period 15
        }
    uint64_t w[8] = {0};
    int64_t f = 77, p = 77, m = 77;
    const int einval[] = {gol_batch_run_cycles_host(0, 8, 8, 12, w, w, 1, 1, 1, &f, &p, &m),
                          gol_batch_run_cycles_host(8, 513, 8, 12, w, w, 9, 1, 1, &f, &p, &m),
                          gol_batch_run_cycles_host(8, 8, 512, 12, w, w, 1, 1, 1, &f, &p, &m),
                          gol_batch_run_cycles_host(8, 8, 8, 512, w, w, 1, 1, 1, &f, &p, &m),
                          gol_batch_run_cycles_host(8, 65, 8, 12, w, w, 1, 1, 1, &f, &p, &m),
                          gol_batch_run_cycles_host(8, 8, 8, 12, nullptr, w, 1, 1, 1, &f, &p, &m),
                          gol_batch_run_cycles_host(8, 8, 8, 12, w, nullptr, 1, 1, 1, &f, &p, &m),
                          gol_batch_run_cycles_host(8, 8, 8, 12, w, w, 1, -1, 1, &f, &p, &m),
                          gol_batch_run_cycles_host(8, 8, 8, 12, w, w, 1, 1, 0, &f, &p, &m),
                          gol_batch_run_cycles_host(8, 8, 8, 12, w, w, 1, 1, 1, nullptr, &p, &m)};
    for (int rc : einval)
        if (rc != GOL_EINVAL || f != 77 || p != 77 || m != 77) {
            printf("a bad argument returned %d\n", rc);
            ++bad;
        }
    if (gol_batch_run_cycles_host(8, 8, 8, 12, w, w, 1, 3, 2, &f, nullptr, nullptr) != GOL_OK || f != 1) {  // (may be NULL)
        printf("a NULL period and made: found %lld\n", (long long)f);
        ++bad;
    }
    printf("batch_check run: %d cases, %d bad\n", n, bad);
    return bad ? 1 : 0;
}

// one call of gol_batch_search_host on result arrays of exact size, against a scan of every soup written here: all states
// kept, the marks a list, the census of the state at the found turn
static int check_search(int64_t H, int64_t W, uint32_t birth, uint32_t survive, uint64_t seed, int64_t first, int64_t total,
                        int64_t slots, int64_t launch, int64_t horizon, int nulls)
{
    const int64_t Ww = (W + 63) / 64, bw = H * Ww;
    const uint64_t tail = tail_of(W);
    int64_t *found = new int64_t[(size_t)total], *period = new int64_t[(size_t)total];
    uint64_t *alive = new uint64_t[(size_t)total], *hash = new uint64_t[(size_t)total];
    for (int64_t g = 0; g < total; ++g) found[g] = period[g] = 77, alive[g] = hash[g] = 77;
    int rc = gol_batch_search_host(H, W, birth, survive, seed, first, total, slots, launch, horizon, found,
                                   nulls & 1 ? nullptr : period, nulls & 2 ? nullptr : alive, nulls & 4 ? nullptr : hash);
    int bad = rc != GOL_OK;
    std::vector<int64_t> marks;
    for (int64_t m = 0; m <= horizon; m = 2 * m + 1) marks.push_back(m);
    for (int64_t g = 0; g < total && !bad; ++g) {
        uint64_t *soup = new uint64_t[(size_t)bw];  // exact size: a write past the soup is a report
        rc = gol_batch_soup_host(H, W, seed, first + g, soup, Ww);
        for (int64_t y = 0; y < H; ++y)
            for (int64_t w = 0; w < Ww; ++w) {
                const uint64_t v = mix(seed ^ (uint64_t)(((first + g) * H + y) * Ww + w)) & (w == Ww - 1 ? tail : ~(uint64_t)0);
                if (soup[y * Ww + w] != v) bad = 1;
            }
        std::vector<std::vector<uint64_t>> st(1, std::vector<uint64_t>(soup, soup + bw));
        delete[] soup;
        int64_t wf = -1, wp = -1;
        uint64_t wa = 0, wh = 0;
        for (int64_t d = 1; d <= horizon && wf < 0; ++d) {
            st.push_back(st[0]);
            naive(H, W, birth, survive, st[(size_t)d - 1].data(), st[(size_t)d].data(), Ww);
            int64_t m = 0;
            for (int64_t v : marks)
                if (v < d) m = v;
            if (st[(size_t)d] == st[(size_t)m]) wf = d, wp = d - m;
        }
        if (wf >= 0)
            for (int64_t i = 0; i < bw; ++i) {
                wa += (uint64_t)__builtin_popcountll(st[(size_t)wf][(size_t)i]);
                wh += mix(st[(size_t)wf][(size_t)i] ^ mix((uint64_t)i));
            }
        if (rc != GOL_OK || found[g] != wf || period[g] != (nulls & 1 ? 77 : wp) || alive[g] != (nulls & 2 ? 77 : wa) ||
            hash[g] != (nulls & 4 ? 77 : wh)) {
            printf("search %lldx%lld B 0x%x S 0x%x soup %lld of [%lld, +%lld) slots %lld launch %lld horizon %lld: rc %d, found "
                   "%lld (%lld), period %lld (%lld), alive %llu (%llu)\n",
                   (long long)H, (long long)W, birth, survive, (long long)g, (long long)first, (long long)total, (long long)slots,
                   (long long)launch, (long long)horizon, rc, (long long)found[g], (long long)wf, (long long)period[g],
                   (long long)wp, (unsigned long long)alive[g], (unsigned long long)wa);
            bad = 1;
        }
    }
    delete[] found;
    delete[] period;
    delete[] alive;
    delete[] hash;
    return bad;
}

static int main_search()
{
    int bad = 0, n = 0;
    static const int shapes[][2] = {{1, 1}, {2, 5}, {16, 16}, {7, 33}, {5, 65}, {65, 31}, {3, 481}};
    static const uint32_t rules[][2] = {{0x008, 0x00C}, {0x048, 0x00C}, {0x000, 0x00C}, {0x0AA, 0x0AA}};
    static const int64_t slots[] = {1, 3}, launches[] = {1, 7, 64, 200};
    for (const auto &s : shapes)
        for (const auto &r : rules)
            for (int64_t k : slots)
                for (int64_t l : launches) {
                    bad += check_search(s[0], s[1], r[0], r[1], 1 + (uint64_t)n, n % 5 ? 0 : 1000003, 7, k, l, 70, n % 8);
                    ++n;
                }
    for (int64_t l : launches) {  // the overshoot (16 x 16, seed 1: soups found at 256 and at 257), no soup, no turn
        n += 3;
        bad += check_search(16, 16, 0x008, 0x00C, 1, 0, 12, 5, l, 256, 0);
        bad += check_search(16, 16, 0x008, 0x00C, 1, 0, 0, 5, l, 70, 0);
        bad += check_search(16, 16, 0x008, 0x00C, 1, ((int64_t)1 << 40) - 3, 3, 5, l, 0, 0);
    }
    int64_t f[2] = {77, 77};
    uint64_t w[8] = {0};
    const int einval[] = {gol_batch_search_host(0, 8, 8, 12, 1, 0, 2, 1, 1, 5, f, f, w, w),
                          gol_batch_search_host(8, 513, 8, 12, 1, 0, 2, 1, 1, 5, f, f, w, w),
                          gol_batch_search_host(8, 8, 512, 12, 1, 0, 2, 1, 1, 5, f, f, w, w),
                          gol_batch_search_host(8, 8, 8, 12, 1, -1, 2, 1, 1, 5, f, f, w, w),
                          gol_batch_search_host(8, 8, 8, 12, 1, 0, -1, 1, 1, 5, f, f, w, w),
                          gol_batch_search_host(8, 8, 8, 12, 1, 0, 2, 0, 1, 5, f, f, w, w),
                          gol_batch_search_host(8, 8, 8, 12, 1, 0, 2, 1, 0, 5, f, f, w, w),
                          gol_batch_search_host(8, 8, 8, 12, 1, 0, 2, 1, 1, -1, f, f, w, w),
                          gol_batch_search_host(8, 8, 8, 12, 1, ((int64_t)1 << 40) - 1, 2, 1, 1, 5, f, f, w, w),
                          gol_batch_search_host(8, 8, 8, 12, 1, 0, ((int64_t)1 << 26) + 1, 1, 1, 5, f, f, w, w),
                          gol_batch_search_host(8, 8, 8, 12, 1, 0, 2, 1, 1, 5, nullptr, f, w, w),
                          gol_batch_soup_host(8, 8, 1, -1, w, 1), gol_batch_soup_host(8, 65, 1, 0, w, 1),
                          gol_batch_soup_host(8, 8, 1, 0, nullptr, 1)};
    for (int rc : einval)
        if (rc != GOL_EINVAL || f[0] != 77 || f[1] != 77 || w[0]) {
            printf("a bad argument returned %d\n", rc);
            ++bad;
        }
    printf("batch_check search: %d cases, %d bad\n", n, bad);
    return bad ? 1 : 0;
}

// gol_batch_launch_ok on the launches of a file: a line per launch, the expected answer (1 accepted, 0 refused) and the
// 20 arguments of gol_dev_batch_step without the stream, a pointer as an integer (0: NULL) that is never dereferenced
static int main_launch(const char *path)
{
    FILE *f = fopen(path, "r");
    if (!f) {
        printf("batch_check launch: cannot read %s\n", path);
        return 2;
    }
    int bad = 0, n[2] = {0, 0};
    long long v[21];
    for (;;) {
        int got = 0;
        while (got < 21 && fscanf(f, "%lld", &v[got]) == 1) ++got;
        if (got == 0) break;
        if (got < 21 || (v[0] != 0 && v[0] != 1)) {
            printf("launch line %d: %d fields\n", n[0] + n[1] + 1, got);
            ++bad;
            break;
        }
        const gol_batch_launch l = {(uint64_t *)(uintptr_t)v[1], (uint64_t *)(uintptr_t)v[2], (int64_t *)(uintptr_t)v[3], v[4], v[5], v[6],
                                    (int32_t)v[7], v[8], v[9] != 0, v[10] != 0, (uint32_t)v[11], (uint32_t)v[12],
                                    (const uint32_t *)(uintptr_t)v[13], (int32_t)v[14], v[15], (const int32_t *)(uintptr_t)v[16],
                                    (const int32_t *)(uintptr_t)v[17], v[18], (int64_t *)(uintptr_t)v[19],
                                    (const int64_t *)(uintptr_t)v[20]};
        // the function, and its export: one answer
        const int rc = gol_batch_step_check_host(l.boards, l.prev, l.settled, l.n, l.H, l.W, l.turns, l.turn0, l.have_prev,
                                                 l.write_prev, l.birth, l.survive, l.rules, l.scan, l.done, l.list, l.count, l.slots,
                                                 l.left, l.born);
        if (gol_batch_launch_ok(l) != (v[0] == 1) || rc != (v[0] == 1 ? GOL_OK : GOL_EINVAL)) {
            printf("launch line %d: expected %lld, rc %d\n", n[0] + n[1] + 1, v[0], rc);
            ++bad;
        }
        ++n[v[0]];
    }
    fclose(f);
    printf("batch_check launch: %d accepted, %d refused, %d bad\n", n[1], n[0], bad);
    return bad || !n[0] || !n[1] ? 1 : 0;
}

int main(int argc, char **argv)
{
    if (argc > 2 && !strcmp(argv[1], "launch")) return main_launch(argv[2]);
    if (argc > 1) {
        if (!strcmp(argv[1], "cycles")) return main_cycles();
        if (!strcmp(argv[1], "run")) return main_run();
        if (!strcmp(argv[1], "search")) return main_search();
        printf("usage: batch_check [cycles | run | search | launch FILE]\n");
        return 2;
    }
    static const int shapes[][2] = {{1, 1}, {1, 2}, {2, 1}, {2, 2}, {3, 3}, {2, 5}, {5, 2}, {16, 16}, {7, 31}, {7, 32}, {7, 33},
                                    {5, 63}, {5, 64}, {5, 65}, {3, 96}, {4, 511}, {4, 512}, {3, 481}, {64, 1}, {65, 31}};
    static const uint32_t rules[][2] = {{0x008, 0x00C}, {0x048, 0x00C}, {0x1C8, 0x1D8}, {0x004, 0x000}, {0x001, 0x100},
                                        {0x1FF, 0x1FF}};  // B3/S23 B36/S23 B3678/S34678 B2/S B0/S8 B012345678/S012345678
    int bad = 0, n = 0;
    for (const auto &s : shapes)
        for (const auto &r : rules)
            for (int pad = 0; pad <= 2; pad += 2, ++n) bad += check(s[0], s[1], pad, r[0], r[1]);
    // the refusals write nothing
    uint64_t w[8] = {0};
    const int einval[] = {gol_batch_step_host(0, 8, 8, 12, w, w, 1),    gol_batch_step_host(8, 0, 8, 12, w, w, 1),
                          gol_batch_step_host(513, 8, 8, 12, w, w, 1),  gol_batch_step_host(8, 513, 8, 12, w, w, 9),
                          gol_batch_step_host(8, 8, 512, 12, w, w, 1),  gol_batch_step_host(8, 8, 8, 512, w, w, 1),
                          gol_batch_step_host(8, 65, 8, 12, w, w, 1),   gol_batch_step_host(8, 8, 8, 12, nullptr, w, 1),
                          gol_batch_step_host(8, 8, 8, 12, w, nullptr, 1)};
    for (int rc : einval)
        if (rc != GOL_EINVAL) {
            printf("a bad argument returned %d\n", rc);
            ++bad;
        }
    printf("batch_check: %d cases, %d bad\n", n, bad);
    return bad ? 1 : 0;
}
