// Sanitizer driver for the host twins of the tally of island kinds (gol_island_host.cpp: gol_island_tally_host,
// gol_island_tally_home_host; gol_batch_host.cpp: gol_batch_census_host).  A stand-alone program: built only by `make
// asan` from those two files with AddressSanitizer + UndefinedBehaviorSanitizer, linked without the GPU runtime, and
// run as a plain child process by tests/test_tally_ref_cpu.py.  Every input and output is a heap block of its exact
// size, so a read or write past one is a sanitizer report.
//   - gol_island_tally_host on random records of few and of many kinds against a tally by a map written here, at
//     kinds_cap 0, below and above the number of kinds, the entries past min(n_kinds, kinds_cap) untouched;
//   - gol_batch_census_host on small searches at both reaches: the first four outputs against gol_batch_search_host,
//     islands and fingerprint against gol_batch_islands_host on s(found) re-made here from the soup by `found` single
//     turns, the kinds against the map tally of those records;
//   - the home slot below 2^log2; the refusals, which write nothing.
// Exit status 0: all equal; 1: a difference (printed).
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <map>
#include <vector>

#include "golhip.h"

static char g_msg[512];
int gol_set_error(int code, const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_msg, sizeof g_msg, fmt, ap);
    va_end(ap);
    return code;
}

static uint64_t g_state = 0x9E3779B97F4A7C15ULL;
static uint64_t rnd()
{
    g_state ^= g_state << 13;
    g_state ^= g_state >> 7;
    g_state ^= g_state << 17;
    return g_state;
}

static bool same(const gol_island_kind &a, const gol_island_kind &b)
{
    return a.hash == b.hash && a.count == b.count && a.first == b.first && a.cells == b.cells && a.rows == b.rows && a.cols == b.cols;
}

// the tally of the pairs by the definition of golhip.h: a map by hash, then the order
static std::vector<gol_island_kind> naive(const gol_island *r, const int64_t *owner, int64_t n)
{
    std::map<uint64_t, gol_island_kind> m;
    for (int64_t i = 0; i < n; ++i) {
        const uint64_t h = r[i].hash ? r[i].hash : 1;
        auto it = m.find(h);
        if (it == m.end()) {
            m[h] = {h, 1, owner[i], r[i].cells, r[i].rows, r[i].cols};
            continue;
        }
        gol_island_kind &k = it->second;
        k.count += 1;
        if (owner[i] < k.first) k.first = owner[i];
        const bool less = r[i].cells != k.cells ? r[i].cells < k.cells : (r[i].rows != k.rows ? r[i].rows < k.rows : r[i].cols < k.cols);
        if (less) k.cells = r[i].cells, k.rows = r[i].rows, k.cols = r[i].cols;
    }
    std::vector<gol_island_kind> out;
    for (const auto &e : m) out.push_back(e.second);
    std::stable_sort(out.begin(), out.end(), [](const gol_island_kind &a, const gol_island_kind &b) { return a.count > b.count; });
    return out;  // (the map is in hash order, the sort stable)
}

// kinds, a heap block of exactly cap entries filled with 0xA5, against want
static int check_kinds(const gol_island *r, const int64_t *owner, int64_t n, int64_t cap, const std::vector<gol_island_kind> &want)
{
    gol_island_kind *got = new gol_island_kind[(size_t)cap];
    memset(got, 0xA5, (size_t)cap * sizeof(gol_island_kind));
    gol_island_kind untouched;
    memset(&untouched, 0xA5, sizeof untouched);
    int64_t nk = -7;
    const int rc = gol_island_tally_host(r, owner, n, cap ? got : nullptr, cap, &nk);
    int bad = rc != GOL_OK || nk != (int64_t)want.size();
    for (int64_t k = 0; k < cap && !bad; ++k) bad = !same(got[k], k < nk ? want[(size_t)k] : untouched);
    if (bad) printf("tally of %lld records, cap %lld: rc %d, %lld kinds (%lld)\n", (long long)n, (long long)cap, rc, (long long)nk, (long long)want.size());
    delete[] got;
    return bad;
}

static int check_tally(int64_t n, int distinct)
{
    gol_island *r = new gol_island[(size_t)n];
    int64_t *owner = new int64_t[(size_t)n];
    std::vector<uint64_t> hashes((size_t)distinct);
    for (auto &h : hashes) h = rnd();
    if (distinct > 2) hashes[1] = 0;  // tallied under 1
    for (int64_t i = 0; i < n; ++i) {
        // (equal hashes with different shapes and owners: the minima are taken)
        r[i] = {(int32_t)(rnd() % 64), (int32_t)(rnd() % 64), (int32_t)(1 + rnd() % 3), (uint16_t)(1 + rnd() % 3), (uint16_t)(1 + rnd() % 3),
                hashes[(size_t)(rnd() % (uint64_t)distinct)]};
        owner[i] = (int64_t)(rnd() % 1000);
    }
    const std::vector<gol_island_kind> want = naive(r, owner, n);
    int bad = 0;
    for (int64_t cap : {(int64_t)0, (int64_t)3, (int64_t)want.size(), (int64_t)want.size() + 5}) bad += check_kinds(r, owner, n, cap, want);
    delete[] r;
    delete[] owner;
    return bad;
}

static int check_census(int64_t H, int64_t W, int64_t total, int64_t first, int64_t slots, int64_t launch, int64_t horizon, int reach)
{
    const uint32_t B = 0x008, S = 0x00C;
    const uint64_t seed = 0x15A4D;
    const int64_t Ww = (W + 63) / 64;
    const size_t t = (size_t)total;
    int64_t *found = new int64_t[t], *period = new int64_t[t], *islands = new int64_t[t];
    uint64_t *alive = new uint64_t[t], *hash = new uint64_t[t], *fp = new uint64_t[t];
    int64_t *found2 = new int64_t[t], *period2 = new int64_t[t];
    uint64_t *alive2 = new uint64_t[t], *hash2 = new uint64_t[t];
    const int64_t cap = 256;
    gol_island_kind *kinds = new gol_island_kind[(size_t)cap];
    int64_t nk = -7;
    int rc = gol_batch_census_host(H, W, B, S, seed, first, total, slots, launch, horizon, reach, found, period, alive, hash, islands, fp,
                                   kinds, cap, &nk);
    int bad = rc != GOL_OK;
    rc = gol_batch_search_host(H, W, B, S, seed, first, total, slots + 2, launch + 3, horizon, found2, period2, alive2, hash2);
    bad += rc != GOL_OK;
    std::vector<gol_island> all;
    std::vector<int64_t> owners;
    int64_t n_found = 0;
    for (int64_t g = 0; g < total && !bad; ++g) {
        bad += found[g] != found2[g] || period[g] != period2[g] || alive[g] != alive2[g] || hash[g] != hash2[g];
        int64_t count = 0;
        uint64_t f = 0;
        if (found[g] >= 0) {  // s(found), one turn at a time
            uint64_t *b = new uint64_t[(size_t)(H * Ww)];
            gol_island *recs = new gol_island[(size_t)(H * W)];
            bad += gol_batch_soup_host(H, W, seed, first + g, b, Ww) != GOL_OK;
            for (int64_t i = 0; i < found[g]; ++i) bad += gol_batch_step_host(H, W, B, S, b, b, Ww) != GOL_OK;
            bad += gol_batch_islands_host(H, W, reach, b, Ww, H * W, &count, recs, &f) != GOL_OK;
            for (int64_t k = 0; k < count; ++k) all.push_back(recs[k]), owners.push_back(first + g);
            delete[] b;
            delete[] recs;
            ++n_found;
        }
        bad += islands[g] != count || fp[g] != f;
    }
    const std::vector<gol_island_kind> want = naive(all.data(), owners.data(), (int64_t)all.size());
    bad += nk != (int64_t)want.size() || nk > cap;
    for (int64_t k = 0; k < nk && !bad; ++k) bad += !same(kinds[k], want[(size_t)k]);
    bad += horizon > 0 && (n_found == 0 || all.empty());  // (a census of nothing would show nothing)
    if (bad)
        printf("census of %lld soups of %lldx%lld from %lld, %lld slots, launch %lld, horizon %lld, reach %d: %lld kinds (%lld), %lld found\n",
               (long long)total, (long long)H, (long long)W, (long long)first, (long long)slots, (long long)launch, (long long)horizon,
               reach, (long long)nk, (long long)want.size(), (long long)n_found);
    delete[] found, delete[] period, delete[] islands, delete[] alive, delete[] hash, delete[] fp;
    delete[] found2, delete[] period2, delete[] alive2, delete[] hash2, delete[] kinds;
    return bad ? 1 : 0;
}

int main()
{
    int bad = 0, n = 0;
    static const int tallies[][2] = {{0, 1}, {1, 1}, {2, 1}, {40, 3}, {500, 17}, {500, 400}, {3000, 64}};
    for (const auto &c : tallies) bad += check_tally(c[0], c[1]), ++n;
    for (int reach = 1; reach <= 2; ++reach) {
        bad += check_census(16, 16, 24, 0, 5, 7, 300, reach), ++n;
        bad += check_census(12, 70, 9, 1000, 3, 64, 200, reach), ++n;
        bad += check_census(16, 16, 6, 3, 9, 16, 0, reach), ++n;  // horizon 0: nothing found, an empty tally
    }
    for (int32_t log2 = 4; log2 <= 24; ++log2)
        for (int i = 0; i < 64; ++i) {
            const int64_t at = gol_island_tally_home_host(i ? rnd() : 0, log2);
            if (at < 0 || at >= ((int64_t)1 << log2)) printf("home slot %lld at log2 %d\n", (long long)at, log2), ++bad;
        }
    if (gol_island_tally_home_host(5, 3) != -1 || gol_island_tally_home_host(5, 25) != -1) printf("home slot of a bad log2\n"), ++bad;
    // the refusals write nothing
    gol_island r[1] = {{0, 0, 1, 1, 1, 5}};
    int64_t owner[1] = {3}, nk = 77, one[1] = {77};
    uint64_t u[1] = {77};
    gol_island_kind k[1], untouched;
    memset(k, 0xA5, sizeof k);
    memset(&untouched, 0xA5, sizeof untouched);
    const int einval[] = {gol_island_tally_host(r, owner, -1, k, 1, &nk),      gol_island_tally_host(nullptr, owner, 1, k, 1, &nk),
                          gol_island_tally_host(r, nullptr, 1, k, 1, &nk),      gol_island_tally_host(r, owner, 1, k, -1, &nk),
                          gol_island_tally_host(r, owner, 1, k, 1, nullptr),    gol_island_tally_host(r, owner, 1, nullptr, 1, &nk),
                          gol_batch_census_host(8, 8, 8, 12, 1, 0, 1, 1, 1, 10, 0, one, one, u, u, one, u, k, 1, &nk),
                          gol_batch_census_host(8, 8, 8, 12, 1, 0, 1, 1, 1, 10, 3, one, one, u, u, one, u, k, 1, &nk),
                          gol_batch_census_host(8, 8, 8, 12, 1, 0, 1, 1, 1, 10, 1, one, one, u, u, one, u, k, -1, &nk),
                          gol_batch_census_host(8, 8, 8, 12, 1, 0, 1, 1, 1, 10, 1, one, one, u, u, one, u, nullptr, 1, &nk),
                          gol_batch_census_host(8, 8, 8, 12, 1, 0, 1, 1, 1, 10, 1, one, one, u, u, one, u, k, 1, nullptr),
                          gol_batch_census_host(8, 8, 8, 12, 1, 0, 1, 0, 1, 10, 1, one, one, u, u, one, u, k, 1, &nk),
                          gol_batch_census_host(0, 8, 8, 12, 1, 0, 1, 1, 1, 10, 1, one, one, u, u, one, u, k, 1, &nk)};
    for (int rc : einval)
        if (rc != GOL_EINVAL || nk != 77 || one[0] != 77 || u[0] != 77 || !same(k[0], untouched)) {
            printf("a bad argument returned %d\n", rc);
            ++bad;
        }
    if (gol_island_tally_host(nullptr, nullptr, 0, nullptr, 0, &nk) != GOL_OK || nk != 0) printf("an empty tally: %lld kinds\n", (long long)nk), ++bad;
    printf("tally_check: %d cases, %d bad\n", n, bad);
    return bad ? 1 : 0;
}
