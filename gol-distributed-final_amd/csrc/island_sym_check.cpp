// Sanitizer driver for the FREE form of the island census's host twins (gol_island_host.cpp: gol_batch_islands_sym_host,
// gol_island_orient_host; gol_batch_host.cpp: gol_batch_census_sym_host; the row functions of gol_island.h that the
// kernel runs).  A stand-alone program: built only by `make asan` from those two files with AddressSanitizer +
// UndefinedBehaviorSanitizer, linked without the GPU runtime, and run as a plain child process by
// tests/test_island_sym_cpu.py.  The board is a heap block of its exact size -- (H - 1) * stride + ceil(W / 64) words,
// its padding bits and the words between its rows set -- and the records a heap block of exactly `cap` records, so a
// read or write past either is a sanitizer report.
//   - gol_batch_islands_sym_host with GOL_ISLAND_FREE on every shape at both reaches, three densities and three caps
//     against a flood fill written here, cell by cell, which takes an island's eight sums geometrically: the code in
//     orientation s is read off the board at the mapped offsets (no bit of a code is ever moved), with its own
//     splitmix64; the free hash is their minimum.  And with GOL_ISLAND_FIXED against gol_batch_islands_host.
//   - gol_batch_census_sym_host with GOL_ISLAND_FREE on small searches: the first four outputs against
//     gol_batch_search_host, islands and fingerprint against that flood on s(found) re-made here from the soup by
//     `found` single turns, the kinds against a tally by a map of those records.
//   - gol_island_orient_host outside its domain; the refusals, which write nothing.
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

static uint64_t mix(uint64_t x)  // splitmix64, written out here
{
    uint64_t z = x + 0x9E3779B97F4A7C15ULL;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
    return z ^ (z >> 31);
}

// the FREE census of the H x W cells of `cell`, by the definition of golhip.h
static void naive(int64_t H, int64_t W, int reach, const std::vector<uint8_t> &cell, std::vector<gol_island> &out, uint64_t *fp)
{
    std::vector<uint8_t> seen((size_t)(H * W), 0);
    std::vector<int64_t> stack;
    out.clear();
    *fp = 0;
    auto at = [&](int64_t y, int64_t x) { return (size_t)((((y % H) + H) % H) * W + (((x % W) + W) % W)); };
    for (int64_t i = 0; i < H * W; ++i) {
        if (!cell[(size_t)i] || seen[(size_t)i]) continue;
        gol_island r = {(int32_t)(i / W), (int32_t)(i % W), 0, 0, 0, 0};
        std::vector<uint8_t> rows((size_t)H, 0), cols((size_t)W, 0);
        uint64_t sums[8] = {0};
        stack.assign(1, i);
        seen[(size_t)i] = 1;
        while (!stack.empty()) {
            const int64_t c = stack.back(), y = c / W, x = c % W;
            stack.pop_back();
            for (int s = 0; s < 8; ++s) {
                const bool t = s & 1, fy = (s >> 1) & 1, fx = (s >> 2) & 1;
                uint64_t code = 0;
                for (int dy = -reach; dy <= reach; ++dy)
                    for (int dx = -reach; dx <= reach; ++dx) {
                        const int a = t ? dx : dy, b = t ? dy : dx;
                        if (cell[at(y + (fy ? -a : a), x + (fx ? -b : b))])
                            code += (uint64_t)1 << ((dy + reach) * (2 * reach + 1) + (dx + reach));
                    }
                sums[s] += mix(code ^ ((uint64_t)reach << 32));
            }
            for (int dy = -reach; dy <= reach; ++dy)
                for (int dx = -reach; dx <= reach; ++dx) {
                    const size_t o = at(y + dy, x + dx);
                    if (cell[o] && !seen[o]) seen[o] = 1, stack.push_back((int64_t)o);
                }
            r.cells += 1;
            r.rows += !rows[(size_t)y];
            r.cols += !cols[(size_t)x];
            rows[(size_t)y] = cols[(size_t)x] = 1;
        }
        r.hash = *std::min_element(sums, sums + 8);
        out.push_back(r);
        *fp += r.hash;
    }
}

static bool same(const gol_island &a, const gol_island &b)
{
    return a.y == b.y && a.x == b.x && a.cells == b.cells && a.rows == b.rows && a.cols == b.cols && a.hash == b.hash;
}

static int check(int64_t H, int64_t W, int64_t pad, int reach, int density, int64_t cap)
{
    const int64_t Ww = (W + 63) / 64, stride = Ww + pad;
    const size_t words = (size_t)((H - 1) * stride + Ww);
    const uint64_t gap = 0xA5A5A5A5A5A5A5A5ULL, tail = W % 64 ? ((uint64_t)1 << (W % 64)) - 1 : ~(uint64_t)0;
    uint64_t *b = new uint64_t[words];
    std::vector<uint8_t> cell((size_t)(H * W), 0);
    for (size_t i = 0; i < words; ++i) b[i] = gap;
    for (int64_t y = 0; y < H; ++y) {
        for (int64_t w = 0; w < Ww; ++w) {
            uint64_t v = density == 0 ? rnd() & rnd() & rnd() & rnd() & rnd() : (density == 1 ? rnd() & rnd() & rnd() : rnd());
            if (w == Ww - 1) v = (v & tail) | (gap & ~tail);  // padding bits set: never read
            b[y * stride + w] = v;
        }
        for (int64_t x = 0; x < W; ++x) cell[(size_t)(y * W + x)] = (uint8_t)(b[y * stride + x / 64] >> (x % 64) & 1);
    }
    std::vector<gol_island> want;
    uint64_t want_fp;
    naive(H, W, reach, cell, want, &want_fp);
    gol_island *got = new gol_island[(size_t)cap], *fixed = new gol_island[(size_t)cap], *plain = new gol_island[(size_t)cap];
    gol_island untouched;
    memset(&untouched, 0xA5, sizeof untouched);
    memset(got, 0xA5, (size_t)cap * sizeof(gol_island));
    memset(fixed, 0xA5, (size_t)cap * sizeof(gol_island));
    memset(plain, 0xA5, (size_t)cap * sizeof(gol_island));
    int64_t count = 77, count0 = 77, count1 = 78;
    uint64_t fp = 77, fp0 = 77, fp1 = 78;
    const int rc = gol_batch_islands_sym_host(H, W, reach, GOL_ISLAND_FREE, b, stride, cap, &count, cap ? got : nullptr, &fp);
    int bad = rc != GOL_OK || count != (int64_t)want.size() || fp != want_fp;
    for (int64_t k = 0; k < cap && !bad; ++k) bad = !same(got[k], k < count ? want[(size_t)k] : untouched);
    // symmetry 0 is the entry without _sym
    bad += gol_batch_islands_sym_host(H, W, reach, GOL_ISLAND_FIXED, b, stride, cap, &count0, cap ? fixed : nullptr, &fp0) != GOL_OK;
    bad += gol_batch_islands_host(H, W, reach, b, stride, cap, &count1, cap ? plain : nullptr, &fp1) != GOL_OK;
    bad += count0 != count1 || fp0 != fp1 || (cap && memcmp(fixed, plain, (size_t)cap * sizeof(gol_island)) != 0);
    if (bad)
        printf("%lldx%lld stride %lld reach %d density %d cap %lld: rc %d, count %lld (%lld), fingerprint %llx (%llx)\n",
               (long long)H, (long long)W, (long long)stride, reach, density, (long long)cap, rc, (long long)count,
               (long long)want.size(), (unsigned long long)fp, (unsigned long long)want_fp);
    delete[] b;
    delete[] got;
    delete[] fixed;
    delete[] plain;
    return bad ? 1 : 0;
}

static bool same_kind(const gol_island_kind &a, const gol_island_kind &b)
{
    return a.hash == b.hash && a.count == b.count && a.first == b.first && a.cells == b.cells && a.rows == b.rows && a.cols == b.cols;
}

// the tally of the pairs by the definition of golhip.h: a map by hash, then the order
static std::vector<gol_island_kind> tally(const std::vector<gol_island> &r, const std::vector<int64_t> &owner)
{
    std::map<uint64_t, gol_island_kind> m;
    for (size_t i = 0; i < r.size(); ++i) {
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
    int rc = gol_batch_census_sym_host(H, W, B, S, seed, first, total, slots, launch, horizon, reach, GOL_ISLAND_FREE, found, period,
                                       alive, hash, islands, fp, kinds, cap, &nk);
    int bad = rc != GOL_OK;
    rc = gol_batch_search_host(H, W, B, S, seed, first, total, slots + 2, launch + 3, horizon, found2, period2, alive2, hash2);
    bad += rc != GOL_OK;
    std::vector<gol_island> all, recs;
    std::vector<int64_t> owners;
    int64_t n_found = 0;
    for (int64_t g = 0; g < total && !bad; ++g) {
        bad += found[g] != found2[g] || period[g] != period2[g] || alive[g] != alive2[g] || hash[g] != hash2[g];
        int64_t count = 0;
        uint64_t f = 0;
        if (found[g] >= 0) {  // s(found), one turn at a time
            uint64_t *b = new uint64_t[(size_t)(H * Ww)];
            bad += gol_batch_soup_host(H, W, seed, first + g, b, Ww) != GOL_OK;
            for (int64_t i = 0; i < found[g]; ++i) bad += gol_batch_step_host(H, W, B, S, b, b, Ww) != GOL_OK;
            std::vector<uint8_t> cell((size_t)(H * W));
            for (int64_t y = 0; y < H; ++y)
                for (int64_t x = 0; x < W; ++x) cell[(size_t)(y * W + x)] = (uint8_t)(b[y * Ww + x / 64] >> (x % 64) & 1);
            naive(H, W, reach, cell, recs, &f);
            count = (int64_t)recs.size();
            for (const gol_island &r : recs) all.push_back(r), owners.push_back(first + g);
            delete[] b;
            ++n_found;
        }
        bad += islands[g] != count || fp[g] != f;
    }
    const std::vector<gol_island_kind> want = tally(all, owners);
    bad += nk != (int64_t)want.size() || nk > cap;
    for (int64_t k = 0; k < nk && !bad; ++k) bad += !same_kind(kinds[k], want[(size_t)k]);
    bad += horizon > 0 && (n_found == 0 || all.empty());  // (a census of nothing would show nothing)
    if (bad)
        printf("free census of %lld soups of %lldx%lld from %lld, %lld slots, launch %lld, horizon %lld, reach %d: %lld kinds (%lld), %lld found\n",
               (long long)total, (long long)H, (long long)W, (long long)first, (long long)slots, (long long)launch, (long long)horizon,
               reach, (long long)nk, (long long)want.size(), (long long)n_found);
    delete[] found, delete[] period, delete[] islands, delete[] alive, delete[] hash, delete[] fp;
    delete[] found2, delete[] period2, delete[] alive2, delete[] hash2, delete[] kinds;
    return bad ? 1 : 0;
}

int main()
{
    static const int shapes[][2] = {{1, 1},  {1, 2},  {2, 1},  {2, 2},  {3, 3},  {1, 5},  {5, 1},  {2, 5},  {5, 4},   {16, 16}, {7, 31},
                                    {7, 32}, {7, 33}, {5, 63}, {5, 64}, {5, 65}, {3, 96}, {4, 97}, {3, 481}, {4, 511}, {4, 512}, {64, 3},
                                    {65, 31}, {129, 40}};
    static const int64_t caps[] = {0, 3, 600};
    int bad = 0, n = 0;
    for (const auto &s : shapes)
        for (int reach = 1; reach <= 2; ++reach)
            for (int density = 0; density < 3; ++density)
                for (int64_t cap : caps) {
                    bad += check(s[0], s[1], n % 3 == 0 ? 2 : 0, reach, density, cap);
                    ++n;
                }
    for (int reach = 1; reach <= 2; ++reach) {
        bad += check_census(16, 16, 24, 0, 5, 7, 300, reach), ++n;
        bad += check_census(12, 70, 9, 1000, 3, 64, 200, reach), ++n;
        bad += check_census(16, 16, 6, 3, 9, 16, 0, reach), ++n;  // horizon 0: nothing found, an empty tally
    }
    // orient outside its domain is 0, and orientation 0 the identity
    for (int s : {-1, 8})
        for (int reach = 1; reach <= 2; ++reach)
            if (gol_island_orient_host(0x1ff, reach, s) != 0) printf("orient at s %d\n", s), ++bad;
    for (int reach : {0, 3})
        if (gol_island_orient_host(0x1ff, reach, 1) != 0) printf("orient at reach %d\n", reach), ++bad;
    if (gol_island_orient_host(0x0a3, 1, 0) != 0x0a3 || gol_island_orient_host(0x1234567, 2, 0) != 0x1234567) printf("orient 0\n"), ++bad;
    // the refusals write nothing
    uint64_t w[8] = {0}, fp = 77;
    int64_t c = 77, nk = 77, one[1] = {77};
    uint64_t u[1] = {77};
    gol_island r[1];
    gol_island_kind k[1];
    memset(r, 0xA5, sizeof r);
    memset(k, 0xA5, sizeof k);
    const int einval[] = {gol_batch_islands_sym_host(8, 8, 1, 2, w, 1, 1, &c, r, &fp),
                          gol_batch_islands_sym_host(8, 8, 1, -1, w, 1, 1, &c, r, &fp),
                          gol_batch_islands_sym_host(8, 8, 0, 1, w, 1, 1, &c, r, &fp),
                          gol_batch_islands_sym_host(8, 8, 3, 1, w, 1, 1, &c, r, &fp),
                          gol_batch_islands_sym_host(8, 65, 1, 1, w, 1, 1, &c, r, &fp),
                          gol_batch_islands_sym_host(8, 8, 1, 1, nullptr, 1, 1, &c, r, &fp),
                          gol_batch_islands_sym_host(8, 8, 1, 1, w, 1, 1, &c, nullptr, &fp),
                          gol_batch_census_sym_host(8, 8, 8, 12, 1, 0, 1, 1, 1, 10, 1, 2, one, one, u, u, one, u, k, 1, &nk),
                          gol_batch_census_sym_host(8, 8, 8, 12, 1, 0, 1, 1, 1, 10, 1, -1, one, one, u, u, one, u, k, 1, &nk),
                          gol_batch_census_sym_host(8, 8, 8, 12, 1, 0, 1, 1, 1, 10, 0, 1, one, one, u, u, one, u, k, 1, &nk),
                          gol_batch_census_sym_host(8, 8, 8, 12, 1, 0, 1, 1, 1, 10, 1, 1, one, one, u, u, one, u, k, 1, nullptr)};
    gol_island untouched;
    gol_island_kind no_kind;
    memset(&untouched, 0xA5, sizeof untouched);
    memset(&no_kind, 0xA5, sizeof no_kind);
    for (int rc : einval)
        if (rc != GOL_EINVAL || c != 77 || fp != 77 || nk != 77 || one[0] != 77 || u[0] != 77 || !same(r[0], untouched) ||
            !same_kind(k[0], no_kind)) {
            printf("a bad argument returned %d\n", rc);
            ++bad;
        }
    printf("island_sym_check: %d cases, %d bad\n", n, bad);
    return bad ? 1 : 0;
}
