// Sanitizer driver for the host twin of the island census (gol_island_host.cpp: gol_batch_islands_host, the row
// functions of gol_island.h that the kernel runs).  A stand-alone program: built only by `make asan` from
// gol_island_host.cpp with AddressSanitizer + UndefinedBehaviorSanitizer, linked without the GPU runtime, and run as a
// plain child process by tests/test_island_ref_cpu.py.  The board is a heap block of its exact size -- (H - 1) * stride
// + ceil(W / 64) words, its padding bits and the words between its rows set -- and the records a heap block of exactly
// `cap` records, so a read or write past either is a sanitizer report.  Every shape runs both reaches at three
// densities and three caps against a flood fill written here, cell by cell, with its own splitmix64: the count, the
// first min(count, cap) records, the fingerprint, and the records past them untouched.  Then the refusals, which write
// nothing.  Exit status 0: all equal; 1: a difference (printed).
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
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

// the census of the H x W cells of `cell`, by the definition of golhip.h
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
        stack.assign(1, i);
        seen[(size_t)i] = 1;
        while (!stack.empty()) {
            const int64_t c = stack.back(), y = c / W, x = c % W;
            stack.pop_back();
            uint64_t code = 0;
            for (int dy = -reach; dy <= reach; ++dy)
                for (int dx = -reach; dx <= reach; ++dx) {
                    const size_t o = at(y + dy, x + dx);
                    if (!cell[o]) continue;
                    code += (uint64_t)1 << ((dy + reach) * (2 * reach + 1) + (dx + reach));
                    if (!seen[o]) seen[o] = 1, stack.push_back((int64_t)o);
                }
            r.cells += 1;
            r.rows += !rows[(size_t)y];
            r.cols += !cols[(size_t)x];
            rows[(size_t)y] = cols[(size_t)x] = 1;
            r.hash += mix(code ^ ((uint64_t)reach << 32));
        }
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
    gol_island *got = new gol_island[(size_t)cap];
    memset(got, 0xA5, (size_t)cap * sizeof(gol_island));
    int64_t count = 77;
    uint64_t fp = 77;
    const int rc = gol_batch_islands_host(H, W, reach, b, stride, cap, &count, cap ? got : nullptr, &fp);
    int bad = rc != GOL_OK || count != (int64_t)want.size() || fp != want_fp;
    for (int64_t k = 0; k < cap && !bad; ++k) {
        gol_island untouched;
        memset(&untouched, 0xA5, sizeof untouched);
        bad = !same(got[k], k < count ? want[(size_t)k] : untouched);
    }
    if (bad)
        printf("%lldx%lld stride %lld reach %d density %d cap %lld: rc %d, count %lld (%lld), fingerprint %llx (%llx)\n",
               (long long)H, (long long)W, (long long)stride, reach, density, (long long)cap, rc, (long long)count,
               (long long)want.size(), (unsigned long long)fp, (unsigned long long)want_fp);
    delete[] b;
    delete[] got;
    return bad;
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
    // the refusals write nothing
    uint64_t w[8] = {0}, fp = 77;
    int64_t c = 77;
    gol_island r[1];
    memset(r, 0xA5, sizeof r);
    const int einval[] = {gol_batch_islands_host(0, 8, 1, w, 1, 1, &c, r, &fp),   gol_batch_islands_host(8, 0, 1, w, 1, 1, &c, r, &fp),
                          gol_batch_islands_host(513, 8, 1, w, 1, 1, &c, r, &fp), gol_batch_islands_host(8, 513, 1, w, 9, 1, &c, r, &fp),
                          gol_batch_islands_host(8, 8, 0, w, 1, 1, &c, r, &fp),   gol_batch_islands_host(8, 8, 3, w, 1, 1, &c, r, &fp),
                          gol_batch_islands_host(8, 65, 1, w, 1, 1, &c, r, &fp),  gol_batch_islands_host(8, 8, 1, nullptr, 1, 1, &c, r, &fp),
                          gol_batch_islands_host(8, 8, 1, w, 1, -1, &c, r, &fp),  gol_batch_islands_host(8, 8, 1, w, 1, 1, nullptr, r, &fp),
                          gol_batch_islands_host(8, 8, 1, w, 1, 1, &c, nullptr, &fp)};
    gol_island untouched;
    memset(&untouched, 0xA5, sizeof untouched);
    for (int rc : einval)
        if (rc != GOL_EINVAL || c != 77 || fp != 77 || !same(r[0], untouched)) {
            printf("a bad argument returned %d\n", rc);
            ++bad;
        }
    if (gol_batch_islands_host(8, 8, 2, w, 1, 0, &c, nullptr, nullptr) != GOL_OK || c != 0) {  // (may be NULL)
        printf("NULL islands and fingerprint: count %lld\n", (long long)c);
        ++bad;
    }
    printf("island_check: %d cases, %d bad\n", n, bad);
    return bad ? 1 : 0;
}
