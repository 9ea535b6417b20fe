// Sanitizer driver for the host twin of the island census (gol_island_host.cpp: gol_batch_islands_host, the row
// functions of gol_island.h that the kernel runs).  A stand-alone program: built only by `make asan` from
// gol_island_host.cpp with AddressSanitizer + UndefinedBehaviorSanitizer, linked without the GPU runtime, and run as a
// plain child process by tests/test_island_ref_cpu.py.  The board is a heap block of its exact size -- (H - 1) * stride
// + ceil(W / 64) words, its padding bits and the words between its rows set -- and the records a heap block of exactly
// `cap` records, so a read or write past either is a sanitizer report.  Every shape runs both reaches at three
// densities and three caps against the flood fill of check_common.h, cell by cell, with its own splitmix64: the count, the
// first min(count, cap) records, the fingerprint, and the records past them untouched.  Then the refusals, which write
// nothing.  Exit status 0: all equal; 1: a difference (printed).
#include "check_common.h"

static int check(int64_t H, int64_t W, int64_t pad, int reach, int density, int64_t cap)
{
    const int64_t stride = (W + 63) / 64 + pad;
    uint64_t *b = random_board(H, W, stride, density);
    std::vector<gol_island> want;
    uint64_t want_fp;
    flood(H, W, reach, GOL_ISLAND_FIXED, cells_of(b, H, W, stride), want, &want_fp);
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
