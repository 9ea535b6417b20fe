// Sanitizer driver for the FREE form of the island census's host twins (gol_island_host.cpp: gol_batch_islands_sym_host,
// gol_island_orient_host; gol_batch_host.cpp: gol_batch_census_sym_host; the row functions of gol_island.h that the
// kernel runs).  A stand-alone program: built only by `make asan` from those two files with AddressSanitizer +
// UndefinedBehaviorSanitizer, linked without the GPU runtime, and run as a plain child process by
// tests/test_island_sym_cpu.py.  The board is a heap block of its exact size -- (H - 1) * stride + ceil(W / 64) words,
// its padding bits and the words between its rows set -- and the records a heap block of exactly `cap` records, so a
// read or write past either is a sanitizer report.
//   - gol_batch_islands_sym_host with GOL_ISLAND_FREE on every shape at both reaches, three densities and three caps
//     against the flood fill of check_common.h, cell by cell, which takes an island's eight sums geometrically: the code
//     in orientation s is read off the board at the mapped offsets (no bit of a code is ever moved), with its own
//     splitmix64; the free hash is their minimum.  And with GOL_ISLAND_FIXED against gol_batch_islands_host.
//   - gol_batch_census_sym_host with GOL_ISLAND_FREE on small searches (check_census of check_common.h): the first
//     four outputs against gol_batch_search_host, islands and fingerprint against that flood on s(found) re-made from
//     the soup by `found` single turns, the kinds against a tally by a map of those records.
//   - gol_island_orient_host outside its domain; the refusals, which write nothing.
// Exit status 0: all equal; 1: a difference (printed).
#include "check_common.h"

static int check(int64_t H, int64_t W, int64_t pad, int reach, int density, int64_t cap)
{
    const int64_t stride = (W + 63) / 64 + pad;
    uint64_t *b = random_board(H, W, stride, density);
    std::vector<gol_island> want;
    uint64_t want_fp;
    flood(H, W, reach, GOL_ISLAND_FREE, cells_of(b, H, W, stride), want, &want_fp);
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
        bad += check_census(16, 16, 24, 0, 5, 7, 300, reach, GOL_ISLAND_FREE), ++n;
        bad += check_census(12, 70, 9, 1000, 3, 64, 200, reach, GOL_ISLAND_FREE), ++n;
        bad += check_census(16, 16, 6, 3, 9, 16, 0, reach, GOL_ISLAND_FREE), ++n;  // horizon 0: nothing found, an empty tally
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
            !same(k[0], no_kind)) {
            printf("a bad argument returned %d\n", rc);
            ++bad;
        }
    printf("island_sym_check: %d cases, %d bad\n", n, bad);
    return bad ? 1 : 0;
}
