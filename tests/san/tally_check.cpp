// Sanitizer driver for the host twins of the tally of island kinds (gol_island_host.cpp: gol_island_tally_host,
// gol_island_tally_home_host; gol_batch_host.cpp: gol_batch_census_host).  A stand-alone program: built only by `make
// asan` from those two files with AddressSanitizer + UndefinedBehaviorSanitizer, linked without the GPU runtime, and
// run as a plain child process by tests/test_tally_ref_cpu.py.  Every input and output is a heap block of its exact
// size, so a read or write past one is a sanitizer report.
//   - gol_island_tally_host on random records of few and of many kinds against the tally by a map of check_common.h, at
//     kinds_cap 0, below and above the number of kinds, the entries past min(n_kinds, kinds_cap) untouched;
//   - gol_batch_census_host on small searches at both reaches (check_census of check_common.h): the first four
//     outputs against gol_batch_search_host, islands and fingerprint against the cell-by-cell flood on s(found)
//     re-made from the soup by `found` single turns, the kinds against the map tally of those records;
//   - the home slot below 2^log2; the refusals, which write nothing.
// Exit status 0: all equal; 1: a difference (printed).
#include "check_common.h"

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
    const std::vector<gol_island_kind> want = tally(r, owner, n);
    int bad = 0;
    for (int64_t cap : {(int64_t)0, (int64_t)3, (int64_t)want.size(), (int64_t)want.size() + 5}) bad += check_kinds(r, owner, n, cap, want);
    delete[] r;
    delete[] owner;
    return bad;
}

int main()
{
    int bad = 0, n = 0;
    static const int tallies[][2] = {{0, 1}, {1, 1}, {2, 1}, {40, 3}, {500, 17}, {500, 400}, {3000, 64}};
    for (const auto &c : tallies) bad += check_tally(c[0], c[1]), ++n;
    for (int reach = 1; reach <= 2; ++reach) {
        bad += check_census(16, 16, 24, 0, 5, 7, 300, reach, GOL_ISLAND_FIXED), ++n;
        bad += check_census(12, 70, 9, 1000, 3, 64, 200, reach, GOL_ISLAND_FIXED), ++n;
        bad += check_census(16, 16, 6, 3, 9, 16, 0, reach, GOL_ISLAND_FIXED), ++n;  // horizon 0: nothing found, an empty tally
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
