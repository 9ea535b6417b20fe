// check_common.h -- what the sanitizer check programs of the batch and of the island census share (batch_check.cpp,
// island_check.cpp, island_sym_check.cpp, tally_check.cpp; each a stand-alone program built by `make asan`, which
// includes this file once): the error stub (check_stub.h), the random numbers (one seed, one
// sequence: the programs' random cases are fixed by it), a splitmix64 written out here, the random board as a heap
// block of its exact size, and the references the census programs compare with -- a flood fill cell by cell, a tally
// by a map, and the check of a census of a search.  Nothing here calls the code under test but check_census, which is
// the test of it.
#pragma once
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <map>
#include <vector>

#include "check_stub.h"
#include "golhip.h"

static uint64_t g_state = 0x9E3779B97F4A7C15ULL;
static inline uint64_t rnd()
{
    g_state ^= g_state << 13;
    g_state ^= g_state >> 7;
    g_state ^= g_state << 17;
    return g_state;
}

static inline uint64_t mix(uint64_t x)  // splitmix64, written out here
{
    uint64_t z = x + 0x9E3779B97F4A7C15ULL;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
    return z ^ (z >> 31);
}

// What lies between the rows of a board and in its padding bits: set, and never read.
static const uint64_t GAP = 0xA5A5A5A5A5A5A5A5ULL;
static inline uint64_t tail_of(int64_t W) { return W % 64 ? ((uint64_t)1 << (W % 64)) - 1 : ~(uint64_t)0; }

// A random board of H rows `stride` words apart as a heap block of its exact size, (H - 1) stride + ceil(W / 64) words
// (delete[]): density 0 one cell in 32, 1 one in 8, 2 one in 2; the words between the rows and the padding bits GAP.
static inline uint64_t *random_board(int64_t H, int64_t W, int64_t stride, int density)
{
    const int64_t Ww = (W + 63) / 64;
    const size_t words = (size_t)((H - 1) * stride + Ww);
    const uint64_t tail = tail_of(W);
    uint64_t *b = new uint64_t[words];
    for (size_t i = 0; i < words; ++i) b[i] = GAP;
    for (int64_t y = 0; y < H; ++y)
        for (int64_t w = 0; w < Ww; ++w) {
            uint64_t v = density == 0 ? rnd() & rnd() & rnd() & rnd() & rnd() : (density == 1 ? rnd() & rnd() & rnd() : rnd());
            if (w == Ww - 1) v = (v & tail) | (GAP & ~tail);
            b[y * stride + w] = v;
        }
    return b;
}

// The H x W cells of a board, one byte each.
static inline std::vector<uint8_t> cells_of(const uint64_t *b, int64_t H, int64_t W, int64_t stride)
{
    std::vector<uint8_t> cell((size_t)(H * W));
    for (int64_t y = 0; y < H; ++y)
        for (int64_t x = 0; x < W; ++x) cell[(size_t)(y * W + x)] = (uint8_t)(b[y * stride + x / 64] >> (x % 64) & 1);
    return cell;
}

// The census of the H x W cells of `cell` by the definition of golhip.h, cell by cell.  An island's eight sums are
// taken geometrically: the code in orientation s is read off the board at the mapped offsets (no bit of a code is ever
// moved).  The hash is sum 0 (GOL_ISLAND_FIXED) or the smallest of the eight (GOL_ISLAND_FREE).
static inline void flood(int64_t H, int64_t W, int reach, int symmetry, const std::vector<uint8_t> &cell, std::vector<gol_island> &out,
                         uint64_t *fp)
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
        r.hash = symmetry == GOL_ISLAND_FREE ? *std::min_element(sums, sums + 8) : sums[0];
        out.push_back(r);
        *fp += r.hash;
    }
}

static inline bool same(const gol_island &a, const gol_island &b)
{
    return a.y == b.y && a.x == b.x && a.cells == b.cells && a.rows == b.rows && a.cols == b.cols && a.hash == b.hash;
}

static inline bool same(const gol_island_kind &a, const gol_island_kind &b)
{
    return a.hash == b.hash && a.count == b.count && a.first == b.first && a.cells == b.cells && a.rows == b.rows && a.cols == b.cols;
}

// the tally of the pairs by the definition of golhip.h: a map by hash, then the order
static inline std::vector<gol_island_kind> tally(const gol_island *r, const int64_t *owner, int64_t n)
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

// One census of a search on result arrays of exact size, through gol_batch_census_host (GOL_ISLAND_FIXED) or
// gol_batch_census_sym_host: the first four outputs against gol_batch_search_host with other slots and launches,
// islands and fingerprint against the flood on s(found) re-made here from the soup by `found` single turns, the kinds
// against the map tally of those records.
static inline int check_census(int64_t H, int64_t W, int64_t total, int64_t first, int64_t slots, int64_t launch, int64_t horizon,
                               int reach, int symmetry)
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
    int rc = symmetry == GOL_ISLAND_FIXED
                 ? gol_batch_census_host(H, W, B, S, seed, first, total, slots, launch, horizon, reach, found, period, alive, hash, islands,
                                         fp, kinds, cap, &nk)
                 : gol_batch_census_sym_host(H, W, B, S, seed, first, total, slots, launch, horizon, reach, symmetry, found, period, alive,
                                             hash, islands, fp, kinds, cap, &nk);
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
            flood(H, W, reach, symmetry, cells_of(b, H, W, Ww), recs, &f);
            count = (int64_t)recs.size();
            for (const gol_island &r : recs) all.push_back(r), owners.push_back(first + g);
            delete[] b;
            ++n_found;
        }
        bad += islands[g] != count || fp[g] != f;
    }
    const std::vector<gol_island_kind> want = tally(all.data(), owners.data(), (int64_t)all.size());
    bad += nk != (int64_t)want.size() || nk > cap;
    for (int64_t k = 0; k < nk && !bad; ++k) bad += !same(kinds[k], want[(size_t)k]);
    bad += horizon > 0 && (n_found == 0 || all.empty());  // (a census of nothing would show nothing)
    if (bad)
        printf("%scensus of %lld soups of %lldx%lld from %lld, %lld slots, launch %lld, horizon %lld, reach %d: %lld kinds (%lld), %lld found\n",
               symmetry == GOL_ISLAND_FREE ? "free " : "", (long long)total, (long long)H, (long long)W, (long long)first, (long long)slots,
               (long long)launch, (long long)horizon, reach, (long long)nk, (long long)want.size(), (long long)n_found);
    delete[] found, delete[] period, delete[] islands, delete[] alive, delete[] hash, delete[] fp;
    delete[] found2, delete[] period2, delete[] alive2, delete[] hash2, delete[] kinds;
    return bad ? 1 : 0;
}
