// gol_island_host.cpp -- gol_batch_islands_host (include/golhip.h): the island census of one small torus on host
// memory with the rotation, dilation, window and term functions of the census kernel (gol_island.h), in the
// instantiation the kernel picks for the width and the reach, row by row as the lanes do; and
// gol_batch_islands_check_host: the check every launch of the kernel passes (gol_island_launch_ok).  The flood visits
// only the rows round the island so far (the rows a step can change lie within `reach` of them), which is what keeps a
// large sparse board cheap; the rest is the kernel's scheme.  symmetry (the _sym entries; the others are their
// GOL_ISLAND_FIXED calls) selects the hash: FREE sums an island's rows in the eight orientations
// (gol_island_row_hash_free) and keeps the smallest sum, as the kernel does; gol_island_orient_host is orient().  And the tally of island kinds: gol_island_tally_host, the
// definition by a sort and a merge, gol_island_tally_home_host and gol_batch_islands_tally_check_host, the table's home
// function and the check of a TALLY launch.  No HIP header: a stand-alone program links this file alone
// (island_check.cpp).
#include <stdint.h>

#include <algorithm>
#include <vector>

#include "gol_island.h"
#include "golhip.h"

int gol_set_error(int code, const char *fmt, ...);

namespace {

template <int NW, int REACH>
void islands_host(int32_t symmetry, int64_t H, int64_t W, const uint64_t *words, int64_t stride, int64_t cap, int64_t *count,
                  gol_island *islands, uint64_t *fingerprint)
{
    const gol_batch_row g = gol_batch_row_init(W);
    auto row_of = [H](int64_t y) { return (size_t)(((y % H) + H) % H); };
    std::vector<uint32_t> rem((size_t)H * NW), win((size_t)H * (NW + 1)), m((size_t)H * NW, 0u), step;
    for (int64_t y = 0; y < H; ++y) {
        uint32_t c[NW], e[NW + 1];
        for (int j = 0; j < NW; ++j)
            c[j] = (j < g.nwr ? (uint32_t)(words[y * stride + j / 2] >> (32 * (j & 1))) : 0u) & gol_island_keep(g, j);
        gol_island_window_row<NW, REACH>(c, g, (int32_t)W, e);
        for (int j = 0; j < NW; ++j) rem[(size_t)y * NW + j] = c[j];
        for (int j = 0; j <= NW; ++j) win[(size_t)y * (NW + 1) + j] = e[j];
    }
    const int64_t bound = H * W;  // of both loops; it cannot be reached (gol_island.hip)
    int64_t k = 0, from = 0;
    uint64_t fp = 0;
    bool over = false;
    for (;; ++k) {
        // the seed: the lowest remaining cell in row-major order
        int sx = -1;
        for (; from < H && sx < 0; ++from)
            for (int j = 0; j < NW && sx < 0; ++j)
                if (rem[(size_t)from * NW + j]) sx = j * 32 + __builtin_ctz(rem[(size_t)from * NW + j]);
        if (sx < 0) break;
        if (k == bound) {
            over = true;
            break;
        }
        const int64_t sy = --from;  // (the row may hold more islands)
        m[(size_t)sy * NW + sx / 32] = 1u << (sx % 32);
        // the flood over the rows top .. top + len - 1 (mod H) that hold M, widened by REACH either way per step
        int64_t top = sy, len = 1;
        for (int64_t s = 0;; ++s) {
            if (s == bound) {
                over = true;
                break;
            }
            const int64_t ntop = top - REACH, nlen = std::min<int64_t>(H, len + 2 * REACH);
            step.assign((size_t)nlen * NW, 0u);
            bool changed = false;
            for (int64_t i = 0; i < nlen; ++i) {
                const int64_t y = ntop + i;
                uint32_t v[NW], board[NW], next[NW];
                for (int j = 0; j < NW; ++j) v[j] = 0u, board[j] = rem[row_of(y) * NW + j];
                for (int dy = -REACH; dy <= REACH; ++dy)
                    for (int j = 0; j < NW; ++j) v[j] |= m[row_of(y + dy) * NW + j];
                gol_island_dilate<NW, REACH>(board, v, g, next);
                for (int j = 0; j < NW; ++j) {
                    changed = changed || next[j] != m[row_of(y) * NW + j];
                    step[(size_t)i * NW + j] = next[j];
                }
            }
            for (int64_t i = 0; i < nlen; ++i)
                for (int j = 0; j < NW; ++j) m[row_of(ntop + i) * NW + j] = step[(size_t)i * NW + j];
            top = ntop, len = nlen;
            if (!changed) break;
        }
        if (over) break;
        // the record, and M off the remaining cells
        gol_island r = {(int32_t)sy, sx, 0, 0, 0, 0};
        uint32_t cols[NW] = {0u};
        uint64_t sums[8] = {0u};  // FREE: the island's sums in the eight orientations
        for (int64_t i = 0; i < len; ++i) {
            const size_t y = row_of(top + i);
            uint32_t mm[NW], e[2 * REACH + 1][NW + 1], any = 0u;
            for (int j = 0; j < NW; ++j) {
                mm[j] = m[y * NW + j];
                any |= mm[j];
                cols[j] |= mm[j];
                r.cells += __builtin_popcount(mm[j]);
                rem[y * NW + j] &= ~mm[j];
                m[y * NW + j] = 0u;
            }
            if (!any) continue;
            r.rows += 1;
            for (int d = 0; d < 2 * REACH + 1; ++d)
                for (int j = 0; j <= NW; ++j) e[d][j] = win[row_of((int64_t)y + d - REACH) * (NW + 1) + j];
            if (symmetry == GOL_ISLAND_FREE) {
                uint64_t h[8];
                gol_island_row_hash_free<NW, REACH>(mm, e, h);
                for (int s = 0; s < 8; ++s) sums[s] += h[s];
            } else {
                r.hash += gol_island_row_hash<NW, REACH>(mm, e);
            }
        }
        if (symmetry == GOL_ISLAND_FREE) r.hash = gol_island_free_hash(sums);
        for (int j = 0; j < NW; ++j) r.cols += (uint16_t)__builtin_popcount(cols[j]);
        fp += r.hash;
        if (k < cap) islands[k] = r;
    }
    *count = over ? -1 : k;
    if (fingerprint) *fingerprint = fp;
}

template <int NW>
void islands_host_of(int32_t reach, int32_t symmetry, int64_t H, int64_t W, const uint64_t *words, int64_t stride, int64_t cap,
                     int64_t *count, gol_island *islands, uint64_t *fingerprint)
{
    if (reach == 1) islands_host<NW, 1>(symmetry, H, W, words, stride, cap, count, islands, fingerprint);
    else islands_host<NW, 2>(symmetry, H, W, words, stride, cap, count, islands, fingerprint);
}

}  // namespace

extern "C" int gol_batch_islands_sym_host(int64_t H, int64_t W, int32_t reach, int32_t symmetry, const uint64_t *words,
                                          int64_t row_stride, int64_t cap, int64_t *count, gol_island *islands,
                                          uint64_t *fingerprint)
{
    // (the check of a launch of one board, and the rows to read)
    const gol_island_launch l = {words, 1, H, W, reach, symmetry, cap, count, islands, fingerprint};
    if (!gol_island_launch_ok(l) || row_stride < (W + 63) / 64)
        return gol_set_error(GOL_EINVAL,
                             "bad host batch islands (H %lld, W %lld, reach %d, symmetry %d, row stride %lld, cap %lld, or NULL)",
                             (long long)H, (long long)W, reach, symmetry, (long long)row_stride, (long long)cap);
    switch (gol_batch_row_init(W).nw) {
    case 1: islands_host_of<1>(reach, symmetry, H, W, words, row_stride, cap, count, islands, fingerprint); break;
    case 2: islands_host_of<2>(reach, symmetry, H, W, words, row_stride, cap, count, islands, fingerprint); break;
    case 4: islands_host_of<4>(reach, symmetry, H, W, words, row_stride, cap, count, islands, fingerprint); break;
    case 8: islands_host_of<8>(reach, symmetry, H, W, words, row_stride, cap, count, islands, fingerprint); break;
    default: islands_host_of<16>(reach, symmetry, H, W, words, row_stride, cap, count, islands, fingerprint); break;
    }
    return GOL_OK;
}

extern "C" int gol_batch_islands_host(int64_t H, int64_t W, int32_t reach, const uint64_t *words, int64_t row_stride, int64_t cap,
                                      int64_t *count, gol_island *islands, uint64_t *fingerprint)
{
    return gol_batch_islands_sym_host(H, W, reach, GOL_ISLAND_FIXED, words, row_stride, cap, count, islands, fingerprint);
}

extern "C" int gol_batch_islands_sym_check_host(const uint64_t *boards, int64_t n, int64_t H, int64_t W, int32_t reach,
                                                int32_t symmetry, int64_t cap, const int64_t *count, const gol_island *islands,
                                                const uint64_t *fingerprint)
{
    // (the check reads the pointers' values alone)
    const gol_island_launch l = {boards, n, H, W, reach, symmetry, cap, const_cast<int64_t *>(count),
                                 const_cast<gol_island *>(islands), const_cast<uint64_t *>(fingerprint)};
    return gol_island_launch_ok(l) ? GOL_OK : GOL_EINVAL;
}

extern "C" int gol_batch_islands_check_host(const uint64_t *boards, int64_t n, int64_t H, int64_t W, int32_t reach, int64_t cap,
                                            const int64_t *count, const gol_island *islands, const uint64_t *fingerprint)
{
    return gol_batch_islands_sym_check_host(boards, n, H, W, reach, GOL_ISLAND_FIXED, cap, count, islands, fingerprint);
}

extern "C" uint64_t gol_island_orient_host(uint64_t code, int32_t reach, int32_t s) { return gol_island_orient(code, reach, s); }

extern "C" int gol_island_tally_host(const gol_island *records, const int64_t *owners, int64_t n, gol_island_kind *kinds,
                                     int64_t kinds_cap, int64_t *n_kinds)
{
    if (n < 0 || (n > 0 && (!records || !owners)) || kinds_cap < 0 || !n_kinds || (kinds_cap > 0 && !kinds))
        return gol_set_error(GOL_EINVAL, "bad host island tally (%lld records, kinds_cap %lld, or NULL)", (long long)n,
                             (long long)kinds_cap);
    std::vector<gol_island_kind> all;
    try {
        all.reserve((size_t)n);
        for (int64_t i = 0; i < n; ++i)
            all.push_back({gol_island_tally_tag(records[i].hash), 1, owners[i], records[i].cells, records[i].rows, records[i].cols});
    } catch (const std::exception &) {
        return gol_set_error(GOL_ENOMEM, "host island tally: %lld records", (long long)n);
    }
    std::sort(all.begin(), all.end(), [](const gol_island_kind &a, const gol_island_kind &b) { return a.hash < b.hash; });
    size_t kept = 0;  // the merge, in place: all[0 .. kept) the kinds so far
    for (size_t i = 0; i < all.size(); ++i) {
        if (kept == 0 || all[kept - 1].hash != all[i].hash) {
            all[kept++] = all[i];
            continue;
        }
        gol_island_kind &k = all[kept - 1];
        k.count += 1;
        k.first = std::min(k.first, all[i].first);
        if (gol_island_shape_pack(all[i].cells, all[i].rows, all[i].cols) < gol_island_shape_pack(k.cells, k.rows, k.cols))
            k.cells = all[i].cells, k.rows = all[i].rows, k.cols = all[i].cols;
    }
    all.resize(kept);
    std::sort(all.begin(), all.end(), gol_island_kind_before);
    for (size_t i = 0; i < kept && (int64_t)i < kinds_cap; ++i) kinds[i] = all[i];
    *n_kinds = (int64_t)kept;
    return GOL_OK;
}

extern "C" int64_t gol_island_tally_home_host(uint64_t hash, int32_t table_log2)
{
    if (table_log2 < GOL_ISLAND_TALLY_MIN_LOG2 || table_log2 > GOL_ISLAND_TALLY_MAX_LOG2) return -1;
    return (int64_t)gol_island_tally_home(gol_island_tally_tag(hash), table_log2);
}

extern "C" int gol_batch_islands_tally_sym_check_host(const uint64_t *boards, int64_t n, int64_t H, int64_t W, int32_t reach,
                                                      int32_t symmetry, const int32_t *pairs, const int32_t *pair_count,
                                                      int64_t max_pairs, const int64_t *found, int64_t owner0, const int64_t *count,
                                                      const uint64_t *fingerprint, const gol_island_kind *table,
                                                      int32_t table_log2, const int64_t *dropped)
{
    // (the check reads the pointers' values alone; a NULL table is the plain launch, which this entry does not make)
    const gol_island_launch l = {boards, n, H, W, reach, symmetry, 0, const_cast<int64_t *>(count), nullptr,
                                 const_cast<uint64_t *>(fingerprint), const_cast<gol_island_kind *>(table), table_log2,
                                 const_cast<int64_t *>(dropped), owner0, pairs, pair_count, max_pairs, found};
    return table && gol_island_launch_ok(l) ? GOL_OK : GOL_EINVAL;
}

extern "C" int gol_batch_islands_tally_check_host(const uint64_t *boards, int64_t n, int64_t H, int64_t W, int32_t reach,
                                                  const int32_t *pairs, const int32_t *pair_count, int64_t max_pairs,
                                                  const int64_t *found, int64_t owner0, const int64_t *count,
                                                  const uint64_t *fingerprint, const gol_island_kind *table, int32_t table_log2,
                                                  const int64_t *dropped)
{
    return gol_batch_islands_tally_sym_check_host(boards, n, H, W, reach, GOL_ISLAND_FIXED, pairs, pair_count, max_pairs, found, owner0,
                                                  count, fingerprint, table, table_log2, dropped);
}
