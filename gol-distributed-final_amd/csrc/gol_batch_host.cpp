// gol_batch_host.cpp -- gol_batch_step_host (include/golhip.h): one turn of one small torus on host
// memory with the row function of the batch kernel (gol_batch.h), in the instantiation the kernel
// picks for the width, row by row as the lanes do; and gol_batch_cycles_host: the cycle scan of one
// board with that turn and the mark functions the kernel and the engine use; and gol_batch_run_cycles_host: the
// retiring scheme of gol_batch_run_cycles on one board, with the remainder function the retire pass runs; and gol_batch_soup_host and
// gol_batch_search_host: a soup from the fill kernels' word function, and the scheme of gol_batch_search; and
// gol_batch_census_host: that scheme with the island census of every kept s(found) (gol_island_host.cpp) and their tally; and
// gol_batch_step_check_host: the check every launch of the step kernel passes (gol_batch_launch_ok).  No HIP
// header: a stand-alone program links this file and gol_island_host.cpp (batch_check.cpp, tally_check.cpp).
#include <stdint.h>

#include <functional>
#include <vector>

#include "gol_batch.h"
#include "gol_island.h"
#include "golhip.h"

int gol_set_error(int code, const char *fmt, ...);

namespace {

template <int NW>
void step_host(int64_t H, const gol_batch_row &g, uint32_t birth, uint32_t survive, const uint64_t *in, uint64_t *out,
               int64_t stride)
{
    gol_rule_tab tab;
    gol_rule_expand(birth, survive, tab);
    // every row's cells (the padding of the input masked off) and sums first: out may be in
    std::vector<uint32_t> cells((size_t)H * NW), s0((size_t)H * NW), s1((size_t)H * NW);
    for (int64_t y = 0; y < H; ++y) {
        uint32_t c[NW], h0[NW], h1[NW];
        gol_batch_unpack_row(g, in + y * stride, c);
        gol_batch_hsum<NW>(c, g.nwr, g.tb, h0, h1);
        for (int j = 0; j < NW; ++j) {
            cells[(size_t)y * NW + j] = c[j];
            s0[(size_t)y * NW + j] = h0[j];
            s1[(size_t)y * NW + j] = h1[j];
        }
    }
    for (int64_t y = 0; y < H; ++y) {
        const size_t ya = (size_t)((y + H - 1) % H) * NW, yb = (size_t)y * NW, yd = (size_t)((y + 1) % H) * NW;
        uint32_t a0[NW], a1[NW], b0[NW], b1[NW], d0[NW], d1[NW], c[NW], next[NW];
        for (int j = 0; j < NW; ++j) {
            a0[j] = s0[ya + j], a1[j] = s1[ya + j];
            b0[j] = s0[yb + j], b1[j] = s1[yb + j];
            d0[j] = s0[yd + j], d1[j] = s1[yd + j];
            c[j] = cells[yb + j];
        }
        if (gol_batch_conway(birth, survive)) gol_batch_next<NW, false>(tab, g, a0, a1, b0, b1, d0, d1, c, ~0u, next);
        else gol_batch_next<NW, true>(tab, g, a0, a1, b0, b1, d0, d1, c, ~0u, next);
        gol_batch_pack_row(g, next, out + y * stride);
    }
}

// The twins' argument check: one board's shape and rule, and rows of row_stride words to read and to write.
bool args_ok(int64_t H, int64_t W, uint32_t birth, uint32_t survive, const void *in, const void *out, int64_t row_stride)
{
    return gol_batch_shape_ok(1, H, W) && birth < 512 && survive < 512 && in && out && row_stride >= (W + 63) / 64;
}

// One board of a scheme: its shape and rule, and its cells as a dense block with the padding clear.
struct Board {
    int64_t H, W, Ww;
    uint32_t birth, survive;
    std::vector<uint64_t> cur;

    Board(int64_t H, int64_t W, uint32_t birth, uint32_t survive, const uint64_t *in, int64_t row_stride)
        : H(H), W(W), Ww((W + 63) / 64), birth(birth), survive(survive), cur((size_t)(H * Ww))
    {
        for (int64_t y = 0; y < H; ++y)
            for (int64_t w = 0; w < Ww; ++w)
                cur[(size_t)(y * Ww + w)] = in[y * row_stride + w] & (w == Ww - 1 ? gol_batch_tail64(W) : ~(uint64_t)0);
    }
    int step() { return gol_batch_step_host(H, W, birth, survive, cur.data(), cur.data(), Ww); }
    void store(uint64_t *out, int64_t row_stride) const  // (the words between the rows stay)
    {
        for (int64_t y = 0; y < H; ++y)
            for (int64_t w = 0; w < Ww; ++w) out[y * row_stride + w] = cur[(size_t)(y * Ww + w)];
    }
};

// The cycle scan of a board from the mark d = 0, at most `turns` turns: *found = the first d with state(d) == state(the
// last mark before d), else -1.  launch > 0: the scan is cut into launches and ends with the launch the board is found in
// (gol_batch_run_cycles); 0: it runs all its turns.  *made = the turns made.
int scan(Board &b, int64_t turns, int64_t launch, int64_t *found, int64_t *made)
{
    std::vector<uint64_t> snap = b.cur;
    int64_t f = -1, d = 1;
    for (; d <= turns && !(launch > 0 && f >= 0 && (d - 1) % launch == 0); ++d) {
        const int rc = b.step();
        if (rc) return rc;
        if (f < 0 && b.cur == snap) f = d;
        if (gol_batch_is_mark(d)) snap = b.cur;  // (after the comparison: a mark is compared with the mark before it)
    }
    *found = f;
    *made = d - 1;
    return GOL_OK;
}

}  // namespace

extern "C" int gol_batch_step_host(int64_t H, int64_t W, uint32_t birth, uint32_t survive, const uint64_t *in, uint64_t *out,
                                   int64_t row_stride)
{
    if (!args_ok(H, W, birth, survive, in, out, row_stride))
        return gol_set_error(GOL_EINVAL, "bad host batch step (H %lld, W %lld, B 0x%x, S 0x%x, row stride %lld)", (long long)H,
                             (long long)W, birth, survive, (long long)row_stride);
    const gol_batch_row g = gol_batch_row_init(W);
    switch (g.nw) {
    case 1: step_host<1>(H, g, birth, survive, in, out, row_stride); break;
    case 2: step_host<2>(H, g, birth, survive, in, out, row_stride); break;
    case 4: step_host<4>(H, g, birth, survive, in, out, row_stride); break;
    case 8: step_host<8>(H, g, birth, survive, in, out, row_stride); break;
    default: step_host<16>(H, g, birth, survive, in, out, row_stride); break;
    }
    return GOL_OK;
}

extern "C" int gol_batch_run_cycles_host(int64_t H, int64_t W, uint32_t birth, uint32_t survive, const uint64_t *in, uint64_t *out,
                                         int64_t row_stride, int64_t turns, int64_t launch, int64_t *found, int64_t *period,
                                         int64_t *made)
{
    if (!args_ok(H, W, birth, survive, in, out, row_stride) || turns < 0 || !found || launch < 1)
        return gol_set_error(GOL_EINVAL,
                             "bad host batch run_cycles (H %lld, W %lld, B 0x%x, S 0x%x, row stride %lld, turns %lld, launch %lld)",
                             (long long)H, (long long)W, birth, survive, (long long)row_stride, (long long)turns, (long long)launch);
    Board b(H, W, birth, survive, in, row_stride);
    int64_t f = -1, did = 0;
    // the search, in launches: the board leaves at the end of the launch it is found in
    int rc = scan(b, turns, launch, &f, &did);
    // the finish: the turns of the call still to come, modulo the period
    for (int64_t left = f < 0 ? 0 : gol_batch_turns_left(f, turns - did); left > 0 && !rc; --left, ++did) rc = b.step();
    if (rc) return rc;
    *found = f;
    if (period) *period = f < 0 ? -1 : gol_batch_period(f);
    if (made) *made = did;
    b.store(out, row_stride);
    return GOL_OK;
}

// (the scan alone, all its turns: the board never leaves, so there is no remainder to make)
extern "C" int gol_batch_cycles_host(int64_t H, int64_t W, uint32_t birth, uint32_t survive, const uint64_t *in, uint64_t *out,
                                     int64_t row_stride, int64_t turns, int64_t *found, int64_t *period)
{
    if (!args_ok(H, W, birth, survive, in, out, row_stride) || turns < 0 || !found)
        return gol_set_error(GOL_EINVAL, "bad host batch cycles (H %lld, W %lld, B 0x%x, S 0x%x, row stride %lld, turns %lld)",
                             (long long)H, (long long)W, birth, survive, (long long)row_stride, (long long)turns);
    Board b(H, W, birth, survive, in, row_stride);
    int64_t made;
    const int rc = scan(b, turns, 0, found, &made);
    if (rc) return rc;  // (not reached: the arguments are good)
    if (period) *period = *found < 0 ? -1 : gol_batch_period(*found);
    b.store(out, row_stride);
    return GOL_OK;
}

extern "C" int gol_batch_verdict_host(int64_t found, int64_t age, int64_t horizon) { return gol_batch_verdict(found, age, horizon); }

extern "C" int gol_batch_soup_host(int64_t H, int64_t W, uint64_t seed, int64_t index, uint64_t *out, int64_t row_stride)
{
    const int64_t Ww = (W + 63) / 64;
    if (!args_ok(H, W, 0, 0, out, out, row_stride) || index < 0 || index > ((int64_t)1 << 40))
        return gol_set_error(GOL_EINVAL, "bad host batch soup (H %lld, W %lld, index %lld, row stride %lld)", (long long)H,
                             (long long)W, (long long)index, (long long)row_stride);
    for (int64_t y = 0; y < H; ++y)
        for (int64_t w = 0; w < Ww; ++w)
            out[y * row_stride + w] = gol_batch_soup_word(seed, (uint64_t)((index * H + y) * Ww + w), Ww, gol_batch_tail64(W));
    return GOL_OK;
}

namespace {

// gol_batch_search on host memory: the slots, the launches, the restock pass in the list's order and the census of the
// kept snapshot, as the kernels and the driver of gol_batch_engine.cpp have them.  harvested (may be empty) sees every
// found soup's number and its s(found), dense, in the harvest's order.
int search_host(int64_t H, int64_t W, uint32_t birth, uint32_t survive, uint64_t seed, int64_t first, int64_t total, int64_t slots,
                int64_t launch, int64_t horizon, int64_t *found, int64_t *period, uint64_t *alive, uint64_t *hash,
                const std::function<int(int64_t, const uint64_t *)> &harvested)
{
    // (no rows of the caller's: the result arrays stand in for them)
    if (!args_ok(H, W, birth, survive, found, found, (W + 63) / 64) || first < 0 || total < 0 || horizon < 0 ||
        first > ((int64_t)1 << 40) || total > ((int64_t)1 << 26) || first + total > ((int64_t)1 << 40) || slots < 1 || launch < 1)
        return gol_set_error(GOL_EINVAL,
                             "bad host batch search (H %lld, W %lld, B 0x%x, S 0x%x, soups [%lld, +%lld), slots %lld, launch %lld, "
                             "horizon %lld)",
                             (long long)H, (long long)W, birth, survive, (long long)first, (long long)total, (long long)slots,
                             (long long)launch, (long long)horizon);
    const int64_t Ww = (W + 63) / 64, bw = H * Ww, m = slots < total ? slots : total;
    gol_batch_no_results(total, found, period, alive, hash);
    if (total == 0 || horizon == 0) return GOL_OK;
    struct Slot {
        std::vector<uint64_t> cur, snap;
        int64_t soup, born, found;
    };
    std::vector<Slot> slot((size_t)m);
    std::vector<int64_t> active;
    auto fill = [&](Slot &s, int64_t g, int64_t now) {
        s.cur.resize((size_t)bw);
        const int rc = gol_batch_soup_host(H, W, seed, first + g, s.cur.data(), Ww);
        s.snap = s.cur;  // the mark at age 0
        s.soup = g;
        s.born = now;
        s.found = -1;
        return rc;
    };
    for (int64_t i = 0; i < m; ++i) {
        const int rc = fill(slot[(size_t)i], i, 0);
        if (rc) return rc;
        active.push_back(i);
    }
    int64_t next = m;
    for (int64_t done = 0; !active.empty();) {
        for (int64_t i : active) {  // one launch of the aged step kernel
            Slot &s = slot[(size_t)i];
            for (int64_t age = done - s.born + 1; age <= done - s.born + launch; ++age) {
                const bool known = s.found >= 0;  // (before this turn's comparison: the snapshot stays from then on)
                const int rc = gol_batch_step_host(H, W, birth, survive, s.cur.data(), s.cur.data(), Ww);
                if (rc) return rc;
                if (!known && s.cur == s.snap) s.found = age;
                if (gol_batch_is_mark(age) && !known) s.snap = s.cur;
            }
        }
        done += launch;
        std::vector<int64_t> stay;  // the restock pass
        for (int64_t i : active) {
            Slot &s = slot[(size_t)i];
            const int v = gol_batch_verdict(s.found, done - s.born, horizon);
            if (v == GOL_BATCH_STAY) {
                stay.push_back(i);
                continue;
            }
            if (v == GOL_BATCH_FOUND) {  // the harvest: s(found) is the snapshot
                uint64_t a, h;
                gol_batch_board_census(s.snap.data(), bw, &a, &h);
                found[s.soup] = s.found;
                if (period) period[s.soup] = gol_batch_period(s.found);
                if (alive) alive[s.soup] = a;
                if (hash) hash[s.soup] = h;
                const int rc = harvested ? harvested(s.soup, s.snap.data()) : GOL_OK;
                if (rc) return rc;
            }
            if (next < total) {
                const int rc = fill(s, next++, done);
                if (rc) return rc;
                stay.push_back(i);
            }
        }
        active.swap(stay);
    }
    return GOL_OK;
}

}  // namespace

extern "C" int gol_batch_search_host(int64_t H, int64_t W, uint32_t birth, uint32_t survive, uint64_t seed, int64_t first,
                                     int64_t total, int64_t slots, int64_t launch, int64_t horizon, int64_t *found,
                                     int64_t *period, uint64_t *alive, uint64_t *hash)
{
    return search_host(H, W, birth, survive, seed, first, total, slots, launch, horizon, found, period, alive, hash, nullptr);
}

extern "C" int gol_batch_census_sym_host(int64_t H, int64_t W, uint32_t birth, uint32_t survive, uint64_t seed, int64_t first,
                                         int64_t total, int64_t slots, int64_t launch, int64_t horizon, int32_t reach,
                                         int32_t symmetry, int64_t *found, int64_t *period, uint64_t *alive, uint64_t *hash,
                                         int64_t *islands, uint64_t *fingerprint, gol_island_kind *kinds, int64_t kinds_cap,
                                         int64_t *n_kinds)
{
    if (!gol_island_mode_ok(reach, symmetry) || kinds_cap < 0 || !n_kinds || (kinds_cap > 0 && !kinds))
        return gol_set_error(GOL_EINVAL, "bad host batch census (reach %d in 1..2, symmetry %d in 0..1, kinds_cap %lld, or NULL)", reach,
                             symmetry, (long long)kinds_cap);
    // every record of every found soup, then the tally; the outputs are written once nothing can fail
    std::vector<gol_island> records, mine;
    std::vector<int64_t> owners, counts;
    std::vector<uint64_t> fps;
    const int64_t Ww = (W + 63) / 64;
    auto harvested = [&](int64_t soup, const uint64_t *snap) -> int {
        int64_t count = 0;
        uint64_t fp = 0;
        mine.resize((size_t)(H * W));
        const int rc = gol_batch_islands_sym_host(H, W, reach, symmetry, snap, Ww, H * W, &count, mine.data(), &fp);
        if (rc) return rc;
        if (count < 0) return gol_set_error(GOL_EINVAL, "host batch census: soup %lld reached the census's trip bound", (long long)soup);
        records.insert(records.end(), mine.begin(), mine.begin() + count);
        owners.insert(owners.end(), (size_t)count, first + soup);
        counts[(size_t)soup] = count;
        fps[(size_t)soup] = fp;
        return GOL_OK;
    };
    if (total > 0 && total <= ((int64_t)1 << 26)) counts.assign((size_t)total, 0), fps.assign((size_t)total, 0);
    int rc = search_host(H, W, birth, survive, seed, first, total, slots, launch, horizon, found, period, alive, hash, harvested);
    if (!rc) rc = gol_island_tally_host(records.data(), owners.data(), (int64_t)records.size(), kinds, kinds_cap, n_kinds);
    if (rc) return rc;
    for (int64_t g = 0; g < total; ++g) {
        if (islands) islands[g] = counts[(size_t)g];
        if (fingerprint) fingerprint[g] = fps[(size_t)g];
    }
    return GOL_OK;
}

extern "C" int gol_batch_census_host(int64_t H, int64_t W, uint32_t birth, uint32_t survive, uint64_t seed, int64_t first,
                                     int64_t total, int64_t slots, int64_t launch, int64_t horizon, int32_t reach, int64_t *found,
                                     int64_t *period, uint64_t *alive, uint64_t *hash, int64_t *islands, uint64_t *fingerprint,
                                     gol_island_kind *kinds, int64_t kinds_cap, int64_t *n_kinds)
{
    return gol_batch_census_sym_host(H, W, birth, survive, seed, first, total, slots, launch, horizon, reach, GOL_ISLAND_FIXED, found,
                                     period, alive, hash, islands, fingerprint, kinds, kinds_cap, n_kinds);
}

extern "C" int gol_batch_step_check_host(const uint64_t *boards, const uint64_t *prev, const int64_t *settled, int64_t n, int64_t H,
                                         int64_t W, int32_t turns, int64_t turn0, int32_t have_prev, int32_t write_prev,
                                         uint32_t birth, uint32_t survive, const uint32_t *rules, int32_t scan, int64_t done,
                                         const int32_t *list, const int32_t *count, int64_t slots, const int64_t *left,
                                         const int64_t *born)
{
    // (the check reads the pointers' values alone)
    const gol_batch_launch l = {const_cast<uint64_t *>(boards), const_cast<uint64_t *>(prev), const_cast<int64_t *>(settled), n, H, W,
                                turns, turn0, have_prev != 0, write_prev != 0, birth, survive, rules, scan, done, list, count, slots,
                                const_cast<int64_t *>(left), born};
    return gol_batch_launch_ok(l) ? GOL_OK : GOL_EINVAL;
}
