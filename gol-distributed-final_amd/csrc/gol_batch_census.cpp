// gol_batch_census.cpp -- the island census of a batch (include/golhip.h) on the host side: the kind table of a tally
// (its size, its clearing, its one read-back and the sort on the host), the one chunked driver of gol_batch_islands and
// gol_batch_islands_tally (the scratch, a launch per chunk, the counts and fingerprints read back), the records'
// strided copy-out, and the entries gol_batch_islands, gol_batch_islands_tally and gol_batch_census with their _sym
// forms.  The handle and the search that gol_batch_census runs are gol_batch_engine.cpp's (gol_batch_int.h); the kernel is
// gol_island.hip, the host twins gol_island_host.cpp and gol_batch_host.cpp.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <functional>
#include <vector>

#include "gol_batch_int.h"

// The island census cuts its range into chunks whose device scratch (counts, fingerprints, records) is at most this.
// (tests/test_gpu_islands.py, test_batch_islands_across_scratch_chunks, repeats the figure: a call of two chunks.)
#define GOL_ISLAND_SCRATCH_BYTES ((int64_t)256 << 20)

bool gol_batch_tally_args_ok(const gol_batch_census_ask &ask)
{
    return gol_island_mode_ok(ask.reach, ask.symmetry) && ask.kinds_cap >= 0 && ask.kinds_cap <= ((int64_t)1 << 23) && ask.n_kinds &&
           (ask.kinds_cap == 0 || ask.kinds);
}

// The handle's table sized for kinds_cap and set to empty, `dropped` to 0.
int gol_batch_tally_begin(gol_batch *b, const gol_batch_census_ask &ask, gol_batch_tally *t)
{
    t->reach = ask.reach;
    t->symmetry = ask.symmetry;
    t->log2 = 10;
    while (((int64_t)1 << t->log2) < 2 * ask.kinds_cap) t->log2 += 1;
    const int64_t slots = (int64_t)1 << t->log2;
    const int rc = grow(b->kind, b->kind_entries, slots + 1);
    if (rc) return rc;
    t->table = b->kind;
    t->dropped = (int64_t *)(b->kind + slots);
    HIPCHK(golk_island_table_clear(t->table, t->log2, t->dropped, b->stream));
    return GOL_OK;
}

// The one read-back of a tally: `dropped`, and unless it is set the table, its kinds unpacked and sorted.
int gol_batch_tally_end(gol_batch *b, const gol_batch_tally &t, const char *what, const gol_batch_census_ask &ask)
{
    const int64_t slots = (int64_t)1 << t.log2;
    int64_t dropped = 0;
    HIPCHK(hipMemcpyAsync(&dropped, t.dropped, sizeof dropped, hipMemcpyDeviceToHost, b->stream));
    HIPCHK(hipStreamSynchronize(b->stream));
    *ask.n_kinds = -1;
    if (dropped != 0)
        return gol_set_error(GOL_ENOMEM, "batch %s: the table of %lld kinds that kinds_cap %lld asks for is full, %lld islands not tallied",
                             what, (long long)slots, (long long)ask.kinds_cap, (long long)dropped);
    std::vector<gol_island_kind> all;
    try {
        all.resize((size_t)slots);
    } catch (const std::exception &) {
        return gol_set_error(GOL_ENOMEM, "batch %s: a table of %lld kinds", what, (long long)slots);
    }
    HIPCHK(hipMemcpyAsync(all.data(), t.table, (size_t)slots * sizeof(gol_island_kind), hipMemcpyDeviceToHost, b->stream));
    HIPCHK(hipStreamSynchronize(b->stream));
    size_t kept = 0;
    for (const gol_island_kind &k : all)
        if (k.hash != 0) all[kept++] = gol_island_slot_kind(reinterpret_cast<const gol_island_slot &>(k));  // (the device layout)
    all.resize(kept);
    std::sort(all.begin(), all.end(), gol_island_kind_before);
    if (kept) memcpy(ask.kinds, all.data(), (size_t)std::min<int64_t>((int64_t)kept, ask.kinds_cap) * sizeof(gol_island_kind));
    *ask.n_kinds = (int64_t)kept;
    return GOL_OK;
}

namespace {

// What a chunk's records are copied out with: boards [c0, c0 + m), their records on the device from drec on, `most`
// the largest number any of them has to bring back.
typedef std::function<int(int64_t c0, int64_t m, int64_t most, const gol_island *drec)> RecordsOut;

// The census of boards [i0, i1), plain or TALLY, in chunks of at most `per` boards whose scratch (a count, a fingerprint
// and base.cap records per board) fits GOL_ISLAND_SCRATCH_BYTES, one launch each: `base` with the chunk's boards, the
// scratch and, in a tally, the owner of its first board filled in.  A chunk's counts and fingerprints come back whole;
// records_out then sees a chunk that has records to bring back (none with cap 0, so a tally passes an empty one).
// (A tally's scratch is 16 bytes a board and n <= 2^20: one chunk.)
int census_chunks(gol_batch *b, const char *what, int64_t i0, int64_t i1, const gol_island_launch &base, int64_t *count,
                  uint64_t *fingerprint, const RecordsOut &records_out)
{
    const int64_t each = 2 * (int64_t)sizeof(int64_t) + base.cap * (int64_t)sizeof(gol_island);  // bytes of a board's scratch
    const int64_t per = std::min(i1 - i0, std::max<int64_t>(1, GOL_ISLAND_SCRATCH_BYTES / each));
    const int rc = grow(b->isl, b->isl_bytes, per * each);
    if (rc) return rc;
    gol_island_launch l = base;
    l.count = (int64_t *)b->isl;
    l.fingerprint = (uint64_t *)(b->isl + per * 8);
    l.islands = base.cap ? (gol_island *)(b->isl + per * 16) : nullptr;
    for (int64_t c0 = i0; c0 < i1; c0 += per) {
        const int64_t m = std::min(per, i1 - c0);
        l.boards = b->boards + c0 * b->H * b->Ww;
        l.n = m;
        if (l.table) l.owner0 = c0;
        HIPCHK(golk_batch_islands(l, b->stream));
        HIPCHK(hipMemcpyAsync(count + (c0 - i0), l.count, (size_t)m * sizeof(int64_t), hipMemcpyDeviceToHost, b->stream));
        if (fingerprint)
            HIPCHK(hipMemcpyAsync(fingerprint + (c0 - i0), l.fingerprint, (size_t)m * sizeof(uint64_t), hipMemcpyDeviceToHost, b->stream));
        HIPCHK(hipStreamSynchronize(b->stream));
        int64_t most = 0;  // the records to bring back per board
        for (int64_t i = c0; i < c0 + m; ++i) {
            if (count[i - i0] < 0)
                return gol_set_error(GOL_EHIP, "batch %s: board %lld reached the census's trip bound", what, (long long)i);
            most = std::max(most, std::min(count[i - i0], base.cap));
        }
        const int out = most ? records_out(c0, m, most, l.islands) : GOL_OK;
        if (out) return out;
    }
    return GOL_OK;
}

}  // namespace

// The census of boards [i0, i1): of a chunk's records the first min(dcap, the chunk's largest count) of every board come
// back in one strided copy to a host block, from which a board's own records go to the caller's.  No board holds more
// than H W islands, so the device never keeps more records per board than that, whatever cap says.
extern "C" int gol_batch_islands_sym(gol_batch *b, int64_t i0, int64_t i1, int32_t reach, int32_t symmetry, int64_t cap,
                                     int64_t *count, gol_island *islands, uint64_t *fingerprint)
{
    if (!b || !count || i0 < 0 || i0 > i1 || i1 > b->n || !gol_island_mode_ok(reach, symmetry) || cap < 0 || (cap > 0 && !islands))
        return gol_set_error(GOL_EINVAL,
                             "bad batch islands (boards [%lld, %lld) of %lld, reach %d in 1..2, symmetry %d in 0..1, cap %lld, or NULL)",
                             (long long)i0, (long long)i1, b ? (long long)b->n : 0LL, reach, symmetry, (long long)cap);
    if (i0 == i1) return GOL_OK;
    OnDevice dev(b->device);
    HIPCHK(dev.err);
    const int64_t dcap = std::min(cap, b->H * b->W), rec = (int64_t)sizeof(gol_island);
    std::vector<gol_island> stage;
    const RecordsOut records_out = [&](int64_t c0, int64_t m, int64_t most, const gol_island *drec) -> int {
        try {
            stage.resize((size_t)(m * most));
        } catch (const std::exception &) {
            return gol_set_error(GOL_ENOMEM, "batch islands: %lld records of %lld boards", (long long)most, (long long)m);
        }
        HIPCHK(hipMemcpy2DAsync(stage.data(), (size_t)(most * rec), drec, (size_t)(dcap * rec), (size_t)(most * rec), (size_t)m,
                                hipMemcpyDeviceToHost, b->stream));
        HIPCHK(hipStreamSynchronize(b->stream));
        for (int64_t i = c0; i < c0 + m; ++i)
            memcpy(islands + (i - i0) * cap, stage.data() + (i - c0) * most, (size_t)(std::min(count[i - i0], dcap) * rec));
        return GOL_OK;
    };
    const gol_island_launch base = {nullptr, 0, b->H, b->W, reach, symmetry, dcap};  // (the rest 0: plain)
    return census_chunks(b, "islands", i0, i1, base, count, fingerprint, records_out);
}

extern "C" int gol_batch_islands(gol_batch *b, int64_t i0, int64_t i1, int32_t reach, int64_t cap, int64_t *count,
                                 gol_island *islands, uint64_t *fingerprint)
{
    return gol_batch_islands_sym(b, i0, i1, reach, GOL_ISLAND_FIXED, cap, count, islands, fingerprint);
}

// The tally of boards [i0, i1) as they stand: the chunks of gol_batch_islands (counts and fingerprints alone in the
// scratch), each one dense TALLY launch with owner = the board's index, then the table's one read-back.
extern "C" int gol_batch_islands_tally_sym(gol_batch *b, int64_t i0, int64_t i1, int32_t reach, int32_t symmetry, int64_t *count,
                                           uint64_t *fingerprint, gol_island_kind *kinds, int64_t kinds_cap, int64_t *n_kinds)
{
    const gol_batch_census_ask ask = {reach, symmetry, kinds, kinds_cap, n_kinds};
    if (!b || !count || i0 < 0 || i0 > i1 || i1 > b->n || !gol_batch_tally_args_ok(ask))
        return gol_set_error(GOL_EINVAL,
                             "bad batch islands_tally (boards [%lld, %lld) of %lld, reach %d in 1..2, symmetry %d in 0..1, kinds_cap "
                             "%lld in 0..2^23, or NULL)",
                             (long long)i0, (long long)i1, b ? (long long)b->n : 0LL, reach, symmetry, (long long)kinds_cap);
    if (i0 == i1) {
        *n_kinds = 0;
        return GOL_OK;
    }
    OnDevice dev(b->device);
    HIPCHK(dev.err);
    gol_batch_tally t;
    int rc = gol_batch_tally_begin(b, ask, &t);
    if (rc) return rc;
    const gol_island_launch base = {nullptr, 0, b->H, b->W, reach, symmetry, 0, nullptr, nullptr, nullptr, t.table, t.log2, t.dropped};
    rc = census_chunks(b, "islands_tally", i0, i1, base, count, fingerprint, nullptr);
    return rc ? rc : gol_batch_tally_end(b, t, "islands_tally", ask);
}

extern "C" int gol_batch_islands_tally(gol_batch *b, int64_t i0, int64_t i1, int32_t reach, int64_t *count, uint64_t *fingerprint,
                                       gol_island_kind *kinds, int64_t kinds_cap, int64_t *n_kinds)
{
    return gol_batch_islands_tally_sym(b, i0, i1, reach, GOL_ISLAND_FIXED, count, fingerprint, kinds, kinds_cap, n_kinds);
}

extern "C" int gol_batch_census_sym(gol_batch *b, uint64_t seed, int64_t first, int64_t total, int64_t horizon, int32_t reach,
                                    int32_t symmetry, int64_t *found, int64_t *period, uint64_t *alive, uint64_t *hash,
                                    int64_t *islands, uint64_t *fingerprint, gol_island_kind *kinds, int64_t kinds_cap,
                                    int64_t *n_kinds, gol_batch_search_stats *stats)
{
    const gol_batch_census_ask ask = {reach, symmetry, kinds, kinds_cap, n_kinds};
    return gol_batch_search_call(b, seed, first, total, horizon, {found, period, alive, hash, islands, fingerprint}, &ask, stats);
}

extern "C" int gol_batch_census(gol_batch *b, uint64_t seed, int64_t first, int64_t total, int64_t horizon, int32_t reach,
                                int64_t *found, int64_t *period, uint64_t *alive, uint64_t *hash, int64_t *islands,
                                uint64_t *fingerprint, gol_island_kind *kinds, int64_t kinds_cap, int64_t *n_kinds,
                                gol_batch_search_stats *stats)
{
    return gol_batch_census_sym(b, seed, first, total, horizon, reach, GOL_ISLAND_FIXED, found, period, alive, hash, islands,
                                fingerprint, kinds, kinds_cap, n_kinds, stats);
}
