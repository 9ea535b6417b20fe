// gol_batch_int.h -- what the batch's two host units share (private): the handle (struct gol_batch), the device guard
// of a call, the on-demand and the grown device buffers, the per-soup outputs and the census request of a search,
// and the few functions that cross gol_batch_engine.cpp (the handle, rules, stepping, search, copies) and
// gol_batch_census.cpp (the island census, the tally of kinds and their entries).
#pragma once
#include <vector>

#include "gol_batch.h"
#include "gol_batch_kernels.h"
#include "gol_error.h"
#include "gol_island.h"
#include "gol_map.h"

struct gol_batch {
    int64_t n = 0, H = 0, W = 0, Ww = 0;
    int device = 0;
    int tpl = 1;  // turns per launch at most
    bool auto_tpl = false;  // the automatic length: run_cycles sizes each launch by the boards still in it
    int wpb = 1, bpw = 1, nw = 1;
    uint32_t birth = GOL_RULE_BIRTH_CONWAY, survive = GOL_RULE_SURVIVE_CONWAY;
    // empty: every board under birth / survive; else n pairs (birth, survive), not all equal
    std::vector<uint32_t> rules;
    uint32_t *drules = nullptr;  // the device copy of `rules` (on demand), stale while rules_dirty
    bool rules_dirty = false;
    // MAP rules (gol_map.h).  empty: the batch runs under birth / survive or `rules`; 16 words: every board under this
    // map; 16 n words, not all boards equal: a map per board.  Set: `rules` is empty and the masks are not used.
    std::vector<uint32_t> maps;
    uint32_t *dmaps = nullptr;  // the device copy of `maps` (16 n words, on demand), stale while maps_dirty
    bool maps_dirty = false;
    int64_t turn = 0;
    hipStream_t stream = nullptr;
    uint64_t *boards = nullptr;
    uint64_t *prev = nullptr;  // state(start - 1) between the launches of a scanning call (on demand)
    uint64_t *aux = nullptr;   // n words: the settle turns, the counts, the hashes (on demand)
    // run_cycles (on demand): the active list, the finish list (n entries each) and the two counts; the turns left per board
    int32_t *lists = nullptr;
    int64_t *left = nullptr;
    int32_t *hcounts = nullptr;  // pinned host memory: the two counts read back after every launch
    // search (on demand): the active list (n), the harvest list (2 n), the soup per slot (n) and the four counts; born and
    // the found age per slot (2 n); the result tables found, period, alive, hash, islands, fingerprint (grown and reused:
    // tab_words words, six tables of the largest call's soups); four pinned counts
    int32_t *slists = nullptr;
    int64_t *sages = nullptr;
    int64_t *tab = nullptr;
    int64_t tab_words = 0;
    int32_t *scounts = nullptr;
    // islands (on demand, grown and reused): per chunk of boards the counts, the fingerprints and the records
    unsigned char *isl = nullptr;
    int64_t isl_bytes = 0;
    // the tally of kinds (on demand, grown and reused): kind_entries entries, the table's slots and then the counter `dropped`
    gol_island_kind *kind = nullptr;
    int64_t kind_entries = 0;
};

#pragma GCC visibility push(hidden)  // nothing below is part of the library's exported symbols

// The batch's device for the length of a call.
struct OnDevice {
    int before = -1;
    hipError_t err;
    explicit OnDevice(int device)
    {
        err = hipGetDevice(&before);
        if (err == hipSuccess && before != device) err = hipSetDevice(device);
    }
    ~OnDevice()
    {
        if (before >= 0) (void)hipSetDevice(before);
    }
};

// An on-demand device buffer of the batch (prev, aux, lists, left, slists, sages, drules): allocated at its first use,
// freed by gol_batch_destroy.
template <class T>
int need(T *&p, int64_t count)
{
    if (!p) HIPCHK(hipMalloc(&p, (size_t)count * sizeof(T)));
    return GOL_OK;
}

// A grown and reused device buffer of the batch (tab, isl, kind): at least `want` elements (have: those it holds).  The
// old block is freed and the handle says "none" before the new one is asked for, so a failed allocation leaves the
// handle consistent.
template <class T>
int grow(T *&p, int64_t &have, int64_t want)
{
    if (have >= want) return GOL_OK;
    if (p) HIPCHK(hipFree(p));
    p = nullptr;
    have = 0;
    HIPCHK(hipMalloc(&p, (size_t)want * sizeof(T)));
    have = want;
    return GOL_OK;
}

// The per-soup outputs of a search or a census (found is required; islands and fingerprint are a census's).
struct gol_batch_soup_out {
    int64_t *found, *period;
    uint64_t *alive, *hash;
    int64_t *islands;
    uint64_t *fingerprint;
};

// What a census asks for on top of a search.
struct gol_batch_census_ask {
    int32_t reach, symmetry;
    gol_island_kind *kinds;
    int64_t kinds_cap;
    int64_t *n_kinds;
};

// The kind table of one tally call: log2 from kinds_cap (the smallest power of two >= 2 max(kinds_cap, 512), at most 2^24).
struct gol_batch_tally {
    int32_t reach = 1, symmetry = GOL_ISLAND_FIXED, log2 = 0;
    gol_island_kind *table = nullptr;
    int64_t *dropped = nullptr;
};

// The functions that cross the two units.
// gol_batch_engine.cpp: gol_batch_search (ask NULL) and gol_batch_census_sym
int gol_batch_search_call(gol_batch *b, uint64_t seed, int64_t first, int64_t total, int64_t horizon, const gol_batch_soup_out &out,
                          const gol_batch_census_ask *ask, gol_batch_search_stats *stats);
// gol_batch_census.cpp
bool gol_batch_tally_args_ok(const gol_batch_census_ask &ask);
int gol_batch_tally_begin(gol_batch *b, const gol_batch_census_ask &ask, gol_batch_tally *t);
int gol_batch_tally_end(gol_batch *b, const gol_batch_tally &t, const char *what, const gol_batch_census_ask &ask);
#pragma GCC visibility pop
