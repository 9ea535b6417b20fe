// gol_engine_int.h -- what the board engine's translation units share (private): the check
// macros and the few functions that cross files.  State is struct gol_engine / gol_shard
// (gol_internal.h); everything not declared here is static in its file.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <vector>

#include "golhip.h"
#include "gol_comm.h"
#include "gol_internal.h"
#include "gol_launch.h"  // GOL_COUNT_SLOTS

#define NCCLCHK(expr)                                                                             \
    do {                                                                                          \
        ncclResult_t r_ = (expr);                                                                 \
        if (r_ != ncclSuccess)                                                                    \
            return gol_set_error(GOL_ECOMM, "%s failed: %s", #expr, ncclGetErrorString(r_));      \
    } while (0)

#define RCCHK(expr)                  \
    do {                             \
        int rc_ = (expr);            \
        if (rc_ != GOL_OK) return rc_; \
    } while (0)

// The count points of a stepping call: the launch that ends point ci adds its cells into slot
// array 1 + ci % GOL_SLOT_BATCH, and one reduce kernel sums a run of such arrays into counts[]
// (gol_step.cpp flush_counts); array 0 serves single counts (count_into_slots, hash).  Against a
// reduce per point: 65536^2 139.5 -> 140.3 TCUPS, the big boards +0.3 % (same box, 3 reps, same
// counts; profiles/r04/r04l_count_batch.jsonl).
#define GOL_SLOT_BATCH 64
static constexpr size_t SLOT_WORDS = GOL_COUNT_SLOTS * 8;
static constexpr size_t SLOT_BYTES = SLOT_WORDS * sizeof(uint64_t);

#pragma GCC visibility push(hidden)  // none of these is part of the library's exported symbols
// gol_engine.cpp
int sync_all(gol_engine *e, bool collective = true);
int rank_barrier(gol_engine *e);
int agree_step_state(gol_engine *e);
int invalidate_halo(gol_engine *e);
int convert(gol_engine *e, bool to_band);
int ensure_staging(gol_engine *e, gol_shard &s);
int ensure_counts(gol_engine *e, int64_t n);
void free_exact_bytes(gol_shard &s);
// gol_exchange.cpp
int exchange(gol_engine *e, bool on_compute = false);
int exchange_current(gol_engine *e);
// gol_timing.cpp
int timing_begin(gol_engine *e);
int timing_end(gol_engine *e);
int xtime_start(gol_engine *e, gol_shard &s, hipStream_t st, size_t *ev);
int xtime_wait(gol_shard &s, hipStream_t st, size_t ev);
int xtime_waited(gol_shard &s, hipStream_t st, size_t ev);
int xtime_stop(gol_engine *e, gol_shard &s, hipStream_t st, size_t ev, int shard);
// gol_step.cpp
int pick_k(int family, int want, int64_t remaining, int64_t rows, int dw);
int rule_step_check(const gol_engine *e);
int launch_k(gol_engine *e, int k, int64_t count_ci);
int exact_turn(gol_engine *e);
int advance(gol_engine *e, int64_t n, int64_t ci);
// gol_pgm.cpp (HIP-free)
bool gol_pgm_is_space(uint8_t c);
int gol_pgm_parse_header(const uint8_t *h, size_t n, int64_t W, int64_t H, int64_t *off);
int gol_pgm_format_header(char *buf, size_t cap, int64_t W, int64_t H);
#pragma GCC visibility pop

static inline int set_dev(int d)
{
    HIPCHK(hipSetDevice(d));
    return GOL_OK;
}

// Ranks in several processes: whole-board calls are collective (gol_comm).
static inline bool several(const gol_engine *e) { return e->rank_mode && e->nranks > 1; }

// One shard that is the whole torus (LOCAL transport): the step launches read the wrap rows from
// the board itself (step_launch), so there is nothing to exchange.  (Copying them into the ghost
// rows beside the interior instead, for the contiguous-row kernel that ran 1.3-2 % faster in
// tools/step_cost.py, measured -0.5 % on the weak board through bench.py, same box:
// profiles/r04/r04d_ab_steps.jsonl.)
static inline bool local_wrap(const gol_engine *e)
{
    return e->transport == GOL_TRANSPORT_LOCAL && e->sh.size() == 1 && e->nranks == 1;
}

// A stepping call is being timed (timing_begin .. timing_end): launches outside such a call
// (gol_engine_step_flips) are not.
static inline bool timing_open(const gol_engine *e) { return e->timing && e->tcall_ev.size() == e->sh.size(); }

static inline int ensure_standard(gol_engine *e) { return convert(e, false); }

// Shard s's compute stream behind every launch of the last step: the edge stream's (ev_edge) and
// the halo copies (ev_halo).  For sync_all and the queries between steps, never for launch_k.
static inline int join_last_step(gol_shard &s)
{
    HIPCHK(hipStreamWaitEvent(s.stream, s.ev_edge, 0));
    HIPCHK(hipStreamWaitEvent(s.stream, s.ev_halo, 0));
    return GOL_OK;
}

// Shard s's rows of the current board in any mode: `rows` rows from `ptr` (global row gy0), each
// `units` units (uint32 words of a bit board, else bytes), `pitch` units apart.
struct gol_rows {
    void *ptr;
    bool bits;
    int64_t rows, units, pitch, gy0;
    uint32_t *words() const { return static_cast<uint32_t *>(ptr); }
    uint8_t *bytes() const { return static_cast<uint8_t *>(ptr); }
};
static inline gol_rows board_rows(const gol_engine *e, const gol_shard &s)
{
    if (e->mode == GOL_MODE_BITS) return {s.bits[e->cur], true, s.R, e->Wd, e->pitch, s.y0};
    if (e->mode == GOL_MODE_EXACT)  // the loaded bytes before turn 1: row 0 of bytes[0] is the halo row above
        return {s.bytes[0] + e->bstride, false, s.R, e->W, e->bstride, s.y0};
    return {s.bytes[e->bcur], false, e->H, e->W, e->bstride, 0};  // one shard holds the byte board
}
