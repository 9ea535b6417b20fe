// gol_timing.cpp -- event timing of the board engine's stepping calls (gol_engine_set_timing):
// the per-shard event pool, the pair around a stepping call, the four events around a halo
// exchange, and the queries that fold them into means.
#include "gol_engine_int.h"

// Timing of one shard-step: events on the compute stream from the step's start to its end
// (the edge stream joined).  The pool is folded into running sums when it is full -- only between
// stepping calls (timing_begin): a call still open holds its start event and its exchanges' events,
// unrecorded or unfolded, so within a call the pool grows instead.
static int fold_timing(gol_engine *e)
{
    for (const auto &t : e->timed) {
        gol_shard &s = e->sh[t.shard];
        RCCHK(set_dev(s.device));
        HIPCHK(hipEventSynchronize(s.tev[t.ev + 1]));
        float x = 0;
        HIPCHK(hipEventElapsedTime(&x, s.tev[t.ev], s.tev[t.ev + 1]));
        if (t.exchange) {
            float w = 0;
            HIPCHK(hipEventElapsedTime(&w, s.tev[t.ev + 2], s.tev[t.ev + 3]));
            e->x_ms += x;
            e->x_wait_ms += w;
            e->x_n += 1;
            continue;
        }
        e->t_ms += x;
        e->t_cells += t.cell_updates;
        e->t_n += t.steps;
    }
    e->timed.clear();
    for (auto &s : e->sh) s.tused = 0;
    return GOL_OK;
}

// n consecutive events of shard s's pool (never folds: see fold_timing).
static int timing_event(gol_shard &s, size_t *ev, size_t n = 2)
{
    while (s.tused + n > s.tev.size()) {
        hipEvent_t x;
        HIPCHK(hipEventCreate(&x));
        s.tev.push_back(x);
    }
    *ev = s.tused;
    s.tused += n;
    return GOL_OK;
}

// Timing of one stepping call (gol_engine_set_timing): one event pair per shard on its compute
// stream around all the call's launches (per-launch events cost the GPU ~10-30 us each, a large
// share of a 0.4 ms step), averaged over its steps by gol_engine_timing.
int timing_begin(gol_engine *e)
{
    if (!e->timing) return GOL_OK;
    bool full = false;
    for (const auto &s : e->sh) full |= s.tused + 2 > GOL_TIMING_EVENTS;
    if (full) RCCHK(fold_timing(e));  // (no call is open here)
    e->tcall_ev.assign(e->sh.size(), 0);
    e->tcall_cells.assign(e->sh.size(), 0.0);
    e->tcall_steps = 0;
    for (size_t i = 0; i < e->sh.size(); ++i) {
        gol_shard &s = e->sh[i];
        int rc = set_dev(s.device);
        if (rc == GOL_OK) rc = timing_event(s, &e->tcall_ev[i]);
        if (rc == GOL_OK && hipEventRecord(s.tev[e->tcall_ev[i]], s.stream) != hipSuccess)
            rc = gol_set_error(GOL_EHIP, "timing: hipEventRecord failed");
        if (rc != GOL_OK) {
            e->tcall_ev.clear();  // no call is open
            return rc;
        }
    }
    return GOL_OK;
}

// GOL_TIMING_EXCHANGE: four events around one shard's part of a halo exchange on stream st --
// xtime_start before the exchange's first operation on st, xtime_wait / xtime_waited around the
// part that waits for the neighbours (gol_engine_exchange_split), xtime_stop after its last.
int xtime_start(gol_engine *e, gol_shard &s, hipStream_t st, size_t *ev)
{
    *ev = SIZE_MAX;
    if (!e->timing_x || !timing_open(e)) return GOL_OK;
    RCCHK(timing_event(s, ev, 4));
    HIPCHK(hipEventRecord(s.tev[*ev], st));
    return GOL_OK;
}
int xtime_wait(gol_shard &s, hipStream_t st, size_t ev)
{
    if (ev != SIZE_MAX) HIPCHK(hipEventRecord(s.tev[ev + 2], st));
    return GOL_OK;
}
int xtime_waited(gol_shard &s, hipStream_t st, size_t ev)
{
    if (ev != SIZE_MAX) HIPCHK(hipEventRecord(s.tev[ev + 3], st));
    return GOL_OK;
}
int xtime_stop(gol_engine *e, gol_shard &s, hipStream_t st, size_t ev, int shard)
{
    if (ev == SIZE_MAX) return GOL_OK;
    HIPCHK(hipEventRecord(s.tev[ev + 1], st));
    gol_timed t{shard, ev, 0.0, 0};
    t.exchange = true;
    e->timed.push_back(t);
    return GOL_OK;
}

int timing_end(gol_engine *e)
{
    if (!timing_open(e)) return GOL_OK;
    for (size_t i = 0; i < e->sh.size(); ++i) {
        gol_shard &s = e->sh[i];
        RCCHK(set_dev(s.device));
        HIPCHK(hipStreamWaitEvent(s.stream, s.ev_edge, 0));  // (edge launches of the last step)
        HIPCHK(hipEventRecord(s.tev[e->tcall_ev[i] + 1], s.stream));
        if (e->tcall_steps > 0) e->timed.push_back({(int)i, e->tcall_ev[i], e->tcall_cells[i], e->tcall_steps});
    }
    e->tcall_ev.clear();
    return GOL_OK;
}

extern "C" int gol_engine_set_timing(gol_engine *e, int32_t enable)
{
    if (!e) return gol_set_error(GOL_EINVAL, "engine is NULL");
    for (auto &s : e->sh) {  // events of earlier steps may still be pending
        RCCHK(set_dev(s.device));
        HIPCHK(hipStreamSynchronize(s.stream));
    }
    e->timing = enable != 0;
    e->timing_x = enable == GOL_TIMING_EXCHANGE;
    e->timed.clear();
    for (auto &s : e->sh) s.tused = 0;
    e->t_ms = e->t_cells = 0;
    e->t_n = 0;
    e->x_ms = e->x_wait_ms = 0;
    e->x_n = 0;
    return GOL_OK;
}

// Local, like gol_engine_timing.
extern "C" int gol_engine_exchange_timing(gol_engine *e, int64_t *exchanges, double *mean_ms)
{
    if (!e || !exchanges || !mean_ms) return gol_set_error(GOL_EINVAL, "bad arguments");
    if (timing_open(e)) return gol_set_error(GOL_ESTATE, "a timed stepping call is in progress");
    RCCHK(fold_timing(e));
    *exchanges = e->x_n;
    *mean_ms = e->x_n ? e->x_ms / e->x_n : 0.0;
    return GOL_OK;
}

extern "C" int gol_engine_exchange_split(gol_engine *e, int64_t *exchanges, double *mean_wait_ms, double *mean_transfer_ms)
{
    if (!e || !exchanges || !mean_wait_ms || !mean_transfer_ms) return gol_set_error(GOL_EINVAL, "bad arguments");
    if (timing_open(e)) return gol_set_error(GOL_ESTATE, "a timed stepping call is in progress");
    RCCHK(fold_timing(e));
    *exchanges = e->x_n;
    *mean_wait_ms = e->x_n ? e->x_wait_ms / e->x_n : 0.0;
    *mean_transfer_ms = e->x_n ? (e->x_ms - e->x_wait_ms) / e->x_n : 0.0;
    return GOL_OK;
}

// Local (not collective): waits only for this process's timed steps.
extern "C" int gol_engine_timing(gol_engine *e, int64_t *launches, double *mean_ms, double *mean_cell_updates)
{
    if (!e || !launches || !mean_ms || !mean_cell_updates) return gol_set_error(GOL_EINVAL, "bad arguments");
    if (timing_open(e)) return gol_set_error(GOL_ESTATE, "a timed stepping call is in progress");
    RCCHK(fold_timing(e));
    const int64_t n = e->t_n;
    *launches = n;
    *mean_ms = n ? e->t_ms / n : 0.0;
    *mean_cell_updates = n ? e->t_cells / n : 0.0;
    return GOL_OK;
}
