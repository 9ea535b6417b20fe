// gol_step.cpp -- the k-turn step of the board engine (gol_engine.cpp): the choice of k and of the
// step plan, the launches of one step and the exchange that follows it, the exact first turn, the
// stepping calls with their batched count points, and the whole-board count and hash.
#include "gol_engine_int.h"
#include "gol_step_kernels.h"
#include "gol_util_kernels.h"

// Turns per launch: the largest k of (family, dw) in the kernel table (gol_step_launch.h; every
// kernel, the engine-only one included) that is <= want, the remaining turns and the smallest shard.
int pick_k(int family, int want, int64_t remaining, int64_t rows, int dw)
{
    const int k = gol_step_max_k(family, dw, std::min<int64_t>({want, remaining, rows}));
    return k ? k : 1;
}

// The bit board's launches under the engine's rule: the kernel family and the words per lane that
// run them, and their turns per launch.  The rule families have no k above 8, so under them
// e->kx (the exchanged halo, from the Conway k) stays >= k.
static int step_family(const gol_engine *e, bool band)
{
    return e->rule_generic ? (band ? GOL_FAMILY_RULE_BAND : GOL_FAMILY_RULE_STD) : (band ? GOL_FAMILY_BAND : GOL_FAMILY_BITS);
}
static int step_dw(const gol_engine *e, bool band) { return e->rule_generic ? GOLK_RULE_DW : (band ? e->band_dw : e->dw); }
static int step_pick_k(const gol_engine *e, int64_t remaining, bool band)
{
    return pick_k(step_family(e, band), e->k, remaining, e->min_rows, step_dw(e, band));
}

// Stepping calls under a non-B3/S23 rule: the reference's byte semantics (exactly 0 / exactly
// 255) are defined for B3/S23 only, so a board still holding loaded bytes other than 0/255 (its
// exact first turn pending) cannot be stepped.
int rule_step_check(const gol_engine *e)
{
    if (e->rule_generic && e->mode == GOL_MODE_EXACT && (e->birth != 0x008 || e->survive != 0x00C))
        return gol_set_error(GOL_ESTATE, "the board holds loaded bytes other than 0/255: their first turn is defined for B3/S23 only");
    return GOL_OK;
}

// ------------------------------------------------------------------ one k-turn step
static int step_launch(gol_engine *e, gol_shard &s, hipStream_t st, int k, int64_t row0, int64_t rows, uint64_t *slots)
{
    if (rows <= 0) return GOL_OK;
    uint32_t *mid = s.bits[e->cur];
    const uint32_t *top = mid - (int64_t)k * e->pitch, *bot = mid + s.R * e->pitch;  // the ghost rows
    if (local_wrap(e)) {  // the torus wrap straight from the board: rows R-k .. R-1 above, 0 .. k-1 below
        top = mid + (s.R - k) * e->pitch;
        bot = mid;
    }
    const gol_step_launch l = {step_family(e, e->band), top, mid, bot, s.bits[1 - e->cur], s.R, e->Wd, e->pitch, row0, rows, k,
                               step_dw(e, e->band), e->strip, e->birth, e->survive, slots, s.err, 0, 0};
    HIPCHK(golk_step(l, st));
    return GOL_OK;
}

// The step plan of shard s (gol_step_plan flags): as configured, else OVERLAP when the shard's
// launch runs many rounds of workgroups (the edge launches then share the CUs with the interior
// at no cost: +1 % on the 2^17 x 2^20 board), SERIAL when it is a launch of one or a few rounds,
// whose rank-weighted strips (gol_strips.h StripMap) assume they have the CUs to themselves
// (a concurrent edge launch cost 7 % on a 32768 x 262144 shard, profiles/r03a_step_cost).
static int step_mode(gol_engine *e, const gol_shard &s, int k)
{
    if (e->step_flags) return e->step_flags;
    if (local_wrap(e)) return GOL_STEP_SERIAL;  // nothing to exchange, nothing to overlap
    if (e->rule_generic) return GOL_STEP_OVERLAP;  // the rule kernels: equal strips, launches of many rounds
    const double rounds = golk_step_rounds(step_family(e, e->band), s.R, e->Wd, e->pitch, k, step_dw(e, e->band), e->strip);
    return rounds > GOL_OVERLAP_ROUNDS ? GOL_STEP_OVERLAP : GOL_STEP_SERIAL;
}

// k turns of every shard, as gol_step_plan lays them out: the edge rows (they read the halo)
// on the edge stream and the interior beside them on the compute stream; the next step's halo
// exchange starts as soon as the edge rows are written, while the interior is still running.
// With `count` the alive cells of the output are added to each shard's slots.
static uint64_t *batch_slots(gol_shard &s, int64_t ci) { return s.slots + (1 + ci % GOL_SLOT_BATCH) * SLOT_WORDS; }

// Reduce the pending count points' slot arrays into counts[pend_first, pend_first + pend_n) (the
// reduce leaves them zeroed).
static int flush_counts(gol_engine *e)
{
    if (e->pend_n == 0) return GOL_OK;
    for (auto &s : e->sh) {
        RCCHK(set_dev(s.device));
        HIPCHK(golk_slots_reduce(batch_slots(s, e->pend_first), e->pend_n, s.counts + e->pend_first, s.stream));
    }
    e->pend_n = 0;
    return GOL_OK;
}

// Before the counted launch of point ci: the pending run must stay contiguous in the arrays, and
// after a fault every array is zeroed again.
static int batch_begin(gol_engine *e, int64_t ci)
{
    if (e->pend_n && (e->pend_first + e->pend_n != ci || ci % GOL_SLOT_BATCH == 0)) RCCHK(flush_counts(e));
    for (auto &s : e->sh) {
        if (s.batch_zero) continue;
        RCCHK(set_dev(s.device));
        HIPCHK(hipMemsetAsync(s.slots + SLOT_WORDS, 0, SLOT_BYTES * GOL_SLOT_BATCH, s.stream));
        s.batch_zero = true;
    }
    return GOL_OK;
}

#ifndef GOL_LAZY_EVENTS
#define GOL_LAZY_EVENTS 1
#endif
#ifndef GOL_HALO_ON_COMPUTE
#define GOL_HALO_ON_COMPUTE 1
#endif
int launch_k(gol_engine *e, int k, int64_t count_ci)
{
    const bool count = count_ci >= 0;
    if (k > e->kx) return gol_set_error(GOL_EINVAL, "k %d > the exchanged halo (%d rows)", k, e->kx);
    if (!e->halo_ok) RCCHK(exchange_current(e));
    const int n = (int)e->sh.size();
    bool serial = true;  // every shard's launches on its compute stream
    for (int i = 0; i < n; ++i) serial &= step_mode(e, e->sh[i], k) == GOL_STEP_SERIAL;
    // the next step's halo: RCCL after a SERIAL step goes on the compute streams themselves
    const bool on_compute = GOL_HALO_ON_COMPUTE && serial && e->transport == GOL_TRANSPORT_RCCL;
    // A step whose events no other stream reads records none: one shard with nothing to exchange,
    // or an RCCL exchange on the compute streams, and every launch on the compute stream.  Each
    // record is a marker between two band launches that left the GPU idle ~10 us (65536^2: 3 % of
    // a 0.33 ms launch).  ev_edge then keeps an older record, which later waits pass at once
    // (they are all on the compute stream).
    const bool quiet = GOL_LAZY_EVENTS && (local_wrap(e) || on_compute);
    for (int i = 0; i < n; ++i) {
        gol_shard &s = e->sh[i];
        RCCHK(set_dev(s.device));
        gol_launch plan[3];
        int32_t np = 0;
        const int mode = step_mode(e, s, k);
        RCCHK(gol_step_plan(s.R, k, e->kx, mode, plan, 3, &np));
        uint64_t *slots = count ? batch_slots(s, count_ci) : nullptr;  // (zeroed: batch_begin)
        if (timing_open(e)) e->tcall_cells[i] += (double)s.R * (double)e->W * k;
        bool plan_edge = false;
        for (int j = 0; j < np; ++j) plan_edge |= plan[j].stream == GOL_LAUNCH_EDGE;
        const bool markers = !(quiet && !plan_edge);
        if (markers) HIPCHK(hipEventRecord(s.ev_start, s.stream));  // the step's inputs are complete, slots zeroed
        bool edge_used = false, waited[2] = {false, false};
        int last_halo = -1;  // the last launch that reads the halo writes the rows the exchange sends
        for (int j = 0; j < np; ++j)
            if (plan[j].needs_halo) last_halo = j;
        for (int j = 0; j < np; ++j) {
            const gol_launch &L = plan[j];
            const bool on_edge = L.stream == GOL_LAUNCH_EDGE;
            hipStream_t st = on_edge ? s.edge : s.stream;
            if (on_edge && !edge_used) HIPCHK(hipStreamWaitEvent(st, s.ev_start, 0));
            edge_used |= on_edge;
            if (L.needs_halo && !waited[on_edge]) {
                waited[on_edge] = true;
                // the halo is in; and my rows the peers' copies read (LOCAL / LOOPBACK) are no
                // longer read when this launch overwrites them (RCCL on the compute stream:
                // stream order, no wait)
                if (!(e->halo_on_compute && e->transport == GOL_TRANSPORT_RCCL))
                    for (auto &t : e->sh) HIPCHK(hipStreamWaitEvent(st, t.ev_halo, 0));
            }
            RCCHK(step_launch(e, s, st, k, L.row0, L.rows, slots));
            if (j == last_halo && markers) HIPCHK(hipEventRecord(s.ev_edge, st));
        }
        if (edge_used) HIPCHK(hipStreamWaitEvent(s.stream, s.ev_edge, 0));
    }
    if (timing_open(e)) e->tcall_steps += 1;
    e->cur = 1 - e->cur;
    // the next step's halo: waits only for each shard's ev_edge (or, on_compute, stream order)
    e->halo_on_compute = on_compute;
    RCCHK(exchange(e, e->halo_on_compute));
    e->halo_ok = true;
    return GOL_OK;
}

// Turn 1 of a board loaded with bytes other than 0/255 (worker.go:26-37): every shard runs the
// exact byte kernel over its R rows plus the two halo rows it loaded, then packs the result.
int exact_turn(gol_engine *e)
{
    RCCHK(invalidate_halo(e));
    for (auto &s : e->sh) {
        RCCHK(set_dev(s.device));
        HIPCHK(golk_bytes_step(s.bytes[0], s.R + 2, e->W, e->bstride, 1, s.R + 1, s.bytes[1], e->bstride, s.stream));
        HIPCHK(golk_pack(s.bytes[1], s.R, e->W, e->bstride, s.bits[0], e->pitch, nullptr, s.stream));
    }
    e->cur = 0;
    e->band = false;
    e->mode = GOL_MODE_BITS;
    return GOL_OK;
}

// Alive count of the current board through each shard's slots (zeroed first) into its counts[ci].
static int count_into_slots(gol_engine *e, int64_t ci)
{
    for (auto &s : e->sh) {
        RCCHK(set_dev(s.device));
        if (!s.slots_zero) HIPCHK(hipMemsetAsync(s.slots, 0, SLOT_BYTES, s.stream));
        s.slots_zero = false;
        const gol_rows b = board_rows(e, s);
        if (b.bits) HIPCHK(golk_popcount(b.words(), b.rows, b.units, b.pitch, s.slots, s.stream));
        else HIPCHK(golk_count_bytes(b.bytes(), b.rows, b.units, b.pitch, s.slots, s.stream));
    }
    for (auto &s : e->sh) {
        RCCHK(set_dev(s.device));
        HIPCHK(golk_slots_reduce(s.slots, 1, s.counts + ci, s.stream));
        s.slots_zero = true;
    }
    return GOL_OK;
}

// Advance n turns; with ci >= 0 store the alive count after them in every shard's counts[ci].
int advance(gol_engine *e, int64_t n, int64_t ci)
{
    bool counted = false;  // the last launch fused the count
    while (n > 0) {
        counted = false;
        if (e->mode == GOL_MODE_EXACT) {
            RCCHK(exact_turn(e));
            e->turn += 1;
            n -= 1;
            continue;
        }
        if (e->mode == GOL_MODE_BYTES) {  // W % 64 != 0 or GOL_LAYOUT_BYTES: one shard, the byte board
            gol_shard &s = e->sh[0];
            RCCHK(set_dev(s.device));
            const uint8_t *mid = s.bytes[e->bcur];
            if (e->bytes_binary && e->W % 32 == 0) {
                // 0/255 byte board: k turns per launch on the bytes (torus wrap through top/bot)
                const int k = pick_k(GOL_FAMILY_BYTES, e->k, n, e->H, 1);
                const bool last = n == k && ci >= 0;
                if (last) RCCHK(batch_begin(e, ci));
                const gol_step_launch l = {GOL_FAMILY_BYTES, mid + (e->H - k) * e->bstride, mid, mid, s.bytes[1 - e->bcur], e->H, e->W,
                                           e->bstride, 0, e->H, k, 1, e->strip, 0, 0, last ? batch_slots(s, ci) : nullptr, s.err, 0, 0};
                HIPCHK(golk_step(l, s.stream));
                if (timing_open(e)) {
                    e->tcall_cells[0] += (double)e->H * (double)e->W * k;
                    e->tcall_steps += 1;
                }
                e->bcur = 1 - e->bcur;
                e->turn += k;
                n -= k;
                counted = last;
                continue;
            }
            HIPCHK(golk_bytes_step(mid, e->H, e->W, e->bstride, 0, e->H, s.bytes[1 - e->bcur], e->bstride, s.stream));
            e->bcur = 1 - e->bcur;
            e->bytes_binary = true;  // one exact turn leaves only 0/255
            e->turn += 1;
            n -= 1;
            continue;
        }
        if (e->band_capable) RCCHK(convert(e, true));
        const int k = step_pick_k(e, n, e->band);
        const bool last = n == k && ci >= 0;
        if (last) RCCHK(batch_begin(e, ci));
        RCCHK(launch_k(e, k, last ? ci : -1));
        e->turn += k;
        n -= k;
        counted = last;
    }
    if (ci >= 0 && counted) {  // reduced with its run (flush_counts)
        if (e->pend_n == 0) e->pend_first = ci;
        ++e->pend_n;
    } else if (ci >= 0) {
        RCCHK(flush_counts(e));
        RCCHK(count_into_slots(e, ci));
    }
    return GOL_OK;
}

int gol_engine_step_async(gol_engine *e, int64_t turns) { return advance(e, turns, -1); }

extern "C" int gol_engine_step(gol_engine *e, int64_t turns)
{
    if (!e || turns < 0) return gol_set_error(GOL_EINVAL, "bad step arguments");
    RCCHK(rule_step_check(e));
    RCCHK(agree_step_state(e));
    RCCHK(timing_begin(e));
    int rc = advance(e, turns, -1);
    const int rt = timing_end(e);
    if (!rc) rc = rt;
    const int rs = sync_all(e);
    return rc ? rc : rs;
}

// Per-shard counts[0..n) -> the whole board's counts (host sum over local shards, RCCL sum
// over the ranks of other processes).
static int collect_counts(gol_engine *e, int64_t n, uint64_t *out)
{
    std::vector<uint64_t> tmp(e->sh.size() * n);
    for (size_t i = 0; i < e->sh.size(); ++i) {
        gol_shard &s = e->sh[i];
        RCCHK(set_dev(s.device));
        if (several(e)) RCCHK(e->comm->allreduce_sum_u64(s.counts, n, s.stream));
        HIPCHK(hipMemcpyAsync(tmp.data() + i * n, s.counts, n * sizeof(uint64_t), hipMemcpyDeviceToHost, s.stream));
    }
    RCCHK(sync_all(e));
    for (int64_t j = 0; j < n; ++j) {
        uint64_t v = 0;
        for (size_t i = 0; i < e->sh.size(); ++i) v += tmp[i * n + j];
        out[j] = v;
    }
    return GOL_OK;
}

extern "C" int gol_engine_step_counted(gol_engine *e, int64_t turns, int64_t every, uint64_t *counts, int64_t cap)
{
    if (!e || turns < 0 || every <= 0 || (turns / every > 0 && (!counts || cap < turns / every)))
        return gol_set_error(GOL_EINVAL, "bad step_counted arguments (turns %lld, every %lld, cap %lld)", (long long)turns,
                             (long long)every, (long long)cap);
    const int64_t n = turns / every;
    RCCHK(rule_step_check(e));
    RCCHK(ensure_counts(e, n));
    RCCHK(agree_step_state(e));
    e->pend_n = 0;
    int rc = timing_begin(e);
    int64_t left = turns, ci = 0;
    while (left > 0 && rc == GOL_OK) {
        const int64_t seg = std::min(every, left);
        rc = advance(e, seg, seg == every ? ci : -1);
        if (seg == every) ++ci;
        left -= seg;
    }
    if (rc == GOL_OK) rc = flush_counts(e);
    if (rc != GOL_OK && e->pend_n) {  // (arrays of points never reduced: zeroed before the next use)
        e->pend_n = 0;
        for (auto &s : e->sh) s.batch_zero = false;
    }
    if (rc == GOL_OK) rc = timing_end(e);
    else e->tcall_ev.clear();  // (a failed call is not timed: the timing queries stay usable)
    if (rc != GOL_OK) {
        (void)sync_all(e);
        return rc;
    }
    if (n == 0) return sync_all(e);
    return collect_counts(e, n, counts);
}

extern "C" int gol_engine_turn(gol_engine *e, int64_t *turn)
{
    if (!e || !turn) return gol_set_error(GOL_EINVAL, "bad arguments");
    *turn = e->turn;
    return GOL_OK;
}

extern "C" int gol_engine_alive_count(gol_engine *e, uint64_t *count)
{
    if (!e || !count) return gol_set_error(GOL_EINVAL, "bad arguments");
    RCCHK(ensure_counts(e, 1));
    RCCHK(count_into_slots(e, 0));
    return collect_counts(e, 1, count);
}

extern "C" int gol_engine_hash(gol_engine *e, uint64_t *hash)
{
    if (!e || !hash) return gol_set_error(GOL_EINVAL, "bad arguments");
    if (!e->bit_capable) return gol_set_error(GOL_EINVAL, "hash needs a bit board (W %% 64 == 0, layout not BYTES)");
    RCCHK(ensure_standard(e));
    RCCHK(ensure_counts(e, 1));
    for (auto &s : e->sh) {
        RCCHK(set_dev(s.device));
        if (!s.slots_zero) HIPCHK(hipMemsetAsync(s.slots, 0, SLOT_BYTES, s.stream));
        s.slots_zero = false;
        const gol_rows b = board_rows(e, s);
        if (!b.bits)  // loaded non-binary bytes at turn 0: hash the 255-cells
            HIPCHK(golk_pack(b.bytes(), b.rows, b.units, b.pitch, s.bits[0], e->pitch, nullptr, s.stream));
        HIPCHK(golk_hash(b.bits ? b.words() : s.bits[0], b.rows, b.gy0, e->Wd, e->pitch, s.slots, s.stream));
        HIPCHK(golk_slots_reduce(s.slots, 1, s.counts, s.stream));
        s.slots_zero = true;
    }
    return collect_counts(e, 1, hash);
}

// ------------------------------------------------------------------ info
extern "C" int gol_engine_info(gol_engine *e, int32_t *k, int32_t *cells_per_lane, int32_t *strip_rows,
                               int32_t *bit_mode)
{
    if (!e) return gol_set_error(GOL_EINVAL, "engine is NULL");
    const bool bits = e->mode == GOL_MODE_BITS;
    const bool band = bits && e->band_capable;
    const bool blocked = e->mode == GOL_MODE_BYTES && e->bytes_binary && e->W % 32 == 0;  // the 0/255 byte board
    const int family = bits ? step_family(e, band) : (blocked ? GOL_FAMILY_BYTES : GOL_FAMILY_BITS);
    const int dw = bits ? step_dw(e, band) : e->dw;
    // the k of the next launch, as advance() picks it; 1: the exact one-turn kernel (a board before
    // its exact first turn, a byte board of W % 32 != 0 or non-0/255 bytes)
    const int kk = bits ? step_pick_k(e, e->k, band) : (blocked ? pick_k(family, e->k, e->k, e->H, 1) : 1);
    if (k) *k = kk;
    if (cells_per_lane) *cells_per_lane = 32 * dw;
    if (strip_rows) {  // of a one-wave kernel over the smallest shard, as the launch computes it
        gol_step_geometry g;
        gol_step_strips(gol_step_kernel_of(family, kk, blocked ? 1 : dw), e->Wd, e->min_rows, kk, e->strip, g);
        *strip_rows = g.strip;
    }
    if (bit_mode) *bit_mode = bits ? (band ? 2 : 1) : 0;
    return GOL_OK;
}
