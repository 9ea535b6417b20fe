// gol_plan.cpp -- the schedule of a row-sharded step, as data (include/golhip.h, "plans").
//
// The reference partitions rows per turn and ships the whole board to every worker
// (broker.go:135-206, 143-157).  The sharded engine applies the same partition once and, per
// k-turn step, exchanges kx halo rows with the ring neighbours.  What a shard sends and
// receives (gol_halo_plan) and which launches make up a step (gol_step_plan) are computed
// here, in plain host code: the engine (gol_exchange.cpp exchange(), gol_step.cpp launch_k()) executes
// exactly these plans, and so does the Python mirror (golhip.sharded) that the multi-process
// gloo tests drive on the CPU, so both run one schedule.
#include <stdint.h>

#include <vector>

#include "golhip.h"
#include "gol_internal.h"
#include "gol_strips.h"

extern "C" int gol_halo_plan(int64_t H, int32_t nranks, int32_t rank, int32_t k, gol_halo_op *ops, int32_t cap,
                             int32_t *n)
{
    if (!n || nranks < 1 || rank < 0 || rank >= nranks || k < 1 || H < nranks || (cap > 0 && !ops) || cap < 0)
        return gol_set_error(GOL_EINVAL, "bad halo plan arguments (H %lld, rank %d of %d, k %d)", (long long)H, rank,
                             nranks, k);
    int64_t y0 = 0, y1 = 0;
    int rc = gol_partition_rows(H, nranks, rank, &y0, &y1);
    if (rc) return rc;
    const int64_t R = y1 - y0;
    if (k > H / nranks) return gol_set_error(GOL_EINVAL, "k %d exceeds the smallest shard (%lld rows)", k, (long long)(H / nranks));
    const int32_t prev = (rank + nranks - 1) % nranks, next = (rank + 1) % nranks;
    // Issue order.  ncclSend/ncclRecv (and torch's P2P ops) match the sends of one rank to
    // another with that rank's receives from it in issue order.  For nranks = 2 both
    // neighbours are one peer: my first send (top rows) meets the peer's first receive (its
    // bottom ghost rows, the rows below its last row on the torus), my second send (bottom
    // rows) its second receive (top ghost rows).  nranks = 1 sends to itself: the torus wrap.
    const gol_halo_op plan[4] = {
        {GOL_HALO_SEND, prev, 0, k},      // my first k rows -> the rank above (its bottom ghosts)
        {GOL_HALO_RECV, next, R, k},      // ghost rows [R, R+k) <- the first k rows of the rank below
        {GOL_HALO_SEND, next, R - k, k},  // my last k rows -> the rank below (its top ghosts)
        {GOL_HALO_RECV, prev, -k, k},     // ghost rows [-k, 0) <- the last k rows of the rank above
    };
    for (int i = 0; i < 4 && i < cap; ++i) ops[i] = plan[i];
    *n = 4;
    return GOL_OK;
}

// The matching rule above, for a transport that pairs the operations itself (gol_exchange.cpp: the
// device copies of LOCAL / LOOPBACK, the IPC pulls): receive mine[j] is my n-th from its peer, so it
// meets the n-th send to my_rank in `theirs`, that peer's plan.  Returns the send's index there;
// -1 (error set) when there is none or it carries other rows.
int gol_halo_match(const gol_halo_op *mine, int j, const gol_halo_op *theirs, int n_theirs, int my_rank)
{
    int nth = 0;
    for (int jj = 0; jj < j; ++jj) nth += mine[jj].kind == GOL_HALO_RECV && mine[jj].peer == mine[j].peer;
    for (int m = 0, cnt = 0; m < n_theirs; ++m)
        if (theirs[m].kind == GOL_HALO_SEND && theirs[m].peer == my_rank && cnt++ == nth) {
            if (theirs[m].rows == mine[j].rows) return m;
            break;
        }
    (void)gol_set_error(GOL_EINVAL, "halo plan: unmatched receive");
    return -1;
}

extern "C" int gol_step_plan(int64_t R, int32_t k, int32_t kx, int32_t flags, gol_launch *out, int32_t cap,
                             int32_t *n)
{
    if (!n || R < 1 || k < 1 || kx < k || kx > R || cap < 0 || (cap > 0 && !out))
        return gol_set_error(GOL_EINVAL, "bad step plan arguments (R %lld, k %d, kx %d)", (long long)R, k, kx);
    gol_launch plan[3];
    int m = 0;
    const bool split = !(flags & GOL_STEP_SERIAL) && (flags & (GOL_STEP_OVERLAP | GOL_STEP_EDGE_FIRST)) &&
                       R >= 3 * (int64_t)kx;
    if (!split) {
        // one launch over every row, once the halo is in; the next exchange waits for it
        plan[m++] = {GOL_LAUNCH_MAIN, 1, 0, R};
    } else {
        // the rows the next exchange sends (and that need this step's halo) first -- on the edge
        // stream (OVERLAP) or ahead of the interior on the compute stream (EDGE_FIRST); the
        // interior [kx, R - kx) reads no ghost row and runs beside the next exchange
        const int32_t st = (flags & GOL_STEP_OVERLAP) ? GOL_LAUNCH_EDGE : GOL_LAUNCH_MAIN;
        plan[m++] = {st, 1, 0, kx};
        plan[m++] = {st, 1, R - kx, kx};
        plan[m++] = {GOL_LAUNCH_MAIN, 0, kx, R - 2 * (int64_t)kx};
    }
    for (int i = 0; i < m && i < cap; ++i) out[i] = plan[i];
    *n = m;
    return GOL_OK;
}

// The viewport rows a shard holds (include/golhip.h, "viewport frames"): viewport row v is global
// row (y0 + v) mod H, so the viewport is rows [y0, min(y0 + vrows, H)) and, past the torus wrap,
// rows [0, y0 + vrows - H); each part meets the shard's rows [a, b) in at most one run.
extern "C" int gol_view_plan(int64_t H, int32_t nranks, int32_t rank, int64_t y0, int64_t vrows, gol_view_run *runs,
                             int32_t cap, int32_t *n)
{
    if (!n || nranks < 1 || rank < 0 || rank >= nranks || H < nranks || y0 < 0 || y0 >= H || vrows < 1 || vrows > H ||
        cap < 0 || (cap > 0 && !runs))
        return gol_set_error(GOL_EINVAL, "bad view plan arguments (H %lld, rank %d of %d, y0 %lld, %lld rows)",
                             (long long)H, rank, nranks, (long long)y0, (long long)vrows);
    int64_t a = 0, b = 0;
    int rc = gol_partition_rows(H, nranks, rank, &a, &b);
    if (rc) return rc;
    const int64_t wrapped = vrows - (H - y0);  // viewport rows past the torus wrap (no sum that could overflow)
    const int64_t part[2][3] = {
        {y0, wrapped > 0 ? H : y0 + vrows, 0},   // global rows [y0, ..) are viewport rows 0 ..
        {0, wrapped > 0 ? wrapped : 0, H - y0},  // the wrapped rows [0, ..) are viewport rows H - y0 ..
    };
    int m = 0;
    for (const auto &p : part) {
        const int64_t lo = p[0] > a ? p[0] : a, hi = p[1] < b ? p[1] : b;
        if (lo >= hi) continue;
        if (m < cap) runs[m] = {lo - a, hi - lo, p[2] + (lo - p[0])};
        ++m;
    }
    *n = m;
    return GOL_OK;
}

// The strip schedule of a pipelined launch (include/golhip.h, gol_strip_plan): the plan the
// launchers make (gol_strips.h band_strip_plan / bytes_strip_plan) and, per workgroup id, what the
// kernels' own work_item / work_dir / pair_extent give for it.
extern "C" int gol_strip_plan(int32_t kernel, int64_t rows, int64_t row0, int64_t width, int64_t pitch, int32_t k,
                              int32_t strip_rows, int32_t cus, int32_t slots, gol_strip_info *info, gol_strip_rec *recs,
                              int64_t cap, int64_t *n)
{
    using namespace golk;
    const bool band = kernel == GOL_STRIP_KERNEL_BAND;
    const int K = band ? GOL_BAND_KW * GOL_BAND_P : GOL_BYTES_PIPE_KW * GOL_BYTES_PIPE_P;
    if (!n || !info || (!band && kernel != GOL_STRIP_KERNEL_BYTES) || k != K || rows < 1 || row0 < 0 || width < 1 ||
        pitch < 1 || row0 + rows > INT32_MAX || (band ? pitch < width || width % 4 : pitch < width || width % 32) ||
        cus < 0 || slots < 0 || cap < 0 || (cap > 0 && !recs))
        return gol_set_error(GOL_EINVAL, "bad strip plan arguments (kernel %d, rows %lld at %lld, width %lld, pitch %lld, k %d)",
                             kernel, (long long)rows, (long long)row0, (long long)width, (long long)pitch, k);
    const StripPlan p = band ? band_strip_plan(rows, width, pitch, k, strip_rows, cus, slots)
                             : bytes_strip_plan(rows, width, pitch, k, strip_rows, cus, slots);
    const int RPB = band ? GOL_BAND_RPB : GOL_BYTES_RPB, NS = band ? GOL_BAND_NS : GOL_BYTES_NS;
    *info = gol_strip_info{p.mode, p.ngroups, p.strip, K, RPB, NS, p.sm.per_cu, p.sm.period, p.sm.tail_l, p.sm.tail_row,
                           p.sm.tail_strip, 0};
    if (p.nwg > INT32_MAX) return gol_set_error(GOL_EINVAL, "the launch would take %lld workgroups", (long long)p.nwg);
    StripMap sm = p.sm;
    std::vector<uint32_t> counters((size_t)(sm.ranked ? sm.cus : 0) * 2 * 16 + 1);  // as the launchers size them: 16 words each
    sm.claims = counters.data();
    for (int64_t l = 0; l < p.nwg && l < cap; ++l) {
        gol_strip_rec r{};
        int rot = 0;
        uint32_t *ctr = nullptr;
        work_item(sm, p.ngroups, row0, rows, p.strip, (int)l, [&] { return p.nwg; }, r.group, r.s0, r.s1, rot);
        r.dir = work_dir(sm, (int)l, ctr);
        r.claim = r.dir ? (int32_t)((ctr - counters.data()) / 16) : -1;
        if (band) pair_extent<GOL_BAND_KW * GOL_BAND_P, GOL_BAND_RPB, GOL_BAND_NS>(r.dir, r.s0, r.s1, r.s1e, r.nclaim);
        else pair_extent<GOL_BYTES_PIPE_KW * GOL_BYTES_PIPE_P, GOL_BYTES_RPB, GOL_BYTES_NS>(r.dir, r.s0, r.s1, r.s1e, r.nclaim);
        recs[l] = r;
    }
    *n = p.nwg;
    return GOL_OK;
}
