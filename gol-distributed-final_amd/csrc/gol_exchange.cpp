// gol_exchange.cpp -- the halo exchange of the board engine (gol_engine.cpp): every shard's
// gol_halo_plan executed over one of three transports -- device copies between the shards of one
// process (LOCAL / LOOPBACK), HIP IPC pulls between the ranks of one node, RCCL send/recv.
#include <array>

#include "gol_engine_int.h"

static int copy_rows(gol_shard &dst_s, uint32_t *dst, const gol_shard &src_s, const uint32_t *src, size_t bytes,
                     hipStream_t st)
{
    if (dst_s.device == src_s.device) HIPCHK(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, st));
    else HIPCHK(hipMemcpyPeerAsync(dst, dst_s.device, src, src_s.device, bytes, st));
    return GOL_OK;
}

// The halo plan of local shard i (gol_halo_plan: the schedule golhip.sharded runs as well).
static int plan_of(gol_engine *e, int i, gol_halo_op *ops)  // ops[4]
{
    int32_t n = 0;
    RCCHK(gol_halo_plan(e->H, e->nranks, e->rank + i, e->kx, ops, 4, &n));
#ifdef GOL_TEST_MISPAIR
    // Test build only (make mispair -> libgolhip_mispair.so, tests/test_gpu_ranks.py): the rows
    // received from below land in the ghost rows above and vice versa -- a mis-paired halo that
    // bench.py's parity check must catch.
    int r[2], nr = 0;
    for (int j = 0; j < 4; ++j)
        if (ops[j].kind == GOL_HALO_RECV && nr < 2) r[nr++] = j;
    if (nr == 2) std::swap(ops[r[0]].row, ops[r[1]].row);
#endif
    return n == 4 ? GOL_OK : gol_set_error(GOL_EINVAL, "halo plan of %d ops", n);
}

// IPC transport (one shard per process): this rank's exchange xn on its comm stream, pulling
// each ghost block out of the neighbour's send buffer (ipc_out, mapped by the peers):
//   1. once the rows this rank sends are written (ev_edge), copy every send of my gol_halo_plan
//      into ipc_out slot (xn & 1, op index), then signal READY = xn;
//   2. wait until each neighbour's READY has reached xn (its send rows for this exchange are in);
//   3. copy every receive of my gol_halo_plan from the peer's matching send slot (the peer's nth
//      send to me for my nth receive from it: the pairing RCCL applies to the same plans).
// A neighbour overwrites send slot (xn & 1) only at its exchange xn+2, which follows (on its comm
// stream) its exchange xn+1, which waited for my READY xn+1, which I signal on my comm stream
// after my pulls of xn: so nothing else orders my copies against its writes, whether or not steps
// run between the exchanges.  Peers never read my board, so writes of the board outside a step
// (a load, a layout conversion, the exact first turn) need no cross-process wait either.
static int exchange_ipc(gol_engine *e)
{
    gol_shard &s = e->sh[0];
    RCCHK(set_dev(s.device));
    const int c = e->cur;
    const int64_t P = e->pitch;
    gol_halo_op mine[4];
    RCCHK(plan_of(e, 0, mine));
    const uint32_t xn = ++e->xn;
    const int64_t slot_words = (int64_t)GOL_GHOST_ROWS * P;
    auto out_slot = [&](uint32_t *base, int m) { return base + ((int64_t)(xn & 1) * 4 + m) * slot_words; };
    HIPCHK(hipStreamWaitEvent(s.comm, s.ev_edge, 0));
    size_t xev;
    RCCHK(xtime_start(e, s, s.comm, &xev));
    for (int m = 0; m < 4; ++m)
        if (mine[m].kind == GOL_HALO_SEND) {
            if (mine[m].rows > GOL_GHOST_ROWS) return gol_set_error(GOL_EINVAL, "halo plan: %d rows per send", mine[m].rows);
            HIPCHK(hipMemcpyAsync(out_slot(s.ipc_out, m), s.bits[c] + mine[m].row * P, (size_t)mine[m].rows * P * sizeof(uint32_t),
                                  hipMemcpyDeviceToDevice, s.comm));
        }
    RCCHK(e->ipc->signal(s.comm, GOL_IPC_READY, xn));
    RCCHK(xtime_wait(s, s.comm, xev));
    RCCHK(e->ipc->wait(s.comm, e->ipc_peers, GOL_IPC_READY, xn, s.err));
    RCCHK(xtime_waited(s, s.comm, xev));
    for (int j = 0; j < 4; ++j) {
        const gol_halo_op &rv = mine[j];
        if (rv.kind != GOL_HALO_RECV) continue;
        gol_halo_op theirs[4];
        int32_t n = 0;
        RCCHK(gol_halo_plan(e->H, e->nranks, rv.peer, e->kx, theirs, 4, &n));
        const int sm = gol_halo_match(mine, j, theirs, n, e->rank);  // the peer's send slot (its op index)
        if (sm < 0) return GOL_EINVAL;
        uint32_t *base = rv.peer == e->rank ? s.ipc_out : e->ipc->peer_buf(rv.peer, 0);
        if (!base) return gol_set_error(GOL_ESTATE, "IPC: rank %d is not mapped", rv.peer);
        HIPCHK(hipMemcpyAsync(s.bits[c] + rv.row * P, out_slot(base, sm), (size_t)rv.rows * P * sizeof(uint32_t),
                              hipMemcpyDeviceToDevice, s.comm));
    }
    RCCHK(xtime_stop(e, s, s.comm, xev, 0));
    HIPCHK(hipEventRecord(s.ev_halo, s.comm));
    e->halo_issued = true;
    return GOL_OK;
}

// Exchange the kx halo rows of bits[cur] on the comm streams, once every shard's ev_edge (the
// rows it sends are written) has been recorded; records ev_halo.  Every transport runs the
// shards' gol_halo_plan in issue order.  LOCAL / LOOPBACK execute it as device copies, pairing
// each receive with the sender's matching send exactly as RCCL does (gol_halo_match), so the
// one-GPU loopback tests exercise the RCCL matching of the same plan, including nranks = 2 (one
// peer on both sides) and the one-shard torus wrap (a shard sending to itself).
int exchange(gol_engine *e, bool on_compute)
{
    if (local_wrap(e)) {
        e->halo_issued = false;
        return GOL_OK;
    }
    if (e->transport == GOL_TRANSPORT_IPC) return exchange_ipc(e);
    const int n = (int)e->sh.size();
    const int c = e->cur;
    const int64_t P = e->pitch;
    const size_t hb = (size_t)e->kx * P * sizeof(uint32_t);
    std::vector<std::array<gol_halo_op, 4>> plans(n);
    for (int i = 0; i < n; ++i) RCCHK(plan_of(e, i, plans[i].data()));
    auto local = [&](int global) { return global - e->rank; };  // local shard index of a global rank
    if (e->transport != GOL_TRANSPORT_RCCL) {
        for (int i = 0; i < n; ++i) {
            gol_shard &s = e->sh[i];
            RCCHK(set_dev(s.device));
            // my ghost rows are no longer read (my edge launches) and the rows my peers send me
            // are written (theirs)
            for (const auto &op : plans[i])
                HIPCHK(hipStreamWaitEvent(s.comm, e->sh[local(op.peer)].ev_edge, 0));
            size_t xev = SIZE_MAX;
            for (int j = 0; j < 4; ++j) {
                const gol_halo_op &rv = plans[i][j];
                if (rv.kind != GOL_HALO_RECV) continue;
                const int p = local(rv.peer);
                const int sm = gol_halo_match(plans[i].data(), j, plans[p].data(), 4, e->rank + i);
                if (sm < 0) return GOL_EINVAL;
                const gol_halo_op *sd = &plans[p][sm];  // the peer's rows that land in mine
                gol_shard &ps = e->sh[p];
                if (xev == SIZE_MAX) {  // (the peers' rows are in once the event waits above pass: no wait here)
                    RCCHK(xtime_start(e, s, s.comm, &xev));
                    RCCHK(xtime_wait(s, s.comm, xev));
                    RCCHK(xtime_waited(s, s.comm, xev));
                }
                RCCHK(copy_rows(s, s.bits[c] + rv.row * P, ps, ps.bits[c] + sd->row * P, hb, s.comm));
            }
            RCCHK(xtime_stop(e, s, s.comm, xev, i));
            HIPCHK(hipEventRecord(s.ev_halo, s.comm));
        }
        e->halo_issued = true;
        return GOL_OK;
    }
    // RCCL: one group over every local shard (ncclCommInitAll comms must be driven together),
    // on the comm streams once ev_edge is in, or -- on_compute: after a step whose launches were
    // all on the compute stream (SERIAL) -- right on the compute stream, which orders it after
    // the step and before the next without two cross-stream event hops (config 4's 32768-row
    // share: 0.77 -> 0.74 ms per step)
    auto xs = [&](gol_shard &s) { return on_compute ? s.stream : s.comm; };
    if (!on_compute)
        for (auto &s : e->sh) {
            RCCHK(set_dev(s.device));
            HIPCHK(hipStreamWaitEvent(s.comm, s.ev_edge, 0));
        }
    std::vector<size_t> xev(n);
    bool timed = false;
    for (int i = 0; i < n; ++i) {
        RCCHK(set_dev(e->sh[i].device));
        RCCHK(xtime_start(e, e->sh[i], xs(e->sh[i]), &xev[i]));
        RCCHK(xtime_wait(e->sh[i], xs(e->sh[i]), xev[i]));
        timed |= xev[i] != SIZE_MAX;
    }
    ncclResult_t first = ncclSuccess;
    if (timed) {
        // Only while exchanges are timed (gol_engine_exchange_split): one word to and from each
        // distinct ring neighbour first.  It completes once every neighbour has reached its
        // exchange, so its duration is this rank's wait for them and the group after it is the
        // transfer of the halo rows.  (Device words coll[8..10]: not used by the agreement.)
        first = ncclGroupStart();
        for (int i = 0; i < n && first == ncclSuccess; ++i) {
            gol_shard &s = e->sh[i];
            int peers[4], np = 0;
            for (const auto &op : plans[i])
                if (std::find(peers, peers + np, op.peer) == peers + np) peers[np++] = op.peer;
            for (int j = 0; j < np; ++j) {
                ncclResult_t x = ncclSend(s.coll + 8, 1, ncclUint32, peers[j], s.nccl, xs(s));
                if (x == ncclSuccess) x = ncclRecv(s.coll + 9 + (j & 1), 1, ncclUint32, peers[j], s.nccl, xs(s));
                if (x != ncclSuccess && first == ncclSuccess) first = x;
            }
        }
        const ncclResult_t end = ncclGroupEnd();
        if (first != ncclSuccess || end != ncclSuccess)
            return gol_set_error(GOL_ECOMM, "halo handshake: %s", ncclGetErrorString(first != ncclSuccess ? first : end));
    }
    for (int i = 0; i < n; ++i) {
        RCCHK(set_dev(e->sh[i].device));
        RCCHK(xtime_waited(e->sh[i], xs(e->sh[i]), xev[i]));
    }
    first = ncclGroupStart();
    for (int i = 0; i < n && first == ncclSuccess; ++i) {
        gol_shard &s = e->sh[i];
        uint32_t *mid = s.bits[c];
        for (const auto &op : plans[i]) {
            const size_t cnt = (size_t)op.rows * P;
            const ncclResult_t x = op.kind == GOL_HALO_SEND
                                       ? ncclSend(mid + op.row * P, cnt, ncclUint32, op.peer, s.nccl, xs(s))
                                       : ncclRecv(mid + op.row * P, cnt, ncclUint32, op.peer, s.nccl, xs(s));
            if (x != ncclSuccess && first == ncclSuccess) first = x;
        }
    }
    const ncclResult_t end = ncclGroupEnd();
    if (first != ncclSuccess || end != ncclSuccess)
        return gol_set_error(GOL_ECOMM, "halo exchange: %s", ncclGetErrorString(first != ncclSuccess ? first : end));
    for (int i = 0; i < n; ++i) {
        gol_shard &s = e->sh[i];
        RCCHK(set_dev(s.device));
        RCCHK(xtime_stop(e, s, xs(s), xev[i], i));
        HIPCHK(hipEventRecord(s.ev_halo, xs(s)));
    }
    e->halo_issued = true;
    return GOL_OK;
}

// Exchange the halo of the board as it stands (after a load, a conversion or a step outside
// launch_k): the sent rows are whatever the compute stream wrote last.
int exchange_current(gol_engine *e)
{
    for (auto &s : e->sh) {
        RCCHK(set_dev(s.device));
        HIPCHK(hipStreamWaitEvent(s.stream, s.ev_edge, 0));
        HIPCHK(hipEventRecord(s.ev_edge, s.stream));
    }
    e->halo_on_compute = false;
    RCCHK(exchange(e));
    e->halo_ok = true;
    return GOL_OK;
}
