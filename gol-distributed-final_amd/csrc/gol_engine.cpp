// gol_engine.cpp -- the board engine of libgolhip.so: a Game-of-Life torus resident in HBM,
// on one GPU or row-sharded over several (include/golhip.h, "engine").
//
// The reference keeps the board in the broker and ships ALL of it to every worker every turn
// (broker.go:143-157, 182-211), then gathers the slabs and copies them into cWorld
// (broker.go:153-169).  Here the broker's row partition (broker.go:135-206) is applied once,
// to GPUs: shard r keeps rows [y0_r, y1_r) bit-packed in its own HBM for the whole run, and the
// only traffic between shards is a k-row halo every k turns (RCCL send/recv over xGMI, or
// device copies between the shards of one process).
//
// This file: construction and teardown, the synchronisation points, the ranks' agreement and the
// layout conversion.  The halo exchange is gol_exchange.cpp, the k-turn step gol_step.cpp, event
// timing gol_timing.cpp, byte / PGM / word I/O and the cell lists gol_board_io.cpp, the viewport
// frames and the paste gol_frames.cpp, the P5 header gol_pgm.cpp (gol_engine_int.h).
#include "gol_engine_int.h"
#include "gol_step_kernels.h"

// The IPC transport's send buffer (exchange_ipc): 2 exchange parities x 4 plan ops x the ghost rows.
static size_t ipc_out_bytes(const gol_engine *e) { return (size_t)2 * 4 * GOL_GHOST_ROWS * e->pitch * sizeof(uint32_t); }

// ------------------------------------------------------------------ allocation
int ensure_staging(gol_engine *e, gol_shard &s)
{
    if (!s.staging) {
        // byte staging for chunked load/store/PGM: >= 1 row, <= 64 MiB
        const int64_t rows = std::max<int64_t>(s.R, 1);
        s.stage_rows = std::max<int64_t>(1, std::min<int64_t>(rows, (64LL << 20) / e->bstride));
        HIPCHK(hipMalloc(&s.staging, s.stage_rows * e->bstride));
        HIPCHK(hipHostMalloc((void **)&s.host_staging, s.stage_rows * e->bstride, hipHostMallocDefault));
    }
    return GOL_OK;
}

int ensure_counts(gol_engine *e, int64_t n)  // every shard's counts[0, n)
{
    for (auto &s : e->sh) {
        RCCHK(set_dev(s.device));
        if (s.counts_cap >= n) continue;
        if (s.counts) (void)hipFree(s.counts);
        s.counts = nullptr;
        s.counts_cap = 0;
        const int64_t cap = std::max<int64_t>(n, 64);
        HIPCHK(hipMalloc(&s.counts, cap * sizeof(uint64_t)));
        s.counts_cap = cap;
    }
    return GOL_OK;
}

void free_exact_bytes(gol_shard &s)
{
    for (auto &b : s.bytes)
        if (b) { (void)hipFree(b); b = nullptr; }
}

static void shard_release(gol_shard &s)
{
    (void)hipSetDevice(s.device);
    if (s.stream) (void)hipStreamSynchronize(s.stream);
    if (s.edge) (void)hipStreamSynchronize(s.edge);
    if (s.comm) (void)hipStreamSynchronize(s.comm);
    if (s.nccl) (void)ncclCommDestroy(s.nccl);
    if (s.stream) golk_release_claims(s.stream);
    if (s.edge) golk_release_claims(s.edge);
    for (auto &b : s.bits_alloc)
        if (b) (void)hipFree(b);
    free_exact_bytes(s);
    if (s.slots) (void)hipFree(s.slots);
    if (s.counts) (void)hipFree(s.counts);
    if (s.flag) (void)hipFree(s.flag);
    if (s.err) (void)hipFree(s.err);
    if (s.coll) (void)hipFree(s.coll);
    if (s.ipc_out) (void)hipFree(s.ipc_out);
    if (s.host_word) (void)hipHostFree(s.host_word);
    if (s.staging) (void)hipFree(s.staging);
    if (s.host_staging) (void)hipHostFree(s.host_staging);
    for (gol_scratch *b : {&s.view, &s.edit, &s.read}) {
        if (b->dev) (void)hipFree(b->dev);
        if (b->host) (void)hipHostFree(b->host);
    }
    for (auto ev : s.tev) (void)hipEventDestroy(ev);
    for (hipEvent_t ev : {s.ev_start, s.ev_edge, s.ev_halo})
        if (ev) (void)hipEventDestroy(ev);
    for (hipStream_t st : {s.stream, s.edge, s.comm})
        if (st) (void)hipStreamDestroy(st);
    s = gol_shard();
}

static int shard_alloc(gol_engine *e, gol_shard &s)
{
    RCCHK(set_dev(s.device));
    for (hipStream_t *st : {&s.stream, &s.edge, &s.comm}) HIPCHK(hipStreamCreateWithFlags(st, hipStreamNonBlocking));
    golk_own_stream(s.stream);
    golk_own_stream(s.edge);
    for (hipEvent_t *ev : {&s.ev_start, &s.ev_edge, &s.ev_halo}) HIPCHK(hipEventCreateWithFlags(ev, hipEventDisableTiming));
    HIPCHK(hipMalloc(&s.slots, SLOT_BYTES * (1 + GOL_SLOT_BATCH)));
    HIPCHK(hipMalloc(&s.flag, sizeof(uint32_t)));
    HIPCHK(hipMalloc(&s.err, sizeof(uint32_t)));
    HIPCHK(hipMalloc(&s.coll, GOL_COLL_WORDS * sizeof(uint32_t)));
    HIPCHK(hipHostMalloc((void **)&s.host_word, GOL_HOST_WORDS * sizeof(uint32_t), hipHostMallocDefault));
    // on the shard's stream: it is non-blocking, so a null-stream memset could still be running
    // when the first load or fill kernel writes the board
    HIPCHK(hipMemsetAsync(s.err, 0, sizeof(uint32_t), s.stream));
    if (e->bit_capable) {
        const int64_t rows = s.R + 2 * GOL_GHOST_ROWS;
        for (int i = 0; i < 2; ++i) {
            HIPCHK(hipMalloc(&s.bits_alloc[i], rows * e->pitch * sizeof(uint32_t)));
            HIPCHK(hipMemsetAsync(s.bits_alloc[i], 0, rows * e->pitch * sizeof(uint32_t), s.stream));
            s.bits[i] = s.bits_alloc[i] + GOL_GHOST_ROWS * e->pitch;
        }
    } else {
        for (auto &b : s.bytes) HIPCHK(hipMalloc(&b, e->H * e->bstride));
        HIPCHK(hipMemsetAsync(s.bytes[0], 0, e->H * e->bstride, s.stream));
        e->bytes_binary = true;  // an all-dead board: 0/255 only
    }
    HIPCHK(hipStreamSynchronize(s.stream));
    return GOL_OK;
}

// Board geometry and kernel parameters from the configuration (shared by both constructors).
static int engine_setup(gol_engine *e, int64_t H, int64_t W, const gol_config *cfg)
{
    if (H <= 0 || W <= 0 || W > (int64_t)INT32_MAX * 32 || H > INT32_MAX)
        return gol_set_error(GOL_EINVAL, "bad board size %lldx%lld", (long long)W, (long long)H);
    e->H = H;
    e->W = W;
    const int layout = cfg ? cfg->layout : GOL_LAYOUT_AUTO;
    if (layout < GOL_LAYOUT_AUTO || layout > GOL_LAYOUT_BYTES)
        return gol_set_error(GOL_EINVAL, "layout must be GOL_LAYOUT_AUTO, _STANDARD, _BAND or _BYTES");
    e->bit_capable = (W % 64) == 0 && layout != GOL_LAYOUT_BYTES;
    e->mode = e->bit_capable ? GOL_MODE_BITS : GOL_MODE_BYTES;
    e->Wd = W / 32;
    e->pitch = (e->Wd + 3) / 4 * 4;
    e->bstride = (W + 15) / 16 * 16;
    e->k = (cfg && cfg->turns_per_launch > 0) ? cfg->turns_per_launch : 0;  // 0: per layout, below
    const int req = cfg ? cfg->cells_per_lane : 0;
    const int cpl = req > 0 ? req : 32 * GOL_DEFAULT_DW;
    if (cpl != 32 && cpl != 64 && cpl != 128) return gol_set_error(GOL_EINVAL, "cells_per_lane must be 32, 64 or 128");
    e->dw = cpl / 32;
    while (e->dw > 1 && (e->Wd % e->dw) != 0) e->dw >>= 1;
    e->band_dw = req == 64 ? 2 : (req == 128 ? 4 : GOL_BAND_DEFAULT_DW);
    e->strip = cfg ? cfg->strip_rows : 0;
    if (layout == GOL_LAYOUT_BAND && W % 1024 != 0) return gol_set_error(GOL_EINVAL, "the band layout needs W %% 1024 == 0");
    e->band_capable = e->bit_capable && layout != GOL_LAYOUT_STANDARD && W % 1024 == 0;
    if (e->k == 0)
        e->k = !e->bit_capable ? GOL_DEFAULT_BYTES_K
                               : ((e->band_capable && e->band_dw == 4) ? GOL_DEFAULT_BAND_K : GOL_DEFAULT_K);
    e->step_flags = cfg ? (cfg->flags & (GOL_STEP_SERIAL | GOL_STEP_EDGE_FIRST | GOL_STEP_OVERLAP)) : 0;
    return GOL_OK;
}

// Shards [0, n) of this process are global ranks e->rank + i of e->nranks.
static int engine_shards(gol_engine *e, const std::vector<int> &devices)
{
    if (e->nranks > 1 && !e->bit_capable)
        return gol_set_error(GOL_EINVAL, "a sharded board needs a bit board: W %% 64 == 0 (W = %lld), layout not BYTES", (long long)e->W);
    if (e->H < e->nranks)
        return gol_set_error(GOL_EINVAL, "%d shards cannot split %lld rows", e->nranks, (long long)e->H);
    e->min_rows = e->H / e->nranks;  // broker.go:172-206: the smallest shard
    // every exchange carries the rows of the longest launch the engine makes
    e->kx = pick_k(e->band_capable ? GOL_FAMILY_BAND : GOL_FAMILY_BITS, e->k, INT64_MAX, e->min_rows, e->band_capable ? e->band_dw : e->dw);
    e->sh.resize(devices.size());
    for (size_t i = 0; i < devices.size(); ++i) {
        gol_shard &s = e->sh[i];
        s.device = devices[i];
        const int64_t r = e->rank + (int64_t)i;
        int rc = gol_partition_rows(e->H, e->nranks, r, &s.y0, &s.y1);
        if (rc) return rc;
        s.R = s.y1 - s.y0;
        RCCHK(shard_alloc(e, s));
    }
    return GOL_OK;
}

extern "C" int gol_engine_create(int64_t H, int64_t W, const gol_config *cfg, gol_engine **out)
{
    if (!out) return gol_set_error(GOL_EINVAL, "out is NULL");
    *out = nullptr;
    gol_engine *e = new gol_engine();
    int rc = engine_setup(e, H, W, cfg);
    const int n = cfg && cfg->shards > 1 ? cfg->shards : 1;
    const int same = cfg && (cfg->flags & GOL_SHARDS_SAME_DEVICE);
    int transport = cfg ? cfg->transport : GOL_TRANSPORT_AUTO;
    std::vector<int> devs(n);
    if (rc == GOL_OK) {
        int dev0 = cfg ? cfg->device : -1, ndev = 0;
        if (dev0 < 0 && hipGetDevice(&dev0) != hipSuccess) dev0 = 0;
        if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
            rc = gol_set_error(GOL_EHIP, "no HIP device");
        for (int i = 0; rc == GOL_OK && i < n; ++i) devs[i] = same ? dev0 : (dev0 + i) % ndev;
        std::vector<int> sorted(devs);
        std::sort(sorted.begin(), sorted.end());
        const bool distinct = std::unique(sorted.begin(), sorted.end()) == sorted.end();
        if (transport == GOL_TRANSPORT_AUTO)
            transport = n == 1 ? GOL_TRANSPORT_LOCAL : (distinct ? GOL_TRANSPORT_RCCL : GOL_TRANSPORT_LOOPBACK);
        if (transport != GOL_TRANSPORT_LOCAL && transport != GOL_TRANSPORT_LOOPBACK && transport != GOL_TRANSPORT_RCCL)
            rc = gol_set_error(GOL_EINVAL, "unknown transport %d", transport);
        if (transport == GOL_TRANSPORT_LOCAL && n > 1) rc = gol_set_error(GOL_EINVAL, "the local transport has one shard");
    }
    e->nranks = n;
    e->rank = 0;
    e->transport = transport;
    if (rc == GOL_OK) rc = engine_shards(e, devs);
    if (rc == GOL_OK && transport == GOL_TRANSPORT_RCCL) {
        std::vector<ncclComm_t> comms(n);
        ncclResult_t r = ncclCommInitAll(comms.data(), n, devs.data());
        if (r != ncclSuccess) rc = gol_set_error(GOL_ECOMM, "ncclCommInitAll(%d GPUs): %s", n, ncclGetErrorString(r));
        else
            for (int i = 0; i < n; ++i) e->sh[i].nccl = comms[i];
    }
    if (rc == GOL_OK && transport == GOL_TRANSPORT_LOOPBACK)  // peer access between distinct GPUs (copies work without)
        for (int i = 0; i < n; ++i)
            for (int j = 0; j < n; ++j)
                if (devs[i] != devs[j] && hipSetDevice(devs[i]) == hipSuccess) {
                    (void)hipDeviceEnablePeerAccess(devs[j], 0);
                    (void)hipGetLastError();
                }
    if (rc != GOL_OK) {
        gol_engine_destroy(e);
        return rc;
    }
    *out = e;
    return GOL_OK;
}

extern "C" int gol_rccl_unique_id(uint8_t *id, int64_t len)
{
    if (!id || len < (int64_t)sizeof(ncclUniqueId)) return gol_set_error(GOL_EINVAL, "id needs %d bytes", GOL_RCCL_ID_BYTES);
    ncclUniqueId u;
    NCCLCHK(ncclGetUniqueId(&u));
    memcpy(id, &u, sizeof u);
    return GOL_OK;
}

extern "C" int gol_engine_create_rank(int64_t H, int64_t W, int32_t nranks, int32_t rank, const uint8_t *id,
                                      const gol_config *cfg, gol_engine **out)
{
    if (!out || nranks < 1 || rank < 0 || rank >= nranks || (!id && nranks > 1))
        return gol_set_error(GOL_EINVAL, "bad rank arguments (rank %d of %d)", rank, nranks);
    if (cfg && cfg->shards > 1) return gol_set_error(GOL_EINVAL, "one shard per rank");
    *out = nullptr;
    gol_engine *e = new gol_engine();
    int rc = engine_setup(e, H, W, cfg);
    int dev = cfg ? cfg->device : -1;
    if (dev < 0 && hipGetDevice(&dev) != hipSuccess) dev = 0;
    int transport = cfg ? cfg->transport : GOL_TRANSPORT_AUTO;
    if (transport == GOL_TRANSPORT_AUTO) transport = nranks > 1 ? GOL_TRANSPORT_RCCL : GOL_TRANSPORT_LOCAL;
    if (rc == GOL_OK && transport != GOL_TRANSPORT_RCCL && transport != GOL_TRANSPORT_IPC &&
        !(transport == GOL_TRANSPORT_LOCAL && nranks == 1))
        rc = gol_set_error(GOL_EINVAL, "ranks in several processes exchange halos over RCCL or IPC");
    if (rc == GOL_OK && transport == GOL_TRANSPORT_IPC && !id) rc = gol_set_error(GOL_EINVAL, "the IPC transport needs an id");
    e->nranks = nranks;
    e->rank = rank;
    e->rank_mode = true;
    e->transport = transport;
    if (rc == GOL_OK) rc = engine_shards(e, {dev});
    if (rc == GOL_OK && transport == GOL_TRANSPORT_RCCL) {
        ncclUniqueId u;
        if (id) memcpy(&u, id, sizeof u);
        else if (ncclGetUniqueId(&u) != ncclSuccess) rc = gol_set_error(GOL_ECOMM, "ncclGetUniqueId failed");
        ncclResult_t r = rc == GOL_OK ? ncclCommInitRank(&e->sh[0].nccl, nranks, u, rank) : ncclSuccess;
        if (r != ncclSuccess) rc = gol_set_error(GOL_ECOMM, "ncclCommInitRank(rank %d of %d): %s", rank, nranks, ncclGetErrorString(r));
        if (rc == GOL_OK) e->comm = gol_comm_rccl(e->sh[0].nccl);
    }
    if (rc == GOL_OK && transport == GOL_TRANSPORT_IPC) {
        // the ring neighbours this rank pulls its ghost rows from (gol_halo_plan's peers)
        for (int p : {(rank + nranks - 1) % nranks, (rank + 1) % nranks})
            if (p != rank && std::find(e->ipc_peers.begin(), e->ipc_peers.end(), p) == e->ipc_peers.end())
                e->ipc_peers.push_back(p);
        rc = set_dev(dev);
        // the peers pull from a small send buffer, not from the board: importing whole boards
        // (2 GiB each for config 4 over 4 ranks) hung inside the runtime's IPC import
        gol_shard &s0 = e->sh[0];
        const size_t ob = ipc_out_bytes(e);
        if (rc == GOL_OK && hipMalloc(&s0.ipc_out, ob) != hipSuccess) rc = gol_set_error(GOL_EHIP, "IPC send rows: hipMalloc failed");
        if (rc == GOL_OK && (hipMemset(s0.ipc_out, 0, ob) != hipSuccess || hipDeviceSynchronize() != hipSuccess))
            rc = gol_set_error(GOL_EHIP, "IPC send rows: hipMemset failed");
        uint32_t *const bufs[2] = {s0.ipc_out, nullptr};
        if (rc == GOL_OK) rc = gol_ipc::open(id, nranks, rank, dev, H, W, e->kx, bufs, e->ipc_peers, &e->ipc);
        e->comm = e->ipc;
    }
    if (rc != GOL_OK) {
        gol_engine_destroy(e);
        return rc;
    }
    *out = e;
    return GOL_OK;
}

extern "C" void gol_engine_destroy(gol_engine *e)
{
    if (!e) return;
    for (auto &s : e->sh) {  // (an IPC wait or signal may still read or write the flag words)
        (void)hipSetDevice(s.device);
        for (hipStream_t st : {s.stream, s.edge, s.comm})
            if (st) (void)hipStreamSynchronize(st);
    }
    delete e->comm;  // the IPC transport unmaps the peers' buffers; RCCL's comm is the shard's
    for (auto &s : e->sh) shard_release(s);
    delete e;
}

extern "C" int gol_engine_topology(gol_engine *e, int32_t *shards, int32_t *nranks, int32_t *rank, int32_t *transport)
{
    if (!e) return gol_set_error(GOL_EINVAL, "engine is NULL");
    if (shards) *shards = (int32_t)e->sh.size();
    if (nranks) *nranks = e->nranks;
    if (rank) *rank = e->rank;
    if (transport) *transport = e->transport;
    return GOL_OK;
}

extern "C" int gol_engine_shard(gol_engine *e, int32_t i, int32_t *device, int64_t *y0, int64_t *y1)
{
    if (!e || i < 0 || i >= (int32_t)e->sh.size()) return gol_set_error(GOL_EINVAL, "no local shard %d", i);
    if (device) *device = e->sh[i].device;
    if (y0) *y0 = e->sh[i].y0;
    if (y1) *y1 = e->sh[i].y1;
    return GOL_OK;
}
// ------------------------------------------------------------------ synchronisation, errors

// Wait for every shard's work and read the shards' device error words (one pinned readback
// queued behind the work, so the check costs no extra synchronisation).
// With ranks in several processes the error words are all-reduced first (max), so a fault on
// one rank -- whose rows reach the others through the halo -- fails the call on every rank; it
// also ends every rank's halo copies (the IPC transport's all-reduce is a host barrier behind
// the streams), so no rank reads a neighbour's buffers past this point.  `collective` = false:
// this process's shards only (a call that other ranks do not make).
int sync_all(gol_engine *e, bool collective)
{
    const bool coll = collective && several(e);
    for (auto &s : e->sh) {
        RCCHK(set_dev(s.device));
        RCCHK(join_last_step(s));  // (the edge launches' error word writes; the halo copies, the IPC waits' error word)
        if (coll) RCCHK(e->comm->allreduce_max_u32(s.err, 1, s.stream));
        HIPCHK(hipMemcpyAsync(s.host_word, s.err, sizeof(uint32_t), hipMemcpyDeviceToHost, s.stream));
    }
    uint32_t flags = 0;
    for (auto &s : e->sh) {
        RCCHK(set_dev(s.device));
        HIPCHK(hipStreamSynchronize(s.stream));
        HIPCHK(hipStreamSynchronize(s.edge));
        HIPCHK(hipStreamSynchronize(s.comm));
        flags |= s.host_word[0];
    }
    e->halo_issued = false;
    if (flags) {
        for (auto &s : e->sh) {
            RCCHK(set_dev(s.device));
            HIPCHK(hipMemsetAsync(s.err, 0, sizeof(uint32_t), s.stream));
            s.slots_zero = false;  // a faulted launch may have left counts in them
            s.batch_zero = false;
            // a timed-out pair may have left its claims set: this engine's streams only
            HIPCHK(golk_reset_claims(s.stream));
            HIPCHK(golk_reset_claims(s.edge));
            // a workgroup that gave up may not have freed its CU slot (role placement: speed only)
            HIPCHK(golk_reset_cu_slots(s.device, s.stream));
            HIPCHK(hipStreamSynchronize(s.stream));
            HIPCHK(hipStreamSynchronize(s.edge));
        }
        e->halo_ok = false;
        return gol_set_error(GOL_EHIP, "device fault in a step kernel (error flags 0x%x: %s); the board is not valid",
                             flags, (flags & GOLK_ERR_SPIN) ? "a pipeline wave timed out waiting for its neighbour"
                                    : (flags & GOLK_ERR_IPC) ? "an IPC rank timed out waiting for a neighbour's halo rows"
                                                             : "?");
    }
    if (e->mode == GOL_MODE_BITS)
        for (auto &s : e->sh) free_exact_bytes(s);  // the exact first turn's byte rows, once used
    return GOL_OK;
}

// Collective barrier of the ranks of a several-process engine (a one-element all-reduce).
int rank_barrier(gol_engine *e)
{
    if (!several(e)) return GOL_OK;
    gol_shard &s = e->sh[0];
    RCCHK(set_dev(s.device));
    return e->comm->barrier(s.coll, s.stream);
}

// Before a stepping call with several ranks: the ranks agree on the board state, and any rank
// whose halo is stale (its rows changed outside a step: load_words on that rank alone) makes
// every rank exchange again, so the exchanges -- collective, paired in order -- stay matched.
int agree_step_state(gol_engine *e)
{
    if (!several(e)) return GOL_OK;
    gol_shard &s = e->sh[0];
    RCCHK(set_dev(s.device));
    uint32_t *v = s.host_word + 4;  // [stale halo, mode, cur, band, ~mode, ~cur, ~band]: max of x and of ~x
    const uint32_t st[3] = {(uint32_t)e->mode, (uint32_t)e->cur, (uint32_t)e->band};
    v[0] = e->halo_ok ? 0u : 1u;
    for (int i = 0; i < 3; ++i) {
        v[1 + i] = st[i];
        v[4 + i] = ~st[i];
    }
    HIPCHK(hipMemcpyAsync(s.coll, v, 7 * sizeof(uint32_t), hipMemcpyHostToDevice, s.stream));
    RCCHK(e->comm->allreduce_max_u32(s.coll, 7, s.stream));
    HIPCHK(hipMemcpyAsync(v, s.coll, 7 * sizeof(uint32_t), hipMemcpyDeviceToHost, s.stream));
    HIPCHK(hipStreamSynchronize(s.stream));
    for (int i = 0; i < 3; ++i)
        if (v[1 + i] != ~v[4 + i])
            return gol_set_error(GOL_ESTATE, "the ranks disagree on the board state (mode / buffer / layout)");
    if (v[0]) e->halo_ok = false;
    return GOL_OK;
}

// The board is about to change outside a step (load, layout conversion, exact first turn):
// the halo of the current buffer is no longer the board's, and the exchange still in flight
// (it reads and writes the buffers) finishes before the compute stream writes them.
int invalidate_halo(gol_engine *e)
{
    if (e->halo_issued)
        for (auto &s : e->sh) {
            RCCHK(set_dev(s.device));
            HIPCHK(hipStreamWaitEvent(s.stream, s.ev_edge, 0));
            for (auto &t : e->sh) HIPCHK(hipStreamWaitEvent(s.stream, t.ev_halo, 0));  // (loopback: t reads my rows)
            // (IPC: the neighbours read only this rank's send buffer ipc_out, never its board, and
            // its own copies into ipc_out are behind ev_halo: nothing to wait for across processes)
        }
    e->halo_ok = false;
    return GOL_OK;
}

// ------------------------------------------------------------------ layout conversion
// The band layout is a stepping detail: convert on the first step, convert back before
// anything reads the bits.  Both are one HBM pass (32x32 bit transposes) per shard.
int convert(gol_engine *e, bool to_band)
{
    if (e->band == to_band || e->mode != GOL_MODE_BITS) return GOL_OK;
    RCCHK(invalidate_halo(e));
    for (auto &s : e->sh) {
        RCCHK(set_dev(s.device));
        HIPCHK(golk_band_convert(to_band, s.bits[e->cur], s.bits[1 - e->cur], s.R, e->Wd, e->pitch, e->pitch, s.stream));
    }
    e->cur = 1 - e->cur;
    e->band = to_band;
    return GOL_OK;
}
// ------------------------------------------------------------------ rules
extern "C" int gol_engine_set_rule(gol_engine *e, uint32_t birth, uint32_t survive, int32_t flags)
{
    if (!e) return gol_set_error(GOL_EINVAL, "engine is NULL");
    if (birth >= 512 || survive >= 512 || (flags & ~GOL_RULE_GENERIC))
        return gol_set_error(GOL_EINVAL, "bad rule (B 0x%x, S 0x%x, flags 0x%x): 9-bit masks, flags GOL_RULE_GENERIC", birth,
                             survive, flags);
    const bool conway = birth == 0x008 && survive == 0x00C;
    const bool generic = !conway || (flags & GOL_RULE_GENERIC);
    if (generic && !e->bit_capable)
        return gol_set_error(GOL_EINVAL, "rules other than B3/S23 (and GOL_RULE_GENERIC) need a bit board: W %% 64 == 0 (W = %lld), layout not BYTES",
                             (long long)e->W);
    // nothing else changes: the board, the turn and the halo (cells, whatever rule made them) stay
    e->birth = birth;
    e->survive = survive;
    e->rule_generic = generic;
    return GOL_OK;
}

extern "C" int gol_engine_rule(gol_engine *e, uint32_t *birth, uint32_t *survive, int32_t *generic)
{
    if (!e) return gol_set_error(GOL_EINVAL, "engine is NULL");
    if (birth) *birth = e->birth;
    if (survive) *survive = e->survive;
    if (generic) *generic = e->rule_generic ? 1 : 0;
    return GOL_OK;
}

extern "C" int gol_engine_device_bits(gol_engine *e, uint32_t **bits, int64_t *pitch)
{
    if (!e || !bits || !pitch) return gol_set_error(GOL_EINVAL, "bad arguments");
    if (e->mode != GOL_MODE_BITS) return gol_set_error(GOL_ESTATE, "board is not bit-resident");
    RCCHK(ensure_standard(e));
    RCCHK(sync_all(e, false));
    *bits = e->sh[0].bits[e->cur];
    *pitch = e->pitch;
    return GOL_OK;
}
