/*
 * golhip.h -- C ABI of libgolhip.so, the MI355X (gfx950) Game-of-Life hot path.
 *
 * The reference (ao22174/Gol-distributed-final) is Go; its hot path is reached
 * over net/rpc.  This ABI is what a cgo binding of that path would bind (the
 * stub is in INTEGRATION.md).  Every entry point names the reference
 * interface it replaces (file:line inside the reference tree).
 *
 * Conventions
 *  - Every call returns an int status: GOL_OK (0) or a negative GOL_E* code.
 *    It never aborts the process.  gol_last_error() gives a thread-local
 *    message for the last failing call on the calling thread.  (The
 *    reference panics on local failures, util/check.go:3-7, and its RPC
 *    handlers always return nil; a Go host maps nonzero codes to `error`.)
 *  - Host buffers are caller-owned and only borrowed for the duration of a
 *    call; the library never retains a host pointer.  Device memory created
 *    by an engine is engine-owned and released by gol_engine_destroy.
 *  - Boards: byte boards are row-major [y][x], one byte per cell, 255 = alive,
 *    0 = dead (README.md:25-32); `stride` is the row pitch in bytes.
 *    Bit boards are row-major, 64 cells per uint64 (LSB = lowest x), i.e. 32
 *    cells per uint32 little-endian; `pitch` is the row pitch in uint32 words.
 *  - Torus semantics: rows wrap with H, columns with W.  The reference wraps
 *    both axes with len(world[0]) (worker.go:48-59) and is only defined for
 *    square boards, where the two agree.
 *  - Thread safety: gol_next_state_slab and the gol_dev_* launchers are
 *    re-entrant.  A gol_engine handle is not internally synchronised; callers
 *    serialise access (the broker mirror does, like broker.go's `mt`).
 */
#ifndef GOLHIP_H
#define GOLHIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GOL_ABI_VERSION 6

enum {
    GOL_OK = 0,
    GOL_EINVAL = -1,   /* bad argument */
    GOL_EHIP = -2,     /* HIP runtime error, or a kernel reported a device-side fault */
    GOL_ENOMEM = -3,   /* allocation failed */
    GOL_EIO = -4,      /* file I/O */
    GOL_EFORMAT = -5,  /* malformed PGM (io.go:101-117 panics) */
    GOL_ESTATE = -6,   /* call not valid in the current state */
    GOL_EQUIT = -7,    /* broker was shut down (SuperQuit) */
    GOL_ECOMM = -8     /* RCCL (halo exchange / reduction) error */
};

/* ---------------------------------------------------------------- library */
int gol_abi_version(void);
const char *gol_last_error(void);
int gol_device_count(int *n);

/* ---------------------------------------------------------------- worker path
 * Replaces worker.go:15-42 calculateNextState + worker.go:44-70
 * calculateSurroundings, as called by GameOfLifeOperations.Update
 * (worker.go:77-80).  Exact reference semantics per byte: a cell that is
 * exactly 0 with exactly 3 neighbours equal to 255 becomes 255; a cell equal to
 * 255 with 2 or 3 such neighbours stays 255; every other cell becomes 0.
 * world: H x W bytes (row pitch `stride`); out: (y1-y0) x W bytes (pitch
 * out_stride) = next state of rows [y0, y1).  Runs on the current device. */
int gol_next_state_slab(const uint8_t *world, int64_t H, int64_t W, int64_t stride,
                        int64_t y0, int64_t y1, uint8_t *out, int64_t out_stride);

/* Replaces the row split of broker.go:135-139 (H % T == 0: StartY = i*H/T,
 * EndY = (i+1)*H/T) and broker.go:172-206 (else the first H % T slabs get
 * H/T + 1 rows, the rest H/T, in order).  Also used to row-shard a board over
 * GPUs. */
int gol_partition_rows(int64_t H, int64_t parts, int64_t i, int64_t *y0, int64_t *y1);

/* ---------------------------------------------------------------- engine
 * A board resident in HBM, on one GPU or row-sharded over several.  Replaces
 * the broker's per-turn state (`world`, `cWorld`, `cTurn`: broker.go:22-36,
 * 62-234) and the per-turn scatter/gather to workers (broker.go:143-157,
 * 182-211): the board stays in HBM and is stepped in k-turn launches.
 *
 * Row sharding (broker.go:135-206 applied to GPUs): the board's rows are split
 * with gol_partition_rows over `nranks` shards; shard r keeps rows
 * [y0_r, y1_r) plus 16 ghost rows above and below.  Every k-turn step needs in
 * its ghost rows the k rows above the shard (from shard r-1) and below it
 * (from shard r+1, mod nranks): gol_halo_plan.  A step first computes the kx
 * rows at each edge of the shard (they read the halo) and, beside them, the
 * interior; the next step's halo is exchanged as soon as the edge rows are
 * written, while the interior is still running (gol_step_plan).  One shard
 * (the whole torus) runs the same step with its own rows as the halo.
 * k <= kx <= min shard rows.
 *  - one process, `shards` local shards (gol_config.shards): GPUs device,
 *    device+1, ... (or all on `device` with GOL_SHARDS_SAME_DEVICE);
 *  - one process per GPU (gol_engine_create_rank): this process holds shard
 *    `rank` of `nranks`; whole-board queries (alive count, hash, PGM write,
 *    counted steps) are collective: every rank calls them.
 * Transports of the halo rows: RCCL ncclSend/ncclRecv on a per-shard comm
 * stream (xGMI between GPUs), LOOPBACK device copies between the shards of
 * one process (shards may share a GPU: multi-shard logic on a 1-GPU box), or
 * IPC between the rank processes of one node: each rank copies its ghost rows
 * out of its neighbours' HBM through HIP IPC mappings, ordered by sequence
 * flags in device memory, and the collectives (counts, error words, barriers)
 * run on the host through a shared-memory segment.  IPC ranks may share a GPU
 * (RCCL refuses two ranks on one GPU), so the one-process-per-GPU engine runs
 * with 2-16 processes on a 1-GPU box exactly as it runs on 8 GPUs. */
typedef struct gol_engine gol_engine;

/* Bit-board layout used while stepping.  STANDARD: word s of a row holds cells
 * 32s .. 32s+31.  BAND: word w holds, at bit b, cell b*(W/32) + w (32 column
 * bands), which makes a generation shift-free.  AUTO picks
 * BAND when W % 1024 == 0.  The layout is internal: every reader (store,
 * alive list, PGM, hash, device_bits) sees the standard layout, and converts
 * the board to it; only the viewport frames read it, and gol_engine_paste
 * writes it, as it is.  BYTES keeps
 * the board as the reference's one byte per cell (a W % 64 != 0 board always
 * does): one shard, 32 turns per launch on a 0/255 board with W % 32 == 0 (the
 * byte pipeline), the exact byte kernel otherwise; the
 * bit-board calls (load_words, store_words, device_bits, hash) are EINVAL. */
#define GOL_LAYOUT_AUTO 0
#define GOL_LAYOUT_STANDARD 1
#define GOL_LAYOUT_BAND 2
#define GOL_LAYOUT_BYTES 3
/* Halo transport between shards. */
#define GOL_TRANSPORT_AUTO 0     /* 1 shard: local torus wrap; shards on distinct GPUs: RCCL; else LOOPBACK */
#define GOL_TRANSPORT_LOOPBACK 1 /* device copies between the shards of this process */
#define GOL_TRANSPORT_RCCL 2     /* ncclSend/ncclRecv (with one shard: send to self) */
#define GOL_TRANSPORT_LOCAL 3    /* (reported only) one shard, wrap rows read from the board itself */
#define GOL_TRANSPORT_IPC 4      /* gol_engine_create_rank only: HIP IPC halo pulls + host collectives */
/* gol_config.flags */
#define GOL_SHARDS_SAME_DEVICE 1 /* every local shard on `device` (loopback testing on one GPU) */
#define GOL_STEP_SERIAL 2        /* one launch per shard and step, after the halo exchange (gol_step_plan) */
#define GOL_STEP_EDGE_FIRST 4    /* the edge rows first on the compute stream, then the interior (gol_step_plan) */
#define GOL_STEP_OVERLAP 8       /* the edge rows on the edge stream beside the interior (gol_step_plan) */
                                 /* (16: ABI 3's persistent multi-round launch, removed in ABI 4) */
typedef struct gol_config {
    int32_t device;           /* HIP device ordinal (first shard); -1 = current device */
    int32_t turns_per_launch; /* k (temporal blocking); 0 = library default */
    int32_t strip_rows;       /* rows per wave strip; 0 = automatic */
    int32_t cells_per_lane;   /* 32, 64 or 128 bits per lane; 0 = automatic */
    int32_t layout;           /* bit-board layout while stepping: GOL_LAYOUT_* */
    int32_t shards;           /* row shards in this process (0 or 1 = one GPU, no sharding) */
    int32_t transport;        /* GOL_TRANSPORT_* */
    int32_t flags;            /* GOL_SHARDS_* */
} gol_config;

int gol_engine_create(int64_t H, int64_t W, const gol_config *cfg, gol_engine **out);
/* One process per GPU: every rank calls this (collective) with the same H, W,
 * nranks and unique id, made on one rank and shared by the caller's own means
 * (e.g. torch.distributed or the Go broker's RPC): gol_rccl_unique_id for
 * cfg->transport GOL_TRANSPORT_RCCL (the default with nranks > 1),
 * gol_ipc_unique_id for GOL_TRANSPORT_IPC (at most GOL_IPC_MAX_RANKS ranks, one
 * node; the id names the ranks' shared-memory segment, which exists only while
 * they connect).  cfg->device is this rank's GPU (IPC ranks may name the same
 * one).  Needs W % 64 == 0 and H >= nranks.  With several ranks every stepping
 * call starts by agreeing on the halo state: a rank whose rows changed outside
 * a step (load_words on it alone) makes every rank exchange its halo again. */
#define GOL_RCCL_ID_BYTES 128
#define GOL_IPC_ID_BYTES 128
#define GOL_IPC_MAX_RANKS 16
int gol_rccl_unique_id(uint8_t *id, int64_t len);
int gol_ipc_unique_id(uint8_t *id, int64_t len);
int gol_engine_create_rank(int64_t H, int64_t W, int32_t nranks, int32_t rank, const uint8_t *id,
                           const gol_config *cfg, gol_engine **out);
void gol_engine_destroy(gol_engine *e);
/* Layout of the engine: local shards, global ranks, the first local shard's
 * global rank, and the halo transport in use (GOL_TRANSPORT_LOOPBACK, _RCCL or
 * _LOCAL). */
int gol_engine_topology(gol_engine *e, int32_t *shards, int32_t *nranks, int32_t *rank, int32_t *transport);
/* Local shard i: its GPU and its global rows [y0, y1). */
int gol_engine_shard(gol_engine *e, int32_t i, int32_t *device, int64_t *y0, int64_t *y1);
/* Load a byte board (operations.Run's req.World, broker.go:65) and reset the
 * turn counter to 0.  Any byte value is accepted (exact semantics above).
 * `world` is the whole H x W board (as the reference ships it to every
 * worker); every rank reads its own rows.  Only the first W bytes of a row are
 * read: with stride > W the bytes between the rows are ignored, whatever they
 * hold (they neither count as cells nor leave the exact first turn pending). */
int gol_engine_load_bytes(gol_engine *e, const uint8_t *world, int64_t stride);
/* Load images/<W>x<H>.pgm-style P5 (readPgmImage, gol/io.go:90-126: fields
 * "P5", W, H, 255, then the raster): every shard streams its own rows from
 * the file.  GOL_EFORMAT with the reference's panic text on a bad header, a
 * short raster or (the reference's strings.Fields split) whitespace bytes in
 * it. */
int gol_engine_load_pgm(gol_engine *e, const char *path);
/* Synthetic board: word(y, w) = splitmix64(seed ^ (y*W/64 + w)), Bernoulli(1/2)
 * per cell (W % 64 == 0 only; on a GOL_LAYOUT_BYTES board as 0/255 bytes).
 * Resets the turn counter. */
int gol_engine_load_random(gol_engine *e, uint64_t seed);
/* Advance exactly `turns` turns (blocking).  Replaces the turn loop body of
 * broker.go:75-226. */
int gol_engine_step(gol_engine *e, int64_t turns);
/* Advance exactly `turns` turns and record the alive count every `every`
 * turns (the AliveCellsCount events of distributor.go:39-51, computed on the
 * GPU: fused into the launch that ends at each such turn, then reduced on the
 * device and, between ranks, with one RCCL all-reduce at the end).  counts[i]
 * = alive cells after turn (start + (i+1)*every); writes turns/every counts
 * (cap >= turns/every).  One host synchronisation for the whole call. */
int gol_engine_step_counted(gol_engine *e, int64_t turns, int64_t every, uint64_t *counts, int64_t cap);
int gol_engine_turn(gol_engine *e, int64_t *turn);
/* Number of cells != 0 -- len(calculateAliveCells(...)), broker.go:273. */
int gol_engine_alive_count(gol_engine *e, uint64_t *count);
/* Copy the board out as bytes (0/255, or the loaded bytes before turn 1).
 * Needs every row local (not with nranks > 1 ranks: use store_rows). */
int gol_engine_store_bytes(gol_engine *e, uint8_t *out, int64_t stride);
/* Rows [y0, y1) of the board (global row numbers, all held by this process):
 * row y goes to out + (y - y0)*stride, W bytes of it; with stride > W the bytes
 * between the rows are not touched, and y0 == y1 writes nothing. */
int gol_engine_store_rows(gol_engine *e, int64_t y0, int64_t y1, uint8_t *out, int64_t stride);
/* calculateAliveCells (broker.go:47-58): (x, y) int32 pairs in row-major
 * order; writes min(n, cap) pairs, *n = total alive cells whatever cap is (the
 * pairs past min(n, cap) of xy are not touched; cap == 0 allows xy == NULL and
 * returns the total alone; with several local shards the cap runs across them:
 * the pairs are the row-major prefix of the whole list).  With ranks in
 * several processes: the cells of this rank's rows. */
int gol_engine_alive_cells(gol_engine *e, int32_t *xy, int64_t cap, int64_t *n);
/* Advance exactly one turn and list the cells whose state changed, (x, y) int32
 * pairs in row-major order: the CellFlipped{CompletedTurns, Cell} events of
 * that turn (gol/event.go:50-60; sent per flipped cell by the controller the
 * reference never finished, README.md:260-262).  Writes min(n, cap) pairs,
 * *n = number of flipped cells (of this rank's rows with several processes);
 * cap and xy as for gol_engine_alive_cells, and the turn is taken whatever cap is. */
int gol_engine_step_flips(gol_engine *e, int32_t *xy, int64_t cap, int64_t *n);
/* writePgmImage byte stream (gol/io.go:52-81): "P5\n<W> <H>\n255\n" + H*W
 * bytes, streamed from the device in chunks; with several processes every
 * rank writes its own rows at their offset (collective). */
int gol_engine_write_pgm(gol_engine *e, const char *path);
/* The same byte stream handed to a caller's sink instead of a file (a pipe,
 * a socket, a hash, a compressor: config 5's 2^20 x 2^20 board is 1 TiB as
 * P5).  The sink gets (user, file offset, bytes, length) for the header and
 * then every chunk of rows (at most 64 MiB each) of the shards of this process
 * in row order, and returns 0 (nonzero aborts the write with GOL_EIO).  With
 * ranks in several processes every rank calls it (collective) and its sink
 * sees its own rows at their offsets; rank 0's also gets the header. */
typedef int (*gol_write_fn)(void *user, int64_t offset, const uint8_t *data, int64_t len);
int gol_engine_write_pgm_to(gol_engine *e, gol_write_fn sink, void *user);
/* Bit-packed rows [y0, y1) (global, held by this process) in or out: 64 cells
 * per uint64 (LSB = lowest x), `stride` uint64 words per row, W % 64 == 0.
 * load_words overwrites those rows of the current board (several calls may
 * load a board piece by piece), resets the turn counter to 0.  On a board
 * loaded with bytes other than 0/255, its exact first turn pending, load_words
 * ends that state: the rows it does not load keep their cells equal to 255,
 * every other byte is dead, and the board is a bit board at turn 0.  store_words
 * reads them (GOL_ESTATE before turn 1 of a board loaded with bytes other than
 * 0/255: use store_bytes).  One eighth of the PCIe traffic of the byte calls.
 * Only W/64 words of a row are read or written: with stride > W/64 the words
 * between the rows are ignored by load_words and not touched by store_words. */
int gol_engine_load_words(gol_engine *e, int64_t y0, int64_t y1, const uint64_t *words, int64_t stride);
int gol_engine_store_words(gol_engine *e, int64_t y0, int64_t y1, uint64_t *words, int64_t stride);
/* Order-independent board hash (same definition as oracle_hash_words):
 * sum over 64-bit words of splitmix64(word ^ splitmix64(y*W/64 + w)).
 * W % 64 == 0 only. */
int gol_engine_hash(gol_engine *e, uint64_t *hash);
/* Chosen kernel parameters (k, cells per lane, strip rows, resident mode: 0 =
 * byte board, 1 = standard bit board, 2 = band bit board). */
int gol_engine_info(gol_engine *e, int32_t *k, int32_t *cells_per_lane, int32_t *strip_rows,
                    int32_t *bit_mode);
/* Raw device pointer to the current bit board of local shard 0 (pitch in
 * uint32 words), for tests. */
int gol_engine_device_bits(gol_engine *e, uint32_t **bits, int64_t *pitch);
/* Step timing: with timing on, HIP events on each shard's compute stream
 * bracket every k-turn step of the shard: from before its first launch to the
 * end of its last one, the edge launches included (gol_step_plan).
 * gol_engine_timing returns the number of timed shard-steps since timing was
 * (re)enabled, their mean duration and their mean cell-updates (R x W x k). */
int gol_engine_set_timing(gol_engine *e, int32_t enable);
int gol_engine_timing(gol_engine *e, int64_t *launches, double *mean_ms, double *mean_cell_updates);
/* enable = GOL_TIMING_EXCHANGE (ABI 5): also one event pair around every halo
 * exchange of a timed stepping call, on the stream the exchange runs on (the
 * RCCL send/recv group, or the IPC transport's copies and flag waits, from the
 * moment its sent rows are written); gol_engine_exchange_timing returns how many
 * were timed since timing was (re)enabled and their mean duration.  Local (this
 * process's shards); an engine whose one shard is the whole torus exchanges
 * nothing (0). */
#define GOL_TIMING_EXCHANGE 2
int gol_engine_exchange_timing(gol_engine *e, int64_t *exchanges, double *mean_ms);
/* ABI 6: the same exchanges split in two.  mean_wait_ms is the part spent
 * waiting for the ring neighbours to reach the exchange: the IPC transport's
 * poll of their READY flags; on RCCL a one-word send/recv with each neighbour
 * issued first (only while exchanges are timed), whose completion means every
 * neighbour has posted its side.  mean_transfer_ms is the rest (the halo rows
 * themselves once both sides are there).  Transports without peers in other
 * processes (LOCAL, LOOPBACK) wait for nothing on the exchange's stream: 0. */
int gol_engine_exchange_split(gol_engine *e, int64_t *exchanges, double *mean_wait_ms, double *mean_transfer_ms);

/* ---------------------------------------------------------------- viewport frames
 * (Added after ABI 6 without a version bump: GOL_ABI_VERSION stays 6, and a
 * host that may meet an older library probes for gol_engine_view,
 * gol_engine_view_counts, gol_view_plan and gol_broker_view by symbol.)
 *
 * A density-downsampled picture of a torus rectangle of the running board, for
 * boards far larger than a screen (the reference's SDL view, sdl/, draws its
 * 16^2-512^2 boards cell by cell).  A view is (x0, y0, scale, out_w, out_h):
 * pixel (i, j) covers the scale x scale box of cells
 *   x = (x0 + i*scale + dx) mod W,  y = (y0 + j*scale + dy) mod H,  0 <= dx, dy < scale
 * and n(i, j) is the number of alive cells in it (set bits; bytes != 0 on a byte
 * board and before the exact first turn: what gol_engine_alive_count counts, so
 * a view that tiles the whole board sums to it).
 *  - gol_engine_view_counts: counts[j*stride + i] = n(i, j), uint32.
 *  - gol_engine_view: pixels[j*stride + i] = (255*n + scale^2 - 1) / scale^2
 *    (integer division: ceil(255 n / scale^2)); at scale 1 the 0/255 bytes of
 *    the PGM, at any scale non-zero for a box with one alive cell and 255 for a
 *    full one.
 * Valid: 1 <= scale <= 4096, out_w, out_h >= 1, out_w*scale <= W,
 * out_h*scale <= H, 0 <= x0 < W, 0 <= y0 < H, out_w*out_h <= 2^26, stride >=
 * out_w (in elements); anything else is GOL_EINVAL before any GPU work.
 * The frame is computed on the GPU from the board in place, in whatever layout
 * it is currently stepped in (no conversion to the standard layout, unlike the
 * other readers; the next step pays nothing for the view), reading only the rows
 * and words the viewport covers: the work follows the viewport, not the board.
 * *src_layout (may be NULL) reports what was read: 0 byte rows, 1 standard bit
 * rows, 2 band bit rows (gol_engine_info's bit_mode values, for the board's
 * current state).  Blocking; ordered after the last step.  Several local shards
 * each count their rows on their own GPU (gol_view_plan) and the frames are
 * added.  view_counts is not collective: with ranks in several processes it
 * returns the counts of the cells in this process's rows, and the caller adds
 * the ranks' frames (as with gol_engine_alive_cells); view needs every row
 * local (like gol_engine_store_bytes), else GOL_EINVAL. */
int gol_engine_view_counts(gol_engine *e, int64_t x0, int64_t y0, int32_t scale, int32_t out_w, int32_t out_h,
                           uint32_t *counts, int64_t stride, int32_t *src_layout);
int gol_engine_view(gol_engine *e, int64_t x0, int64_t y0, int32_t scale, int32_t out_w, int32_t out_h,
                    uint8_t *pixels, int64_t stride, int32_t *src_layout);

/* ---------------------------------------------------------------- life-like rules
 * (Added after ABI 6 without a version bump, like the viewport calls:
 * GOL_ABI_VERSION stays 6; probe for gol_engine_set_rule, gol_engine_rule,
 * gol_rule_parse, gol_rule_format, gol_rule_eval_host and gol_dev_rule_step by
 * symbol.)
 *
 * A rule is two 9-bit masks over the number n of alive cells among a cell's 8
 * neighbours: birth bit n (0 <= n <= 8) = a dead cell with exactly n alive
 * neighbours becomes alive, survive bit n = an alive cell with exactly n stays
 * alive; every other cell is dead next turn.  B3/S23 (the default, the
 * reference's rule) is birth 0x008, survive 0x00C.  Bit 0 of birth (B0 rules)
 * is legal: the board is a finite torus.
 *
 * gol_rule_parse / gol_rule_format / gol_rule_eval_host are host functions (no
 * GPU needed).
 *  - parse: "B<digits>/S<digits>", case-insensitive, digits 0-8 in any order,
 *    either list may be empty ("B2/S").  GOL_EINVAL for a digit 9, a repeated
 *    digit, a missing half or trailing text.
 *  - format: the canonical text (upper case, ascending digits) into buf[len]
 *    (at most 22 bytes with the NUL); GOL_EINVAL for masks >= 512 or a buffer
 *    too small.
 *  - eval_host: the circuit of the rule kernels (csrc/gol_rule.h: the bit-sliced
 *    3x3 count and a mux tree over the masks) applied to 32 independent cells;
 *    bit i of nb[j] is neighbour j of cell i, bit i of centre the cell itself. */
int gol_rule_parse(const char *text, uint32_t *birth, uint32_t *survive);
int gol_rule_format(uint32_t birth, uint32_t survive, char *buf, int64_t len);
int gol_rule_eval_host(uint32_t birth, uint32_t survive, const uint32_t nb[8], uint32_t centre, uint32_t *next);
/* gol_engine_set_rule: the rule of every later turn.  Valid between stepping
 * calls at any turn; the board, the turn counter and the halo stay as they are.
 * A rule other than B3/S23 -- or B3/S23 with GOL_RULE_GENERIC, for tests and A/B
 * measurement -- is stepped by the rule kernels (masks as data, at most 8 turns
 * per launch, 64 cells per lane, standard and band layout); B3/S23 with flags 0
 * restores the B3/S23 kernels exactly.  GOL_EINVAL for masks >= 512, unknown
 * flags, or the rule kernels on a board that is not a bit board (W % 64 != 0
 * or GOL_LAYOUT_BYTES).  The reference's byte semantics (exactly 0 / exactly
 * 255) are defined for B3/S23 only: while another rule is set and the board
 * holds loaded bytes other than 0/255 (its exact first turn pending), stepping
 * calls return GOL_ESTATE and change nothing.  With several ranks every rank
 * must set the same rule before the next collective stepping call (the
 * caller's duty, like H and W).
 * gol_engine_rule: the current masks; *generic != 0 while the rule kernels are
 * in use (any pointer may be NULL). */
#define GOL_RULE_GENERIC 1
int gol_engine_set_rule(gol_engine *e, uint32_t birth, uint32_t survive, int32_t flags);
int gol_engine_rule(gol_engine *e, uint32_t *birth, uint32_t *survive, int32_t *generic);

/* ---------------------------------------------------------------- board edits
 * (Added after ABI 6 without a version bump, like the viewport and rule calls:
 * GOL_ABI_VERSION stays 6; probe for gol_engine_paste, gol_paste_host,
 * gol_rle_parse, gol_rle_format and gol_broker_paste by symbol.)
 *
 * gol_engine_paste: a w x h rectangle of cells written into the running board
 * where it is and as it is (the write-side twin of the viewport frames; the
 * load calls replace whole rows or the whole board and restart the turn count).
 * Pattern cell (c, r), 0 <= c < w, 0 <= r < h, is bit c % 64 of
 * pattern[r*stride + c/64] (the bit order of load_words; bits at c >= w of a
 * row's last word are ignored) and lands on board cell ((x0 + c) mod W,
 * (y0 + r) mod H) under `op`.  pattern == NULL: every p = 1 and stride is
 * ignored (COPY sets the rectangle, ANDNOT clears it, XOR inverts it).
 * Valid: 1 <= w <= W, 1 <= h <= H, 0 <= x0 < W, 0 <= y0 < H, w*h <= 2^26,
 * stride >= ceil(w/64), op 0..3; anything else is GOL_EINVAL before any GPU work.
 * The board is written on the GPU in the layout it is currently stepped in
 * (*dst_layout, may be NULL: 0 byte rows, 1 standard bit rows, 2 band bit rows,
 * as the views' src_layout): no conversion, and the buffer, the layout and the
 * turn counter stay as they are.  Only the words (bytes) and rows the rectangle
 * covers are touched.  *changed (may be NULL) = the cells of this process's
 * rows whose state changed.  Blocking; ordered after the last step and before
 * the next one, whose halo exchange is made again.
 *  - byte boards: a cell is alive if its byte is non-zero; written cells become
 *    0 or 255, and under OR, XOR and ANDNOT only cells whose pattern bit is set
 *    are written (other bytes, whatever their value, stay);
 *  - a bit-capable board loaded with bytes other than 0/255, its exact first
 *    turn pending: GOL_ESTATE, nothing changes;
 *  - several local shards each apply their own rows (gol_view_plan) on their own
 *    GPU; with ranks in several processes the call is not collective (like
 *    view_counts): each process applies the rows it holds, a rank that holds
 *    none may skip the call, and the next collective stepping call makes every
 *    rank exchange its halo again. */
#define GOL_PASTE_COPY   0  /* cell  = p  (the whole rectangle is overwritten) */
#define GOL_PASTE_OR     1  /* cell |= p */
#define GOL_PASTE_XOR    2  /* cell ^= p */
#define GOL_PASTE_ANDNOT 3  /* cell &= ~p */
int gol_engine_paste(gol_engine *e, int64_t x0, int64_t y0, int64_t w, int64_t h,
                     const uint64_t *pattern, int64_t stride, int32_t op,
                     int64_t *changed, int32_t *dst_layout);
/* The per-word function of the paste kernels (csrc/gol_edit.h) applied to a
 * host buffer (a host function, no GPU needed): pattern rows [prow, prow + rows)
 * go to rows [row, row + rows) of `board`, a buffer of W-cell rows in `layout`
 * (0 bytes, 1 standard, 2 band: W % 32 == 0 / W % 1024 == 0 for the bit
 * layouts), row pitch `pitch` in uint32 words (bytes for layout 0); x0, w,
 * pattern, stride, op and *changed (may be NULL) as above. */
int gol_paste_host(int32_t layout, void *board, int64_t pitch, int64_t W,
                   int64_t row, int64_t rows, int64_t prow, int64_t x0, int64_t w,
                   const uint64_t *pattern, int64_t stride, int32_t op, int64_t *changed);
/* RLE, the text form Life patterns are exchanged in ("x = 3, y = 3, rule =
 * B3/S23\nbob$2bo$3o!"); host functions.
 * gol_rle_parse reads text[0, len): lines that start with '#' are skipped; the
 * header is "x = m, y = n[, rule = text]" (free blanks, either case); the body
 * is [count]b (dead), [count]o (alive), [count]$ (end of row) and '!', with
 * blanks and newlines between tokens; text after '!' is ignored.  *w = m, *h =
 * n; with pattern != NULL the cells go to pattern[r*stride + c/64] bit c % 64
 * (rows shorter than x are dead to the right); pattern == NULL returns the
 * size only (the two-call form).  `rule` (may be NULL) receives the header's
 * rule text verbatim, "" if there is none; it is not interpreted.
 * GOL_EFORMAT, with a message naming the offset: no header, x or y < 1, x*y >
 * 2^26, any other body character (multi-state RLE is refused), a count of 0
 * or one that overflows, a run past x, rows past y (a '$' may close row y - 1),
 * a missing '!'.  GOL_EINVAL: stride < ceil(m/64), cap_rows < n, a rule buffer
 * too small.
 * gol_rle_format writes the header (with the rule when rule != NULL), rows
 * without their trailing dead cells, empty rows merged into n$, lines of at
 * most 70 characters, and "!\n".  *need (may be NULL) = bytes with the NUL;
 * buf == NULL returns it alone, a buffer too small is GOL_EINVAL with *need
 * set. */
int gol_rle_parse(const char *text, int64_t len, int64_t *w, int64_t *h,
                  uint64_t *pattern, int64_t stride, int64_t cap_rows,
                  char *rule, int64_t rule_len);
int gol_rle_format(const uint64_t *pattern, int64_t stride, int64_t w, int64_t h,
                   const char *rule, char *buf, int64_t len, int64_t *need);

/* ---------------------------------------------------------------- region reads
 * (Added after ABI 6 without a version bump, like the viewport, rule and edit
 * calls: GOL_ABI_VERSION stays 6; probe for gol_engine_copy, gol_engine_bounds,
 * gol_copy_host, gol_bounds_host, gol_broker_copy and gol_broker_bounds by
 * symbol.)
 *
 * gol_engine_copy: the exact cells of a w x h rectangle of the running board as
 * bit-packed rows, read where the board is and as it is (the read-side twin of
 * gol_engine_paste at cell precision; store_words / store_rows return whole rows
 * in the standard layout, the views one byte per pixel).  Bit c % 64 of
 * pattern[r*stride + c/64] is board cell ((x0 + c) mod W, (y0 + r) mod H), 0 <= c
 * < w, 0 <= r < h: the pattern gol_engine_paste takes, so a copy followed by a
 * paste under GOL_PASTE_COPY at the same place is the identity.  Words
 * [0, ceil(w/64)) of every row are written whole, the bits at c >= w zero; the
 * words from ceil(w/64) to stride are not touched.  A cell is alive if its bit
 * is set, on byte rows if its byte is non-zero (what the views count; this holds
 * for a bit-capable board whose exact first turn is pending, too).  *alive (may
 * be NULL) = the alive cells copied; *src_layout (may be NULL) as the views'.
 * Valid: 1 <= w <= W, 1 <= h <= H, 0 <= x0 < W, 0 <= y0 < H, w*h <= 2^26,
 * stride >= ceil(w/64), pattern != NULL, flags 0 or GOL_COPY_CUT; anything else
 * is GOL_EINVAL before any GPU work.
 * The rectangle is gathered on the GPU from the layout the board is currently
 * stepped in, reading only the rows and words it covers.  Blocking; ordered
 * after the last step.  A plain copy changes nothing: the buffer, the layout,
 * the turn counter and the halo stay, and the next step pays nothing for it.
 *  - GOL_COPY_CUT: the rectangle is cleared after it is read -- exactly
 *    gol_engine_paste(e, x0, y0, w, h, NULL, 0, GOL_PASTE_ANDNOT, ..), queued
 *    behind the read, with one host synchronisation for the call.  It makes the
 *    halo stale as a paste does, and *alive is that paste's `changed`.  On a
 *    bit-capable board loaded with bytes other than 0/255, its exact first turn
 *    pending, a cut is GOL_ESTATE and changes nothing (a plain copy is allowed);
 *  - several local shards each read their own rows (gol_view_plan) on their own
 *    GPU; with ranks in several processes the call is not collective (like
 *    view_counts and paste): the pattern rows this process does not hold are
 *    written as zero, *alive counts its rows only, and the caller ORs the
 *    ranks' patterns.
 *
 * gol_engine_bounds: the smallest box that holds every alive cell of the
 * rectangle, in the rectangle's own coordinates: those cells are the rectangle
 * cells (c, r) with bx <= c < bx + bw, by <= r < by + bh.  (A minimal box on a
 * torus is ambiguous; relative to a rectangle the caller names it is not.  (0, 0,
 * W, H) gives plain board coordinates.)  No alive cell: bx = by = bw = bh = 0.
 * *alive = the alive cells of the rectangle; for the whole board,
 * gol_engine_alive_count.  Valid as for the copy, without the w*h limit and
 * without a pattern: the whole board is legal.  Reads only: the halo stays, and
 * the call is allowed while the exact first turn is pending.  Several local
 * shards are unioned; with ranks in several processes the box is that of this
 * process's rows, still in rectangle coordinates, and the caller unions.  Every
 * output pointer may be NULL. */
#define GOL_COPY_CUT 1
int gol_engine_copy(gol_engine *e, int64_t x0, int64_t y0, int64_t w, int64_t h,
                    uint64_t *pattern, int64_t stride, int32_t flags,
                    int64_t *alive, int32_t *src_layout);
int gol_engine_bounds(gol_engine *e, int64_t x0, int64_t y0, int64_t w, int64_t h,
                      int64_t *bx, int64_t *by, int64_t *bw, int64_t *bh,
                      int64_t *alive, int32_t *src_layout);
/* The per-unit mapping of the region-read kernels (csrc/gol_copy.h) applied to a
 * host buffer (host functions, no GPU needed); layout, board, pitch, W, row,
 * rows, prow, x0, w, pattern and stride as for gol_paste_host, with board rows
 * [row, row + rows) read into pattern rows [prow, prow + rows).
 * gol_bounds_host returns the inclusive minima and maxima of the alive cells'
 * columns and rows relative to x0 and `row` (any pointer may be NULL); rows
 * without an alive cell give *cmin > *cmax and *rmin > *rmax. */
int gol_copy_host(int32_t layout, const void *board, int64_t pitch, int64_t W,
                  int64_t row, int64_t rows, int64_t prow, int64_t x0, int64_t w,
                  uint64_t *pattern, int64_t stride, int64_t *alive);
int gol_bounds_host(int32_t layout, const void *board, int64_t pitch, int64_t W,
                    int64_t row, int64_t rows, int64_t x0, int64_t w,
                    int64_t *cmin, int64_t *cmax, int64_t *rmin, int64_t *rmax, int64_t *alive);

/* ---------------------------------------------------------------- batches of small boards
 * (Added after ABI 6 without a version bump, like the viewport, rule, edit and
 * copy calls: GOL_ABI_VERSION stays 6; probe for the gol_batch_* calls by
 * symbol.)
 *
 * A batch is n independent tori, all H x W, 1 <= H <= 512, 1 <= W <= 512 (any
 * width), 1 <= n <= 2^20, on one GPU, with one turn counter and one rule
 * (default B3/S23) or a rule per board.  The engine steps one board per launch, and a launch on a board
 * of this size is latency-bound; a batch steps all its boards
 * in one launch, each resident in one workgroup for all the launch's turns
 * (DESIGN.md §4.15).
 * Board i is bit-packed in the bit order of load_words: bit c % 64 of word c / 64
 * of a row is cell c, Ww = ceil(W / 64) uint64 words per row, H rows.  The bits
 * at c >= W of a row's last word are zero in device memory and in everything
 * returned.  Strides are in uint64 words: row y of board i of a caller's buffer
 * is at words + (i - i0)*board_stride + y*row_stride.
 *  - create: `device` as gol_config.device; turns_per_launch 0 = automatic (a
 *    launch is bounded to a fixed number of cell-updates), else the most turns
 *    one launch makes.  The boards start empty at turn 0.
 *  - info: n, H, W, the waves per board, the boards per workgroup, the 32-bit
 *    words of a row per lane and the turns-per-launch bound in use (any pointer
 *    may be NULL).
 *  - set_rule / rule: the 9-bit masks of "life-like rules"; masks >= 512 are
 *    GOL_EINVAL.  Valid between stepping calls: the boards and the turn stay.  B0
 *    rules are legal, and the padding bits still stay zero.  set_rule sets
 *    every board; rule returns the rule that all boards share (also after
 *    set_rules made them equal), and on a batch of different rules GOL_ESTATE,
 *    its outputs untouched.
 *  - set_rules: the masks of boards [i0, i1) from birth[i - i0] and survive[i -
 *    i0]; the other boards keep their rules, the boards and the turn stay.
 *    Every mask is checked first: a call that fails (NULL, i0 < 0, i0 > i1, i1 >
 *    n, a mask >= 512) sets none.  rules returns the masks of boards [i0, i1).
 *    A batch whose boards share one rule runs the one-rule kernels, whichever
 *    call made it so; only boards of different rules run the kernel that reads
 *    a rule per board (there B3/S23 boards take the table circuit, too).
 *  - load_words overwrites boards [i0, i1) only (set bits at c >= W of the
 *    input are ignored) and resets the turn counter to 0; store_words writes Ww
 *    words per row and touches neither the words between rows nor those between
 *    boards.
 *  - load_random: word(i, y, w) = splitmix64(seed ^ ((i*H + y)*Ww + w)) masked to
 *    W, i.e. oracle_random_words(seed, 0, n*H, Ww) with the padding cleared;
 *    generated on the GPU; resets the turn counter.
 *  - step: every board advances exactly `turns` >= 0 turns (blocking).  settled
 *    may be NULL; else int64_t[n]: settled[i] = the smallest turn t with turn0 +
 *    2 <= t <= turn0 + turns (turn0: the turn before the call) at which board i
 *    equals its own state two turns earlier, else -1: still lifes and period-2
 *    oscillators.  The scan is per call (a board that settled in an earlier call
 *    is found again at turn0 + 2), and every board is at turn0 + turns after
 *    the call, whatever it settled at.
 *  - step_cycles: every board advances exactly `turns` >= 0 turns, as in step,
 *    and is scanned for a cycle of any period (Brent's cycle detection).  With
 *    t0 the turn before the call and s(t) a board's state at turn t, the marks
 *    are m_j = t0 + 2^j - 1 (t0, t0 + 1, t0 + 3, t0 + 7, ...), and for t = t0 + 1 ..
 *    t0 + turns, m(t) is the largest mark < t.  The board is found at the
 *    smallest t with s(t) == s(m(t)): found[i] = t and period[i] = t - m(t); a
 *    board never found has -1 in both.  (At a turn that is itself a mark the
 *    comparison is with the mark before it.)  It follows that period is the
 *    exact minimal period of the board's cycle (a snapshot inside the cycle
 *    recurs first after exactly one period), and that a board entering its
 *    cycle mu turns after t0 with period lambda is found no later than t0 +
 *    3*max(mu + 1, lambda).  found is therefore an upper bound of the settle
 *    turn, not the settle turn: step(..., settled) stays the exact scan for
 *    periods <= 2.  found and period are int64_t[n]; found must not be NULL,
 *    period may be.  The scan is per call (a second call starts again from its
 *    own t0), there is no early exit here (run_cycles has it), turns == 0
 *    leaves every board at -1, and rules per board apply.
 *  - run_cycles: step_cycles with the boards retired as they are found.  After
 *    the call the boards, found, period, the turn counter and the rules are
 *    exactly what step_cycles(b, turns, found, period) leaves, for every board,
 *    one rule or a rule per board, every turns >= 0 and every
 *    turns_per_launch; only the work differs.  A board found at f with period p
 *    has s(t + p) == s(t) for every t >= f - p, so its state at the call's end
 *    t_end is its state at any turn t_L >= f advanced by (t_end - t_L) mod p
 *    turns.  The search runs in launches over a list of the boards not yet
 *    found; after each launch a retire pass on the GPU takes the boards just
 *    found off that list and gives each its remainder, which later launches
 *    make (boards of one workgroup make different numbers of turns).  made is
 *    optional (int64_t[n], may be NULL; period may be NULL as in step_cycles):
 *    the turns each board actually computed.  With t0 the turn before the call
 *    and a batch created with turns_per_launch = L > 0, the search runs in
 *    launches of L turns, the last one shorter; a board found at f leaves after
 *    the first launch that ends at t_L >= f, t_L = t0 + min(turns, L *
 *    ceil((f - t0) / L)), and made = (t_L - t0) + ((t0 + turns - t_L) mod
 *    period); a board never found has made = turns.  With the automatic length
 *    (turns_per_launch 0) each launch's bound is recomputed from the boards
 *    still in it (2^35 cell-updates / (active * H * W), clamped to 1..4096), and
 *    made is only known to be <= turns, and >= found - t0 where found.  The
 *    search ends when no board is left in it or turns are made.  The host
 *    reads the two list counts back after every launch, to size the next grid
 *    and to stop: one small blocking read per launch, where step_cycles blocks
 *    once per call.  On a batch in which nothing is ever found the lists, the
 *    pass and the reads are pure overhead (DESIGN.md 4.17 has the measured
 *    points): a caller who knows that most boards outlive the horizon should
 *    prefer step_cycles.  Refusals as step_cycles (NULL handle, NULL found,
 *    turns < 0), the batch and the outputs untouched; turns == 0 gives found
 *    -1, period -1, made 0.
 *  - load_soups: board i becomes soup first + i (below); load_random(seed) is
 *    this call with first = 0 and keeps its own code path.  Resets the turn
 *    counter.  GOL_EINVAL: first < 0 or first + n > 2^40.
 *  - search: soups.  Soup g of (seed, H, W) is the board whose word (y, w) is
 *    splitmix64(seed ^ ((g*H + y)*Ww + w)), masked to W: board g of
 *    load_random(seed) on a batch large enough to hold it.  For soup g let s(0)
 *    be the soup; the scan is step_cycles' own, with t0 = 0, over `horizon`
 *    turns, under the batch's one rule.  The results are found[g] and period[g]
 *    exactly as step_cycles defines them, alive[g] = the cells alive in
 *    s(found), and hash[g] = oracle_hash_words of s(found), the definition
 *    hashes uses.  A soup not found within `horizon` has -1, -1, 0, 0; it can be
 *    re-made from its index (load_soups, gol_batch_soup_host).  The results do
 *    not depend on the number of slots, on turns_per_launch, or on which slot
 *    a soup ran in.
 *    gol_batch_search runs soups [first, first + total) through the batch's n
 *    boards as slots, min(n, total) of them: a slot whose soup is found, or
 *    has outlived the horizon, hands its result to a table indexed by soup
 *    number and takes the next soup of the supply at the same launch boundary,
 *    so the GPU stays full until the supply runs out.  The output arrays have
 *    `total` entries, indexed g - first; period, alive and hash may each be
 *    NULL.  Every launch makes L turns: L = turns_per_launch, or with the
 *    automatic length the create bound computed for min(n, total) boards, in
 *    both cases at most `horizon`.  A soup's age at a launch boundary is a
 *    multiple of L; a soup found in a launch that ran past the horizon, at an
 *    age above it, is not a find.  stats may be NULL; it receives the launches,
 *    the slots used, L, the board-turns computed (summed over the launches as
 *    boards in the launch x L) and the board-turns a full grid would have made
 *    (launches x slots x L).  The call blocks (the host reads four counts back
 *    after every launch).  Afterwards every board is empty, the turn counter is
 *    0 and the rule stays.  Refused before any GPU work, the batch and the
 *    outputs untouched: GOL_EINVAL for a NULL handle or found, first, total or
 *    horizon < 0, first + total > 2^40, total > 2^26; GOL_ESTATE for a batch
 *    with differing rules per board (a rule per soup is not built).  total == 0
 *    and horizon == 0 are legal; with horizon == 0 every soup is at -1.
 *  - alive_counts / hashes: one uint64 per board, cap >= n; the hash of board i
 *    is oracle_hash_words(words_i, 0, H, Ww) (gol_engine_hash's definition on
 *    the board's zero-padded words, for every W).
 * GOL_EINVAL before any GPU work: n, H or W out of range, i0 > i1 or i1 > n, a
 * row stride < Ww (a board stride < (H - 1)*row_stride + Ww), a cap < n, turns
 * < 0, a NULL handle or buffer.  A call that fails leaves the batch and its
 * turn as they were.  A handle is not internally synchronised. */
typedef struct gol_batch gol_batch;
int gol_batch_create(int64_t n, int64_t H, int64_t W, int32_t device, int32_t turns_per_launch, gol_batch **out);
void gol_batch_destroy(gol_batch *b);
int gol_batch_info(gol_batch *b, int64_t *n, int64_t *H, int64_t *W, int32_t *waves_per_board,
                   int32_t *boards_per_workgroup, int32_t *words_per_lane, int32_t *turns_per_launch);
int gol_batch_set_rule(gol_batch *b, uint32_t birth, uint32_t survive);
int gol_batch_rule(gol_batch *b, uint32_t *birth, uint32_t *survive);
int gol_batch_set_rules(gol_batch *b, int64_t i0, int64_t i1, const uint32_t *birth, const uint32_t *survive);
int gol_batch_rules(gol_batch *b, int64_t i0, int64_t i1, uint32_t *birth, uint32_t *survive);
int gol_batch_load_words(gol_batch *b, int64_t i0, int64_t i1, const uint64_t *words, int64_t row_stride,
                         int64_t board_stride);
int gol_batch_store_words(gol_batch *b, int64_t i0, int64_t i1, uint64_t *words, int64_t row_stride,
                          int64_t board_stride);
int gol_batch_load_random(gol_batch *b, uint64_t seed);
int gol_batch_load_soups(gol_batch *b, uint64_t seed, int64_t first);
typedef struct gol_batch_search_stats {
    int64_t launches;     /* step launches of the call */
    int64_t slots;        /* min(n, total) */
    int64_t launch_turns; /* L, the turns of every launch */
    int64_t board_turns;  /* sum over the launches of (boards in the launch) * L */
    int64_t full_turns;   /* launches * slots * L: what a full grid would have made */
} gol_batch_search_stats;
int gol_batch_search(gol_batch *b, uint64_t seed, int64_t first, int64_t total, int64_t horizon, int64_t *found,
                     int64_t *period, uint64_t *alive, uint64_t *hash, gol_batch_search_stats *stats);
int gol_batch_step(gol_batch *b, int64_t turns, int64_t *settled);
int gol_batch_step_cycles(gol_batch *b, int64_t turns, int64_t *found, int64_t *period);
int gol_batch_run_cycles(gol_batch *b, int64_t turns, int64_t *found, int64_t *period, int64_t *made);
int gol_batch_turn(gol_batch *b, int64_t *turn);
int gol_batch_alive_counts(gol_batch *b, uint64_t *counts, int64_t cap);
int gol_batch_hashes(gol_batch *b, uint64_t *hashes, int64_t cap);
/* One turn of one H x W torus on host memory (a host function, no GPU needed)
 * with the row function the batch kernel runs (csrc/gol_batch.h): `in` and `out`
 * are H rows of row_stride uint64 words each (they may be the same buffer).  Set
 * bits at c >= W of `in` are ignored; Ww words of every row of `out` are written,
 * their padding zero, and the words between the rows are not touched.
 * GOL_EINVAL: H or W outside 1..512, masks >= 512, row_stride < Ww, NULL. */
int gol_batch_step_host(int64_t H, int64_t W, uint32_t birth, uint32_t survive, const uint64_t *in, uint64_t *out,
                        int64_t row_stride);
/* The cycle scan of gol_batch_step_cycles on one board in host memory (a host
 * function, no GPU needed), with the turn of gol_batch_step_host and the mark
 * arithmetic the kernel runs (csrc/gol_batch.h), t0 = 0: `out` receives s(turns)
 * (for turns == 0 `in` with its padding cleared), *found and *period as above
 * (found in 1..turns or -1).  `in` and `out` as for gol_batch_step_host (they
 * may be the same buffer); period may be NULL.  GOL_EINVAL as there, and for
 * turns < 0 or a NULL found. */
int gol_batch_cycles_host(int64_t H, int64_t W, uint32_t birth, uint32_t survive, const uint64_t *in, uint64_t *out,
                          int64_t row_stride, int64_t turns, int64_t *found, int64_t *period);
/* The scheme of gol_batch_run_cycles on one board in host memory (a host
 * function, no GPU needed), t0 = 0: the search in launches of `launch` >= 1
 * turns with the turn and the mark arithmetic of gol_batch_cycles_host, the
 * board retired at the end of the launch it is found in, and its remainder from
 * the function the retire pass runs (csrc/gol_batch.h).  `out`, *found and
 * *period are those of gol_batch_cycles_host; *made (may be NULL, as period)
 * = the turns computed, by the formula above.  GOL_EINVAL as there, and for
 * launch < 1. */
int gol_batch_run_cycles_host(int64_t H, int64_t W, uint32_t birth, uint32_t survive, const uint64_t *in, uint64_t *out,
                              int64_t row_stride, int64_t turns, int64_t launch, int64_t *found, int64_t *period,
                              int64_t *made);
/* One soup on host memory (a host function, no GPU needed): soup `index` of
 * (seed, H, W) into H rows of row_stride uint64 words, Ww of each written, with
 * the word function the fill kernels run (csrc/gol_batch.h).  GOL_EINVAL: H or
 * W outside 1..512, index outside 0..2^40, row_stride < Ww, NULL. */
int gol_batch_soup_host(int64_t H, int64_t W, uint64_t seed, int64_t index, uint64_t *out, int64_t row_stride);
/* The scheme of gol_batch_search on host memory (a host function, no GPU
 * needed): soups [first, first + total) through `slots` >= 1 slots in launches
 * of `launch` >= 1 turns, with the row function of gol_batch_step_host, the mark
 * functions and the verdict function the restock pass runs (csrc/gol_batch.h),
 * the snapshot kept once a soup is found as the kernel keeps it, and the
 * refills in the pass's order.  Outputs and refusals as gol_batch_search
 * (period, alive and hash may be NULL); also GOL_EINVAL for H or W outside
 * 1..512, masks >= 512, slots or launch < 1. */
int gol_batch_search_host(int64_t H, int64_t W, uint32_t birth, uint32_t survive, uint64_t seed, int64_t first, int64_t total,
                          int64_t slots, int64_t launch, int64_t horizon, int64_t *found, int64_t *period, uint64_t *alive,
                          uint64_t *hash);
/* The verdict of the restock pass on one slot (a host function; the function of
 * csrc/gol_batch.h): 0 the soup stays, 1 it is found (0 <= found <= horizon), 2 it
 * has expired (not found and age >= horizon, or found at an age above horizon).
 * found < 0: not found yet. */
int gol_batch_verdict_host(int64_t found, int64_t age, int64_t horizon);
/* The argument check of gol_dev_batch_step (a host function, no GPU needed; the
 * function of csrc/gol_batch.h that every launch of the step kernel passes):
 * the arguments of gol_dev_batch_step without the stream.  GOL_OK where that
 * call would launch, GOL_EINVAL where it refuses.  Launches nothing and reads
 * no memory: of a pointer only whether it is NULL counts. */
int gol_batch_step_check_host(const uint64_t *boards, const uint64_t *prev, const int64_t *settled, int64_t n, int64_t H,
                              int64_t W, int32_t turns, int64_t turn0, int32_t have_prev, int32_t write_prev, uint32_t birth,
                              uint32_t survive, const uint32_t *rules, int32_t scan, int64_t done, const int32_t *list,
                              const int32_t *count, int64_t slots, const int64_t *left, const int64_t *born);
/* MAP rules of a batch: any two-state rule of the 3x3 block, the isotropic
 * non-totalistic and the anisotropic ones included, as a table of 512 bits (no
 * version bump: probe by symbol).  The kernel is csrc/gol_batch_map.hip, the
 * circuit it shares with the host functions csrc/gol_map.h.
 *
 * A map is uint32_t map[16].  Its bit i is (map[i >> 5] >> (i & 31)) & 1, for i
 * in 0..511.  For cell (y, x) of an H x W torus:
 *   i = 256 NW + 128 N + 64 NE + 32 W + 16 C + 8 E + 4 SW + 2 S + SE
 * where N is the cell at row (y - 1) mod H and S the one at row (y + 1) mod H, W
 * is at column (x - 1) mod W and E at column (x + 1) mod W, and C is the cell
 * itself.  The formula holds as written on every torus: on W = 1 the three
 * columns are the same cell, on H = 2 the row above is the row below.  The cell
 * is alive next turn iff bit i is set, i = 0 included: a map may give birth on
 * empty ground, as B0 rules do, and the padding of a row's last word still
 * stays clear.
 * Text: "MAP" followed by the base64 (standard alphabet) of the 64 bytes whose
 * bit i is bit 7 - (i & 7) of byte i >> 3, MSB first: 86 characters, which
 * gol_map_parse accepts with or without a trailing "==" (and whose last four
 * bits must be zero); gol_map_format writes the 86.  This is the form Golly and
 * LifeViewer write.  Hensel notation ("B2-a/S12") is not parsed: a caller
 * builds such a rule as a table.
 *  - gol_map_parse: "MAP..." as above, or a life-like rule "B.../S..." through
 *    gol_rule_parse, into map[16].  GOL_EINVAL: NULL, a wrong length, a character
 *    that is not base64, bits after the 512th; map is then untouched.
 *  - gol_map_format: the text of a map into buf, 90 bytes with the final 0;
 *    GOL_EINVAL: NULL, len < 90.
 *  - gol_map_from_rule_host: the life-like rule (9-bit masks) as a map: bit i is
 *    the survive (C set) or birth mask's bit at the count of the other eight.
 *  - gol_map_eval_host: the circuit on nine planes of 32 cells, x[k] the plane of
 *    weight 2^(8 - k) in i, that is x = {NW, N, NE, W, C, E, SW, S, SE}: bit j of
 *    *next = the map's bit at the index formed from bit j of every plane.
 *  - gol_batch_step_map_host: `turns` >= 0 turns of one H x W torus on host
 *    memory under a map, with the row function the kernel runs; in, out and
 *    row_stride as for gol_batch_step_host (they may be the same buffer).
 *    GOL_EINVAL: H or W outside 1..512, row_stride < Ww, turns < 0, NULL.
 *  - gol_batch_set_map: every board under one map.  gol_batch_set_maps: boards
 *    [i0, i1) under maps + 16 (i - i0); the other boards keep what they run
 *    under, a life-like rule as its map; a batch whose maps are all equal runs
 *    as after set_map.  gol_batch_maps: the maps of boards [i0, i1) as the batch
 *    stands (a life-like rule as its map).  The boards and the turn stay.
 *    gol_batch_set_rule and set_rules clear the maps (after set_rules the boards
 *    outside its range run under the rule set_rule gave last, default B3/S23),
 *    and set_map / set_maps clear the rules.  While maps are set gol_batch_rule
 *    and gol_batch_rules return GOL_ESTATE, their outputs untouched.
 *  - Under maps step (with and without settled), step_cycles and run_cycles
 *    work as described above, with one map or a map per board; search, census
 *    and census_sym work under one map and return GOL_ESTATE under differing
 *    maps, as for differing rules.  The island calls, alive_counts, hashes,
 *    loads and stores do not depend on the rule.
 *  - gol_batch_step_map_check_host: the argument check of gol_dev_batch_step_map
 *    (below), its arguments without the stream; as gol_batch_step_check_host. */
int gol_map_parse(const char *text, uint32_t *map);
int gol_map_format(const uint32_t *map, char *buf, int64_t len);
int gol_map_from_rule_host(uint32_t birth, uint32_t survive, uint32_t *map);
int gol_map_eval_host(const uint32_t *map, const uint32_t x[9], uint32_t *next);
int gol_batch_step_map_host(int64_t H, int64_t W, const uint32_t *map, const uint64_t *in, uint64_t *out, int64_t row_stride,
                            int64_t turns);
int gol_batch_set_map(gol_batch *b, const uint32_t *map);
int gol_batch_set_maps(gol_batch *b, int64_t i0, int64_t i1, const uint32_t *maps);
int gol_batch_maps(gol_batch *b, int64_t i0, int64_t i1, uint32_t *maps);
int gol_batch_step_map_check_host(const uint64_t *boards, const uint64_t *prev, const int64_t *settled, int64_t n, int64_t H,
                                  int64_t W, int32_t turns, int64_t turn0, int32_t have_prev, int32_t write_prev,
                                  const uint32_t *maps, int32_t map_each, int32_t scan, int64_t done, const int32_t *list,
                                  const int32_t *count, int64_t slots, const int64_t *left, const int64_t *born);
/* The island census of a batch: per board its islands, the connected groups of
 * alive cells, each with a fingerprint that no torus translation changes,
 * labelled on the GPU in one launch on the boards where they lie (the kernel
 * is csrc/gol_island.hip, the functions it shares with the host twin
 * csrc/gol_island.h).  No version bump: probe by symbol.
 * Board i of a batch is an H x W torus; reach is 1 or 2.
 *  - Link: two alive cells are linked when one is at ((y + dy) mod H, (x + dx)
 *    mod W) of the other for some |dy|, |dx| <= reach.
 *  - Island: a class of the transitive closure of the link.  reach 1 gives the
 *    8-connected islands; reach 2 joins everything that shares a neighbour cell.
 *  - Window code of an alive cell (y, x): the sum over dy, dx in [-reach, reach]
 *    of alive((y + dy) mod H, (x + dx) mod W) << ((dy + reach) (2 reach + 1) + (dx
 *    + reach)).  The formula holds as written on tori narrower than the window,
 *    where a cell may appear in it more than once.
 *  - Term of a cell: splitmix64(code ^ ((uint64_t)reach << 32)), the splitmix64
 *    of the soup words (gol_batch_soup_host).
 *  - Record of an island (gol_island, 24 bytes): (y, x) its first cell in
 *    row-major order, cells its population, rows and cols the numbers of
 *    distinct rows and columns it occupies, hash the wrapping sum of its cells'
 *    terms.
 *  - Order: a board's records are ordered by (y, x) ascending.
 *  - Fingerprint of a board: the wrapping sum of all its islands' hash.
 * Every cell in the window of a cell is linked to it, so it belongs to the
 * cell's own island: cells, rows, cols, hash and the fingerprint do not change
 * under any torus translation of the board (y and x do).  hash and the
 * fingerprint do change under rotation and reflection; the free hash ("island
 * kinds free of orientation", below: the _sym entries with GOL_ISLAND_FREE) does
 * not.
 *
 * gol_batch_islands: boards [i0, i1) of the batch.  count[i - i0] is always the
 * full number of islands of board i.  islands may be NULL when cap == 0;
 * otherwise it has (i1 - i0) cap records, the first min(count, cap) records of
 * board i are written at islands + (i - i0) cap and the rest are not touched.
 * fingerprint may be NULL; otherwise fingerprint[i - i0] covers all islands of
 * the board, those past cap included.  The boards, the turn and the rules
 * stay; the call blocks.  The device scratch for counts and records lives in
 * the handle, grown and reused, and the range is cut into chunks so that it
 * stays at or below 256 MiB.  GOL_EINVAL before any GPU work, outputs
 * untouched: a NULL handle or count, a bad range, reach outside 1..2, cap < 0,
 * or cap > 0 with NULL islands.
 * gol_batch_islands_host: the same census of one board in host memory (a host
 * function, no GPU needed) with the rotation, dilation and term functions the
 * kernel runs; rows of row_stride >= ceil(W / 64) words, the padding bits and
 * the words between the rows are not read.  The outputs and the refusals are
 * those of one board of gol_batch_islands (and a NULL `words` or a short row
 * stride).
 * gol_batch_islands_check_host: the argument check of gol_dev_batch_islands (a
 * host function: the function of csrc/gol_island.h that every launch passes),
 * its arguments without the stream.  GOL_OK where that call would launch,
 * GOL_EINVAL where it refuses; reads no memory. */
typedef struct gol_island {
    int32_t y, x;        /* the island's first cell in row-major order */
    int32_t cells;       /* its population */
    uint16_t rows, cols; /* the distinct rows and columns it occupies */
    uint64_t hash;       /* the wrapping sum of its cells' terms */
} gol_island;
int gol_batch_islands(gol_batch *b, int64_t i0, int64_t i1, int32_t reach, int64_t cap, int64_t *count, gol_island *islands,
                      uint64_t *fingerprint);
int gol_batch_islands_host(int64_t H, int64_t W, int32_t reach, const uint64_t *words, int64_t row_stride, int64_t cap,
                           int64_t *count, gol_island *islands, uint64_t *fingerprint);
int gol_batch_islands_check_host(const uint64_t *boards, int64_t n, int64_t H, int64_t W, int32_t reach, int64_t cap,
                                 const int64_t *count, const gol_island *islands, const uint64_t *fingerprint);
/* The tally of island kinds: what a census of many boards adds up to, built on
 * the GPU so that nothing per island crosses the bus (the kernel is the TALLY
 * form of csrc/gol_island.hip).  No version bump: probe by symbol.
 *  - Kind of an island: its hash, as gol_island.hash is defined above.  Islands
 *    with equal hash nearly always have equal shape, but different islands
 *    with the same multiset of window codes exist: they count as one kind.
 *  - Tally over a set of (owner, island) pairs, an owner being a soup number or
 *    a board index: one gol_island_kind (32 bytes) per distinct kind, with
 *    count the islands of the kind, first the lowest owner that holds one, and
 *    (cells, rows, cols) the smallest such triple, compared in that order,
 *    among the kind's islands.  Every field is an order-independent reduction
 *    (a sum, a minimum, a minimum of cells << 32 | rows << 16 | cols), so the
 *    tally is a function of the set of pairs alone.
 *  - Order of a tally: count descending, then hash ascending.
 *  - Device table: an open-addressing array of 2^log2 slots of 32 bytes, 4 <=
 *    log2 <= 24.  A slot is four 64-bit words: hash (the tag, claimed by a
 *    compare-and-swap from 0), count, first, and the shape packed as cells << 32
 *    | rows << 16 | cols in one word (so its minimum is one 64-bit atomic; a
 *    gol_island_kind has the same bytes but for this word, which
 *    gol_batch_census and gol_batch_islands_tally unpack on the host).  An
 *    empty slot is {0, 0, INT64_MAX, all ones}.  An island whose hash is 0 is
 *    tallied under hash 1 (one hash in 2^64; no field is spent on it).  An
 *    island's home slot is gol_island_tally_home_host(hash, log2) < 2^log2 and
 *    a probe goes on to the next slot, round the table.  Which slot a kind
 *    ends in depends on the order of insertion: no public output depends on
 *    it, every one is sorted on the host after one read-back.
 *  - Full table: an island whose probe has visited all 2^log2 slots without
 *    finding its kind or an empty slot is not tallied, and the device counter
 *    `dropped` grows by one.
 *
 * gol_batch_census: gol_batch_search (above) with the census of every soup's
 * s(found) taken inside the search's harvest, one more launch per round over
 * the same harvest list.  found, period, alive, hash and stats are exactly those
 * of gol_batch_search for the same arguments (period, alive, hash, islands,
 * fingerprint and stats may each be NULL).  islands[g - first] and fingerprint[g
 * - first] are the island count and the fingerprint of s(found) at `reach`, 0
 * and 0 for a soup not found.  The tally is over the pairs (g, island of
 * s(found) of soup g): *n_kinds is the number of distinct kinds, and `kinds`
 * receives the first min(*n_kinds, kinds_cap) of them in the tally's order;
 * `first` holds the soup number g (first included), so gol_batch_soup_host
 * re-makes an example.  Nothing depends on the number of slots, on
 * turns_per_launch or on which slot a soup ran in.  The kind table lives in
 * the handle: the smallest power of two >= 2 max(kinds_cap, 512) slots, at most
 * 2^24.  `dropped` is read once, at the end: if it is not 0 the call returns
 * GOL_ENOMEM with a message naming kinds_cap, the per-soup outputs written and
 * valid, `kinds` untouched and *n_kinds = -1.  Refused before any GPU work, the
 * batch and the outputs untouched: as gol_batch_search, and GOL_EINVAL for
 * reach outside 1..2, kinds_cap < 0 or > 2^23, a NULL n_kinds, kinds_cap > 0 with
 * NULL kinds.
 * gol_batch_islands_tally: the tally of boards [i0, i1) as they stand, owner =
 * the board's index: count[i - i0] and fingerprint[i - i0] (may be NULL) as
 * gol_batch_islands gives them, kinds, kinds_cap, *n_kinds, the table's size and
 * GOL_ENOMEM as for gol_batch_census.  The range is cut into chunks by the rule
 * of gol_batch_islands; no record is kept on the device.  The boards, the turn
 * and the rules stay.  GOL_EINVAL as gol_batch_islands and as above.
 * gol_island_tally_host: the definition on host memory (a host function, no
 * GPU needed): the tally of the pairs (owners[i], records[i]), i < n, by a sort
 * and a merge; outputs as above.  GOL_EINVAL: n < 0, NULL records or owners
 * with n > 0, kinds_cap < 0, NULL n_kinds, kinds_cap > 0 with NULL kinds.
 * gol_batch_census_host: gol_batch_search_host, gol_batch_islands_host on every
 * soup's s(found) and gol_island_tally_host (a host function); arguments,
 * outputs and refusals as those three (no table, so no GOL_ENOMEM for a small
 * kinds_cap).
 * gol_island_tally_home_host: the home slot of a hash in a table of 2^log2
 * slots (the function of csrc/gol_island.h the kernel runs); -1 for log2
 * outside 4..24.
 * gol_batch_islands_tally_check_host: the argument check of
 * gol_dev_batch_islands_tally (below; a host function), its arguments without
 * the stream: GOL_OK where that call would launch, GOL_EINVAL where it refuses;
 * reads no memory. */
typedef struct gol_island_kind {
    uint64_t hash;       /* the kind */
    int64_t count;       /* islands of this kind */
    int64_t first;       /* the lowest owner (soup number, or board index) that holds one */
    int32_t cells;       /* the smallest (cells, rows, cols), compared in that order, among them */
    uint16_t rows, cols;
} gol_island_kind;
int gol_batch_census(gol_batch *b, uint64_t seed, int64_t first, int64_t total, int64_t horizon, int32_t reach, int64_t *found,
                     int64_t *period, uint64_t *alive, uint64_t *hash, int64_t *islands, uint64_t *fingerprint,
                     gol_island_kind *kinds, int64_t kinds_cap, int64_t *n_kinds, gol_batch_search_stats *stats);
int gol_batch_islands_tally(gol_batch *b, int64_t i0, int64_t i1, int32_t reach, int64_t *count, uint64_t *fingerprint,
                            gol_island_kind *kinds, int64_t kinds_cap, int64_t *n_kinds);
int gol_island_tally_host(const gol_island *records, const int64_t *owners, int64_t n, gol_island_kind *kinds, int64_t kinds_cap,
                          int64_t *n_kinds);
int gol_batch_census_host(int64_t H, int64_t W, uint32_t birth, uint32_t survive, uint64_t seed, int64_t first, int64_t total,
                          int64_t slots, int64_t launch, int64_t horizon, int32_t reach, int64_t *found, int64_t *period,
                          uint64_t *alive, uint64_t *hash, int64_t *islands, uint64_t *fingerprint, gol_island_kind *kinds,
                          int64_t kinds_cap, int64_t *n_kinds);
int64_t gol_island_tally_home_host(uint64_t hash, int32_t table_log2);
int gol_batch_islands_tally_check_host(const uint64_t *boards, int64_t n, int64_t H, int64_t W, int32_t reach, const int32_t *pairs,
                                       const int32_t *pair_count, int64_t max_pairs, const int64_t *found, int64_t owner0,
                                       const int64_t *count, const uint64_t *fingerprint, const gol_island_kind *table,
                                       int32_t table_log2, const int64_t *dropped);
/* Island kinds free of orientation: a hash that no rotation or reflection of
 * an island changes, so that a tally holds one line per object however it is
 * turned (the FREE form of the kernel of csrc/gol_island.hip).  No version
 * bump: probe by symbol.  reach, window code and term are those of the island
 * census above.
 *  - Orientations: the eight symmetries of the square are numbered s = 0..7
 *    with t = s & 1 (transpose), fy = (s >> 1) & 1 (rows flipped), fx = (s >> 2)
 *    & 1 (columns flipped).
 *  - The code in orientation s: for a window code c, orient(c, reach, s) is the
 *    code whose bit at (dy, dx) is the bit of c at (dy', dx'), where (a, b) = t ?
 *    (dx, dy) : (dy, dx), dy' = fy ? -a : a, dx' = fx ? -b : b.  orient(c, reach,
 *    0) == c.
 *  - The hash of an island in orientation s: the wrapping sum of
 *    term(orient(code, reach, s)) over its cells.  Its free hash is the smallest
 *    of the eight, compared as unsigned 64-bit numbers.
 *  - Free fingerprint of a board: the wrapping sum of its islands' free hashes.
 * The eight maps are the whole group, and the window of a cell holds only
 * cells of its own island, so the eight sums of an island are the hashes
 * (symmetry 0) of its eight images, and the set of eight is the same for every
 * image: the minimum does not change under translation, rotation or
 * reflection.  The window formula holds as written on tori narrower than the
 * window, so this is true on every torus, and between an H x W board and its W
 * x H transpose.  Phase is not factored out: an oscillator whose phases are not
 * images of each other has one kind per phase.
 * symmetry selects the hash: GOL_ISLAND_FIXED (the hash of the island census
 * above) or GOL_ISLAND_FREE; every other value is refused.  With
 * GOL_ISLAND_FREE gol_island.hash, the fingerprint, gol_island_kind.hash and the
 * table's tag are the free ones; y, x, cells, rows and cols (they describe the
 * island as it lies), the order of records, the rule that hash 0 is tallied
 * under 1, the tally's reductions and order and both struct layouts stay.
 *
 * Every _sym entry is the entry of the same name without _sym, with symmetry
 * after reach: with GOL_ISLAND_FIXED it is that entry (which is this call),
 * outputs and refusals alike; and GOL_EINVAL before any GPU work, outputs
 * untouched, for a symmetry outside 0..1.  (gol_island_tally_host takes records,
 * so it tallies either kind of hash.)
 * gol_island_orient_host: orient(code, reach, s) (a host function: the function
 * of csrc/gol_island.h the kernel runs); 0 for an s outside 0..7 or a reach
 * outside 1..2. */
#define GOL_ISLAND_FIXED 0
#define GOL_ISLAND_FREE 1
int gol_batch_islands_sym(gol_batch *b, int64_t i0, int64_t i1, int32_t reach, int32_t symmetry, int64_t cap, int64_t *count,
                          gol_island *islands, uint64_t *fingerprint);
int gol_batch_islands_tally_sym(gol_batch *b, int64_t i0, int64_t i1, int32_t reach, int32_t symmetry, int64_t *count,
                                uint64_t *fingerprint, gol_island_kind *kinds, int64_t kinds_cap, int64_t *n_kinds);
int gol_batch_census_sym(gol_batch *b, uint64_t seed, int64_t first, int64_t total, int64_t horizon, int32_t reach,
                         int32_t symmetry, int64_t *found, int64_t *period, uint64_t *alive, uint64_t *hash, int64_t *islands,
                         uint64_t *fingerprint, gol_island_kind *kinds, int64_t kinds_cap, int64_t *n_kinds,
                         gol_batch_search_stats *stats);
int gol_batch_islands_sym_host(int64_t H, int64_t W, int32_t reach, int32_t symmetry, const uint64_t *words, int64_t row_stride,
                               int64_t cap, int64_t *count, gol_island *islands, uint64_t *fingerprint);
int gol_batch_census_sym_host(int64_t H, int64_t W, uint32_t birth, uint32_t survive, uint64_t seed, int64_t first, int64_t total,
                              int64_t slots, int64_t launch, int64_t horizon, int32_t reach, int32_t symmetry, int64_t *found,
                              int64_t *period, uint64_t *alive, uint64_t *hash, int64_t *islands, uint64_t *fingerprint,
                              gol_island_kind *kinds, int64_t kinds_cap, int64_t *n_kinds);
int gol_batch_islands_sym_check_host(const uint64_t *boards, int64_t n, int64_t H, int64_t W, int32_t reach, int32_t symmetry,
                                     int64_t cap, const int64_t *count, const gol_island *islands, const uint64_t *fingerprint);
int gol_batch_islands_tally_sym_check_host(const uint64_t *boards, int64_t n, int64_t H, int64_t W, int32_t reach,
                                           int32_t symmetry, const int32_t *pairs, const int32_t *pair_count, int64_t max_pairs,
                                           const int64_t *found, int64_t owner0, const int64_t *count,
                                           const uint64_t *fingerprint, const gol_island_kind *table, int32_t table_log2,
                                           const int64_t *dropped);
uint64_t gol_island_orient_host(uint64_t code, int32_t reach, int32_t s);
/* The argument check of the step launches (a host function, no GPU needed; the
 * function of csrc/gol_step_launch.h that every launch of a step kernel passes,
 * from gol_dev_bits_step, _band_step(_on), _rule_step, _bytes_step_k(_on) and from
 * the engine).  family: the kernels of gol_dev_bits_step, gol_dev_band_step,
 * gol_dev_rule_step in the standard and in the band layout, gol_dev_bytes_step_k.
 * The arguments are those entries' (width and pitch: Wd and pitch in words, for
 * BYTES W and stride in bytes; cus, slots: those of the _on entries, else 0)
 * with words_per_lane in place of cells_per_lane: cells_per_lane / 32, the
 * default resolved (64 cells; band 128), 1 for BYTES.  as_entry != 0: as the C
 * entries answer; 0: as the engine's launches are checked, which also have the
 * band kernel of k = 12 at 2 words per lane.  GOL_OK where the launch would be
 * made, GOL_EINVAL where it is refused (what only a device can refuse -- cus or
 * slots above its own -- is not looked at).  geometry (may be NULL) receives,
 * for a launch that passes: [0] the output words of a wave's column group, [1]
 * the column groups of a row, [2] 1 where the ghost rows are contiguous with
 * the shard (top + k rows == mid and bot == mid + R rows), [3] 1 for a
 * pipelined kernel.  Launches nothing and reads no memory: of a pointer only
 * its value counts.  No version bump: probe by symbol. */
#define GOL_FAMILY_BITS 0
#define GOL_FAMILY_BAND 1
#define GOL_FAMILY_RULE_STD 2
#define GOL_FAMILY_RULE_BAND 3
#define GOL_FAMILY_BYTES 4
int gol_step_check_host(int32_t family, const void *top, const void *mid, const void *bot, const void *dst, int64_t R,
                        int64_t width, int64_t pitch, int64_t row0, int64_t rows, int32_t k, int32_t words_per_lane,
                        uint32_t birth, uint32_t survive, int32_t cus, int32_t slots, int32_t as_entry, int32_t *geometry);

/* ---------------------------------------------------------------- plans
 * The schedule of a sharded step as data (host functions, no GPU needed).  The
 * engine runs exactly these plans; golhip.sharded (the torch.distributed
 * mirror) and the tests read them.  Replaces the broker's per-turn fan-out
 * (broker.go:135-206: every worker gets the whole board) by a k-row halo with
 * the ring neighbours.
 *
 * gol_halo_plan: the halo exchange of global rank `rank` of an H-row board
 * split over nranks shards (gol_partition_rows), k rows each way, in issue
 * order.  Sends read shard-local rows [row, row + rows) of the shard, receives
 * write its ghost rows [row, row + rows) (row = -k or R).  A receiver matches
 * the sends addressed to it by one sender with its receives from that sender
 * in issue order (ncclSend/ncclRecv semantics; for nranks = 2 both neighbours
 * are one peer, for nranks = 1 the shard sends to itself: the torus wrap).
 * Writes min(4, cap) ops; *n = 4. */
#define GOL_HALO_SEND 0
#define GOL_HALO_RECV 1
typedef struct gol_halo_op {
    int32_t kind;  /* GOL_HALO_SEND / GOL_HALO_RECV */
    int32_t peer;  /* global rank of the other side */
    int64_t row;   /* first shard-local row of the block */
    int64_t rows;  /* k */
} gol_halo_op;
int gol_halo_plan(int64_t H, int32_t nranks, int32_t rank, int32_t k, gol_halo_op *ops, int32_t cap, int32_t *n);
/* gol_step_plan: the launches of one k-turn step of a shard of R rows whose
 * halo exchanges carry kx >= k rows, in launch order.  EDGE launches run on
 * the shard's edge stream, MAIN launches on its compute stream; a launch that
 * needs_halo waits for the exchange.  The next step's exchange starts when the
 * last launch that needs the halo (they write rows [0, kx) and [R - kx, R),
 * the rows it sends) is done.  With R >= 3 kx:
 *  - GOL_STEP_OVERLAP: rows [0, kx) and [R - kx, R) on the edge stream, the
 *    interior [kx, R - kx) (it reads no ghost row) on the compute stream
 *    beside them: nothing waits for the exchange but the edge launches;
 *  - GOL_STEP_EDGE_FIRST: the same three launches in order on the compute
 *    stream (the exchange overlaps the interior; no second kernel competes
 *    with the interior for the CUs);
 *  - neither (or GOL_STEP_SERIAL, or R < 3 kx): one MAIN launch over [0, R).
 * The engine picks per step: OVERLAP for launches of many
 * rounds of workgroups, SERIAL below, unless gol_config.flags forces one.
 * Writes min(n, cap) launches. */
#define GOL_LAUNCH_MAIN 0
#define GOL_LAUNCH_EDGE 1
typedef struct gol_launch {
    int32_t stream;     /* GOL_LAUNCH_MAIN / GOL_LAUNCH_EDGE */
    int32_t needs_halo; /* reads the ghost rows: waits for the exchange */
    int64_t row0;       /* first shard-local output row */
    int64_t rows;
} gol_launch;
int gol_step_plan(int64_t R, int32_t k, int32_t kx, int32_t flags, gol_launch *out, int32_t cap, int32_t *n);
/* gol_view_plan: the rows of a viewport that shard `rank` of gol_partition_rows(H,
 * nranks, .) holds.  Viewport row v (0 <= v < vrows <= H) is global row
 * (y0 + v) mod H; a run is `rows` consecutive rows from shard-local row `row`,
 * which are viewport rows vrow .. vrow + rows - 1.  Runs come in increasing
 * vrow order, at most 2 per shard (the second from the torus wrap); over all
 * ranks they cover every viewport row once.  Writes min(*n, cap) runs.  The
 * engine's view calls run exactly this plan. */
typedef struct gol_view_run {
    int64_t row;   /* first shard-local source row */
    int64_t rows;
    int64_t vrow;  /* first viewport row */
} gol_view_run;
int gol_view_plan(int64_t H, int32_t nranks, int32_t rank, int64_t y0, int64_t vrows, gol_view_run *runs, int32_t cap,
                  int32_t *n);
/* gol_strip_plan: which workgroup of a pipelined launch computes which output
 * rows.  The two pipeline kernels (k = 12 of gol_dev_band_step at 128 cells per
 * lane, k = 32 of gol_dev_bytes_step_k) run one workgroup per (column group,
 * range of rows), and the launch code picks one of several schedules from the
 * launch's shape and two device properties: the CU count `cus` and `slots`, the
 * workgroups of the kernel resident on the whole device at once.  This is that
 * choice and its outcome as data, from the functions the launchers and the
 * kernels themselves run (csrc/gol_strips.h); no GPU needed.  (Added without a
 * version bump: GOL_ABI_VERSION stays 6; probe for gol_strip_plan,
 * gol_dev_band_step_on and gol_dev_bytes_step_k_on by symbol.)
 * Arguments as the kernel's launcher takes them: `width` and `pitch` are Wd and
 * pitch in words (band), W in cells and stride in bytes (bytes); rows
 * [row0, row0 + rows) are written; strip_rows > 0 asks for strips of that
 * length.  k must be the pipeline's (12 / 32); cus >= 0, slots >= 0.
 * The modes:
 *  - SMALL: ~512 tiles of >= 2 rows on a latency-bound board (band only);
 *  - EXPLICIT: strip_rows > 0;
 *  - PLAIN: strips of the default length, a launch of many rounds with no tail;
 *  - ROUND_TILED: at most 4 rounds of workgroups, the strip count a multiple of
 *    a round;
 *  - TAIL: strips, the last round of workgroups on shorter ones from row
 *    tail_row on (band only);
 *  - RANKED_STATIC: one round of cus x per_cu workgroups; a CU takes `period`
 *    rows of one column group and splits them over its workgroups by arrival
 *    rank;
 *  - RANKED_PAIRED: as RANKED_STATIC, with pairs of workgroups that walk one
 *    range from both ends and claim blocks of RPB rows, NS blocks at a time,
 *    from a counter of the pair until nclaim blocks are claimed.  A walker that
 *    claimed n blocks stores RPB*n - 2K rows: from s0 down (dir +1), from s1e
 *    up (dir -1), clipped to [s0, s1).
 * Record l is workgroup id l: column group, rows [s0, s1) (s0 >= s1: the
 * workgroup has no rows and leaves at once), dir 0 (a strip of its own) or +1 /
 * -1 (a pair's walkers), claim = index of the pair's counter (-1 without),
 * s1e, nclaim (dir 0: s1e = s1).  Writes min(*n, cap) records; recs may be NULL
 * with cap 0 (the two-call form). */
#define GOL_STRIP_KERNEL_BAND 0
#define GOL_STRIP_KERNEL_BYTES 1
#define GOL_STRIPS_SMALL 0
#define GOL_STRIPS_EXPLICIT 1
#define GOL_STRIPS_PLAIN 2
#define GOL_STRIPS_ROUND_TILED 3
#define GOL_STRIPS_TAIL 4
#define GOL_STRIPS_RANKED_STATIC 5
#define GOL_STRIPS_RANKED_PAIRED 6
typedef struct gol_strip_info {
    int32_t mode;       /* GOL_STRIPS_* */
    int32_t ngroups;    /* column groups */
    int32_t strip;      /* rows per strip (ranked modes: unused) */
    int32_t K, RPB, NS; /* the kernel's turns, rows per block, blocks per claim */
    int32_t per_cu;     /* ranked modes: workgroups per CU, */
    int32_t period;     /*   rows of a column group per CU */
    int32_t tail_first; /* TAIL: first workgroup id of the tail, */
    int32_t tail_row;   /*   its first row (relative to row0), */
    int32_t tail_strip; /*   its rows per strip */
    int32_t reserved;
} gol_strip_info;
typedef struct gol_strip_rec {
    int32_t group;
    int32_t s0, s1;
    int32_t dir;
    int32_t claim;
    int32_t s1e, nclaim;
} gol_strip_rec;
int gol_strip_plan(int32_t kernel, int64_t rows, int64_t row0, int64_t width, int64_t pitch, int32_t k,
                   int32_t strip_rows, int32_t cus, int32_t slots, gol_strip_info *info, gol_strip_rec *recs,
                   int64_t cap, int64_t *n);

/* ---------------------------------------------------------------- device launchers
 * Asynchronous kernel launches on caller-owned device memory and a caller
 * stream (hipStream_t passed as void*; NULL = default stream).  These are the
 * building blocks of the row-sharded multi-GPU board (one process per GPU;
 * broker.go:135-206's partition applied to GPUs) and of bench.py.
 * Arguments are checked before anything is launched (GOL_EINVAL); rows == 0 (an
 * empty slab) is GOL_OK and launches nothing.  With a pitch or stride larger than
 * the width the words or bytes between the rows are neither read nor written.
 *
 * Bit board of one shard: R local rows, Wd = W/32 uint32 words per row, row
 * pitch `pitch` words.  Input row y of the shard (-k <= y < R + k) is read
 * from: top + (y + k)*pitch for y < 0, mid + y*pitch for 0 <= y < R,
 * bot + (y - R)*pitch for y >= R.  (One GPU: top = mid + (R-k)*pitch,
 * bot = mid, the torus wrap; several GPUs: the k-row halo buffers received
 * from the neighbouring ranks.)  Writes rows [row0, row0 + rows) of dst
 * after k turns.  If count_slots is non-NULL the alive cells of the written
 * rows are added to count_slots[0 .. GOL_COUNT_SLOTS*8) (sum them all). */
#define GOL_COUNT_SLOTS 256
int gol_dev_bits_step(const uint32_t *top, const uint32_t *mid, const uint32_t *bot, uint32_t *dst,
                      int64_t R, int64_t Wd, int64_t pitch, int64_t row0, int64_t rows, int32_t k,
                      int32_t cells_per_lane, int32_t strip_rows, uint64_t *count_slots,
                      void *stream);
/* Fill rows [0, rows) of a bit board with the synthetic board rows
 * [grow0, grow0 + rows) of a W-wide torus (W % 64 == 0; pitch even, dst 8-byte
 * aligned: a row is written as 64-bit words). */
int gol_dev_random_fill(uint32_t *dst, int64_t rows, int64_t grow0, int64_t W, int64_t pitch,
                        uint64_t seed, void *stream);
/* Add popcount(rows x Wd words) to slots (GOL_COUNT_SLOTS*8 uint64: sum them
 * all); any Wd >= 1, odd ones too. */
int gol_dev_popcount(const uint32_t *src, int64_t rows, int64_t Wd, int64_t pitch,
                     uint64_t *slots, void *stream);
/* Add the board-hash contribution of rows whose first global row is grow0 to
 * slots (as gol_dev_popcount; sums are modulo 2^64, so the parts of any split of
 * the rows add up to the whole).  Wd and pitch even, src 8-byte aligned. */
int gol_dev_hash(const uint32_t *src, int64_t rows, int64_t grow0, int64_t Wd, int64_t pitch,
                 uint64_t *slots, void *stream);
/* Bytes <-> bits for rows x W cells (W % 32 == 0): bit = (byte == 255), byte =
 * 0 or 255; pack also ORs 1 into *nonbinary when a byte other than 0/255 is
 * seen inside the rows x W cells (may be NULL).  The byte rows may start at any
 * address and have any stride >= W (unpack stores 16 bytes at a time where a
 * row is 16-byte aligned and single bytes elsewhere). */
int gol_dev_pack(const uint8_t *bytes, int64_t rows, int64_t W, int64_t stride, uint32_t *bits,
                 int64_t pitch, uint32_t *nonbinary, void *stream);
int gol_dev_unpack(const uint32_t *bits, int64_t rows, int64_t W, int64_t pitch, uint8_t *bytes,
                   int64_t stride, void *stream);
/* One exact-semantics byte turn (worker.go:15-70) for rows [y0, y1) of an
 * H x W byte torus; out row i = next state of row y0 + i.  Any W, strides and
 * addresses: 16 cells per lane when W, both strides and both pointers are
 * multiples of 16, one cell per thread otherwise, with the same result. */
int gol_dev_bytes_step(const uint8_t *world, int64_t H, int64_t W, int64_t stride, int64_t y0,
                       int64_t y1, uint8_t *out, int64_t out_stride, void *stream);

/* k turns (1, 2, 4, 8, 16 or 32; 32 runs as 8 waves x 4 turns of one workgroup, the
 * byte pipeline) of a byte board whose bytes are all 0 or 255 (every
 * board after its first turn), W % 32 == 0, stride % 16 == 0, 16-byte aligned
 * rows; row addressing as gol_dev_bits_step (top/mid/bot are byte rows, pitch
 * `stride`).  Same results as k exact turns on such boards; 2 bytes of HBM
 * traffic per cell per k turns.  count_slots as in gol_dev_bits_step. */
int gol_dev_bytes_step_k(const uint8_t *top, const uint8_t *mid, const uint8_t *bot, uint8_t *dst, int64_t R,
                         int64_t W, int64_t stride, int64_t row0, int64_t rows, int32_t k, int32_t strip_rows,
                         uint64_t *count_slots, void *stream);

/* k turns of a BAND-layout bit board (bit b of word w = cell b*Wd + w); row
 * addressing and count_slots as gol_dev_bits_step.  cells_per_lane: 64 or 128
 * (2 or 4 words per lane; 0 = library default); k in {1, 2, 4, 8}, 16 with 64
 * cells per lane, 12 with 128 (the split pipeline: 4 waves x 3 turns); Wd and
 * pitch multiples of the words per lane, rows aligned to 4 bytes x words per
 * lane.  Same cells as gol_dev_bits_step on the standard layout, with no bit
 * shifts in the generation.  The pipelined kernels (k = 12 here, k = 32 in
 * gol_dev_bytes_step_k) report a device-side protocol fault in the device's
 * error word: check it with gol_dev_error after synchronising the stream. */
int gol_dev_band_step(const uint32_t *top, const uint32_t *mid, const uint32_t *bot, uint32_t *dst,
                      int64_t R, int64_t Wd, int64_t pitch, int64_t row0, int64_t rows, int32_t k,
                      int32_t cells_per_lane, int32_t strip_rows, uint64_t *count_slots, void *stream);
/* gol_dev_band_step / gol_dev_bytes_step_k with the launch scheduled as for a
 * device of `cus` CUs holding `slots` resident workgroups of the kernel
 * (gol_strip_plan with the same arguments is the schedule it runs); 0, 0 = this
 * device, the plain call.  GOL_EINVAL unless cus % 8 == 0, cus <= the device's
 * CU count, slots <= the device's resident count for the kernel, and k is the
 * pipelined one (12 at 128 cells per lane / 32).  Per-call arguments: no
 * process-wide state.  Paired workgroups never wait for each other, so a
 * pretended device computes the same rows whatever else is resident.
 * gol_dev_pipe_limits reports the current device's two values for the kernel
 * (GOL_STRIP_KERNEL_*) as a launch with contiguous ghost rows (band: top + k
 * rows == mid and bot == mid + R rows; the byte kernel has one form) and with
 * count_slots (`counted`) runs it.  No version bump: probe by symbol. */
int gol_dev_band_step_on(const uint32_t *top, const uint32_t *mid, const uint32_t *bot, uint32_t *dst,
                         int64_t R, int64_t Wd, int64_t pitch, int64_t row0, int64_t rows, int32_t k,
                         int32_t cells_per_lane, int32_t strip_rows, uint64_t *count_slots, void *stream,
                         int32_t cus, int32_t slots);
int gol_dev_bytes_step_k_on(const uint8_t *top, const uint8_t *mid, const uint8_t *bot, uint8_t *dst, int64_t R,
                            int64_t W, int64_t stride, int64_t row0, int64_t rows, int32_t k, int32_t strip_rows,
                            uint64_t *count_slots, void *stream, int32_t cus, int32_t slots);
int gol_dev_pipe_limits(int32_t kernel, int32_t contiguous, int32_t counted, int32_t *cus, int32_t *slots);
/* k turns (1, 2, 4 or 8) of a life-like rule (birth / survive: 9-bit masks, see
 * "life-like rules") on a bit board in the standard (GOL_LAYOUT_STANDARD) or
 * the band (GOL_LAYOUT_BAND) layout; row addressing and count_slots as
 * gol_dev_bits_step.  cells_per_lane: 64 (0 = default, the same); Wd and pitch
 * even, rows 8-byte aligned.  No version bump: probe by symbol. */
int gol_dev_rule_step(const uint32_t *top, const uint32_t *mid, const uint32_t *bot, uint32_t *dst,
                      int64_t R, int64_t Wd, int64_t pitch, int64_t row0, int64_t rows, int32_t k,
                      int32_t layout, uint32_t birth, uint32_t survive, int32_t cells_per_lane,
                      int32_t strip_rows, uint64_t *count_slots, void *stream);
/* Largest k gol_dev_band_step accepts for this cells_per_lane (0 = default);
 * 0 if cells_per_lane is not supported. */
int gol_band_max_k(int32_t cells_per_lane);
/* Convert rows x Wd words between the standard and the band layout (to_band
 * != 0: standard -> band), out of place; Wd % 32 == 0 (W % 1024 == 0). */
int gol_dev_band_convert(int32_t to_band, const uint32_t *src, uint32_t *dst, int64_t rows, int64_t Wd,
                         int64_t src_pitch, int64_t dst_pitch, void *stream);
/* The retire pass of gol_batch_run_cycles on caller device memory (one
 * workgroup; stable and deterministic; no version bump: probe by symbol).
 * counts is int32_t[2] in device memory, read and written: counts[0] the entries
 * of list_in on entry and of active on return, counts[1] those of finish on
 * entry and on return.  Boards are numbers in 0..n-1, 1 <= n <= 2^20 (an entry
 * outside is dropped); found and left are int64_t[n], indexed by board.  First
 * finish loses, in place, every board whose left[] is 0.  Then, in the order of
 * list_in: a board with found[] < 0 goes to active (which may be list_in
 * itself); a board found gets left[] = (t_end - t_now) mod (found - the last
 * mark before found, the marks t0 + 2^j - 1) and, unless that is 0, goes to the
 * end of finish, which must hold n entries.  Entries past the two new counts
 * and left[] of boards not in list_in are not written.  GOL_EINVAL: NULL, n out
 * of range, or not 0 <= t0 <= t_now <= t_end. */
int gol_dev_batch_retire(const int32_t *list_in, int32_t *counts, const int64_t *found, int64_t n, int64_t t0,
                         int64_t t_now, int64_t t_end, int32_t *active, int32_t *finish, int64_t *left, void *stream);
/* The restock pass of gol_batch_search on caller device memory (one workgroup;
 * stable and deterministic; no version bump: probe by symbol).  Slots are
 * numbers in 0..n-1, 1 <= n <= 2^20 (an entry outside is dropped); found_age,
 * born (int64_t[n]) and soup (int32_t[n], a soup's number in 0..total-1, total <=
 * 2^26) are indexed by slot, out_found and out_period (int64_t[total]) by soup.
 * counts is int32_t[4] in device memory: [0] the entries of `active`, read and
 * written; [1] written: the slots that are done; [2] written: those of them
 * refilled; [3] the soups handed out so far, read and written.  In the order
 * of `active`: a slot's verdict comes from found_age[slot], its age now -
 * born[slot] and horizon (gol_batch_verdict_host).  A slot that stays stays.  A
 * slot that is done writes out_found and out_period of its soup (the found age
 * and found age - the last mark before it, or -1, -1 when expired) and goes on
 * the harvest list (int32_t[2 n]) as the pair (slot, soup); the r-th done slot
 * takes soup counts[3] + r while that is below total (soup[slot] that number,
 * born[slot] = now, found_age[slot] = -1; it stays in `active`), else it leaves
 * `active`, which is compacted in place.  The refilled slots are therefore the
 * first counts[2] pairs of the harvest list.  Entries past the new counts are
 * not written.  GOL_EINVAL: NULL, n or total out of range, now or horizon < 0. */
int gol_dev_batch_restock(int32_t *active, int32_t *counts, int64_t *found_age, int64_t *born, int32_t *soup, int64_t n,
                          int64_t now, int64_t horizon, int64_t total, int64_t *out_found, int64_t *out_period,
                          int32_t *harvest, void *stream);
/* One launch of the batch step kernel on caller device memory (the launch the
 * gol_batch_* stepping calls are made of; no version bump: probe by symbol).
 * boards: n boards (1 <= n <= 2^20) of H rows of Ww = ceil(W / 64) uint64 words,
 * dense, in the batch's bit order, padding bits zero; 1 <= H, W <= 512.  Board b
 * holds s_b(turn0) before the launch; s_b(t + 1) is one turn of s_b(t) under the
 * board's rule: rules == NULL: birth / survive (9-bit masks) for every board, else
 * rules is uint32_t[2 n], board b under birth rules[2 b], survive rules[2 b + 1].
 * turns >= 1.  prev has the shape of boards, settled, left and born are int64_t[n],
 * all indexed by the board's own number.  The mode is in the arguments:
 *  - plain (scan 0; settled, list, count, left, born NULL; slots 0; have_prev
 *    and write_prev 0): every board becomes s(turn0 + turns).  prev is not used.
 *  - settle (scan 1, settled and prev not NULL, no list): every board becomes
 *    s(turn0 + turns).  have_prev != 0: prev[b] holds s_b(turn0 - 1), and f is the
 *    smallest t in turn0 + 1 .. turn0 + turns with s(t) == s(t - 2); have_prev ==
 *    0: prev is not read and t starts at turn0 + 2.  write_prev != 0: prev[b]
 *    becomes s_b(turn0 + turns - 1); else prev is not written.
 *  - cycles (scan 2, settled and prev not NULL; done >= 0 the turns of the scan
 *    before this launch, have_prev == (done > 0)): every board becomes s(turn0 +
 *    turns).  The board's snapshot is prev[b] when done > 0, else s_b(turn0).  For
 *    it = 1 .. turns in turn: s(turn0 + it) is compared with the snapshot, f is
 *    the first turn0 + it at which they are equal, and after the comparison, if
 *    done + it is a mark (2^j - 1), the snapshot becomes s(turn0 + it).
 *    write_prev != 0: prev[b] becomes the snapshot after the last turn.
 *  - list + cycles (list, count, settled and prev not NULL, left and born NULL,
 *    scan 2, 1 <= slots <= n): cycles on the boards list[0 .. *count) alone.
 *  - finish (list, count and left not NULL, settled and born NULL, scan 0,
 *    have_prev and write_prev 0, 1 <= slots <= n): a listed board b makes m =
 *    min(turns, left[b]) turns, to s_b(turn0 + m), and left[b] becomes left[b] - m
 *    (left[b] >= 0; it is not written when m == 0).
 *  - aged (born not NULL: list + cycles with turn0 == 0, rules == NULL, write_prev
 *    != 0, have_prev == (done > 0)): a listed board b has the age a = done -
 *    born[b] >= 0 before the launch and becomes s_b(a + turns), its turns counted
 *    in its own age.  Its snapshot is prev[b] when a > 0, else the board as
 *    loaded (prev[b] is not read).  For it = 1 .. turns: s(a + it) is compared with
 *    the snapshot, f is the first age a + it at which they are equal, and after
 *    the comparison, if a + it is a mark and the launch has not found the board
 *    at a + it or before, the snapshot becomes s(a + it).  prev[b] becomes the
 *    snapshot: s(f) for a board this launch found.
 * In every scanning mode settled[b] (the found turn; aged: the found age) becomes
 * f where the launch has an f for board b and settled[b] was negative; it is
 * written in no other case.  A slot at or past *count, and every board not listed,
 * is left untouched in every buffer; list, count, born and rules are only read.
 * Not checked (the caller's part): the entries list[0 .. *count) are distinct
 * board numbers in 0 .. n - 1, 0 <= *count <= slots, left[] >= 0 and born[] <= done
 * of the listed boards, and all pointers are device memory of the stated sizes
 * (list: at least *count entries).  GOL_EINVAL, nothing launched: a combination of
 * arguments that is none of the modes above, n, H, W out of range, turns < 1, a
 * mask >= 512, done < 0, slots outside 1 .. n with a list. */
int gol_dev_batch_step(uint64_t *boards, uint64_t *prev, int64_t *settled, int64_t n, int64_t H, int64_t W, int32_t turns,
                       int64_t turn0, int32_t have_prev, int32_t write_prev, uint32_t birth, uint32_t survive,
                       const uint32_t *rules, int32_t scan, int64_t done, const int32_t *list, const int32_t *count,
                       int64_t slots, int64_t *left, const int64_t *born, void *stream);
/* The same launch under MAP rules ("MAP rules of a batch", above; no version
 * bump: probe by symbol): gol_dev_batch_step's arguments with maps and map_each
 * in place of birth, survive and rules.  map_each == 0: maps is uint32_t[16], the
 * map of every board; else uint32_t[16 n], board b under maps + 16 b.  Every mode
 * above is taken with the same meaning; the aged mode requires map_each == 0.
 * maps is only read.  GOL_EINVAL, nothing launched: as gol_dev_batch_step, and a
 * NULL maps. */
int gol_dev_batch_step_map(uint64_t *boards, uint64_t *prev, int64_t *settled, int64_t n, int64_t H, int64_t W, int32_t turns,
                           int64_t turn0, int32_t have_prev, int32_t write_prev, const uint32_t *maps, int32_t map_each,
                           int32_t scan, int64_t done, const int32_t *list, const int32_t *count, int64_t slots, int64_t *left,
                           const int64_t *born, void *stream);
/* One launch of the island census (gol_batch_islands, above, where islands,
 * records and fingerprints are defined) on caller device memory: boards as for
 * gol_dev_batch_step, only read; count int64_t[n]; islands n cap records (may be
 * NULL when cap == 0), board b's first min(count[b], cap) at islands + b cap, the
 * rest not touched; fingerprint uint64_t[n] or NULL.  Not checked: that the
 * pointers are device memory of the stated sizes.  GOL_EINVAL, nothing
 * launched: NULL boards or count, n, H, W out of range, reach outside 1..2, cap <
 * 0, or cap > 0 with NULL islands.  No version bump: probe by symbol. */
int gol_dev_batch_islands(const uint64_t *boards, int64_t n, int64_t H, int64_t W, int32_t reach, int64_t cap, int64_t *count,
                          gol_island *islands, uint64_t *fingerprint, void *stream);
/* One launch of the census in its TALLY form (the tally of island kinds, above)
 * on caller device memory: every island of the boards it visits goes into
 * `table` (2^table_log2 slots in the device layout, 4 <= table_log2 <= 24) under
 * its owner, and *dropped counts those a full table turned away.  The call adds
 * to the table and to *dropped; it clears neither (gol_dev_island_table_clear
 * sets a table to empty and *dropped to 0).  No record array is written.
 *  - pairs == NULL (pair_count, found NULL, max_pairs 0): dense.  Board i of n
 *    has the owner owner0 + i; count[i] and fingerprint[i] are written.
 *  - otherwise: listed.  pairs is the harvest list of gol_dev_batch_restock,
 *    (slot, soup) pairs, its length *pair_count in device memory; max_pairs (1 ..
 *    n) workgroups run and the first min(*pair_count, max_pairs) of them work.
 *    The board is slot `slot` of `boards` (the search's snapshots, which hold
 *    s(found)), the owner owner0 + soup, and count[soup], fingerprint[soup] are
 *    written.  A pair whose found[soup] < 0 (the soup expired) gets 0 and 0, its
 *    board is not read and nothing of it is tallied; a pair with a slot
 *    outside 0 .. n - 1 or a soup < 0 is passed over.  Entries of count and
 *    fingerprint that no pair names are not written.
 * fingerprint may be NULL.  Not checked: that the pointers are device memory
 * of the stated sizes (count, fingerprint and found hold every soup listed).
 * GOL_EINVAL, nothing launched: NULL boards, count, table or dropped, n, H, W out
 * of range, reach outside 1..2, table_log2 outside 4..24, owner0 outside 0..2^40,
 * a combination that is neither mode, max_pairs outside 1..n with pairs.  No
 * version bump: probe by symbol. */
int gol_dev_batch_islands_tally(const uint64_t *boards, int64_t n, int64_t H, int64_t W, int32_t reach, const int32_t *pairs,
                                const int32_t *pair_count, int64_t max_pairs, const int64_t *found, int64_t owner0,
                                int64_t *count, uint64_t *fingerprint, gol_island_kind *table, int32_t table_log2,
                                int64_t *dropped, void *stream);
int gol_dev_island_table_clear(gol_island_kind *table, int32_t table_log2, int64_t *dropped, void *stream);
/* The two launches above with the hash that symmetry selects ("island kinds
 * free of orientation", above): GOL_ISLAND_FIXED is the entry without _sym,
 * GOL_ISLAND_FREE writes free hashes and free fingerprints and tags the table
 * with free hashes.  Arguments, outputs and refusals as those entries', and
 * GOL_EINVAL, nothing launched, for a symmetry outside 0..1.  No version bump:
 * probe by symbol. */
int gol_dev_batch_islands_sym(const uint64_t *boards, int64_t n, int64_t H, int64_t W, int32_t reach, int32_t symmetry, int64_t cap,
                              int64_t *count, gol_island *islands, uint64_t *fingerprint, void *stream);
int gol_dev_batch_islands_tally_sym(const uint64_t *boards, int64_t n, int64_t H, int64_t W, int32_t reach, int32_t symmetry,
                                    const int32_t *pairs, const int32_t *pair_count, int64_t max_pairs, const int64_t *found,
                                    int64_t owner0, int64_t *count, uint64_t *fingerprint, gol_island_kind *table,
                                    int32_t table_log2, int64_t *dropped, void *stream);
/* Read and clear the error word of `device` (-1 = current) that the gol_dev_*
 * launchers' kernels report into (*flags = 0: no fault; nonzero: a pipeline
 * wave timed out waiting for its neighbour, so the launch's output is not
 * valid).  Synchronous; returns GOL_EHIP when *flags != 0. */
int gol_dev_error(int32_t device, uint32_t *flags);
/* ---------------------------------------------------------------- RPC service mirror
 * The broker's net/rpc service `Operations` (broker.go:62-277) and the
 * worker's `GameOfLifeOperations` (worker.go:77-86) with the gob field names
 * of stubs.go:13-38.  A Go drop-in registers these names and forwards here. */
typedef struct gol_request {     /* stubs.Request, stubs.go:20-29 */
    const uint8_t *World;        /* ImageHeight x ImageWidth bytes, row pitch world_stride */
    int64_t world_stride;
    int64_t Turns;
    int64_t ImageHeight;
    int64_t ImageWidth;
    int64_t Threads;
    int64_t EndY;
    int64_t StartY;
    int64_t Worker;
} gol_request;

typedef struct gol_response {    /* stubs.Response, stubs.go:31-38 */
    int32_t *Alive;              /* caller buffer for (X, Y) pairs (util.Cell, util/cell.go:4-5) */
    int64_t alive_cap;           /* capacity in pairs */
    int64_t alive_len;           /* out: len(Alive) (may exceed alive_cap: then truncated) */
    int64_t AliveCount;          /* out */
    int64_t TurnsCompleted;      /* out */
    uint8_t *World;              /* caller buffer, ImageHeight x ImageWidth, pitch world_stride */
    int64_t world_stride;
    uint8_t *WorkSlice;          /* caller buffer, (EndY-StartY) x width, pitch work_stride */
    int64_t work_stride;
    int64_t Worker;
} gol_response;

typedef struct gol_broker gol_broker;
int gol_broker_create(const gol_config *cfg, gol_broker **out);
void gol_broker_destroy(gol_broker *b);
int gol_broker_run(gol_broker *b, const gol_request *req, gol_response *res);      /* Operations.Run, broker.go:62-234 */
int gol_broker_retrieve(gol_broker *b, const gol_request *req, gol_response *res); /* Operations.RetrieveCurrentData, broker.go:256-277 */
int gol_broker_pause(gol_broker *b);                                              /* Operations.Pause, broker.go:251-254 */
int gol_broker_quit(gol_broker *b);                                               /* Operations.Quit, broker.go:236-239 */
int gol_broker_superquit(gol_broker *b);                                          /* Operations.SuperQuit, broker.go:241-249 */
int gol_broker_paused(gol_broker *b, int32_t *paused);
/* gol_engine_view of the broker's board, served between the chunks of a running
 * Run like RetrieveCurrentData; *turns_completed = cTurn (may be NULL).
 * GOL_ESTATE with no board.  No reference counterpart (the reference's live
 * view is the controller's SDL window): it shows the engine's board as it is,
 * so at turn 0 the loaded board -- deliberately not RetrieveCurrentData's
 * all-zero cWorld of broker.go:67-70. */
int gol_broker_view(gol_broker *b, int64_t x0, int64_t y0, int32_t scale, int32_t out_w, int32_t out_h,
                    uint8_t *pixels, int64_t stride, int64_t *turns_completed, int32_t *src_layout);
/* gol_engine_paste on the broker's board, served between the chunks of a running
 * Run like gol_broker_view; *turns_completed (may be NULL) = cTurn, the turn the
 * edit landed after.  GOL_ESTATE with no board.  No reference counterpart. */
int gol_broker_paste(gol_broker *b, int64_t x0, int64_t y0, int64_t w, int64_t h,
                     const uint64_t *pattern, int64_t stride, int32_t op,
                     int64_t *changed, int64_t *turns_completed);
/* gol_engine_copy and gol_engine_bounds of the broker's board, served between
 * the chunks of a running Run like gol_broker_view and gol_broker_paste;
 * *turns_completed (may be NULL) = cTurn, the turn the read saw (a cut lands
 * after it).  GOL_ESTATE with no board.  No reference counterpart. */
int gol_broker_copy(gol_broker *b, int64_t x0, int64_t y0, int64_t w, int64_t h, uint64_t *pattern,
                    int64_t stride, int32_t flags, int64_t *alive, int64_t *turns_completed);
int gol_broker_bounds(gol_broker *b, int64_t x0, int64_t y0, int64_t w, int64_t h, int64_t *bx, int64_t *by,
                      int64_t *bw, int64_t *bh, int64_t *alive, int64_t *turns_completed);
int gol_worker_update(const gol_request *req, gol_response *res);                 /* GameOfLifeOperations.Update, worker.go:77-80 */

#ifdef __cplusplus
}
#endif
#endif /* GOLHIP_H */
