// gol_util_kernels.h -- the launchers of gol_util.hip: the board utilities, the list kernels and the
// IPC transport's flag kernels; internal, not part of the C ABI.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

hipError_t golk_nonbinary(const uint8_t *bytes, int64_t rows, int64_t W, int64_t stride, uint32_t *flag, hipStream_t s);
hipError_t golk_random_fill(uint32_t *dst, int64_t rows, int64_t grow0, int64_t W, int64_t pitch, uint64_t seed,
                            hipStream_t s);
hipError_t golk_popcount(const uint32_t *src, int64_t rows, int64_t Wd, int64_t pitch, uint64_t *slots,
                         hipStream_t s);
// out[i] = sum of the GOL_COUNT_SLOTS slots of slot array i (arrays of GOL_COUNT_SLOTS*8 uint64;
// gol_launch.h); the slots are left zeroed.
hipError_t golk_slots_reduce(uint64_t *slots, int64_t n, uint64_t *out, hipStream_t s);
hipError_t golk_hash(const uint32_t *src, int64_t rows, int64_t grow0, int64_t Wd, int64_t pitch, uint64_t *slots,
                     hipStream_t s);
hipError_t golk_count_bytes(const uint8_t *src, int64_t rows, int64_t W, int64_t stride, uint64_t *slots,
                            hipStream_t s);
hipError_t golk_pack(const uint8_t *bytes, int64_t rows, int64_t W, int64_t stride, uint32_t *bits, int64_t pitch,
                     uint32_t *nonbinary, hipStream_t s);
hipError_t golk_unpack(const uint32_t *bits, int64_t rows, int64_t W, int64_t pitch, uint8_t *bytes, int64_t stride,
                       hipStream_t s);
// Per-row counts and the row-major (x, y) list of alive cells; with prev != NULL of the cells
// whose alive state differs between board and prev (same layout and pitch).  y0 is added to
// the listed y (global row of the first row).
hipError_t golk_row_counts(bool bits_mode, const void *board, const void *prev, int64_t rows, int64_t width_units,
                           int64_t pitch, int64_t *out, hipStream_t s);
hipError_t golk_alive_list(bool bits_mode, const void *board, const void *prev, int64_t rows, int64_t width_units,
                           int64_t pitch, const int64_t *offs, int32_t *xy, int64_t cap, int64_t y0, hipStream_t s);

// IPC transport (gol_comm.h): set *flag = value with release ordering at system scope after the
// stream's earlier work; wait (one wave on the stream) until every flags[i] (i < n <= 4, other
// processes' flag words mapped through IPC) has reached `want` (wrap-safe sequence compare),
// then acquire; after timeout_ticks of s_memrealtime (100 MHz) without it, OR GOLK_ERR_IPC
// (gol_launch.h) into err.
#define GOLK_IPC_MAX_WAIT 4
hipError_t golk_ipc_signal(uint32_t *flag, uint32_t value, hipStream_t s);
hipError_t golk_ipc_wait(const uint32_t *const *flags, int n, uint32_t want, uint64_t timeout_ticks, uint32_t *err,
                         hipStream_t s);
