// gol_launch.h -- the launch state the kernel units share (gol_launch.cpp; private, not part of the C
// ABI): the error word of a launch and its flags, the count slots, the CU slot masks, the paired
// ranks' claim counters, and what the units' launchers take from it -- the default error word, the
// strips of a pipelined launch, the device's CU count and the grid of a grid-stride launch.  No
// device code: host files include it too.  No launcher of any unit is declared here (each family
// of units has a header of its own), and the strip types are names alone: gol_strips.h is for the
// units that plan strips.  What a step launch must satisfy on any device is gol_step_launch_ok
// (gol_step_launch.h); pipe_plan adds the one thing that needs the device, a pretended device no
// larger than this one.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#ifndef GOL_COUNT_SLOTS
#define GOL_COUNT_SLOTS 256
#endif

// Flags of a launch's device error word (ORed by the failing waves).
#define GOLK_ERR_SPIN 1u  // a pipeline wave gave up waiting for an LDS flag (protocol fault)
#define GOLK_ERR_IPC 2u   // an IPC rank gave up waiting for a neighbour's flag (gol_comm.h)

// Per-device error word for launches made without one (lazily allocated, zeroed).
uint32_t *golk_device_err_word(int device);
// Per-device CU slot masks of the band pipeline's role placement (indexed by XCC, SE, SH, CU).
#define GOL_CU_SLOT_WORDS 2048
uint32_t *golk_cu_slots(int device);
// Zero them again on `s` (after a faulted launch whose workgroups may not have freed their slots).
hipError_t golk_reset_cu_slots(int device, hipStream_t s);
// Paired-rank claim counters (one buffer per launch stream; gol_strips.h StripMap).
// golk_reset_claims: zero the buffer of stream s, ordered on s (after a faulted launch).
// golk_release_claims: free it (the caller has synchronised s; an engine destroying its streams).
// golk_own_stream: mark s as an engine's stream; golk_reset_claims_device (gol_dev_error, after a
// fault in a launcher call on a caller's stream) then leaves its buffer alone.
hipError_t golk_reset_claims(hipStream_t s);
void golk_release_claims(hipStream_t s);
void golk_own_stream(hipStream_t s);
hipError_t golk_reset_claims_device(int device);

static inline int grid_for(int64_t n, int block = 256, int64_t cap = 256 * 16)
{
    int64_t g = (n + block - 1) / block;
    if (g < 1) g = 1;
    if (g > cap) g = cap;
    return (int)g;
}

namespace golk {
struct StripPlan;  // gol_strips.h
struct StripMap;
}

#pragma GCC visibility push(hidden)  // none of these is part of the library's exported symbols
// err, or this device's default error word (golk_device_err_word) without one.
uint32_t *err_or_default(uint32_t *err);
int device_cus();
// The strips of a pipelined launch: the device it is scheduled for (this one, or a pretended
// smaller one of as_cus CUs holding as_slots resident workgroups of `kernel`; false: this device
// has fewer of either), `plan`'s StripPlan for it (band_strip_plan / bytes_strip_plan) and, for a paired plan,
// the stream's claim counters.
typedef golk::StripPlan (*StripPlanFn)(int64_t, int64_t, int64_t, int, int, int, int64_t, bool);
bool pipe_plan(StripPlanFn plan, const void *kernel, int block, int64_t rows, int64_t width, int64_t pitch, int k,
               int strip_rows, int as_cus, int64_t as_slots, hipStream_t s, int32_t &strip, golk::StripMap &sm,
               unsigned &nwg);
#pragma GCC visibility pop
