// gol_launch.h -- what the kernel units' launchers take from the launch state (gol_launch.cpp;
// private): the default error word, the strips of a pipelined launch, the device's CU count and
// the grid of a grid-stride launch.  No device code: host files include it too.  What a step
// launch must satisfy on any device is gol_step_launch_ok (gol_step_launch.h); pipe_plan adds the
// one thing that needs the device, a pretended device no larger than this one.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gol_kernels.h"
#include "gol_strips.h"

static inline int grid_for(int64_t n, int block = 256, int64_t cap = 256 * 16)
{
    int64_t g = (n + block - 1) / block;
    if (g < 1) g = 1;
    if (g > cap) g = cap;
    return (int)g;
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
