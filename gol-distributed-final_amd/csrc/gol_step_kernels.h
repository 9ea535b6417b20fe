// gol_step_kernels.h -- the launchers of the step kernels' units (gol_kernels.hip, gol_band_pipe.hip,
// gol_bytes_pipe.hip) and what gol_launch.cpp answers about them; internal, not part of the C ABI.
// The step kernels have one launcher that takes a descriptor, golk_step; the descriptor and its
// check are gol_step_launch.h, which a caller that fills one includes itself.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

struct gol_step_launch;

// One launch of a step kernel -- bits_step_kernel, band_step_kernel, their TableRule forms,
// bytes_blocked_kernel or one of the two split pipelines behind them -- of what the descriptor says
// (gol_step_launch.h, where the kernel table, every field and the check are).  hipErrorInvalidValue,
// nothing launched, unless gol_step_launch_ok accepts the descriptor and, for a pretended device
// (as_cus, as_slots), neither value exceeds this device's; hipSuccess at once for rows == 0.
hipError_t golk_step(const gol_step_launch &launch, hipStream_t s);
// This device's CU count and resident workgroups of a pipeline kernel (band: band_pipe_kernel with
// contiguous ghost rows or not; else bytes_pipe_kernel), with the fused count or not.
bool golk_pipe_limits(bool band, bool contig, bool count, int *cus, int64_t *slots);
// The pipeline kernels' host handles (gol_band_pipe.hip, gol_bytes_pipe.hip): for occupancy
// queries, and what the units' _launch launches (gol_step_device.h).
const void *golk_band_pipe_fn(bool contig, bool count);
const void *golk_bytes_pipe_fn(bool count);
// Rounds of resident workgroups a step launch of (family, k, dw) over `rows` rows makes (the band
// pipeline: 1 for its one-round rank-weighted launch; other kernels: 1e9, i.e. many); for the
// engine's choice of step plan.
double golk_step_rounds(int family, int64_t rows, int64_t Wd, int64_t pitch, int k, int dw, int strip);
// Standard <-> band rows (Wd % 32 == 0), out of place.
hipError_t golk_band_convert(bool to_band, const uint32_t *src, uint32_t *dst, int64_t rows, int64_t Wd,
                             int64_t spitch, int64_t dpitch, hipStream_t s);
hipError_t golk_bytes_step(const uint8_t *world, int64_t H, int64_t W, int64_t stride, int64_t y0, int64_t y1,
                           uint8_t *out, int64_t out_stride, hipStream_t s);
