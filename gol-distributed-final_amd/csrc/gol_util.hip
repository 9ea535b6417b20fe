// gol_util.hip -- the board utilities, untuned: random fill, popcount, slot reduce, hash, byte count,
// non-binary flag, pack / unpack, the alive-cell list and row-count kernels, the IPC flag kernels,
// each with its launcher.  gol_device.h: splitmix64, slot_add, the wave sums.
#include "gol_device.h"
#include "gol_launch.h"
#include "gol_util_kernels.h"

namespace golk {

// ------------------------------------------------------------------ board utilities
// Synthetic board: 64-bit word (y, w) = splitmix64(seed ^ (y*Ww + w)).
__global__ void random_fill_kernel(uint32_t *dst, int64_t rows, int64_t grow0, int64_t Ww, int64_t pitch,
                                   uint64_t seed)
{
    const int64_t n = rows * Ww;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t y = i / Ww, w = i % Ww;
        const uint64_t v = splitmix64(seed ^ (uint64_t)((grow0 + y) * Ww + w));
        *reinterpret_cast<uint2 *>(dst + y * pitch + 2 * w) = make_uint2((uint32_t)v, (uint32_t)(v >> 32));
    }
}

__global__ void popcount_kernel(const uint32_t *src, int64_t rows, int64_t Wd, int64_t pitch, uint64_t *slots)
{
    uint64_t c = 0;
    const int64_t n = rows * Wd;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t y = i / Wd, w = i % Wd;
        c += __popc(src[y * pitch + w]);
    }
    slot_add(slots, c);
}

// Sum the GOL_COUNT_SLOTS slots of `n` consecutive slot arrays into out[0..n) (one wave each).
__global__ void slots_reduce_kernel(uint64_t *slots, int64_t n, uint64_t *out)
{
    const int lane = threadIdx.x & 63;
    const int64_t i = blockIdx.x * (int64_t)(blockDim.x >> 6) + (threadIdx.x >> 6);
    if (i >= n) return;
    uint64_t s = 0;
    for (int j = lane; j < GOL_COUNT_SLOTS; j += 64) {
        uint64_t *p = &slots[(i * GOL_COUNT_SLOTS + j) * 8];
        s += *p;
        *p = 0;  // left zeroed: the next counted launch needs no memset (gol_engine.cpp slots_zero)
    }
    s = wave_sum_u64(s);
    if (lane == 0) out[i] = s;
}

__global__ void hash_kernel(const uint32_t *src, int64_t rows, int64_t grow0, int64_t Ww, int64_t pitch,
                            uint64_t *slots)
{
    uint64_t h = 0;
    const int64_t n = rows * Ww;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t y = i / Ww, w = i % Ww;
        const uint2 v = *reinterpret_cast<const uint2 *>(src + y * pitch + 2 * w);
        const uint64_t word = (uint64_t)v.x | ((uint64_t)v.y << 32);
        h += splitmix64(word ^ splitmix64((uint64_t)((grow0 + y) * Ww + w)));
    }
    slot_add(slots, h);
}

__global__ void count_nonzero_bytes_kernel(const uint8_t *src, int64_t rows, int64_t W, int64_t stride,
                                           uint64_t *slots)
{
    uint64_t c = 0;
    const int64_t n = rows * W;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t y = i / W, x = i % W;
        c += src[y * stride + x] != 0;
    }
    slot_add(slots, c);
}

// flag |= 1 if any byte of the rows x W board is neither 0 nor 255
__global__ void nonbinary_kernel(const uint8_t *bytes, int64_t rows, int64_t W, int64_t stride, uint32_t *flag)
{
    const int64_t n = rows * W;
    uint32_t bad = 0;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const uint8_t c = bytes[(i / W) * stride + i % W];
        bad |= (c != 0 && c != 255);
    }
    if (__ballot(bad) && (threadIdx.x & 63) == 0) atomicOr(flag, 1u);
}

// bytes -> bits: one thread per 32-cell word
__global__ void pack_kernel(const uint8_t *bytes, int64_t rows, int64_t W, int64_t stride, uint32_t *bits,
                            int64_t pitch, uint32_t *nonbinary)
{
    const int64_t Wd = W / 32;
    const int64_t n = rows * Wd;
    uint32_t bad = 0;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t y = i / Wd, w = i % Wd;
        const uint8_t *p = bytes + y * stride + 32 * w;
        uint32_t v = 0;
#pragma unroll 8
        for (int b = 0; b < 32; ++b) {
            const uint8_t c = p[b];
            v |= (uint32_t)(c == 255) << b;
            bad |= (c != 0 && c != 255);
        }
        bits[y * pitch + w] = v;
    }
    if (nonbinary && bad) atomicOr(nonbinary, 1u);
}

// bits -> bytes (0/255): one thread per 32-cell word, two 16-byte stores
__global__ void unpack_kernel(const uint32_t *bits, int64_t rows, int64_t W, int64_t pitch, uint8_t *bytes,
                              int64_t stride)
{
    const int64_t Wd = W / 32;
    const int64_t n = rows * Wd;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t y = i / Wd, w = i % Wd;
        const uint32_t v = bits[y * pitch + w];
        uint32_t o[8];
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            const uint32_t nib = (v >> (4 * q)) & 0xF;
            // spread 4 bits to 4 bytes, then 0x01 -> 0xFF
            const uint32_t s = (nib & 1) | ((nib & 2) << 7) | ((nib & 4) << 14) | ((nib & 8) << 21);
            o[q] = (s << 8) - s;
        }
        uint8_t *dst = bytes + y * stride + 32 * w;
        if (((uintptr_t)dst & 15) == 0) {
            reinterpret_cast<uint4 *>(dst)[0] = make_uint4(o[0], o[1], o[2], o[3]);
            reinterpret_cast<uint4 *>(dst)[1] = make_uint4(o[4], o[5], o[6], o[7]);
        } else {
            for (int q = 0; q < 8; ++q)
                for (int b = 0; b < 4; ++b) dst[4 * q + b] = (uint8_t)(o[q] >> (8 * b));
        }
    }
}

// Alive-cell list, row-major (broker.go:47-58): one wave per row, ballot + mbcnt prefix over
// 64 cells at a time.  offs[y] = first output index of row y.  With `prev` the listed cells
// are those that differ from `prev` (the CellFlipped events of one turn,
// gol/event.go:50-60): the same kernels over bits ^ prev.  y0 is the global row of row 0.
__global__ void alive_list_bits_kernel(const uint32_t *bits, const uint32_t *prev, int64_t rows, int64_t Wd,
                                       int64_t pitch, const int64_t *offs, int32_t *xy, int64_t cap, int64_t y0)
{
    const int lane = threadIdx.x & 63;
    const int64_t y = blockIdx.x * (int64_t)(blockDim.x >> 6) + (threadIdx.x >> 6);
    if (y >= rows) return;
    int64_t base = offs[y];
    for (int64_t w0 = 0; w0 < Wd; w0 += 64) {
        const int64_t w = w0 + lane;
        const uint32_t v = w < Wd ? bits[y * pitch + w] ^ (prev ? prev[y * pitch + w] : 0u) : 0u;
        const uint32_t c = __popc(v);
        // exclusive prefix of c over the wave
        uint32_t incl = c;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const uint32_t t = __shfl_up(incl, off, 64);
            if (lane >= off) incl += t;
        }
        int64_t o = base + (incl - c);
        uint32_t m = v;
        while (m) {
            const int b = __ffs(m) - 1;
            m &= m - 1;
            if (o < cap) { xy[2 * o] = (int32_t)(32 * w + b); xy[2 * o + 1] = (int32_t)(y0 + y); }
            ++o;
        }
        base += __shfl(incl, 63, 64);
    }
}

// bytes: a cell is alive when != 0 (broker.go:50-55); with `prev`, listed when its alive state
// differs from prev's.
__device__ __forceinline__ bool byte_listed(const uint8_t *bytes, const uint8_t *prev, int64_t i)
{
    return (bytes[i] != 0) != (prev ? prev[i] != 0 : false);
}

__global__ void alive_list_bytes_kernel(const uint8_t *bytes, const uint8_t *prev, int64_t rows, int64_t W,
                                        int64_t stride, const int64_t *offs, int32_t *xy, int64_t cap, int64_t y0)
{
    const int lane = threadIdx.x & 63;
    const int64_t y = blockIdx.x * (int64_t)(blockDim.x >> 6) + (threadIdx.x >> 6);
    if (y >= rows) return;
    int64_t base = offs[y];
    for (int64_t x0 = 0; x0 < W; x0 += 64) {
        const int64_t x = x0 + lane;
        const bool alive = x < W && byte_listed(bytes, prev, y * stride + x);
        const uint64_t m = __ballot(alive);
        if (alive) {
            const int64_t o = base + __popcll(m & ((1ULL << lane) - 1));
            if (o < cap) { xy[2 * o] = (int32_t)x; xy[2 * o + 1] = (int32_t)(y0 + y); }
        }
        base += __popcll(m);
    }
}

__global__ void row_counts_bits_kernel(const uint32_t *bits, const uint32_t *prev, int64_t rows, int64_t Wd,
                                       int64_t pitch, int64_t *out)
{
    const int lane = threadIdx.x & 63;
    const int64_t y = blockIdx.x * (int64_t)(blockDim.x >> 6) + (threadIdx.x >> 6);
    if (y >= rows) return;
    uint64_t c = 0;
    for (int64_t w = lane; w < Wd; w += 64) c += __popc(bits[y * pitch + w] ^ (prev ? prev[y * pitch + w] : 0u));
    c = wave_sum_u64(c);
    if (lane == 0) out[y] = (int64_t)c;
}

__global__ void row_counts_bytes_kernel(const uint8_t *bytes, const uint8_t *prev, int64_t rows, int64_t W,
                                        int64_t stride, int64_t *out)
{
    const int lane = threadIdx.x & 63;
    const int64_t y = blockIdx.x * (int64_t)(blockDim.x >> 6) + (threadIdx.x >> 6);
    if (y >= rows) return;
    uint64_t c = 0;
    for (int64_t x = lane; x < W; x += 64) c += byte_listed(bytes, prev, y * stride + x);
    c = wave_sum_u64(c);
    if (lane == 0) out[y] = (int64_t)c;
}

}  // namespace golk

// ------------------------------------------------------------------ IPC sequence flags
// The IPC halo transport (gol_ipc.cpp): a rank's flag words live in its own HBM and are polled by
// its ring neighbours' kernels through IPC mappings (other processes, the same or another GPU).
// Stream order puts a signal after the launches whose rows it announces (their end-of-kernel
// release has written them back), and the copy after the wait that acquired the flag.
__global__ void ipc_signal_kernel(uint32_t *flag, uint32_t value)
{
    if (threadIdx.x == 0) __hip_atomic_store(flag, value, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}

struct IpcWaitArgs {
    const uint32_t *f0, *f1, *f2, *f3;
    int32_t n;
    uint32_t want;
    uint64_t timeout;
    uint32_t *err;
};

// Lane i < n polls flag i (a bounded wait: every lane leaves, with or without the flag).
__global__ void ipc_wait_kernel(IpcWaitArgs a)
{
    const int lane = threadIdx.x;
    bool ok = true;
    if (lane < a.n) {
        const uint32_t *f = lane == 0 ? a.f0 : (lane == 1 ? a.f1 : (lane == 2 ? a.f2 : a.f3));
        const uint64_t t0 = __builtin_amdgcn_s_memrealtime();
        for (;;) {
            const uint32_t v = __hip_atomic_load(f, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_SYSTEM);
            if ((int32_t)(v - a.want) >= 0) break;
            if (__builtin_amdgcn_s_memrealtime() - t0 > a.timeout) {
                ok = false;
                break;
            }
            __builtin_amdgcn_s_sleep(8);
        }
    }
    if (!ok) atomicOr(a.err, GOLK_ERR_IPC);
}

// ------------------------------------------------------------------ launchers
using namespace golk;

hipError_t golk_nonbinary(const uint8_t *bytes, int64_t rows, int64_t W, int64_t stride, uint32_t *flag, hipStream_t s)
{
    if (rows <= 0) return hipSuccess;
    hipLaunchKernelGGL(nonbinary_kernel, dim3(grid_for(rows * W, 256, 256 * 16)), dim3(256), 0, s, bytes, rows, W, stride,
                       flag);
    return hipGetLastError();
}

hipError_t golk_random_fill(uint32_t *dst, int64_t rows, int64_t grow0, int64_t W, int64_t pitch, uint64_t seed,
                            hipStream_t s)
{
    const int64_t Ww = W / 64;
    if (rows <= 0) return hipSuccess;
    hipLaunchKernelGGL(random_fill_kernel, dim3(grid_for(rows * Ww, 256, 256 * 64)), dim3(256), 0, s, dst, rows,
                       grow0, Ww, pitch, seed);
    return hipGetLastError();
}

hipError_t golk_popcount(const uint32_t *src, int64_t rows, int64_t Wd, int64_t pitch, uint64_t *slots, hipStream_t s)
{
    hipLaunchKernelGGL(popcount_kernel, dim3(grid_for(rows * Wd, 256, 256 * 16)), dim3(256), 0, s, src, rows, Wd,
                       pitch, slots);
    return hipGetLastError();
}

hipError_t golk_slots_reduce(uint64_t *slots, int64_t n, uint64_t *out, hipStream_t s)
{
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(slots_reduce_kernel, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, s, slots, n, out);
    return hipGetLastError();
}

hipError_t golk_hash(const uint32_t *src, int64_t rows, int64_t grow0, int64_t Wd, int64_t pitch, uint64_t *slots,
                     hipStream_t s)
{
    hipLaunchKernelGGL(hash_kernel, dim3(grid_for(rows * (Wd / 2), 256, 256 * 16)), dim3(256), 0, s, src, rows,
                       grow0, Wd / 2, pitch, slots);
    return hipGetLastError();
}

hipError_t golk_count_bytes(const uint8_t *src, int64_t rows, int64_t W, int64_t stride, uint64_t *slots,
                            hipStream_t s)
{
    hipLaunchKernelGGL(count_nonzero_bytes_kernel, dim3(grid_for(rows * W, 256, 256 * 16)), dim3(256), 0, s, src,
                       rows, W, stride, slots);
    return hipGetLastError();
}

hipError_t golk_pack(const uint8_t *bytes, int64_t rows, int64_t W, int64_t stride, uint32_t *bits, int64_t pitch,
                     uint32_t *nonbinary, hipStream_t s)
{
    if (rows <= 0) return hipSuccess;
    hipLaunchKernelGGL(pack_kernel, dim3(grid_for(rows * (W / 32), 256, 256 * 64)), dim3(256), 0, s, bytes, rows, W,
                       stride, bits, pitch, nonbinary);
    return hipGetLastError();
}

hipError_t golk_unpack(const uint32_t *bits, int64_t rows, int64_t W, int64_t pitch, uint8_t *bytes, int64_t stride,
                       hipStream_t s)
{
    if (rows <= 0) return hipSuccess;
    hipLaunchKernelGGL(unpack_kernel, dim3(grid_for(rows * (W / 32), 256, 256 * 64)), dim3(256), 0, s, bits, rows, W,
                       pitch, bytes, stride);
    return hipGetLastError();
}

hipError_t golk_row_counts(bool bits_mode, const void *board, const void *prev, int64_t rows, int64_t width_units,
                           int64_t pitch, int64_t *out, hipStream_t s)
{
    const int wpb = 4;
    if (rows <= 0) return hipSuccess;
    dim3 grid((unsigned)((rows + wpb - 1) / wpb));
    if (bits_mode)
        hipLaunchKernelGGL(row_counts_bits_kernel, grid, dim3(64 * wpb), 0, s, (const uint32_t *)board,
                           (const uint32_t *)prev, rows, width_units, pitch, out);
    else
        hipLaunchKernelGGL(row_counts_bytes_kernel, grid, dim3(64 * wpb), 0, s, (const uint8_t *)board,
                           (const uint8_t *)prev, rows, width_units, pitch, out);
    return hipGetLastError();
}

hipError_t golk_alive_list(bool bits_mode, const void *board, const void *prev, int64_t rows, int64_t width_units,
                           int64_t pitch, const int64_t *offs, int32_t *xy, int64_t cap, int64_t y0, hipStream_t s)
{
    const int wpb = 4;
    if (rows <= 0) return hipSuccess;
    dim3 grid((unsigned)((rows + wpb - 1) / wpb));
    if (bits_mode)
        hipLaunchKernelGGL(alive_list_bits_kernel, grid, dim3(64 * wpb), 0, s, (const uint32_t *)board,
                           (const uint32_t *)prev, rows, width_units, pitch, offs, xy, cap, y0);
    else
        hipLaunchKernelGGL(alive_list_bytes_kernel, grid, dim3(64 * wpb), 0, s, (const uint8_t *)board,
                           (const uint8_t *)prev, rows, width_units, pitch, offs, xy, cap, y0);
    return hipGetLastError();
}

hipError_t golk_ipc_signal(uint32_t *flag, uint32_t value, hipStream_t s)
{
    hipLaunchKernelGGL(ipc_signal_kernel, dim3(1), dim3(64), 0, s, flag, value);
    return hipGetLastError();
}

hipError_t golk_ipc_wait(const uint32_t *const *flags, int n, uint32_t want, uint64_t timeout_ticks, uint32_t *err,
                         hipStream_t s)
{
    if (n <= 0) return hipSuccess;
    if (n > GOLK_IPC_MAX_WAIT || !err) return hipErrorInvalidValue;
    IpcWaitArgs a;
    a.f0 = flags[0];
    a.f1 = n > 1 ? flags[1] : flags[0];
    a.f2 = n > 2 ? flags[2] : flags[0];
    a.f3 = n > 3 ? flags[3] : flags[0];
    a.n = n;
    a.want = want;
    a.timeout = timeout_ticks;
    a.err = err;
    hipLaunchKernelGGL(ipc_wait_kernel, dim3(1), dim3(64), 0, s, a);
    return hipGetLastError();
}
