// gol_launch.cpp -- the launch state of the kernel units, as host code: the per-device words (error
// word, CU slot masks), the paired ranks' claim counters per stream with their recovery after a
// faulted launch, the resident-workgroup cache and the strips of a pipelined launch (gol_strips.h),
// and the rounds of a launch the engine asks for.  A kernel is an opaque handle here (const void *).
#include <algorithm>
#include <map>
#include <mutex>
#include <set>
#include <utility>

#include "gol_launch.h"
#include "gol_step_kernels.h"
#include "gol_step_launch.h"

using namespace golk;

// A per-device buffer of `words` zeroed words, allocated at its first use and kept in `bufs`.
// Zeroed and synchronised: launches on non-blocking streams are not ordered after the null stream.
static uint32_t *device_words(std::map<int, uint32_t *> &bufs, int device, size_t words)
{
    static std::mutex mu;
    std::lock_guard<std::mutex> lock(mu);
    auto it = bufs.find(device);
    if (it != bufs.end()) return it->second;
    int prev = 0;
    uint32_t *w = nullptr;
    if (hipGetDevice(&prev) != hipSuccess || hipSetDevice(device) != hipSuccess) return nullptr;
    if (hipMalloc(&w, words * sizeof(uint32_t)) != hipSuccess || hipMemset(w, 0, words * sizeof(uint32_t)) != hipSuccess ||
        hipDeviceSynchronize() != hipSuccess)
        w = nullptr;
    (void)hipSetDevice(prev);
    if (w) bufs[device] = w;
    return w;
}

// Per-device error word used when a launcher is called without one (gol_dev_* launchers).
uint32_t *golk_device_err_word(int device)
{
    static std::map<int, uint32_t *> words;
    return device_words(words, device, 1);
}

// Per-device CU slot masks of the band pipeline (GOL_BAND_PLACE; zeroed once, every workgroup
// frees its slot on exit).
uint32_t *golk_cu_slots(int device)
{
    static std::map<int, uint32_t *> tabs;
    return device_words(tabs, device, GOL_CU_SLOT_WORDS);
}

hipError_t golk_reset_cu_slots(int device, hipStream_t s)
{
    uint32_t *w = golk_cu_slots(device);
    return w ? hipMemsetAsync(w, 0, GOL_CU_SLOT_WORDS * sizeof(uint32_t), s) : hipErrorOutOfMemory;
}

uint32_t *err_or_default(uint32_t *err)
{
    if (err) return err;
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return nullptr;
    return golk_device_err_word(dev);
}

// Workgroups of `kernel` (block threads) resident on the whole device at once (cached).
static int64_t resident_workgroups(const void *kernel, int block)
{
    static std::mutex mu;
    static std::map<std::pair<const void *, int>, int64_t> cache;
    int dev = 0, cus = 0, per_cu = 0;
    if (hipGetDevice(&dev) != hipSuccess) return 0;
    std::lock_guard<std::mutex> lock(mu);
    auto it = cache.find({kernel, dev});
    if (it != cache.end()) return it->second;
    int64_t n = 0;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess &&
        hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel, block, 0) == hipSuccess)
        n = (int64_t)cus * per_cu;
    cache[{kernel, dev}] = n;
    return n;
}

int device_cus()
{
    int dev = 0, cus = 0;
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess)
        return 0;
    return cus;
}

// Claim counters of the paired ranks (StripMap), one zeroed buffer per stream: launches on one
// stream run in order and leave their counters zeroed; launches on different streams may run
// at once and must not share counters.  The buffer is zeroed ON that stream (stream-ordered
// before the launch that asks for it): a null-stream hipMemset is not ordered before work on a
// non-blocking stream, and a first launch that raced it counted rows twice (overlapping claims;
// tests/test_gpu_engine.py::test_band_paired_narrow_board).  A launch that faults (a pipeline
// wave timed out) can leave counters set: golk_reset_claims zeroes a device's buffers again.
static std::mutex claims_mu;
static std::map<std::pair<hipStream_t, int>, uint32_t *> claims_bufs;
static size_t claims_bytes(int cus) { return (size_t)cus * 2 * 16 * sizeof(uint32_t); }
static uint32_t *claim_counters(hipStream_t s, int cus)
{
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return nullptr;
    std::lock_guard<std::mutex> lock(claims_mu);
    auto it = claims_bufs.find({s, dev});
    if (it != claims_bufs.end()) return it->second;
    uint32_t *c = nullptr;
    if (hipMalloc(&c, claims_bytes(cus)) != hipSuccess) return nullptr;
    if (hipMemsetAsync(c, 0, claims_bytes(cus), s) != hipSuccess) {
        (void)hipFree(c);
        return nullptr;
    }
    claims_bufs[{s, dev}] = c;
    return c;
}

static std::set<hipStream_t> engine_streams;  // streams owned by an engine (golk_own_stream)

hipError_t golk_reset_claims(hipStream_t s)
{
    std::lock_guard<std::mutex> lock(claims_mu);
    hipError_t e = hipSuccess;
    for (auto &kv : claims_bufs) {
        if (kv.first.first != s) continue;
        int cus = 0;
        e = hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, kv.first.second);
        if (e == hipSuccess) e = hipMemsetAsync(kv.second, 0, claims_bytes(cus), s);  // before any later launch on s
        if (e != hipSuccess) break;
    }
    return e;
}

void golk_release_claims(hipStream_t s)
{
    std::lock_guard<std::mutex> lock(claims_mu);
    for (auto it = claims_bufs.begin(); it != claims_bufs.end();) {
        if (it->first.first == s) {
            (void)hipFree(it->second);
            it = claims_bufs.erase(it);
        } else {
            ++it;
        }
    }
    engine_streams.erase(s);
}

void golk_own_stream(hipStream_t s)
{
    std::lock_guard<std::mutex> lock(claims_mu);
    engine_streams.insert(s);
}

hipError_t golk_reset_claims_device(int device)
{
    // Synchronous, on the null stream between two device-wide synchronisations: a caller's stream
    // that owns a buffer here may have been destroyed since (its handle is not used), and the
    // second synchronisation orders the zeroing before any later launch on a non-blocking stream.
    std::lock_guard<std::mutex> lock(claims_mu);
    int cus = 0, prev = 0;
    hipError_t e = hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device);
    if (e == hipSuccess) e = hipGetDevice(&prev);
    if (e == hipSuccess) e = hipSetDevice(device);
    if (e != hipSuccess) return e;
    e = hipDeviceSynchronize();
    for (auto &kv : claims_bufs) {
        if (e != hipSuccess) break;
        if (kv.first.second != device || engine_streams.count(kv.first.first)) continue;
        e = hipMemset(kv.second, 0, claims_bytes(cus));
    }
    if (e == hipSuccess) {
        uint32_t *w = golk_cu_slots(device);  // (placement only: a timed-out workgroup kept its slot)
        if (w) e = hipMemset(w, 0, GOL_CU_SLOT_WORDS * sizeof(uint32_t));
    }
    if (e == hipSuccess) e = hipDeviceSynchronize();
    (void)hipSetDevice(prev);
    return e;
}

// The device a pipelined launch is scheduled for: this one (as_cus = as_slots = 0), or a
// pretended smaller one of as_cus CUs holding as_slots resident workgroups of `kernel` (what the
// two must be on any device: gol_step_launch_ok); false: it asks for more than this device has,
// which is checked here and nowhere else.
static bool pipe_device(const void *kernel, int block, int as_cus, int64_t as_slots, int &cus, int64_t &slots)
{
    cus = device_cus();
    slots = resident_workgroups(kernel, block);
    if (!as_cus && !as_slots) return true;
    if (as_cus > cus || as_slots > slots) return false;
    cus = as_cus;
    slots = as_slots;
    return true;
}

// The strips of a pipelined launch: the device it is scheduled for (pipe_device; false: no such
// device), `plan`'s StripPlan for it (band_strip_plan / bytes_strip_plan) and, for a paired plan,
// the stream's claim counters -- sized by the device itself, whichever device the launch is
// scheduled for; without them the plan is made again unpaired.
bool pipe_plan(StripPlanFn plan, const void *kernel, int block, int64_t rows, int64_t width, int64_t pitch, int k,
               int strip_rows, int as_cus, int64_t as_slots, hipStream_t s, int32_t &strip, StripMap &sm,
               unsigned &nwg)
{
    int cus = 0;
    int64_t resident = 0;
    if (!pipe_device(kernel, block, as_cus, as_slots, cus, resident)) return false;
    StripPlan p = plan(rows, width, pitch, k, strip_rows, cus, resident, true);
    uint32_t *claims = p.mode == GOL_STRIPS_RANKED_PAIRED ? claim_counters(s, device_cus()) : nullptr;
    if (p.mode == GOL_STRIPS_RANKED_PAIRED && !claims) p = plan(rows, width, pitch, k, strip_rows, cus, resident, false);
    strip = p.strip;
    sm = p.sm;
    sm.claims = claims;
    nwg = (unsigned)p.nwg;
    return true;
}

bool golk_pipe_limits(bool band, bool contig, bool count, int *cus, int64_t *slots)
{
    *cus = device_cus();
    *slots = band ? resident_workgroups(golk_band_pipe_fn(contig, count), 64 * GOL_BAND_P)
                  : resident_workgroups(golk_bytes_pipe_fn(count), 64 * GOL_BYTES_PIPE_P);
    return *cus > 0 && *slots > 0;
}

double golk_step_rounds(int family, int64_t rows, int64_t Wd, int64_t pitch, int k, int dw, int strip)
{
    if (family != GOL_FAMILY_BAND || !gol_step_kernel_of(family, k, dw).pipelined || rows <= 0) return 1e9;
    const int64_t slots = resident_workgroups(golk_band_pipe_fn(true, true), 64 * GOL_BAND_P);
    if (slots <= 0) return 1e9;
    const StripPlan p = band_strip_plan(rows, Wd, pitch, k, strip, device_cus(), slots);  // the launch's own plan
    return p.sm.ranked ? 1.0 : (double)p.nwg / (double)slots;
}
