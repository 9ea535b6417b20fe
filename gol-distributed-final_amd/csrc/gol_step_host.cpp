// gol_step_host.cpp -- gol_step_check_host: the check every launch of a step kernel passes
// (gol_step_launch_ok, gol_step_launch.h) and the geometry of the launch, as a C export.  No HIP.
#include "gol_step_launch.h"

extern "C" int gol_step_check_host(int32_t family, const void *top, const void *mid, const void *bot, const void *dst, int64_t R,
                                   int64_t width, int64_t pitch, int64_t row0, int64_t rows, int32_t k, int32_t words_per_lane,
                                   uint32_t birth, uint32_t survive, int32_t cus, int32_t slots, int32_t as_entry, int32_t *geometry)
{
    // (the check reads the pointers' values alone)
    const gol_step_launch l = {family, top, mid, bot, const_cast<void *>(dst), R, width, pitch, row0, rows, k, words_per_lane,
                               0, birth, survive, nullptr, nullptr, cus, slots};
    if (!gol_step_launch_ok(l, as_entry != 0)) return GOL_EINVAL;
    if (geometry) {
        const gol_step_geometry g = gol_step_geometry_of(l);
        geometry[0] = g.useful;
        geometry[1] = g.ngroups;
        geometry[2] = g.contig;
        geometry[3] = g.pipelined;
    }
    return GOL_OK;
}
