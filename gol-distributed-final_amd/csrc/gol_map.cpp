// gol_map.cpp -- MAP rules on the host (include/golhip.h, "MAP rules of a batch"): the text codec (gol_map_parse,
// gol_map_format), the life-like rule as a map (gol_map_from_rule_host), the circuit of gol_map.h on nine planes
// (gol_map_eval_host), turns of one small torus with the row function the map kernel runs (gol_batch_step_map_host),
// and gol_batch_step_map_check_host: the check every launch of the map kernel passes (gol_batch_launch_ok).  No HIP
// header: a stand-alone program links this file (map_check.cpp).
#include <stdint.h>
#include <string.h>

#include <vector>

#include "gol_map.h"
#include "golhip.h"

int gol_set_error(int code, const char *fmt, ...);

namespace {

// "MAP" + the base64 of 64 bytes: 86 characters (the last one carries 2 bits), then nothing or "=="
const int MAP_CHARS = 86;

int b64_value(char c)
{
    if (c >= 'A' && c <= 'Z') return c - 'A';
    if (c >= 'a' && c <= 'z') return c - 'a' + 26;
    if (c >= '0' && c <= '9') return c - '0' + 52;
    return c == '+' ? 62 : (c == '/' ? 63 : -1);
}

const char B64[] = "ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz0123456789+/";

template <int NW>
void step_host(int64_t H, const gol_batch_row &g, const uint32_t *map, std::vector<uint32_t> &cells, std::vector<uint32_t> &next)
{
    for (int64_t y = 0; y < H; ++y) {
        uint32_t up[NW], c[NW], dn[NW], out[NW];
        for (int j = 0; j < NW; ++j) {
            up[j] = cells[(size_t)((y + H - 1) % H) * NW + j];
            c[j] = cells[(size_t)y * NW + j];
            dn[j] = cells[(size_t)((y + 1) % H) * NW + j];
        }
        gol_batch_map_next<NW>(map, g, up, c, dn, ~0u, out);
        for (int j = 0; j < NW; ++j) next[(size_t)y * NW + j] = out[j];
    }
    cells.swap(next);
}

}  // namespace

extern "C" int gol_map_from_rule_host(uint32_t birth, uint32_t survive, uint32_t *map)
{
    if (!map || birth >= 512 || survive >= 512)
        return gol_set_error(GOL_EINVAL, "bad map_from_rule arguments (B 0x%x, S 0x%x: masks are 9 bits, or NULL)", birth, survive);
    gol_map_from_rule(birth, survive, map);
    return GOL_OK;
}

extern "C" int gol_map_parse(const char *text, uint32_t *map)
{
    if (!text || !map) return gol_set_error(GOL_EINVAL, "bad map_parse arguments (NULL)");
    if (strncmp(text, "MAP", 3) != 0) {  // a life-like rule
        uint32_t birth = 0, survive = 0;
        const int rc = gol_rule_parse(text, &birth, &survive);
        if (rc) return rc;
        gol_map_from_rule(birth, survive, map);
        return GOL_OK;
    }
    const char *p = text + 3;
    const size_t len = strlen(p);
    if (len != (size_t)MAP_CHARS && !(len == (size_t)MAP_CHARS + 2 && p[MAP_CHARS] == '=' && p[MAP_CHARS + 1] == '='))
        return gol_set_error(GOL_EINVAL, "map \"%.20s...\": expected MAP and %d base64 characters (%d with ==), got %lld", text,
                             MAP_CHARS, MAP_CHARS + 2, (long long)len);
    uint8_t bytes[66] = {0};  // 86 characters are 516 bits: the last four must be zero
    for (int k = 0; k < MAP_CHARS; ++k) {
        const int v = b64_value(p[k]);
        if (v < 0) return gol_set_error(GOL_EINVAL, "map \"%.20s...\": character %d is not base64", text, k);
        for (int b = 0; b < 6; ++b)
            if (v >> (5 - b) & 1) bytes[(6 * k + b) >> 3] |= (uint8_t)(0x80 >> ((6 * k + b) & 7));
    }
    if (bytes[64]) return gol_set_error(GOL_EINVAL, "map \"%.20s...\": bits set after the 512th", text);
    uint32_t out[GOL_MAP_WORDS] = {0};
    for (uint32_t i = 0; i < 512; ++i)
        if (bytes[i >> 3] >> (7 - (i & 7)) & 1) out[i >> 5] |= 1u << (i & 31);
    memcpy(map, out, sizeof out);
    return GOL_OK;
}

extern "C" int gol_map_format(const uint32_t *map, char *buf, int64_t len)
{
    if (!map || !buf) return gol_set_error(GOL_EINVAL, "bad map_format arguments (NULL)");
    if (len < 3 + MAP_CHARS + 1)
        return gol_set_error(GOL_EINVAL, "map_format: the buffer holds %lld bytes, the text needs %d", (long long)len, 3 + MAP_CHARS + 1);
    memcpy(buf, "MAP", 3);
    for (int k = 0; k < MAP_CHARS; ++k) {
        int v = 0;
        for (int b = 0; b < 6; ++b) {
            const uint32_t i = (uint32_t)(6 * k + b);  // bit i of the table is bit 7 - (i & 7) of byte i >> 3: MSB first
            v = v << 1 | (int)(i < 512 ? gol_map_bit(map, i) : 0u);
        }
        buf[3 + k] = B64[v];
    }
    buf[3 + MAP_CHARS] = 0;
    return GOL_OK;
}

extern "C" int gol_map_eval_host(const uint32_t *map, const uint32_t x[9], uint32_t *next)
{
    if (!map || !x || !next) return gol_set_error(GOL_EINVAL, "bad map_eval_host arguments (NULL)");
    *next = gol_map_eval(map, x);
    return GOL_OK;
}

extern "C" int gol_batch_step_map_host(int64_t H, int64_t W, const uint32_t *map, const uint64_t *in, uint64_t *out, int64_t row_stride,
                                       int64_t turns)
{
    if (!gol_batch_shape_ok(1, H, W) || !map || !in || !out || row_stride < (W + 63) / 64 || turns < 0)
        return gol_set_error(GOL_EINVAL, "bad host batch map step (H %lld, W %lld, row stride %lld, turns %lld, or NULL)", (long long)H,
                             (long long)W, (long long)row_stride, (long long)turns);
    const gol_batch_row g = gol_batch_row_init(W);
    const int NW = g.nw;
    // every row's cells first (the padding of the input masked off): out may be in
    std::vector<uint32_t> cells((size_t)H * NW), next((size_t)H * NW);
    for (int64_t y = 0; y < H; ++y) gol_batch_unpack_row(g, in + y * row_stride, &cells[(size_t)y * NW]);
    for (int64_t t = 0; t < turns; ++t) switch (NW) {
        case 1: step_host<1>(H, g, map, cells, next); break;
        case 2: step_host<2>(H, g, map, cells, next); break;
        case 4: step_host<4>(H, g, map, cells, next); break;
        case 8: step_host<8>(H, g, map, cells, next); break;
        default: step_host<16>(H, g, map, cells, next); break;
        }
    for (int64_t y = 0; y < H; ++y) gol_batch_pack_row(g, &cells[(size_t)y * NW], out + y * row_stride);
    return GOL_OK;
}

extern "C" int gol_batch_step_map_check_host(const uint64_t *boards, const uint64_t *prev, const int64_t *settled, int64_t n, int64_t H,
                                             int64_t W, int32_t turns, int64_t turn0, int32_t have_prev, int32_t write_prev,
                                             const uint32_t *maps, int32_t map_each, int32_t scan, int64_t done, const int32_t *list,
                                             const int32_t *count, int64_t slots, const int64_t *left, const int64_t *born)
{
    // (the check reads the pointers' values alone)
    const gol_batch_launch l = {const_cast<uint64_t *>(boards), const_cast<uint64_t *>(prev), const_cast<int64_t *>(settled), n, H, W,
                                turns, turn0, have_prev != 0, write_prev != 0, 0, 0, nullptr, scan, done, list, count, slots,
                                const_cast<int64_t *>(left), born, maps, map_each != 0};
    return maps && gol_batch_launch_ok(l) ? GOL_OK : GOL_EINVAL;
}
