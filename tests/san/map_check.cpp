// Sanitizer driver for MAP rules on the host (gol_map.cpp: gol_batch_step_map_host, the row function of gol_map.h that
// the map kernel runs, and the text codec).  A stand-alone program: built only by `make asan` from gol_map.cpp with
// AddressSanitizer + UndefinedBehaviorSanitizer, linked without the GPU runtime, and run as a plain child process by
// tests/test_batch_map_cpu.py.  Every board is a heap block of its exact size -- (H - 1) * stride + ceil(W / 64) words
// -- so a read or write past a row is a sanitizer report.  Each shape runs 1, 2 and 3 turns under random maps and under
// maps that give birth on empty ground, from a random board whose padding bits are set, out of place and in place,
// against a table lookup cell by cell.  The codec reads malformed text from heap strings of exact size: short, long,
// bad characters, "MAP" alone.  And gol_batch_launch_ok (gol_batch.h) is asked what a launch with maps may carry.
// Exit status 0: all as expected; 1: a difference (printed).
#include "check_common.h"
#include "gol_map.h"

// (gol_map_parse hands a text without "MAP" to gol_rule_parse, which lives with the GPU entries; this program links
// without them, so the stand-in refuses: the B/S route is tested through the library)
extern "C" int gol_rule_parse(const char *, uint32_t *, uint32_t *) { return gol_set_error(GOL_EINVAL, "no rule parser here"); }

static int cell(const uint64_t *b, int64_t stride, int64_t y, int64_t x) { return (int)(b[y * stride + x / 64] >> (x % 64) & 1); }

// the next state of the H x W cells of `in` by the definition of golhip.h, as a block like `in` with the padding zero
static void naive(int64_t H, int64_t W, const uint32_t *map, const uint64_t *in, uint64_t *out, int64_t stride)
{
    const int64_t Ww = (W + 63) / 64;
    for (int64_t y = 0; y < H; ++y) {
        for (int64_t w = 0; w < Ww; ++w) out[y * stride + w] = 0;
        for (int64_t x = 0; x < W; ++x) {
            int i = 0;
            for (int dy = -1; dy <= 1; ++dy)
                for (int dx = -1; dx <= 1; ++dx) i = 2 * i + cell(in, stride, (y + dy + H) % H, (x + dx + W) % W);
            if (map[i >> 5] >> (i & 31) & 1u) out[y * stride + x / 64] |= (uint64_t)1 << (x % 64);
        }
    }
}

static int check(int64_t H, int64_t W, int64_t pad, const uint32_t *map, int turns, bool in_place)
{
    const int64_t Ww = (W + 63) / 64, stride = Ww + pad;
    const size_t words = (size_t)((H - 1) * stride + Ww);
    uint64_t *a = random_board(H, W, stride, 2), *b = new uint64_t[words], *want = new uint64_t[words], *tmp = new uint64_t[words];
    uint32_t *m = new uint32_t[GOL_MAP_WORDS];  // exact size, too
    memcpy(m, map, GOL_MAP_WORDS * sizeof(uint32_t));
    for (size_t i = 0; i < words; ++i) want[i] = tmp[i] = b[i] = GAP;
    for (int64_t y = 0; y < H; ++y)  // the input's cells, the padding masked, as turn 0
        for (int64_t w = 0; w < Ww; ++w) tmp[y * stride + w] = a[y * stride + w] & (w == Ww - 1 ? tail_of(W) : ~(uint64_t)0);
    for (int t = 0; t < turns; ++t) {
        naive(H, W, m, tmp, want, stride);
        memcpy(tmp, want, words * sizeof(uint64_t));
    }
    if (turns == 0) memcpy(want, tmp, words * sizeof(uint64_t));
    if (in_place) {  // the words between the rows are the input's, not the gap pattern
        memcpy(b, a, words * sizeof(uint64_t));
        for (int64_t y = 0; y + 1 < H; ++y)
            for (int64_t w = Ww; w < stride; ++w) want[y * stride + w] = a[y * stride + w];
    }
    const int rc = gol_batch_step_map_host(H, W, m, in_place ? b : a, b, stride, turns);
    const int bad = rc != GOL_OK || memcmp(b, want, words * sizeof(uint64_t));
    if (bad) printf("%lldx%lld stride %lld turns %d%s: rc %d, differs\n", (long long)H, (long long)W, (long long)stride, turns,
                    in_place ? " in place" : "", rc);
    delete[] a, delete[] b, delete[] want, delete[] tmp, delete[] m;
    return bad;
}

// gol_map_parse on a heap copy of `text` of its exact size
static int parse(const char *text, uint32_t *map)
{
    const size_t n = strlen(text) + 1;
    char *t = new char[n];
    memcpy(t, text, n);
    const int rc = gol_map_parse(t, map);
    delete[] t;
    return rc;
}

static int check_codec()
{
    int bad = 0;
    char buf[90], text[128];
    for (int k = 0; k < 20; ++k) {  // a round trip, with and without "=="
        uint32_t m[GOL_MAP_WORDS], back[GOL_MAP_WORDS];
        for (uint32_t &w : m) w = (uint32_t)rnd();
        bad += gol_map_format(m, buf, sizeof buf) != GOL_OK || strlen(buf) != 89 || memcmp(buf, "MAP", 3);
        bad += parse(buf, back) != GOL_OK || memcmp(m, back, sizeof m);
        snprintf(text, sizeof text, "%s==", buf);
        memset(back, 0, sizeof back);
        bad += parse(text, back) != GOL_OK || memcmp(m, back, sizeof m);
    }
    uint32_t zero[GOL_MAP_WORDS] = {0}, m[GOL_MAP_WORDS];
    bad += gol_map_format(zero, buf, sizeof buf) != GOL_OK;
    char good[90];
    memcpy(good, buf, sizeof good);  // "MAP" and 86 times 'A'
    struct {
        const char *what;
        char text[128];
    } cases[8] = {{"MAP alone", "MAP"}, {"empty", ""}, {"short", ""}, {"long", ""}, {"one =", ""}, {"a bad character", ""},
                  {"bits after the 512th", ""}, {"= inside", ""}};
    snprintf(cases[2].text, 128, "%.88s", good);
    snprintf(cases[3].text, 128, "%sA", good);
    snprintf(cases[4].text, 128, "%s=", good);
    snprintf(cases[5].text, 128, "%s", good), cases[5].text[40] = '*';
    snprintf(cases[6].text, 128, "%s", good), cases[6].text[88] = 'B';  // value 1: the last of the four spare bits
    snprintf(cases[7].text, 128, "%s", good), cases[7].text[50] = '=';
    for (const auto &c : cases) {
        for (uint32_t &w : m) w = 0x77777777u;
        const int rc = parse(c.text, m);
        bool touched = false;
        for (uint32_t w : m) touched = touched || w != 0x77777777u;
        if (rc != GOL_EINVAL || touched) {
            printf("codec: %s returned %d%s\n", c.what, rc, touched ? ", map written" : "");
            ++bad;
        }
    }
    char small[89];
    bad += gol_map_format(zero, small, sizeof small) != GOL_EINVAL || gol_map_format(nullptr, buf, sizeof buf) != GOL_EINVAL ||
           gol_map_format(zero, nullptr, 90) != GOL_EINVAL || gol_map_parse(nullptr, m) != GOL_EINVAL ||
           gol_map_parse(good, nullptr) != GOL_EINVAL;
    // bit i is bit 7 - (i & 7) of byte i >> 3: bit 0 alone is the first character 'g' (100000), bit 511 the last 'Q' (01 0000)
    uint32_t one[GOL_MAP_WORDS] = {1u};
    bad += gol_map_format(one, buf, sizeof buf) != GOL_OK || buf[3] != 'g' || buf[4] != 'A';
    uint32_t lastbit[GOL_MAP_WORDS] = {0};
    lastbit[15] = 0x80000000u;
    bad += gol_map_format(lastbit, buf, sizeof buf) != GOL_OK || buf[88] != 'Q' || buf[87] != 'A';
    return bad;
}

static int check_launch()
{
    uint64_t w[1];
    int64_t s[1];
    int32_t li[1];
    uint32_t m[GOL_MAP_WORDS], r[2];
    const gol_batch_launch plain = {w, nullptr, nullptr, 1, 5, 5, 3, 0, false, false, 0, 0, nullptr, GOL_BATCH_SCAN_NONE, 0, nullptr,
                                    nullptr, 0, nullptr, nullptr, m, false};
    gol_batch_launch aged = plain;
    aged.prev = w, aged.settled = s, aged.scan = GOL_BATCH_SCAN_CYCLES, aged.list = li, aged.count = li, aged.slots = 1, aged.born = s;
    aged.write_prev = true;
    int bad = !gol_batch_launch_ok(plain) || !gol_batch_launch_ok(aged);
    gol_batch_launch l = plain;
    l.map_each = true;
    bad += !gol_batch_launch_ok(l);
    l = plain, l.rules = r;
    bad += gol_batch_launch_ok(l);
    l = plain, l.birth = 8;
    bad += gol_batch_launch_ok(l);
    l = plain, l.survive = 12;
    bad += gol_batch_launch_ok(l);
    l = plain, l.maps = nullptr, l.map_each = true;
    bad += gol_batch_launch_ok(l);
    l = aged, l.map_each = true;
    bad += gol_batch_launch_ok(l);
    bad += gol_batch_step_map_check_host(w, nullptr, nullptr, 1, 5, 5, 3, 0, 0, 0, m, 0, 0, 0, nullptr, nullptr, 0, nullptr, nullptr) != GOL_OK;
    bad += gol_batch_step_map_check_host(w, nullptr, nullptr, 1, 5, 5, 3, 0, 0, 0, nullptr, 0, 0, 0, nullptr, nullptr, 0, nullptr, nullptr) !=
           GOL_EINVAL;
    bad += gol_batch_step_map_check_host(w, w, s, 1, 5, 5, 3, 0, 0, 1, m, 1, 2, 0, li, li, 1, nullptr, s) != GOL_EINVAL;
    if (bad) printf("launch check under maps: %d bad\n", bad);
    return bad;
}

int main()
{
    static const int shapes[][2] = {{1, 1}, {1, 2}, {2, 1}, {2, 2}, {3, 3}, {2, 5}, {5, 2}, {16, 16}, {7, 31}, {7, 32}, {7, 33}, {5, 63},
                                    {5, 64}, {5, 65}, {3, 96}, {4, 511}, {4, 512}, {3, 481}, {64, 1}, {65, 31}, {3, 129}, {2, 257}};
    int bad = 0, n = 0;
    for (const auto &s : shapes)
        for (int kind = 0; kind < 3; ++kind)
            for (int pad = 0; pad <= 2; pad += 2, ++n) {
                uint32_t map[GOL_MAP_WORDS];
                for (uint32_t &w : map) w = (uint32_t)rnd();
                map[0] = kind == 0 ? map[0] & ~1u : map[0] | 1u;  // kinds 1, 2: birth on empty ground
                if (kind == 2) gol_map_from_rule(0x001, 0x100, map);  // B0/S8
                bad += check(s[0], s[1], pad, map, 1 + n % 3, pad != 0);
            }
    uint32_t map[GOL_MAP_WORDS] = {0};
    bad += check(5, 70, 1, map, 0, false) + check(5, 70, 1, map, 0, true);  // no turn: the board, masked
    // the refusals write nothing
    uint64_t w[8] = {0};
    const int einval[] = {gol_batch_step_map_host(0, 8, map, w, w, 1, 1),   gol_batch_step_map_host(8, 0, map, w, w, 1, 1),
                          gol_batch_step_map_host(513, 8, map, w, w, 1, 1), gol_batch_step_map_host(8, 513, map, w, w, 9, 1),
                          gol_batch_step_map_host(8, 65, map, w, w, 1, 1),  gol_batch_step_map_host(8, 8, nullptr, w, w, 1, 1),
                          gol_batch_step_map_host(8, 8, map, nullptr, w, 1, 1), gol_batch_step_map_host(8, 8, map, w, nullptr, 1, 1),
                          gol_batch_step_map_host(8, 8, map, w, w, 1, -1)};
    for (int rc : einval)
        if (rc != GOL_EINVAL) {
            printf("a bad argument returned %d\n", rc);
            ++bad;
        }
    // the circuit on single-index planes: all 512, every plane all ones or all zeros
    uint32_t rmap[GOL_MAP_WORDS];
    for (uint32_t &v : rmap) v = (uint32_t)rnd();
    for (uint32_t i = 0; i < 512; ++i) {
        uint32_t *x = new uint32_t[9], next = 77;
        for (int k = 0; k < 9; ++k) x[k] = i >> (8 - k) & 1 ? ~0u : 0u;
        const int rc = gol_map_eval_host(rmap, x, &next);
        if (rc != GOL_OK || next != (gol_map_bit(rmap, i) ? ~0u : 0u)) ++bad;
        delete[] x;
    }
    bad += check_codec();
    bad += check_launch();
    printf("map_check: %d cases, %d bad\n", n, bad);
    return bad ? 1 : 0;
}
