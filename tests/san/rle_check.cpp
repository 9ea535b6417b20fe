// Sanitizer driver for the RLE codec (gol_rle.cpp) and the host paste function (gol_edit_host.cpp,
// the paste kernels' word function of gol_edit.h).  A stand-alone program: built only by `make asan`
// from those two sources with AddressSanitizer + UndefinedBehaviorSanitizer, linked without the GPU
// runtime, and run as a plain child process by tests/test_edit_cpu.py, which compares every verdict
// and every edited buffer with numpy.  Every input is copied into a heap block of its exact size,
// so a read or write past it is a sanitizer report.
//
// rle_check rle    stdin: records of uint32 n, n text bytes.
//                  stdout: one line per record "<rc> <w> <h> <round trip>": the parse verdict, and for
//                  a valid text whether parse(format(parse(text))) gives the same cells (1) or not (0).
// rle_check paste  stdin: records of 12 int64 (layout, W, pitch, buffer rows, row, rows, prow, x0, w,
//                  stride, op, pattern words; pattern words 0 = no pattern), the buffer, the pattern.
//                  stdout (binary): per record int64 rc, int64 changed, the buffer after the call.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "check_stub.h"
#include "golhip.h"

static bool read_exact(void *p, size_t n) { return n == 0 || fread(p, 1, n, stdin) == n; }

static int check_rle()
{
    uint32_t n;
    while (fread(&n, sizeof n, 1, stdin) == 1) {
        char *text = new char[n ? n : 1];
        if (!read_exact(text, n)) return 2;
        int64_t w = -1, h = -1;
        char rule[64];
        int rc = gol_rle_parse(text, n, &w, &h, nullptr, 0, 0, rule, sizeof rule);
        int same = 0;
        if (rc == GOL_OK) {
            const int64_t pw = (w + 63) / 64;
            uint64_t *pat = new uint64_t[h * pw];
            memset(pat, 0xA5, h * pw * sizeof(uint64_t));  // (parse must clear what it does not set)
            rc = gol_rle_parse(text, n, &w, &h, pat, pw, h, nullptr, 0);
            if (rc == GOL_OK) {
                int64_t need = 0;
                if (gol_rle_format(pat, pw, w, h, rule[0] ? rule : nullptr, nullptr, 0, &need) != GOL_OK) return 3;
                char *out = new char[need];
                if (gol_rle_format(pat, pw, w, h, rule[0] ? rule : nullptr, out, need, nullptr) != GOL_OK) return 3;
                if (need > 1 && gol_rle_format(pat, pw, w, h, nullptr, out, need - 1 > 8 ? 8 : need - 1, nullptr) != GOL_EINVAL) return 4;
                uint64_t *back = new uint64_t[h * pw];
                int64_t w2 = 0, h2 = 0;
                const int rc2 = gol_rle_parse(out, need - 1, &w2, &h2, back, pw, h, nullptr, 0);
                same = rc2 == GOL_OK && w2 == w && h2 == h;
                // (bits past w of a row's last word: parse leaves them 0 in both)
                same = same && memcmp(pat, back, h * pw * sizeof(uint64_t)) == 0;
                delete[] back;
                delete[] out;
            }
            delete[] pat;
        }
        delete[] text;
        printf("%d %lld %lld %d\n", rc, (long long)w, (long long)h, same);
    }
    return 0;
}

static int check_paste()
{
    int64_t a[12];
    while (fread(a, sizeof a, 1, stdin) == 1) {
        const int64_t layout = a[0], W = a[1], pitch = a[2], brows = a[3], row = a[4], rows = a[5], prow = a[6], x0 = a[7],
                      w = a[8], stride = a[9], op = a[10], pwords = a[11];
        const size_t bbytes = (size_t)(brows * pitch) * (layout == 0 ? 1 : 4);
        std::vector<uint8_t> in(bbytes ? bbytes : 1);
        if (!read_exact(in.data(), bbytes)) return 2;
        uint8_t *board = new uint8_t[bbytes ? bbytes : 1];
        memcpy(board, in.data(), bbytes);
        uint64_t *pat = nullptr;
        if (pwords) {
            pat = new uint64_t[pwords];
            if (!read_exact(pat, pwords * sizeof(uint64_t))) return 2;
        }
        int64_t changed = -1;
        const int64_t rc = gol_paste_host((int32_t)layout, board, pitch, W, row, rows, prow, x0, w, pat, stride, (int32_t)op,
                                          &changed);
        fwrite(&rc, sizeof rc, 1, stdout);
        fwrite(&changed, sizeof changed, 1, stdout);
        fwrite(board, 1, bbytes, stdout);
        delete[] pat;
        delete[] board;
    }
    return 0;
}

int main(int argc, char **argv)
{
    if (argc == 2 && !strcmp(argv[1], "rle")) return check_rle();
    if (argc == 2 && !strcmp(argv[1], "paste")) return check_paste();
    fprintf(stderr, "usage: rle_check rle|paste < records\n");
    return 64;
}
