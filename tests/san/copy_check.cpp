// Sanitizer driver for the host twins of the region reads (gol_copy_host.cpp: gol_copy_host and
// gol_bounds_host, the mapping of gol_copy.h that the copy and bounds kernels run).  A stand-alone
// program: built only by `make asan` from gol_copy_host.cpp and gol_edit_host.cpp with
// AddressSanitizer + UndefinedBehaviorSanitizer, linked without the GPU runtime, and run as a plain
// child process by tests/test_copy_cpu.py, which compares every result with numpy.  Every buffer is
// a heap block of its exact size, so a read or write past it is a sanitizer report.
//
// copy_check copy    stdin: records of 10 int64 (layout, W, pitch, buffer rows, row, rows, prow, x0,
//                    w, stride), then the buffer.  The pattern block holds exactly the words the call
//                    may write, (prow + rows - 1) * stride + ceil(w / 64), all ones before the call.
//                    stdout (binary): per record int64 rc, int64 alive, the pattern block, int64 rc
//                    of gol_paste_host(COPY) of that pattern at the same place, the buffer after it.
// copy_check bounds  stdin: records of 8 int64 (layout, W, pitch, buffer rows, row, rows, x0, w),
//                    then the buffer.  stdout (binary): per record int64 rc, cmin, cmax, rmin, rmax, alive.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "check_stub.h"
#include "golhip.h"

static bool read_exact(void *p, size_t n) { return n == 0 || fread(p, 1, n, stdin) == n; }

// The record's buffer in a heap block of its exact size (4-byte aligned at least, as operator new gives).
static uint8_t *read_board(int64_t layout, int64_t brows, int64_t pitch, size_t *bytes)
{
    *bytes = (size_t)(brows * pitch) * (layout == 0 ? 1 : 4);
    uint8_t *board = new uint8_t[*bytes ? *bytes : 1];
    if (!read_exact(board, *bytes)) {
        delete[] board;
        return nullptr;
    }
    return board;
}

static int check_copy()
{
    int64_t a[10];
    while (fread(a, sizeof a, 1, stdin) == 1) {
        const int64_t layout = a[0], W = a[1], pitch = a[2], brows = a[3], row = a[4], rows = a[5], prow = a[6], x0 = a[7],
                      w = a[8], stride = a[9];
        size_t bbytes;
        uint8_t *board = read_board(layout, brows, pitch, &bbytes);
        if (!board) return 2;
        const int64_t pwords = (prow + rows - 1) * stride + (w + 63) / 64;
        uint64_t *pat = new uint64_t[pwords];
        memset(pat, 0xff, pwords * sizeof(uint64_t));
        int64_t alive = -1, changed = -1;
        const int64_t rc = gol_copy_host((int32_t)layout, board, pitch, W, row, rows, prow, x0, w, pat, stride, &alive);
        const int64_t rc2 = gol_paste_host((int32_t)layout, board, pitch, W, row, rows, prow, x0, w, pat, stride, GOL_PASTE_COPY,
                                           &changed);
        fwrite(&rc, sizeof rc, 1, stdout);
        fwrite(&alive, sizeof alive, 1, stdout);
        fwrite(pat, sizeof(uint64_t), pwords, stdout);
        fwrite(&rc2, sizeof rc2, 1, stdout);
        fwrite(board, 1, bbytes, stdout);
        delete[] pat;
        delete[] board;
    }
    return 0;
}

static int check_bounds()
{
    int64_t a[8];
    while (fread(a, sizeof a, 1, stdin) == 1) {
        size_t bbytes;
        uint8_t *board = read_board(a[0], a[3], a[2], &bbytes);
        if (!board) return 2;
        int64_t out[6] = {0, -7, -7, -7, -7, -7};
        out[0] = gol_bounds_host((int32_t)a[0], board, a[2], a[1], a[4], a[5], a[6], a[7], &out[1], &out[2], &out[3], &out[4],
                                 &out[5]);
        fwrite(out, sizeof out, 1, stdout);
        delete[] board;
    }
    return 0;
}

int main(int argc, char **argv)
{
    if (argc == 2 && !strcmp(argv[1], "copy")) return check_copy();
    if (argc == 2 && !strcmp(argv[1], "bounds")) return check_bounds();
    fprintf(stderr, "usage: copy_check copy|bounds < records\n");
    return 64;
}
