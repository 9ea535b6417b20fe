// Differential / sanitizer driver for the native PGM header parser (gol_pgm.cpp,
// gol_pgm_parse_header: gol/io.go:97-117 rules).  A stand-alone program: built only by
// `make -C gol-distributed-final_amd/csrc asan` from this file and gol_pgm.cpp with AddressSanitizer +
// UndefinedBehaviorSanitizer, linked without the GPU runtime, and run by
// tests/test_sanitizers_cpu.py, which compares every verdict with golhip.pgm.pgm_header.
//
// stdin: records of  int64 W, int64 H, uint32 n, n header bytes.
// stdout: one line per record: "<rc> <offset>" (offset -1 on error).
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "check_stub.h"
#include "golhip.h"

int gol_pgm_parse_header(const uint8_t *h, size_t n, int64_t W, int64_t H, int64_t *off);

int main()
{
    int64_t wh[2];
    uint32_t n;
    std::vector<uint8_t> buf;
    while (fread(wh, sizeof wh, 1, stdin) == 1 && fread(&n, sizeof n, 1, stdin) == 1) {
        buf.assign(n, 0);
        if (n && fread(buf.data(), 1, n, stdin) != n) return 2;
        // an exact-size heap copy, so a read past the header is an ASan report
        uint8_t *h = new uint8_t[n ? n : 1];
        memcpy(h, buf.data(), n);
        int64_t off = -1;
        const int rc = gol_pgm_parse_header(h, n, wh[0], wh[1], &off);
        delete[] h;
        printf("%d %lld\n", rc, (long long)(rc == GOL_OK ? off : -1));
    }
    return 0;
}
