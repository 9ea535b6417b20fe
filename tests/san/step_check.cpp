// step_check.cpp -- stand-alone driver of the step launches' check (gol_step_launch.h) and its
// export (gol_step_host.cpp), for the sanitizer build: plain C++, no GPU runtime.
//
// `step_check launch FILE`: a line per launch, the expected answer (1 accepted, 0 refused) and the
// 17 arguments of gol_step_check_host without the geometry, a pointer as an integer (0: NULL)
// that is never dereferenced.  Every line goes through gol_step_launch_ok and through the export,
// which must give the one answer; an accepted launch's geometry must be that of
// gol_step_geometry_of.  Prints `step_check launch: N accepted, M refused, 0 bad`.
#include <stdio.h>
#include <string.h>

#include "gol_step_launch.h"

static int main_launch(const char *path)
{
    FILE *f = fopen(path, "r");
    if (!f) {
        printf("step_check launch: cannot read %s\n", path);
        return 2;
    }
    int bad = 0, n[2] = {0, 0};
    long long v[18];
    for (;;) {
        int got = 0;
        while (got < 18 && fscanf(f, "%lld", &v[got]) == 1) ++got;
        if (got == 0) break;
        if (got < 18 || (v[0] != 0 && v[0] != 1)) {
            printf("launch line %d: %d fields\n", n[0] + n[1] + 1, got);
            ++bad;
            break;
        }
        const gol_step_launch l = {(int32_t)v[1], (const void *)(uintptr_t)v[2], (const void *)(uintptr_t)v[3], (const void *)(uintptr_t)v[4],
                                   (void *)(uintptr_t)v[5], v[6], v[7], v[8], v[9], v[10], (int32_t)v[11], (int32_t)v[12], 0,
                                   (uint32_t)v[13], (uint32_t)v[14], nullptr, nullptr, (int32_t)v[15], v[16]};
        const bool entry = v[17] != 0;
        int32_t geo[4] = {-1, -1, -1, -1};
        const int rc = gol_step_check_host(l.family, l.top, l.mid, l.bot, l.dst, l.R, l.width, l.pitch, l.row0, l.rows, l.k, l.dw,
                                           l.birth, l.survive, l.as_cus, (int32_t)l.as_slots, entry, geo);
        bool ok = gol_step_launch_ok(l, entry) == (v[0] == 1) && rc == (v[0] == 1 ? GOL_OK : GOL_EINVAL);
        if (ok && v[0] == 1) {
            const gol_step_geometry g = gol_step_geometry_of(l);
            ok = geo[0] == g.useful && geo[1] == g.ngroups && geo[2] == (int)g.contig && geo[3] == (int)g.pipelined;
        } else if (ok) {
            ok = geo[0] == -1 && geo[3] == -1;  // a refusal writes nothing
        }
        if (!ok) {
            printf("launch line %d: expected %lld, rc %d\n", n[0] + n[1] + 1, v[0], rc);
            ++bad;
        }
        ++n[v[0]];
    }
    fclose(f);
    printf("step_check launch: %d accepted, %d refused, %d bad\n", n[1], n[0], bad);
    return bad || !n[0] || !n[1] ? 1 : 0;
}

int main(int argc, char **argv)
{
    if (argc > 2 && !strcmp(argv[1], "launch")) return main_launch(argv[2]);
    printf("usage: step_check launch FILE\n");
    return 2;
}
