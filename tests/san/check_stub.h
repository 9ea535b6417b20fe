// check_stub.h -- the error stub every stand-alone check program links its HIP-free host sources against: the
// library's gol_set_error, which here keeps the message and hands the code back.  A program includes it once
// (the census programs through check_common.h).
#pragma once
#include <stdarg.h>
#include <stdio.h>

static char g_msg[512];
int gol_set_error(int code, const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_msg, sizeof g_msg, fmt, ap);
    va_end(ap);
    return code;
}
