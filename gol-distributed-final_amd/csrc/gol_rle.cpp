// gol_rle.cpp -- the RLE pattern codec (include/golhip.h, gol_rle_parse / gol_rle_format): the
// text form Life patterns are exchanged in, "x = 3, y = 3, rule = B3/S23\nbob$2bo$3o!".  Two-state
// patterns only.  Host code with no HIP header: a stand-alone program links this file alone
// (rle_check.cpp runs it under the sanitizers).
#include <stdint.h>
#include <string.h>

#include <string>

#include "golhip.h"

int gol_set_error(int code, const char *fmt, ...);

namespace {

constexpr int64_t RLE_MAX_CELLS = int64_t(1) << 26;
constexpr size_t RLE_LINE = 70;  // characters per body line at most

bool blank(char c) { return c == ' ' || c == '\t' || c == '\r' || c == '\v' || c == '\f'; }

struct Reader {
    const char *s;
    int64_t n, i = 0;
    bool end() const { return i >= n; }
    char at() const { return s[i]; }
    void skip_blank()
    {
        while (i < n && blank(s[i])) ++i;
    }
    void skip_line()
    {
        while (i < n && s[i] != '\n') ++i;
        if (i < n) ++i;
    }
    bool take(char c)
    {
        skip_blank();
        if (i < n && s[i] == c) {
            ++i;
            return true;
        }
        return false;
    }
    // a decimal number of at most `cap` (-1: none here, -2: larger than cap)
    int64_t number(int64_t cap)
    {
        if (i >= n || s[i] < '0' || s[i] > '9') return -1;
        int64_t v = 0;
        bool over = false;
        for (; i < n && s[i] >= '0' && s[i] <= '9'; ++i) {
            if (!over) v = v * 10 + (s[i] - '0');
            if (v > cap) over = true;
        }
        return over ? -2 : v;
    }
};

int bad(int64_t off, const char *what) { return gol_set_error(GOL_EFORMAT, "RLE: %s at offset %lld", what, (long long)off); }

// "<key> = <number>" with free blanks; the key in either case
int header_field(Reader &r, char key, int64_t *v)
{
    r.skip_blank();
    if (r.end() || (r.at() | 0x20) != key) return bad(r.i, key == 'x' ? "no header (x = ...)" : "no y in the header");
    ++r.i;
    if (!r.take('=')) return bad(r.i, "no '=' in the header");
    r.skip_blank();
    const int64_t at = r.i;
    *v = r.number(RLE_MAX_CELLS);
    if (*v == -1) return bad(at, "no number in the header");
    if (*v == -2) return bad(at, "x * y is more than 2^26 cells");
    if (*v < 1) return bad(at, "x and y must be at least 1");
    return GOL_OK;
}

}  // namespace

extern "C" int gol_rle_parse(const char *text, int64_t len, int64_t *w, int64_t *h, uint64_t *pattern, int64_t stride,
                             int64_t cap_rows, char *rule, int64_t rule_len)
{
    if (!text || len < 0 || !w || !h || (rule && rule_len < 1)) return gol_set_error(GOL_EINVAL, "bad RLE parse arguments");
    Reader r{text, len};
    // comment lines and blank lines before the header
    for (;;) {
        r.skip_blank();
        if (!r.end() && (r.at() == '#' || r.at() == '\n')) r.skip_line();
        else break;
    }
    int64_t x = 0, y = 0;
    int rc = header_field(r, 'x', &x);
    if (rc) return rc;
    if (!r.take(',')) return bad(r.i, "no ',' after x in the header");
    rc = header_field(r, 'y', &y);
    if (rc) return rc;
    if (x * y > RLE_MAX_CELLS) return bad(r.i, "x * y is more than 2^26 cells");
    int64_t rule0 = 0, rule1 = 0;  // the rule text: [rule0, rule1)
    if (r.take(',')) {
        r.skip_blank();
        const char *key = "rule";
        for (int k = 0; k < 4; ++k, ++r.i)
            if (r.end() || (r.at() | 0x20) != key[k]) return bad(r.i, "the header's third field is not a rule");
        if (!r.take('=')) return bad(r.i, "no '=' in the header");
        r.skip_blank();
        rule0 = r.i;
        while (!r.end() && r.at() != '\n') ++r.i;
        rule1 = r.i;
        while (rule1 > rule0 && blank(text[rule1 - 1])) --rule1;
    }
    r.skip_blank();
    if (!r.end() && r.at() != '\n') return bad(r.i, "text after the header");
    if (rule) {
        if (rule1 - rule0 + 1 > rule_len) return gol_set_error(GOL_EINVAL, "RLE: the rule buffer is too small (%lld bytes needed)", (long long)(rule1 - rule0 + 1));
        memcpy(rule, text + rule0, (size_t)(rule1 - rule0));
        rule[rule1 - rule0] = 0;
    }
    const int64_t pw = (x + 63) / 64;
    if (pattern) {
        if (stride < pw || cap_rows < y)
            return gol_set_error(GOL_EINVAL, "RLE: a %lld x %lld pattern needs stride >= %lld and %lld rows", (long long)x,
                                 (long long)y, (long long)pw, (long long)y);
        for (int64_t j = 0; j < y; ++j) memset(pattern + j * stride, 0, (size_t)pw * sizeof(uint64_t));
    }
    // the body
    int64_t col = 0, row = 0;
    bool line_start = true, done = false;
    if (!r.end()) ++r.i;  // the header's newline
    while (!r.end() && !done) {
        const char c = r.at();
        if (c == '\n') {
            line_start = true;
            ++r.i;
            continue;
        }
        if (blank(c)) {
            ++r.i;
            continue;
        }
        if (c == '#' && line_start) {
            r.skip_line();
            continue;
        }
        line_start = false;
        const int64_t at = r.i;
        int64_t count = r.number(RLE_MAX_CELLS);
        if (count == -2) return bad(at, "a count overflows");
        if (count == 0) return bad(at, "a count of 0");
        const bool counted = count > 0;
        if (!counted) count = 1;
        else
            while (!r.end() && (blank(r.at()) || r.at() == '\n')) ++r.i;  // (a line break between a count and its tag)
        if (r.end()) break;
        const char tag = r.at();
        if (tag == 'b' || tag == 'o') {
            if (row >= y) return bad(at, "rows past y");
            if (count > x - col) return bad(at, "a run past x");
            if (tag == 'o' && pattern)
                for (int64_t cc = col; cc < col + count; ++cc) pattern[row * stride + (cc >> 6)] |= uint64_t(1) << (cc & 63);
            col += count;
        } else if (tag == '$') {
            if (count > y - row) return bad(at, "rows past y");
            row += count;  // <= y: a '$' that closes the last row is accepted, cells after it are not
            col = 0;
        } else if (tag == '!') {
            if (counted) return bad(at, "a count before '!'");
            done = true;
        } else {
            return bad(r.i, "not a two-state RLE body character (b, o, $, !)");
        }
        ++r.i;
    }
    if (!done) return bad(r.i, "no '!' at the end of the pattern");
    *w = x;
    *h = y;
    return GOL_OK;
}

extern "C" int gol_rle_format(const uint64_t *pattern, int64_t stride, int64_t w, int64_t h, const char *rule, char *buf,
                              int64_t len, int64_t *need)
{
    if (!pattern || w < 1 || h < 1 || w > RLE_MAX_CELLS / h || stride < (w + 63) / 64 || len < 0 || (!buf && !need) ||
        (rule && strpbrk(rule, "\r\n")))
        return gol_set_error(GOL_EINVAL, "bad RLE format arguments");
    std::string out = "x = " + std::to_string(w) + ", y = " + std::to_string(h);
    if (rule) out += std::string(", rule = ") + rule;
    out += '\n';
    size_t line = 0;  // characters on the current body line
    auto emit = [&](int64_t count, char tag) {
        const std::string tok = (count > 1 ? std::to_string(count) : std::string()) + tag;
        if (line + tok.size() > RLE_LINE) {
            out += '\n';
            line = 0;
        }
        out += tok;
        line += tok.size();
    };
    int64_t pending = 0;  // row ends not yet written: empty rows merge into one n$
    for (int64_t j = 0; j < h; ++j) {
        const uint64_t *row = pattern + j * stride;
        int64_t last = -1;  // the last alive cell: trailing dead cells are dropped
        for (int64_t c = w - 1; c >= 0 && last < 0; --c)
            if ((row[c >> 6] >> (c & 63)) & 1) last = c;
        if (last >= 0) {
            if (pending) emit(pending, '$');
            pending = 0;
            for (int64_t c = 0; c <= last;) {
                const uint64_t v = (row[c >> 6] >> (c & 63)) & 1;
                int64_t e = c + 1;
                while (e <= last && ((row[e >> 6] >> (e & 63)) & 1) == v) ++e;
                emit(e - c, v ? 'o' : 'b');
                c = e;
            }
        }
        ++pending;
    }
    emit(1, '!');
    out += '\n';
    const int64_t n = (int64_t)out.size() + 1;
    if (need) *need = n;
    if (!buf) return GOL_OK;  // the two-call form: the size only
    if (len < n) return gol_set_error(GOL_EINVAL, "RLE: the buffer is too small (%lld bytes needed)", (long long)n);
    memcpy(buf, out.c_str(), (size_t)n);
    return GOL_OK;
}
