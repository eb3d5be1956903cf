// The host side of garlic_amd/csrc/tgls_number.hpp against strtod (stand-alone: built under -fsanitize=address,undefined by
// tests/test_tgls_cpu.py and run as a child process, never loaded into python).
//   tgls_number_unit              the fixed token sets and 10^6 random tokens
//   tgls_number_unit --file F     every whitespace-separated token of F from the fifth of each line on; prints
//                                 "tokens N deferred D"; a token that gets a value other than strtod's is a failure
#include "../../garlic_amd/csrc/tgls_number.hpp"

#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <random>
#include <sstream>
#include <string>
#include <vector>

using garlic::tgls_number;

static int failures = 0;

static uint64_t bits_of(double v)
{
    uint64_t b;
    memcpy(&b, &v, sizeof b);
    return b;
}

enum Want { VALUE, DEFER, EITHER };

// the token exactly as long as it is (no terminator behind it: the sanitizer sees a read past the token)
static bool run(const std::string &tok, double *out)
{
    std::vector<uint8_t> buf(tok.begin(), tok.end());
    return tgls_number(buf.data(), (int)buf.size(), out);
}

static bool check(const std::string &tok, Want want)
{
    double got = 0;
    const bool ok = run(tok, &got);
    if (ok) {
        char *end = nullptr;
        const double ref = strtod(tok.c_str(), &end);
        if (*end != '\0' || bits_of(ref) != bits_of(got)) {
            if (failures++ < 20)
                fprintf(stderr, "FAIL %s: got %.17g (%016" PRIx64 "), strtod %.17g (%016" PRIx64 ")\n", tok.c_str(), got, bits_of(got), ref, bits_of(ref));
            return ok;
        }
        std::stringstream ss(tok);      // and what the reader's operator>> gives
        double viaStream = 0;
        ss >> viaStream;
        if (ss.fail() || bits_of(viaStream) != bits_of(got)) {
            if (failures++ < 20) fprintf(stderr, "FAIL %s: operator>> gives %.17g\n", tok.c_str(), viaStream);
        }
    }
    if ((want == VALUE && !ok) || (want == DEFER && ok)) {
        if (failures++ < 20) fprintf(stderr, "FAIL %s: %s\n", tok.c_str(), ok ? "got a value, must defer" : "deferred, must get a value");
    }
    return ok;
}

static int file_mode(const char *path)
{
    std::ifstream in(path);
    if (!in) { fprintf(stderr, "cannot open %s\n", path); return 2; }
    std::string line, tok;
    long long n = 0, deferred = 0;
    while (std::getline(in, line)) {
        std::stringstream ss(line);
        for (int k = 0; ss >> tok; k++) {
            if (k < 4) continue;
            n++;
            if (!check(tok, EITHER)) deferred++;
        }
    }
    printf("tokens %lld deferred %lld\n", n, deferred);
    return failures ? 1 : 0;
}

int main(int argc, char **argv)
{
    if (argc == 3 && !strcmp(argv[1], "--file")) return file_mode(argv[2]);
    if (argc != 1) { fprintf(stderr, "usage: tgls_number_unit [--file F]\n"); return 2; }
    char buf[128];
    for (int k = 0; k <= 120; k++) check(std::to_string(k), VALUE);
    // every -d.ddd with up to 4 decimals over a grid
    for (int whole = 0; whole <= 12; whole++)
        for (int decimals = 1; decimals <= 4; decimals++) {
            int scale = 1;
            for (int d = 0; d < decimals; d++) scale *= 10;
            const int step = scale > 1000 ? 7 : 1;
            for (int frac = 0; frac < scale; frac += step) {
                snprintf(buf, sizeof buf, "-%d.%0*d", whole, decimals, frac);
                check(buf, VALUE);
                check(buf + 1, VALUE);
            }
        }
    for (const char *t : {"0", "-0", "+0", "0.0", "-0.0", "-0.000", "0e0", "-0e5", ".0", "-.0", "0."}) check(t, VALUE);
    {
        double z = 1;
        if (!run("-0", &z) || bits_of(z) != 0x8000000000000000ull) { failures++; fprintf(stderr, "FAIL -0 is not -0.0\n"); }
        if (!run("0", &z) || bits_of(z) != 0) { failures++; fprintf(stderr, "FAIL 0 is not +0.0\n"); }
    }
    for (const char *t : {".5", "5.", "+5", "1e-22", "1E22", "9007199254740992", "9007199254740992e22", "9007199254740991e-22", "1e+5",
                          "00012", "000.5", "-00.25e1", "123456789012345e-15", "0.1", "0.3", "1.7976931348623157", "12345678901234567e0"})
        check(t, t == std::string("1.7976931348623157") || t == std::string("12345678901234567e0") ? DEFER : VALUE);
    for (const char *t : {"9007199254740993", "1e23", "1e-23", "1234567890123456e7x", "inf", "-inf", "nan", "NaN", "0x1p3", "1e", "1e+", "e5",
                          ".", "-", "+", "", "--1", "1.2.3", "1,5", "1 ", "1d5", "12345678901234567890123", "1e400", "1e-400",
                          "0.000000000000000000000000000000001", "100000000000000000000000000000000"})
        check(t, DEFER);
    // 16-digit significands past 2^53 must defer; those at or under it may answer, and then exactly
    for (const char *t : {"9999999999999999", "9.007199254740993", "1234567890.1234567", "9007199254740994"}) check(t, DEFER);
    check("1234567890.123456", VALUE);
    check("0.1234567890123456", VALUE);
    // 10^6 random tokens with <= 15 digits and |e| <= 22 in every spelling of the grammar: all must get values
    std::mt19937_64 rng(20240607);
    for (int k = 0; k < 1000000; k++) {
        const int nd = 1 + (int)(rng() % 15);
        std::string digits;
        for (int d = 0; d < nd; d++) digits += (char)('0' + rng() % 10);
        const int point = (int)(rng() % (nd + 2));       // nd + 1: no point
        std::string tok;
        const int sign = (int)(rng() % 3);
        if (sign) tok += sign == 1 ? '-' : '+';
        int fold = 0;
        if (point <= nd) {
            tok += digits.substr(0, (size_t)point) + "." + digits.substr((size_t)point);
            fold = nd - point;
            if (nd == 0) continue;
        } else {
            tok += digits;
        }
        if (rng() % 2) {
            const int lo = -22 + fold, hi = 22 + fold;      // the folded exponent stays inside [-22, 22]
            const int x = lo + (int)(rng() % (uint64_t)(hi - lo + 1));
            snprintf(buf, sizeof buf, "%c%s%d", rng() % 2 ? 'e' : 'E', x >= 0 && rng() % 2 ? "+" : "", x);
            tok += buf;
        }
        if (tok.size() > (size_t)garlic::TGLS_TOKEN_MAX) continue;
        check(tok, VALUE);
    }
    if (failures) { fprintf(stderr, "%d failures\n", failures); return 1; }
    printf("tgls_number_unit ok\n");
    return 0;
}
