// Decimal text -> double, on the host and on the device, exactly where that is provable and not at all elsewhere.
//
// tgls_number(p, len, out) reads the len bytes of one token of a --tgls file and answers either with the double that
// operator>>(double&) / strtod give for it (true), or with "defer" (false): the caller then leaves the token to strtod.
//   grammar   [+-]? (digits [. digits*]? | . digits) ([eE] [+-]? digits)?          the whole token, nothing before or behind
//   value     leading zeros dropped, the digits read as one integer m, the fraction digits folded into the decimal exponent e;
//             m == 0 -> +-0.0;  m <= 2^53 and |e| <= 22 -> m * 10^e (e >= 0) or m / 10^-e (e < 0);  everything else: defer.
// Why one operation is enough: m <= 2^53 and 10^k, k <= 22 (5^22 < 2^53), are doubles without error, so the decimal's value
// IS the exact product or quotient of two doubles, and IEEE 754 rounds one multiplication or division of them correctly,
// to nearest even -- which is what strtod returns.  The build has -fno-fast-math -ffp-contract=off (csrc/Makefile), so `/` is
// the IEEE division on the device as well, not a reciprocal and a multiplication.
// Deferred, never guessed: more significant digits than 2^53 holds, larger exponents, inf / nan / hex floats, an exponent
// without digits, any byte outside the grammar, and tokens longer than TGLS_TOKEN_MAX (the kernel's look-ahead).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define TGLS_HD __host__ __device__
#else
#define TGLS_HD
#endif

namespace garlic {

constexpr int TGLS_TOKEN_MAX = 32;      // bytes of the longest token that gets a value

TGLS_HD inline double tgls_pow10(int k)      // 10^k, 0 <= k <= 22: every entry exact (a constant table, no private copy per call)
{
    static constexpr double P[23] = {1e0,  1e1,  1e2,  1e3,  1e4,  1e5,  1e6,  1e7,  1e8,  1e9,  1e10, 1e11,
                              1e12, 1e13, 1e14, 1e15, 1e16, 1e17, 1e18, 1e19, 1e20, 1e21, 1e22};
    return P[k];
}

TGLS_HD inline bool tgls_number(const uint8_t *p, int len, double *out)
{
    if (len < 1 || len > TGLS_TOKEN_MAX) return false;
    int i = 0;
    const bool neg = p[0] == '-';
    if (p[0] == '-' || p[0] == '+') i++;
    uint64_t m = 0;
    int e = 0, ndigits = 0;
    bool dot = false;
    for (; i < len; i++) {
        const uint32_t c = p[i];
        if (c == '.') {
            if (dot) return false;
            dot = true;
            continue;
        }
        if (c < '0' || c > '9') break;
        ndigits++;
        if (m >= 1000000000000000000ull) return false;       // a 20th significant digit: m would not fit (and is past 2^53 anyway)
        m = 10 * m + (c - '0');
        if (dot) e--;
    }
    if (ndigits == 0) return false;
    if (i < len) {
        if (p[i] != 'e' && p[i] != 'E') return false;
        i++;
        bool eneg = false;
        if (i < len && (p[i] == '-' || p[i] == '+')) eneg = p[i++] == '-';
        if (i >= len) return false;
        int x = 0;
        for (; i < len; i++) {
            const uint32_t c = p[i];
            if (c < '0' || c > '9') return false;
            x = 10 * x + (int)(c - '0');
            if (x > 100000) x = 100000;                      // (far outside +-22 whatever the fraction folds in; a zero stays a zero)
        }
        e += eneg ? -x : x;
    }
    if (m == 0) {
        *out = neg ? -0.0 : 0.0;
        return true;
    }
    if (m > (1ull << 53) || e > 22 || e < -22) return false;
    const double v = e >= 0 ? (double)m * tgls_pow10(e) : (double)m / tgls_pow10(-e);
    *out = neg ? -v : v;
    return true;
}

} // namespace garlic
