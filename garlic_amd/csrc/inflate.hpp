// Raw DEFLATE (RFC 1951) of one BGZF block, and the CRC32 of its bytes: one body for the host and the device.
//
// inflate_block(in, n_in, out, n_out, tables): the compressed bytes [in, in + n_in) to [out, out + n_out), n_out = the
// block's ISIZE.  It returns a GARLIC_BGZF_* status on any input whatever and touches nothing but its two ranges and its
// tables: every read is checked against n_in, every write and copy against n_out, every table index against its table.  It
// accepts what zlib's inflate accepts for such a stream (a raw stream without dictionary), byte for byte, and refuses what
// zlib refuses:
//   stored lengths that do not complement, block type 3                              GARLIC_BGZF_BAD_BLOCK_TYPE
//   more than 286 / 30 symbols, an over-subscribed set, an incomplete one (but a tree of ONE code of length 1, as zlib
//   allows; a distance tree without any code is fine too), a repeat without a predecessor or beyond the last length,
//   no end-of-block code                                                              GARLIC_BGZF_BAD_CODE_LENGTHS
//   a code no symbol has, literal/length symbols 286 / 287, distance symbols 30 / 31  GARLIC_BGZF_BAD_SYMBOL
//   a distance beyond the bytes produced so far (blocks are independent)              GARLIC_BGZF_BAD_DISTANCE
//   bits wanted behind n_in                                                           GARLIC_BGZF_INPUT_ENDED
//   more bytes than n_out / fewer                                                     GARLIC_BGZF_OUTPUT_FULL / _SHORT
//   bytes left over behind the final block (zlib would take its trailer from there)   GARLIC_BGZF_BAD_CRC
//
// On the device one wave runs the body with every lane in step (the same bits, the same branches): symbol decode is
// sequential.  What the lanes share is the table clear and fill, the stored copy and the match copy, byte i of a match from
// out[at - dist + i % dist], which is right for overlapping matches too since all those bytes stand before the copy starts.
// Writes that must happen once come from lane 0 (INFLATE_LANE == 0).  Global and LDS accesses of one wave are served in
// program order, so a lane reads what another lane of its wave stored before; INFLATE_WAVE_SYNC() stands between every such
// store and read, so that the compiler keeps that order too.  On the host: one lane.
//
// A symbol is decoded through a first-level table of the codes up to FAST bits, entry = symbol << 4 | length, 0 = longer
// (or no code): then by the canonical walk over count[] / symbol[], one bit per step.  InflateTables is 3,968 bytes.
#pragma once
#include <stdint.h>

#include "../../include/garlic_hip.h"

#if defined(__HIPCC__) || defined(__CUDACC__)
#include <hip/hip_runtime.h>
#define INFLATE_HD __host__ __device__ inline
#else
#define INFLATE_HD inline
#endif

#if defined(__HIP_DEVICE_COMPILE__)
#define INFLATE_LANE ((uint32_t)(threadIdx.x & 63u))
#define INFLATE_LANES 64u
// what the lanes of the wave stored in front of it, every lane may read behind it: a release and an acquire fence at wavefront
// scope around a wave barrier.  None of the three emits an instruction; they keep the compiler from moving memory accesses across.
#define INFLATE_WAVE_SYNC()                                      \
    do {                                                         \
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");   \
        __builtin_amdgcn_wave_barrier();                         \
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");   \
    } while (0)
#else
#define INFLATE_LANE 0u
#define INFLATE_LANES 1u
#define INFLATE_WAVE_SYNC() do { } while (0)
#endif

namespace garlic {

constexpr int INFLATE_LIT_FAST = 10, INFLATE_DIST_FAST = 8;
constexpr int INFLATE_LIT_SYMBOLS = 288, INFLATE_DIST_SYMBOLS = 32;

struct InflateTables {
    uint16_t lit_fast[1 << INFLATE_LIT_FAST];
    uint16_t dist_fast[1 << INFLATE_DIST_FAST];
    uint16_t lit_count[16], dist_count[16], offs[16], code_count[16];
    uint16_t lit_symbol[INFLATE_LIT_SYMBOLS], dist_symbol[INFLATE_DIST_SYMBOLS];
    uint16_t code_symbol[32];                     // the code-length code: 19 symbols
    uint16_t code_fast[1 << 7];
    uint8_t lens[INFLATE_LIT_SYMBOLS + INFLATE_DIST_SYMBOLS];
};

struct InflateBits {
    const uint8_t *in;
    uint32_t n_in, pos;       // pos: the next byte to take into hold
    uint64_t hold;
    uint32_t bits;            // bits of hold in use; what lies above them is 0
};

INFLATE_HD void inflate_refill(InflateBits &b)
{
    if (b.bits <= 32 && b.pos + 4 <= b.n_in) {
        const uint32_t v = (uint32_t)b.in[b.pos] | (uint32_t)b.in[b.pos + 1] << 8 | (uint32_t)b.in[b.pos + 2] << 16 |
                           (uint32_t)b.in[b.pos + 3] << 24;
        b.hold |= (uint64_t)v << b.bits;
        b.bits += 32;
        b.pos += 4;
    }
    while (b.bits <= 56 && b.pos < b.n_in) {
        b.hold |= (uint64_t)b.in[b.pos++] << b.bits;
        b.bits += 8;
    }
}

// n <= 32 bits, refilled; false: the input has fewer
INFLATE_HD bool inflate_get(InflateBits &b, uint32_t n, uint32_t &v)
{
    inflate_refill(b);
    if (n > b.bits) return false;
    v = (uint32_t)(b.hold & ((1ull << n) - 1ull));
    b.hold >>= n;
    b.bits -= n;
    return true;
}

INFLATE_HD uint32_t inflate_reverse(uint32_t code, int len)
{
    uint32_t r = 0;
    for (int k = 0; k < len; k++) r |= ((code >> k) & 1u) << (len - 1 - k);
    return r;
}

// The tables of one code from its n lengths (n <= n_symbols, the room of symbol[]): count[len], symbol[] sorted by
// (length, symbol), fast[] over fast_bits.  Returns 0 for a complete set, 1 for an incomplete one, -1 for an
// over-subscribed one; max_len = the longest length in use (0: no code at all).
INFLATE_HD int inflate_build(const uint8_t *lens, int n, uint16_t *count, uint16_t *offs, uint16_t *symbol, int n_symbols,
                             uint16_t *fast, int fast_bits, int &max_len)
{
    const uint32_t lane = INFLATE_LANE;
    if (n > n_symbols) n = n_symbols;
    if (lane == 0) {
        for (int len = 0; len < 16; len++) count[len] = 0;
        for (int s = 0; s < n; s++) count[lens[s] & 15]++;
    }
    for (uint32_t k = lane; k < (1u << fast_bits); k += INFLATE_LANES) fast[k] = 0;
    INFLATE_WAVE_SYNC();
    max_len = 0;
    int left = 1;
    for (int len = 1; len < 16; len++) {
        const int c = count[len];
        if (c) max_len = len;
        left = 2 * left - c;
        if (left < 0) return -1;
    }
    if (lane == 0) {
        offs[1] = 0;
        for (int len = 1; len < 15; len++) offs[len + 1] = (uint16_t)(offs[len] + count[len]);
        for (int s = 0; s < n; s++) {
            const int len = lens[s] & 15;
            if (len) {
                const uint32_t at = offs[len]++;
                if (at < (uint32_t)n_symbols) symbol[at] = (uint16_t)s;
            }
        }
    }
    INFLATE_WAVE_SYNC();
    uint32_t code = 0, index = 0;
    for (int len = 1; len <= fast_bits; len++) {
        const uint32_t c = count[len];
        for (uint32_t k = 0; k < c; k++, code++, index++) {
            if (index >= (uint32_t)n_symbols) return -1;
            const uint16_t entry = (uint16_t)(symbol[index] << 4 | len);
            for (uint32_t j = inflate_reverse(code, len) + (lane << len); j < (1u << fast_bits); j += INFLATE_LANES << len) fast[j] = entry;
        }
        code <<= 1;
    }
    INFLATE_WAVE_SYNC();
    return left > 0 ? 1 : 0;
}

// the next symbol of a code, or -status
INFLATE_HD int inflate_symbol(InflateBits &b, const uint16_t *fast, int fast_bits, const uint16_t *count, const uint16_t *symbol,
                              int n_symbols)
{
    inflate_refill(b);
    const uint32_t e = fast[b.hold & ((1u << fast_bits) - 1u)];
    if (e) {
        const uint32_t len = e & 15u;
        if (len > b.bits) return -GARLIC_BGZF_INPUT_ENDED;
        b.hold >>= len;
        b.bits -= len;
        return (int)(e >> 4);
    }
    uint64_t h = b.hold;
    int code = 0, first = 0, index = 0;
    for (uint32_t len = 1; len < 16; len++) {
        code |= (int)(h & 1u);
        h >>= 1;
        const int c = count[len];
        if (code - c < first) {
            if (len > b.bits) return -GARLIC_BGZF_INPUT_ENDED;
            const int at = index + (code - first);
            if (at < 0 || at >= n_symbols) return -GARLIC_BGZF_BAD_SYMBOL;
            b.hold >>= len;
            b.bits -= len;
            return symbol[at];
        }
        index += c;
        first = (first + c) << 1;
        code <<= 1;
    }
    return b.bits < 15 ? -GARLIC_BGZF_INPUT_ENDED : -GARLIC_BGZF_BAD_SYMBOL;
}

// zlib's rule for a literal/length or distance set: complete, or one code of length 1, or (distance) none at all
INFLATE_HD bool inflate_set_ok(int built, int max_len) { return built == 0 || (built > 0 && max_len <= 1); }

// the code lengths of a dynamic block into t.lens and both codes built; 0 or a status
INFLATE_HD int inflate_dynamic(InflateBits &b, InflateTables &t)
{
    const uint8_t order[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
    const uint32_t lane = INFLATE_LANE;
    uint32_t nlen, ndist, ncode, v;
    if (!inflate_get(b, 5, nlen) || !inflate_get(b, 5, ndist) || !inflate_get(b, 4, ncode)) return GARLIC_BGZF_INPUT_ENDED;
    nlen += 257;
    ndist += 1;
    ncode += 4;
    if (nlen > 286 || ndist > 30) return GARLIC_BGZF_BAD_CODE_LENGTHS;
    if (lane == 0)
        for (int k = 0; k < 19; k++) t.lens[k] = 0;
    for (uint32_t k = 0; k < ncode; k++) {
        if (!inflate_get(b, 3, v)) return GARLIC_BGZF_INPUT_ENDED;
        if (lane == 0) t.lens[order[k]] = (uint8_t)v;
    }
    INFLATE_WAVE_SYNC();
    int max_len;
    if (inflate_build(t.lens, 19, t.code_count, t.offs, t.code_symbol, 32, t.code_fast, 7, max_len) != 0 || max_len == 0)
        return GARLIC_BGZF_BAD_CODE_LENGTHS;
    uint32_t have = 0, prev = 0;
    while (have < nlen + ndist) {
        const int s = inflate_symbol(b, t.code_fast, 7, t.code_count, t.code_symbol, 32);
        if (s < 0) return -s;
        uint32_t len = 0, rep = 1;
        if (s < 16) {
            len = (uint32_t)s;
        } else if (s == 16) {
            if (!have) return GARLIC_BGZF_BAD_CODE_LENGTHS;
            len = prev;
            if (!inflate_get(b, 2, v)) return GARLIC_BGZF_INPUT_ENDED;
            rep = 3 + v;
        } else if (s == 17) {
            if (!inflate_get(b, 3, v)) return GARLIC_BGZF_INPUT_ENDED;
            rep = 3 + v;
        } else if (s == 18) {
            if (!inflate_get(b, 7, v)) return GARLIC_BGZF_INPUT_ENDED;
            rep = 11 + v;
        } else {
            return GARLIC_BGZF_BAD_SYMBOL;
        }
        if (have + rep > nlen + ndist) return GARLIC_BGZF_BAD_CODE_LENGTHS;
        if (lane == 0)
            for (uint32_t k = 0; k < rep; k++) t.lens[have + k] = (uint8_t)len;
        have += rep;
        prev = len;
    }
    INFLATE_WAVE_SYNC();
    if (t.lens[256] == 0) return GARLIC_BGZF_BAD_CODE_LENGTHS;
    int built = inflate_build(t.lens, (int)nlen, t.lit_count, t.offs, t.lit_symbol, INFLATE_LIT_SYMBOLS, t.lit_fast, INFLATE_LIT_FAST, max_len);
    if (!inflate_set_ok(built, max_len)) return GARLIC_BGZF_BAD_CODE_LENGTHS;
    built = inflate_build(t.lens + nlen, (int)ndist, t.dist_count, t.offs, t.dist_symbol, INFLATE_DIST_SYMBOLS, t.dist_fast, INFLATE_DIST_FAST,
                          max_len);
    if (max_len != 0 && !inflate_set_ok(built, max_len)) return GARLIC_BGZF_BAD_CODE_LENGTHS;
    return GARLIC_BGZF_OK;
}

// the fixed codes: 288 literal/length and 32 distance symbols, both sets complete (286, 287, 30 and 31 are refused in use)
INFLATE_HD void inflate_fixed(InflateTables &t)
{
    for (uint32_t s = INFLATE_LANE; s < (uint32_t)(INFLATE_LIT_SYMBOLS + INFLATE_DIST_SYMBOLS); s += INFLATE_LANES)
        t.lens[s] = (uint8_t)(s < 144 ? 8 : s < 256 ? 9 : s < 280 ? 7 : s < 288 ? 8 : 5);
    INFLATE_WAVE_SYNC();
    int max_len;
    (void)inflate_build(t.lens, INFLATE_LIT_SYMBOLS, t.lit_count, t.offs, t.lit_symbol, INFLATE_LIT_SYMBOLS, t.lit_fast, INFLATE_LIT_FAST, max_len);
    (void)inflate_build(t.lens + INFLATE_LIT_SYMBOLS, INFLATE_DIST_SYMBOLS, t.dist_count, t.offs, t.dist_symbol, INFLATE_DIST_SYMBOLS, t.dist_fast,
                        INFLATE_DIST_FAST, max_len);
}

// the literals, lengths and distances of one block behind its tables, until its end-of-block code
INFLATE_HD int inflate_codes(InflateBits &b, const InflateTables &t, uint8_t *out, uint32_t n_out, uint32_t &at)
{
    const uint32_t lane = INFLATE_LANE;
    for (;;) {
        int s = inflate_symbol(b, t.lit_fast, INFLATE_LIT_FAST, t.lit_count, t.lit_symbol, INFLATE_LIT_SYMBOLS);
        if (s < 0) return -s;
        if (s < 256) {
            if (at >= n_out) return GARLIC_BGZF_OUTPUT_FULL;
            if (lane == 0) out[at] = (uint8_t)s;
            at++;
            continue;
        }
        if (s == 256) return GARLIC_BGZF_OK;
        if (s > 285) return GARLIC_BGZF_BAD_SYMBOL;
        uint32_t len, dist, extra, v = 0;
        if (s < 265) {
            len = (uint32_t)s - 254u;
        } else if (s == 285) {
            len = 258;
        } else {
            extra = ((uint32_t)s - 261u) >> 2;
            if (!inflate_get(b, extra, v)) return GARLIC_BGZF_INPUT_ENDED;
            len = 3u + ((4u + (((uint32_t)s - 261u) & 3u)) << extra) + v;
        }
        s = inflate_symbol(b, t.dist_fast, INFLATE_DIST_FAST, t.dist_count, t.dist_symbol, INFLATE_DIST_SYMBOLS);
        if (s < 0) return -s;
        if (s > 29) return GARLIC_BGZF_BAD_SYMBOL;
        if (s < 4) {
            dist = (uint32_t)s + 1u;
        } else {
            extra = ((uint32_t)s >> 1) - 1u;
            if (!inflate_get(b, extra, v)) return GARLIC_BGZF_INPUT_ENDED;
            dist = 1u + ((2u + ((uint32_t)s & 1u)) << extra) + v;
        }
        if (dist > at) return GARLIC_BGZF_BAD_DISTANCE;
        if (len > n_out - at) return GARLIC_BGZF_OUTPUT_FULL;
        const uint8_t *from = out + (at - dist);
        INFLATE_WAVE_SYNC();                       // the literals of lane 0 and the matches in front of this one
        if (dist >= len)
            for (uint32_t i = lane; i < len; i += INFLATE_LANES) out[at + i] = from[i];
        else
            for (uint32_t i = lane; i < len; i += INFLATE_LANES) out[at + i] = from[i % dist];
        at += len;
    }
}

INFLATE_HD int inflate_block(const uint8_t *in, uint32_t n_in, uint8_t *out, uint32_t n_out, InflateTables &t)
{
    InflateBits b = {in, n_in, 0, 0, 0};
    uint32_t at = 0, last = 0, type = 0, v = 0;
    do {
        if (!inflate_get(b, 1, last) || !inflate_get(b, 2, type)) return GARLIC_BGZF_INPUT_ENDED;
        if (type == 0) {
            if (!inflate_get(b, b.bits & 7u, v)) return GARLIC_BGZF_INPUT_ENDED;        // to the byte border
            uint32_t len, nlen;
            if (!inflate_get(b, 16, len) || !inflate_get(b, 16, nlen)) return GARLIC_BGZF_INPUT_ENDED;
            if ((len ^ 0xFFFFu) != nlen) return GARLIC_BGZF_BAD_BLOCK_TYPE;
            b.pos -= b.bits >> 3;                  // the whole bytes in hold go back
            b.hold = 0;
            b.bits = 0;
            if (len > b.n_in - b.pos) return GARLIC_BGZF_INPUT_ENDED;
            if (len > n_out - at) return GARLIC_BGZF_OUTPUT_FULL;
            for (uint32_t i = INFLATE_LANE; i < len; i += INFLATE_LANES) out[at + i] = in[b.pos + i];
            b.pos += len;
            at += len;
        } else if (type == 1 || type == 2) {
            int rc = GARLIC_BGZF_OK;
            if (type == 1) inflate_fixed(t);
            else rc = inflate_dynamic(b, t);
            if (rc) return rc;
            rc = inflate_codes(b, t, out, n_out, at);
            if (rc) return rc;
        } else {
            return GARLIC_BGZF_BAD_BLOCK_TYPE;
        }
    } while (!last);
    INFLATE_WAVE_SYNC();                           // whoever reads the bytes next (the CRC32) reads all lanes' stores
    if (at != n_out) return GARLIC_BGZF_OUTPUT_SHORT;
    if (b.pos - (b.bits >> 3) != n_in) return GARLIC_BGZF_BAD_CRC;
    return GARLIC_BGZF_OK;
}

// ---- CRC32 (the gzip polynomial, reflected: bit 31 of a word is the coefficient of x^0)

constexpr uint32_t CRC32_POLY = 0xEDB88320u;

INFLATE_HD uint32_t crc32_table_entry(uint32_t i)
{
    for (int k = 0; k < 8; k++) i = (i >> 1) ^ ((i & 1u) ? CRC32_POLY : 0u);
    return i;
}

// a * b mod the polynomial
INFLATE_HD uint32_t crc32_mul(uint32_t a, uint32_t b)
{
    uint32_t p = 0;
    for (int i = 0; i < 32; i++) {
        if (a & (0x80000000u >> i)) p ^= b;
        b = (b >> 1) ^ ((b & 1u) ? CRC32_POLY : 0u);
    }
    return p;
}

// x^(8 n) mod the polynomial
INFLATE_HD uint32_t crc32_x8n(uint32_t n)
{
    uint32_t r = 0x80000000u, base = 0x00800000u;
    for (; n; n >>= 1) {
        if (n & 1u) r = crc32_mul(r, base);
        base = crc32_mul(base, base);
    }
    return r;
}

// What lane `lane` of `lanes` adds to the CRC32 of p[0, n): the register over its piece of ceil(n / lanes) bytes -- from
// all ones in lane 0, from 0 elsewhere -- times x^(8 * the bytes behind the piece).  The CRC is the XOR of all lanes'
// parts, complemented.  table: the 256 entries of crc32_table_entry.
INFLATE_HD uint32_t crc32_lane_part(const uint8_t *p, uint32_t n, uint32_t lane, uint32_t lanes, const uint32_t *table)
{
    const uint32_t piece = (n + lanes - 1) / lanes;
    const uint32_t lo = lane * piece < n ? lane * piece : n, hi = lo + piece < n ? lo + piece : n;
    uint32_t s = lane == 0 ? 0xFFFFFFFFu : 0u;
    for (uint32_t k = lo; k < hi; k++) s = table[(s ^ p[k]) & 0xFFu] ^ (s >> 8);
    return crc32_mul(crc32_x8n(n - hi), s);
}

} // namespace garlic
