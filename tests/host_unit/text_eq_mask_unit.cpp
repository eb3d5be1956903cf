// text_eq_mask of garlic_amd/csrc/text_line.hpp (the side of the header a host compiler sees) against the plain byte loop:
// every byte value x every c x each of the 16 positions of a piece, over two fillers, and 10^5 random pieces.
#include <cstdint>
#include <cstdio>
#include <cstring>

#include "../../garlic_amd/csrc/text_line.hpp"

static uint32_t plain_mask(const uint32_t w[4], uint32_t c)
{
    uint8_t b[16];
    memcpy(b, w, 16);
    uint32_t m = 0;
    for (int k = 0; k < 16; k++) m |= (b[k] == c ? 1u : 0u) << k;
    return m;
}

static long long failures = 0;

static void check(const uint8_t piece[16], uint32_t c)
{
    uint32_t w[4];
    memcpy(w, piece, 16);
    const uint32_t got = garlic::text_eq_mask(w, c), want = plain_mask(w, c);
    uint32_t f[4];
    for (int k = 0; k < 4; k++) f[k] = garlic::text_eq_flags(w[k], c);
    const uint32_t by_flags = garlic::text_flag_mask(f);
    if (got != want || by_flags != want) {
        if (failures++ < 10) printf("c = %u: got %04x, by flags %04x, want %04x\n", c, got, by_flags, want);
    }
}

int main()
{
    const uint8_t fillers[2] = {0x00, 0xFF};       // a filler equals c twice over the 256 values: 15 more bits set
    for (uint8_t filler : fillers)
        for (int pos = 0; pos < 16; pos++)
            for (uint32_t v = 0; v < 256; v++)
                for (uint32_t c = 0; c < 256; c++) {
                    uint8_t piece[16];
                    memset(piece, filler, 16);
                    piece[pos] = (uint8_t)v;
                    check(piece, c);
                }
    uint64_t x = 0x9E3779B97F4A7C15ull;            // xorshift64
    auto next = [&]() { x ^= x << 13; x ^= x >> 7; x ^= x << 17; return x; };
    for (int t = 0; t < 100000; t++) {
        uint8_t piece[16];
        const uint64_t a = next(), b = next(), pick = next();
        memcpy(piece, &a, 8);
        memcpy(piece + 8, &b, 8);
        if (t & 1)                                 // a text-like piece: few values, many hits
            for (int k = 0; k < 16; k++) piece[k] = (uint8_t)("\t\n\r :01./|"[piece[k] % 10]);
        check(piece, (pick & 1) ? piece[(pick >> 1) & 15] : (uint32_t)((pick >> 8) & 0xFF));
    }
    if (failures) {
        printf("text_eq_mask_unit: %lld failures\n", failures);
        return 1;
    }
    printf("text_eq_mask_unit ok\n");
    return 0;
}
