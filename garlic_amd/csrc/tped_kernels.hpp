// TPED text -> the rows of a garlic_bed image, of its order plane and of its census (gfx950, wave64).
//
// A TPED line is four leading tokens (chr, name, gpos, ppos: any width, not read here) and then 2 * nind allele tokens of one
// byte each, separated by runs of blanks (' ', '\t', '\r').  The rule of src/garlic-data.cpp:103-141:
//     one      = the first allele of the line that is not the missing character (none: the missing character)
//     genotype = the number of its alleles equal to `one`; missing when either allele is missing
//     total    = the non-missing alleles of the line, those of half-missing genotypes (`0 G`) included
//     nalleles = the alleles equal to `one`
// As an image row with A1 := one:  one one -> 00   one x, x one -> 10   x y -> 11   either missing -> 01 (x, y: any other
// letters, alike or not), order bit = (a1 != one) on a non-missing genotype: "the first allele is A2".  The census of such a
// row cannot be recomputed from the row (`0 G` then `A A` has one = G although the first complete genotype is hom A2, and
// half-missing alleles count in total), so the kernel writes it: counts[row] = {nalleles, total}, counted[row] = 0 (A1), or 2
// when every allele is missing, and the letter `one` itself.
//
// tped_parse_kernel: one workgroup of 256 lanes per line; the line goes through it in passes of 256 aligned 16-byte pieces
// (4 KB), every piece read from HBM once and decoded from the registers that hold it.  Per pass:
//   1, 2. the line walk of text_line.hpp with the masks of the blanks, the newlines, the offending bytes (\v \f NUL) and the
//      missing character; the first newline ends the line and the bytes at and behind it are blanks.  A token START is a
//      non-blank byte behind a blank (the byte in front of a piece comes from the neighbour lane, the wave in front, or the
//      previous pass); a non-blank byte behind a non-blank one CONTINUES a token -- inside an allele token that is the
//      offence "longer than one byte", seen from its second byte, so no lane looks into the piece behind its own;
//   3. popcount of the start mask through text_block_scan: the index of each piece's first token; token 4 + a is allele a,
//      individual a >> 1;
//   4. while `one` is unknown: the pass's first non-missing allele (ballot per wave, first wave through LDS).  The alleles in
//      front of it are all missing, so nothing coded before depends on it;
//   5. every allele goes to an LDS byte (0 = one, 1 = other, 2 = missing) in a window that starts at a multiple of 16 alleles;
//      after the pass every complete group of 8 individuals is packed by one lane into two image bytes and one plane byte
//      (byte stores: a row starts at any byte) and the <= 15 alleles left move to the window's front.
// nalleles and total are per-lane popcounts, summed over a wave by shuffles and over the four waves through LDS in wave order.
// The first offence of the line is a 64-bit minimum in LDS over (column << 3 | code): independent of arrival order.  No global
// atomics; every store is a vector store into the row's own bytes; a row of the image, the plane and the census is written by
// one workgroup only.  No switch point: any line length, leading-field width and nind_total < 2^30 take this one path.
// LDS: 2080 bytes of alleles and a few scan cells (2.2 KB per workgroup), so the 32-wave cap of a CU (8 workgroups), not LDS,
// bounds the occupancy; a 4 KB pass keeps 32 KB of loads in flight per CU at that occupancy.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "lod_kernels.hpp"
#include "text_line.hpp"

namespace garlic {

constexpr int TPED_OK = 0;
constexpr int TPED_LONG_ALLELE = 1;    // an allele token longer than one byte
constexpr int TPED_BAD_BYTE = 2;       // \v, \f or NUL in the line
constexpr int TPED_FEW_COLUMNS = 3;    // column = the allele tokens found / 2
constexpr int TPED_MANY_COLUMNS = 4;   // column = nind_total

constexpr int TPED_STAGE = 8 * TEXT_PASS_PIECES + 32;      // the alleles that can start in a pass + the 15 left over

__global__ void __launch_bounds__(256)
tped_parse_kernel(const uint8_t *__restrict__ text, int64_t text_bytes, const int64_t *__restrict__ line_begin, int64_t row_begin,
                  int32_t nind, uint32_t missing, uint8_t *__restrict__ image, int64_t row_bytes, uint8_t *__restrict__ plane,
                  int64_t plane_row_bytes, int32_t *__restrict__ counts, uint8_t *__restrict__ counted, uint8_t *__restrict__ allele,
                  int32_t *__restrict__ status)
{
    __shared__ __attribute__((aligned(16))) uint8_t s_stage[TPED_STAGE];
    __shared__ int64_t s_end[4];
    __shared__ uint32_t s_starts[4];
    __shared__ uint32_t s_tail[4];         // per wave: is the last byte of its last piece a blank
    __shared__ uint32_t s_one[4];          // per wave: its first non-missing allele, 0x100 for none
    __shared__ int32_t s_sum[8];
    __shared__ unsigned long long s_offence;

    const int tid = threadIdx.x, wv = tid >> 6, lane = tid & (WAVE - 1);
    const int64_t r = blockIdx.x;
    const TextLine ln = text_line_of(text, text_bytes, line_begin, r);
    const int64_t nall_tokens = 2 * (int64_t)nind;

    if (tid == 0) s_offence = ~0ull;
    unsigned long long offence = ~0ull;
    int64_t tok = 0;              // tokens of the line that start before this pass
    int64_t abase = 0;            // allele of s_stage[0], a multiple of 16
    uint32_t prev_tail = 1;       // the byte in front of the pass is a blank (the line's first byte follows one)
    uint32_t one = 0;
    bool have_one = false;
    int32_t n_one = 0, n_total = 0;
    bool ended = false;
    for (int64_t p0 = ln.p_first; !ended; p0 += TEXT_PASS_PIECES) {
        __syncthreads();          // the previous pass has let go of the scan cells and of the window's front
        uint32_t w[4], live;
        text_load_piece(ln, p0 + tid, w, live);
        uint32_t nlf[4], blf[4], badf[4];
#pragma unroll
        for (int k = 0; k < 4; k++) {
            nlf[k] = text_eq_flags(w[k], '\n');
            blf[k] = nlf[k] | text_eq_flags(w[k], ' ') | text_eq_flags(w[k], '\t') | text_eq_flags(w[k], '\r');
            badf[k] = text_eq_flags(w[k], '\v') | text_eq_flags(w[k], '\f') | text_eq_flags(w[k], 0);
        }
        const uint32_t bl = text_flag_mask(blf);
        uint32_t bad = text_flag_mask(badf);
        const uint32_t ms = text_eq_mask(w, missing);
        // a byte in front of the line's end has its neighbour in front of it too: the raw mask serves
        if (lane == WAVE - 1) s_tail[wv] = bl >> 15;         // (read behind the barrier of text_first_end)
        const int64_t end = text_first_end(text_flag_mask(nlf) & live, s_end, tid);
        const bool last = text_last_pass(ln, p0, end);
        const uint32_t keep = text_keep_mask(end, tid);
        uint32_t prevb = __shfl_up(bl >> 15, 1, WAVE);
        if (lane == 0) prevb = wv ? s_tail[wv - 1] : prev_tail;
        prev_tail = s_tail[3];
        const uint32_t behind_blank = (bl << 1) | prevb;
        const uint32_t start = ~bl & behind_blank & keep;
        const uint32_t cont = ~bl & ~behind_blank & keep;
        bad &= keep;
        uint32_t before, pass_starts;
        text_block_scan(__popc(start), s_starts, tid, before, pass_starts);
        const int64_t first_tok = tok + before;                       // tokens that start before this piece
        tok += pass_starts;
        // the allele tokens among the piece's starts
        uint32_t am = start;
        int64_t a0 = first_tok - 4;                                   // the allele of am's lowest bit
        while (a0 < 0 && am) { am &= am - 1; a0++; }
        if (a0 + __popc(am) > nall_tokens) {
            text_offend(offence, nind, TPED_MANY_COLUMNS);
            uint32_t t = am;
            am = 0;
            for (int64_t a = a0; a < nall_tokens && t; a++) { am |= t & (0u - t); t &= t - 1; }
        }
        for (uint32_t odd = cont | bad; odd;) {                       // (no clean line comes here)
            const int q = __ffs(odd) - 1;
            odd &= odd - 1;
            const int64_t t = first_tok + __popc(start & ((2u << q) - 1u)) - 1;      // the token that holds byte q
            const int64_t j = t < 4 ? 0 : ((t - 4) >> 1) < nind ? (t - 4) >> 1 : nind;
            if ((bad >> q) & 1u) text_offend(offence, j, TPED_BAD_BYTE);
            if (((cont >> q) & 1u) && t >= 4) text_offend(offence, j, TPED_LONG_ALLELE);
        }
        const uint32_t nonmiss = am & ~ms;
        if (!have_one) {          // (uniform over the workgroup)
            const uint64_t got = __ballot(nonmiss != 0);
            const int q = nonmiss ? __ffs(nonmiss) - 1 : 0;
            const uint32_t my = (w[q >> 2] >> (8 * (q & 3))) & 0xFFu;
            const int fl = got ? __ffsll((unsigned long long)got) - 1 : 0;
            const uint32_t cand = __shfl(my, fl, WAVE);
            if (lane == 0) s_one[wv] = got ? cand : 0x100u;
            __syncthreads();
#pragma unroll
            for (int k = 3; k >= 0; k--)
                if (s_one[k] < 0x100u) { one = s_one[k]; have_one = true; }
        }
        const uint32_t oneeq = have_one ? text_eq_mask(w, one) : 0u;
        n_total += __popc(nonmiss);
        n_one += __popc(nonmiss & oneeq);
        {
            int64_t a = a0;
            for (uint32_t m = am; m; m &= m - 1, a++) {
                const int q = __ffs(m) - 1;
                s_stage[a - abase] = (uint8_t)(((ms >> q) & 1u) ? 2u : ((oneeq >> q) & 1u) ? 0u : 1u);
            }
        }
        __syncthreads();
        // alleles coded so far
        int64_t adone = tok - 4 > 0 ? tok - 4 : 0;
        if (last && adone < nall_tokens) text_offend(offence, adone >> 1, TPED_FEW_COLUMNS);
        adone = adone < nall_tokens ? adone : nall_tokens;
        const int64_t done = adone >> 1;                              // individuals with both alleles coded
        const int64_t g_lo = abase >> 4;
        const int64_t g_hi = last ? (done + 7) >> 3 : done >> 3;      // groups of 8 individuals to store now
        uint8_t *img_row = image + (row_begin + r) * row_bytes;
        uint8_t *pl_row = plane + (row_begin + r) * plane_row_bytes;
        for (int64_t g = g_lo + tid; g < g_hi; g += 256) {
            const uint4 v = *reinterpret_cast<const uint4 *>(s_stage + 16 * (g - g_lo));
            const uint32_t vv[4] = {v.x, v.y, v.z, v.w};
            const int n = (int)(done - 8 * g < 8 ? done - 8 * g : 8);  // individuals of the group that exist
            uint32_t codes = 0, order = 0;
#pragma unroll
            for (int k = 0; k < 8; k++) {
                const uint32_t pair = (vv[k >> 1] >> (16 * (k & 1))) & 0xFFFFu;
                const uint32_t x1 = pair & 0xFFu, x2 = pair >> 8;
                const bool miss = x1 == 2u || x2 == 2u;
                const uint32_t others = x1 + x2;
                const uint32_t code = miss ? 1u : others == 0u ? 0u : others == 1u ? 2u : 3u;
                if (k < n) {
                    codes |= code << (2 * k);
                    order |= (!miss && x1 == 1u ? 1u : 0u) << k;
                }
            }
            img_row[2 * g] = (uint8_t)codes;
            if (n > 4) img_row[2 * g + 1] = (uint8_t)(codes >> 8);
            pl_row[g] = (uint8_t)order;
        }
        __syncthreads();
        if (!last && tid == 0) {
            const int left = (int)(adone - 16 * g_hi);                // 0 .. 15
            const int from = (int)(16 * (g_hi - g_lo));
            for (int k = 0; k < left; k++) s_stage[k] = s_stage[from + k];
        }
        abase = 16 * g_hi;
        ended = last;
    }
#pragma unroll
    for (int d = WAVE / 2; d; d >>= 1) {
        n_one += __shfl_down(n_one, d, WAVE);
        n_total += __shfl_down(n_total, d, WAVE);
    }
    if (lane == 0) { s_sum[2 * wv] = n_one; s_sum[2 * wv + 1] = n_total; }
    text_write_status(&s_offence, offence, status, r, tid);      // (its barrier stands behind the store of s_sum too)
    if (tid == 0) {
        counts[2 * (row_begin + r)] = s_sum[0] + s_sum[2] + s_sum[4] + s_sum[6];
        counts[2 * (row_begin + r) + 1] = s_sum[1] + s_sum[3] + s_sum[5] + s_sum[7];
        counted[row_begin + r] = have_one ? 0 : 2;
        allele[r] = (uint8_t)(have_one ? one : missing);
    }
}

} // namespace garlic
