// PLINK .bed rows on the device (gfx950, wave64): the allele census, the recode into the packed panel, the column subset
// and the hom rows of a feature set.
//
// A .bed row holds the N individuals of one SNP at 2 bits each, 4 per byte, individual j at bits 2 * (j % 4) of byte j / 4:
// 00 hom A1, 01 missing, 10 het, 11 hom A2.  GARLIC counts "the first non-missing allele on the line"
// (src/garlic-data.cpp:107-113); on the TPED line the row stands for a hom A1 genotype reads "A1 A1", a het "A1 A2", a hom A2
// "A2 A2", so the counted allele is A2 when the first non-missing genotype is hom A2 and A1 otherwise.  Both kernels are
// integer work and exact.
//
// The image keeps the rows back to back, (N + 3) / 4 bytes each: a row starts at any byte.  Both kernels therefore read the
// image in ALIGNED 16-byte pieces (the buffer is 256-byte aligned and padded past its last row) and mask what a piece holds
// of the neighbouring rows.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "lod_kernels.hpp"

namespace garlic {

constexpr uint64_t BED_LO = 0x5555555555555555ull;
constexpr int BED_IMAGE_PAD = 32;      // bytes past the last row that an aligned 16-byte read may touch

// the fields [a, b) of a 64-bit word of 32 two-bit fields, as a mask on the low bit of each field (0 <= a, b <= 32)
__device__ __forceinline__ uint64_t bed_field_mask(int a, int b)
{
    if (b <= a) return 0;
    const uint64_t upto_b = b >= 32 ? ~0ull : ((1ull << (2 * b)) - 1);
    const uint64_t upto_a = (1ull << (2 * a)) - 1;     // a < b <= 32: a <= 31
    return (upto_b & ~upto_a) & BED_LO;
}

// One row per group of `group` lanes (a power of two, 1 .. 64; 64 / group rows share a wave, so the 12-byte rows of a
// 45-individual panel go 32 to a wave); a group walks its row in 16-byte pieces, `group` of them a trip.  Per lane: the
// class counts of its pieces by popcount and the first non-missing genotype as the key  2 * individual + (hom A2);  per
// group: sums and the minimum key over the lanes by cross-lane exchange -- no atomics, nothing depends on arrival order.
// counts[r] = {nalleles, total}, counted[r] = 0 (A1), 1 (A2), 2 (none: every genotype missing).
// An image with an order plane (`order` != NULL: one bit per genotype, rows of order_row_bytes, bit i & 7 of byte i >> 3 =
// "the first allele of individual i's genotype is A2") takes the low bit of the winning key from the plane: a het that reads
// "A2 A1" on its TPED line counts A2.
__global__ void __launch_bounds__(256)
bed_census_kernel(const uint8_t *__restrict__ image, int64_t nrows, int32_t nind, int64_t row_bytes, int32_t group,
                  int32_t *__restrict__ counts, uint8_t *__restrict__ counted, const uint8_t *__restrict__ order,
                  int64_t order_row_bytes)
{
    const int lane = threadIdx.x & (WAVE - 1);
    const int sub = lane & (group - 1);
    const int64_t rows_per_wave = WAVE / group;
    const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const int64_t nwaves = ((int64_t)gridDim.x * blockDim.x) >> 6;
    const int64_t nsteps = (nrows + rows_per_wave - 1) / rows_per_wave;
    for (int64_t step = wave; step < nsteps; step += nwaves) {
        const int64_t r = step * rows_per_wave + lane / group;
        const bool live = r < nrows;
        const int64_t begin = live ? r * row_bytes : 0;              // first byte of the row
        const int64_t a0 = begin & ~(int64_t)15;
        const int64_t npieces = live ? ((begin + row_bytes - a0 + 15) >> 4) : 0;
        uint32_t n_a1 = 0, n_het = 0, n_a2 = 0, first = 0xFFFFFFFFu;
        for (int64_t pc = sub; pc < npieces; pc += group) {
            const int64_t at = a0 + 16 * pc;
            const uint4 v = *reinterpret_cast<const uint4 *>(image + at);
            const uint64_t w2[2] = {(uint64_t)v.x | ((uint64_t)v.y << 32), (uint64_t)v.z | ((uint64_t)v.w << 32)};
#pragma unroll
            for (int h = 0; h < 2; h++) {
                // field t of this word is individual j0 + t
                const int64_t j0 = 4 * (at + 8 * h - begin);
                const int lo_t = j0 < 0 ? (int)(-j0 < 32 ? -j0 : 32) : 0;
                const int64_t left = (int64_t)nind - j0;
                const int hi_t = left < 0 ? 0 : (left < 32 ? (int)left : 32);
                const uint64_t valid = bed_field_mask(lo_t, hi_t);
                const uint64_t lo = w2[h] & BED_LO, hi = (w2[h] >> 1) & BED_LO;
                const uint64_t a1 = ~lo & ~hi & valid, het = ~lo & hi & valid, a2 = lo & hi & valid;
                n_a1 += __popcll(a1);
                n_het += __popcll(het);
                n_a2 += __popcll(a2);
                const uint64_t nm = a1 | het | a2;
                if (nm) {
                    const int t = (__ffsll((unsigned long long)nm) - 1) >> 1;
                    const uint32_t key = (uint32_t)(2 * (j0 + t)) + (uint32_t)((a2 >> (2 * t)) & 1);
                    first = key < first ? key : first;
                }
            }
        }
        for (int d = group >> 1; d > 0; d >>= 1) {
            n_a1 += __shfl_xor(n_a1, d, WAVE);
            n_het += __shfl_xor(n_het, d, WAVE);
            n_a2 += __shfl_xor(n_a2, d, WAVE);
            const uint32_t o = __shfl_xor(first, d, WAVE);
            first = o < first ? o : first;
        }
        if (live && sub == 0) {
            const bool none = first == 0xFFFFFFFFu;
            if (order && !none) {     // the genotype's own first allele instead of the implied "hom A2"
                const uint32_t i = first >> 1;
                first = (first & ~1u) | (((uint32_t)order[r * order_row_bytes + (i >> 3)] >> (i & 7u)) & 1u);
            }
            const uint32_t c = none ? 2u : (first & 1u);
            counts[2 * r] = none ? 0 : (int32_t)(2 * (c ? n_a2 : n_a1) + n_het);
            counts[2 * r + 1] = none ? 0 : (int32_t)(2 * (n_a1 + n_het + n_a2));
            counted[r] = (uint8_t)c;
        }
    }
}

// PLINK codes -> the panel's (copies of the counted allele; 3 = missing), 32 fields at once.  By field value v = 2 hi + lo:
// counted A1: 0 -> 2, 1 -> 3, 2 -> 1, 3 -> 0;  counted A2: 0 -> 0, 1 -> 3, 2 -> 1, 3 -> 2;  none: all 3.  In both the new
// low bit is lo ^ hi; the new high bit is ~hi (A1) or lo (A2).
__device__ __forceinline__ uint64_t bed_recode64(uint64_t w, uint32_t c)
{
    const uint64_t lo = w & BED_LO, hi = (w >> 1) & BED_LO;
    const uint64_t nh = c == 0 ? (~hi & BED_LO) : lo;
    return c >= 2 ? ~0ull : ((lo ^ hi) | (nh << 1));
}

// The transpose of pack_genotypes_2bit_kernel into the same [64-individual block][word row][64 individuals] layout, with the
// code map chosen per file row and the rows of a 16-locus word gathered through word_rows (built by the host from dest_locus):
// word_rows[(w - word_lo) * 16 + q] = file row whose genotypes go to bit position q of word row w, -1 = none (that position
// keeps its bits).  A workgroup takes one word row and a span of 64 blocks (4096 individuals): each of its 4 waves reads the
// pieces of 4 of the 16 file rows ONCE, 16 bytes per lane, 1 KB per wave instruction, recodes them and leaves them in LDS;
// then lane = individual, wave = block, and every lane picks its 16 codes from LDS (4 lanes share a byte: a broadcast) and
// writes one word -- 256 contiguous bytes per wave store.  (The one-byte-per-lane-and-locus reads of pack_genotypes_2bit_kernel
// fetch every row piece once per individual block and word.)
constexpr int BED_SPAN_BLOCKS = 64;
constexpr int BED_ROW_PIECES = BED_SPAN_BLOCKS + 2;    // 1 KB of a row + its misalignment (15 B) + the shift inside a byte
constexpr int BED_ROW_LDS = BED_ROW_PIECES * 16;

__global__ void __launch_bounds__(256)
bed_pack_kernel(const uint8_t *__restrict__ image, int64_t image_bytes /* padded: every aligned piece below it may be read */,
                int64_t row_bytes, const uint8_t *__restrict__ counted, const int32_t *__restrict__ word_rows,
                int64_t ind_offset, int32_t nind, int64_t nind_pad, int64_t nwordrows, uint32_t *__restrict__ packed,
                int64_t word_lo)
{
    __shared__ __attribute__((aligned(16))) uint8_t tile[16][BED_ROW_LDS];
    __shared__ int64_t row_a0[16];       // image offset of tile[q][0]; -1: no row at this position
    const int wv = threadIdx.x >> 6, lane = threadIdx.x & (WAVE - 1);
    const int64_t w = word_lo + blockIdx.x;
    const int64_t blk0 = (int64_t)blockIdx.y * BED_SPAN_BLOCKS;
    const int32_t *rows = word_rows + (int64_t)blockIdx.x * 16;
    // the span's individuals of the whole data set: [j_lo, j_hi]
    const int64_t j_lo = ind_offset + blk0 * 64;
    const int64_t last = (blk0 + BED_SPAN_BLOCKS) * 64 < nind ? (blk0 + BED_SPAN_BLOCKS) * 64 : nind;
    const int64_t j_hi = ind_offset + last - 1;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const int q = wv + 4 * k;
        const int32_t r = rows[q];
        if (r < 0 || j_hi < j_lo) {
            if (lane == 0) row_a0[q] = -1;
            continue;
        }
        const int64_t begin = (int64_t)r * row_bytes;
        const int64_t a0 = (begin + (j_lo >> 2)) & ~(int64_t)15;
        const int64_t end = begin + (j_hi >> 2);                 // last byte the span needs of this row
        const uint32_t c = counted[r];
        if (lane == 0) row_a0[q] = a0;
        for (int pc = lane; pc < BED_ROW_PIECES; pc += WAVE) {
            const int64_t at = a0 + 16 * (int64_t)pc;
            if (at > end || at + 16 > image_bytes) continue;
            const uint4 v = *reinterpret_cast<const uint4 *>(image + at);
            const uint64_t x = bed_recode64((uint64_t)v.x | ((uint64_t)v.y << 32), c);
            const uint64_t y = bed_recode64((uint64_t)v.z | ((uint64_t)v.w << 32), c);
            *reinterpret_cast<uint4 *>(&tile[q][16 * pc]) = make_uint4((uint32_t)x, (uint32_t)(x >> 32), (uint32_t)y, (uint32_t)(y >> 32));
        }
    }
    __syncthreads();
    // (rows[] is the same for the whole workgroup: a word without rows is left alone, pad individuals included -- they are
    // 0xFFFFFFFF since the panel was created)
    bool word_any = false;
#pragma unroll
    for (int q = 0; q < 16; q++) word_any = word_any || rows[q] >= 0;
    if (!word_any) return;
    for (int b = wv; b < BED_SPAN_BLOCKS; b += 4) {
        const int64_t ind = (blk0 + b) * 64 + lane;
        if (ind >= nind_pad) break;
        uint32_t *dst = packed + packed_index(w, ind, nwordrows);
        if (ind >= nind) { *dst = 0xFFFFFFFFu; continue; }
        const int64_t j = ind_offset + ind;
        const int sh = 2 * (int)(j & 3);
        uint32_t word = *dst;             // positions no row maps to keep their previous bits
#pragma unroll
        for (int q = 0; q < 16; q++) {
            const int64_t a0 = row_a0[q];
            if (a0 < 0) continue;
            const int64_t off = (int64_t)rows[q] * row_bytes + (j >> 2) - a0;
            const uint32_t code = ((uint32_t)tile[q][off] >> sh) & 3u;
            word = (word & ~(3u << (2 * q))) | (code << (2 * q));
        }
        *dst = word;
    }
}

// A column subset of an image as a new image: individual i of every new row is individual idx[i] of the same source row, in
// PLINK's codes, unchanged; the pad bits of a new row's last byte are zero.  Exact: bytes are moved, nothing is computed.
//
// A thread owns one 8-byte word of the new row (32 subset individuals) and keeps where each of them sits in the source row
// -- (byte, shift) relative to the first source byte its span needs -- in 32 registers across all the rows it walks.  A
// workgroup covers a span of 256 words (8192 subset individuals); blockIdx.x is the span, blockIdx.y walks steps of rows with
// the grid's stride.  A span of fewer than 129 words is laid over the workgroup several times (`words` lanes a copy, a power
// of two), each copy taking other rows of the step, so that a narrow subset leaves no lane idle.
//
// Per step the workgroup stages, for each of the step's rows, the source bytes [lo, hi] the span needs (lo / hi: the bytes of
// the span's smallest / largest index, found by the host) into LDS, in the aligned 16-byte pieces and under the image_bytes
// guard of bed_pack_kernel; a source row starts at any byte, so (begin + lo) & 15 is a per-row scalar on the lane's LDS
// offset.  Then every lane assembles its word from 32 LDS byte reads.  LDS budget: BED_EXTRACT_LDS bytes per workgroup (32
// KiB; 4 workgroups of it fit a CU's 160 KB); a row's range takes `pieces` = ((hi - lo + 15) >> 4) + 1 pieces whatever its
// alignment, and min(BED_EXTRACT_ROWS, budget / range) rows go into a step.  A span whose range does not fit once (hi - lo
// + 1 > 32,753 bytes: more than 131,012 file individuals between its smallest and largest index) has pieces = 0 and takes
// the global form: the same 32 byte reads per lane, from the image itself.
//
// New rows start at any byte as well: a full word is stored with two 4-byte stores when its address is 4-byte aligned and
// with byte stores otherwise, a row's ragged last word always with byte stores of its own bytes only -- no store touches a
// byte of a neighbouring row, so nothing depends on the order of the stores.
constexpr int BED_EXTRACT_SPAN_WORDS = 256;
constexpr int BED_EXTRACT_LDS = 32 * 1024;
constexpr int BED_EXTRACT_ROWS = 16;                   // rows of a step at the most
constexpr int BED_EXTRACT_MAX_RANGE = BED_EXTRACT_LDS - 15;    // hi - lo + 1 above this: global form

struct BedSpan {
    int32_t lo;          // first source byte of a row that the span needs
    int32_t pieces;      // 16-byte pieces per row in LDS; 0 = global form
};

__global__ void __launch_bounds__(256)
bed_extract_kernel(const uint8_t *__restrict__ image, int64_t image_bytes, int64_t nrows, int64_t src_row_bytes,
                   const int32_t *__restrict__ idx, int32_t n_idx, const BedSpan *__restrict__ spans, uint8_t *__restrict__ out,
                   int64_t out_row_bytes)
{
    __shared__ __attribute__((aligned(16))) uint8_t tile[BED_EXTRACT_LDS];
    const int tid = threadIdx.x;
    const BedSpan span = spans[blockIdx.x];
    const int64_t nwords = ((int64_t)n_idx + 31) >> 5;
    const int64_t word0 = (int64_t)blockIdx.x * BED_EXTRACT_SPAN_WORDS;
    const int span_words = (int)(nwords - word0 < BED_EXTRACT_SPAN_WORDS ? nwords - word0 : BED_EXTRACT_SPAN_WORDS);
    int words = 1;                                      // lanes per copy of the span
    while (words < span_words) words <<= 1;
    const int copies = 256 / words;
    const int my_copy = tid / words, my_word = tid & (words - 1);
    const bool owner = my_word < span_words;
    const int64_t w = word0 + my_word;                  // the word of the new row
    // where the 32 individuals of the word sit, relative to 4 * lo; `valid`: the low bit of every field that has an individual
    uint32_t rel[32];
    uint64_t valid = 0;
#pragma unroll
    for (int k = 0; k < 32; k++) {
        const int64_t i = 32 * w + k;
        const bool have = owner && i < n_idx;
        rel[k] = have ? (uint32_t)(idx[i] - 4 * span.lo) : 0u;
        valid |= have ? 1ull << (2 * k) : 0ull;
    }
    valid |= valid << 1;
    const int word_bytes = owner ? (int)(out_row_bytes - 8 * w < 8 ? out_row_bytes - 8 * w : 8) : 0;
    const int range = span.pieces * 16;                 // LDS bytes per row of a step
    const int step_rows = span.pieces ? (BED_EXTRACT_LDS / range < BED_EXTRACT_ROWS ? BED_EXTRACT_LDS / range : BED_EXTRACT_ROWS)
                                      : BED_EXTRACT_ROWS;
    const int64_t nsteps = (nrows + step_rows - 1) / step_rows;
    for (int64_t step = blockIdx.y; step < nsteps; step += gridDim.y) {
        const int64_t r0 = step * step_rows;
        const int nr = (int)(nrows - r0 < step_rows ? nrows - r0 : step_rows);
        if (span.pieces) {
            __syncthreads();                            // the previous step's reads are done
            for (int p = tid; p < nr * span.pieces; p += 256) {
                const int q = p / span.pieces, pc = p - q * span.pieces;
                const int64_t first = (r0 + q) * src_row_bytes + span.lo;       // first byte the span needs of this row
                const int64_t at = (first & ~(int64_t)15) + 16 * (int64_t)pc;
                const int64_t end = (r0 + q + 1) * src_row_bytes - 1;            // the row's last byte
                if (at > end || at + 16 > image_bytes) continue;
                *reinterpret_cast<uint4 *>(&tile[q * range + 16 * pc]) = *reinterpret_cast<const uint4 *>(image + at);
            }
            __syncthreads();
        }
        for (int q = my_copy; q < nr; q += copies) {
            if (!owner) break;
            const int64_t first = (r0 + q) * src_row_bytes + span.lo;
            uint64_t word = 0;
            if (span.pieces) {
                const uint8_t *src = tile + q * range + (int)(first & 15);
#pragma unroll
                for (int k = 0; k < 32; k++)
                    word |= (uint64_t)(((uint32_t)src[rel[k] >> 2] >> (2 * (rel[k] & 3u))) & 3u) << (2 * k);
            } else {
                const uint8_t *src = image + first;
#pragma unroll
                for (int k = 0; k < 32; k++)
                    word |= (uint64_t)(((uint32_t)src[rel[k] >> 2] >> (2 * (rel[k] & 3u))) & 3u) << (2 * k);
            }
            word &= valid;
            uint8_t *dst = out + (r0 + q) * out_row_bytes + 8 * w;
            if (word_bytes == 8 && ((uintptr_t)dst & 3) == 0) {
                reinterpret_cast<uint32_t *>(dst)[0] = (uint32_t)word;
                reinterpret_cast<uint32_t *>(dst)[1] = (uint32_t)(word >> 32);
            } else {
                for (int t = 0; t < word_bytes; t++) dst[t] = (uint8_t)(word >> (8 * t));
            }
        }
    }
}

// .bed rows -> the hom rows of a feature set (feature_kernels.hpp): output row k is "homozygous for A1" (selector 0: code 00,
// ~lo & ~hi), "homozygous for A2" (1: code 11, lo & hi) or empty (2) of image row file_row[k], one bit per individual, stored
// block-major: the word of the 64 individuals of block blk at bits[blk * set_rows + row_begin + k].  file_row comes in any
// order and may repeat (the two alleles of one site).  Integer work, exact; no atomics, no LDS.
//
// A thread owns one output row and BED_HOM_BLOCKS consecutive blocks: 64 contiguous bytes of its image row, which start at any
// byte -- it reads the 5 aligned 16-byte pieces that hold them (those that begin inside the row, under the image_bytes guard of
// bed_pack_kernel: nothing past the image is read, pieces that are not read stay zero), shifts the 80 bytes down by the row's
// misalignment in registers and compacts every 2 x 64 code bits to 64 hom bits by mask and shift.  Adjacent lanes take adjacent
// k, so each of a wave's four stores is 512 contiguous bytes; the waves of a workgroup take consecutive block groups of the
// same 64 rows, so the 64-byte sectors a row's pieces share between two groups are fetched by one CU.  Bits of individuals
// >= nind are cleared by the mask of the valid fields whatever the image holds there: the pad bits of a row's last byte, the
// neighbouring row's bytes in a piece, and the zeros of a piece that was not read would otherwise read as genotypes (a zero pad
// is code 00, "hom A1").
constexpr int BED_HOM_BLOCKS = 4;      // (the kernel's body is written out for 4)

// the low bits of the 32 two-bit fields of x, gathered into bits 0 .. 31
__device__ __forceinline__ uint64_t bed_gather_fields(uint64_t x)
{
    x &= BED_LO;
    x = (x | (x >> 1)) & 0x3333333333333333ull;
    x = (x | (x >> 2)) & 0x0F0F0F0F0F0F0F0Full;
    x = (x | (x >> 4)) & 0x00FF00FF00FF00FFull;
    x = (x | (x >> 8)) & 0x0000FFFF0000FFFFull;
    return (x | (x >> 16)) & 0x00000000FFFFFFFFull;
}

// one aligned 16-byte piece as two words, or zeros
__device__ __forceinline__ void bed_piece(const uint8_t *__restrict__ image, int64_t at, bool read, uint64_t &lo, uint64_t &hi)
{
    uint4 v = make_uint4(0, 0, 0, 0);
    if (read) v = *reinterpret_cast<const uint4 *>(image + at);
    lo = (uint64_t)v.x | ((uint64_t)v.y << 32);
    hi = (uint64_t)v.z | ((uint64_t)v.w << 32);
}

// the hom word of block blk from its 16 code bytes, which begin sh bits into the three words a, b, c
__device__ __forceinline__ uint64_t bed_hom_word(uint64_t a, uint64_t b, uint64_t c, int sh, uint32_t sel, int32_t nind, int64_t blk)
{
    uint64_t word = 0;
#pragma unroll
    for (int h = 0; h < 2; h++) {
        const uint64_t u = h ? b : a, v = h ? c : b;
        const uint64_t x = sh ? (u >> sh) | (v << (64 - sh)) : u;        // field t: individual 64 blk + 32 h + t
        const int64_t left = (int64_t)nind - (64 * blk + 32 * h);
        const uint64_t valid = bed_field_mask(0, left < 0 ? 0 : (left < 32 ? (int)left : 32));
        const uint64_t hom = (sel == 0 ? ~(x | (x >> 1)) : sel == 1 ? (x & (x >> 1)) : 0ull) & valid;
        word |= bed_gather_fields(hom) << (32 * h);
    }
    return word;
}

__global__ void __launch_bounds__(256)
bed_hom_rows_kernel(const uint8_t *__restrict__ image, int64_t image_bytes, int64_t row_bytes, int32_t nind,
                    const int64_t *__restrict__ file_row, const uint8_t *__restrict__ allele, int64_t row_begin, int64_t row_count,
                    int64_t set_rows, int32_t nblk, uint64_t *__restrict__ bits)
{
    const int lane = threadIdx.x & (WAVE - 1);
    const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const int64_t nwaves = ((int64_t)gridDim.x * blockDim.x) >> 6;
    const int64_t ngroups = ((int64_t)nblk + BED_HOM_BLOCKS - 1) / BED_HOM_BLOCKS;
    const int64_t nitems = ((row_count + WAVE - 1) / WAVE) * ngroups;      // (64 rows) x (block group), the group fastest
    for (int64_t item = wave; item < nitems; item += nwaves) {
        const int64_t tile = item / ngroups;
        const int64_t blk0 = (item - tile * ngroups) * BED_HOM_BLOCKS;
        const int64_t k = tile * WAVE + lane;
        if (k >= row_count) continue;
        const uint32_t sel = allele[k];
        // (a selector 2 reads nothing: file row 0 stands in for its addresses)
        const int64_t row = (sel < 2 ? file_row[k] : 0) * row_bytes;
        const int64_t begin = row + 16 * blk0;                       // the byte of the group's first individual
        const int64_t end = row + row_bytes;                         // one past the row's last byte
        const int64_t a0 = begin & ~(int64_t)15;
        const int64_t last = (end < image_bytes - 15 ? end : image_bytes - 15);      // a piece is read iff it begins below this
        const bool live = sel < 2;
        uint64_t w0, w1, w2, w3, w4, w5, w6, w7, w8, w9;
        bed_piece(image, a0, live && a0 < last, w0, w1);
        bed_piece(image, a0 + 16, live && a0 + 16 < last, w2, w3);
        bed_piece(image, a0 + 32, live && a0 + 32 < last, w4, w5);
        bed_piece(image, a0 + 48, live && a0 + 48 < last, w6, w7);
        bed_piece(image, a0 + 64, live && a0 + 64 < last, w8, w9);
        // down by the row's misalignment: first by a whole word, then by the bytes inside a word (selects: all in registers)
        const int s = (int)(begin & 15);
        const bool by_word = s >= 8;
        const int sh = 8 * (s & 7);
        const uint64_t c0 = by_word ? w1 : w0, c1 = by_word ? w2 : w1, c2 = by_word ? w3 : w2, c3 = by_word ? w4 : w3,
                       c4 = by_word ? w5 : w4, c5 = by_word ? w6 : w5, c6 = by_word ? w7 : w6, c7 = by_word ? w8 : w7,
                       c8 = by_word ? w9 : w8;
        uint64_t *out = bits + row_begin + k;
        if (blk0 < nblk) out[blk0 * set_rows] = bed_hom_word(c0, c1, c2, sh, sel, nind, blk0);
        if (blk0 + 1 < nblk) out[(blk0 + 1) * set_rows] = bed_hom_word(c2, c3, c4, sh, sel, nind, blk0 + 1);
        if (blk0 + 2 < nblk) out[(blk0 + 2) * set_rows] = bed_hom_word(c4, c5, c6, sh, sel, nind, blk0 + 2);
        if (blk0 + 3 < nblk) out[(blk0 + 3) * set_rows] = bed_hom_word(c6, c7, c8, sh, sel, nind, blk0 + 3);
    }
}

} // namespace garlic
