// VCF text -> the rows of a garlic_bed image and of its order plane (gfx950, wave64), and what reads the plane: the phase fill.
//
// A data line of a VCF is nine tab-separated fixed columns and then one column per sample, of which only the leading GT is
// read: `a sep b`, a and b one of 0 1 . , sep / or | , followed by : tab \r \n or the end of the line.
//     0?0 -> 00 (hom A1 = REF)   1?1 -> 11 (hom A2 = ALT)   0?1, 1?0 -> 10 (het)   .?. -> 01 (missing)
// in PLINK's codes, and the order bit of the genotype is (a == '1'): "the first allele is A2".  Everything else is an offence,
// answered by a status code (VCF_*) and the sample column of the line's first offence; nothing else is done about it.
//
// vcf_parse_kernel: one workgroup of 256 lanes per line; the line goes through it in passes of 256 aligned 16-byte pieces
// (4 KB), every piece read from HBM once.  Fields have any width, so a lane finds the sample of a byte by counting tabs:
//   1. a lane loads its piece, replaces the bytes outside the line's [begin, limit) by '\n' (what a poisoned neighbour holds
//      never reaches a decision), and compares for tab and newline: two 16-bit masks;
//   2. the first newline of the pass (ballot per wave, minimum over the four waves through LDS) ends the line: tabs behind it
//      are dropped from the masks;
//   3. popcount of the tab mask, inclusive scan by __shfl_up inside a wave and over the four wave totals through LDS: the
//      column of each piece's first byte;
//   4. the pieces, their masks and columns stand in LDS as slots 1 .. 256; slot 0 is the previous pass's last piece and slot
//      257 is all '\n'.  A lane decodes the fields that START in slot `lane` (the byte after each of its tabs) from four LDS
//      bytes, which may reach into the next slot -- that is why the decode runs one slot behind the load (slot 256 is decoded
//      as slot 0 of the next pass, or by lane 0 in the last pass) and why no byte is loaded twice;
//   5. the decoded code | order << 2 goes to an LDS byte per sample, a window that starts at a multiple of 8 samples; after
//      the pass every complete group of 8 samples is packed by one lane into two image bytes and one plane byte and stored
//      with byte stores (a row starts at any byte); the <= 7 samples left move to the window's front.
// The first offence of the line is a 64-bit minimum in LDS over (column << 3 | code): independent of arrival order.  No global
// atomics; every store is a vector byte store into the row's own bytes; a row of the image or the plane is written by one
// workgroup only.  No switch point: any line length, field width and nind_total < 2^30 take this one path.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "lod_kernels.hpp"

namespace garlic {

constexpr int VCF_OK = 0;
constexpr int VCF_BAD_BYTE = 1;        // a byte the grammar has no place for (an empty field included)
constexpr int VCF_HALF_MISSING = 2;    // ./1, 0|.
constexpr int VCF_HAPLOID = 3;         // one allele and no separator
constexpr int VCF_ALLELE_INDEX = 4;    // an allele index >= 2
constexpr int VCF_FEW_COLUMNS = 5;     // column = the number of sample columns the line has
constexpr int VCF_MANY_COLUMNS = 6;    // column = nind_total

constexpr int VCF_PASS_PIECES = 256;
constexpr int VCF_SLOTS = VCF_PASS_PIECES + 2;
constexpr int VCF_STAGE = 16 * (VCF_PASS_PIECES + 1) + 16;     // samples that can start in the 257 slots of a last pass + the 7 left over

// the 16-bit mask of the bytes of a piece that equal c
__device__ __forceinline__ uint32_t vcf_eq_mask(const uint32_t w[4], uint32_t c)
{
    uint32_t m = 0;
#pragma unroll
    for (int k = 0; k < 16; k++) m |= (((w[k >> 2] >> (8 * (k & 3))) & 0xFFu) == c ? 1u : 0u) << k;
    return m;
}

__device__ __forceinline__ bool vcf_is_digit(uint32_t c) { return c >= '0' && c <= '9'; }
__device__ __forceinline__ bool vcf_is_end(uint32_t c) { return c == ':' || c == '\t' || c == '\r' || c == '\n'; }

// the leading GT of a field from its first four bytes: the status code; on VCF_OK `out` = PLINK code | order << 2
__device__ __forceinline__ int vcf_decode_gt(uint32_t a, uint32_t s, uint32_t b, uint32_t e, uint32_t &out)
{
    if (a != '0' && a != '1' && a != '.') return vcf_is_digit(a) ? VCF_ALLELE_INDEX : VCF_BAD_BYTE;
    if (s != '/' && s != '|') return vcf_is_end(s) ? VCF_HAPLOID : (vcf_is_digit(s) && a != '.') ? VCF_ALLELE_INDEX : VCF_BAD_BYTE;
    if (b != '0' && b != '1' && b != '.') return vcf_is_digit(b) ? VCF_ALLELE_INDEX : VCF_BAD_BYTE;
    if (!vcf_is_end(e)) return (vcf_is_digit(e) && b != '.') ? VCF_ALLELE_INDEX : VCF_BAD_BYTE;
    if ((a == '.') != (b == '.')) return VCF_HALF_MISSING;
    const uint32_t code = a == '.' ? 1u : a != b ? 2u : a == '1' ? 3u : 0u;
    out = code | (a == '1' ? 4u : 0u);
    return VCF_OK;
}

__global__ void __launch_bounds__(256)
vcf_parse_kernel(const uint8_t *__restrict__ text, int64_t text_bytes, const int64_t *__restrict__ line_begin, int64_t row_begin,
                 int32_t nind, uint8_t *__restrict__ image, int64_t row_bytes, uint8_t *__restrict__ plane, int64_t plane_row_bytes,
                 int32_t *__restrict__ status)
{
    __shared__ __attribute__((aligned(16))) uint8_t s_text[VCF_SLOTS * 16];
    __shared__ uint32_t s_mask[VCF_SLOTS];
    __shared__ int64_t s_col[VCF_SLOTS];
    __shared__ __attribute__((aligned(8))) uint8_t s_stage[VCF_STAGE];
    __shared__ int64_t s_end[4];
    __shared__ uint32_t s_tabs[4];
    __shared__ unsigned long long s_offence;

    const int tid = threadIdx.x, wv = tid >> 6, lane = tid & (WAVE - 1);
    const int64_t r = blockIdx.x;
    int64_t begin = line_begin[r], limit = line_begin[r + 1];
    limit = limit < text_bytes ? limit : text_bytes;
    begin = begin < limit ? begin : limit;
    // pieces are aligned in memory, not in the slab: byte `o` of the slab sits at piece (o + shift) >> 4
    const int64_t shift = (int64_t)((uintptr_t)text & 15);
    const uint8_t *base = text - shift;                       // 16-byte aligned
    const int64_t p_first = (begin + shift) >> 4;
    const int64_t p_end = (limit + shift + 15) >> 4;          // one past the last piece that holds a byte of the line
    const int64_t lo = begin + shift, hi = limit + shift;     // the line's bytes as offsets from `base`

    if (tid == 0) {
        s_offence = ~0ull;
        s_mask[0] = 0;
        s_col[0] = 0;
    }
    if (tid < 4) {
        reinterpret_cast<uint32_t *>(s_text)[tid] = 0x0A0A0A0Au;
        reinterpret_cast<uint32_t *>(s_text + 16 * (VCF_SLOTS - 1))[tid] = 0x0A0A0A0Au;
    }
    if (tid == 0) s_mask[VCF_SLOTS - 1] = 0;
    unsigned long long offence = ~0ull;
    int64_t col = 0;              // tabs of the line before this pass = column of the pass's first byte
    int64_t jbase = 0;            // sample of s_stage[0], a multiple of 8
    bool ended = false;
    for (int64_t p0 = p_first; !ended; p0 += VCF_PASS_PIECES) {
        __syncthreads();          // the previous pass has let go of the slots and the scan cells
        const int64_t pc = p0 + tid;
        const int64_t at = 16 * pc;
        uint32_t w[4] = {0x0A0A0A0Au, 0x0A0A0A0Au, 0x0A0A0A0Au, 0x0A0A0A0Au};
        uint32_t live = 0;        // bytes of the piece at or behind the line's first
        if (pc < p_end) {
            const uint4 v = *reinterpret_cast<const uint4 *>(base + at);
            w[0] = v.x; w[1] = v.y; w[2] = v.z; w[3] = v.w;
            live = 0xFFFFu;
            if (at < lo || at + 16 > hi) {                    // a piece at an end of the line
                live = 0;
#pragma unroll
                for (int k = 0; k < 16; k++) {
                    const int64_t o = at + k;
                    if (o < lo || o >= hi) w[k >> 2] = (w[k >> 2] & ~(0xFFu << (8 * (k & 3)))) | (0x0Au << (8 * (k & 3)));
                    if (o >= lo) live |= 1u << k;
                }
            }
        } else {
            live = 0xFFFFu;
        }
        *reinterpret_cast<uint4 *>(s_text + 16 * (tid + 1)) = make_uint4(w[0], w[1], w[2], w[3]);
        uint32_t tabs = vcf_eq_mask(w, '\t');
        const uint32_t nls = vcf_eq_mask(w, '\n') & live;
        // the first newline of the pass, as a byte offset from the pass's first piece
        const uint64_t has = __ballot(nls != 0);
        const int my_nl = nls ? __ffs(nls) - 1 : 0;
        const int first_lane = has ? __ffsll((unsigned long long)has) - 1 : 0;
        const int nl_byte = __shfl(my_nl, first_lane, WAVE);
        if (lane == 0) s_end[wv] = has ? (int64_t)(16 * (64 * wv + first_lane) + nl_byte) : INT64_MAX;
        __syncthreads();
        int64_t end = s_end[0];
#pragma unroll
        for (int k = 1; k < 4; k++) end = s_end[k] < end ? s_end[k] : end;
        const bool last = end != INT64_MAX || p0 + VCF_PASS_PIECES >= p_end;
        // tabs behind the line's end are no columns
        const int64_t mine = 16 * (int64_t)tid;
        if (end <= mine) tabs = 0;
        else if (end < mine + 16) tabs &= (1u << (int)(end - mine)) - 1u;
        uint32_t incl = __popc(tabs);
#pragma unroll
        for (int d = 1; d < WAVE; d <<= 1) {
            const uint32_t o = __shfl_up(incl, d, WAVE);
            if (lane >= d) incl += o;
        }
        if (lane == WAVE - 1) s_tabs[wv] = incl;
        __syncthreads();
        int64_t before = col;
        uint32_t pass_tabs = 0;
#pragma unroll
        for (int k = 0; k < 4; k++) {
            if (k < wv) before += s_tabs[k];
            pass_tabs += s_tabs[k];
        }
        s_mask[tid + 1] = tabs;
        s_col[tid + 1] = before + incl - __popc(tabs);
        col += pass_tabs;
        __syncthreads();
        // decode the fields that start behind the tabs of slots 0 .. 255 (and of slot 256 when no pass follows)
        const int nslots = last ? VCF_PASS_PIECES + 1 : VCF_PASS_PIECES;
        for (int slot = tid; slot < nslots; slot += 256) {
            uint32_t m = s_mask[slot];
            int64_t c = s_col[slot];
            while (m) {
                const int q = __ffs(m) - 1;
                m &= m - 1;
                c++;                                          // the column that starts at byte q + 1 of the slot
                const int64_t j = c - 9;
                if (j < 0) continue;
                if (j >= nind) {
                    const unsigned long long key = ((unsigned long long)nind << 3) | VCF_MANY_COLUMNS;
                    offence = key < offence ? key : offence;
                    continue;
                }
                const uint8_t *f = s_text + 16 * slot + q + 1;
                uint32_t out = 0;
                const int code = vcf_decode_gt(f[0], f[1], f[2], f[3], out);
                if (code != VCF_OK) {
                    const unsigned long long key = ((unsigned long long)j << 3) | (unsigned)code;
                    offence = key < offence ? key : offence;
                }
                s_stage[j - jbase] = (uint8_t)out;
            }
        }
        __syncthreads();
        // samples decoded so far: those whose tab lies in a decoded slot
        const int64_t cols_done = last ? col : s_col[VCF_PASS_PIECES];
        int64_t done = cols_done - 8 > 0 ? cols_done - 8 : 0;
        if (last && done < nind) {
            const unsigned long long key = ((unsigned long long)done << 3) | VCF_FEW_COLUMNS;
            offence = key < offence ? key : offence;
        }
        done = done < nind ? done : nind;
        const int64_t g_lo = jbase >> 3;
        const int64_t g_hi = last ? (done + 7) >> 3 : done >> 3;      // groups of 8 samples to store now
        uint8_t *img_row = image + (row_begin + r) * row_bytes;
        uint8_t *pl_row = plane + (row_begin + r) * plane_row_bytes;
        for (int64_t g = g_lo + tid; g < g_hi; g += 256) {
            const uint2 v = *reinterpret_cast<const uint2 *>(s_stage + 8 * (g - g_lo));
            const int n = (int)(done - 8 * g < 8 ? done - 8 * g : 8);  // samples of the group that exist
            uint32_t codes = 0, order = 0;
#pragma unroll
            for (int k = 0; k < 8; k++) {
                const uint32_t b = k < n ? ((k < 4 ? v.x : v.y) >> (8 * (k & 3))) & 0xFFu : 0u;
                codes |= (b & 3u) << (2 * k);
                order |= ((b >> 2) & 1u) << k;
            }
            img_row[2 * g] = (uint8_t)codes;
            if (n > 4) img_row[2 * g + 1] = (uint8_t)(codes >> 8);
            pl_row[g] = (uint8_t)order;
        }
        __syncthreads();
        if (!last && tid == 0) {
            const int left = (int)(done - 8 * g_hi);                  // 0 .. 7
            const int from = (int)(8 * (g_hi - g_lo));
            for (int k = 0; k < left; k++) s_stage[k] = s_stage[from + k];
            *reinterpret_cast<uint4 *>(s_text) = *reinterpret_cast<const uint4 *>(s_text + 16 * VCF_PASS_PIECES);
            s_mask[0] = s_mask[VCF_PASS_PIECES];
            s_col[0] = s_col[VCF_PASS_PIECES];
        }
        jbase = 8 * g_hi;
        ended = last;
    }
    if (offence != ~0ull) atomicMin(&s_offence, offence);
    __syncthreads();
    if (tid == 0) {
        const unsigned long long o = s_offence;
        const bool clean = o == ~0ull;
        status[2 * r] = clean ? 0 : (int32_t)(o & 7u);
        status[2 * r + 1] = clean ? 0 : (int32_t)((o >> 3) < 0x7FFFFFFFull ? (o >> 3) : 0x7FFFFFFFull);
    }
}

// HapData::firstCopy of the TPED line an image row stands for, as the panel's phase planes [blk][nloci]:
//     firstCopy = non-missing && (order bit == (counted == A2));   a row whose counted allele is none: all ones.
// One wave per (file row, 64-individual block), lane = individual ind_offset + 64 blk + lane of the row (any ind_offset: the
// code and the order bit are picked out of their bytes, which the lanes of a byte share); the word is a ballot, so the bits
// past the panel's last individual are clear, as phase_bits_planes_kernel leaves them.  Rows with dest[r] < 0 are skipped.
__global__ void __launch_bounds__(256)
bed_phase_planes_kernel(const uint8_t *__restrict__ image, int64_t row_bytes, const uint8_t *__restrict__ plane, int64_t plane_row_bytes,
                        const uint8_t *__restrict__ counted, const int64_t *__restrict__ dest, int64_t nrows, int64_t ind_offset,
                        int32_t nind, int32_t nblk, int64_t nloci, uint64_t *__restrict__ planeF)
{
    const int lane = threadIdx.x & (WAVE - 1);
    const int64_t nitems = nrows * nblk;
    const int64_t nwaves = ((int64_t)gridDim.x * blockDim.x) >> 6;
    for (int64_t item = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6; item < nitems; item += nwaves) {
        const int64_t r = item / nblk;
        const int blk = (int)(item - r * nblk);
        const int64_t l = dest[r];
        if (l < 0) continue;
        const int64_t ind = (int64_t)blk * WAVE + lane;
        bool fc = false;
        if (ind < nind) {
            const int64_t j = ind_offset + ind;
            const uint32_t c = counted[r];
            const uint32_t code = ((uint32_t)image[r * row_bytes + (j >> 2)] >> (2 * (int)(j & 3))) & 3u;
            const uint32_t bit = ((uint32_t)plane[r * plane_row_bytes + (j >> 3)] >> (int)(j & 7)) & 1u;
            fc = c >= 2 ? true : (code != 1u && bit == c);
        }
        const uint64_t word = __ballot(fc);
        if (lane == 0) planeF[(int64_t)blk * nloci + l] = word;
    }
}

} // namespace garlic
