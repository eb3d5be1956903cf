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
//   1, 2. the line walk of text_line.hpp with the masks of the tabs and the newlines; the first newline ends the line and the
//      tabs behind it are dropped;
//   3. popcount of the tab mask through text_block_scan: the column of each piece's first byte;
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
#include "text_line.hpp"

namespace garlic {

constexpr int VCF_OK = 0;
constexpr int VCF_BAD_BYTE = 1;        // a byte the grammar has no place for (an empty field included)
constexpr int VCF_HALF_MISSING = 2;    // ./1, 0|.
constexpr int VCF_HAPLOID = 3;         // one allele and no separator
constexpr int VCF_ALLELE_INDEX = 4;    // an allele index >= 2
constexpr int VCF_FEW_COLUMNS = 5;     // column = the number of sample columns the line has
constexpr int VCF_MANY_COLUMNS = 6;    // column = nind_total

constexpr int VCF_SLOTS = TEXT_PASS_PIECES + 2;
constexpr int VCF_STAGE = 16 * (TEXT_PASS_PIECES + 1) + 16;    // samples that can start in the 257 slots of a last pass + the 7 left over

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

    const int tid = threadIdx.x;
    const int64_t r = blockIdx.x;
    const TextLine ln = text_line_of(text, text_bytes, line_begin, r);

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
    for (int64_t p0 = ln.p_first; !ended; p0 += TEXT_PASS_PIECES) {
        __syncthreads();          // the previous pass has let go of the slots and the scan cells
        uint32_t w[4], live;
        text_load_piece(ln, p0 + tid, w, live);
        *reinterpret_cast<uint4 *>(s_text + 16 * (tid + 1)) = make_uint4(w[0], w[1], w[2], w[3]);
        const int64_t end = text_first_end(text_eq_mask(w, '\n') & live, s_end, tid);
        const bool last = text_last_pass(ln, p0, end);
        // tabs behind the line's end are no columns
        const uint32_t tabs = text_eq_mask(w, '\t') & text_keep_mask(end, tid);
        uint32_t before, pass_tabs;
        text_block_scan(__popc(tabs), s_tabs, tid, before, pass_tabs);
        s_mask[tid + 1] = tabs;
        s_col[tid + 1] = col + before;
        col += pass_tabs;
        __syncthreads();
        // decode the fields that start behind the tabs of slots 0 .. 255 (and of slot 256 when no pass follows)
        const int nslots = last ? TEXT_PASS_PIECES + 1 : TEXT_PASS_PIECES;
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
                    text_offend(offence, nind, VCF_MANY_COLUMNS);
                    continue;
                }
                const uint8_t *f = s_text + 16 * slot + q + 1;
                uint32_t out = 0;
                const int code = vcf_decode_gt(f[0], f[1], f[2], f[3], out);
                if (code != VCF_OK) text_offend(offence, j, code);
                s_stage[j - jbase] = (uint8_t)out;
            }
        }
        __syncthreads();
        // samples decoded so far: those whose tab lies in a decoded slot
        const int64_t cols_done = last ? col : s_col[TEXT_PASS_PIECES];
        int64_t done = cols_done - 8 > 0 ? cols_done - 8 : 0;
        if (last && done < nind) text_offend(offence, done, VCF_FEW_COLUMNS);
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
            *reinterpret_cast<uint4 *>(s_text) = *reinterpret_cast<const uint4 *>(s_text + 16 * TEXT_PASS_PIECES);
            s_mask[0] = s_mask[TEXT_PASS_PIECES];
            s_col[0] = s_col[TEXT_PASS_PIECES];
        }
        jbase = 8 * g_hi;
        ended = last;
    }
    text_write_status(&s_offence, offence, status, r, tid);
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
