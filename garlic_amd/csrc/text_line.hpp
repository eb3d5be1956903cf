// The line walk that the text parsers share (gfx950, wave64): vcf_parse_kernel, tped_parse_kernel, tgls_parse_kernel and
// tgls_vcf_parse_kernel.  One workgroup of 256 lanes takes one line of a slab through passes of TEXT_PASS_PIECES aligned
// 16-byte pieces (4 KB), every piece read from HBM once.  A pass opens with the same two steps in every parser:
//   1. text_load_piece: a lane loads its piece and replaces the bytes outside the line's [begin, limit) by '\n' (what a
//      poisoned neighbour holds never reaches a decision); the parser compares the piece for the bytes of its grammar
//      (text_eq_mask, or text_eq_flags / text_flag_bits where several bytes make one mask): 16-bit masks, bit k = byte k;
//   2. text_first_end: the first line end of the pass (ballot per wave, minimum over the four waves through LDS) ends the
//      line; text_keep_mask clears what stands at and behind it from the parser's masks.
// Where a parser numbers what it found (columns, tokens), text_block_scan is the popcount scan over the pass: __shfl_up inside
// a wave, the four wave totals through LDS.  The first offence of a line is a 64-bit minimum over (column << 3 | code),
// independent of arrival order: text_offend per lane, text_write_status once behind the last pass.
// Each kernel keeps its own pass loop, its own LDS slots and its own decode; the cells these steps need (s_end, the scan cells,
// s_offence) are the kernel's and come in as parameters.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#include <hip/hip_runtime.h>

#include "lod_kernels.hpp"
#define TEXT_HD __host__ __device__ __forceinline__
#else
#define TEXT_HD inline
#endif

namespace garlic {

// 0x80 in every byte of x that equals c (exact: no borrow crosses a byte)
TEXT_HD uint32_t text_eq_flags(uint32_t x, uint32_t c)
{
    const uint32_t t = x ^ (c * 0x01010101u);
    return ~(((t & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | t | 0x7F7F7F7Fu);
}

// the four 0x80 flags of a word as bits 0 .. 3
TEXT_HD uint32_t text_flag_bits(uint32_t f) { return (((f >> 7) * 0x00204081u) >> 21) & 0xFu; }

// the four flag words of a piece as its 16-bit mask
TEXT_HD uint32_t text_flag_mask(const uint32_t f[4])
{
    return text_flag_bits(f[0]) | text_flag_bits(f[1]) << 4 | text_flag_bits(f[2]) << 8 | text_flag_bits(f[3]) << 12;
}

// the 16-bit mask of the bytes of a piece that equal c
TEXT_HD uint32_t text_eq_mask(const uint32_t w[4], uint32_t c)
{
    const uint32_t f[4] = {text_eq_flags(w[0], c), text_eq_flags(w[1], c), text_eq_flags(w[2], c), text_eq_flags(w[3], c)};
    return text_flag_mask(f);
}

#if defined(__HIPCC__) || defined(__CUDACC__)

constexpr int TEXT_PASS_PIECES = 256;      // pieces of a pass = lanes of the workgroup

// A line of the slab as aligned pieces.  Pieces are aligned in memory, not in the slab: byte `o` of the slab sits at piece
// (o + shift) >> 4 of `base`, shift = text & 15.
struct TextLine {
    const uint8_t *base;          // 16-byte aligned
    int64_t p_first, p_end;       // the piece of the line's first byte; one past the last piece that holds a byte of the line
    int64_t lo, hi;               // the line's bytes as offsets from `base`
};

// line r: [line_begin[r], line_begin[r + 1]), clamped to the slab
__device__ __forceinline__ TextLine text_line_of(const uint8_t *text, int64_t text_bytes, const int64_t *line_begin, int64_t r)
{
    int64_t begin = line_begin[r], limit = line_begin[r + 1];
    limit = limit < text_bytes ? limit : text_bytes;
    begin = begin < limit ? begin : limit;
    const int64_t shift = (int64_t)((uintptr_t)text & 15);
    TextLine ln;
    ln.base = text - shift;
    ln.p_first = (begin + shift) >> 4;
    ln.p_end = (limit + shift + 15) >> 4;
    ln.lo = begin + shift;
    ln.hi = limit + shift;
    return ln;
}

// Piece pc of the line into w, the bytes outside the line replaced by '\n' (a piece behind the line's last: all '\n', not
// loaded).  live = the bytes of the piece at or behind the line's first: a '\n' that stands in for a byte in front of the
// line is no line end.
__device__ __forceinline__ void text_load_piece(const TextLine &ln, int64_t pc, uint32_t w[4], uint32_t &live)
{
    const int64_t at = 16 * pc;
    w[0] = w[1] = w[2] = w[3] = 0x0A0A0A0Au;
    live = 0xFFFFu;
    if (pc < ln.p_end) {
        const uint4 v = *reinterpret_cast<const uint4 *>(ln.base + at);
        w[0] = v.x; w[1] = v.y; w[2] = v.z; w[3] = v.w;
        if (at < ln.lo || at + 16 > ln.hi) {                  // a piece at an end of the line
            live = 0;
#pragma unroll
            for (int k = 0; k < 16; k++) {
                const int64_t o = at + k;
                if (o < ln.lo || o >= ln.hi) w[k >> 2] = (w[k >> 2] & ~(0xFFu << (8 * (k & 3)))) | (0x0Au << (8 * (k & 3)));
                if (o >= ln.lo) live |= 1u << k;
            }
        }
    }
}

// The first line end of the pass as a byte offset from the pass's first piece, INT64_MAX for none; nls = the lane's mask of
// line ends (live bytes only).  Holds ONE __syncthreads(), between the store of the four wave minima and their read: what a
// kernel stores to its own LDS cells in front of the call is visible to the workgroup behind it (tped_parse_kernel's s_tail
// relies on that), and s_end may be written again only behind a further barrier.
__device__ __forceinline__ int64_t text_first_end(uint32_t nls, int64_t s_end[4], int tid)
{
    const int wv = tid >> 6, lane = tid & (WAVE - 1);
    const uint64_t has = __ballot(nls != 0);
    const int my_nl = nls ? __ffs(nls) - 1 : 0;
    const int first_lane = has ? __ffsll((unsigned long long)has) - 1 : 0;
    const int nl_byte = __shfl(my_nl, first_lane, WAVE);
    if (lane == 0) s_end[wv] = has ? (int64_t)(16 * (64 * wv + first_lane) + nl_byte) : INT64_MAX;
    __syncthreads();
    int64_t end = s_end[0];
#pragma unroll
    for (int k = 1; k < 4; k++) end = s_end[k] < end ? s_end[k] : end;
    return end;
}

// no pass follows: the line ended in this one, or its last piece lies in it
__device__ __forceinline__ bool text_last_pass(const TextLine &ln, int64_t p0, int64_t end)
{
    return end != INT64_MAX || p0 + TEXT_PASS_PIECES >= ln.p_end;
}

// the 16-bit mask of the bytes of lane tid's piece that stand in front of the line's end
__device__ __forceinline__ uint32_t text_keep_mask(int64_t end, int tid)
{
    const int64_t mine = 16 * (int64_t)tid;
    return end <= mine ? 0u : end < mine + 16 ? (1u << (int)(end - mine)) - 1u : 0xFFFFu;
}

// The popcount scan of a pass: before = the sum of `count` over the lanes in front of tid, total = over all 256.  Holds ONE
// __syncthreads(), between the store of the four wave totals to s_cells and their read; s_cells may be written again only
// behind a further barrier.
__device__ __forceinline__ void text_block_scan(uint32_t count, uint32_t s_cells[4], int tid, uint32_t &before, uint32_t &total)
{
    const int wv = tid >> 6, lane = tid & (WAVE - 1);
    uint32_t incl = count;
#pragma unroll
    for (int d = 1; d < WAVE; d <<= 1) {
        const uint32_t o = __shfl_up(incl, d, WAVE);
        if (lane >= d) incl += o;
    }
    if (lane == WAVE - 1) s_cells[wv] = incl;
    __syncthreads();
    before = incl - count;
    total = 0;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        if (k < wv) before += s_cells[k];
        total += s_cells[k];
    }
}

// a lane's first offence so far: the minimum over (column << 3 | code); none: ~0
__device__ __forceinline__ void text_offend(unsigned long long &offence, int64_t column, int code)
{
    const unsigned long long key = ((unsigned long long)column << 3) | (unsigned)code;
    offence = key < offence ? key : offence;
}

// The line's first offence over the workgroup (s_offence: ~0 since the kernel's begin) as status[2 r] = its code and
// status[2 r + 1] = its column, clamped to INT32_MAX; a clean line: 0 0.  Holds ONE __syncthreads(), behind the LDS minimum:
// what a kernel stores to LDS in front of the call, lane 0 may read behind it.
__device__ __forceinline__ void text_write_status(unsigned long long *s_offence, unsigned long long offence,
                                                  int32_t *__restrict__ status, int64_t r, int tid)
{
    if (offence != ~0ull) atomicMin(s_offence, offence);
    __syncthreads();
    if (tid == 0) {
        const unsigned long long o = *s_offence;
        const bool clean = o == ~0ull;
        status[2 * r] = clean ? 0 : (int32_t)(o & 7u);
        status[2 * r + 1] = clean ? 0 : (int32_t)((o >> 3) < 0x7FFFFFFFull ? (o >> 3) : 0x7FFFFFFFull);
    }
}

#endif

} // namespace garlic
