// BGZF text on the device (gfx950, wave64): bgzf_inflate_kernel inflates the blocks of a slab, text_lines_* index its lines.
//
// bgzf_inflate_kernel: one wave per BGZF block, four waves per workgroup.  The wave reads the member's header for the
// place of its deflate data (12 + XLEN) and its footer for CRC32 and ISIZE, runs inflate_block (inflate.hpp) with its own
// InflateTables in LDS, then sums the CRC32 of what it wrote, every lane over one 64th of the bytes (crc32_lane_part),
// and writes one status.  A block owns its output range; nothing is shared between blocks, no atomics.
// LDS per workgroup: 4 x 3,968 B of tables + the 1 KB CRC table = 16,896 B, so nine workgroups fit a CU's 160 KB: the LDS
// allows 8 waves per SIMD.  The registers allow 4 (128 VGPRs; bounded to 64 the compiler spills), DESIGN.md says more.
//
// text_lines_*: what text::SlabLines::take gives for a slab, in three launches over tiles of 256 aligned 16-byte pieces:
//   count  per tile: its line ends (text_eq_mask for '\n'), and how many of them end a line that is not blank
//   scan   the exclusive sums of both over the tiles (one workgroup) and the totals
//   write  every line end numbers itself by the popcount scan inside the tile plus the tile's sum: line end j ends line j
//          (`end`, `number`) and starts line j + 1 (`begin`); the slot of either is the count of non-blank lines before it.
//          Whether a line is blank shows in the two bytes at its begin or in front of its end, so no lane needs the
//          line end before its own.  The order is by position, never by arrival.
//   text_heads_kernel gathers the first head_bytes bytes of every line into a dense [lines][head_bytes] buffer, zeros behind
//   a shorter line.
#pragma once
#include "inflate.hpp"
#include "text_line.hpp"

namespace garlic {

constexpr int BGZF_WAVES = 4;                    // blocks per workgroup
constexpr int64_t BGZF_MEMBER_MAX = 65536;       // bytes of a member (BSIZE is 16 bits) and of what it inflates to
constexpr int64_t BGZF_MEMBER_MIN = 12 + 6 + 2 + 8;   // header, the BC subfield, an empty final block, the footer

__global__ __launch_bounds__(64 * BGZF_WAVES, 4) void bgzf_inflate_kernel(const uint8_t *comp, const int64_t *__restrict__ block_begin,
                                                                       int64_t nblocks, uint8_t *out,
                                                                       const int64_t *__restrict__ out_begin, int32_t *__restrict__ status)
{
    __shared__ InflateTables s_tab[BGZF_WAVES];
    __shared__ uint32_t s_crc[256];
    const int tid = threadIdx.x, wv = tid >> 6, lane = tid & (WAVE - 1);
    s_crc[tid] = crc32_table_entry((uint32_t)tid);
    __syncthreads();
    const int64_t blk = (int64_t)blockIdx.x * BGZF_WAVES + wv;
    if (blk >= nblocks) return;
    const int64_t m_at = block_begin[blk], m_bytes = block_begin[blk + 1] - m_at;
    const int64_t o_at = out_begin[blk], o_bytes = out_begin[blk + 1] - o_at;
    int rc = GARLIC_BGZF_OK;
    // the launcher has checked both lists: what follows holds for any pair of them all the same
    if (m_bytes < BGZF_MEMBER_MIN || m_bytes > BGZF_MEMBER_MAX || o_bytes < 0 || o_bytes > BGZF_MEMBER_MAX) rc = GARLIC_BGZF_INPUT_ENDED;
    if (!rc) {
        const uint8_t *m = comp + m_at;
        const uint32_t xlen = (uint32_t)m[10] | (uint32_t)m[11] << 8;
        const int64_t data_at = 12 + (int64_t)xlen;
        if (m[0] != 0x1F || m[1] != 0x8B || m[2] != 8 || m[3] != 4) rc = GARLIC_BGZF_BAD_BLOCK_TYPE;
        else if (data_at + 8 > m_bytes) rc = GARLIC_BGZF_INPUT_ENDED;
        if (!rc) {
            const uint8_t *f = m + m_bytes - 8;
            const uint32_t crc = (uint32_t)f[0] | (uint32_t)f[1] << 8 | (uint32_t)f[2] << 16 | (uint32_t)f[3] << 24;
            const uint32_t isize = (uint32_t)f[4] | (uint32_t)f[5] << 8 | (uint32_t)f[6] << 16 | (uint32_t)f[7] << 24;
            if (isize > (uint32_t)o_bytes) rc = GARLIC_BGZF_OUTPUT_FULL;
            else if (isize < (uint32_t)o_bytes) rc = GARLIC_BGZF_OUTPUT_SHORT;
            if (!rc) rc = inflate_block(m + data_at, (uint32_t)(m_bytes - data_at - 8), out + o_at, (uint32_t)o_bytes, s_tab[wv]);
            if (!rc) {
                uint32_t part = crc32_lane_part(out + o_at, (uint32_t)o_bytes, (uint32_t)lane, WAVE, s_crc);
#pragma unroll
                for (int d = 1; d < WAVE; d <<= 1) part ^= __shfl_xor(part, d, WAVE);
                if ((part ^ 0xFFFFFFFFu) != crc) rc = GARLIC_BGZF_BAD_CRC;
            }
        }
    }
    if (lane == 0) status[blk] = rc;
}

// ---- the line index

constexpr int TEXT_LINES_TILE = 16 * TEXT_PASS_PIECES;       // bytes of a tile

// what the write pass leaves for the host
struct TextLinesResult {
    int64_t newlines, lines, consumed;
    int64_t taken;            // lines of the slab taken, blank ones counted: the line ends, and a last line without one
};

// the line ends of lane tid's piece of a tile, as a 16-bit mask; e0 = the slab offset of the piece's byte 0 (may be < 0)
__device__ __forceinline__ uint32_t text_lines_mask(const uint8_t *text, int64_t n, int64_t tile, int tid, int64_t &e0)
{
    const int64_t shift = (int64_t)((uintptr_t)text & 15);
    const int64_t piece = tile * TEXT_PASS_PIECES + tid;
    e0 = 16 * piece - shift;
    if (e0 >= n || e0 + 16 <= 0) return 0;
    const uint4 v = *reinterpret_cast<const uint4 *>(text + e0);
    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
    uint32_t mask = text_eq_mask(w, 0x0Au);
    if (e0 < 0) mask &= 0xFFFFu << (int)(-e0);
    if (e0 + 16 > n) mask &= 0xFFFFu >> (int)(e0 + 16 - n);
    return mask;
}

// the line that ends at the '\n' of offset e holds more than a '\r'
__device__ __forceinline__ bool text_line_ends_full(const uint8_t *text, int64_t e)
{
    if (e == 0) return false;
    const uint8_t c = text[e - 1];
    if (c == 0x0A) return false;
    return !(c == 0x0D && (e == 1 || text[e - 2] == 0x0A));
}

// the non-blank lines that end in lane tid's piece
__device__ __forceinline__ uint32_t text_lines_full(const uint8_t *text, uint32_t mask, int64_t e0)
{
    uint32_t full = 0;
    for (uint32_t m = mask; m; m &= m - 1) full += text_line_ends_full(text, e0 + (__ffs(m) - 1)) ? 1u : 0u;
    return full;
}

__global__ __launch_bounds__(TEXT_PASS_PIECES) void text_lines_count_kernel(const uint8_t *__restrict__ text, int64_t n,
                                                                            int32_t *__restrict__ tile_newlines, int32_t *__restrict__ tile_full)
{
    __shared__ uint32_t s_a[4], s_b[4];
    const int tid = threadIdx.x;
    int64_t e0;
    const uint32_t mask = text_lines_mask(text, n, blockIdx.x, tid, e0);
    uint32_t before, newlines, full;
    text_block_scan((uint32_t)__popc(mask), s_a, tid, before, newlines);
    text_block_scan(text_lines_full(text, mask, e0), s_b, tid, before, full);
    if (tid == 0) {
        tile_newlines[blockIdx.x] = (int32_t)newlines;
        tile_full[blockIdx.x] = (int32_t)full;
    }
}

// the counts of the tiles into their exclusive sums, in place; the totals into res->newlines and res->lines.  One workgroup.
__global__ __launch_bounds__(TEXT_PASS_PIECES) void text_lines_scan_kernel(int32_t *__restrict__ tile_newlines, int32_t *__restrict__ tile_full,
                                                                           int64_t tiles, TextLinesResult *__restrict__ res)
{
    __shared__ uint32_t s_a[4], s_b[4];
    const int tid = threadIdx.x;
    uint32_t sum_a = 0, sum_b = 0;
    for (int64_t t0 = 0; t0 < tiles; t0 += TEXT_PASS_PIECES) {
        const int64_t t = t0 + tid;
        const uint32_t a = t < tiles ? (uint32_t)tile_newlines[t] : 0u, b = t < tiles ? (uint32_t)tile_full[t] : 0u;
        uint32_t before_a, total_a, before_b, total_b;
        text_block_scan(a, s_a, tid, before_a, total_a);
        text_block_scan(b, s_b, tid, before_b, total_b);
        if (t < tiles) {
            tile_newlines[t] = (int32_t)(sum_a + before_a);
            tile_full[t] = (int32_t)(sum_b + before_b);
        }
        sum_a += total_a;
        sum_b += total_b;
        __syncthreads();                          // the scan cells are written again in the next round
    }
    if (tid == 0) {
        res->newlines = sum_a;
        res->lines = sum_b;
    }
}

// Line `line` (0-based over all lines of the slab, blank ones counted) begins at offset at, behind line end line - 1; `slot` =
// the non-blank lines in front of it.  If it is not blank and ends in the slab -- at a further line end, or at n when
// `last` -- its begin goes to its slot.  The slab's last line (line == newlines) also leaves the result.
__device__ __forceinline__ void text_lines_begin(const uint8_t *text, int64_t n, int last, int64_t seen, int64_t newlines, int64_t line,
                                                 int64_t at, int64_t slot, int64_t cap, int64_t *begin, int64_t *end, int64_t *number,
                                                 TextLinesResult *res)
{
    if (line < newlines) {
        const uint8_t c = text[at];               // in the slab: a line end stands at or behind it
        if (c != 0x0A && !(c == 0x0D && text[at + 1] == 0x0A) && slot < cap) begin[slot] = at;
        return;
    }
    const bool tail = last && at < n && !(n == at + 1 && text[at] == 0x0D);
    if (tail && slot < cap) {
        begin[slot] = at;
        end[slot] = n;
        number[slot] = seen + line + 1;
    }
    res->lines = slot + (tail ? 1 : 0);
    res->consumed = last ? n : at;
    res->taken = newlines + (last && at < n ? 1 : 0);
}

// cap = the room of begin / end / number: the count pass's total + 1
__global__ __launch_bounds__(TEXT_PASS_PIECES) void text_lines_write_kernel(const uint8_t *__restrict__ text, int64_t n, int last, int64_t seen,
                                                                            const int32_t *__restrict__ tile_newlines,
                                                                            const int32_t *__restrict__ tile_full, int64_t newlines, int64_t cap,
                                                                            int64_t *__restrict__ begin, int64_t *__restrict__ end,
                                                                            int64_t *__restrict__ number, TextLinesResult *__restrict__ res)
{
    __shared__ uint32_t s_a[4], s_b[4];
    const int tid = threadIdx.x;
    int64_t e0;
    const uint32_t mask = text_lines_mask(text, n, blockIdx.x, tid, e0);
    uint32_t before_a, before_b, total;
    text_block_scan((uint32_t)__popc(mask), s_a, tid, before_a, total);
    text_block_scan(text_lines_full(text, mask, e0), s_b, tid, before_b, total);
    int64_t line = (int64_t)tile_newlines[blockIdx.x] + before_a;         // the line that the next line end ends
    int64_t slot = (int64_t)tile_full[blockIdx.x] + before_b;
    if (blockIdx.x == 0 && tid == 0) text_lines_begin(text, n, last, seen, newlines, 0, 0, 0, cap, begin, end, number, res);
    for (uint32_t m = mask; m; m &= m - 1) {
        const int64_t e = e0 + (__ffs(m) - 1);
        if (text_line_ends_full(text, e)) {
            if (slot < cap) {
                end[slot] = e;
                number[slot] = seen + line + 1;
            }
            slot++;
        }
        line++;
        text_lines_begin(text, n, last, seen, newlines, line, e + 1, slot, cap, begin, end, number, res);
    }
}

// heads[k][0, head_bytes) = the first bytes of line k, zeros behind a shorter line; one lane per byte of the heads
__global__ __launch_bounds__(256) void text_heads_kernel(const uint8_t *__restrict__ text, const int64_t *__restrict__ begin,
                                                         const int64_t *__restrict__ end, int64_t cap, const TextLinesResult *__restrict__ res,
                                                         int64_t head_bytes, int64_t n, uint8_t *__restrict__ heads)
{
    const int64_t lines = res->lines < cap ? res->lines : cap;
    const int64_t total = lines * head_bytes;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t k = i / head_bytes, o = i - k * head_bytes;
        const int64_t b = begin[k], e = end[k] < n ? end[k] : n;            // inside the slab whatever the lists hold
        heads[i] = b >= 0 && o < e - b ? text[b + o] : (uint8_t)0;
    }
}

} // namespace garlic
