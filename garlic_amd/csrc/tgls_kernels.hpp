// --tgls text -> the rows of a garlic_tgls object (gfx950, wave64): the parser, the dictionary coder and what reads the codes.
//
// A line of a --tgls file is four leading columns (chromosome, id, genetic and physical position) and then one number per
// individual, separated as operator>> and countFields of the reader separate them: by runs of isspace() bytes (space, \t, \v,
// \f, \r; the '\n' ends the line), with leading and trailing runs allowed.  A token starts at a non-blank byte whose predecessor
// is blank or the line's begin; token 4 + j is sample column j.
//
// tgls_parse_kernel: one workgroup of 256 lanes per line; the line goes through it in passes of 256 aligned 16-byte pieces
// (4 KB), every piece read from HBM once:
//   1, 2. the line walk of text_line.hpp with the masks of the non-blank bytes and the newlines; the first newline ends the line
//      and what lies behind it is blank;
//   3. start mask = non-blank and predecessor blank (the predecessor of a piece's first byte is the last byte of the slot in
//      front, read from LDS); popcount through text_block_scan: the token index of each piece's first start;
//   4. the pieces and their masks stand in LDS as slots 2 .. 257; slots 0 and 1 are the previous pass's last two pieces and slots
//      258, 259 are blank.  A lane decodes the tokens that START in its slot.  A token's length is the distance to the next
//      blank in the non-blank masks of the slot and the two behind it, so a token of up to TGLS_TOKEN_MAX = 32 bytes that starts
//      at the slot's last byte is seen whole (15 + 32 < 48): that is the look-ahead, and a longer token is deferred.  That is
//      why the decode runs two slots behind the load (slots 256, 257 are decoded as slots 0, 1 of the next pass, or in the last
//      pass itself) and why no byte is loaded twice;
//   5. a kept column's token (col_dest[j] >= 0, read once per token) goes through tgls_number (tgls_number.hpp); its double is
//      stored with a plain 8-byte vector store at raw[row][col_dest[j]].  A token of a column that is not kept is not read.
// The first offence of the line is a 64-bit minimum in LDS over (sample column << 3 | code): independent of arrival order.  No
// global atomics; a staging row is written by one workgroup only.  No switch point: any line length, field width and column
// count take this one path.
//
// tgls_encode_kernel: staged doubles -> uint16 codes by binary search of the bit pattern in the object's sorted table (global
// memory, 512 KB at most, 16 probes); a value the table does not hold joins a set of unknowns (open addressing in global memory,
// 2 x the code space, compare-and-swap on the report path only), from which the host extends the table, and the rows run again.
// The SET of a slab's unknown values does not depend on the order the lanes arrive in, and the host sorts it: code numbers are
// a function of the file and the slab boundaries alone.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "lod_kernels.hpp"
#include "text_line.hpp"
#include "tgls_number.hpp"

namespace garlic {

constexpr int TGLS_OK = 0;
constexpr int TGLS_DEFERRED = 1;        // a token tgls_number leaves to the host; column = its sample column
constexpr int TGLS_FEW_COLUMNS = 2;     // column = the number of sample columns the line has
constexpr int TGLS_MANY_COLUMNS = 3;    // column = ncols_total

constexpr int TGLS_CARRY = 2;                                   // slots a token may reach behind the one it starts in
constexpr int TGLS_SLOTS = TEXT_PASS_PIECES + 2 * TGLS_CARRY;
static_assert(15 + TGLS_TOKEN_MAX < 16 * (TGLS_CARRY + 1), "a token that starts at a slot's last byte ends inside the look-ahead");

constexpr int TGLS_DICT_MAX = 65536;
constexpr uint32_t TGLS_SET_SLOTS = 2u * TGLS_DICT_MAX;         // the set of unknown values: a power of two
constexpr uint32_t TGLS_PROBE_MAX = 1024;                        // probes of one element (a half-full set needs a few)
constexpr uint64_t TGLS_SET_EMPTY = ~0ull;                      // (a NaN no text parses to; reported through flags[1])

// the 16-bit mask of the bytes of a piece that isspace() calls blank
__device__ __forceinline__ uint32_t tgls_blank_mask(const uint32_t w[4])
{
    uint32_t m = 0;
#pragma unroll
    for (int k = 0; k < 16; k++) {
        const uint32_t c = (w[k >> 2] >> (8 * (k & 3))) & 0xFFu;
        m |= ((c == ' ' || (c - 9u) <= 4u) ? 1u : 0u) << k;
    }
    return m;
}

__global__ void __launch_bounds__(256)
tgls_parse_kernel(const uint8_t *__restrict__ text, int64_t text_bytes, const int64_t *__restrict__ line_begin, int32_t ncols,
                  const int32_t *__restrict__ col_dest, double *__restrict__ raw, int64_t raw_ld, int32_t *__restrict__ status)
{
    __shared__ __attribute__((aligned(16))) uint8_t s_text[TGLS_SLOTS * 16];
    __shared__ uint32_t s_nb[TGLS_SLOTS];         // non-blank bytes of the slot that belong to the line
    __shared__ uint32_t s_start[TGLS_SLOTS];
    __shared__ int64_t s_tok[TGLS_SLOTS];         // tokens of the line that start in front of the slot
    __shared__ int64_t s_end[4];
    __shared__ uint32_t s_cnt[4];
    __shared__ unsigned long long s_offence;

    const int tid = threadIdx.x;
    const int64_t r = blockIdx.x;
    const TextLine ln = text_line_of(text, text_bytes, line_begin, r);

    if (tid == 0) s_offence = ~0ull;
    if (tid < 2 * TGLS_CARRY) {                               // the carry slots in front and the blank slots behind
        const int slot = tid < TGLS_CARRY ? tid : TEXT_PASS_PIECES + tid;
        *reinterpret_cast<uint4 *>(s_text + 16 * slot) = make_uint4(0x0A0A0A0Au, 0x0A0A0A0Au, 0x0A0A0A0Au, 0x0A0A0A0Au);
        s_nb[slot] = 0;
        s_start[slot] = 0;
        s_tok[slot] = 0;
    }
    double *raw_row = raw + r * raw_ld;
    unsigned long long offence = ~0ull;
    int64_t tok = 0;              // tokens of the line that start in front of this pass
    bool ended = false;
    for (int64_t p0 = ln.p_first; !ended; p0 += TEXT_PASS_PIECES) {
        __syncthreads();          // the previous pass has let go of the slots and the scan cells
        uint32_t w[4], live;
        text_load_piece(ln, p0 + tid, w, live);
        *reinterpret_cast<uint4 *>(s_text + 16 * (tid + TGLS_CARRY)) = make_uint4(w[0], w[1], w[2], w[3]);
        const int64_t end = text_first_end(text_eq_mask(w, '\n') & live, s_end, tid);
        const bool last = text_last_pass(ln, p0, end);
        // what lies behind the line's end is blank
        const uint32_t nb = ~tgls_blank_mask(w) & text_keep_mask(end, tid);
        s_nb[tid + TGLS_CARRY] = nb;
        __syncthreads();
        const uint32_t prev = s_nb[tid + TGLS_CARRY - 1] >> 15;       // the byte in front of the piece is part of a token
        const uint32_t start = nb & ~((nb << 1) | prev) & 0xFFFFu;
        uint32_t before, pass_starts;
        text_block_scan(__popc(start), s_cnt, tid, before, pass_starts);
        s_start[tid + TGLS_CARRY] = start;
        s_tok[tid + TGLS_CARRY] = tok + before;
        tok += pass_starts;
        __syncthreads();
        // decode the tokens that start in slots 0 .. 255 (and in slots 256, 257 when no pass follows)
        const int nslots = last ? TEXT_PASS_PIECES + TGLS_CARRY : TEXT_PASS_PIECES;
        for (int slot = tid; slot < nslots; slot += 256) {
            uint32_t m = s_start[slot];
            if (!m) continue;
            int64_t t = s_tok[slot];
            const uint64_t run = (uint64_t)s_nb[slot] | ((uint64_t)s_nb[slot + 1] << 16) | ((uint64_t)s_nb[slot + 2] << 32);
            while (m) {
                const int q = __ffs(m) - 1;
                m &= m - 1;
                const int64_t j = t - 4;                      // the sample column of the token that starts at byte q
                t++;
                if (j < 0) continue;
                if (j >= ncols) {
                    text_offend(offence, ncols, TGLS_MANY_COLUMNS);
                    continue;
                }
                const int32_t d = col_dest[j];
                if (d < 0) continue;
                const int len = __ffsll((unsigned long long)~(run >> q)) - 1;      // <= 48 - q: the bits past the three slots are clear
                double v = 0.0;
                if (len <= TGLS_TOKEN_MAX && tgls_number(s_text + 16 * slot + q, len, &v)) {
                    raw_row[d] = v;
                } else {
                    text_offend(offence, j, TGLS_DEFERRED);
                }
            }
        }
        __syncthreads();
        if (last) {
            const int64_t found = tok > 4 ? tok - 4 : 0;
            if (found < ncols) text_offend(offence, found, TGLS_FEW_COLUMNS);
        } else if (tid < TGLS_CARRY) {
            const int from = TEXT_PASS_PIECES + tid;
            *reinterpret_cast<uint4 *>(s_text + 16 * tid) = *reinterpret_cast<const uint4 *>(s_text + 16 * from);
            s_nb[tid] = s_nb[from];
            s_start[tid] = s_start[from];
            s_tok[tid] = s_tok[from];
        }
        ended = last;
    }
    text_write_status(&s_offence, offence, status, r, tid);
}

__device__ __forceinline__ uint32_t tgls_hash(uint64_t b)
{
    b ^= b >> 33;
    b *= 0xff51afd7ed558ccdull;
    b ^= b >> 33;
    return (uint32_t)b;
}

// Staged rows raw[row_count][raw_ld] -> codes[row_count][n_kept] (the object's rows from row_begin on).  Kept column k reads
// the staged column k_src[k] (a column index named twice is staged once); k_src == NULL: column k.  Rows whose status code is
// not TGLS_OK are skipped (status == NULL: none is).  flags[0]: distinct unknown values put into `set`; flags[1]: the value
// TGLS_SET_EMPTY itself is unknown; flags[2]: a value found no slot within TGLS_PROBE_MAX probes.  room = the codes the dictionary
// has left: once flags[0] passes it the call is refused whatever else comes, so an element that sees that does nothing more.
// The work of the report path is bounded: while flags[0] <= room the set is at most half full (probe runs of a few slots),
// and what the lanes in flight put in beyond that costs each of them TGLS_PROBE_MAX probes at the most.
__global__ void __launch_bounds__(256)
tgls_encode_kernel(const double *__restrict__ raw, int64_t raw_ld, const int32_t *__restrict__ status, int64_t row_count, int32_t n_kept,
                   const int32_t *__restrict__ k_src, const uint64_t *__restrict__ dict_bits, const uint16_t *__restrict__ dict_code,
                   int ndict, uint16_t *__restrict__ codes, unsigned long long *__restrict__ set, int32_t room, int32_t *__restrict__ flags)
{
    const int64_t n = row_count * n_kept;
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += (int64_t)gridDim.x * blockDim.x) {
        const int64_t r = e / n_kept;
        const int64_t k = e - r * n_kept;
        if (status && status[2 * r] != TGLS_OK) continue;
        const uint64_t b = reinterpret_cast<const uint64_t *>(raw)[r * raw_ld + (k_src ? k_src[k] : k)];
        int lo = 0, hi = ndict;                                 // first entry >= b
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (dict_bits[mid] < b) lo = mid + 1; else hi = mid;
        }
        if (lo < ndict && dict_bits[lo] == b) {
            codes[e] = dict_code[lo];
            continue;
        }
        if (b == TGLS_SET_EMPTY) {
            flags[1] = 1;
            continue;
        }
        // the outcome is decided once more unknown values are counted than the dictionary has room for: no further work then
        if (*reinterpret_cast<volatile int32_t *>(flags) > room) continue;
        uint32_t h = tgls_hash(b) & (TGLS_SET_SLOTS - 1);
        uint32_t probe = 0;
        for (; probe < TGLS_PROBE_MAX; probe++) {
            const unsigned long long old = atomicCAS(set + h, (unsigned long long)TGLS_SET_EMPTY, (unsigned long long)b);
            if (old == TGLS_SET_EMPTY) {
                atomicAdd(flags, 1);
                break;
            }
            if (old == b) break;
            h = (h + 1) & (TGLS_SET_SLOTS - 1);
        }
        if (probe == TGLS_PROBE_MAX) flags[2] = 1;             // the value is in no slot: the host must not take the set for complete
    }
}

// out[row_count][ld] = table[codes[row][k]]: what garlic_tgls_get_rows answers (table: the raw values or the converted ones)
__global__ void __launch_bounds__(256)
tgls_decode_kernel(const uint16_t *__restrict__ codes, int64_t row_count, int32_t n_kept, const double *__restrict__ table,
                   double *__restrict__ out, int64_t ld)
{
    const int64_t n = row_count * n_kept;
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += (int64_t)gridDim.x * blockDim.x) {
        const int64_t r = e / n_kept;
        out[r * ld + (e - r * n_kept)] = table[codes[e]];
    }
}

// used[c] = 1 for every code c among the n codes (plain byte stores of the same value: the order does not matter)
__global__ void __launch_bounds__(256)
tgls_mark_kernel(const uint16_t *__restrict__ codes, int64_t n, uint8_t *__restrict__ used)
{
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += (int64_t)gridDim.x * blockDim.x) used[codes[e]] = 1;
}

// The kept rows of the object, compacted for a panel: out[k][i] = map[codes[src_row[k]][ind_offset + i]], k < nrows_out,
// i < nind, as Code = uint8_t (the one-byte door) or uint16_t; map: the object's code -> the code of its converted value.
template <class Code>
__global__ void __launch_bounds__(256)
tgls_compact_kernel(const uint16_t *__restrict__ codes, int32_t n_kept, const int64_t *__restrict__ src_row, int64_t nrows_out,
                    int64_t ind_offset, int32_t nind, const uint16_t *__restrict__ map, Code *__restrict__ out)
{
    const int64_t n = nrows_out * nind;
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += (int64_t)gridDim.x * blockDim.x) {
        const int64_t k = e / nind;
        const int64_t i = e - k * nind;
        out[e] = (Code)map[codes[src_row[k] * n_kept + ind_offset + i]];
    }
}

} // namespace garlic
