// VCF text -> the staged rows of a garlic_tgls object (gfx950, wave64): one scalar FORMAT subfield per sample column.
//
// A data line of a VCF is eight tab-separated columns, FORMAT (column 8: keys joined by ':') and one column per sample,
// whose subfields stand in FORMAT's order.  The line ends at its first '\r' or '\n', at the next line_begin or at text_bytes.
// k = the index of the first FORMAT subfield that equals the key bytewise, decided per line; sample j is column 9 + j and its
// value is subfield k of the column: the bytes between the column's k-th ':' and the next ':' or the column's end.  The value
// is MISSING when the column has fewer than k colons, when the subfield is empty and when it is exactly ".".  Any other
// subfield of a kept column goes through tgls_number (at most TGLS_TOKEN_MAX bytes); what that leaves open is
// TGLS_DEFERRED, as for --tgls text.  A missing value becomes 0.0, or the caller's missing value, where the column starts
// with '.' (a missing genotype: no score reads the value); on any other column it becomes the caller's missing value or,
// when the caller gave none, the offence TGLS_VCF_NO_VALUE.  Columns that are not kept are counted and nothing else.
//
// tgls_vcf_parse_kernel: one workgroup of 256 lanes per line; the line goes through it in passes of 256 aligned 16-byte
// pieces (4 KB), every piece read from HBM once:
//   1, 2. the line walk of text_line.hpp with the masks of the tabs, the colons and the stops (tab : \r \n); the first \r or
//      \n ends the line, and tabs and colons at or behind it are dropped;
//   3. column starts = the bytes behind a tab (the tab of a piece's last byte starts a column in the next slot: read from LDS).
//      A segmented scan over the pieces with the element (column starts, colons at or behind the last start, has a start,
//      the last start's byte is '.') -- __shfl_up inside a wave, the four wave totals through LDS, the state of the passes
//      before in registers -- gives every piece the state at its first byte: column, colons of that column so far, and
//      whether the column began with '.';
//   4. the pieces and their masks stand in LDS as slots 3 .. 258; slots 0 .. 2 are the previous pass's last three and slots
//      259 .. 261 are all stops.  A lane walks the column starts and colons of its slot in order.  In column 8 every subfield
//      start is compared with the key and the lowest matching index is an LDS minimum: k.  Behind a barrier the same walk
//      handles the samples: a column start closes the column in front (fewer than k colons: missing), and the colon that
//      makes the count k is followed by the value.  The value's length is the distance to the next stop in the masks of the
//      slot and the three behind it, so a value of TGLS_TOKEN_MAX bytes that starts behind the slot's last byte is seen whole
//      (16 + 32 < 64): that is why the walk runs three slots behind the load and why no byte is loaded twice.  Every FORMAT
//      subfield lies in front of every sample, so k is known wherever a sample needs it;
//   5. a kept column's double is stored with a plain 8-byte vector store at raw[row][col_dest[j]];
//   6. behind the last pass lane 0 closes the line's last column.  A tab that is the line's last byte starts an empty column
//      behind it, as for every tab; where that tab is also the last byte of the pass and the line ends by its limit, the
//      column's first byte lies in a slot that no lane holds, and lane 0 opens and counts it before it closes the line.
// The first offence of the line is a 64-bit minimum in LDS over (sample column << 3 | code): independent of arrival order.  No
// global atomics; a staging row is written by one workgroup only.  No switch point: any line length, subfield width and
// sample count take this one path.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "lod_kernels.hpp"
#include "text_line.hpp"
#include "tgls_kernels.hpp"

namespace garlic {

constexpr int TGLS_VCF_NO_KEY = 4;      // FORMAT does not name the key; column 0
constexpr int TGLS_VCF_NO_VALUE = 5;    // a called genotype without a value and no missing value to take; column = the sample

constexpr int VGL_KEY_MAX = 16;
constexpr int VGL_CARRY = 3;                                    // slots a value may reach behind the one its colon stands in
constexpr int VGL_SLOTS = TEXT_PASS_PIECES + 2 * VGL_CARRY;
constexpr uint32_t VGL_NO_KEY = 0xFFFFFFFFu;
static_assert(16 + TGLS_TOKEN_MAX < 16 * (VGL_CARRY + 1), "a value behind a slot's last byte ends inside the look-ahead");
static_assert(16 + VGL_KEY_MAX < 16 * (VGL_CARRY + 1), "and so does a FORMAT subfield as long as the longest key");

// the element of the segmented scan: n column starts, cc colons at or behind the last of them (all colons when n == 0),
// dot: the last start's byte is '.' (read only when n > 0)
struct VglSeg {
    uint32_t n, cc, dot;
};

__device__ __forceinline__ VglSeg vgl_join(const VglSeg &a, const VglSeg &b)      // a in front of b
{
    VglSeg r;
    r.n = a.n + b.n;
    r.cc = b.n ? b.cc : a.cc + b.cc;
    r.dot = b.n ? b.dot : a.dot;
    return r;
}

__global__ void __launch_bounds__(256)
tgls_vcf_parse_kernel(const uint8_t *__restrict__ text, int64_t text_bytes, const int64_t *__restrict__ line_begin, int32_t ncols,
                      const int32_t *__restrict__ col_dest, uint64_t key_lo, uint64_t key_hi, int32_t key_len, double missing_value,
                      int32_t has_missing, double *__restrict__ raw, int64_t raw_ld, int32_t *__restrict__ status)
{
    __shared__ __attribute__((aligned(16))) uint8_t s_text[VGL_SLOTS * 16];
    __shared__ uint32_t s_stop[VGL_SLOTS];        // tab : \r \n and what lies outside the line
    __shared__ uint32_t s_tab[VGL_SLOTS];
    __shared__ uint32_t s_ev[VGL_SLOTS];          // column starts | colons << 16
    __shared__ int64_t s_col[VGL_SLOTS];          // the state at the slot's first byte: column starts in front of it,
    __shared__ uint32_t s_cc[VGL_SLOTS];          // colons of the open column in front of it,
    __shared__ uint32_t s_dot[VGL_SLOTS];         // the open column began with '.'
    __shared__ int64_t s_end[4];
    __shared__ uint32_t s_wn[4], s_wcc[4], s_wdot[4];
    __shared__ uint32_t s_k;
    __shared__ unsigned long long s_offence;

    const int tid = threadIdx.x, wv = tid >> 6, lane = tid & (WAVE - 1);
    const int64_t r = blockIdx.x;
    const TextLine ln = text_line_of(text, text_bytes, line_begin, r);

    if (tid == 0) {
        s_offence = ~0ull;
        s_k = VGL_NO_KEY;
    }
    if (tid < 2 * VGL_CARRY) {                                // the carry slots in front and the stop slots behind
        const int slot = tid < VGL_CARRY ? tid : TEXT_PASS_PIECES + tid;
        *reinterpret_cast<uint4 *>(s_text + 16 * slot) = make_uint4(0x0A0A0A0Au, 0x0A0A0A0Au, 0x0A0A0A0Au, 0x0A0A0A0Au);
        s_stop[slot] = 0xFFFFu;
        s_tab[slot] = 0;
        s_ev[slot] = 0;
        s_col[slot] = 0;
        s_cc[slot] = 0;
        s_dot[slot] = 0;
    }
    double *raw_row = raw + r * raw_ld;
    unsigned long long offence = ~0ull;
    const auto offend = [&](int64_t column, int code) { text_offend(offence, column, code); };
    // a missing value of sample j, whose column began with '.' (dot) or did not
    const auto missing = [&](int64_t j, uint32_t dot) {
        const int32_t d = col_dest[j];
        if (d < 0) return;
        if (has_missing) raw_row[d] = missing_value;
        else if (dot) raw_row[d] = 0.0;
        else offend(j, TGLS_VCF_NO_VALUE);
    };
    int64_t col = 0;              // the state at the pass's first byte, as in s_col / s_cc / s_dot
    uint32_t ccarry = 0, dcarry = 0;
    bool ended = false;
    for (int64_t p0 = ln.p_first; !ended; p0 += TEXT_PASS_PIECES) {
        __syncthreads();          // the previous pass has let go of the slots and the scan cells
        uint32_t w[4], live;
        text_load_piece(ln, p0 + tid, w, live);
        const int me = tid + VGL_CARRY;
        *reinterpret_cast<uint4 *>(s_text + 16 * me) = make_uint4(w[0], w[1], w[2], w[3]);
        uint32_t tabs = text_eq_mask(w, '\t'), colons = text_eq_mask(w, ':');
        const uint32_t ends = text_eq_mask(w, '\n') | text_eq_mask(w, '\r');
        s_stop[me] = tabs | colons | ends;
        const int64_t end = text_first_end(ends & live, s_end, tid);
        const bool last = text_last_pass(ln, p0, end);
        // tabs and colons at or behind the line's end are none
        const uint32_t keep = text_keep_mask(end, tid);
        tabs &= keep;
        colons &= keep;
        s_tab[me] = tabs;
        __syncthreads();
        const uint32_t cs = ((tabs << 1) | (s_tab[me - 1] >> 15)) & 0xFFFFu;      // the bytes behind a tab
        VglSeg own;
        own.n = __popc(cs);
        own.cc = __popc(cs ? colons & ~((1u << (31 - __clz(cs))) - 1u) : colons);
        own.dot = 0;
        if (cs) {
            const int q = 31 - __clz(cs);
            own.dot = ((w[q >> 2] >> (8 * (q & 3))) & 0xFFu) == '.' ? 1u : 0u;
        }
        VglSeg incl = own;
#pragma unroll
        for (int d = 1; d < WAVE; d <<= 1) {
            VglSeg o;
            o.n = __shfl_up(incl.n, d, WAVE);
            o.cc = __shfl_up(incl.cc, d, WAVE);
            o.dot = __shfl_up(incl.dot, d, WAVE);
            if (lane >= d) incl = vgl_join(o, incl);
        }
        if (lane == WAVE - 1) {
            s_wn[wv] = incl.n;
            s_wcc[wv] = incl.cc;
            s_wdot[wv] = incl.dot;
        }
        VglSeg excl;              // the pieces of the wave in front of this one
        excl.n = __shfl_up(incl.n, 1, WAVE);
        excl.cc = __shfl_up(incl.cc, 1, WAVE);
        excl.dot = __shfl_up(incl.dot, 1, WAVE);
        if (lane == 0) excl.n = excl.cc = excl.dot = 0;
        __syncthreads();
        VglSeg before, total;     // the state at the wave's first byte and behind the pass, both within the pass
        before.n = before.cc = before.dot = 0;
        total = before;
#pragma unroll
        for (int k = 0; k < 4; k++) {
            VglSeg wk;
            wk.n = s_wn[k];
            wk.cc = s_wcc[k];
            wk.dot = s_wdot[k];
            if (k < wv) before = vgl_join(before, wk);
            total = vgl_join(total, wk);
        }
        before = vgl_join(before, excl);
        s_ev[me] = cs | (colons << 16);
        s_col[me] = col + before.n;
        s_cc[me] = before.n ? before.cc : ccarry + before.cc;
        s_dot[me] = before.n ? before.dot : dcarry;
        col += total.n;
        ccarry = total.n ? total.cc : ccarry + total.cc;
        dcarry = total.n ? total.dot : dcarry;
        __syncthreads();
        // walk slots 0 .. 255 (and slots 256 .. 258 when no pass follows)
        const int nslots = last ? TEXT_PASS_PIECES + VGL_CARRY : TEXT_PASS_PIECES;
        // FORMAT: the subfield starts of column 8 against the key
        for (int slot = tid; slot < nslots; slot += 256) {
            uint32_t ev = s_ev[slot];
            int64_t c = s_col[slot];
            if (!ev || c > 8 || c + __popc(ev & 0xFFFFu) < 8) continue;
            uint32_t cc = s_cc[slot];
            const uint64_t stop = (uint64_t)s_stop[slot] | ((uint64_t)s_stop[slot + 1] << 16) | ((uint64_t)s_stop[slot + 2] << 32) |
                                  ((uint64_t)s_stop[slot + 3] << 48);
            uint32_t m = (ev | (ev >> 16)) & 0xFFFFu;
            while (m) {
                const int q = __ffs(m) - 1;
                m &= m - 1;
                int at_byte = -1;                             // where a subfield of column 8 starts, index cc
                if ((ev >> q) & 1u) {
                    c++;
                    cc = 0;
                    if (c == 8) at_byte = q;
                }
                if ((ev >> (16 + q)) & 1u) {
                    cc++;
                    if (c == 8) at_byte = q + 1;              // (a column that starts with ':' has an empty subfield 0: no key)
                }
                if (at_byte < 0) continue;
                const uint64_t rest = stop >> at_byte;
                const int len = rest ? __ffsll((unsigned long long)rest) - 1 : 64;
                if (len != key_len) continue;
                const uint8_t *f = s_text + 16 * slot + at_byte;
                bool same = true;
                for (int i = 0; i < key_len; i++) {
                    const uint32_t kb = (uint32_t)((i < 8 ? key_lo >> (8 * i) : key_hi >> (8 * (i - 8))) & 0xFFu);
                    same = same && f[i] == kb;
                }
                if (same) atomicMin(&s_k, cc);
            }
        }
        __syncthreads();
        const uint32_t k = s_k;
        // the samples
        for (int slot = tid; slot < nslots; slot += 256) {
            uint32_t ev = s_ev[slot];
            if (!ev) continue;
            int64_t c = s_col[slot];
            if (c + __popc(ev & 0xFFFFu) < 9) continue;
            uint32_t cc = s_cc[slot], dot = s_dot[slot];
            const uint64_t stop = (uint64_t)s_stop[slot] | ((uint64_t)s_stop[slot + 1] << 16) | ((uint64_t)s_stop[slot + 2] << 32) |
                                  ((uint64_t)s_stop[slot + 3] << 48);
            uint32_t m = (ev | (ev >> 16)) & 0xFFFFu;
            while (m) {
                const int q = __ffs(m) - 1;
                m &= m - 1;
                int at_byte = -1;                             // where the value of sample c - 9 starts
                if ((ev >> q) & 1u) {
                    const int64_t jc = c - 9;                 // the column in front closes here
                    if (jc >= 0 && jc < ncols && k != VGL_NO_KEY && cc < k) missing(jc, dot);
                    c++;
                    cc = 0;
                    dot = s_text[16 * slot + q] == '.' ? 1u : 0u;
                    if (c - 9 >= ncols) offend(ncols, TGLS_MANY_COLUMNS);
                    else if (c >= 9 && k == 0) at_byte = q;
                }
                if ((ev >> (16 + q)) & 1u) {
                    cc++;
                    if (c >= 9 && c - 9 < ncols && cc == k) at_byte = q + 1;
                }
                if (at_byte < 0) continue;
                const int64_t j = c - 9;
                const int32_t d = col_dest[j];
                if (d < 0) continue;
                const uint64_t rest = stop >> at_byte;
                const int len = rest ? __ffsll((unsigned long long)rest) - 1 : 64;
                const uint8_t *f = s_text + 16 * slot + at_byte;
                if (len == 0 || (len == 1 && f[0] == '.')) {
                    missing(j, dot);
                    continue;
                }
                double v = 0.0;
                if (len <= TGLS_TOKEN_MAX && tgls_number(f, len, &v)) raw_row[d] = v;
                else offend(j, TGLS_DEFERRED);
            }
        }
        __syncthreads();
        if (last) {
            if (tid == 0) {
                if (end == INT64_MAX && (s_tab[TEXT_PASS_PIECES + VGL_CARRY - 1] >> 15)) {
                    // the line ends by `limit` behind a tab that is the pass's last byte: the empty column it starts lies in
                    // a slot no lane holds.  It closes the column in front and is counted here.
                    const int64_t jf = col - 9;
                    if (jf >= 0 && jf < ncols && k != VGL_NO_KEY && ccarry < k) missing(jf, dcarry);
                    col++;
                    ccarry = dcarry = 0;
                    if (col - 9 >= ncols) offend(ncols, TGLS_MANY_COLUMNS);
                    else if (col >= 9 && k == 0) missing(col - 9, 0);
                }
                const int64_t jc = col - 9;                   // the line's end closes its last column
                if (jc >= 0 && jc < ncols && k != VGL_NO_KEY && ccarry < k) missing(jc, dcarry);
                const int64_t found = col >= 8 ? col - 8 : 0;
                if (found < ncols) offend(found, TGLS_FEW_COLUMNS);
                if (k == VGL_NO_KEY) offend(0, TGLS_VCF_NO_KEY);
            }
        } else if (tid < VGL_CARRY) {
            const int from = TEXT_PASS_PIECES + tid;
            *reinterpret_cast<uint4 *>(s_text + 16 * tid) = *reinterpret_cast<const uint4 *>(s_text + 16 * from);
            s_stop[tid] = s_stop[from];
            s_tab[tid] = s_tab[from];
            s_ev[tid] = s_ev[from];
            s_col[tid] = s_col[from];
            s_cc[tid] = s_cc[from];
            s_dot[tid] = s_dot[from];
        }
        ended = last;
    }
    text_write_status(&s_offence, offence, status, r, tid);
}

} // namespace garlic
