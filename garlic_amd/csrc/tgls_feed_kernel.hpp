// TGLS chain for the KDE feed: the ring chain of tgls_ring_kernel.hpp storing only the sampled windows.
//
// convertWinData2DoubleData (src/garlic-data.cpp:2026-2069) looks at the windows at chromosome-local loci
// 0, step, 2 * step, .. and nothing else.  A TGLS window is a rolling sum (acc = (acc - t_out) + t_in,
// src/garlic-roh.cpp:89-102), so every window of a run is still computed, in order, with the same two rounded
// operations -- the sampled values are bit-identical to the full scores -- but nothing behind the add is kept:
// no transposed write-out of 8 B per window, no full-size score scratch, no strided passes over it.  Algorithmically
// the kernel reads 8 B of terms per window and writes 8 / step B (the samples are isolated 8-byte words, one per row
// of the thinned matrix, so the sectors HBM really writes are more; FETCH / WRITE counters were not collected).
//
//   * work items, queue, loaders: those of lod_chain_ring_kernel, unchanged (tg_loader; LOAD0 / LOAD1 stream
//     every 512-B term row through the LDS ring once, by LDS-DMA; a loader publishes what has landed before it
//     blocks on ring room).  The ring keeps its TG_RING rows and with them the switch to the two-stream form
//     at W > TG_SINGLE_MAX_W.  Of the 34 KB the two transpose tiles of the score kernel take, 17 KB stay here
//     as the sample patch; the other 17 KB would buy 32 more rows (the switch at W = 177 instead of 145).  A
//     deeper ring was not measured for this kernel, so the depth is simply the score kernel's; one ring size
//     also keeps one set of boundaries for the tests of both kernels.
//   * CHAIN: a tile of 32 windows that holds no sampled locus (two in three at step = 100) is the bare
//     recurrence.  A tile that holds one puts its 32 scores into one wave-private 64 x 32 patch in LDS and picks
//     the sampled columns out of it: one lane-strided store per sample (lane = individual = row of the thinned
//     matrix, column = locus / step).  At step = W = 100 that is one vector-memory instruction per 100 windows
//     of the chain wave.  Collecting the samples for a fourth wave to write out in whole-row pieces was not
//     built (three waves per workgroup here), so the two were not timed against each other.  Measured against the
//     full-score path (profiles/tgls_feed_ab.txt): kernel 1.2 - 1.5 x faster at step = W = 10 .. 300, level at
//     steps 4 - 6, where the stores (8 per tile at step 4) cost what the missing write-out saved; the call is
//     shorter at every step >= 4 because the flatten passes shrink with the matrix.
//   * the thinned matrix make_layout(p, 32, nind, step) is filled with -9999.0 in front of the launch, as for
//     lod_feed_kernel: the kernel overwrites the sampled loci that hold a window.
#pragma once
#include "tgls_ring_kernel.hpp"

namespace garlic {

constexpr int TGF_THREADS = 3 * WAVE;    // LOAD0, LOAD1, CHAIN

struct TglsFeedArgs {
    const double *terms;      // [blk - blk0][term_rows][64]
    int64_t term_rows;
    const ChainItem *items;
    const ChrDev *chrs;       // out_base / out_pitch: the thinned matrix
    double *out;
    int32_t ind_begin, ind_count, winsize, n_items, thin_step;
    int32_t blk0;             // first block `terms` holds (TglsArgs::blk0)
    int32_t *next_item;       // [0] queue head, [1] workgroups that have left (both zero at launch; reset by the last one)
};

__global__ void __launch_bounds__(TGF_THREADS)
tgls_feed_kernel(TglsFeedArgs p)
{
    __shared__ __attribute__((aligned(1024))) double ring[TG_RING * WAVE];
    __shared__ __attribute__((aligned(16))) double patch[WAVE * TPITCH];
    __shared__ int flags[8];      // [0] tiles finished by CHAIN, [2] / [3] requests landed (LOAD0 / LOAD1), [4] the item
    const int lane = threadIdx.x & (WAVE - 1);
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t ring_lds = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) double *)ring;
    for (;;) {
        if (threadIdx.x == 0) {
            flags[4] = atomicAdd(p.next_item, 1);
            flags[0] = 0; flags[2] = 0; flags[3] = 0;
        }
        __syncthreads();
        const int item_idx = __builtin_amdgcn_readfirstlane(flags[4]);
        if (item_idx >= p.n_items) {
            if (threadIdx.x == 0) {
                __threadfence();
                if (atomicAdd(p.next_item + 1, 1) == (int)gridDim.x - 1) {
                    p.next_item[0] = 0;
                    p.next_item[1] = 0;
                }
            }
            return;
        }
        const ChainItem it = p.items[item_idx];
        const ChrDev c = p.chrs[it.chr];
        const int W = p.winsize, a = it.a, b = it.b, step = p.thin_step;
        const int first = a & ~(TILE - 1);
        const int ntiles = (b - first) / TILE + 1;
        const bool single = W <= TG_SINGLE_MAX_W;
        const int ring_rows = single ? TG_RING : TG_RING / 2;
        const int64_t col0 = (int64_t)p.ind_begin + it.ind0;            // block-aligned (host-checked)
        const int64_t Gbase = c.loc_base + GOFF;
        const double *blk = p.terms + (((col0 >> 6) - p.blk0) * p.term_rows) * WAVE;   // the block's rows, 64 doubles each
        // row streams: leaving rows start at local locus first - 1, entering rows at first + W - 1
        const double *trail = blk + (Gbase + first - 1) * WAVE;
        const double *lead = blk + (Gbase + first + W - 1) * WAVE;

        if (wave < 2) {   // ---- loaders (as in lod_chain_ring_kernel)
            if (single) {
                const int n_rows = TILE * ntiles + W;
                const int n_pieces = (n_rows + 1) / 2;
                const int mine = (n_pieces - wave + 1) / 2;              // pieces wave, wave + 2, ..
                tg_loader(trail, mine, 2, wave, ring_rows, ring_lds, &flags[0], &flags[2 + wave], lane);
            } else {
                const int n_pieces = TILE * ntiles / 2;
                tg_loader(wave == 0 ? lead : trail, n_pieces, 1, 0, ring_rows,
                          ring_lds + (wave == 0 ? 0u : (uint32_t)ring_rows * 512u), &flags[0], &flags[2 + wave], lane);
            }
        } else {   // ---- chain
            // first window of the run: its first W-1 terms, left to right (garlic-roh.cpp:57-71); the W-th
            // enters in the first tile.  Straight from memory, 32 loads in flight (once per item).
            const double *tcol = blk + lane;
            double acc = 0.0;
            for (int l0 = a; l0 < a + W - 1; l0 += 32) {
                double t[32];
#pragma unroll
                for (int q = 0; q < 32; q++) t[q] = tcol[(Gbase + min(l0 + q, a + W - 2)) * WAVE];
#pragma unroll
                for (int q = 0; q < 32; q++) acc += (l0 + q < a + W - 1) ? t[q] : 0.0;
            }
            int so = 0, si = single ? W % ring_rows : 0;
            const int base_out = single ? 0 : ring_rows * WAVE;
            // the lane's row of the thinned matrix; the next sampled locus at or after a
            const bool row_ok = it.ind0 + lane < p.ind_count;
            double *const out_row = p.out + c.out_base + (int64_t)(it.ind0 + (row_ok ? lane : 0)) * c.out_pitch;
            // (64-bit: garlic_lod_feed takes any step >= 1, and next + step must not wrap)
            int64_t col = ((int64_t)a + step - 1) / step, next = col * step;
            for (int k = 0; k < ntiles; k++) {
                // inputs: every row this tile reads has landed
                if (single) {
                    const int pieces = (TILE * (k + 1) + W + 1) / 2;            // stream pieces 0 .. pieces-1
                    const int need0 = (pieces + 1) / 2, need1 = pieces / 2;      // of loader 0 (even) / 1 (odd)
                    while (LDS_FLAG_GET(flags[2]) < need0 || LDS_FLAG_GET(flags[3]) < need1) __builtin_amdgcn_s_sleep(1);
                } else {
                    const int need = TILE * (k + 1) / 2;
                    while (LDS_FLAG_GET(flags[2]) < need || LDS_FLAG_GET(flags[3]) < need) __builtin_amdgcn_s_sleep(1);
                }
                lds_acquire();
                const int s0 = first + k * TILE;
                const bool edge = (s0 <= a) || (s0 + TILE - 1 > b);
                const bool sampled = next < s0 + TILE && next <= b;             // (next >= s0 always)
                double t_in[TILE], t_out[TILE];
                if (si + TILE <= ring_rows && so + TILE <= ring_rows) {
                    // neither stream wraps inside this tile: one address per stream, the rows at immediate offsets
                    const double *pi = ring + si * WAVE + lane, *po = ring + base_out + so * WAVE + lane;
#pragma unroll
                    for (int j = 0; j < TILE; j++) {
                        t_in[j] = pi[j * WAVE];
                        t_out[j] = po[j * WAVE];
                    }
                    si = (si + TILE == ring_rows) ? 0 : si + TILE;
                    so = (so + TILE == ring_rows) ? 0 : so + TILE;
                } else {
#pragma unroll
                    for (int j = 0; j < TILE; j++) {
                        t_in[j] = ring[si * WAVE + lane];
                        t_out[j] = ring[base_out + so * WAVE + lane];
                        si = (si + 1 == ring_rows) ? 0 : si + 1;
                        so = (so + 1 == ring_rows) ? 0 : so + 1;
                    }
                }
                if (edge) {
#pragma unroll
                    for (int j = 0; j < TILE; j++) {
                        const int s = s0 + j;
                        const bool in = (s >= a && s <= b);
                        const double ti = in ? t_in[j] : 0.0;
                        const double to = (in && s > a) ? t_out[j] : 0.0;
                        acc = (acc - to) + ti;
                        if (sampled) patch[lane * TPITCH + j] = acc;
                    }
                } else if (sampled) {
#pragma unroll
                    for (int j = 0; j < TILE; j++) {
                        acc = (acc - t_out[j]) + t_in[j];
                        patch[lane * TPITCH + j] = acc;
                    }
                } else {
#pragma unroll
                    for (int j = 0; j < TILE; j++) acc = (acc - t_out[j]) + t_in[j];
                }
                // the ring rows of this tile are in registers: the loaders may have them
                lds_release();
                if (lane == 0) LDS_FLAG_SET(flags[0], k + 1);
                if (sampled) {
                    // (the patch is this wave's own: program order is all the ordering it needs)
                    const int64_t last = min(s0 + TILE - 1, b);
                    for (; next <= last; next += step, col++) {
                        const double v = patch[lane * TPITCH + (int)(next - s0)];
                        if (row_ok) out_row[col] = v;
                    }
                }
            }
        }
        __syncthreads();   // the item's ring and counters are free again
    }
}

} // namespace garlic
