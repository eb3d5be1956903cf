// wLOD (garlic-roh.cpp:204-277) for the thinned KDE feed: only the sampled windows.
//
// Every wLOD window is an ordered sum of its own (parallelwLOD, garlic-roh.cpp:253-273), so a window that
// convertWinData2DoubleData (garlic-data.cpp:2033-2037) does not sample -- it keeps the windows at the chromosome-local
// loci 0, step, 2 step, .. -- need not be computed.  With step >= W the sampled windows do not overlap: every scaled
// term is used at most once, and the kernel is one pass over the genotypes (0.25 B per SNP and individual) or over the
// scaled term matrix (8 B), against W multiply-adds per SNP and individual in the kernels that score every window.
//
// A work item is WFD_COLS consecutive columns of the thinned score matrix (make_layout(.., step): row = individual,
// column = locus / step) of one chromosome, for WFD_WAVES 64-individual blocks -- a wave each, lane = individual; the
// blocks come from a list, so a subset feed only visits the blocks that hold a listed individual.  Per sampled window s:
//   * no score there by the position mask (the byte the other wLOD kernels read): -9999.0;
//   * else, WFD_CHUNK terms at a time, the workgroup stages what is the same for every lane in LDS, coalesced: the
//     window's weights 1 / LD[s][k] (the skewed table holds them W + 1 doubles apart: D[s + k][k]) and, without
//     likelihoods, the score rows wtab[s + k][0 .. 3]; a lane then adds sc * weight for k = 0 .. W-1, from +0.0, the
//     product rounded before the add, nothing skipped (a missing genotype's +0.0 still meets its weight: 0 * inf is
//     the reference's NaN).  sc: the row's entry for the lane's genotype (one 32-bit word = 16 SNPs per load, the next
//     word requested before this one is used), or with likelihoods the lane's own entry of the scaled term matrix
//     (512 B per wave and row).
// The wave's 64 x WFD_COLS sums are transposed through a patch of its own in LDS and leave as 128 aligned bytes per
// row (16 B per lane, eight lanes a row).
#pragma once
#include "variant_kernels.hpp"

namespace garlic {

constexpr int WFD_COLS = 16;       // columns of the thinned matrix per work item (128 B of every row)
constexpr int WFD_WAVES = 4;       // 64-individual blocks per workgroup
constexpr int WFD_CHUNK = 256;     // terms staged per pass (windows up to 4096: sixteen passes)
constexpr int WFD_PITCH = 18;      // doubles per patch row (16 + pad, rows stay 16-B aligned)

struct WlodFeedArgs {
    const uint32_t *packed;    // [nind_pad/64][nwordrows][64]
    const double *sc;          // GL: scaled term matrix [block][score_rows][64]; else wtab [GOFF + nloci + pad][4]
    const double *skew;        // D[l][j] = 1 / LD[l - j][j]
    const uint8_t *valid;      // [nloci] 1 = window holds a score
    const ChrDev *chrs;        // out_base / out_pitch: the thinned layout
    const int2 *groups;        // per work item: {chromosome, first column}
    const int32_t *blocks;     // the 64-individual blocks in play
    double *out;
    int64_t nwordrows, score_rows;
    int32_t ind_count, winsize, step, nblocks, nquad;      // nquad = workgroups per column group
    uint32_t n_work;           // column groups x nquad
    int32_t blk0;              // GL: sc is the slab [block - blk0][score_rows][64] and `blocks` lists that slab's blocks; 0: the whole matrix
};

template <bool GL>
__global__ void __launch_bounds__(WFD_WAVES * WAVE)
wlod_feed_kernel(WlodFeedArgs p)
{
    __shared__ __attribute__((aligned(16))) double rows[GL ? 2 : WFD_CHUNK * 4];
    __shared__ __attribute__((aligned(16))) double wts[WFD_CHUNK];
    __shared__ __attribute__((aligned(16))) double patches[WFD_WAVES * WAVE * WFD_PITCH];
    if (blockIdx.x >= p.n_work) return;
    const int lane = threadIdx.x & (WAVE - 1);
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int2 gd = p.groups[blockIdx.x / (unsigned)p.nquad];
    const ChrDev c = p.chrs[gd.x];
    const int W = p.winsize, col0 = gd.y;
    const int ncol = min(WFD_COLS, (c.nloci + p.step - 1) / p.step - col0);
    const int bi = (int)(blockIdx.x % (unsigned)p.nquad) * WFD_WAVES + wave;
    const bool active = bi < p.nblocks;                    // (wave-uniform)
    const int ind0 = active ? p.blocks[bi] * WAVE : 0;
    const int64_t col = (int64_t)ind0 + lane;
    double *patch = patches + wave * (WAVE * WFD_PITCH);
    for (int j = 0; j < ncol; j++) {
        const int s = (col0 + j) * p.step;                 // < nloci
        const int64_t ls = c.loc_base + s;
        double acc = MISSING_D;
        if (p.valid[ls] != 0) {                            // (the same for the whole workgroup)
            acc = 0.0;
            for (int k0 = 0; k0 < W; k0 += WFD_CHUNK) {
                const int n = min(WFD_CHUNK, W - k0);
                const int64_t G = ls + GOFF + k0;          // padded index of the chunk's first SNP
                __syncthreads();
                const double *wsrc = p.skew + ls * W + (int64_t)k0 * (W + 1);
                for (int k = threadIdx.x; k < n; k += WFD_WAVES * WAVE) wts[k] = wsrc[(int64_t)k * (W + 1)];
                if (!GL) {
                    const double2 *src = reinterpret_cast<const double2 *>(p.sc + G * 4);
                    double2 *dst = reinterpret_cast<double2 *>(rows);
                    for (int k = threadIdx.x; k < 2 * n; k += WFD_WAVES * WAVE) dst[k] = src[k];
                }
                __syncthreads();
                if (!active) continue;
                if (GL) {
                    const double *t = p.sc + (((int64_t)((ind0 >> 6) - p.blk0) * p.score_rows + G) << 6) + lane;
#pragma unroll 8
                    for (int k = 0; k < n; k++) {
                        const double pr = __builtin_nontemporal_load(t + (int64_t)k * WAVE) * wts[k];
                        acc = acc + pr;
                    }
                } else {
                    const uint32_t *gp = p.packed + packed_index(G >> 4, col, p.nwordrows);
                    uint32_t first = (uint32_t)(G & 15), word = *gp;
                    for (int k = 0; k < n;) {
                        gp += WAVE;
                        const uint32_t next = *gp;         // (pad rows follow the last chromosome)
                        const int m = min(n - k, 16 - (int)first);
                        uint32_t bits = word >> (2 * first);
                        for (int i = 0; i < m; i++) {
                            const double pr = rows[(k + i) * 4 + (bits & 3u)] * wts[k + i];
                            acc = acc + pr;
                            bits >>= 2;
                        }
                        k += m;
                        first = 0;
                        word = next;
                    }
                }
            }
        }
        patch[lane * WFD_PITCH + j] = acc;
    }
    if (!active) return;
    // the wave's own patch: no barrier, a wave's LDS operations execute in order
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
    const int r8 = lane >> 3, cc = 2 * (lane & 7);
    double *dst = p.out + c.out_base + col0 + cc;
#pragma unroll
    for (int pass = 0; pass < WAVE / 8; pass++) {
        const int r = pass * 8 + r8;
        const double2 v = *reinterpret_cast<const double2 *>(patch + r * WFD_PITCH + cc);
        if (ind0 + r < p.ind_count) {
            double *d = dst + (int64_t)(ind0 + r) * c.out_pitch;
            if (cc + 1 < ncol) *reinterpret_cast<double2 *>(d) = v;
            else if (cc < ncol) *d = v.x;
        }
    }
}

} // namespace garlic
