// TGLS chain for the KDE feeds of several window sizes at once: tgls_feed_kernel's one-stream form for a group of up
// to TGM_MAX_SIZES sizes (garlic_lod_feed_multi_tgls; the window-size sweeps of src/garlic-roh.cpp:726-751, 798-837,
// 881-920 run the same likelihoods through every candidate size).
//
// Two facts let one pass over the terms serve every size of the group bit for bit:
//   * a run of valid windows is a gap- and centromere-free stretch of SNPs [p, q] with at least W of them, its windows
//     p .. q - W + 1: the runs of every size over one stretch start at the same window and differ in their last one;
//   * the first window of a run is (((0.0 + t[p]) + t[p+1]) + ..), left to right: one walk over t[p .. p + Wmax - 2]
//     passes through every size's partial first-window sum -- the value after W_i - 1 terms is size i's, rounded
//     as the single kernel rounds it.
// In acc_i = (acc_i - t[s-1]) + t[s+W_i-1] the leaving term is the same for every size.
//
//   * work item: (stretch, 64-individual block), a = p, ChainItem::b = q (the stretch's last SNP, not a window); per
//     size b_i = q - W_i + 1.  The sizes are sorted ascending, so the sizes that hold a window in the stretch are a
//     prefix of the group (the host lists only stretches that hold the smallest size), and so are the sizes still
//     running in a tile.  Items longest first; queue head and leave counter as in tgls_feed_kernel.
//   * LOAD0 / LOAD1: tg_loader as it stands, rows first - 1 .. q (+ 1 for an even count) through the TG_RING-row ring
//     once -- nothing behind the stretch's last SNP is read, where the single kernel reads up to 31 + W rows of slack.
//     The widest size of the item paces them (the chain waits for row 32 (k + 1) + Wmax of the stream before tile k),
//     hence Wmax <= TG_SINGLE_MAX_W as for the single kernel's one-stream form.
//   * CHAIN: per tile of 32 windows t_out[32] is read from the ring once; per size still running t_in[32] from the
//     ring rows W_i ahead and the 32 steps, with the single kernel's two rounded operations and its edge handling
//     (first tile; the last tile of each size).  A tile that holds a sampled locus of size i goes through the
//     wave-private patch into size i's own thinned matrix (make_layout(p, 32, nind, step_i), filled with -9999.0 in
//     front of the launch), one lane-strided store per sample.  The ring rows of a tile are released once the last size
//     has them in registers.
//
// TGM_MAX_SIZES = 4.  VGPRs are not what bounds it: the chain wave holds t_out[32] and one size's t_in[32] (128 VGPRs)
// and one accumulator, one sample column and one sample locus per size, and a 192-thread workgroup alone on its CU may
// use 512.  LDS holds one ring (120 KB) and one patch (17 KB) whatever the count.  The bound is the chain wave's time:
// it is the wave that paces the single kernel, every size adds its 32 ds_read_b64 and 64 dependent
// adds per tile to that one wave, and the loaders, which a group shares, idle the longer the more sizes it holds.
// Four is the sweep width of the reference's own lists (--winsize-multi is usually given 3 - 5 sizes); the default was
// NOT chosen from a timing, see DESIGN.md section 3 for what was and was not measured.
#pragma once
#include "tgls_feed_kernel.hpp"

namespace garlic {

constexpr int TGM_MAX_SIZES = 4;

struct TglsFeedMultiArgs {
    const double *terms;      // [blk - blk0][term_rows][64]
    int64_t term_rows;
    const ChainItem *items;   // a: the stretch's first SNP (= first window of every size), b: its LAST SNP
    const ChrDev *chrs;       // [n_sizes][nchr]; out_base / out_pitch: size i's thinned matrix
    double *out[TGM_MAX_SIZES];
    int32_t winsize[TGM_MAX_SIZES], thin_step[TGM_MAX_SIZES];   // ascending window sizes, 2 <= W <= TG_SINGLE_MAX_W
    int32_t n_sizes, nchr, ind_begin, ind_count, n_items;
    int32_t blk0;             // first block `terms` holds (TglsArgs::blk0)
    int32_t *next_item;       // [0] queue head, [1] workgroups that have left (both zero at launch; reset by the last one)
};

// one size's share of a tile: its 32 entering terms from the ring, the 32 steps, its samples
__device__ __forceinline__ void tgm_size_tile(const double *ring, double *patch, const double (&t_out)[TILE], double &acc, int si,
                                              int s0, int a, int b, int step, int64_t &next, int64_t &col, double *out_row,
                                              bool row_ok, int lane)
{
    double t_in[TILE];
    if (si + TILE <= TG_RING) {
        const double *pi = ring + si * WAVE + lane;
#pragma unroll
        for (int j = 0; j < TILE; j++) t_in[j] = pi[j * WAVE];
    } else {
#pragma unroll
        for (int j = 0; j < TILE; j++) {
            t_in[j] = ring[si * WAVE + lane];
            si = (si + 1 == TG_RING) ? 0 : si + 1;
        }
    }
    const bool edge = (s0 <= a) || (s0 + TILE - 1 > b);
    const bool sampled = next < s0 + TILE && next <= b;             // (next >= s0 always)
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
    if (sampled) {
        // (the patch is this wave's own: program order is all the ordering it needs)
        const int64_t last = min(s0 + TILE - 1, b);
        for (; next <= last; next += step, col++) {
            const double v = patch[lane * TPITCH + (int)(next - s0)];
            if (row_ok) out_row[col] = v;
        }
    }
}

__global__ void __launch_bounds__(TGF_THREADS)
tgls_feed_multi_kernel(TglsFeedMultiArgs p)
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
        const int a = it.a, q = it.b;
        // the sizes with a window in this stretch: a prefix (ascending sizes), never empty (host-checked)
        int n_act = 1;
#pragma unroll
        for (int i = 1; i < TGM_MAX_SIZES; i++)
            if (i < p.n_sizes && q - p.winsize[i] + 1 >= a) n_act = i + 1;
        int Wm = p.winsize[0];
#pragma unroll
        for (int i = 1; i < TGM_MAX_SIZES; i++)
            if (i < n_act) Wm = p.winsize[i];
        const int first = a & ~(TILE - 1);
        const int ntiles = (q - p.winsize[0] + 1 - first) / TILE + 1;      // the smallest size runs longest
        const int n_rows = q - first + 2;                                   // stream rows: local loci first - 1 .. q
        const int64_t col0 = (int64_t)p.ind_begin + it.ind0;            // block-aligned (host-checked)
        const int64_t Gbase = p.chrs[it.chr].loc_base + GOFF;
        const double *blk = p.terms + (((col0 >> 6) - p.blk0) * p.term_rows) * WAVE;   // the block's rows, 64 doubles each
        const double *trail = blk + (Gbase + first - 1) * WAVE;

        if (wave < 2) {   // ---- loaders (as in tgls_feed_kernel, one stream)
            const int n_pieces = (n_rows + 1) / 2;
            const int mine = (n_pieces - wave + 1) / 2;              // pieces wave, wave + 2, ..
            tg_loader(trail, mine, 2, wave, TG_RING, ring_lds, &flags[0], &flags[2 + wave], lane);
        } else {   // ---- chain
            // first windows: one walk over the widest size's first Wm - 1 terms, left to right (garlic-roh.cpp:57-71),
            // size i's sum taken as it passes W_i - 1 terms; the W_i-th enters in the first tile.  Straight from memory.
            const double *tcol = blk + lane;
            double acc[TGM_MAX_SIZES] = {0.0, 0.0, 0.0, 0.0};
            double run = 0.0;
            for (int l0 = a; l0 < a + Wm - 1; l0 += 32) {
                double t[32];
#pragma unroll
                for (int j = 0; j < 32; j++) t[j] = tcol[(Gbase + min(l0 + j, a + Wm - 2)) * WAVE];
#pragma unroll
                for (int j = 0; j < 32; j++) {
                    run += (l0 + j < a + Wm - 1) ? t[j] : 0.0;
                    const int n = l0 + j - a + 1;                   // terms summed so far
#pragma unroll
                    for (int i = 0; i < TGM_MAX_SIZES; i++)
                        if (i < n_act && n == p.winsize[i] - 1) acc[i] = run;
                }
            }
            const bool row_ok = it.ind0 + lane < p.ind_count;
            const int row = it.ind0 + (row_ok ? lane : 0);
            double *out_row[TGM_MAX_SIZES];
            int64_t col[TGM_MAX_SIZES], next[TGM_MAX_SIZES];
#pragma unroll
            for (int i = 0; i < TGM_MAX_SIZES; i++) {
                out_row[i] = nullptr;
                col[i] = next[i] = 0;
                if (i < n_act) {
                    const ChrDev c = p.chrs[i * p.nchr + it.chr];
                    out_row[i] = p.out[i] + c.out_base + (int64_t)row * c.out_pitch;
                    // (64-bit: any step >= 1 is taken, and next + step must not wrap)
                    col[i] = ((int64_t)a + p.thin_step[i] - 1) / p.thin_step[i];
                    next[i] = col[i] * p.thin_step[i];
                }
            }
            int so = 0;
            for (int k = 0; k < ntiles; k++) {
                // inputs: every row this tile reads has landed (the widest size's lead, or the end of the stream)
                const int pieces = (min(TILE * (k + 1) + Wm, n_rows) + 1) / 2;   // stream pieces 0 .. pieces-1
                const int need0 = (pieces + 1) / 2, need1 = pieces / 2;          // of loader 0 (even) / 1 (odd)
                while (LDS_FLAG_GET(flags[2]) < need0 || LDS_FLAG_GET(flags[3]) < need1) __builtin_amdgcn_s_sleep(1);
                lds_acquire();
                const int s0 = first + k * TILE;
                double t_out[TILE];
                if (so + TILE <= TG_RING) {
                    const double *po = ring + so * WAVE + lane;
#pragma unroll
                    for (int j = 0; j < TILE; j++) t_out[j] = po[j * WAVE];
                } else {
                    int s = so;
#pragma unroll
                    for (int j = 0; j < TILE; j++) {
                        t_out[j] = ring[s * WAVE + lane];
                        s = (s + 1 == TG_RING) ? 0 : s + 1;
                    }
                }
                // the sizes still running in this tile: a prefix again (b_i falls as W_i grows)
#pragma unroll
                for (int i = 0; i < TGM_MAX_SIZES; i++) {
                    if (i >= n_act) continue;
                    const int W = p.winsize[i], b = q - W + 1;
                    if (s0 > b) continue;
                    int si = so + W;
                    if (si >= TG_RING) si -= TG_RING;
                    tgm_size_tile(ring, patch, t_out, acc[i], si, s0, a, b, p.thin_step[i], next[i], col[i], out_row[i], row_ok, lane);
                }
                so = (so + TILE >= TG_RING) ? so + TILE - TG_RING : so + TILE;
                // the ring rows of this tile are in registers, for every size: the loaders may have them
                lds_release();
                if (lane == 0) LDS_FLAG_SET(flags[0], k + 1);
            }
        }
        __syncthreads();   // the item's ring and counters are free again
    }
}

} // namespace garlic
