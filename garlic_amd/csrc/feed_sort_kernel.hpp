// The KDE feed in ascending order: a least-significant-digit radix sort of FP64 keys, 8-bit digits.
//
// computeKDE (src/garlic-kde.cpp:14) starts with nrd0 (:43, :130-139), whose first statement is gsl_sort(x, 1, N) on the
// feed, in place; everything behind it reads the sorted array.  The feed holds neither NaN nor -0.0 (garlic_hip.h), so its
// ascending arrangement is unique and any correct sort leaves the same bytes.
//
//   * key: k(x) = bits(x) ^ (sign ? ~0 : 1 << 63), compared as unsigned -- numeric order for everything that is not NaN,
//     -0.0 in front of +0.0, NaNs with the sign bit first and the others last: total, so the sorter can be tested alone.
//     Every kernel transforms on load and every store writes the double back, so memory never holds a transformed key.
//   * fs_hist_kernel reads the keys once for all eight 256-bin histograms: per workgroup in LDS, then 64-bit vector
//     atomic adds into FsTable::hist (integer adds: the result does not depend on their order).  fs_plan_kernel (one
//     workgroup) turns the table into what the passes need: per pass "trivial" (one bin holds every key: the pass would
//     move nothing), the buffer it reads (by the number of non-trivial passes in front of it) and the digits' bases.
//   * a pass = fs_count_kernel (digit counts per tile, [digit][tile]) -> fs_scan_kernel (exclusive scan over the tiles of
//     each digit + the digit's base, in place) -> fs_scatter_kernel.  Every one of them reads the plan and returns at once
//     when its pass is trivial: the host enqueues all eight passes without looking at anything, and no workgroup ever
//     waits for another (no look-back, no polled flags).
//   * fs_scatter_kernel, one tile of FS_TILE keys per workgroup: wave w owns keys [w * FS_TILE / 4, (w + 1) * FS_TILE / 4)
//     of the tile and walks them 64 at a time.  The lanes that hold the same digit are found from eight __ballot()s; a
//     key's rank among them is the population count of the peers below it (v_mbcnt), plus the wave's running count of the
//     digit (LDS, bumped by the topmost peer).  After a barrier thread d adds up digit d's counts over the waves (cross-wave
//     offsets), the digit starts of the tile are scanned, and every key goes to its place in an LDS image of the sorted
//     tile; the image then leaves in order, so keys of one digit go out as contiguous runs.  Stable throughout, as LSD
//     needs.  The keys past n in the last tile become ~0: digit 255 in every pass and behind every real key, so they end
//     up at the image's tail and are not stored.
//   * 64-bit element indices and counts everywhere; a tile count fits 32 bits.
//
// Traffic per pass and key: 8 B read (count) + 8 B read + 8 B write (scatter) = 24 B, plus 6 KB of tile counts per
// 32-KB tile.  LDS of the scatter: 32 KB image + 4 KB wave counts + 3 KB digit tables: four workgroups per CU.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace garlic {

constexpr int FS_TILE = 4096;              // keys per tile (tests read this)
constexpr int FS_THREADS = 256;            // count / scatter workgroup: 4 waves
constexpr int FS_WAVES = FS_THREADS / 64;
constexpr int FS_PER_THREAD = FS_TILE / FS_THREADS;
constexpr int FS_WAVE_KEYS = FS_TILE / FS_WAVES;
constexpr int FS_SCAN_THREADS = 1024;
constexpr int FS_HIST_KEYS = 16 * FS_THREADS;   // keys a histogram workgroup takes per round

struct FsTable {
    unsigned long long hist[8][256];       // zero at launch of fs_hist_kernel
    unsigned long long base[8][256];       // keys with a smaller digit, per pass
    int32_t trivial[8];                    // the pass moves nothing
    int32_t src_scratch[8];                // the pass reads the scratch buffer (and writes the caller's)
    int32_t n_run;                         // non-trivial passes
    int32_t in_scratch;                    // the sorted keys end in the scratch buffer
};

__device__ __forceinline__ unsigned long long fs_key(double x)
{
    const unsigned long long b = (unsigned long long)__double_as_longlong(x);
    return b ^ ((b >> 63) ? 0xFFFFFFFFFFFFFFFFull : 0x8000000000000000ull);
}

__device__ __forceinline__ double fs_value(unsigned long long k)
{
    return __longlong_as_double((long long)(k ^ ((k >> 63) ? 0x8000000000000000ull : 0xFFFFFFFFFFFFFFFFull)));
}

// one count for every lane's digit; a wave whose lanes all hold the same digit (the top bytes of a feed) adds once
__device__ __forceinline__ void fs_lds_count(unsigned int *bins, unsigned int d, bool valid)
{
    const unsigned long long live = __ballot(valid);
    if (!live) return;
    const unsigned int d0 = (unsigned int)__builtin_amdgcn_readlane((int)d, __builtin_ctzll(live));
    if (__ballot(valid && d == d0) == live) {
        if ((threadIdx.x & 63) == (unsigned)__builtin_ctzll(live)) atomicAdd(&bins[d0], (unsigned int)__popcll(live));
    } else if (valid) {
        atomicAdd(&bins[d], 1u);
    }
}

__global__ void __launch_bounds__(FS_THREADS)
fs_hist_kernel(const double *keys, int64_t n, FsTable *tab)
{
    __shared__ unsigned int bins[8 * 256];
    for (int i = threadIdx.x; i < 8 * 256; i += FS_THREADS) bins[i] = 0;
    __syncthreads();
    const int64_t stride = (int64_t)gridDim.x * FS_HIST_KEYS;
    for (int64_t i0 = (int64_t)blockIdx.x * FS_HIST_KEYS; i0 < n; i0 += stride)
        for (int j = 0; j < FS_HIST_KEYS / FS_THREADS; j++) {      // (uniform trip counts: the ballots see whole waves)
            const int64_t i = i0 + (int64_t)j * FS_THREADS + threadIdx.x;
            const bool valid = i < n;
            const unsigned long long k = valid ? fs_key(keys[i]) : 0;
#pragma unroll
            for (int p = 0; p < 8; p++) fs_lds_count(bins + p * 256, (unsigned int)(k >> (8 * p)) & 255u, valid);
        }
    __syncthreads();
    for (int i = threadIdx.x; i < 8 * 256; i += FS_THREADS)
        if (bins[i]) atomicAdd(&tab->hist[0][0] + i, (unsigned long long)bins[i]);
}

__global__ void __launch_bounds__(256)
fs_plan_kernel(FsTable *tab, int64_t n)
{
    __shared__ unsigned long long h[256];
    __shared__ int32_t triv[8];
    const int t = threadIdx.x;
    if (t < 8) triv[t] = 0;
    for (int p = 0; p < 8; p++) {
        __syncthreads();
        h[t] = tab->hist[p][t];
        if (h[t] == (unsigned long long)n) triv[p] = 1;
        __syncthreads();
        unsigned long long b = 0;
        for (int d = 0; d < t; d++) b += h[d];
        tab->base[p][t] = b;
    }
    __syncthreads();
    if (t == 0) {
        int32_t run = 0;
        for (int p = 0; p < 8; p++) {
            tab->trivial[p] = triv[p];
            tab->src_scratch[p] = run & 1;
            run += !triv[p];
        }
        tab->n_run = run;
        tab->in_scratch = run & 1;
    }
}

// digit counts of every tile for `pass`: counts[d * n_tiles + tile]
__global__ void __launch_bounds__(FS_THREADS)
fs_count_kernel(const double *buf, const double *scratch, int64_t n, int64_t n_tiles, int pass, const FsTable *tab,
                unsigned long long *counts)
{
    if (tab->trivial[pass]) return;
    __shared__ unsigned int bins[256];
    const double *src = tab->src_scratch[pass] ? scratch : buf;
    bins[threadIdx.x] = 0;
    __syncthreads();
    const int64_t tile = blockIdx.x;
    const int64_t i0 = tile * FS_TILE;
#pragma unroll 4
    for (int j = 0; j < FS_PER_THREAD; j++) {
        const int64_t i = i0 + (int64_t)j * FS_THREADS + threadIdx.x;
        const bool valid = i < n;
        const unsigned long long k = valid ? fs_key(src[i]) : 0;
        fs_lds_count(bins, (unsigned int)(k >> (8 * pass)) & 255u, valid);
    }
    __syncthreads();
    counts[(int64_t)threadIdx.x * n_tiles + tile] = bins[threadIdx.x];
}

// workgroup d: counts[d][tile] -> where the tile's keys of digit d begin in the destination (in place)
__global__ void __launch_bounds__(FS_SCAN_THREADS)
fs_scan_kernel(int64_t n_tiles, int pass, const FsTable *tab, unsigned long long *counts)
{
    if (tab->trivial[pass]) return;
    __shared__ unsigned int wsum[FS_SCAN_THREADS / 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    unsigned long long *row = counts + (int64_t)blockIdx.x * n_tiles;
    unsigned long long carry = tab->base[pass][blockIdx.x];
    for (int64_t t0 = 0; t0 < n_tiles; t0 += FS_SCAN_THREADS) {
        const int64_t t = t0 + threadIdx.x;
        const unsigned int v = t < n_tiles ? (unsigned int)row[t] : 0u;      // (a tile count: at most FS_TILE)
        unsigned int x = v;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const unsigned int y = (unsigned int)__shfl_up((int)x, o, 64);
            if (lane >= o) x += y;
        }
        if (lane == 63) wsum[wave] = x;
        __syncthreads();
        unsigned int before = 0, total = 0;
#pragma unroll
        for (int w = 0; w < FS_SCAN_THREADS / 64; w++) {
            const unsigned int s = wsum[w];
            if (w < wave) before += s;
            total += s;
        }
        if (t < n_tiles) row[t] = carry + before + (x - v);
        carry += total;
        __syncthreads();
    }
}

__global__ void __launch_bounds__(FS_THREADS)
fs_scatter_kernel(double *buf, double *scratch, int64_t n, int64_t n_tiles, int pass, const FsTable *tab,
                  const unsigned long long *offsets)
{
    if (tab->trivial[pass]) return;
    __shared__ unsigned long long image[FS_TILE];
    __shared__ unsigned int wcount[FS_WAVES][256];     // running count of the wave per digit; then its cross-wave offset
    __shared__ unsigned int dstart[256];               // first place of the digit in the image
    __shared__ unsigned long long gstart[256];         // first place of the tile's keys of the digit in the destination
    __shared__ unsigned int wtot[FS_WAVES];
    const bool from_scratch = tab->src_scratch[pass] != 0;
    const double *src = from_scratch ? scratch : buf;
    double *dst = from_scratch ? buf : scratch;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int shift = 8 * pass;
    const int64_t tile = blockIdx.x;
    const int64_t i0 = tile * FS_TILE;
    const int tile_n = (int)(n - i0 < FS_TILE ? n - i0 : FS_TILE);
    for (int w = 0; w < FS_WAVES; w++) wcount[w][threadIdx.x] = 0;
    gstart[threadIdx.x] = offsets[(int64_t)threadIdx.x * n_tiles + tile];
    unsigned long long key[FS_PER_THREAD];
    unsigned int rank[FS_PER_THREAD];
#pragma unroll
    for (int j = 0; j < FS_PER_THREAD; j++) {
        const int64_t i = i0 + wave * FS_WAVE_KEYS + j * 64 + lane;
        key[j] = i < n ? fs_key(src[i]) : 0xFFFFFFFFFFFFFFFFull;
    }
    __syncthreads();
    // ---- the wave's piece, 64 keys at a time: rank among the wave's keys of the same digit
#pragma unroll
    for (int j = 0; j < FS_PER_THREAD; j++) {
        const unsigned int d = (unsigned int)(key[j] >> shift) & 255u;
        unsigned long long peers = ~0ull;
#pragma unroll
        for (int b = 0; b < 8; b++) {
            const bool bit = (d >> b) & 1u;
            const unsigned long long m = __ballot(bit);
            peers &= bit ? m : ~m;
        }
        const unsigned int below = __builtin_amdgcn_mbcnt_hi((unsigned int)(peers >> 32), __builtin_amdgcn_mbcnt_lo((unsigned int)peers, 0u));
        const unsigned int cnt = (unsigned int)__popcll(peers);
        volatile unsigned int *wc = &wcount[wave][d];
        const unsigned int seen = *wc;                 // every peer reads before the topmost one writes: one wave, in order
        rank[j] = seen + below;
        __builtin_amdgcn_wave_barrier();
        if (below == cnt - 1) *wc = seen + cnt;
        __builtin_amdgcn_wave_barrier();
    }
    __syncthreads();
    // ---- digit d: offsets of the waves' keys among the tile's keys of the digit, the digit's place in the image
    {
        const int d = threadIdx.x;
        unsigned int sum = 0;
#pragma unroll
        for (int w = 0; w < FS_WAVES; w++) {
            const unsigned int c = wcount[w][d];
            wcount[w][d] = sum;
            sum += c;
        }
        unsigned int x = sum;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const unsigned int y = (unsigned int)__shfl_up((int)x, o, 64);
            if (lane >= o) x += y;
        }
        if (lane == 63) wtot[wave] = x;
        __syncthreads();
        unsigned int before = 0;
#pragma unroll
        for (int w = 0; w < FS_WAVES; w++)
            if (w < wave) before += wtot[w];
        dstart[d] = before + x - sum;
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < FS_PER_THREAD; j++) {
        const unsigned int d = (unsigned int)(key[j] >> shift) & 255u;
        image[dstart[d] + wcount[wave][d] + rank[j]] = key[j];
    }
    __syncthreads();
    // ---- the image leaves in order: place i of the image is place i - dstart[d] among the tile's keys of its digit
#pragma unroll 4
    for (int j = 0; j < FS_PER_THREAD; j++) {
        const int i = j * FS_THREADS + threadIdx.x;
        if (i < tile_n) {
            const unsigned long long k = image[i];
            const unsigned int d = (unsigned int)(k >> shift) & 255u;
            const unsigned long long at = gstart[d] + (unsigned long long)(i - dstart[d]);
            if (at < (unsigned long long)n) dst[at] = fs_value(k);      // (always true for consistent counts; never out of bounds)
        }
    }
}

// device destination: the sorted keys back into the caller's buffer when an odd number of passes ran
__global__ void __launch_bounds__(FS_THREADS)
fs_copy_back_kernel(double *buf, const double *scratch, int64_t n, const FsTable *tab)
{
    if (!tab->in_scratch) return;
    const int64_t stride = (int64_t)gridDim.x * FS_THREADS;
    for (int64_t i = (int64_t)blockIdx.x * FS_THREADS + threadIdx.x; i < n; i += stride) buf[i] = scratch[i];
}

} // namespace garlic
