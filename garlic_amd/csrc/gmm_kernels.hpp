// GMM::update (src/gmm.cpp:276-331) on the device: one EM iteration of the 1-D Gaussian mixture that selectSizeClasses
// (src/garlic-roh.cpp:935-1003) fits to the ROH lengths is one pass over x[0 .. n).  The formulas are the reference's,
// term for term and in its association (the library is built with -ffp-contract=off); only the n-term sums differ: their
// order, and each carries the rounding errors of its adds in a second double (below).  exp and log are the device
// library's FP64 functions.
//
//   * gmm_em_kernel<K>: one workgroup per GMM_BLOCK_POINTS consecutive points.  Lanes own points (thread t takes
//     i0 + t, i0 + t + 256, ... in that order); the 3K + 1 partial sums -- per component the responsibilities, x times
//     them, x * x times them, and the log-likelihood -- live in registers.  log(a_i), C - 0.5 log(var_i) and 2 var_i
//     depend on the iteration only and are formed once per thread, by the same operations, so with the same values.
//     The sums are added across the wave by an xor butterfly (offsets 32, 16, ... 1), across the four waves through LDS
//     ((w0 + w1) + w2) + w3, and written to partial[sum][block] (hi) and partial[3K + 1 + sum][block] (lo).
//   * every sum is a pair (hi, lo): hi is the plain FP64 sum in the order above, lo collects what each add of hi rounded
//     away (Knuth's two-sum, branch-free, exact in round-to-nearest) and travels with hi through the butterfly, LDS and
//     the partials; the total is hi + lo, formed once at the end.  EM feeds every sum back into the next update, and
//     var = S2 / S0 - mean^2 cancels: with plain sums the order of the adds alone moved var by 1e-14 relative after 25
//     updates of 64 points.  With the pair the total is the sum of the terms to about n * 2^-106
//     before its one rounding, so the order no longer shows.  A sum that is not finite is hi alone: Inf and NaN come out
//     as the plain sum gives them.  Six adds per term beside some 2K exp and log.
//   * gmm_finish: one workgroup adds the blocks' partials -- thread t blocks t, t + 256, ... in order, then the same
//     butterfly and LDS step -- and thread 0 turns the totals into the next parameters, L, BIC, the iteration count and
//     the stop rule |L - L_prev| <= precision (never true for a NaN, nor for precision < 0).  It runs as a kernel of
//     its own behind a multi-block pass, and at the tail of the pass itself when the grid is one workgroup: no data is
//     handed from one workgroup to another inside a launch, so no fences, tickets or write-through stores are needed
//     (on this device a hand-off inside a launch costs an agent-scope release and acquire, about what the second
//     launch costs, and is far easier to get wrong across the eight L2s).
//   * every kernel returns at once when the state's converged flag is set: the host enqueues iterations in batches and
//     reads the state once per batch.
//   * the grid (ceil(n / GMM_BLOCK_POINTS)) and the combination tree are functions of n and K alone: not of the device's
//     CU count, not of timing.  No floating-point atomics, no atomics at all.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace garlic {

constexpr int GMM_MAX_K = 8;               // GARLIC_GMM_MAX_K
constexpr int GMM_THREADS = 256;
constexpr int GMM_BLOCK_POINTS = 2048;     // points per workgroup (tests read this)
constexpr int GMM_WAVES = GMM_THREADS / 64;
constexpr double GMM_LOG_NORM = -0.9189385332046727;   // -0.5 * log(2 pi), normalLog's C
constexpr double GMM_DBL_MAX = 1.7976931348623157e308;

struct GmmState {
    double a[GMM_MAX_K], mean[GMM_MAX_K], var[GMM_MAX_K];
    double loglik, bic, prev;              // prev: the L the stop rule compares with (-DBL_MAX before the first update)
    int32_t iterations, converged;
};

// (hi, lo) += v: hi the rounded sum, lo gains exactly what that add rounded away
__device__ __forceinline__ void gmm_add(double &hi, double &lo, double v)
{
    const double s = hi + v;
    const double b = s - hi;
    lo += (hi - (s - b)) + (v - b);
    hi = s;
}

// (hi, lo) += (ohi, olo)
__device__ __forceinline__ void gmm_merge(double &hi, double &lo, double ohi, double olo)
{
    gmm_add(hi, lo, ohi);
    lo += olo;
}

// the workgroup's totals of the pairs (hi[s], lo[s]) in tot[s], tot[NS + s] (LDS), visible to every thread on return
template <int NS> __device__ __forceinline__ void gmm_block_sums(const double (&hi)[NS], const double (&lo)[NS], double *red, double *tot)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int s = 0; s < NS; s++) {
        double h = hi[s], l = lo[s];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const double oh = __shfl_xor(h, o), ol = __shfl_xor(l, o);
            gmm_merge(h, l, oh, ol);
        }
        if (lane == 0) {
            red[wave * 2 * NS + s] = h;
            red[wave * 2 * NS + NS + s] = l;
        }
    }
    __syncthreads();
    if ((int)threadIdx.x < NS) {
        double h = red[threadIdx.x], l = red[NS + threadIdx.x];
#pragma unroll
        for (int w = 1; w < GMM_WAVES; w++) gmm_merge(h, l, red[w * 2 * NS + threadIdx.x], red[w * 2 * NS + NS + threadIdx.x]);
        tot[threadIdx.x] = h;
        tot[NS + threadIdx.x] = l;
    }
    __syncthreads();
}

// the value of a pair: hi + lo, or hi alone where the sum left the finite range (lo is NaN then)
__device__ __forceinline__ double gmm_total(double hi, double lo)
{
    return fabs(hi) <= GMM_DBL_MAX ? hi + lo : hi;
}

// the blocks' partials -> the state of the next iteration (every thread of one workgroup calls it)
template <int K> __device__ __forceinline__ void gmm_finish(const double *partial, int64_t n_blocks, int64_t n, double log_n,
                                                            double precision, GmmState *st, double *red, double *tot)
{
    constexpr int NS = 3 * K + 1;
    double acc[NS], low[NS];
#pragma unroll
    for (int s = 0; s < NS; s++) acc[s] = low[s] = 0.0;
    for (int64_t b = threadIdx.x; b < n_blocks; b += GMM_THREADS) {
#pragma unroll
        for (int s = 0; s < NS; s++) gmm_merge(acc[s], low[s], partial[(int64_t)s * n_blocks + b], partial[(int64_t)(NS + s) * n_blocks + b]);
    }
    gmm_block_sums<NS>(acc, low, red, tot);
    if (threadIdx.x == 0) {
#pragma unroll
        for (int k = 0; k < K; k++) {
            const double s0 = gmm_total(tot[k], tot[NS + k]), s1 = gmm_total(tot[K + k], tot[NS + K + k]);
            const double s2 = gmm_total(tot[2 * K + k], tot[NS + 2 * K + k]);
            const double mean = s1 / s0;
            st->a[k] = s0 / (double)n;
            st->mean[k] = mean;
            st->var[k] = s2 / s0 - mean * mean;
        }
        const double L = gmm_total(tot[3 * K], tot[NS + 3 * K]);
        st->loglik = L;
        st->bic = -2.0 * L + (double)(3.0 * K - 1) * log_n;
        st->iterations += 1;
        if (fabs(L - st->prev) <= precision) st->converged = 1;
        st->prev = L;
    }
}

template <int K> __global__ void __launch_bounds__(GMM_THREADS)
gmm_em_kernel(const double *x, int64_t n, int64_t n_blocks, double log_n, double precision, GmmState *st, double *partial)
{
    constexpr int NS = 3 * K + 1;
    __shared__ double red[GMM_WAVES * 2 * NS];
    __shared__ double tot[2 * NS];
    if (st->converged) return;             // the same word for every thread of the launch: nothing writes it before the finish
    double la[K], cv[K], tv[K], mean[K];
#pragma unroll
    for (int i = 0; i < K; i++) {
        const double var = st->var[i];
        la[i] = log(st->a[i]);
        cv[i] = GMM_LOG_NORM - 0.5 * log(var);
        tv[i] = 2.0 * var;
        mean[i] = st->mean[i];
    }
    double acc[NS], low[NS];
#pragma unroll
    for (int s = 0; s < NS; s++) acc[s] = low[s] = 0.0;
    const int64_t i0 = (int64_t)blockIdx.x * GMM_BLOCK_POINTS;
    for (int j = 0; j < GMM_BLOCK_POINTS / GMM_THREADS; j++) {
        const int64_t at = i0 + (int64_t)j * GMM_THREADS + threadIdx.x;
        if (at >= n) break;
        const double xj = x[at];
        double r[K];
        double l_max = -GMM_DBL_MAX;
#pragma unroll
        for (int i = 0; i < K; i++) {
            const double d = xj - mean[i];
            r[i] = la[i] + (cv[i] - (d * d) / tv[i]);
            if (r[i] > l_max) l_max = r[i];
        }
        double sum = 0.0;
#pragma unroll
        for (int i = 0; i < K; i++) sum += exp(r[i] - l_max);
        const double tmp = l_max + log(sum);
        gmm_add(acc[3 * K], low[3 * K], tmp);
        double den = 0.0;
#pragma unroll
        for (int i = 0; i < K; i++) {
            r[i] = exp(r[i] - tmp);
            den += r[i];
        }
#pragma unroll
        for (int k = 0; k < K; k++) {
            gmm_add(acc[k], low[k], r[k] / den);
            gmm_add(acc[K + k], low[K + k], xj * r[k] / den);
            gmm_add(acc[2 * K + k], low[2 * K + k], xj * xj * r[k] / den);
        }
    }
    gmm_block_sums<NS>(acc, low, red, tot);
    if ((int)threadIdx.x < 2 * NS) partial[(int64_t)threadIdx.x * n_blocks + blockIdx.x] = tot[threadIdx.x];
    if (n_blocks == 1) {                   // one workgroup: its own stores, read behind its own barrier
        __syncthreads();
        gmm_finish<K>(partial, n_blocks, n, log_n, precision, st, red, tot);
    }
}

template <int K> __global__ void __launch_bounds__(GMM_THREADS)
gmm_finish_kernel(const double *partial, int64_t n_blocks, int64_t n, double log_n, double precision, GmmState *st)
{
    constexpr int NS = 3 * K + 1;
    __shared__ double red[GMM_WAVES * 2 * NS];
    __shared__ double tot[2 * NS];
    if (st->converged) return;
    gmm_finish<K>(partial, n_blocks, n, log_n, precision, st, red, tot);
}

constexpr int GMM_BATCH = 64;              // updates enqueued between two reads of the state

// `updates` iterations on stream s: the pass, and behind a multi-block pass its finish
template <int K> void gmm_enqueue(hipStream_t s, const double *d_x, int64_t n, int64_t n_blocks, double log_n, double precision,
                                  GmmState *st, double *partial, int updates)
{
    for (int u = 0; u < updates; u++) {
        hipLaunchKernelGGL(gmm_em_kernel<K>, dim3((unsigned)n_blocks), dim3(GMM_THREADS), 0, s, d_x, n, n_blocks, log_n, precision, st, partial);
        if (n_blocks > 1)
            hipLaunchKernelGGL(gmm_finish_kernel<K>, dim3(1), dim3(GMM_THREADS), 0, s, partial, n_blocks, n, log_n, precision, st);
    }
}

} // namespace garlic
