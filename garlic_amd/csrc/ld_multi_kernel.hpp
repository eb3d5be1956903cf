// The LD weights of several window sizes from ONE pass of ordered sums (garlic_panel_compute_ld_multi).
//
//   LD_W[s][k] = 0.0 + sum_{i = s .. s+W-1, in this order} (i == s+k ? 1 : c(i, s+k))       (ld_kernels.hpp)
//
// The pair value c does not depend on W, so for W' < W and k < W' the accumulator of LD_W[s][k] after its first W'
// terms IS LD_W'[s][k]: same operands, same order, same roundings.  ld_sum_multi_kernel is ld_sum_col_kernel at the
// largest size of a group (thread = SNP of the window, 32 accumulators = window starts, rows of the combined table by
// LDS-DMA in batches, the adds behind the computed jump, XCD-contiguous block numbering) and takes a SNAPSHOT of the
// running sums for every smaller size: at step j (SNP i = s0 + j), after the adds, the start q = j - W' + 1 has
// received exactly the terms i = s0+q .. s0+q+W'-1.
//
// Differences from ld_sum_col_kernel:
//   - the table pitch is 2 * Wtab with Wtab >= W (one pair stage at the largest size of a call serves every group)
//   - the grid covers the starts s <= nloci_c - Wmin of a chromosome; a start past nloci_c - W accumulates up to the
//     chromosome's last SNP only and is snapshot for the sizes that still have a full window there -- no row past the
//     chromosome's end is requested, and no accumulator that received fewer than W' terms is stored for W'
//   - acc[q] with q wave-uniform but dynamic leaves its register through a second jump table (ld_col_pick)
//   - the skewed weights D'[(s0+tl) W' + tl - q] of a snapshot go to an LDS tile [thread][LDMS_CHUNK starts] of the
//     size; when a chunk is complete each wave writes the rows of its own 64 threads, LDMS_CHUNK consecutive doubles
//     per row (wave-local: no workgroup barrier)
// What the kernel leaves alone in D' is what ld_sum_col_kernel would leave alone at W': every D'[l][k] whose start
// l - k has a full window of W' inside the chromosome is written (the grid reaches every such start), so the entries
// not written belong to windows without a score, as for the single-size kernel.
#pragma once
#include "ld_kernels.hpp"

namespace garlic {

constexpr int LDM_MAX_SIZES = 4;                     // sizes per launch (not tuned; as TGM_MAX_SIZES)
constexpr int LDMS_CHUNK = 8;                        // snapshot starts per flush of a size's D tile
constexpr int LDMS_PITCH = LDMS_CHUNK + 1;           // doubles per thread in a tile (odd: conflict-free both ways)
constexpr size_t LDMS_LDS_MAX = 128 * 1024;          // bytes of LDS a launch may ask for (of the CU's 160 KB)

struct LdMultiChr {      // one chromosome's share of the grid
    int64_t lo, hi;      // its SNPs
    int64_t nstarts;     // hi - lo - Wmin + 1 (>= 1): starts with a full window of the smallest size
    int64_t block0;      // first workgroup of the chromosome
};
struct LdMultiSmall {    // the sizes below the launch's W, ascending
    int32_t n;
    int32_t w[LDM_MAX_SIZES - 1];
    double *ld[LDM_MAX_SIZES - 1];     // LD matrix [nloci][w] or NULL
    double *d[LDM_MAX_SIZES - 1];      // skewed weights (behind SKEW_FRONT)
};

// doubles of LDS in front of the snapshot tiles: ld_sum_col_kernel's ring and its slack
__host__ __device__ constexpr size_t ldms_ring_doubles(int pieces)
{
    return (size_t)LD_COL_BATCH * LD_COL_NBATCH * pieces * 128 + 130;
}
// bytes of LDS of a launch at W (threads = W + 16 in whole waves) with n_small snapshot sizes
inline size_t ldms_lds_bytes(int threads, int n_small)
{
    const int pieces = (threads * 8 + 1023) / 1024;
    const size_t ring_and_tiles = ldms_ring_doubles(pieces) + (size_t)n_small * threads * LDMS_PITCH;
    return sizeof(double) * (ring_and_tiles > (size_t)threads * 17 ? ring_and_tiles : (size_t)threads * 17);
}

// acc[q], q wave-uniform: a jump into 32 entries of {v_mov_b64, s_branch} (8 bytes each)
#define LD_COL_PICK(q) "v_mov_b64 %[t], %[a" #q "]\n\ts_branch LD_COL_PICKED_%=\n\t"
#define LD_COL_INS(a)                                                                                              \
    [a0] "v"(a[0]), [a1] "v"(a[1]), [a2] "v"(a[2]), [a3] "v"(a[3]), [a4] "v"(a[4]), [a5] "v"(a[5]),                \
    [a6] "v"(a[6]), [a7] "v"(a[7]), [a8] "v"(a[8]), [a9] "v"(a[9]), [a10] "v"(a[10]), [a11] "v"(a[11]),            \
    [a12] "v"(a[12]), [a13] "v"(a[13]), [a14] "v"(a[14]), [a15] "v"(a[15]), [a16] "v"(a[16]),                       \
    [a17] "v"(a[17]), [a18] "v"(a[18]), [a19] "v"(a[19]), [a20] "v"(a[20]), [a21] "v"(a[21]),                       \
    [a22] "v"(a[22]), [a23] "v"(a[23]), [a24] "v"(a[24]), [a25] "v"(a[25]), [a26] "v"(a[26]),                       \
    [a27] "v"(a[27]), [a28] "v"(a[28]), [a29] "v"(a[29]), [a30] "v"(a[30]), [a31] "v"(a[31])
__device__ __forceinline__ double ld_col_pick(const double (&a)[LD_COL_B], int q)
{
    static_assert(LD_COL_B == 32, "32 entries are written out");
    double t;
    const uint32_t off = (uint32_t)__builtin_amdgcn_readfirstlane(q * 8 + 12);
    asm volatile(LD_COL_JUMP
                 LD_COL_PICK(0) LD_COL_PICK(1) LD_COL_PICK(2) LD_COL_PICK(3) LD_COL_PICK(4) LD_COL_PICK(5) LD_COL_PICK(6)
                 LD_COL_PICK(7) LD_COL_PICK(8) LD_COL_PICK(9) LD_COL_PICK(10) LD_COL_PICK(11) LD_COL_PICK(12)
                 LD_COL_PICK(13) LD_COL_PICK(14) LD_COL_PICK(15) LD_COL_PICK(16) LD_COL_PICK(17) LD_COL_PICK(18)
                 LD_COL_PICK(19) LD_COL_PICK(20) LD_COL_PICK(21) LD_COL_PICK(22) LD_COL_PICK(23) LD_COL_PICK(24)
                 LD_COL_PICK(25) LD_COL_PICK(26) LD_COL_PICK(27) LD_COL_PICK(28) LD_COL_PICK(29) LD_COL_PICK(30)
                 LD_COL_PICK(31)
                 "LD_COL_PICKED_%=:\n\t"
                 : [t] "=&v"(t) : LD_COL_INS(a), [off] "s"(off) : "s98", "s99", "scc");
    return t;
}

// the snapshot of start q (0 <= q < nsz, wave-uniform) for the size Wz: LD_z[s0+q][tl - q] and, through the tile, D_z
__device__ __forceinline__ void ld_multi_snapshot(const double (&acc)[LD_COL_B], int q, int Wz, int nsz, int64_t s0, int tl,
                                                  double *__restrict__ ldz, double *__restrict__ Dz, double *tile)
{
    const double v = x86_nan_if_nan(ld_col_pick(acc, q));
    const int k = tl - q;
    if (ldz && k >= 0 && k < Wz) ldz[(s0 + q) * Wz + k] = v;
    if (!Dz) return;
    const int u = q & (LDMS_CHUNK - 1);
    tile[tl * LDMS_PITCH + u] = reciprocal_x86(v);
    if (u != LDMS_CHUNK - 1 && q != nsz - 1) return;
    // the chunk q0 .. q is complete: row s0 + t2 of D_z takes its thread's values back to front, the rows of this
    // wave's own threads (the tile entries of a wave are written and read by that wave alone, in program order)
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    const int q0 = q - u, lane = tl & 63, t0 = tl - lane;
    for (int e = lane; e < WAVE * LDMS_CHUNK; e += WAVE) {
        const int t2 = t0 + e / LDMS_CHUNK, uu = e % LDMS_CHUNK, qq = q0 + uu, kk = t2 - qq;
        if (qq <= q && kk >= 0 && kk < Wz) Dz[(s0 + t2) * Wz + kk] = tile[t2 * LDMS_PITCH + uu];
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
}

template <int PIECES>
__global__ void __launch_bounds__(LD_COL_MAX_THREADS)
ld_sum_multi_kernel(const double *__restrict__ C, const LdMultiChr *__restrict__ chrs, int nchr, int Wtab, int W, int B,
                    LdMultiSmall small, double *__restrict__ ld, double *__restrict__ D, unsigned nwork)
{
    const unsigned per_xcd = gridDim.x >> 3;                   // (gridDim.x is a multiple of 8: see ld_sum_col_kernel)
    const unsigned vblock = (blockIdx.x & 7u) * per_xcd + (blockIdx.x >> 3);
    if (vblock >= nwork) return;
    constexpr int BATCH = LD_COL_BATCH, NB = LD_COL_NBATCH, NRING = BATCH * NB, STEADY = (NB - 2) * BATCH * PIECES;
    static_assert(STEADY <= 63, "requests that can be counted");
    extern __shared__ double ld_rows[];
    const int tl = threadIdx.x, P = 2 * Wtab, nthreads = blockDim.x;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    int c = 0;
    while (c + 1 < nchr && (int64_t)vblock >= chrs[c + 1].block0) c++;
    const int64_t s0 = chrs[c].lo + ((int64_t)vblock - chrs[c].block0) * B, hi = chrs[c].hi;
    const int ns = (int)min<int64_t>(B, chrs[c].lo + chrs[c].nstarts - s0);
    // starts of the workgroup with a full window of a size: s0 + q + W' <= hi
    auto full = [&](int w) { return (int)max<int64_t>(0, min<int64_t>(ns, hi - w + 1 - s0)); };
    const int ns_top = full(W);
    int nsz[LDM_MAX_SIZES - 1];
#pragma unroll
    for (int z = 0; z < LDM_MAX_SIZES - 1; z++) nsz[z] = z < small.n ? full(small.w[z]) : 0;
    // the steps stop at the chromosome's last SNP
    const int nsteps = (int)min<int64_t>(ns + W - 1, hi - s0), nbatches = (nsteps + BATCH - 1) / BATCH;
    const uint32_t ring = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) double *)ld_rows;
    constexpr uint32_t row_bytes = (uint32_t)PIECES * 1024u, ring_bytes = row_bytes * NRING;
    const uint32_t lane16 = (uint32_t)(tl & 63) * 16u;
    const char *req_row = reinterpret_cast<const char *>(C + s0 * P);
    int req_e = Wtab - 1, req_left = nsteps;
    uint32_t req_off = 0;
    auto request_batch = [&]() {
#pragma unroll
        for (int u = 0; u < BATCH; u++) {
            if (req_left > 0) {
                const char *g = req_row + (int64_t)(req_e & ~1) * 8;
#pragma unroll
                for (int q = 0; q < PIECES; q++)
                    asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %2"
                                 :: "s"(ring + req_off + (uint32_t)q * 1024u), "v"(lane16), "s"(g + q * 1024) : "memory");
                req_row += (int64_t)P * 8;
                req_e--;
                req_left--;
            }
            req_off += row_bytes;
        }
        if (req_off == ring_bytes) req_off = 0;
    };
    if (wave == 0)
        for (int k = 0; k < NB - 1; k++) request_batch();
    double acc[LD_COL_B];
#pragma unroll
    for (int q = 0; q < LD_COL_B; q++) acc[q] = 0.0;
    double *tiles = ld_rows + ldms_ring_doubles(PIECES);          // [size][thread][LDMS_PITCH]
    uint32_t rd_addr = ring + (uint32_t)tl * 8u;
    const uint32_t rd_end = rd_addr + ring_bytes;
    const uint32_t odd = (uint32_t)(Wtab - 1) & 1u;
    static_assert(BATCH % 2 == 0, "the parity of Wtab-1-j repeats per batch");
    for (int k = 0; k < nbatches; k++) {
        if (wave == 0) {
            const int rows_later = min(nsteps, (k + NB - 1) * BATCH) - (k + 1) * BATCH;
            if (rows_later == (NB - 2) * BATCH) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(STEADY) : "memory");
            else ld_col_wait(max(rows_later, 0) * PIECES);
        }
        __syncthreads();
        if (wave == 0) request_batch();
        const int j0 = k * BATCH;
        double h[BATCH];
#pragma unroll
        for (int u = 0; u < BATCH; u++)
            asm volatile("ds_read_b64 %0, %1" : "=v"(h[u]) : "v"(rd_addr + (uint32_t)u * row_bytes + ((odd ^ (uint32_t)(u & 1)) * 8u)) : "memory");
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        rd_addr += BATCH * row_bytes;
        if (rd_addr == rd_end) rd_addr -= ring_bytes;
#pragma unroll
        for (int u = 0; u < BATCH; u++) {
            const int j = j0 + u;
            if (j < nsteps) {
                const bool leaving = j >= W;
                ld_col_adds(acc, h[u], leaving, leaving ? j - W + 1 : (j < LD_COL_B - 1 ? LD_COL_B - 1 - j : 0));
#pragma unroll
                for (int z = 0; z < LDM_MAX_SIZES - 1; z++) {
                    const int q = j - small.w[z] + 1;              // (z >= small.n: nsz[z] = 0)
                    if (q >= 0 && q < nsz[z])
                        ld_multi_snapshot(acc, q, small.w[z], nsz[z], s0, tl, small.ld[z], small.d[z],
                                          tiles + (size_t)z * nthreads * LDMS_PITCH);
                }
            }
        }
    }
    // the largest size leaves at the end, as in ld_sum_col_kernel (the starts with a full window of W)
    if (ld) {
#pragma unroll
        for (int q = 0; q < LD_COL_B; q++) {
            const int k = tl - q;
            if (q < ns_top && k >= 0 && k < W) ld[(s0 + q) * W + k] = x86_nan_if_nan(acc[q]);
        }
    }
    if (!D) return;
    __syncthreads();                                          // neither the ring nor a snapshot tile is read any more
    double *tile = ld_rows;
    for (int q0 = 0; q0 < LD_COL_B; q0 += 16) {
#pragma unroll
        for (int u = 0; u < 16; u++)
            if (q0 == 0) tile[tl * 17 + u] = reciprocal_x86(x86_nan_if_nan(acc[u]));
            else tile[tl * 17 + u] = reciprocal_x86(x86_nan_if_nan(acc[16 + u]));
        __syncthreads();
        for (int e = tl; e < nthreads * 16; e += nthreads) {
            const int t2 = e >> 4, u = e & 15, q = q0 + u, k = t2 - q;
            if (q < ns_top && k >= 0 && k < W) D[(s0 + t2) * W + k] = tile[t2 * 17 + u];
        }
        __syncthreads();
    }
}

// pair counts of a table [nloci][Wfrom][2] at the pitch of a narrower one: the counts of (i, i + d) do not depend on the width
__global__ void __launch_bounds__(256)
ld_pair_repitch_kernel(const int32_t *__restrict__ from, int Wfrom, int64_t nloci, int Wto, int32_t *__restrict__ to)
{
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= nloci * Wto) return;
    const int64_t i = e / Wto;
    const int d = (int)(e - i * Wto);
    *reinterpret_cast<int2 *>(to + e * 2) = *reinterpret_cast<const int2 *>(from + (i * Wfrom + d) * 2);
}

} // namespace garlic
