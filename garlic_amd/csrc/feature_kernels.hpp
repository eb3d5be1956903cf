// count_features_in_roh.pl (the reference's src/) on the device: for every individual, the homozygous genotypes of annotated
// alleles inside ROH of each size class and outside any ROH.  The script runs one binary search per (variant, individual);
// here the work is a merge join of two sorted lists per individual -- the annotated rows (sorted by chromosome, position)
// and the individual's classified intervals (sorted the same way, not overlapping) -- and all of it is integer.
//
//   * hom rows: one row per annotated (site, allele), bit i = individual i is homozygous for that allele.  Block-major on the
//     device: word [blk][row] holds the 64 individuals of block blk, so the rows of one block are contiguous (the layout of
//     the phase planes, filled by phase_bits_planes_kernel, which also clears the bits past the last individual).
//   * feature_counts_kernel: one wavefront = one 64-individual block x FEAT_CHUNK_ROWS consecutive rows; lanes own
//     individuals.  The rows are read a tile of 64 at a time, lane j the word of row j (one 512-B load); chromosome,
//     position and effect of a row are loaded only where its word is not zero.  Homozygotes of rare alleles are sparse, so
//     most words are zero and cost nothing more: the loop over a tile visits the set bits of a ballot.  A visited row's
//     word, chromosome, position and effect are broadcast from their lane; the lanes whose bit is set advance a cursor
//     into their own interval list (placed once per chunk by binary search at the chunk's first row, then only ever moved
//     forward: rows and intervals are sorted alike) and add one to their counter [class][effect] in LDS.
//   * inside an interval: start <= position < stop.  stop is the `end` column of a .roh.bed line, where the writer puts
//     the LAST SNP's position: the script subtracts one, so a variant exactly there counts as outside.  Reproduced.
//   * counters: int32 [class][effect][lane] in LDS, a lane only ever touches its own column (no barrier, no LDS atomics, no
//     bank conflicts: lane l is bank l mod 32, the two halves are separate lane groups).  A chunk holds 4096 rows, so no
//     counter overflows.  Flushed once per wavefront with integer atomic adds into counts[ind][n_classes + 1][n_effects]
//     (int64; class n_classes is NONE): integer sums are exact in any order, so the result is the same from run to run.
//   * a launch counts the effects [e0, e0 + ge), ge <= FEAT_GROUP_EFFECTS, and passes over rows of other effects; more
//     effects are further launches.  The rows' words are then read once per launch.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace garlic {

constexpr int FEAT_CHUNK_ROWS = 4096;      // rows per wavefront (garlic_feature_counts_info reports the chunks)
constexpr int FEAT_GROUP_EFFECTS = 32;     // effects per launch
constexpr int FEAT_MAX_CLASSES = 8;        // GARLIC_GMM_MAX_K
constexpr int FEAT_MAX_EFFECTS = 256;      // GARLIC_FEATURE_MAX_EFFECTS

struct FeatInterval {                      // garlic_roh_interval
    int32_t ind, chr, start, stop, cls;
};

// bytes of LDS one wavefront needs for ge effects
inline size_t feature_counts_lds(int n_classes, int ge) { return (size_t)(n_classes + 1) * ge * 64 * sizeof(int32_t); }

__device__ __forceinline__ int feat_bcast(int v, int lane) { return __builtin_amdgcn_readlane(v, lane); }

__global__ void __launch_bounds__(64)
feature_counts_kernel(const uint64_t *__restrict__ bits, const int32_t *__restrict__ row_chr, const int32_t *__restrict__ row_pos,
                      const int32_t *__restrict__ row_eff, int64_t nrows, int nind, int64_t n_chunks,
                      const FeatInterval *__restrict__ iv, const int32_t *__restrict__ iv_off, int n_classes, int n_effects, int e0,
                      int ge, unsigned long long *__restrict__ counts, unsigned long long *__restrict__ skipped)
{
    extern __shared__ int32_t feat_cnt[];          // [(cls * ge + effect - e0) * 64 + lane]
    const int lane = threadIdx.x;
    const int64_t blk = (int64_t)blockIdx.x / n_chunks, chunk = (int64_t)blockIdx.x % n_chunks;
    const int64_t r0 = chunk * FEAT_CHUNK_ROWS, r1 = min(r0 + (int64_t)FEAT_CHUNK_ROWS, nrows);
    const int64_t ind = blk * 64 + lane;
    const bool valid = ind < nind;
    const int n_slots = (n_classes + 1) * ge;
    for (int s = 0; s < n_slots; s++) feat_cnt[s * 64 + lane] = 0;

    // the lane's intervals and its cursor: the first interval that does not lie wholly before the chunk's first row
    int cur = 0, end = 0;
    if (valid) {
        cur = iv_off[ind];
        end = iv_off[ind + 1];
    }
    {
        const int c0 = row_chr[r0], p0 = row_pos[r0];
        int lo = cur, hi = end;
        while (lo < hi) {
            const int mid = lo + ((hi - lo) >> 1);
            const FeatInterval m = iv[mid];
            if (m.chr < c0 || (m.chr == c0 && m.stop <= p0)) lo = mid + 1;
            else hi = mid;
        }
        cur = lo;
    }
    int ic = 0, istart = 0, istop = 0, icls = 0;               // the interval at the cursor (read only while cur < end)
    if (cur < end) {
        const FeatInterval m = iv[cur];
        ic = m.chr; istart = m.start; istop = m.stop; icls = m.cls;
    }

    const uint64_t *words = bits + blk * nrows;
    unsigned zero_words = 0;
    bool any = false;
    for (int64_t t0 = r0; t0 < r1; t0 += 64) {
        const int64_t r = t0 + lane;
        uint64_t w = 0;
        int c = 0, p = 0, e = -1;
        if (r < r1) {
            w = words[r];
            if (w != 0) {
                c = row_chr[r];
                p = row_pos[r];
                e = row_eff[r];
            }
        }
        zero_words += (unsigned)__popcll(__ballot(r < r1 && w == 0));
        uint64_t todo = __ballot(w != 0 && (unsigned)(e - e0) < (unsigned)ge);
        const int wlo = (int)(uint32_t)w, whi = (int)(uint32_t)(w >> 32);
        while (todo) {
            const int j = __ffsll((unsigned long long)todo) - 1;
            todo &= todo - 1;
            const uint32_t half = (uint32_t)(lane < 32 ? feat_bcast(wlo, j) : feat_bcast(whi, j));
            const int rc = feat_bcast(c, j), rp = feat_bcast(p, j), re = feat_bcast(e, j);
            if (valid && ((half >> (lane & 31)) & 1u)) {
                while (cur < end && (ic < rc || (ic == rc && istop <= rp))) {
                    cur++;
                    if (cur < end) {
                        const FeatInterval m = iv[cur];
                        ic = m.chr; istart = m.start; istop = m.stop; icls = m.cls;
                    }
                }
                const int cls = (cur < end && ic == rc && istart <= rp) ? icls : n_classes;
                feat_cnt[(cls * ge + (re - e0)) * 64 + lane] += 1;
                any = true;
            }
        }
    }
    if (skipped && lane == 0 && zero_words) atomicAdd(skipped, (unsigned long long)zero_words);
    if (!any) return;
    unsigned long long *mine = counts + ind * (int64_t)(n_classes + 1) * n_effects;
    for (int cls = 0; cls <= n_classes; cls++)
        for (int k = 0; k < ge; k++) {
            const int32_t v = feat_cnt[(cls * ge + k) * 64 + lane];
            if (v) atomicAdd(mine + (int64_t)cls * n_effects + e0 + k, (unsigned long long)v);
        }
}

} // namespace garlic
