// TGLS with a 16-bit likelihood dictionary (GARLIC_TGLS_DICTIONARY16): printed GL / PL columns hold a few thousand
// distinct values after readTGLSData's clamp -- more than a one-byte dictionary, far fewer than genotypes.  The panel
// keeps uint16 codes in the term matrix's layout, codes[blk][rows][64] (2 B per genotype, a wave's 64 codes of a SNP
// are one 128-B row), and ONE panel-wide value table of at most 65,536 doubles (512 KB: it stays in every XCD's L2,
// so the look-up is a cached gather; it is not staged in LDS).  A per-SNP table of terms as the one-byte dictionary
// has (ncodes x 4 doubles per SNP) is out of the question, so the terms come from lod() evaluated on the device with
// glibc's log10 restated (tgls_math.hpp), as for continuous likelihoods, and every consumer reads the term matrix or
// its slabs.  The codes are never overwritten: terms, raw or scaled, whole or slab by slab, are rebuilt from them.
#pragma once
#include "variant_kernels.hpp"

namespace garlic {

constexpr int GL_WIDE_MAX = 65536;

// ---- ingest.  Caller rows [locus_count][ld] of uint16 codes into the caller's table -> the panel's codes
// (remap[caller code] = panel code, nremap entries; codes past the caller's table are taken as its code 0).
__global__ void __launch_bounds__(256)
gl_recode16_kernel(const uint16_t *__restrict__ rows_in, int64_t ld, int64_t l0, int64_t locus_count, int32_t nind,
                   const uint16_t *__restrict__ remap, int32_t nremap, int64_t rows, uint16_t *__restrict__ codes)
{
    const int64_t n = locus_count * nind;
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += (int64_t)gridDim.x * blockDim.x) {
        const int64_t l = e / nind;
        const int64_t i = e - l * nind;
        const int32_t c = rows_in[l * ld + i];
        codes[((i >> 6) * rows + GOFF + l0 + l) * WAVE + (i & 63)] = remap[c < nremap ? c : 0];
    }
}

// the same for one-byte caller codes (garlic_panel_set_gl_codes on a panel that holds 16-bit codes)
__global__ void __launch_bounds__(256)
gl_recode8to16_kernel(const uint8_t *__restrict__ rows_in, int64_t ld, int64_t l0, int64_t locus_count, int32_t nind,
                      const uint16_t *__restrict__ remap, int64_t rows, uint16_t *__restrict__ codes)
{
    const int64_t n = locus_count * nind;
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += (int64_t)gridDim.x * blockDim.x) {
        const int64_t l = e / nind;
        const int64_t i = e - l * nind;
        codes[((i >> 6) * rows + GOFF + l0 + l) * WAVE + (i & 63)] = remap[rows_in[l * ld + i]];
    }
}

// the one-byte dictionary grew past 256 values: its codes [rows][nind_pad] widened into codes16[blk][rows][64]
// (the code numbers stay: the 16-bit table begins with the one-byte table)
__global__ void __launch_bounds__(256)
gl_widen_kernel(const uint8_t *__restrict__ codes8, int64_t nind_pad, int64_t rows, uint16_t *__restrict__ codes16)
{
    const int64_t n = rows * nind_pad;
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += (int64_t)gridDim.x * blockDim.x) {
        const int64_t G = e / nind_pad;
        const int64_t i = e - G * nind_pad;
        codes16[((i >> 6) * rows + G) * WAVE + (i & 63)] = codes8[e];
    }
}

// the 16-bit dictionary is full as well: what has been coded becomes values (same layout: element for element)
__global__ void __launch_bounds__(256)
gl_decode16_kernel(const uint16_t *__restrict__ codes16, const double *__restrict__ values, int32_t nvalues, int64_t n,
                   double *__restrict__ vals)
{
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += (int64_t)gridDim.x * blockDim.x) {
        const int32_t c = codes16[e];
        vals[e] = c < nvalues ? values[c] : 0.0;
    }
}

// caller's 16-bit codes + value table straight to values (garlic_panel_set_gl_codes16 on a continuous panel)
__global__ void __launch_bounds__(256)
gl_store_codes16_kernel(const uint16_t *__restrict__ rows_in, int64_t ld, int64_t l0, int64_t locus_count, int32_t nind,
                        const double *__restrict__ dict, int32_t ndict, int64_t rows, double *__restrict__ vals)
{
    const int64_t n = locus_count * nind;
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += (int64_t)gridDim.x * blockDim.x) {
        const int64_t l = e / nind;
        const int64_t i = e - l * nind;
        const int32_t c = rows_in[l * ld + i];
        vals[((i >> 6) * rows + GOFF + l0 + l) * WAVE + (i & 63)] = dict[c < ndict ? c : 0];
    }
}

// garlic_panel_set_gl on a panel that holds 16-bit codes: doubles -> codes against the dictionary so far (dict_bits
// sorted, in global memory: 512 KB at most, 16 probes per value); values it does not know are reported as in
// gl_encode_kernel and the rows are run again once the host has extended the dictionary.
__global__ void __launch_bounds__(256)
gl_encode16_kernel(const double *__restrict__ gl, int64_t ld, int64_t l0, int64_t locus_count, int32_t nind,
                   const uint64_t *__restrict__ dict_bits, const uint16_t *__restrict__ dict_code, int ndict, int64_t rows,
                   uint16_t *__restrict__ codes, uint64_t *__restrict__ unknown, int32_t *__restrict__ n_unknown, int cap)
{
    const int64_t n = locus_count * nind;
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += (int64_t)gridDim.x * blockDim.x) {
        const int64_t l = e / nind;
        const int64_t i = e - l * nind;
        const uint64_t b = reinterpret_cast<const uint64_t *>(gl)[l * ld + i];
        int lo = 0, hi = ndict;                                 // first entry >= b
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (dict_bits[mid] < b) lo = mid + 1; else hi = mid;
        }
        if (lo < ndict && dict_bits[lo] == b) {
            codes[((i >> 6) * rows + GOFF + l0 + l) * WAVE + (i & 63)] = dict_code[lo];
        } else {
            const int k = atomicAdd(n_unknown, 1);
            if (k < cap) unknown[k] = b;
        }
    }
}

// ---- the term pass: terms[blk - b0][G][lane] = lod(genotype, freq[G], values[codes[blk][G][lane]]) for the blocks
// [b0, b1) and ALL padded rows -- the whole matrix (b0 = 0, b1 = nind_pad / 64) or one slab of it, slab-local like
// gl_terms_slab_kernel's.  A plain streaming kernel: lanes = individuals; per wave and SNP one 128-B code row and one
// 256-B genotype-word row in (the word serves 16 SNPs from the cache), 64 cached 8-B table reads, one 512-B term row
// out.  Pad rows have frequency 0 and pad columns genotype code 3 -> +0.0 whatever their code says (lod_term).
// decay != NULL: the slab of the weighted kernels, (term * nomut) * norec -- two separately rounded multiplications
// in that order, as gl_scale_kernel / gl_terms_slab_kernel make them (pad rows: +0.0 * 0.0 * 0.0 = +0.0).
// min_bits (GL_MIN_SLOTS entries, zeroed by the caller; may be NULL): the most negative finite RAW term, collected as
// in gl_terms_cont_kernel.
__global__ void __launch_bounds__(256)
gl_terms_wide_kernel(const uint32_t *__restrict__ packed, int64_t nwordrows, const double *__restrict__ freq,
                     const double *__restrict__ logtab, const uint16_t *__restrict__ codes, const double *__restrict__ values,
                     int32_t nvalues, const double *__restrict__ decay, int64_t rows, int b0, int b1,
                     double *__restrict__ terms, unsigned long long *__restrict__ min_bits)
{
    __shared__ double tab_s[256];
    __shared__ unsigned long long red[4];
    tab_s[threadIdx.x] = logtab[threadIdx.x];
    __syncthreads();
    const int lane = threadIdx.x & (WAVE - 1), wave = threadIdx.x >> 6;
    const int64_t g0 = (int64_t)blockIdx.x * 64;
    const int64_t g1 = min(rows, g0 + 64);
    double m = 0.0;
    for (int64_t blk = b0 + (int64_t)blockIdx.y; blk < b1; blk += gridDim.y) {
        const int64_t col = blk * WAVE + lane;
        for (int64_t G = g0 + wave; G < g1; G += 4) {
            const uint32_t word = packed[packed_index(G >> 4, col, nwordrows)];
            const uint32_t g = (word >> (2 * (int)(G & 15))) & 3u;
            const int32_t c = codes[(blk * rows + G) * WAVE + lane];
            const double v = values[c < nvalues ? c : 0];
            double t = lod_term(g, freq[G], v, tab_s);
            if (t < m && t > -1.7976931348623157e308) m = t;     // NaN and -inf fail the comparisons
            if (decay) t = (t * decay[2 * G]) * decay[2 * G + 1];
            terms[((blk - b0) * rows + G) * WAVE + lane] = t;
        }
    }
    if (min_bits) {
        unsigned long long b = m < 0.0 ? f64_bits(m) : 0ull;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) b = max(b, (unsigned long long)__shfl_xor((long long)b, o));
        if (lane == 0) red[wave] = b;
        __syncthreads();
        if (threadIdx.x == 0) {
            b = max(max(red[0], red[1]), max(red[2], red[3]));
            if (b) atomicMax(min_bits + ((blockIdx.x * 7u + blockIdx.y * 131u) & (unsigned)(GL_MIN_SLOTS - 1)), b);
        }
    }
}

} // namespace garlic
