/*
 * garlic_hip.h -- C ABI of libgarlic_hip.so: GARLIC Phase-I window LOD scores on MI355X (gfx950).
 *
 * This is the drop-in boundary for the one hot path this project replaces.  The reference
 * (szpiech/garlic v1.1.6a) has no FFI layer; the boundary is the pair of C++ entry points
 *
 *     calcLODWindows   src/garlic-roh.h:96-102   (body src/garlic-roh.cpp:279-309, calcLOD :18-132)
 *     calcwLODWindows  src/garlic-roh.h:104-112  (body src/garlic-roh.cpp:311-347, calcwLOD :144-277)
 *
 * and the structs they borrow (src/garlic-data.h:32-108).  Every function below takes plain
 * pointers and sizes; the C++ adapter in garlic_amd/host mirrors the reference signatures on top
 * (INTEGRATION.md shows the few lines a GARLIC maintainer would add).
 *
 * Conventions
 *   - Every call returns GARLIC_OK (0) or a GARLIC_ERR_* code; garlic_hip_last_error() gives the
 *     text for the calling thread.  The reference throws `int 0` (src/garlic-data.cpp:1619); the
 *     adapter converts non-zero to `throw 0`.
 *   - `where` says whether a caller buffer is host (GARLIC_HOST) or device (GARLIC_DEVICE) memory.
 *   - Loci of all chromosomes are concatenated in file order ("global locus index"); chromosome c
 *     owns [chr_off[c], chr_off[c+1]).
 *   - Genotypes are the reference's codes (src/garlic-data.cpp:109-129): 0,1,2 = copies of the
 *     counted allele, anything else (-9) = missing.
 *   - LOD output is individual-major like WinData::data (src/garlic-data.h:83): element
 *     (chr c, ind i, locus l) lives at  chr_base[c] + i*chr_pitch[c] + l  (in doubles), see
 *     garlic_lod_out_layout().  Windows that hold no score are exactly -9999.0
 *     (MISSING, src/garlic-data.h:24); every element is written by the call, no pre-fill needed.
 *   - Results are bit-identical to the reference's doubles on the same inputs and host libm.
 *   - A context is bound to one device and one HIP stream; calls on one context must not overlap
 *     in time, different contexts are independent (one per GPU for individual sharding).
 */
#ifndef GARLIC_HIP_H
#define GARLIC_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 2: the LD functions take `phased`; garlic_panel_set_phase
 * 3: likelihoods may be continuous (no 256-value limit), garlic_panel_tgls_mode; an LD subsample may be
 *    empty (sub_idx != NULL, n_sub = 0); garlic_lod_feed_subset
 * 4: garlic_device_alloc / garlic_device_free (score matrices), garlic_panel_chain_kind
 * 5: garlic_lod_feed_multi (the feeds of several window sizes in one call); garlic_panel_alloc_scores,
 *    garlic_device_alloc_stats, garlic_device_trim
 * 6: garlic_roh_coverage_fused (coverage counts without the score matrix)
 * 7: garlic_roh_segments (the ROH segments of assembleROHWindows without scores or counts)
 * 8: garlic_call_stats::n_stall_reruns / n_count_timeouts, garlic_panel_alloc_scores_info; garlic_lod_feed_info (added
 *    under the same number: nothing that existed changed); GARLIC_FEED_TGLS_CHAIN (a fourth value of its form, likewise);
 *    garlic_panel_set_tgls_term_budget, garlic_panel_tgls_terms_info (likewise); garlic_lod_feed_multi_tgls,
 *    garlic_lod_feed_multi_info, GARLIC_FEED_TGLS_CHAIN_SHARED (likewise); garlic_panel_compute_ld_multi,
 *    garlic_ld_finish_multi, garlic_panel_ld_info (likewise); garlic_panel_set_feed_order, garlic_feed_sort,
 *    garlic_feed_sort_info, GARLIC_FEED_ORDER_* (likewise); garlic_panel_set_phase_bits, garlic_panel_ld_form_info,
 *    GARLIC_LD_PAIR_* / GARLIC_LD_SUM_* (likewise); garlic_panel_set_gl_codes16, GARLIC_TGLS_DICTIONARY16 (likewise);
 *    garlic_bed_create, garlic_bed_set_rows, garlic_bed_census, garlic_bed_destroy, garlic_panel_set_genotypes_bed (likewise);
 *    garlic_kde, GARLIC_KDE_POINTS, garlic_feed_kde, garlic_lod_kde, garlic_feed_kde_info, garlic_feed_kde_times (likewise);
 *    garlic_gmm, GARLIC_GMM_MAX_K, garlic_gmm_fit, garlic_gmm_fit_info (likewise); garlic_kde_part,
 *    GARLIC_KDE_MAX_PARTS, garlic_kde_part_create, garlic_lod_kde_part, garlic_kde_part_destroy, garlic_kde_part_count,
 *    garlic_kde_part_moment, garlic_kde_part_rank, garlic_kde_part_sums, garlic_kde_parts, garlic_kde_parts_info (likewise);
 *    garlic_feature_set, garlic_roh_interval, GARLIC_FEATURE_MAX_EFFECTS, garlic_feature_set_create,
 *    garlic_feature_set_destroy, garlic_feature_set_rows, garlic_feature_set_sites, garlic_feature_counts,
 *    garlic_feature_counts_info (likewise); GARLIC_KDE_MAX_FEEDS, garlic_feed_kde_multi, garlic_lod_kde_multi,
 *    garlic_feed_kde_multi_info (likewise); garlic_kde_part_set, garlic_kde_part_set_create, garlic_lod_kde_part_set,
 *    garlic_kde_part_set_destroy, garlic_kde_part_set_counts, garlic_kde_part_set_moment, garlic_kde_part_set_rank,
 *    garlic_kde_part_set_sums, garlic_kde_parts_multi, garlic_kde_parts_multi_info (likewise); garlic_bed_extract,
 *    garlic_bed_get_rows (likewise); garlic_feature_set_rows_bed, garlic_feature_set_get_rows (likewise);
 *    garlic_bed_set_order_rows, garlic_bed_get_order_rows, garlic_bed_set_rows_vcf, GARLIC_VCF_*, garlic_panel_set_phase_bed
 *    (likewise); garlic_tgls, garlic_tgls_create, garlic_tgls_set_rows_text, garlic_tgls_set_rows_values, garlic_tgls_get_rows,
 *    garlic_tgls_info, garlic_tgls_count_values, garlic_tgls_get_values, garlic_tgls_destroy, garlic_panel_set_gl_tgls, GARLIC_TGLS_OK / _DEFERRED / _FEW_COLUMNS /
 *    _MANY_COLUMNS / _RAW, GARLIC_ERR_RANGE (likewise); garlic_bed_set_rows_tped, GARLIC_TPED_*, garlic_bed_set_census (likewise);
 *    garlic_tgls_set_rows_vcf, GARLIC_TGLS_VCF_NO_KEY / _NO_VALUE, garlic_device_upload (likewise); garlic_bgzf_inflate,
 *    GARLIC_BGZF_*, garlic_text_lines, garlic_device_download, garlic_device_copy (likewise) */
#define GARLIC_HIP_ABI_VERSION 8

#define GARLIC_OK 0
#define GARLIC_ERR_INVALID 1  /* bad argument (e.g. winsize <= 1: src/garlic-cli.cpp:433-442) */
#define GARLIC_ERR_HIP 2      /* HIP runtime failure / no gfx950 device */
#define GARLIC_ERR_STATE 3    /* inputs missing for the requested computation */
#define GARLIC_ERR_NOMEM 4
#define GARLIC_ERR_RANGE 5    /* the input is outside what the object can hold (garlic_tgls: a 65,537th distinct raw value) */

#define GARLIC_HOST 0
#define GARLIC_DEVICE 1

#define GARLIC_MISSING (-9999.0)

#define GARLIC_GL_GQ 0 /* --gl-type GQ, src/garlic-data.cpp:1557 */
#define GARLIC_GL_GL 1 /* --gl-type GL, src/garlic-data.cpp:1562 */
#define GARLIC_GL_PL 2 /* --gl-type PL, src/garlic-data.cpp:1566 */

typedef struct garlic_ctx garlic_ctx;
typedef struct garlic_panel garlic_panel;

int garlic_hip_abi_version(void);
const char *garlic_hip_last_error(void);
int garlic_hip_device_count(int32_t *count);

/* Context: device ordinal + stream.  hip_stream == NULL: the context creates its own stream;
 * otherwise a hipStream_t owned by the caller (e.g. torch's current stream).  On a caller's stream the calls keep plain
 * stream order: a device buffer that stream is still writing when a `where = GARLIC_DEVICE` call starts is read with its
 * final contents, and a device output is complete for whatever the caller enqueues next on it
 * (tests/test_gpu_caller_stream.py).
 * The DEFAULT (null) stream cannot be handed over: its handle is 0, which is the NULL that means "create my own", so
 * e.g. torch.cuda.current_stream().cuda_stream on torch's default stream silently gives a private non-blocking stream
 * that is not ordered with the caller's work.  Pass a stream created for the purpose (torch.cuda.Stream()). */
int garlic_ctx_create(int32_t device, void *hip_stream, garlic_ctx **ctx);
int garlic_ctx_destroy(garlic_ctx *ctx);
int garlic_ctx_synchronize(garlic_ctx *ctx);
/* By default every call returns after its device work has finished.  With on != 0,
 * garlic_lod_windows / garlic_wlod_windows calls whose output stays on the device and whose
 * arguments repeat the previous call's (same window size, range, layout: the work plan is reused)
 * only enqueue their kernels on the context's stream; garlic_ctx_synchronize (or
 * garlic_last_call_stats, or any synchronous call) waits.  For callers that issue passes back to
 * back (benchmarks, pipelines that consume the scores on the same stream). */
int garlic_ctx_set_async(garlic_ctx *ctx, int32_t on);

/* Device memory for score matrices (the `out` of garlic_lod_windows & co. with GARLIC_DEVICE): any device pointer
 * works as `out`; garlic_device_alloc / garlic_device_free / garlic_panel_alloc_scores (below, by the other score
 * calls) hand out memory the unweighted kernel runs fastest into.  GARLIC itself has no counterpart (WinData rows
 * are host memory, garlic-data.cpp:1690); keep the buffer across window sizes as GARLIC keeps its WinData. */
/* HIP-event durations (ms) of the dominant kernel of the context's most recent window-score calls,
 * oldest first, at most 32: lets a caller time asynchronous passes without waiting for each.  Waits
 * for the stream.  *got = number of values written (<= n). */
int garlic_recent_kernel_ms(garlic_ctx *ctx, float *ms, int32_t n, int32_t *got);

/* Panel = what calcLODWindows borrows: HapData / MapData / FreqData (/ GenoLikeData / LDData)
 * of every chromosome, for the nind individuals this context owns (a shard of the TFAM order).
 * chr_nloci[c] = MapData::nloci of chromosome c (src/garlic-data.h:58). */
int garlic_panel_create(garlic_ctx *ctx, int32_t nchr, const int32_t *chr_nloci, int32_t nind,
                        garlic_panel **panel);
int garlic_panel_destroy(garlic_panel *panel);

/* MapData::physicalPos / geneticPos (src/garlic-data.h:53-54) concatenated over chromosomes
 * (host arrays), and centromere::centromereStart/End per chromosome
 * (src/garlic-roh.cpp:36-37; unknown chromosome => 0,0).  gpos may be NULL (unweighted). */
int garlic_panel_set_map(garlic_panel *panel, const int32_t *pos, const double *gpos,
                         const int32_t *centro_start, const int32_t *centro_end);

/* FreqData::freq concatenated (host array, src/garlic-data.h:71). */
int garlic_panel_set_freq(garlic_panel *panel, const double *freq);

/* HapData::data rows (src/garlic-data.h:35) for global loci [locus_begin, locus_begin+locus_count):
 * geno[(l - locus_begin) * ld + i] is individual i of this shard (ld >= nind lets a shard read a
 * column block of the full matrix).  May be called repeatedly to stream a panel in chunks.
 * Device side: 2-bit packed, 16 loci per 32-bit word, individual-minor. */
int garlic_panel_set_genotypes(garlic_panel *panel, const int16_t *geno, int64_t ld,
                               int64_t locus_begin, int64_t locus_count, int32_t where);

/* The same genotypes from SNP-major 2-bit rows -- what a genotype cache or a bed-like reader holds:
 * 4 genotypes per byte, codes 0/1/2 = HapData::data values, 3 = missing (-9).  Row l - locus_begin
 * starts at rows + (l - locus_begin) * row_bytes and holds the individuals of the WHOLE data set;
 * this shard's individual i is number ind_offset + i of the row (byte / 4, bits 2 * (% 4)).
 * An eighth of the host memory and PCIe traffic of the int16 rows; same device layout. */
int garlic_panel_set_genotypes_2bit(garlic_panel *panel, const uint8_t *rows, int64_t row_bytes,
                                    int64_t ind_offset, int64_t locus_begin, int64_t locus_count,
                                    int32_t where);

/* PLINK .bed input.  A garlic_bed is the SNP-major .bed image of a data set on the context's device: nrows rows of
 * (nind_total + 3) / 4 bytes, individual j of a row at bits 2 * (j % 4) of byte j / 4, in PLINK's codes 00 hom A1,
 * 01 missing, 10 het, 11 hom A2; the bits past individual nind_total - 1 are ignored, whatever they hold.  (The three magic
 * bytes 6c 1b 01 of the file are the caller's to check and skip.)  1 <= nrows < 2^31, 1 <= nind_total < 2^30 (the counts are
 * int32).  Calls on one image, like calls on one context, must not overlap in time; panels of several contexts on the image's
 * device may fill from it one after the other.
 *   garlic_bed_set_rows  rows [row_begin, row_begin + row_count) from `rows`, row_bytes apart (>= (nind_total + 3) / 4:
 *                        padded sources are fine; no alignment is asked for); host or device memory; in as many calls as
 *                        the caller likes, a row may be set again.
 *   garlic_bed_census    per row, GARLIC's counted allele -- "the first non-missing allele on the line"
 *                        (src/garlic-data.cpp:107-113) of the TPED line the row stands for, on which a hom A1 genotype reads
 *                        "A1 A1", a het "A1 A2" and a hom A2 "A2 A2": A2 when the first non-missing genotype in file order is
 *                        hom A2, A1 otherwise, none when every genotype is missing -- as counted[r] = 0 (A1), 1 (A2), 2
 *                        (none), and counts[r] = {nalleles, total} = {2 * #hom(counted) + #het, 2 * #non-missing} ({0, 0}
 *                        for none), the two integers of the reference's frequency double(nalleles) / double(total) (:141).
 *                        GARLIC_ERR_STATE until every row has been set.  Computed once per image content and kept with it;
 *                        either output may be NULL.
 *   garlic_panel_set_genotypes_bed   recodes rows of the image into the panel (copies of the row's counted allele 0 / 1 / 2,
 *                        missing 3; a row whose counted allele is none: all 3): dest_locus[r] (host array, nrows entries) is
 *                        the panel's global locus for file row r, or -1 for a row the caller's site filters dropped.  The
 *                        destinations of the kept rows must be strictly ascending (GARLIC_ERR_INVALID otherwise) and need not
 *                        be consecutive; loci no row maps to keep their previous bits.  The panel's individual i is individual
 *                        ind_offset + i of the row (a shard's column block).  The panel's context must be on the image's
 *                        device.  Runs the census first when it has not been run.  Otherwise the effect of
 *                        garlic_panel_set_genotypes_2bit. */
typedef struct garlic_bed garlic_bed;
int garlic_bed_create(garlic_ctx *ctx, int64_t nrows, int32_t nind_total, garlic_bed **bed);
int garlic_bed_set_rows(garlic_bed *bed, const uint8_t *rows, int64_t row_bytes, int64_t row_begin, int64_t row_count,
                        int32_t where);
int garlic_bed_census(garlic_bed *bed, int32_t *counts /* [nrows][2]: nalleles, total */, uint8_t *counted /* [nrows] */,
                      int32_t where);
int garlic_panel_set_genotypes_bed(garlic_panel *panel, garlic_bed *bed, int64_t ind_offset,
                                   const int64_t *dest_locus /* [nrows] */);
int garlic_bed_destroy(garlic_bed *bed);
/* A column subset of an image as a new image on the same context and device -- one population of a multi-population file:
 * nrows = src's, nind_total = n_idx, and individual i of every new row is individual ind_idx[i] of the same row of src, in
 * PLINK's codes, unchanged; rows of (n_idx + 3) / 4 bytes back to back, the pad bits behind individual n_idx - 1 zero.
 * ind_idx is a host array in any order, repeats allowed, every entry in [0, src nind_total).  The result is complete (every
 * row set), its census has not been run, and it is an ordinary garlic_bed: garlic_bed_census is the census of the subset
 * alone in ind_idx order ("first non-missing genotype" = first in the new row), garlic_panel_set_genotypes_bed cuts shards
 * out of it by ind_offset, garlic_bed_destroy frees it.  It does not depend on src once the call has returned (src may be
 * destroyed); it shares src's context, which must outlive it.  The work runs on the context's stream.
 * GARLIC_ERR_STATE: src is not fully set.  GARLIC_ERR_INVALID: NULL arguments, n_idx < 1, n_idx >= 2^30, an index out of
 * range (the message names the first).  GARLIC_ERR_NOMEM: the new image does not fit; *out is untouched and nothing is left
 * allocated. */
int garlic_bed_extract(garlic_bed *src, const int32_t *ind_idx, int32_t n_idx, garlic_bed **out);
/* Rows [row_begin, row_begin + row_count) of an image, row_bytes (>= (nind_total + 3) / 4) apart, to host or device memory;
 * bytes past a row's own are untouched.  (What garlic_bed_set_rows put in, or what garlic_bed_extract made.) */
int garlic_bed_get_rows(garlic_bed *bed, int64_t row_begin, int64_t row_count, uint8_t *rows, int64_t row_bytes,
                        int32_t where);

/* The order plane of an image: one bit per genotype, 1 = "the genotype's first allele is A2" (a VCF's `1|0`, `1|1`), 0 for a
 * missing genotype; rows of (nind_total + 7) / 8 bytes back to back, bit i & 7 of byte i >> 3 of a row is individual i, the
 * bits past the last individual are ignored (the VCF call writes them as zeros).  A .bed has no such thing: an image gets its
 * plane, all zeros, with the first set_order_rows or set_rows_vcf call, and without one it behaves as before.  With a plane,
 *   garlic_bed_census   counts A2 when the first non-missing genotype in file order has its order bit set, A1 otherwise --
 *                       "the first non-missing allele on the line" of the TPED line on which every genotype reads in the
 *                       VCF's own allele order; nalleles and total follow the counted allele as before;
 *   garlic_bed_extract  is not built: GARLIC_ERR_INVALID.
 * garlic_bed_set_order_rows / garlic_bed_get_order_rows take the arguments of garlic_bed_set_rows / garlic_bed_get_rows
 * (row_bytes >= (nind_total + 7) / 8); get: GARLIC_ERR_STATE on an image without a plane. */
int garlic_bed_set_order_rows(garlic_bed *bed, const uint8_t *rows, int64_t row_bytes, int64_t row_begin, int64_t row_count,
                              int32_t where);
int garlic_bed_get_order_rows(garlic_bed *bed, int64_t row_begin, int64_t row_count, uint8_t *rows, int64_t row_bytes,
                              int32_t where);
/* Image rows and order rows [row_begin, row_begin + row_count) parsed on the device from VCF text.  `text` is a slab of
 * text_bytes bytes in host or device memory (no alignment asked for; the device reads the aligned 16-byte pieces that overlap
 * the slab and nothing else).  line_begin (host, row_count + 1 ascending offsets) names the data lines: line_begin[r] is the
 * first byte of the line that becomes row row_begin + r, and the line ends at its own '\n', at line_begin[r + 1] or at
 * text_bytes, whichever comes first -- lines the caller leaves out simply lie between two kept ones.  Of a line, nine
 * tab-separated columns are skipped; sample j is column 9 + j, of which the leading GT `a sep b` is read: a, b one of 0 1 . ,
 * sep / or | , followed by : tab \r \n or the line's end.  0?0 -> 00, 1?1 -> 11, 0?1 and 1?0 -> 10, .?. -> 01 (PLINK's
 * codes: A1 = REF, A2 = ALT), order bit = (a == '1'); pad bits of the row's last bytes zero.
 * Everything else is an offence: row_status[r] = {code, sample column (0-based) of the line's first offence in file order},
 * {0, 0} for a clean line (host array, may be NULL): GARLIC_VCF_BAD_BYTE, _HALF_MISSING (./1), _HAPLOID (one allele, no
 * separator), _ALLELE_INDEX (an index >= 2), _FEW_COLUMNS (column = the number of sample columns found), _MANY_COLUMNS
 * (column = nind_total).  The call then returns GARLIC_ERR_INVALID and garlic_hip_last_error names the lowest such row; the
 * clean rows of the call are written and count as set, an offending row's bits are unspecified and it does not.
 * Any line length, field width and nind_total work.  Device memory: the image keeps the staging buffer of its largest host
 * slab (text_bytes + 16), the line offsets and the status words until garlic_bed_destroy, so that a file's slabs reuse them. */
#define GARLIC_VCF_BAD_BYTE 1
#define GARLIC_VCF_HALF_MISSING 2
#define GARLIC_VCF_HAPLOID 3
#define GARLIC_VCF_ALLELE_INDEX 4
#define GARLIC_VCF_FEW_COLUMNS 5
#define GARLIC_VCF_MANY_COLUMNS 6
int garlic_bed_set_rows_vcf(garlic_bed *bed, const char *text, int64_t text_bytes, const int64_t *line_begin,
                            int64_t row_begin, int64_t row_count, int32_t *row_status, int32_t where);

/* Image rows, order rows and the census of rows [row_begin, row_begin + row_count) parsed on the device from TPED text.
 * text, text_bytes, line_begin and where mean what they mean for garlic_bed_set_rows_vcf.  A line is tokens separated by runs
 * of blanks (' ', '\t', '\r'; leading and trailing runs, a '\r' before the '\n' and a last line without '\n' are fine): four
 * leading tokens of any width, which are not read, then 2 * nind_total allele tokens of exactly one byte; any byte value is
 * an allele (compared as unsigned bytes) except the blanks, '\n', and '\v', '\f', NUL, which are offences anywhere in the
 * line.  `missing` is the --tped-missing character (a blank or '\n': GARLIC_ERR_INVALID).  The rule is the reference's
 * (src/garlic-data.cpp:103-141): `one` is the line's first allele that is not `missing`; with A1 := one a genotype becomes
 * 00 (one one), 10 (exactly one allele is one), 11 (neither is), 01 (either allele missing), order bit = (first allele !=
 * one) on a non-missing genotype, 0 on a missing one; pad bits zero.  row_allele[r] (host, may be NULL) is `one`, or `missing`
 * when every allele of the line is missing.  Every letter that is not `one` folds into A2, so such an image cannot tell
 * `C C` from `C G` when one = A: feature counting (--tped-counting) does not read through it.
 * The census travels with the image: the parse writes {nalleles, total} per row -- the alleles equal to `one` and the
 * non-missing alleles, those of half-missing genotypes (`0 G`) included, which no rule could recount from the image -- and
 * garlic_bed_census returns them with counted[r] = 0 (A1 = one), or 2 when every allele is missing (GARLIC_ERR_STATE until
 * every row is set); garlic_panel_set_genotypes_bed and garlic_panel_set_phase_bed use it unchanged.
 * row_status[r] = {code, individual (0-based) of the line's first offence in file order}, {0, 0} for a clean line (host, may
 * be NULL): GARLIC_TPED_LONG_ALLELE (an allele token longer than one byte), _BAD_BYTE ('\v', '\f', NUL; individual 0 inside the
 * leading tokens), _FEW_COLUMNS (fewer than 4 + 2 * nind_total tokens; individual = allele tokens found / 2), _MANY_COLUMNS
 * (more; individual = nind_total).  The call then returns GARLIC_ERR_INVALID and garlic_hip_last_error names the lowest such
 * row; the clean rows of the call are written and count as set, an offending row's bits are unspecified and it does not.
 * The sources do not mix on one image: GARLIC_ERR_STATE for this call on an image that has rows from garlic_bed_set_rows,
 * garlic_bed_set_order_rows, garlic_bed_set_rows_vcf or garlic_bed_extract, and for those calls on an image filled by this
 * one.  garlic_bed_extract stays refused, as on every image with an order plane.  The staging buffers (slab, line offsets,
 * status words, row alleles) are kept with the image and reused across a file's slabs. */
#define GARLIC_TPED_LONG_ALLELE 1
#define GARLIC_TPED_BAD_BYTE 2
#define GARLIC_TPED_FEW_COLUMNS 3
#define GARLIC_TPED_MANY_COLUMNS 4
int garlic_bed_set_rows_tped(garlic_bed *bed, const char *text, int64_t text_bytes, const int64_t *line_begin,
                             int64_t row_begin, int64_t row_count, uint8_t missing,
                             uint8_t *row_allele /* host [row_count], may be NULL */,
                             int32_t *row_status /* host [row_count][2], may be NULL */, int32_t where);
/* Gives a fully set image the census its source computed, in place of the one the image rule would compute: counts[r] =
 * {nalleles, total}, counted[r] = 0 (A1), 1 (A2), 2 (none); host or device arrays.  This is how a TPED image reaches a second
 * device: rows through garlic_bed_set_rows, plane through garlic_bed_set_order_rows, census through this call.
 * GARLIC_ERR_STATE when a row is not set; GARLIC_ERR_INVALID for a counted outside 0..2, negative counts or nalleles > total.
 * Setting rows or order rows afterwards discards the supplied census, exactly as it discards a computed one. */
int garlic_bed_set_census(garlic_bed *bed, const int32_t *counts /* [nrows][2] */, const uint8_t *counted /* [nrows] */,
                          int32_t where);

/* GenoLikeData::data (src/garlic-data.h:91): per-genotype error probabilities, already converted
 * as readTGLSData does (src/garlic-data.cpp:1557-1576); same addressing as genotypes.  Any doubles.
 * A panel holds its likelihoods in one of three forms (garlic_panel_tgls_mode):
 *   GARLIC_TGLS_DICTIONARY    one-byte codes, at most 256 distinct values (--gl-type GQ, PL integers): the host tabulates
 *                             lod() per (SNP, value, genotype) with the host libm.
 *   GARLIC_TGLS_DICTIONARY16  16-bit codes (2 bytes per genotype) and one panel-wide table of at most 65,536 values
 *                             (--gl-type GL / PL as printed numbers: a column of three decimals holds about 10,000).
 *   GARLIC_TGLS_CONTINUOUS    the values themselves, 8 bytes per genotype.
 * In the last two forms lod() (src/garlic-roh.cpp:355-386) runs on the device with glibc's log10 restated operation by
 * operation -- checked against the host's log10 when first needed; should they ever differ, the terms
 * are computed on the host instead.  Same scores in every form: those of the reference on this host.
 * Transitions.  A panel enters DICTIONARY16 through garlic_panel_set_gl_codes16 only: from no likelihoods, or from
 * one-byte codes, which a kernel widens (the code numbers stay).  Once there, garlic_panel_set_gl and
 * garlic_panel_set_gl_codes uploads are coded into the 16-bit table as well, and the panel turns CONTINUOUS (its codes
 * expanded on the device) when the merged table would pass 65,536 values.  A panel that has never seen
 * garlic_panel_set_gl_codes16 behaves as it always has: a garlic_panel_set_gl / garlic_panel_set_gl_codes upload that
 * takes the table past 256 values turns it CONTINUOUS directly.  A continuous panel stays continuous.
 * (Dictionary codes: the terms are expanded into a matrix of 8 bytes per genotype when the device has room for it, whole
 * or -- garlic_panel_set_tgls_term_budget -- slab by slab; with neither the chain looks them up.)
 * When the device cannot hold values and terms side by side the values are converted in place at the
 * first computation; changing genotypes, frequencies, the map or the weighting parameters (M, mu)
 * afterwards then needs the likelihoods uploaded again, over all loci (GARLIC_ERR_STATE says so). */
int garlic_panel_set_gl(garlic_panel *panel, const double *gl, int64_t ld, int64_t locus_begin,
                        int64_t locus_count, int32_t where);

/* The same likelihoods already dictionary-coded, as a reader that converts GQ / PL integers produces
 * them anyway: codes[(l - locus_begin) * ld + i] indexes values[0 .. nvalues), nvalues <= 256, the
 * error probabilities as readTGLSData converts them.  One byte per genotype on the host and over
 * PCIe instead of eight.  Every call may bring its own table; a one-byte panel whose tables add up to more than
 * 256 distinct values keeps the values themselves from then on, a panel of 16-bit codes merges them into its table
 * (see garlic_panel_set_gl). */
int garlic_panel_set_gl_codes(garlic_panel *panel, const uint8_t *codes, int64_t ld, int64_t locus_begin,
                              int64_t locus_count, const double *values, int32_t nvalues, int32_t where);

/* The same with 16-bit codes: codes[(l - locus_begin) * ld + i] indexes values[0 .. nvalues), nvalues <= 65536 (a code
 * past the table counts as code 0).  Addressing and chunking as garlic_panel_set_gl_codes; every call may bring its own
 * table, the tables are merged by bit pattern in first-seen order.  The panel becomes (or stays) GARLIC_TGLS_DICTIONARY16:
 * 2 bytes per genotype on the host, over PCIe and on the device.  The codes are never overwritten -- terms, raw or scaled
 * by (M, mu), are rebuilt from them, so no change of genotypes, frequencies, map or weighting ever asks for the
 * likelihoods again -- and the panel honours garlic_panel_set_tgls_term_budget (below).  When the merged table would pass
 * 65,536 values the panel turns GARLIC_TGLS_CONTINUOUS.  On a continuous panel the call stores the values. */
int garlic_panel_set_gl_codes16(garlic_panel *panel, const uint16_t *codes, int64_t ld, int64_t locus_begin,
                                int64_t locus_count, const double *values, int32_t nvalues, int32_t where);

/* How the panel holds its likelihoods: 0 none yet, GARLIC_TGLS_DICTIONARY, GARLIC_TGLS_CONTINUOUS, GARLIC_TGLS_DICTIONARY16.
 * *terms_by (may be NULL): who computed the current TGLS term matrix -- 0 nothing computed yet (or the terms come slab
 * by slab) or tabulated from the one-byte dictionary, 1 the device (log10 verified against the host), 2 the host. */
#define GARLIC_TGLS_DICTIONARY 1
#define GARLIC_TGLS_CONTINUOUS 2
#define GARLIC_TGLS_DICTIONARY16 3
int garlic_panel_tgls_mode(garlic_panel *panel, int32_t *mode, int32_t *terms_by);

/* A --tgls file's likelihoods, parsed from the text and dictionary-coded on the device (csrc/tgls_kernels.hpp).
 * The object holds nrows rows of n_kept = (col_idx ? n_idx : ncols_total) uint16 codes and ONE dictionary of the RAW values --
 * the doubles as operator>> reads them, before readTGLSData's conversion -- of at most 65,536 entries.  col_idx (host, may be
 * NULL = every column in file order) names the sample columns the object keeps, in the order it keeps them; any order, and an
 * index may repeat.  Code numbers are issued slab by slab: the values a call meets for the first time get the next codes in
 * ascending order of their bit patterns, so the numbers depend on the file and the slab boundaries alone, and a code, once
 * issued, never changes.
 *
 * garlic_tgls_set_rows_text   rows [row_begin, row_begin + row_count) from a slab of text; text, text_bytes, line_begin and
 *     where mean what they mean for garlic_bed_set_rows_vcf (host or device text, no alignment asked for; a line ends at its
 *     '\n', at the next line_begin or at text_bytes).  Of a line, four tokens are skipped; token 4 + j is sample column j.
 *     Tokens are separated as operator>> and countFields separate them: by runs of isspace() bytes, leading and trailing
 *     runs and a '\r' before the '\n' included.  A kept column's token becomes a double only where that is provably what
 *     strtod gives (csrc/tgls_number.hpp: [+-]? (digits [. digits*]? | . digits) ([eE] [+-]? digits)?, at most 32 bytes,
 *     the digits an integer <= 2^53, the decimal exponent within +-22); columns that are not kept are not read.
 *     row_status[r] = {code, sample column of the line's first offence in file order}, {0, 0} for a clean line (host, may be
 *     NULL):
 *       GARLIC_TGLS_DEFERRED       a kept token that gets no value here.  NOT an error: the call returns GARLIC_OK, the row
 *                                  counts as not set (rows_deferred of garlic_tgls_info) until garlic_tgls_set_rows_values
 *                                  brings its doubles as the host parses them.  (A line whose first offence is a deferred
 *                                  token is not looked at further: the host that parses it counts its fields as well.)
 *       GARLIC_TGLS_FEW_COLUMNS    column = the number of sample columns found;
 *       GARLIC_TGLS_MANY_COLUMNS   column = ncols_total.  Either makes the call GARLIC_ERR_INVALID, with the lowest such row
 *                                  in garlic_hip_last_error; the clean rows of the call are written and count as set.
 *     GARLIC_ERR_RANGE: the call met the 65,537th distinct raw value; the file needs the host reader, and every later call
 *     on the object but destroy and info answers GARLIC_ERR_STATE.  (A form of 8 bytes per genotype is deliberately not
 *     built: it needs the conversion's pow on the device, and GQ / GL / PL columns do not print that many values.)
 *     The object keeps its staging buffers (the largest host slab + 16 bytes, 8 bytes per kept genotype of the largest call,
 *     the line offsets and status pairs) until garlic_tgls_destroy, so that a file's slabs reuse them.
 * garlic_tgls_set_rows_vcf    the same rows from the data lines of a VCF (csrc/vcf_gl_kernels.hpp): one scalar FORMAT subfield
 *     per sample.  A line ends at its first '\r' or '\n' (or as above).  Eight tab-separated columns are skipped; column 8
 *     is FORMAT, keys joined by ':', and k is the index of the first of them that equals `key` bytewise -- per line, FORMAT
 *     may change.  key: 1 to 16 bytes of [A-Za-z0-9_.], not "GT" (GARLIC_ERR_INVALID).  Sample j is column 9 + j; its value
 *     is the bytes between the column's k-th ':' and the next ':' or the column's end, and goes through the same number
 *     grammar with the same limits.  The value is MISSING when the column has fewer than k colons (trailing subfields may be
 *     dropped), when the subfield is empty and when it is exactly ".".  A missing value of a column that starts with '.' (a
 *     missing genotype, whose score never reads the value) becomes *missing_raw, or 0.0 when missing_raw is NULL; on any
 *     other column it becomes *missing_raw, or is an offence when missing_raw is NULL.  Columns that are not kept are counted
 *     and nothing else.  Status codes: _DEFERRED, _FEW_COLUMNS and _MANY_COLUMNS as above (a list such as 0,12,40, nan, a
 *     token of more than 32 bytes and an integer above 2^53 are deferred), and
 *       GARLIC_TGLS_VCF_NO_KEY     FORMAT does not name the key; column = 0;
 *       GARLIC_TGLS_VCF_NO_VALUE   a called genotype without a value and no missing_raw; column = the sample column.
 *     Either makes the call GARLIC_ERR_INVALID as the column counts do.  Behind the parse the call is set_rows_text's --
 *     staging, encode, dictionary, GARLIC_ERR_RANGE -- and the rows of one object may come from either call.
 * garlic_tgls_set_rows_values the same rows from raw doubles raw[(r - row_begin) * ld + k], k < n_kept in the object's own
 *     column order, ld >= n_kept, host or device.
 * garlic_tgls_get_rows        out[(r - row_begin) * ld + k] (host or device) = the row's values: GARLIC_TGLS_RAW as parsed, or
 *     GARLIC_GL_GQ / _GL / _PL converted as readTGLSData converts them (src/garlic-data.cpp:1557-1576, host libm, applied
 *     to the dictionary).  GARLIC_ERR_STATE when a row of the range is not set.
 * garlic_tgls_info            the dictionary's size and the numbers of set and of deferred rows (any pointer may be NULL).
 * garlic_tgls_count_values    *n_values = the number of distinct values, raw or converted as for get_rows, among the rows of the
 *     range: what decides the form a host reader would have given them (256 / 65,536).  Only a 64 KB flag array leaves the device.
 * garlic_tgls_get_values      values[c] (host, n <= n_raw_values entries) = the value of code c, raw or converted as for get_rows:
 *     the dictionary in the order its codes were issued.
 * garlic_panel_set_gl_tgls    the panel's likelihoods from the object, device to device: row r goes to locus dest_locus[r]
 *     (host, nrows entries, -1 = dropped, the others strictly ascending), individual i of the panel is kept column
 *     ind_offset + i.  The dictionary is converted on the host (at most 65,536 values) and the codes go through the panel's
 *     own doors: a panel without 16-bit codes that faces at most 256 distinct CONVERTED values takes them narrowed to one
 *     byte through garlic_panel_set_gl_codes, every other one through garlic_panel_set_gl_codes16 -- the panel a host
 *     reader's codes would have filled.  GARLIC_ERR_STATE while a row of the object is unset or deferred. */
#define GARLIC_TGLS_OK 0
#define GARLIC_TGLS_DEFERRED 1
#define GARLIC_TGLS_FEW_COLUMNS 2
#define GARLIC_TGLS_MANY_COLUMNS 3
#define GARLIC_TGLS_VCF_NO_KEY 4
#define GARLIC_TGLS_VCF_NO_VALUE 5
#define GARLIC_TGLS_RAW (-1) /* gl_type of garlic_tgls_get_rows: no conversion (GARLIC_GL_GQ is 0) */
typedef struct garlic_tgls garlic_tgls;
int garlic_tgls_create(garlic_ctx *ctx, int64_t nrows, int32_t ncols_total, const int32_t *col_idx /* NULL = all */,
                       int32_t n_idx, garlic_tgls **out);
int garlic_tgls_set_rows_text(garlic_tgls *tgls, const char *text, int64_t text_bytes, const int64_t *line_begin /* row_count + 1 */,
                              int64_t row_begin, int64_t row_count, int32_t *row_status /* [row_count][2], may be NULL */,
                              int32_t where);
int garlic_tgls_set_rows_vcf(garlic_tgls *tgls, const char *text, int64_t text_bytes, const int64_t *line_begin /* row_count + 1 */,
                             int64_t row_begin, int64_t row_count, const char *key, const double *missing_raw /* NULL: refuse */,
                             int32_t *row_status /* [row_count][2], may be NULL */, int32_t where);
int garlic_tgls_set_rows_values(garlic_tgls *tgls, const double *raw, int64_t ld, int64_t row_begin, int64_t row_count,
                                int32_t where);
int garlic_tgls_get_rows(garlic_tgls *tgls, int32_t gl_type, int64_t row_begin, int64_t row_count, double *out, int64_t ld,
                         int32_t where);
int garlic_tgls_info(garlic_tgls *tgls, int32_t *n_raw_values, int64_t *rows_set, int64_t *rows_deferred);
int garlic_tgls_count_values(garlic_tgls *tgls, int32_t gl_type, int64_t row_begin, int64_t row_count, int32_t *n_values);
int garlic_tgls_get_values(garlic_tgls *tgls, int32_t gl_type, double *values, int32_t n);
int garlic_panel_set_gl_tgls(garlic_panel *panel, garlic_tgls *tgls, int32_t gl_type, int64_t ind_offset,
                             const int64_t *dest_locus /* [nrows], -1 = dropped */);
int garlic_tgls_destroy(garlic_tgls *tgls);

/* Unweighted scores from dictionary-coded likelihoods run in two passes: the codes are expanded once into the TGLS term
 * matrix (8 bytes per genotype, 64-individual blocks of rows x 64 doubles, rows = 32 + nloci + 4160), which the chain then
 * streams; the weighted kernels read the same matrix scaled by the decay factors of (M, mu).  By default the panel keeps the
 * whole matrix, and when the device cannot hold it the kernels look every term up themselves (several times slower; feed,
 * coverage and segment calls then also lose their fused forms and need a full-size score scratch).  This sets an upper
 * bound in bytes for the term buffers instead:
 *   0 (default): the whole matrix, or none and the look-up kernels.
 *   > 0: the term buffers of this panel never hold more than `bytes`; when the whole matrix is larger, every use_gl call
 *        -- unweighted: garlic_lod_windows / _multi, garlic_lod_feed / _subset, garlic_roh_coverage_fused,
 *        garlic_roh_segments; weighted: garlic_wlod_windows (to host and device, the whole panel or a range of individuals),
 *        garlic_lod_feed / _subset (GARLIC_FEED_SAMPLED_WLOD at step >= winsize, from full scores below),
 *        garlic_roh_coverage_fused, garlic_roh_segments -- builds and consumes it slab by slab (a slab = consecutive
 *        64-individual blocks; the terms of one slab are built while the kernels read the other, so two buffers, shared by
 *        raw and scaled slabs: slab_blocks is the largest s for which s + min(s, nblk - s) blocks fit in `bytes`,
 *        nblk = ceil(nind / 64) -- the first buffer holds a full slab, the second what the second slab holds).  Same
 *        kernels and forms as budget 0 picks, same doubles, bits and segments; garlic_lod_feed_info answers the same.  A
 *        slab begins at the next block the call scores, so n_slabs = ceil(blocks / slab_blocks) for a range of
 *        individuals; a subset feed's skipped blocks are not scored, a slab of nothing else is not built.  The weighted
 *        kernels group blocks per workgroup (two, four or eight): the grouping restarts at every slab's first block.
 *  -1: the whole matrix when the default's test lets it in, otherwise slabs in half of the memory free at the call.
 * GARLIC_ERR_INVALID when `bytes` > 0 cannot hold the buffers of one-block slabs (2 x rows x 512 bytes; a panel of at
 * most 64 individuals has one slab and one buffer).
 * Slabs are rebuilt by every call, so a sweep over several window sizes pays the term pass per size where the whole matrix
 * is built once and reused: a caller with room for it keeps budget 0.  May be changed between calls in both directions;
 * what the new bound does not allow -- a whole matrix, raw or scaled, from before -- is freed at once or by the next
 * use_gl call.  Panels that hold continuous likelihoods keep 8 bytes per genotype as their data and ignore the budget.
 * Panels of 16-bit codes (GARLIC_TGLS_DICTIONARY16) honour it as one-byte panels do -- whole matrix, slabs or -1, the same
 * calls slab by slab with the same doubles, bits and segments -- with one difference: they have no look-up kernels (a per-SNP
 * table of 65,536 x 4 terms is out of the question).  Where a one-byte panel would look its terms up they instead: under
 * budget 0 without room for the whole matrix, go on as under -1; for the shapes listed next as not covered by slabs (and the
 * unweighted counterparts: an ind_begin that is no multiple of 64, GARLIC_TGLS_NO_RING, a window that sums to exactly
 * -9999.0), use the whole matrix where the budget admits it and otherwise return GARLIC_ERR_NOMEM with a message that says so.
 * Their chain kind (garlic_panel_chain_kind) is decided before any term exists, from log10 of the smallest table value
 * minus 1e-6 as the most negative term: 0 only when W times that bound stays above -9990.
 * Weighted shapes that are not covered by slabs: a slab launch starts at a block of the matrix, so a weighted call whose
 * ind_begin is not a multiple of 64 (the ring, strip, stream and tile forms alike), and every weighted call that keeps
 * the generic kernel (GARLIC_WLOD_GENERIC, GARLIC_WLOD_SMALL_GENERIC below 16, winsize + 64 > 4160) looks its terms up
 * in the code table under a budget (n_slabs 0); nothing is built past the bound.  The generic kernel takes windows up to
 * 250 SNPs: a wider weighted call of such a shape is refused (GARLIC_ERR_INVALID) where budget 0 would have read the
 * whole scaled matrix.  garlic_lod_feed_multi_tgls is unweighted. */
int garlic_panel_set_tgls_term_budget(garlic_panel *panel, int64_t bytes);
/* whole_bytes: what the full matrix needs (rows x 8 x the panel's padded individual count, (nind + 126) / 64 * 64); resident_bytes: term buffers held now;
 * slab_blocks / n_slabs: of the last use_gl call, weighted or not (n_slabs 0: it read a whole matrix or looked terms up).
 * Any pointer may be NULL. */
int garlic_panel_tgls_terms_info(garlic_panel *panel, int64_t *whole_bytes, int64_t *resident_bytes,
                                 int32_t *slab_blocks, int32_t *n_slabs);

/* HapData::firstCopy (src/garlic-data.h:36; filled by readTPED under --phased,
 * src/garlic-data.cpp:106,129: "the first allele of the pair is the counted allele"), one byte per
 * genotype, non-zero = true; same addressing as genotypes.  Only the phased LD weights read it. */
int garlic_panel_set_phase(garlic_panel *panel, const uint8_t *first_copy, int64_t ld,
                           int64_t locus_begin, int64_t locus_count, int32_t where);

/* The same phase at one bit per genotype, as the genotype cache stores HapData::firstCopy: rows are SNP-major, row r
 * (locus locus_begin + r) starts at rows + r * row_bytes, and bit (i & 7) of its byte (i >> 3) is individual i of the
 * panel; row_bytes >= (nind + 7) / 8, bits past the last individual are ignored.  Rows need no alignment.  Same effect on
 * the panel as garlic_panel_set_phase over the same loci, at an eighth of the bytes. */
int garlic_panel_set_phase_bits(garlic_panel *panel, const uint8_t *rows, int64_t row_bytes, int64_t locus_begin,
                                int64_t locus_count, int32_t where);

/* The same phase from an image with an order plane, device to device: HapData::firstCopy of the TPED line a row stands for,
 *     firstCopy = non-missing && (order bit == (counted == A2)),   all ones on a row whose counted allele is none
 * (alleleStr1 == oneAllele at src/garlic-data.cpp:129 when both are the missing character).  ind_offset (any integer in
 * range) and dest_locus mean what they mean for garlic_panel_set_genotypes_bed; runs the census first when it has not been
 * run.  Same effect on the panel as garlic_panel_set_phase_bits over the same loci.  GARLIC_ERR_STATE: the image has no
 * plane. */
int garlic_panel_set_phase_bed(garlic_panel *panel, garlic_bed *bed, int64_t ind_offset, const int64_t *dest_locus /* [nrows] */);

/* LDData::LD (src/garlic-data.h:105) for winsize: ld[l * winsize + k], l global locus. */
int garlic_panel_set_ld(garlic_panel *panel, int32_t winsize, const double *ld, int32_t where);

/* calcLDData (src/garlic-data.cpp:330-375): the LD weights of wLOD, computed on the device from the
 * panel's genotypes,
 *     LD[s][k] = sum_{i = s .. s+winsize-1, in order} (i == s+k ? 1 : c(i, s+k))   for s <= nloci_c - winsize
 * with  phased == 0:  c = hr2 (calcHR2LD :377-527, hr2 :558-583), from homFreq (:656-676) taken over
 *                     every individual of the panel;
 *       phased != 0:  c = r2  (calcR2LD :426-535, r2 :585-617; --phased), from the allele
 *                     frequencies of garlic_panel_set_freq and the phase of garlic_panel_set_phase.
 * The pair counts run over the individuals sub_idx[0 .. n_sub); sub_idx == NULL: all of them; a
 * non-NULL sub_idx with n_sub = 0: none (what a shard that holds no member of a panel-wide subsample
 * passes to garlic_ld_counts: its pair counts are zero, its locus counts still cover everyone).  The
 * reference draws that subsample with a time-seeded RNG (:346-364, --ld-subsample); here the caller
 * supplies it.  The result is installed as the panel's LD weights for winsize (as garlic_panel_set_ld would)
 * and, if ld_out is not NULL, also written there (nloci * winsize doubles, ld[l * winsize + k]). */
int garlic_panel_compute_ld(garlic_panel *panel, int32_t winsize, int32_t phased, const int32_t *sub_idx,
                            int32_t n_sub, double *ld_out, int32_t where);

/* The same in two steps for panels whose individuals are sharded over GPUs: everything that
 * depends on genotypes is an integer count, exact and order-free --
 *     locus_counts[l][2]            = {homozygous, non-missing} individuals of this shard
 *     pair_counts[l][winsize][2]    = over the shard's part of the subsample, for SNP pairs (l, l+d), d >= 1:
 *                                     {both non-missing, both non-missing and homozygous}   (hr2), or
 *                                     {2 * both non-missing, x11 of r2 :592-606}            (phased)
 * -- so the caller sums the count arrays of all shards element-wise (one all-reduce) and every
 * shard finishes with the summed counts; the floating-point part then runs in the reference's
 * operation order and is identical on every GPU.  sub_idx is shard-local.  (Phased: the allele
 * frequencies are the caller's, over all individuals, as for the LOD scores.) */
int garlic_ld_counts(garlic_panel *panel, int32_t winsize, int32_t phased, const int32_t *sub_idx,
                     int32_t n_sub, int32_t *locus_counts, int32_t *pair_counts, int32_t where);
int garlic_ld_finish(garlic_panel *panel, int32_t winsize, int32_t phased, const int32_t *locus_counts,
                     const int32_t *pair_counts, double *ld_out, int32_t where);

/* The LD weights of SEVERAL window sizes (a --weighted sweep over window sizes).  ld_out may be NULL and so may any of
 * its entries; ld_out[i] receives nloci * winsizes[i] doubles, exactly what garlic_panel_compute_ld(winsizes[i]) writes.
 * The call installs the weights of EVERY listed size: the panel keeps a set of weights per window size, and
 * garlic_wlod_windows, the weighted garlic_lod_feed / _subset, garlic_roh_coverage_fused and garlic_roh_segments use the
 * set of their winsize (GARLIC_ERR_STATE when it is not installed).  Sizes may come in any order and may repeat; a
 * repeated size has one set.  garlic_panel_set_ld, garlic_panel_compute_ld and garlic_ld_finish still leave the panel
 * with exactly the one set they install; garlic_panel_release_scratch keeps every installed set.  Per size a set is
 * (16 + (nloci + W + 64) * W) * 8 bytes; when the sets do not fit the call returns GARLIC_ERR_NOMEM and no LD weights
 * stay installed.
 *
 * The pair value c(i, j) does not depend on the window size, so LD_W'[s][k] is LD_W[s][k]'s accumulator after its first
 * W' terms (W' < W, k < W'): one ordered-sum pass at the largest size of a group yields every size of the group as
 * snapshots of the running sums -- same operands, same order, same roundings.  Grouping rule, on the distinct sizes:
 *   - a size SHARES when it takes the SNP-per-thread sum kernel (32 < W <= 512, no sum-form switch set) and
 *     GARLIC_LD_MULTI_SOLO is not set to a non-zero value; if fewer than two sizes share, none does
 *   - the sharing sizes, ascending, are cut greedily into groups: a size joins the current group unless the group has
 *     4 sizes already or 8 * max(R + (n - 1) * 9 * T, 17 * T) > 131072, where n is the group's size count with it,
 *     T = W + 16 rounded up to a multiple of 64 and R = 2048 * ceil(T / 128) + 130 (the launch's LDS in bytes)
 *   - the sharing sizes cost ONE pair stage, at the largest of them (its table serves every group; the stage is the one
 *     garlic_panel_compute_ld / garlic_ld_counts + garlic_ld_finish would pick for that width, hr2 or r2), and one sum
 *     pass per group
 *   - every other size goes through the single-size path unchanged: one pair stage and one sum pass each
 * garlic_ld_finish_multi is the sharded form: pair_counts are those of garlic_ld_counts at max(winsizes), summed over
 * the shards ([nloci][max(winsizes)][2]); the counts of narrower sizes are its first columns.
 * garlic_panel_ld_info lists the installed sizes ascending (up to cap of them; n_installed counts all), for each the
 * index of its group in the last multi call -- the shared groups in ascending order first, then the sizes on their own,
 * ascending; -1: not installed by a multi call -- the bytes the sets hold, and the pair stages and sum passes the last
 * multi call ran (0 after a single-size call).  Any output may be NULL. */
int garlic_panel_compute_ld_multi(garlic_panel *panel, const int32_t *winsizes, int32_t n_sizes, int32_t phased,
                                  const int32_t *sub_idx, int32_t n_sub, double *const *ld_out, int32_t where);
int garlic_ld_finish_multi(garlic_panel *panel, const int32_t *winsizes, int32_t n_sizes, int32_t phased,
                           const int32_t *locus_counts, const int32_t *pair_counts /* of garlic_ld_counts at max(winsizes) */,
                           double *const *ld_out, int32_t where);
int garlic_panel_ld_info(garlic_panel *panel, int32_t cap, int32_t *winsizes, int32_t *groups, int32_t *n_installed,
                         int64_t *weight_bytes, int32_t *n_pair_passes, int32_t *n_sum_passes);

/* Which kernels the last LD call on the panel took (garlic_panel_compute_ld, garlic_ld_counts, garlic_ld_finish and the
 * multi-size calls; for a multi call with sizes that share passes: the pair stage at the widest sharing size).  fused: the
 * pair kernel wrote the hr2 / r2 table itself and no pair-count table was made (garlic_panel_compute_ld{,_multi} only;
 * never under GARLIC_LD_UNFUSED, never for garlic_ld_counts / garlic_ld_finish).  Pair kernels: _MFMA, banded Gram matrices
 * on the matrix cores (16 < winsize <= 129; phased as well as unphased); _LANE / _TILED / _FLAT / _PLAIN: AND + popcount
 * forms.  Any pointer may be NULL; GARLIC_ERR_STATE before the panel's first LD call. */
#define GARLIC_LD_PAIR_PLAIN 0
#define GARLIC_LD_PAIR_MFMA 1
#define GARLIC_LD_PAIR_LANE 2
#define GARLIC_LD_PAIR_TILED 3
#define GARLIC_LD_PAIR_FLAT 4
#define GARLIC_LD_SUM_PLAIN 0
#define GARLIC_LD_SUM_FLAT 1
#define GARLIC_LD_SUM_COL 2
#define GARLIC_LD_SUM_TILED 3
int garlic_panel_ld_form_info(garlic_panel *panel, int32_t *pair_kernel, int32_t *sum_kernel, int32_t *fused, int32_t *phased);

/* A panel keeps its device scratch between calls (LD counting and summing buffers: about
 * 5 x nloci x winsize x 8 bytes; the score scratch of host-output and feed calls), because at scale
 * allocating it costs more than the kernels.  This frees it; inputs, tables, the installed LD weights
 * and the TGLS term matrix stay, and the next call allocates again what it needs. */
int garlic_panel_release_scratch(garlic_panel *panel);

/* Output addressing for this panel: pitch_align = 1 gives the reference's dense rows
 * (chr_pitch[c] = chr_nloci[c], chromosome blocks back to back).  A larger value rounds every row
 * pitch and chromosome base up to that many doubles AND reserves rows up to the next multiple of
 * 64 individuals per chromosome block (32 = 256-byte aligned rows: the layout the tuned kernel
 * needs; with pitch_align = 1 a slower generic kernel path runs).  Pad rows / pad columns are
 * never read back and hold unspecified values.  total = number of doubles the caller's buffer
 * must have for nind_out individuals. */
int garlic_lod_out_layout(garlic_panel *panel, int32_t pitch_align, int32_t nind_out,
                          int64_t *chr_base, int64_t *chr_pitch, int64_t *total);

/* calcLODWindows (src/garlic-roh.cpp:279): unweighted window LOD scores of individuals
 * [ind_begin, ind_begin + ind_count) for one window size.  use_gl != 0 takes the per-genotype
 * error from the panel's GL data (USE_GL, src/garlic-roh.cpp:68) instead of `error`.
 * out has garlic_lod_out_layout(pitch_align, ind_count) doubles. */
int garlic_lod_windows(garlic_panel *panel, int32_t winsize, double error, int32_t max_gap,
                       int32_t use_gl, int32_t ind_begin, int32_t ind_count, int32_t pitch_align,
                       double *out, int32_t where);

/* The same for several window sizes (--winsize-multi; exploreWinsizes, src/garlic-roh.cpp:726-751):
 * the scores of winsizes[k] go to out + k * out_stride (out_stride >= the layout's total).  The
 * panel stays resident, the kernels run one window size after the other. */
int garlic_lod_windows_multi(garlic_panel *panel, const int32_t *winsizes, int32_t n_winsizes, double error,
                             int32_t max_gap, int32_t use_gl, int32_t ind_begin, int32_t ind_count,
                             int32_t pitch_align, double *out, int64_t out_stride, int32_t where);

/* calcwLODWindows (src/garlic-roh.cpp:311): gap-weighted wLOD; needs gpos and LD for winsize
 * (garlic_panel_set_ld or garlic_panel_compute_ld).  winsize up to 4096 (above that:
 * GARLIC_ERR_INVALID; the reference has no limit but no use for such windows either). */
int garlic_wlod_windows(garlic_panel *panel, int32_t winsize, double error, int32_t max_gap,
                        int32_t use_gl, int32_t M, double mu, int32_t ind_begin, int32_t ind_count,
                        int32_t pitch_align, double *out, int32_t where);

/* convertWinData2DoubleData (src/garlic-data.cpp:2026-2069) on the device: the KDE feed.  Reads
 * scores laid out as garlic_lod_out_layout(pitch_align, nind_out) describes (device memory) and
 * writes, in the reference's order chromosome -> individual -> locus, every `step`-th window
 * (locus 0, step, 2*step, ...) that is neither MISSING nor NaN.  feed (device) must hold
 * feed_capacity doubles; *count (host) receives the number written (or needed, if larger than the
 * capacity -- nothing is written then).  The explore / auto-winsize flows keep only these values
 * (step = winsize), 8/winsize bytes per window instead of 8. */
int garlic_lod_flatten(garlic_panel *panel, const double *scores, int32_t pitch_align, int32_t nind_out,
                       int32_t step, double *feed, int64_t feed_capacity, int64_t *count);

/* The explore / auto-winsize flows (src/garlic-roh.cpp:726-751, 798-837, 881-920) compute the
 * scores of a window size only to thin them into the KDE feed and throw them away.  This is both
 * steps in one call with the scores kept on the device: garlic_lod_windows or garlic_wlod_windows
 * (weighted != 0; needs LD for winsize) over every individual of the panel, then
 * convertWinData2DoubleData with `step` (garlic_lod_flatten).  feed: HOST buffer of feed_capacity
 * doubles; *count = values produced (nothing is copied if it exceeds the capacity: an upper bound is
 * sum_c ceil(nloci_c / step) * nind); chr_counts (may be NULL): values per chromosome, so that
 * feeds of individual shards can be merged in the reference's chromosome -> individual order.
 * 8 / step bytes per window cross PCIe instead of 8.  Unweighted --error scores with step >= 4 are
 * thinned by the LOD kernel itself (only the sampled windows are ever stored: 8 / step bytes per
 * window of HBM writes, no full-size scratch).  Weighted scores (with or without per-genotype
 * likelihoods) with step >= winsize, the reference's thinning: every wLOD window is a sum of its
 * own, so only the sampled windows are computed at all, into the same thinned matrix (winsize
 * times less arithmetic, no full-size scratch; GARLIC_WLOD_FEED_FULL=1 in the environment keeps the
 * full scores).  Unweighted scores from per-genotype likelihoods with step >= 4: the ring chain still
 * computes every window (a rolling sum) but stores only the sampled ones (algorithmically 8 + 8 / step
 * bytes per window against 16.25; the samples leave as 8-byte words, one per row, and the thinned
 * matrix is filled with -9999.0 first, so the bytes really written are more) and no full-size scratch; it keeps the full scores when a window could sum to
 * exactly -9999.0 (garlic_panel_chain_kind 1 or 2), when the term matrix was declined or
 * GARLIC_TGLS_NO_RING=1 is set, and under GARLIC_TGLS_FEED_FULL=1.  The other variants (steps below 4,
 * weighted with step < winsize) compute the full scores into device scratch and sample them there.
 * Same values either way; garlic_lod_feed_info tells which it was. */
int garlic_lod_feed(garlic_panel *panel, int32_t winsize, double error, int32_t max_gap, int32_t use_gl,
                    int32_t weighted, int32_t M, double mu, int32_t step, double *feed,
                    int64_t feed_capacity, int64_t *count, int64_t *chr_counts);

/* convertSubsetWinData2DoubleData (src/garlic-data.cpp:2071-2150; selectLODCutoff, src/garlic-roh.cpp:
 * 674-675, --kde-subsample): garlic_lod_feed for the individuals ind_idx[0 .. n_idx) only, in that
 * order inside every chromosome (chromosome -> ind_idx[0] .. ind_idx[n_idx-1] -> locus).  The reference
 * draws them with a time-seeded gsl_ran_choose, which keeps the TFAM order; here the caller supplies
 * them (distinct, each in [0, nind)).  Only the 64-individual blocks that hold a listed individual
 * are scored.  ind_idx == NULL: everyone (= garlic_lod_feed).  chr_counts as there. */
int garlic_lod_feed_subset(garlic_panel *panel, int32_t winsize, double error, int32_t max_gap, int32_t use_gl,
                           int32_t weighted, int32_t M, double mu, int32_t step, const int32_t *ind_idx,
                           int32_t n_idx, double *feed, int64_t feed_capacity, int64_t *count, int64_t *chr_counts);

/* How the last garlic_lod_feed / _subset / _multi call on this panel produced its feed:
 * GARLIC_FEED_FROM_SCORES (full scores in device scratch, then garlic_lod_flatten),
 * GARLIC_FEED_CHAIN (unweighted: the chain stores only the samples),
 * GARLIC_FEED_SAMPLED_WLOD (weighted: only the sampled windows are computed),
 * GARLIC_FEED_TGLS_CHAIN (unweighted per-genotype likelihoods: the ring chain stores only the samples).
 * *score_doubles (may be NULL): doubles of score scratch that call needed (a _multi call whose chains write
 * straight into the feeds: 0). */
#define GARLIC_FEED_FROM_SCORES 0
#define GARLIC_FEED_CHAIN 1
#define GARLIC_FEED_SAMPLED_WLOD 2
#define GARLIC_FEED_TGLS_CHAIN 3
int garlic_lod_feed_info(garlic_panel *panel, int32_t *form, int64_t *score_doubles);

/* The callers that sweep window sizes -- exploreWinsizes (src/garlic-roh.cpp:726-751), selectWinsize (:798-837),
 * selectWinsizeFromList (:881-920: --winsize-multi with --auto-winsize) -- run calcLODWindows + the KDE thinning once
 * per size on the same data.  This is garlic_lod_feed_subset for n_sizes window sizes in one call (unweighted --error
 * scores; steps[i] is the thinning step of winsizes[i], the reference uses the window size).  Every size gets a
 * stream and device scratch of its own and all of them are enqueued before the first feed is fetched: the tail of one
 * size's chain kernel (its longest runs, a few waves per CU) runs beside the bulk of the next size's, and a feed crosses
 * PCIe while the following sizes are computed.  feeds[i]: HOST buffer of feed_capacity[i] doubles; counts[i] as
 * *count there; chr_counts (may be NULL): [n_sizes][nchr].  ind_idx / n_idx as in garlic_lod_feed_subset (NULL:
 * everyone).  Values identical to n_sizes single calls. */
int garlic_lod_feed_multi(garlic_panel *panel, const int32_t *winsizes, const int32_t *steps, int32_t n_sizes, double error,
                          int32_t max_gap, const int32_t *ind_idx, int32_t n_idx, double *const *feeds,
                          const int64_t *feed_capacity, int64_t *counts, int64_t *chr_counts);

/* garlic_lod_feed_multi for per-genotype likelihoods: the sweeps above run with USE_GL (--tgls) exactly as with --error.
 * The results are those of n_sizes garlic_lod_feed_subset(use_gl = 1, weighted = 0) calls -- values, counts,
 * per-chromosome counts and order (chromosome -> ind_idx order -> locus) identical; duplicate sizes with different
 * steps are allowed.  One pass over the term matrix serves several sizes (csrc/tgls_feed_multi_kernel.hpp):
 *
 * Grouping rule.  A size "takes the ring" when a single call would answer GARLIC_FEED_TGLS_CHAIN for it: step >= 4, no
 * window sum of exactly -9999.0 possible, a term matrix (whole, or slabs under garlic_panel_set_tgls_term_budget) that
 * was neither declined nor looked up, neither GARLIC_TGLS_NO_RING nor GARLIC_TGLS_FEED_FULL set.  The sizes that take
 * the ring and are <= 144 (the one-stream ring's widest window) are sorted ascending (ties: call order) and cut greedily
 * into groups of at most 4 (TGM_MAX_SIZES): group 0 holds the 4 smallest, group 1 the next 4, ..  Every other size is a
 * group of one, numbered after those in ascending order again: a size above 144 that takes the ring runs through the
 * single-size ring chain in the same call (and over the same slabs), a size that does not take the ring goes through
 * the single-size path (full scores, then garlic_lod_flatten's passes) after the groups.  GARLIC_TGLS_FEED_MULTI_SOLO=1:
 * groups of one throughout.
 *
 * Whole term matrix: one chain launch per group.  Under a term budget every slab is built ONCE per call and every group
 * chains over it before its buffer is rebuilt (a single call per size builds every slab per size);
 * garlic_panel_tgls_terms_info reports the call's slab_blocks and n_slabs as for a single call.  Each size has a thinned
 * matrix, a stream and a feed buffer of its own; every size's kernels are enqueued before the first feed is fetched.
 * Arguments as in garlic_lod_feed_multi. */
int garlic_lod_feed_multi_tgls(garlic_panel *panel, const int32_t *winsizes, const int32_t *steps, int32_t n_sizes,
                               int32_t max_gap, const int32_t *ind_idx, int32_t n_idx, double *const *feeds,
                               const int64_t *feed_capacity, int64_t *counts, int64_t *chr_counts);

/* What the last garlic_lod_feed_multi_tgls call on this panel did, for its first n sizes (n <= that call's n_sizes;
 * every pointer may be NULL).  forms[i]: GARLIC_FEED_TGLS_CHAIN_SHARED when size i's group held at least two sizes,
 * GARLIC_FEED_TGLS_CHAIN for a ring chain of its own, else what the single-size path reported (GARLIC_FEED_FROM_SCORES).
 * groups[i]: size i's group index under the rule above.  *n_chain_launches: chain kernels enqueued (groups x slabs; a
 * size on the single-size path counts one).  *n_term_builds: term slabs built (0 with the whole matrix) -- the slabs of
 * the call, not slabs x sizes; a size on the single-size path adds its own.  garlic_lod_feed_info keeps reporting the
 * last size processed. */
#define GARLIC_FEED_TGLS_CHAIN_SHARED 4
int garlic_lod_feed_multi_info(garlic_panel *panel, int32_t n, int32_t *forms, int32_t *groups, int32_t *n_chain_launches,
                               int32_t *n_term_builds);

/* The feed in ascending order.  The consumer of every feed above is computeKDE (src/garlic-kde.cpp:14), and its first
 * step is nrd0 (:43, :130-139), whose first statement is gsl_sort(x, 1, N) (:132) -- in place, on the feed: gsl_stats_sd,
 * the two gsl_stats_quantile_from_sorted_data calls, gsl_stats_minmax and figtree (:81) all read the sorted array.  A
 * single-threaded heapsort on the host, once per window size of every sweep; here an FP64 radix sort on the device
 * between the flatten and the copy-out (csrc/feed_sort_kernel.hpp).
 *
 * Key order: k(x) = bits(x) ^ (bits(x) >> 63 ? 0xFFFFFFFFFFFFFFFF : 0x8000000000000000), compared as unsigned.  That is
 * numeric ascending order for everything that is not NaN; -0.0 sorts in front of +0.0, NaNs with the sign bit set sort
 * first and the other NaNs last, so the order is total.
 * Why the result is the one gsl_sort leaves: a feed holds no NaN (the flatten drops them) and no -0.0 (every window sum
 * starts from 0.0 + ..., and under round-to-nearest a + b or a - b is -0.0 only when both operands already carry that
 * sign), so equal values are equal bit patterns and the ascending arrangement of the values is unique -- what any correct
 * comparison sort leaves in the array, bit for bit.
 *
 * garlic_panel_set_feed_order: GARLIC_FEED_ORDER_SORTED makes garlic_lod_feed, _subset, _multi and _multi_tgls sort the
 * values on the device after the flatten's write pass and before the copy to the host (the multi calls: on the size's own
 * stream; which passes run is decided on the device, so nothing is waited for per pass).  *count, chr_counts, the
 * behaviour when the capacity is exceeded (nothing written), garlic_lod_feed_info, garlic_lod_feed_multi_info and the
 * kernel forms chosen are those of the reference order.  Any other value: GARLIC_ERR_INVALID.  garlic_lod_flatten (a
 * device feed buffer of the caller's) stays in reference order; its caller uses garlic_feed_sort.
 * garlic_feed_sort: n doubles sorted in place under the key order above; `where` GARLIC_DEVICE or GARLIC_HOST (upload,
 * sort, download).  n = 0: nothing happens; n < 0, or a NULL pointer with n > 0: GARLIC_ERR_INVALID.  Scratch: n doubles
 * (a host buffer: 2 n) plus 2 KB per FS_TILE keys, kept with the context -- with the panel or the size's slot for feed
 * calls -- until garlic_panel_release_scratch; when it does not fit, GARLIC_ERR_NOMEM and the caller's data untouched.
 * garlic_feed_sort_info: the last sort on the context, the one inside a feed call included (a multi call: the size
 * fetched last).  A pass whose digit is the same in every key moves nothing and is skipped: passes_run + passes_skipped
 * == 8 after any sort of n > 1 keys.  scratch_bytes: what that sorter holds.  Any pointer may be NULL. */
#define GARLIC_FEED_ORDER_REFERENCE 0   /* chromosome -> individual -> locus (default) */
#define GARLIC_FEED_ORDER_SORTED    1   /* ascending: the array nrd0's gsl_sort leaves (garlic-kde.cpp:132) */
int garlic_panel_set_feed_order(garlic_panel *panel, int32_t order);
int garlic_feed_sort(garlic_ctx *ctx, double *values, int64_t n, int32_t where);
int garlic_feed_sort_info(garlic_ctx *ctx, int32_t *passes_run, int32_t *passes_skipped, int64_t *scratch_bytes);

/* computeKDE (src/garlic-kde.cpp:14-140) on the device: nrd0's bandwidth, the 512 targets, the Gaussian sums and their
 * normalisation, from a feed in ascending order (garlic_feed_sort, GARLIC_FEED_ORDER_SORTED) that never has to leave the
 * device (csrc/kde_kernels.hpp; the host arithmetic: host/kde_select.hpp).
 *     sd  = sqrt(sum (x_i - mean)^2 / (n - 1))                       (its mathematical value: two tree-summed passes, not
 *                                                                     gsl_stats_sd's long-double recurrence bit for bit)
 *     q(f) = (1 - d) x[k] + d x[k + 1],  k = (int)(f (n - 1)), d = f (n - 1) - k      (gsl_stats_quantile_from_sorted_data)
 *     h   = 0.9 * min(sd, (q(0.75) - q(0.25)) / 1.34) * pow(n, -0.2)
 *     x[i] = (double(i + 1) / 512) * (max' - min') + min',  min' = lo - 3 h,  max' = hi + 3 h
 *     raw[j] = (1 / n) sum_i exp(-(x_i - x[j])^2 / h^2)              (FIGTree's kernel: no factor 2, no 1 / (h sqrt(pi)))
 *     y[j] = raw[j] / ((raw[0] + raw[1] + ... in order) * (x[1] - x[0]))
 * NOT FIGTree's output: figtree() (:81) approximates raw with |figtree - raw| <= 1e-2 before the normalisation; this is
 * raw itself, FP64 exp of the device library on every (source, target) pair except those whose every term is exactly
 * +0.0 (argument below -746).  The result is a pure function of (values, n): two calls, or a host and a device buffer,
 * give identical bits.
 * garlic_feed_kde: `sorted` holds n doubles, ascending; `where` GARLIC_DEVICE or GARLIC_HOST (uploaded, never modified).
 * It does not sort.  GARLIC_ERR_INVALID, with a message that names the cause and *out untouched: n < 2; a NaN or an
 * infinity; x[i] < x[i - 1] somewhere; h equal to 0 or not finite (all values equal, or more than half of them).  Scratch
 * (8 B per 2048 values, up to 8 MB of slice sums; a host buffer: n doubles more) is kept with the context until
 * garlic_panel_release_scratch; GARLIC_ERR_NOMEM leaves everything untouched.
 * garlic_lod_kde: garlic_lod_feed_subset up to, not including, the copy to the host -- same arguments, same kernel forms,
 * same garlic_lod_feed_info and chr_counts -- always in ascending order whatever garlic_panel_set_feed_order says (the
 * setting is left as found), then garlic_feed_kde on the device buffer: no feed value crosses PCIe.  An empty feed is the
 * n < 2 error.  A sweep over several window sizes: garlic_lod_kde_multi, below.
 * garlic_feed_kde_info: of the last KDE on the context: chunks of 2048 sources, (chunk, target) pairs skipped as exactly
 * zero, bytes of scratch held (the scratch is shared with garlic_feed_kde_multi; the records of the two calls are not: a
 * multi-feed KDE in between changes neither the chunks nor the pairs nor the times reported here).  Any pointer may be NULL.
 * garlic_feed_kde_times: HIP-event times of the last successful KDE on the context: the two moment passes with their
 * tree kernels, and the sums with the slice reduction (tools/bench_variants.py --modes feed_kde).  Any pointer may be NULL. */
#define GARLIC_KDE_POINTS 512
typedef struct garlic_kde {
    int64_t n;            /* sources */
    double h, sd, q25, q75, lo, hi;   /* lo = x[0], hi = x[n-1] of the feed */
    double x[GARLIC_KDE_POINTS], y[GARLIC_KDE_POINTS], raw[GARLIC_KDE_POINTS];
} garlic_kde;
int garlic_feed_kde(garlic_ctx *ctx, const double *sorted, int64_t n, int32_t where, garlic_kde *out);
int garlic_lod_kde(garlic_panel *panel, int32_t winsize, double error, int32_t max_gap, int32_t use_gl,
                   int32_t weighted, int32_t M, double mu, int32_t step, const int32_t *ind_idx, int32_t n_idx,
                   garlic_kde *out, int64_t *chr_counts);
int garlic_feed_kde_info(garlic_ctx *ctx, int64_t *chunks, int64_t *pairs_skipped, int64_t *scratch_bytes);
int garlic_feed_kde_times(garlic_ctx *ctx, float *moments_ms, float *sums_ms);

/* The KDE of several feeds in one call (csrc/kde_multi_kernels.hpp; which workgroup does what: host/kde_multi_plan.hpp):
 * the window sizes of a sweep (exploreWinsizes, selectWinsize, selectWinsizeFromList) without a pass, two waits and six
 * small launches per size.  The four steps of garlic_feed_kde run once each for all feeds -- two moment passes, two tree
 * passes, one sums launch, one slice launch: SIX kernel launches whatever n_feeds is -- and the host waits on the
 * context's stream TWICE in the call: for all feeds' moments (it then computes every h and every target set and uploads
 * them in one copy), and for all feeds' sums and skip counts.  When no feed is left after the moments the sums part is
 * skipped: four launches, one wait.  A feed's partition, element order and summation trees are those of garlic_feed_kde
 * (the same source lines), so every successful outs[i] equals garlic_feed_kde's struct for feed i alone, in every field,
 * bit for bit, whatever else is in the batch.
 * garlic_feed_kde_multi: sorted[i] holds n[i] doubles, ascending, 1 <= n_feeds <= GARLIC_KDE_MAX_FEEDS.  GARLIC_DEVICE:
 * borrowed, never modified; GARLIC_HOST: uploaded one after the other into context scratch.  Per feed:
 *     status != NULL: the call returns GARLIC_OK when it ran; status[i] is GARLIC_OK or GARLIC_ERR_INVALID for what
 *       garlic_feed_kde refuses (n < 2; a NaN or an infinity; not ascending; a bad bandwidth).  outs[i] of a refused feed
 *       is untouched, and garlic_hip_last_error names the lowest refused index and its cause ("feed 3: " and
 *       garlic_feed_kde's words).  A feed refused after the moments takes no part in the sums launches.
 *     status == NULL: any refused feed makes the call return its code, with ALL outs untouched.
 * Argument errors -- a NULL ctx, sorted, n or outs; n_feeds out of range; a bad `where`; sorted[i] NULL with n[i] > 0; more
 * than 2^31 - 1 chunks in all -- and GARLIC_ERR_NOMEM leave everything untouched.  Scratch (8 B + 4 B per 2048 values, the
 * slice sums, 8.5 KB per feed of table; host buffers: the values) is kept with the context until
 * garlic_panel_release_scratch.
 * garlic_lod_kde_multi: unweighted scores (no weighted multi-size feed exists).  garlic_lod_feed_multi (use_gl == 0) or
 * garlic_lod_feed_multi_tgls (use_gl != 0) up to, not including, the copy to the host -- the same validation of winsizes,
 * steps and ind_idx, the same planning, kernel forms and grouping, the same garlic_lod_feed_info /
 * garlic_lod_feed_multi_info answers and chr_counts ([n_sizes][nchr], or NULL) -- always in ascending order (the order
 * setting is left as found); a size that those calls run through the single-size path has its feed moved, device to
 * device, out of the panel's scratch before the next size runs.  Then the batched KDE on the sizes' device buffers, on the
 * context's stream behind an event from every size's stream: no feed value crosses PCIe.  n_sizes <=
 * GARLIC_KDE_MAX_FEEDS.  outs[i] equals garlic_lod_kde(winsizes[i], .., steps[i], ..)'s struct bit for bit; status and the
 * untouched-output rules as above; a size whose feed holds fewer than 2 values (a window wider than every chromosome) is
 * refused in garlic_lod_kde's words.  Like every feed call it makes KDE parts borrowed from the panel earlier stale.
 * garlic_feed_kde_multi_info: of the last multi-feed KDE on the context, for its first n feeds: chunks[i] = ceil(n_i / 2048)
 * (0 for a feed refused before the moments), pairs_skipped[i], *kernel_launches (6, or 4), *host_waits (2, or 1), bytes of
 * scratch held, HIP-event times of the moment part and the sums part.  Any pointer may be NULL. */
#define GARLIC_KDE_MAX_FEEDS 32
int garlic_feed_kde_multi(garlic_ctx *ctx, const double *const *sorted, const int64_t *n, int32_t n_feeds, int32_t where,
                          garlic_kde *outs, int32_t *status);
int garlic_lod_kde_multi(garlic_panel *panel, const int32_t *winsizes, const int32_t *steps, int32_t n_sizes, double error,
                         int32_t max_gap, int32_t use_gl, const int32_t *ind_idx, int32_t n_idx, garlic_kde *outs,
                         int32_t *status, int64_t *chr_counts);
int garlic_feed_kde_multi_info(garlic_ctx *ctx, int32_t n, int64_t *chunks, int64_t *pairs_skipped, int32_t *kernel_launches,
                               int32_t *host_waits, int64_t *scratch_bytes, float *moments_ms, float *sums_ms);

/* The KDE of a feed that is split into sorted parts: a sharded panel makes one part per shard, each on its shard's device,
 * and no feed value leaves its device.  n, the sum, the sum of squared deviations and the 512 Gaussian sums add over the
 * parts; lo / hi are a min and a max; the four order statistics x[k25], x[k25 + 1], x[k75], x[k75 + 1] of the union are
 * found exactly with rank queries (csrc/kde_multi_kernels.hpp: kde_rank_multi_kernel; the descent and the combination rules:
 * host/kde_parts.hpp).
 *
 * garlic_kde_part_create: `sorted` holds n >= 0 doubles in the key order of garlic_feed_sort (the library's own feeds are).
 * GARLIC_DEVICE: borrowed, it must stay valid and unchanged until garlic_kde_part_destroy; GARLIC_HOST: uploaded into
 * memory the part owns (the caller's buffer is free again on return).  A part's scratch (8 B per 2048 values, up to 8 MB
 * of slice sums, 20 KB of probes and counts, a pinned block of the same size on the host) lives and ends with the part;
 * destroy the parts before their context.  GARLIC_ERR_NOMEM leaves everything untouched.
 * garlic_lod_kde_part: garlic_lod_kde up to, not including, the KDE: the panel's sorted device feed becomes the part.  It
 * is borrowed from the panel's scratch: the next call on that panel that computes scores or a feed, or
 * garlic_panel_release_scratch, or garlic_panel_destroy, makes the part stale, and any use of a stale part (destroy
 * excepted) is GARLIC_ERR_STATE.  An empty feed is a valid part.
 *
 * The steps -- what a caller with one process per GPU all-reduces between:
 * garlic_kde_part_moment: pass 0: *value = the part's sum (the tree of garlic_feed_kde), *lo = x[0], *hi = x[n - 1]; an
 * empty part: 0.0, lo / hi untouched; GARLIC_ERR_INVALID with a message that names the cause for a NaN or an infinity,
 * or x[i] < x[i - 1] somewhere.  Pass 1: *value = the sum of (x - mean)^2 for the mean given.  lo / hi may be NULL.
 * garlic_kde_part_rank: below[t] = the number of the part's values whose key (garlic_feed_sort's) is below keys[t],
 * 1 <= m <= 1024; an empty part: 0 everywhere.
 * garlic_kde_part_sums: sums[j] = sum_i exp(-(x_i - targets[j])^2 * (1 / h^2)), 512 targets, NOT divided by anything; the
 * chunk / slice partition (a function of the part's n alone), the exact skipping and the skipped-pair count of
 * garlic_feed_kde.  An empty part: 0.0 everywhere.
 * Every step call of a part runs whatever an earlier one refused: pass 1, the ranks and the sums of a part whose pass 0
 * met a NaN are still computed.  (A garlic_kde_part_set, below, leaves a refused feed out until its next pass 0.)
 *
 * garlic_kde_parts: the whole KDE of the union of parts[0 .. n_parts), 1 <= n_parts <= GARLIC_KDE_MAX_PARTS, on any mix
 * of contexts and devices; each step is enqueued on every part's stream before any is waited for.
 *     n = sum n_p                                    (n < 2: the "at least 2 values" error)
 *     mean = (((0.0 + s_0) + s_1) + ...) / (double)n,  ssq by the same rule,  sd = sqrt(ssq / (n - 1))
 *     lo / hi: the min / max over the non-empty parts
 *     the order statistics: a radix descent over the key, most significant byte first, exactly 8 rounds.  In a round the
 *       four ranks probe their 256 candidate digits with one garlic_kde_part_rank (m = 1024) per part, the host adds the
 *       parts' counts and keeps, per rank r, the largest digit whose count is <= r.  After round 8 the key is the value.
 *     q25, q75, h, x: as garlic_feed_kde from these (same bandwidth errors)
 *     raw[j] = ((((0.0 + S_0[j]) + S_1[j]) + ...) / (double)n,  y from raw as garlic_feed_kde
 * The result is a pure function of (the parts' values, their order).  n, q25, q75, lo and hi do not depend on how the
 * union is split.  With ONE part every field equals garlic_feed_kde's bit for bit.  Parts must be in garlic_feed_sort's
 * key order; for a caller's buffer that puts +0.0 in front of -0.0 the sign of a zero order statistic is unspecified.
 * GARLIC_ERR_INVALID with *out untouched: a NULL part or out, n_parts out of range, the same part twice, and what
 * garlic_feed_kde refuses (it names the cause).
 * garlic_kde_parts_info: of the last garlic_kde_parts (or step call) on these parts: chunks[p] = ceil(n_p / 2048),
 * pairs_skipped[p], *rank_rounds (8 after garlic_kde_parts), sums_ms[p] the HIP-event time of part p's sums.  Any
 * pointer but parts may be NULL. */
#define GARLIC_KDE_MAX_PARTS 64
typedef struct garlic_kde_part garlic_kde_part;
int garlic_kde_part_create(garlic_ctx *ctx, const double *sorted, int64_t n, int32_t where, garlic_kde_part **part);
int garlic_lod_kde_part(garlic_panel *panel, int32_t winsize, double error, int32_t max_gap, int32_t use_gl,
                        int32_t weighted, int32_t M, double mu, int32_t step, const int32_t *ind_idx, int32_t n_idx,
                        garlic_kde_part **part, int64_t *chr_counts);
int garlic_kde_part_destroy(garlic_kde_part *part);
int garlic_kde_part_count(garlic_kde_part *part, int64_t *n);
int garlic_kde_part_moment(garlic_kde_part *part, int32_t pass, double mean, double *value, double *lo, double *hi);
int garlic_kde_part_rank(garlic_kde_part *part, const uint64_t *keys, int32_t m, int64_t *below);
int garlic_kde_part_sums(garlic_kde_part *part, const double *targets, double h, double *sums);
int garlic_kde_parts(garlic_kde_part *const *parts, int32_t n_parts, garlic_kde *out);
int garlic_kde_parts_info(garlic_kde_part *const *parts, int32_t n_parts, int64_t *chunks, int64_t *pairs_skipped,
                          int32_t *rank_rounds, float *sums_ms);

/* The KDEs of several split feeds at once -- every window size of a sweep on a sharded panel (csrc/kde_part_set_kernels.hpp,
 * kde_rank_multi_kernel of csrc/kde_multi_kernels.hpp; the descent for F feeds: host/kde_parts.hpp, kdeSelectRanksMulti).  A garlic_kde_part_set is
 * the F feeds (1 <= F <= GARLIC_KDE_MAX_FEEDS) of ONE shard on one context: feed i of the set is that shard's part of
 * union i.  Every step of garlic_kde_parts runs once per set for all its feeds: per set 4 moment launches, 8 rank launches
 * of F x 1024 probes, 2 sums launches and 11 host waits, whatever F is.
 *
 * garlic_kde_part_set_create: sorted[i] holds n[i] >= 0 doubles in garlic_feed_sort's key order; feed i may be empty
 * (sorted[i] is not read then).  GARLIC_DEVICE: borrowed until garlic_kde_part_set_destroy; GARLIC_HOST: uploaded, one
 * after the other, into memory the set owns.  The set's scratch (8 B per 2048 values, the slice sums, 8.3 KB of table
 * and 16 KB of probes and counts per feed, and a pinned block of the table's and the probes' size on the host) lives and
 * ends with the set; destroy the sets before their context.  GARLIC_ERR_NOMEM leaves everything untouched.
 * garlic_lod_kde_part_set: garlic_lod_kde_multi up to, not including, the KDE -- the same validation, planning, kernel
 * forms and grouping, the same garlic_lod_feed_info, garlic_lod_feed_multi_info and chr_counts; unweighted scores and
 * use_gl only.  The sizes' sorted device feeds become the set's feeds, borrowed from the panel's feed slots: the set is
 * stale by garlic_lod_kde_part's rule, and any use of a stale set (destroy excepted) is GARLIC_ERR_STATE.
 * garlic_kde_part_set_counts: n[i] = the length of feed i, F values.
 *
 * The steps, each for all F feeds in one pass -- what a caller with one process per GPU all-reduces between
 * (INTEGRATION.md).  A feed that is switched off takes no part in a step: no kernel reads it, and its entries of the
 * output arrays are left as they were.  Every feed is switched on by a pass 0; it is switched off by a nonzero status[i]
 * on entry to a moment step, by what a moment step refuses of it, and by active[i] == 0 in the sums step, and stays off
 * up to the set's next pass 0.
 * garlic_kde_part_set_moment: pass 0: values[i] = the sum of feed i (the tree of garlic_feed_kde), lo[i] / hi[i] its ends;
 * an empty feed: 0.0, lo / hi untouched; `means` is not read.  Pass 1: values[i] = the sum of (x - means[i])^2.
 * status: on return of pass 0, status[i] = GARLIC_ERR_INVALID for a feed with a NaN or an infinity or x[j] < x[j - 1]
 * (garlic_hip_last_error names the lowest such feed and the cause), entries that came in nonzero are kept, the others are
 * 0.  status == NULL: every feed takes part and such a feed fails the call.  lo / hi may be NULL.
 * garlic_kde_part_set_rank: keys[i * m + t], below[i * m + t]: garlic_kde_part_rank on feed i, 1 <= m <= 1024, one launch.
 * garlic_kde_part_set_sums: targets[i * 512 + j], h[i], sums[i * 512 + j], pairs_skipped[i]: garlic_kde_part_sums on feed i
 * (undivided).  active and pairs_skipped may be NULL.
 *
 * garlic_kde_parts_multi: the KDEs of the F unions {feed i of sets[0], feed i of sets[1], ...}, 1 <= n_sets <=
 * GARLIC_KDE_MAX_PARTS, all sets with the same F, on any mix of contexts and devices; every step is enqueued on every
 * set's stream before any is waited for.  outs[i] equals, in every field bit for bit, what garlic_kde_parts returns for
 * those parts in that order, whatever else is in the batch: so with ONE set outs[i] is garlic_feed_kde_multi's struct, and
 * n, q25, q75, lo and hi do not depend on the split.  status and the untouched outputs are garlic_feed_kde_multi's:
 * status[i] = GARLIC_OK or the code garlic_kde_parts would fail with (fewer than 2 values in the union; a NaN; not
 * ascending; no bandwidth), outs[i] is written only where status[i] is GARLIC_OK, the call returns GARLIC_OK and
 * garlic_hip_last_error reads "feed <i>: ..." for the lowest refused i ("feed <i>: set <p>: ..." where the values of one
 * part are at fault); status == NULL: a refused feed fails the call at the step that refuses it (the lengths, the first
 * moment pass, the bandwidths) with the code and text of the lowest feed refused by then, all outs untouched.  A feed
 * refused at the moments or at the bandwidth takes no part in the later steps.
 * garlic_kde_parts_multi_info: of the last garlic_kde_parts_multi (or step calls) on these sets: chunks[p * F + i] and
 * pairs_skipped[p * F + i] per set and feed; per set kernel_launches[p], host_waits[p] (a set without any value: 8 and
 * 8, the ranks alone), rank_rounds[p], moments_ms[p] (HIP events from the first moment launch to the last: the host's
 * turn between the two passes is inside) and sums_ms[p].  Any pointer but sets may be NULL. */
typedef struct garlic_kde_part_set garlic_kde_part_set;
int garlic_kde_part_set_create(garlic_ctx *ctx, const double *const *sorted, const int64_t *n, int32_t n_feeds, int32_t where,
                               garlic_kde_part_set **set);
int garlic_lod_kde_part_set(garlic_panel *panel, const int32_t *winsizes, const int32_t *steps, int32_t n_sizes, double error,
                            int32_t max_gap, int32_t use_gl, const int32_t *ind_idx, int32_t n_idx, garlic_kde_part_set **set,
                            int64_t *chr_counts);
int garlic_kde_part_set_destroy(garlic_kde_part_set *set);
int garlic_kde_part_set_counts(garlic_kde_part_set *set, int64_t *n);
int garlic_kde_part_set_moment(garlic_kde_part_set *set, int32_t pass, const double *means, double *values, double *lo, double *hi,
                               int32_t *status);
int garlic_kde_part_set_rank(garlic_kde_part_set *set, const uint64_t *keys, int32_t m, int64_t *below);
int garlic_kde_part_set_sums(garlic_kde_part_set *set, const double *targets, const double *h, const int32_t *active, double *sums,
                             int64_t *pairs_skipped);
int garlic_kde_parts_multi(garlic_kde_part_set *const *sets, int32_t n_sets, garlic_kde *outs, int32_t *status);
int garlic_kde_parts_multi_info(garlic_kde_part_set *const *sets, int32_t n_sets, int64_t *chunks, int64_t *pairs_skipped,
                                int32_t *kernel_launches, int32_t *host_waits, int32_t *rank_rounds, float *moments_ms,
                                float *sums_ms);

/* GMM::estimate (src/gmm.cpp:385-442) on the device: the EM fit of a 1-D mixture of k Gaussians that selectSizeClasses
 * (src/garlic-roh.cpp:935-1003) runs on the ROH lengths (csrc/gmm_kernels.hpp; the initial guess, the ordering of the
 * classes and the boundaries between them: host/size_classes.hpp).  One update (GMM::update, :276-331), per point x_j:
 *     r_i  = log(a_i) + (C - 0.5 log(var_i) - (x_j - mean_i)^2 / (2.0 var_i)),   C = -0.5 log(2 pi)
 *     tmp  = l_max + log(sum_i exp(r_i - l_max)),  l_max = max_i r_i;   L += tmp
 *     r_i <- exp(r_i - tmp),  den = sum_i r_i
 *     S0_k += r_k / den,  S1_k += x_j * r_k / den,  S2_k += x_j * x_j * r_k / den
 * then a_k = S0_k / n, mean_k = S1_k / S0_k, var_k = S2_k / S0_k - mean_k * mean_k, loglik = L,
 * bic = -2 L + (3 k - 1) log(n) -- the reference's operations in its association, the n-term sums in a fixed tree that
 * depends on n and k alone, each with the rounding errors of its adds carried in a second double and added at the end (a sum
 * that is not finite: the plain sum), exp and log of the device library.  The fit stops after the first update with
 * |L - L_prev| <= precision (L_prev starts at -DBL_MAX; a NaN never stops it, nor does precision < 0: then exactly
 * max_iter updates run) or after max_iter updates.  The result is a pure function of the arguments: two calls, a host or a
 * device buffer, any device, give identical bits.
 * garlic_gmm_fit: x holds n doubles, `where` GARLIC_DEVICE or GARLIC_HOST (uploaded, never modified); a0 / mean0 / var0
 * hold the k initial mixture weights, means and variances (host).  out->iterations: the updates run; out->converged: 1
 * when the stop rule ended the fit.  NaN or infinite parameters are no error: they are returned as computed, with
 * converged 0.  GARLIC_ERR_INVALID: a NULL pointer, n < 1, k < 1, k > GARLIC_GMM_MAX_K, max_iter < 1, another `where`.
 * Scratch (2 (3 k + 1) doubles per 2048 points; a host buffer: n doubles more) is kept with the context until
 * garlic_panel_release_scratch; GARLIC_ERR_NOMEM leaves everything untouched.
 * garlic_gmm_fit_info: of the last fit on the context: workgroups of a pass (ceil(n / 2048)), bytes of scratch held, the
 * HIP-event time of the EM loop (the waits for the state between batches of updates included).  Any pointer may be NULL. */
#define GARLIC_GMM_MAX_K 8
typedef struct garlic_gmm {
    int32_t k, iterations, converged;
    double a[GARLIC_GMM_MAX_K], mean[GARLIC_GMM_MAX_K], var[GARLIC_GMM_MAX_K];
    double loglik, bic;
} garlic_gmm;
int garlic_gmm_fit(garlic_ctx *ctx, const double *x, int64_t n, int32_t where, int32_t k,
                   const double *a0, const double *mean0, const double *var0,
                   int32_t max_iter, double precision, garlic_gmm *out);
int garlic_gmm_fit_info(garlic_ctx *ctx, int64_t *blocks, int64_t *scratch_bytes, float *em_ms);

/* First half of assembleROHWindows (src/garlic-roh.cpp:446-454) on the device: for every individual
 * and SNP the number of windows with score >= cutoff that cover the SNP,
 *     inWin[l] = #{ w in (l - winsize, l] : scores[w] >= cutoff }
 * (MISSING and NaN never qualify; the reference indexes past the array for a qualifying window in
 * the last winsize-1 positions, which only a cutoff <= -9999 can produce: here such windows cover
 * the SNPs that exist).  scores: device memory laid out as garlic_lod_out_layout(pitch_align,
 * nind_out); inwin: int16 elements addressed the same way with inwin_pitch_align (1 = dense rows of
 * nloci_c), host or device per `where`.  The caller compares inWin with
 * OVERLAP_FRAC * winsize clamped to [1, winsize] (:422-424) -- 2 bytes per (individual, SNP) cross
 * PCIe instead of 8. */
int garlic_roh_coverage(garlic_panel *panel, const double *scores, int32_t pitch_align, int32_t nind_out,
                        int32_t winsize, double cutoff, int16_t *inwin, int32_t inwin_pitch_align,
                        int32_t where);

/* The same counts for the unweighted --error scores of every individual of the panel, computed WITHOUT the scores:
 * calcLOD's chain (src/garlic-roh.cpp:18-132) leaves one bit per window and individual -- score >= cutoff, the score
 * itself only ever in a register -- and the inWin[] loop (:446-454) becomes a count over the last winsize bits.  What
 * GARLIC's final pass needs when --raw-lod is not asked for: 2 bytes per window leave the device and no score matrix
 * is resident.  inwin as for garlic_roh_coverage (inwin_pitch_align a multiple of 8 lets the kernel store 16 bytes
 * at a time).  use_gl / weighted / M / mu as for garlic_lod_windows / garlic_wlod_windows: with `weighted` the tuned
 * wLOD kernels leave the bits themselves (16 per individual and group instead of 16 scores), with unweighted
 * per-genotype likelihoods the TGLS chain does (32 per individual and tile).  Falls back to scores + garlic_roh_coverage where the bit form
 * does not apply (cutoff <= -9999; unweighted: winsize > 1024, non-finite terms, window sums that can be -9999.0). */
int garlic_roh_coverage_fused(garlic_panel *panel, int32_t winsize, double error, int32_t max_gap, int32_t use_gl,
                              int32_t weighted, int32_t M, double mu, double cutoff, int16_t *inwin,
                              int32_t inwin_pitch_align, int32_t where);

/* The ROH segments themselves: assembleROHWindows (src/garlic-roh.cpp:409-545) from the panel to its
 * rohData->start / stop lists, with neither the scores nor the coverage counts ever in memory.  The window bits come as
 * for garlic_roh_coverage_fused (same arguments, same fallbacks); on the device they become "SNP is covered by at least
 * OVERLAP_FRAC * winsize qualifying windows" bits (threshold clamped to [1, winsize], :421-423), and the four-branch
 * walk over every individual's SNPs (:456-533) becomes: maximal stretches of such SNPs, cut where two neighbours are
 * more than max_gap apart or straddle the centromere, kept when they hold at least the threshold's number of SNPs
 * (and not begun at the chromosome's last SNP: the reference never closes such a segment).
 *   segments[k] = {individual (panel-relative), chromosome (index in the panel), first SNP, last SNP}, SNP indices
 *   chromosome-local and inclusive; the caller maps them to positions (physicalPos / geneticPos of :470-520).
 *   Ordered by individual, chromosome, first SNP -- the order the reference appends them in.
 * *n_segments is the number found; when it exceeds `capacity` nothing usable is in `segments` (call again with room;
 * capacity 0 / segments NULL just counts).  A few MB for a 10M-SNP x 1250-individual shard, against 25 GB of counts.
 * Positions must be >= 0.  The reference tells "a segment is open" by its first POSITION being > 0 and "none" by
 * < 0 (:456, :493, :514): on a 0-based map a stretch opened at a chromosome's SNP 0 is neither -- nothing closes it but
 * a covered SNP behind a break, and it is reported from SNP 0 to the SNP in front of that one whatever lies between.
 * Reproduced as is (pinned against the real assembleROHWindows). */
typedef struct garlic_roh_segment {
    int32_t ind, chr, start, stop;
} garlic_roh_segment;
int garlic_roh_segments(garlic_panel *panel, int32_t winsize, double error, int32_t max_gap, int32_t use_gl, int32_t weighted,
                        int32_t M, double mu, double cutoff, double overlap_frac, garlic_roh_segment *segments,
                        int64_t capacity, int64_t *n_segments);

/* count_features_in_roh.pl (the reference's src/) on the device: for every individual, the homozygous genotypes of
 * annotated alleles that fall inside ROH of each size class and outside any ROH (csrc/feature_kernels.hpp; the file
 * readers, the interval builder and the table writer: host/feature_counts.hpp).
 *
 * A feature set holds `nrows` hom rows over `nind` individuals: one row per annotated (site, allele) that occurs in the
 * counting genotypes, bit i set when individual i is homozygous for that allele (a missing genotype and a heterozygote
 * set nothing).  Destroy the sets before their context.
 * garlic_feature_set_rows: host bit rows, `row_bytes` apart, bit i & 7 of byte i >> 3 is individual i (LSB first, as
 * garlic_panel_set_phase_bits), uploaded in slabs; bits past nind are ignored.  Rows never set hold no homozygote.  The
 * caller's rows are free on return.
 * garlic_feature_set_rows_bed: the rows [row_begin, row_begin + row_count) from a .bed image on the set's device, no
 * genotype crosses the host: row row_begin + k is built from image row file_row[k] (any order, repeats allowed: the two
 * alleles of one site) by allele[k]: 0 = homozygous for A1 (PLINK code 00), 1 = homozygous for A2 (code 11), 2 = no bit
 * (an annotated allele that is neither, or the absent allele `0` of a monomorphic site).  Missing (01) and heterozygous
 * (10) genotypes set nothing; the bits past nind are 0 whatever the pad bits of the image hold.  file_row and allele are
 * host arrays of row_count entries, copied before the call returns; the work runs on the set's context's stream and the
 * call returns when it is done (the image may then be destroyed).  The image may be an ordinary one or one made by
 * garlic_bed_extract; rows set this way and by garlic_feature_set_rows may be mixed in one set; row_count = 0 does
 * nothing.  GARLIC_ERR_INVALID, and the set unchanged: a NULL argument, the set's nind != the image's nind_total, the
 * image on another device than the set's context, a row range outside the set, a file_row outside [0, nrows) or an
 * allele > 2 (the message names the first such entry); GARLIC_ERR_STATE: an image that is not fully set.
 * garlic_feature_set_get_rows: the rows [row_begin, row_begin + row_count) as they stand on the device, in the format
 * garlic_feature_set_rows takes, `row_bytes` >= (nind + 7) / 8 apart; the bytes past a row's own are not touched.  Waits
 * for the work queued on the set.  A door for checks: the rows are transposed on the host.
 * garlic_feature_set_sites: per row the chromosome (any id >= 0 the caller also uses in the intervals), the physical
 * position and the effect id in [0, GARLIC_FEATURE_MAX_EFFECTS).  GARLIC_ERR_INVALID for rows that are not sorted by
 * (chromosome, position); two rows may share a position (two alleles of one site, with different effects).
 * garlic_feature_counts: counts[ind][cls][effect], int64, n_classes + 1 classes of n_effects each: the rows whose bit
 * `ind` is set, by the class of the interval of `ind` that holds the row's position and by the row's effect; class
 * n_classes is NONE, the rows inside no interval.  A position p is inside an interval iff chr is the row's and
 *     start <= p < stop
 * where stop is the `end` column of a .roh.bed line: GARLIC's writer puts the LAST SNP's position there and the script
 * tests p <= end - 1, so a variant exactly at a segment's last SNP counts as outside.  That is reproduced, not mended.
 * An interval with start == stop holds nothing.  The intervals are a host array in the order garlic_roh_segments returns
 * segments in -- individual, chromosome, start -- and must not overlap within an individual (start >= the previous
 * stop); GARLIC_ERR_INVALID names the first interval that is out of order, overlaps, has cls outside [0, n_classes) or
 * ind outside [0, nind).  1 <= n_classes <= GARLIC_GMM_MAX_K; 1 <= n_effects <= GARLIC_FEATURE_MAX_EFFECTS and above
 * every row's effect, else GARLIC_ERR_INVALID; a launch counts 32 effects, more are further launches over the same rows.
 * counts are overwritten, not accumulated: `where` = GARLIC_HOST copies them out and returns when they are there;
 * GARLIC_DEVICE: counts is device memory, the call enqueues on the context's stream and returns (the list of intervals
 * is copied before it returns).  Integer sums: the same bytes from run to run.
 * garlic_feature_counts_info: of the last garlic_feature_counts: the 64-individual blocks, the chunks of rows per block
 * (ceil(nrows / 4096): one wavefront per block and chunk), the 64-bit words that were zero and skipped, the HIP-event
 * time of the kernels.  The last two wait for that call's kernels.  Any pointer but the set may be NULL. */
#define GARLIC_FEATURE_MAX_EFFECTS 256
typedef struct garlic_feature_set garlic_feature_set;
typedef struct garlic_roh_interval {
    int32_t ind, chr, start, stop, cls;
} garlic_roh_interval;
int garlic_feature_set_create(garlic_ctx *ctx, int64_t nrows, int32_t nind, garlic_feature_set **set);
int garlic_feature_set_destroy(garlic_feature_set *set);
int garlic_feature_set_rows(garlic_feature_set *set, const uint8_t *bits, int64_t row_bytes, int64_t row_begin, int64_t row_count);
int garlic_feature_set_rows_bed(garlic_feature_set *set, garlic_bed *bed, const int64_t *file_row, const uint8_t *allele,
                                int64_t row_begin, int64_t row_count);
int garlic_feature_set_get_rows(garlic_feature_set *set, int64_t row_begin, int64_t row_count, uint8_t *bits, int64_t row_bytes);
int garlic_feature_set_sites(garlic_feature_set *set, const int32_t *chr, const int32_t *pos, const int32_t *effect);
int garlic_feature_counts(garlic_feature_set *set, const garlic_roh_interval *intervals, int64_t n_intervals, int32_t n_classes,
                          int32_t n_effects, int64_t *counts, int32_t where);
int garlic_feature_counts_info(garlic_feature_set *set, int64_t *blocks, int64_t *chunks, int64_t *words_skipped, float *kernel_ms);

/* Introspection used by tests and the bench (device work of the last garlic_*_windows call). */
typedef struct garlic_call_stats {
    int64_t n_segments;      /* gap/centromere-free SNP segments over all chromosomes */
    int64_t n_runs;          /* segments long enough to hold a window (maximal valid runs) */
    int64_t n_chain_items;   /* (run, 64-individual block) work items = wavefronts launched */
    int64_t n_valid_windows; /* scored windows per individual */
    int64_t n_missing;       /* MISSING windows per individual */
    float chain_kernel_ms;   /* HIP-event time of the dominant kernel on the context stream */
    float total_ms;          /* HIP-event time of the whole call's device work */
    /* ABI 8: liveness book-keeping, cumulative since the panel was created; both are expected to stay 0.
     * n_stall_reruns: launches of the strip kernel (--weighted with per-genotype likelihoods) in which a wave ran out of
     * its poll budget and that the tile form, enqueued behind every strip launch, therefore recomputed (on the device:
     * no call synchronises for it).  n_count_timeouts: garlic_roh_coverage_fused calls that failed because a count item
     * gave up waiting for its chromosome's chains (GARLIC_COVERAGE_OVERLAP=1 only). */
    int64_t n_stall_reruns;
    int64_t n_count_timeouts;
} garlic_call_stats;
int garlic_last_call_stats(garlic_panel *panel, garlic_call_stats *stats);

/* Which rolling-sum chain the last unweighted / TGLS score call ran.  The reference decides "the previous window
 * holds no score" by VALUE (garlic-roh.cpp:79), so a scored window that sums to exactly -9999.0 restarts the sum.
 * 0: such a sum is impossible for this panel and window size (W x the most negative term stays above -9999): the
 * tuned chain; 1: possible -- the tuned chain ran, its scored windows were scanned, none was -9999.0; 2: one was
 * (or the environment forces it): the chain that follows the reference to the letter ran (11-17 x slower). */
int garlic_panel_chain_kind(garlic_panel *panel, int32_t *kind);

/* Score memory for where = GARLIC_DEVICE calls.  garlic_device_alloc: a virtual range backed by physical chunks of
 * its own (HIP virtual memory management; hipMalloc where the driver has none).  Freed buffers stay mapped in a pool
 * and are handed out again for requests they fit (a caller that allocates per sweep reuses the same few ranges; the
 * pool is capped at a quarter of the device memory, GARLIC_ALLOC_POOL_GB).  garlic_device_alloc_stats: bytes handed
 * out, bytes idle in the pool, bytes of address space reserved in all (any of the three may be NULL).
 * Where a score buffer sits in VRAM decides between two speeds of the unweighted kernel (1.36 / 1.62 ms at 1M SNPs x
 * 1000 individuals).  garlic_panel_alloc_scores allocates `candidates` (0 = 4) buffers for the
 * layout garlic_lod_out_layout(pitch_align, nind_out), times the real kernel for `winsize` into each and keeps the
 * fastest; candidate_ms (may be NULL): the kernel time into each candidate.  Buffers allocated together can all sit on
 * the slow side, so unless the best candidate of a round takes its score bytes at >= 0.74 of the HBM peak (the fast
 * placement; out of reach for small panels, which then simply use the budget) a further round is taken from fresh memory
 * while the earlier ones are held: three rounds at most (GARLIC_ALLOC_ROUNDS), 2 s at most, memory permitting;
 * candidate_ms then holds the times of the round the kept buffer came from.  garlic_panel_alloc_scores_info (ABI 8):
 * how many candidates the last call on this panel drew in how many rounds, the best / median / worst kernel time over
 * all of them, the time the 0.74 target corresponds to and whether the kept buffer reached it (any pointer may be NULL).
 * Free with garlic_device_free.  The library's own full-score scratch (host-output calls) is chosen the same way at first
 * use. */
int garlic_device_alloc(garlic_ctx *ctx, int64_t bytes, void **out);
int garlic_device_free(garlic_ctx *ctx, void *ptr);
/* bytes from host memory into device memory of the context's device (a buffer of garlic_device_alloc, or any device pointer),
 * on the context's stream; returns when the copy is done.  For a caller without a HIP runtime of its own that keeps a slab of
 * text on the device and hands it to several where = GARLIC_DEVICE calls (garlic_bed_set_rows_vcf and
 * garlic_tgls_set_rows_vcf on one upload). */
int garlic_device_upload(garlic_ctx *ctx, void *dst, const void *src, int64_t bytes);
/* the twin: bytes from device memory of the context's device into host memory; returns when they are there */
int garlic_device_download(garlic_ctx *ctx, void *dst, const void *src, int64_t bytes);
/* bytes from device memory to device memory of the context's device, ranges that do not overlap (GARLIC_ERR_INVALID if they
 * do); returns when they are there.  The tail of a slab of text moves to the front of the next one with it. */
int garlic_device_copy(garlic_ctx *ctx, void *dst, const void *src, int64_t bytes);

/* BGZF text on the device (csrc/inflate.hpp, csrc/bgzf_kernels.hpp).
 *
 * garlic_bgzf_inflate: nblocks BGZF blocks (gzip members with a BC subfield, at most 65,536 bytes each and at most 65,536
 * inflated) to device memory, one wave per block.  Block b is comp[block_begin[b], block_begin[b + 1]), header and footer
 * included, and inflates to out[out_begin[b], out_begin[b + 1]): out_begin holds the prefix sums of the footers' ISIZEs.
 * comp is host memory (GARLIC_HOST: uploaded into context scratch) or device memory; block_begin, out_begin and
 * block_status (nblocks entries, may be NULL) are host arrays; out is device memory of out_begin[nblocks] bytes.
 * GARLIC_ERR_INVALID without a launch: a NULL argument, nblocks < 0, lists that do not ascend, a member of fewer than 28 or
 * more than 65,536 bytes, an output range of more than 65,536.  Every block gets a status:
 *     GARLIC_BGZF_OK
 *     GARLIC_BGZF_BAD_BLOCK_TYPE    block type 3, stored lengths that do not complement; a header that is not 1F 8B 08 04.  The
 *                                   device takes the deflate data from 12 + XLEN and does NOT look for the BC subfield or compare
 *                                   BSIZE: the caller's lists say where a member ends (bgzf::walk of host/bgzf_blocks.hpp checks both)
 *     GARLIC_BGZF_BAD_CODE_LENGTHS  an over-subscribed or incomplete set of code lengths, where zlib refuses it
 *     GARLIC_BGZF_BAD_SYMBOL        a code that no symbol has, or a symbol outside the alphabet
 *     GARLIC_BGZF_BAD_DISTANCE      a distance that reaches in front of the block's own output
 *     GARLIC_BGZF_INPUT_ENDED       the deflate data ends inside a code
 *     GARLIC_BGZF_OUTPUT_FULL       more bytes than the output range (than ISIZE)
 *     GARLIC_BGZF_OUTPUT_SHORT      fewer
 *     GARLIC_BGZF_BAD_CRC           the CRC32 of the bytes is not the footer's; deflate data left over behind the final block
 * If any is non-zero the call returns GARLIC_ERR_INVALID and garlic_hip_last_error names the lowest such block; the bytes of
 * the clean blocks are written, those of a bad block are unspecified inside its own range, and nothing outside the ranges
 * is touched.  The call returns when the statuses are on the host. */
#define GARLIC_BGZF_OK 0
#define GARLIC_BGZF_BAD_BLOCK_TYPE 1
#define GARLIC_BGZF_BAD_CODE_LENGTHS 2
#define GARLIC_BGZF_BAD_SYMBOL 3
#define GARLIC_BGZF_BAD_DISTANCE 4
#define GARLIC_BGZF_INPUT_ENDED 5
#define GARLIC_BGZF_OUTPUT_FULL 6
#define GARLIC_BGZF_OUTPUT_SHORT 7
#define GARLIC_BGZF_BAD_CRC 8
int garlic_bgzf_inflate(garlic_ctx *ctx, const void *comp, int64_t comp_bytes, const int64_t *block_begin, int64_t nblocks, void *out,
                        const int64_t *out_begin, int32_t *block_status, int32_t where);

/* garlic_text_lines: the line index of a slab of device text, text[0, text_bytes), text_bytes < 2^31: what the host's
 * SlabLines::take(slab, n, last) gives on the same bytes.  Line k of the lines that are not blank (empty, or a lone '\r')
 * and complete in the slab -- the final one needs no '\n' when `last` -- is text[begin[k], end[k]), end[k] its '\n' or
 * text_bytes; number[k] = seen + its 1-based number in the slab, blank lines counted.  heads (may be NULL; head_bytes >= 1
 * then): [capacity][head_bytes] bytes, row k = the first head_bytes bytes of line k, zeros behind a shorter line.
 * begin, end, number and heads are host arrays with room for `capacity` lines.  The caller cannot know the count: the call
 * always sets *n_lines, *consumed (the bytes those lines and the blank ones between them take; the caller carries the rest to
 * the next slab) and *seen_out (seen + the lines taken, blank ones included); when *n_lines > capacity it returns
 * GARLIC_ERR_RANGE with the arrays untouched, and the same call with that much room succeeds.  Scratch (8 bytes per 4 KB of
 * text, 24 bytes + head_bytes per line) stays with the context. */
int garlic_text_lines(garlic_ctx *ctx, const void *text, int64_t text_bytes, int32_t last, int64_t seen, int64_t head_bytes,
                      int64_t capacity, int64_t *begin, int64_t *end, int64_t *number, void *heads, int64_t *n_lines,
                      int64_t *consumed, int64_t *seen_out);

int garlic_device_alloc_stats(garlic_ctx *ctx, int64_t *live_bytes, int64_t *pooled_bytes, int64_t *reserved_bytes);
int garlic_device_trim(garlic_ctx *ctx);   /* idle pooled buffers give their memory back now (the library does this itself
                                              when one of its own allocations runs out of memory) */
int garlic_panel_alloc_scores(garlic_panel *panel, int32_t pitch_align, int32_t nind_out, int32_t winsize, double error,
                              int32_t max_gap, int32_t candidates, void **out, float *candidate_ms);
int garlic_panel_alloc_scores_info(garlic_panel *panel, int32_t *drawn, int32_t *rounds, float *best_ms, float *median_ms,
                                   float *worst_ms, float *target_ms, int32_t *reached_target);

#ifdef __cplusplus
}
#endif
#endif /* GARLIC_HIP_H */
