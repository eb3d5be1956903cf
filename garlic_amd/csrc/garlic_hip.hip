// libgarlic_hip.so -- C ABI (include/garlic_hip.h) over the gfx950 kernels in lod_kernels.hpp.
//
// Host side of the hot path: what calcLODWindows / calcLOD do around the inner loop
// (src/garlic-roh.cpp:18-44, 279-309) -- per-chromosome bookkeeping, the per-SNP term table
// (lod(), src/garlic-roh.cpp:355-386, evaluated once per SNP and genotype with the HOST libm so
// that log10 is the very function the reference calls), segment -> run -> work-list planning --
// and the launches.  There is no CPU fallback: without a HIP device every compute call fails.
#include "../../include/garlic_hip.h"
#include "lod_kernels.hpp"
#include "variant_kernels.hpp"
#include "ld_kernels.hpp"
#include "ld_multi_kernel.hpp"
#include "tgls_ring_kernel.hpp"
#include "tgls_wide_kernel.hpp"
#include "tgls_feed_kernel.hpp"
#include "tgls_feed_multi_kernel.hpp"
#include "wlod_strip_kernel.hpp"
#include "wlod_small_kernel.hpp"
#include "coverage_kernel.hpp"
#include "roh_segments_kernel.hpp"
#include "feed_kernel.hpp"
#include "wlod_feed_kernel.hpp"
#include "feed_sort_kernel.hpp"
#include "kde_kernels.hpp"
#include "kde_multi_kernels.hpp"
#include "kde_part_set_kernels.hpp"
#include "gmm_kernels.hpp"
#include "feature_kernels.hpp"
#include "../host/kde_select.hpp"
#include "../host/kde_parts.hpp"
#include "../host/chain_order.hpp"
#include "bed_kernels.hpp"
#include "vcf_kernels.hpp"
#include "tped_kernels.hpp"
#include "tgls_kernels.hpp"
#include "vcf_gl_kernels.hpp"
#include "bgzf_kernels.hpp"

#include <algorithm>
#include <chrono>
#include <functional>
#include <memory>
#include <mutex>
#include <queue>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <thread>
#include <tuple>
#include <unordered_map>
#include <vector>

using namespace garlic;

namespace {

thread_local std::string g_last_error;

int fail(int code, const char *fmt, ...)
{
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_last_error = buf;
    return code;
}

#define HIP_TRY(expr)                                                                       \
    do {                                                                                    \
        hipError_t e_ = (expr);                                                             \
        if (e_ != hipSuccess)                                                               \
            return fail(e_ == hipErrorOutOfMemory ? GARLIC_ERR_NOMEM : GARLIC_ERR_HIP,      \
                        "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__,   \
                        __LINE__);                                                          \
    } while (0)

// dynamic LDS a launch may ask for until hipFuncAttributeMaxDynamicSharedMemorySize has raised the kernel's limit
constexpr size_t LDS_DEFAULT_MAX = 48 * 1024;
constexpr size_t LDS_STAGING_MAX = 150 * 1024;      // what a kernel that stages whole tiles may take of the CU's 160 KB

int score_pool_trim();    // idle score buffers (garlic_device_free keeps them mapped) give their memory back

struct NoCopy {
    NoCopy() = default;
    NoCopy(const NoCopy &) = delete;
    NoCopy &operator=(const NoCopy &) = delete;
};

// owns its memory: released when it leaves scope (a scope with work in flight that reads it synchronises first)
template <class T> struct DevBuf : NoCopy {
    T *p = nullptr;
    size_t cap = 0;
    ~DevBuf() { release(); }
    int reserve(size_t n)
    {
        if (n <= cap) return GARLIC_OK;
        if (p) (void)hipFree(p);
        p = nullptr;
        cap = 0;
        if (hipMalloc(reinterpret_cast<void **>(&p), n * sizeof(T)) != hipSuccess) {
            (void)hipGetLastError();
            p = nullptr;
            (void)score_pool_trim();                 // out of memory with score buffers idle in the pool: once more without them
        } else {
            cap = n;
            return GARLIC_OK;
        }
        HIP_TRY(hipMalloc(reinterpret_cast<void **>(&p), n * sizeof(T)));
        cap = n;
        return GARLIC_OK;
    }
    int put(const std::vector<T> &h, hipStream_t s)      // room for a host list and the list on its way there (an empty one: nothing)
    {
        int rc = h.empty() ? GARLIC_OK : reserve(h.size());
        if (rc || h.empty()) return rc;
        HIP_TRY(hipMemcpyAsync(p, h.data(), sizeof(T) * h.size(), hipMemcpyHostToDevice, s));
        return GARLIC_OK;
    }
    void release()
    {
        if (p) (void)hipFree(p);
        p = nullptr;
        cap = 0;
    }
};

// what one feed sorter keeps between calls (feed_sort_kernel.hpp): the second key buffer, the tile counts, the digit table
struct FeedSortScratch {
    DevBuf<double> keys, stage;                    // stage: the keys of a host-buffer garlic_feed_sort
    DevBuf<unsigned long long> tiles;
    DevBuf<FsTable> table;
    size_t bytes() const { return keys.cap * sizeof(double) + tiles.cap * sizeof(unsigned long long) + table.cap * sizeof(FsTable); }
    void release() { keys.release(); stage.release(); tiles.release(); table.release(); }
};

// what garlic_feed_kde and garlic_feed_kde_multi keep between calls (kde_multi_kernels.hpp): the feeds of a host-buffer
// call one after the other, the per-chunk partials and flags and the per-slice sums of all feeds, the table of descriptors
struct KdeMultiScratch {
    DevBuf<double> stage, partial, slices;
    DevBuf<int32_t> flags;
    DevBuf<KdeFeedDesc> table;
    hipEvent_t ev[4] = {};                         // around the moments kernels and around the sums kernels
    size_t bytes() const
    {
        return (stage.cap + partial.cap + slices.cap) * sizeof(double) + flags.cap * sizeof(int32_t) + table.cap * sizeof(KdeFeedDesc);
    }
    void release()
    {
        stage.release(); partial.release(); slices.release(); flags.release(); table.release();
        for (auto &e : ev) {
            if (e) (void)hipEventDestroy(e);
            e = nullptr;
        }
    }
    ~KdeMultiScratch() { release(); }
};

// what a whole-feed KDE leaves for the _info calls, per feed and per call
struct KdeInfo {
    std::vector<int64_t> chunks, skipped;
    int32_t launches = 0, waits = 0;
    float moments_ms = 0.f, sums_ms = 0.f;
};

// what garlic_gmm_fit keeps between calls (gmm_kernels.hpp): the blocks' partial sums, the state of the fit
struct GmmScratch {
    DevBuf<double> stage;                          // the values of a host-buffer call
    DevBuf<double> partial;
    DevBuf<GmmState> state;
    hipEvent_t ev[2] = {};                         // around the EM loop (garlic_gmm_fit_info)
    size_t bytes() const { return (stage.cap + partial.cap) * sizeof(double) + state.cap * sizeof(GmmState); }
    void release()
    {
        stage.release(); partial.release(); state.release();
        for (auto &e : ev) {
            if (e) (void)hipEventDestroy(e);
            e = nullptr;
        }
    }
    ~GmmScratch() { release(); }
};

// what garlic_bgzf_inflate and garlic_text_lines keep between calls (bgzf_kernels.hpp): the compressed bytes of a host-buffer
// call, both offset lists and the statuses; the tile counts, the lines, their heads and the result
struct BgzfScratch {
    DevBuf<uint8_t> comp, heads;
    DevBuf<int64_t> offsets, lines;
    DevBuf<int32_t> status, tiles;
    DevBuf<TextLinesResult> res;
    void release() { comp.release(); heads.release(); offsets.release(); lines.release(); status.release(); tiles.release(); res.release(); }
};

// lod(), src/garlic-roh.cpp:355-386.  Host arithmetic, host libm: identical to the reference.
double host_lod(int genotype, double freq, double error)
{
    double autozygous = 1, nonAutozygous = 1;
    if (freq == 0 || freq == 1) {
    } else if (genotype == 0) {
        nonAutozygous = (1 - freq) * (1 - freq);
        autozygous = (1 - error) * (1 - freq) + error * nonAutozygous;
    } else if (genotype == 1) {
        nonAutozygous = 2 * (freq) * (1 - freq);
        autozygous = error * nonAutozygous;
    } else if (genotype == 2) {
        nonAutozygous = (freq) * (freq);
        autozygous = (1 - error) * (freq) + error * nonAutozygous;
    }
    return log10(autozygous / nonAutozygous);
}

// most negative finite entry of a term table (0 if none is negative)
double min_finite(const double *x, size_t n)
{
    double m = 0.0;
    for (size_t i = 0; i < n; i++)
        if (x[i] < m && x[i] > -1.7976931348623157e308) m = x[i];
    return m;
}

template <class F> void parallel_for(int64_t n, int64_t grain, F f)
{
    unsigned hw = std::thread::hardware_concurrency();
    int nt = (int)std::min<int64_t>(std::min<unsigned>(hw ? hw : 1, 16), (n + grain - 1) / grain);
    if (nt <= 1) { f(0, n); return; }
    std::vector<std::thread> th;
    for (int t = 0; t < nt; t++)
        th.emplace_back([=] { f(n * t / nt, n * (t + 1) / nt); });
    for (auto &x : th) x.join();
}

} // namespace

struct garlic_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    bool own_stream = false;
    hipEvent_t ev_begin = nullptr, ev_end = nullptr;
    bool async_device = false;   // garlic_ctx_set_async
    int n_cu = 256;              // compute units of the device (persistent kernels: one or a few workgroups per CU)
    // the dominant kernel of the last HIST calls, one event pair each (asynchronous passes are
    // timed without being waited for one by one): garlic_recent_kernel_ms
    static constexpr int HIST = 32;
    hipEvent_t hist0[HIST] = {}, hist1[HIST] = {};
    int64_t n_calls = 0;
    // glibc's log table on the device (tgls_math.hpp) and the verdict of the start-up comparison of
    // the device's log10 with the host's: 0 not run yet, 1 identical on every probe, -1 differs
    DevBuf<double> d_logtab;
    int log10_state = 0;
    // garlic_feed_sort: its scratch, and what garlic_feed_sort_info reports (the last sort, a feed call's included)
    FeedSortScratch fs;
    int32_t fs_run = 0, fs_skipped = 0;
    int64_t fs_scratch_bytes = 0;
    // garlic_feed_kde and garlic_feed_kde_multi: their scratch, and what garlic_feed_kde_info and garlic_feed_kde_multi_info
    // report (the last single call and the last multi-feed call, each on its own)
    KdeMultiScratch kdem;
    KdeInfo kde_info, kdem_info;
    // garlic_gmm_fit: its scratch, and what garlic_gmm_fit_info reports
    GmmScratch gmm;
    int64_t gmm_blocks = 0;
    float gmm_em_ms = 0.f;
    // garlic_bgzf_inflate and garlic_text_lines: their scratch
    BgzfScratch bgzf;
};

static int score_alloc(garlic_ctx *ctx, size_t bytes, void **out);   // pooled score memory (below)
static int score_free(garlic_ctx *ctx, void *ptr);

// per-call scratch from the score pool (freed buffers stay mapped there: the next call's request costs no hipMalloc)
template <class T> struct PoolBuf : NoCopy {
    T *p = nullptr;
    garlic_ctx *ctx = nullptr;
    ~PoolBuf() { release(); }
    int reserve(garlic_ctx *c, size_t n)
    {
        release();
        void *q = nullptr;
        const int rc = score_alloc(c, std::max<size_t>(n, 1) * sizeof(T), &q);
        if (rc) return rc;
        p = (T *)q;
        ctx = c;
        return GARLIC_OK;
    }
    void release()
    {
        if (p) (void)score_free(ctx, p);
        p = nullptr;
    }
};


struct garlic_panel {
    garlic_ctx *ctx = nullptr;
    int32_t nchr = 0;
    int32_t nind = 0;
    int64_t nloci = 0;
    int64_t nind_pad = 0;
    int64_t nwordrows = 0;
    std::vector<int32_t> chr_nloci;
    std::vector<int64_t> chr_off; // nchr + 1
    // host copies of the small per-SNP inputs
    std::vector<int32_t> pos, cs, ce;
    std::vector<double> gpos, freq;
    bool have_map = false, have_freq = false, have_geno = false, have_gpos = false;
    // device state
    DevBuf<uint32_t> d_packed;
    DevBuf<int32_t> d_pos, d_cs, d_ce;
    DevBuf<int64_t> d_chr_off;
    DevBuf<double> d_tab;
    bool tab_valid = false;
    double tab_error = 0;
    double tab_min = 0, tabgl_min = 0, glterms_min = 0;   // most negative finite term (lod_exact_needed)
    bool tab_all_finite = false;                   // no infinite or NaN term (--error 0, a NaN frequency): every scored window is finite
    // segment boundaries (global loci, ascending), cached per max_gap
    bool seg_valid = false;
    int32_t seg_max_gap = 0;
    std::vector<int64_t> boundaries;
    DevBuf<int32_t> d_blk_counts, d_blk_offsets, d_total;
    DevBuf<int64_t> d_boundaries;
    // per-call scratch
    DevBuf<ChainItem> d_items;
    DevBuf<FeedItem> d_feed_items;                 // thinned feed: (run, FEED_G blocks) items of lod_feed_kernel
    DevBuf<FillItem> d_fill;
    DevBuf<int32_t> d_counter;
    DevBuf<ChrDev> d_chrs;
    DevBuf<int16_t> d_stage16;
    DevBuf<int32_t> d_bed_word_rows;               // garlic_panel_set_genotypes_bed: the file rows of every 16-locus word of the call
    DevBuf<int64_t> d_row_counts;
    // TGLS: dictionary-coded per-genotype error probabilities
    bool have_gl = false;
    std::vector<double> gl_values;                 // code -> error probability
    std::unordered_map<uint64_t, int> gl_code;     // bit pattern -> code
    DevBuf<uint8_t> d_codes;                       // [GOFF+nloci+pad][nind_pad]
    DevBuf<double> d_tabgl;
    bool tabgl_valid = false;
    DevBuf<double> d_glterms;                      // TGLS term matrix [blk][GOFF+nloci+pad][64]
    bool glterms_valid = false, glterms_scaled = false;   // scaled: holds (term * nomut) * norec of (glterms_M, glterms_mu)
    int32_t glterms_M = 0;
    double glterms_mu = 0.0;
    // ... or, under garlic_panel_set_tgls_term_budget, two slab buffers [blk - b0][GOFF+nloci+pad][64] that every use_gl call
    // fills and reads slab by slab (for_each_tgls_slab) -- raw terms for the unweighted chains, scaled ones for the weighted
    // kernels, in the same two buffers: slab k + 1 is built on slab_stream while the kernels of slab k run on the context's
    // stream, ordered by the events alone
    int64_t terms_budget = 0;                      // 0: whole matrix or none; > 0: bytes; -1: from the free memory
    DevBuf<double> d_slab[2];
    hipStream_t slab_stream = nullptr;
    hipEvent_t ev_slab_begin = nullptr, ev_slab_built[2] = {}, ev_slab_read[2] = {};
    DevBuf<int32_t> d_slab_queues;                 // one queue-head pair per slab
    int32_t last_slab_blocks = 0, last_n_slabs = 0;   // garlic_panel_tgls_terms_info

    int tabgl_ncodes = 0;
    // TGLS, continuous likelihoods (more distinct values than the dictionary holds): the error
    // probabilities themselves, in the term matrix's layout, and lod() on the device
    bool gl_cont = false;
    DevBuf<double> d_glval;                        // [blk][GOFF+nloci+pad][64]; empty once converted in place
    bool gl_vals_dropped = false;                  // d_glterms owns what was d_glval: terms cannot be rebuilt
    bool gl_cover_required = false;                // after a restart of the upload: every locus must come again
    std::vector<uint8_t> gl_cover;                 // loci uploaded since then
    DevBuf<double> d_freq;                         // [GOFF+nloci+pad], pad rows 0
    bool dfreq_valid = false;
    int gl_terms_by = 0;                           // who built the current terms: 1 device log10, 2 host libm
    int slab_terms_by = 0;                         // 16-bit codes: who built the term slabs of the last call
    // wide_term_bound's part that needs the whole table and every frequency: recomputed after either changed
    mutable bool wide_bound_known = false;
    mutable double wide_bound_cached = 0;
    // TGLS, 16-bit dictionary (GARLIC_TGLS_DICTIONARY16; tgls_wide_kernel.hpp): gl_values / gl_code hold up to 65,536 values,
    // the codes sit in the term matrix's layout and are never overwritten; d_codes / d_tabgl are empty
    bool gl_wide = false;
    DevBuf<uint16_t> d_codes16;                    // [blk][GOFF+nloci+pad][64]
    DevBuf<double> d_values16;                     // the value table, GL_WIDE_MAX doubles
    bool values16_valid = false;
    // wLOD
    bool have_ld = false, wlod_use_gl = false, rld_valid = false;
    int32_t last_chain_kind = 0;                   // garlic_panel_chain_kind
    int32_t last_feed_form = GARLIC_FEED_FROM_SCORES;   // garlic_lod_feed_info
    int64_t last_feed_doubles = 0;
    int32_t ld_winsize = 0;
    // garlic_panel_compute_ld_multi / garlic_ld_finish_multi: the weights of the other installed sizes (d_skew holds those
    // of ld_winsize, the size in use; select_ld swaps).  group: the pass of the multi call that made the set, -1: none
    struct LdSet {
        int32_t W = 0, group = -1;
        DevBuf<double> skew;
    };
    std::vector<std::unique_ptr<LdSet>> ld_sets;
    int32_t ld_group = -1;
    int32_t ld_pair_passes = 0, ld_sum_passes = 0; // of the last multi call (garlic_panel_ld_info)
    // the form of the last LD call (garlic_panel_ld_form_info); pair < 0: no LD call yet
    struct { int32_t pair = -1, sum = 0, fused = 0, phased = 0; } ld_last;
    DevBuf<double> d_rld, d_decay, d_stage64;
    DevBuf<uint64_t> d_phase;                      // HapData::firstCopy as bit planes [blk][nloci] (--phased LD)
    uint64_t geno_epoch = 0;                       // bumped by every genotype upload (LD plane cache)
    CovBits cov_pending{nullptr, nullptr, 0.0};    // set by garlic_roh_coverage_fused around a score call: bits, not scores
    bool cov_written = false;                      // ... and a kernel that writes bits took the call
    bool have_phase = false;
    // scratch of the LD-weight kernels, kept between calls (window-size sweeps): at 10M SNPs the six
    // 8-GB allocations and frees of a call cost 9x its kernels.  garlic_panel_release_scratch drops it.
    struct {
        DevBuf<uint64_t> sub, m, h, o;
        DevBuf<int32_t> loc, pair, loc_planes;
        DevBuf<double> hf, fwd, bwd, ld;
        DevBuf<LdSumChr> sum_chrs;
        DevBuf<LdPairChr> pair_chrs;
        DevBuf<LdMultiChr> multi_chrs;
        // the bit planes (and the per-SNP counts made with them) depend on the genotypes and the LD subsample only, not
        // on the window size: kept across calls (--winsize-multi with --weighted: 3.5 of a call's 32 ms at 10M x 1250)
        uint64_t planes_key = 0;
        bool planes_valid = false;
        void release()
        {
            sub.release(); m.release(); h.release(); o.release(); loc.release(); pair.release(); loc_planes.release();
            hf.release(); fwd.release(); bwd.release(); ld.release(); sum_chrs.release(); pair_chrs.release();
            multi_chrs.release();
            planes_valid = false;
        }
    } lds;
    // tuned wLOD path: skewed reciprocal weights, per-SNP score rows, window mask, tile index
    DevBuf<double> d_skew, d_wtab;
    DevBuf<uint8_t> d_valid;
    DevBuf<int2> d_tiles, d_segs;        // wLOD work lists: 32-window tiles; WSM_T-window segments (narrow windows)
    DevBuf<WlodStrip> d_strips;
    DevBuf<int32_t> d_feed_blocks;       // wlod_feed_kernel: the 64-individual blocks in play
    std::vector<double> h_tab, h_decay;            // host copies the score rows are built from
    bool wtab_valid = false;
    double wtab_error = 0.0, wtab_mu = 0.0;
    int32_t wtab_M = 0;
    int64_t wtab_rows = 0;
    bool decay_valid = false;
    int32_t decay_M = 0;
    double decay_mu = 0;
    // full-score scratch of the host-output and feed calls: pooled score memory, for big unweighted panels chosen by
    // placement at first use (garlic_panel_alloc_scores) -- a caller that hands over host buffers cannot do that itself
    struct ScoreBuf {
        double *p = nullptr;
        size_t cap = 0;
        garlic_ctx *ctx = nullptr;
        int reserve(garlic_ctx *c, size_t n)
        {
            if (n <= cap) return GARLIC_OK;
            release();
            void *q = nullptr;
            int rc = score_alloc(c, n * sizeof(double), &q);
            if (rc) return rc;
            p = (double *)q; cap = n; ctx = c;
            return GARLIC_OK;
        }
        void adopt(garlic_ctx *c, void *q, size_t n) { release(); p = (double *)q; cap = n; ctx = c; }
        void release()
        {
            if (p) (void)score_free(ctx, p);
            p = nullptr; cap = 0;
        }
    } d_out;
    bool placing = false;                          // inside the placement probe of d_out
    DevBuf<double> d_feed;
    int32_t feed_order = GARLIC_FEED_ORDER_REFERENCE;   // garlic_panel_set_feed_order
    FeedSortScratch fs;                            // ... SORTED: the sorter's scratch of the single-size feed calls
    // garlic_lod_kde, garlic_lod_kde_multi: set around their feed call -- every size's feed is sorted and stays on the device,
    // where and how many is noted here, one entry per window size of the call.  A size that goes through feed_single leaves
    // its feed in the panel's scratch (d_feed / fs), which the next size overwrites: `at` says which entry it is, and with
    // to_slot the feed is moved into that size's FeedSlot buffer before feed_single returns.
    struct FeedSink {
        struct Entry { const double *data = nullptr; int64_t n = 0; };
        std::vector<Entry> size;
        int32_t at = 0;
        bool to_slot = false;
        explicit FeedSink(int32_t n_sizes = 1) : size((size_t)n_sizes) {}
    } *feed_sink = nullptr;
    // garlic_lod_kde_part: a part borrows the feed from the scratch above.  Every call that may write that scratch (scores,
    // a feed, garlic_panel_release_scratch, the panel's end) moves the count on; a part whose count is behind is stale.
    std::shared_ptr<uint64_t> scratch_gen = std::make_shared<uint64_t>(0);
    // garlic_lod_feed_multi: one set of scratch and one stream per window size of the call, kept for the next call
    struct FeedSlot {
        hipStream_t stream = nullptr;
        hipEvent_t ev0 = nullptr, ev1 = nullptr;
        DevBuf<FeedItem> items;
        DevBuf<ChrDev> chrs;
        DevBuf<int32_t> counter;
        DevBuf<int64_t> row_counts;
        DevBuf<double> out, feed;
        FeedSortScratch fs;
    };
    std::vector<FeedSlot *> feed_slots;
    // garlic_lod_feed_multi_tgls: work lists of all groups, the sizes' ChrDev tables (by size; by group and place in it), one
    // queue-head pair per chain launch; what garlic_lod_feed_multi_info reports
    DevBuf<ChainItem> d_multi_items;
    DevBuf<ChrDev> d_multi_chrs, d_multi_gchrs;
    DevBuf<int32_t> d_multi_queues;
    std::vector<int32_t> multi_forms, multi_groups;
    int32_t multi_chain_launches = 0, multi_term_builds = 0;
    garlic_call_stats stats{};
    bool stats_pending = false;                    // event times of the last call not read yet
    bool stats_one_kernel = false;                 // ... and that call was one kernel between the pair of stats_slot, nothing else recorded
    int stats_slot = 0;                            // the context's event pair that brackets its dominant kernel
    int64_t n_stall_reruns = 0;                    // garlic_call_stats::n_stall_reruns as last read from the device
    bool reruns_stale = false;                     // a strip launch since (launch_wlod): the device's count may have moved
    int64_t n_count_timeouts = 0;                  // garlic_call_stats::n_count_timeouts
    struct Placement { int32_t drawn = 0, rounds = 0; float best_ms = 0, median_ms = 0, worst_ms = 0, target_ms = 0; int32_t reached = 0; };
    Placement placement;                           // the last garlic_panel_alloc_scores on this panel
    // work list of the last call, still on the device: repeated calls with the same arguments
    // (bench steps, window-size sweeps coming back to a size) skip planning and uploads
    struct PlanKey {              // what a plan depends on: compared and stored whole
        int mode = -1;
        int32_t W = 0, max_gap = 0, ind_begin = 0, ind_count = 0, pitch_align = 0, thin_step = 0;
        uint64_t blocks_hash = 0;                  // 0: every 64-individual block; else a hash of the block subset
        bool wlod_tuned = false, wlod_strip = false, feed_kernel = false;
        int32_t slab_blocks = 0;                   // TGLS term slabs: the item list is one list per slab
        auto tie() const { return std::tie(mode, W, max_gap, ind_begin, ind_count, pitch_align, thin_step, blocks_hash, wlod_tuned, wlod_strip, feed_kernel, slab_blocks); }
        bool operator==(const PlanKey &o) const { return tie() == o.tie(); }
    };
    struct Plan {
        bool valid = false;
        PlanKey key;
        size_t n_items = 0, n_fill = 0, n_feed_items = 0;
        int feed_per_cu = 1;      // persistent workgroups per CU the feed kernel of this plan is launched with (feed_grid)
        int32_t n_tiles = 0, n_segs = 0, n_strips = 0, n_feed_blocks = 0;
        int64_t n_runs = 0, n_valid = 0;
        // panel blocks [b0, b1); its items: [item0, item0 + n_items); wlod_feed: its blocks in play, [fb0, fb0 + n_fb) of d_feed_blocks
        struct Slab { int32_t b0, b1; size_t item0, n_items; int32_t fb0 = 0, n_fb = 0; };
        std::vector<Slab> slabs;
    } plan;
};

static bool select_ld(garlic_panel *p, int32_t winsize);   // makes the installed LD weights of winsize the ones in use
static int ensure_rld(garlic_panel *p);   // plain reciprocals of the LD weights, made when the generic wLOD kernel needs them

// ---- Score buffers.  Where 8 GB of scores sit in VRAM decides between two speeds of lod_chain_kernel at 1M SNPs x
// 1000 individuals (1.36 and 1.62 ms: DESIGN.md section 4, "placement"); a virtual range backed by physical chunks
// of its own (HIP virtual memory management, 1 GB each) was in the fast mode more often than plain hipMalloc
// memory.  Falls back to hipMalloc where the driver has no virtual memory management.
//
// Freed buffers stay MAPPED in a pool and are handed out again for requests they fit: measured on ROCm 7.2 / MI355X,
// a virtual range that is unmapped and given new physical memory loses part of the first kernel's writes
// (tools/exp/alloc_dbg.py, tools/exp/vmm_remap_repro.hip); a buffer that keeps its mapping has nothing to lose, and a
// caller that allocates per sweep reuses the same few ranges instead of growing its address space.  The pool is
// capped (GARLIC_ALLOC_POOL_GB, default a quarter of the device memory); what does not fit is unmapped and its
// physical memory released, its range stays reserved (never mapped again: address space only, reported by
// garlic_device_alloc_stats).
struct ScoreAlloc {
    void *ptr;
    size_t size;
    std::vector<hipMemGenericAllocationHandle_t> handles;
    int device;
    bool pooled;          // free, still mapped
    uint64_t stamp;       // when it was pooled (oldest goes first)
};
static std::mutex g_score_mutex;
static std::vector<ScoreAlloc> g_score_allocs;
static int64_t g_score_retired[16] = {};   // bytes of ranges kept reserved after their memory was released, per device
static uint64_t g_score_clock = 0;

static void release_score_alloc(ScoreAlloc &a, size_t mapped, bool keep_range)
{
    if (mapped) (void)hipMemUnmap(a.ptr, mapped);
    for (auto h : a.handles) (void)hipMemRelease(h);
    if (a.ptr && !keep_range) (void)hipMemAddressFree(a.ptr, a.size);
}

static int score_alloc(garlic_ctx *ctx, size_t bytes, void **out)
{
    *out = nullptr;
    int vmm = 0;
    (void)hipDeviceGetAttribute(&vmm, hipDeviceAttributeVirtualMemoryManagementSupported, ctx->device);
    if (vmm && !getenv("GARLIC_ALLOC_PLAIN")) {
        hipMemAllocationProp prop{};
        prop.type = hipMemAllocationTypePinned;
        prop.location.type = hipMemLocationTypeDevice;
        prop.location.id = ctx->device;
        size_t gran = 0;
        if (hipMemGetAllocationGranularity(&gran, &prop, hipMemAllocationGranularityRecommended) == hipSuccess && gran) {
            const size_t chunk = (((size_t)1 << 30) + gran - 1) / gran * gran;
            const size_t size = (bytes + gran - 1) / gran * gran;
            {   // a pooled buffer that fits without wasting more than an eighth
                std::lock_guard<std::mutex> lock(g_score_mutex);
                int pick = -1;
                for (size_t k = 0; k < g_score_allocs.size(); k++) {
                    const ScoreAlloc &a = g_score_allocs[k];
                    if (a.pooled && a.device == ctx->device && a.size >= size && a.size - size <= size / 8 &&
                        (pick < 0 || a.size < g_score_allocs[(size_t)pick].size))
                        pick = (int)k;
                }
                if (pick >= 0) {
                    g_score_allocs[(size_t)pick].pooled = false;
                    *out = g_score_allocs[(size_t)pick].ptr;
                    return GARLIC_OK;
                }
            }
            ScoreAlloc a{nullptr, size, {}, ctx->device, false, 0};
            size_t mapped = 0;
            bool ok = hipMemAddressReserve(&a.ptr, size, 0, nullptr, 0) == hipSuccess;
            for (size_t off = 0; ok && off < size; off += chunk) {
                const size_t n = std::min(chunk, size - off);
                hipMemGenericAllocationHandle_t h;
                ok = hipMemCreate(&h, n, &prop, 0) == hipSuccess;
                if (!ok) break;
                a.handles.push_back(h);
                ok = hipMemMap((char *)a.ptr + off, n, 0, h, 0) == hipSuccess;
                if (ok) mapped = off + n;
            }
            if (ok) {
                hipMemAccessDesc acc{};
                acc.location = prop.location;
                acc.flags = hipMemAccessFlagsProtReadWrite;
                ok = hipMemSetAccess(a.ptr, size, &acc, 1) == hipSuccess;
            }
            if (ok) {
                *out = a.ptr;
                std::lock_guard<std::mutex> lock(g_score_mutex);
                g_score_allocs.push_back(std::move(a));
                return GARLIC_OK;
            }
            release_score_alloc(a, mapped, mapped != 0);
            if (mapped != 0 && a.ptr) {      // (a partly mapped range stays reserved: garlic_device_alloc_stats counts it)
                std::lock_guard<std::mutex> lock(g_score_mutex);
                g_score_retired[ctx->device < 16 ? ctx->device : 15] += (int64_t)a.size;
            }
            (void)hipGetLastError();
            {   // out of device memory with buffers idle in the pool: give those back and try once more
                bool any = false;
                {
                    std::lock_guard<std::mutex> lock(g_score_mutex);
                    for (const ScoreAlloc &b : g_score_allocs) any = any || (b.pooled && b.device == ctx->device);
                }
                if (any) {
                    (void)score_pool_trim();
                    return score_alloc(ctx, bytes, out);
                }
            }
        }
    }
    HIP_TRY(hipMalloc(out, bytes));
    return GARLIC_OK;
}

namespace {
int score_pool_trim()
{
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return GARLIC_OK;
    (void)hipDeviceSynchronize();
    std::lock_guard<std::mutex> lock(g_score_mutex);
    for (size_t k = 0; k < g_score_allocs.size();) {
        ScoreAlloc &b = g_score_allocs[k];
        if (b.pooled && b.device == dev) {
            release_score_alloc(b, b.size, true);
            g_score_retired[dev < 16 ? dev : 15] += (int64_t)b.size;
            g_score_allocs.erase(g_score_allocs.begin() + (long)k);
        } else k++;
    }
    return GARLIC_OK;
}
}

static int score_free(garlic_ctx *ctx, void *ptr)
{
    {
        // (this device's work first, OUTSIDE the lock: one shard's release must not queue behind another device's kernels)
        bool ours = false;
        {
            std::lock_guard<std::mutex> lock(g_score_mutex);
            for (const ScoreAlloc &a : g_score_allocs) ours = ours || (a.ptr == ptr && !a.pooled);
        }
        if (ours) HIP_TRY(hipDeviceSynchronize());
        size_t total_mem = 0, free_mem = 0;
        if (ours) (void)hipMemGetInfo(&free_mem, &total_mem);
        std::lock_guard<std::mutex> lock(g_score_mutex);
        for (size_t k = 0; k < g_score_allocs.size(); k++)
            if (g_score_allocs[k].ptr == ptr && !g_score_allocs[k].pooled) {
                g_score_allocs[k].pooled = true;
                g_score_allocs[k].stamp = ++g_score_clock;
                // cap the pool: the oldest idle buffers give their memory back (their ranges stay reserved, unmapped for good)
                int64_t cap = (int64_t)(total_mem / 4);
                if (const char *e = getenv("GARLIC_ALLOC_POOL_GB")) cap = (int64_t)(atof(e) * 1073741824.0);
                for (;;) {
                    int64_t pooled = 0;
                    int oldest = -1;
                    for (size_t j = 0; j < g_score_allocs.size(); j++) {
                        const ScoreAlloc &a = g_score_allocs[j];
                        if (!a.pooled || a.device != ctx->device) continue;
                        pooled += (int64_t)a.size;
                        if (oldest < 0 || a.stamp < g_score_allocs[(size_t)oldest].stamp) oldest = (int)j;
                    }
                    if (pooled <= cap || oldest < 0) break;
                    ScoreAlloc &b = g_score_allocs[(size_t)oldest];
                    release_score_alloc(b, b.size, true);
                    g_score_retired[ctx->device < 16 ? ctx->device : 15] += (int64_t)b.size;
                    g_score_allocs.erase(g_score_allocs.begin() + oldest);
                }
                return GARLIC_OK;
            }
    }
    HIP_TRY(hipFree(ptr));
    return GARLIC_OK;
}

namespace {

int set_device(garlic_ctx *ctx)
{
    HIP_TRY(hipSetDevice(ctx->device));
    return GARLIC_OK;
}

// ---- segment boundaries on the device (integer scans), read back once per (map, max_gap)
int ensure_segments(garlic_panel *p, int32_t max_gap)
{
    if (p->seg_valid && p->seg_max_gap == max_gap) return GARLIC_OK;
    garlic_ctx *ctx = p->ctx;
    const int64_t per_block = (int64_t)SEG_BLOCK * SEG_ITEMS;
    const int nblocks = (int)((p->nloci + per_block - 1) / per_block);
    int rc;
    if ((rc = p->d_blk_counts.reserve(nblocks))) return rc;
    if ((rc = p->d_blk_offsets.reserve(nblocks))) return rc;
    if ((rc = p->d_total.reserve(1))) return rc;
    hipLaunchKernelGGL(seg_count_kernel, dim3(nblocks), dim3(SEG_BLOCK), 0, ctx->stream, p->d_pos.p,
                       p->d_chr_off.p, p->d_cs.p, p->d_ce.p, p->nchr, p->nloci, max_gap,
                       p->d_blk_counts.p);
    hipLaunchKernelGGL(seg_scan_kernel, dim3(1), dim3(WAVE), 0, ctx->stream, p->d_blk_counts.p,
                       nblocks, p->d_blk_offsets.p, p->d_total.p);
    int32_t total = 0;
    HIP_TRY(hipMemcpyAsync(&total, p->d_total.p, sizeof total, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    if (total < p->nchr) return fail(GARLIC_ERR_HIP, "segment scan returned %d boundaries", total);
    if ((rc = p->d_boundaries.reserve((size_t)total))) return rc;
    hipLaunchKernelGGL(seg_compact_kernel, dim3(nblocks), dim3(SEG_BLOCK), 0, ctx->stream,
                       p->d_pos.p, p->d_chr_off.p, p->d_cs.p, p->d_ce.p, p->nchr, p->nloci, max_gap,
                       p->d_blk_offsets.p, p->d_boundaries.p);
    p->boundaries.resize((size_t)total);
    HIP_TRY(hipMemcpyAsync(p->boundaries.data(), p->d_boundaries.p, sizeof(int64_t) * total,
                           hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    HIP_TRY(hipGetLastError());
    p->seg_valid = true;
    p->seg_max_gap = max_gap;
    return GARLIC_OK;
}

// ---- per-SNP term table {lod(0), lod(1), lod(2), lod(missing)=+0.0}, host libm
int ensure_term_table(garlic_panel *p, double error)
{
    if (p->tab_valid && memcmp(&p->tab_error, &error, sizeof error) == 0) return GARLIC_OK;
    const int64_t rows = GOFF + p->nloci + GPAD_BACK;
    std::vector<double> tab((size_t)rows * 4, 0.0);
    const double *freq = p->freq.data();
    double *t = tab.data() + (size_t)GOFF * 4;
    parallel_for(p->nloci, 1 << 16, [=](int64_t lo, int64_t hi) {
        for (int64_t l = lo; l < hi; l++) {
            t[l * 4 + 0] = host_lod(0, freq[l], error);
            t[l * 4 + 1] = host_lod(1, freq[l], error);
            t[l * 4 + 2] = host_lod(2, freq[l], error);
            t[l * 4 + 3] = host_lod(-9, freq[l], error);
        }
    });
    if (int rc = p->d_tab.put(tab, p->ctx->stream)) return rc;
    HIP_TRY(hipStreamSynchronize(p->ctx->stream));
    p->tab_valid = true;
    p->tab_error = error;
    p->tab_min = min_finite(tab.data(), tab.size());
    p->tab_all_finite = true;
    for (double x : tab)
        if (!std::isfinite(x)) { p->tab_all_finite = false; break; }
    p->h_tab.swap(tab);
    p->wtab_valid = false;
    return GARLIC_OK;
}

struct Layout {
    std::vector<int64_t> base, pitch;
    int64_t total = 0;
};

// thin_step > 0: the layout of the thinned score matrix (KDE feed) -- per chromosome
// ceil(nloci / thin_step) columns instead of nloci
Layout make_layout(const garlic_panel *p, int32_t pitch_align, int32_t nind_out, int32_t thin_step = 0)
{
    Layout L;
    L.base.resize(p->nchr);
    L.pitch.resize(p->nchr);
    int64_t off = 0;
    const int64_t al = std::max(1, pitch_align);
    // pitch_align >= 2: rows are also padded to a multiple of 64 individuals, so every wavefront
    // stores 64 full rows (the pad rows belong to the caller's buffer and are never read back)
    const int64_t rows = (pitch_align >= 2) ? ((int64_t)nind_out + 63) / 64 * 64 : nind_out;
    for (int c = 0; c < p->nchr; c++) {
        const int64_t cols = thin_step > 0 ? ((int64_t)p->chr_nloci[c] + thin_step - 1) / thin_step : p->chr_nloci[c];
        int64_t pitch = (cols + al - 1) / al * al;
        off = (off + al - 1) / al * al;
        L.base[c] = off;
        L.pitch[c] = pitch;
        off += pitch * rows;
    }
    L.total = off;
    return L;
}

struct Run {
    int32_t chr, a, b;
};

// run indices, longest run first (LPT); a stable sort: ties keep chromosome and position order, and the order reaches the device
std::vector<int> longest_first(const std::vector<Run> &runs)
{
    std::vector<int> order(runs.size());
    for (size_t i = 0; i < runs.size(); i++) order[i] = (int)i;
    std::stable_sort(order.begin(), order.end(), [&](int x, int y) { return (runs[x].b - runs[x].a) > (runs[y].b - runs[y].a); });
    return order;
}

// segments -> maximal runs of valid windows for one window size, and the MISSING stretches
void plan_runs(const garlic_panel *p, int32_t W, std::vector<Run> &runs, std::vector<FillItem> &fill,
               int64_t &n_valid)
{
    runs.clear();
    fill.clear();
    n_valid = 0;
    size_t k = 0;
    const size_t nb = p->boundaries.size();
    for (int c = 0; c < p->nchr; c++) {
        const int64_t c0 = p->chr_off[c], c1 = p->chr_off[c + 1];
        int32_t cursor = 0; // first chromosome-local window not yet accounted for
        while (k < nb && p->boundaries[k] < c1) {
            const int64_t s = p->boundaries[k];
            const int64_t e = (k + 1 < nb && p->boundaries[k + 1] < c1) ? p->boundaries[k + 1] : c1;
            k++;
            const int64_t len = e - s;
            if (len >= W) {
                Run r{c, (int32_t)(s - c0), (int32_t)(e - W - c0)};
                if (r.a > cursor) fill.push_back(FillItem{c, cursor, r.a, 0});
                runs.push_back(r);
                n_valid += r.b - r.a + 1;
                cursor = r.b + 1;
            }
        }
        const int32_t n = (int32_t)(c1 - c0);
        if (cursor < n) fill.push_back(FillItem{c, cursor, n, 0});
    }
}

enum Mode { MODE_LOD, MODE_LOD_GL, MODE_WLOD };

// internal (never returned through the ABI): launch_lod was asked for coverage bits (garlic_panel::cov_pending) by a shape
// only the score kernels take; garlic_roh_coverage_fused then computes the scores and counts from them
constexpr int GARLIC_INTERNAL_NO_BITS = -1001;
constexpr int GARLIC_INTERNAL_NO_SAMPLED = -1002;   // launch_lod: no kernel with thinned output (wlod_feed_kernel, tgls_feed_kernel) takes this call (feed_single: full scores)

// Work list of lod_feed_kernel: (run, FEED_G blocks) items, longest runs first (`order`); the runs within reach of
// the longest one run at raised issue priority: their length x one wave's pace is the kernel's critical path.
// blocks: per 64-individual block, 1 = score it (NULL: all nblk of them).
// col0[r]: column of run r's first sampled locus in its chromosome's rows of the sample matrix; < 0: the run holds
// no sampled locus, no item.
void build_feed_items(const std::vector<Run> &runs, const std::vector<int> &order, const std::vector<uint8_t> *blocks,
                      int nblk, const std::vector<int32_t> &col0, std::vector<FeedItem> &items)
{
    items.clear();
    std::vector<int> blk;
    for (int k = 0; k < nblk; k++)
        if (!blocks || (*blocks)[(size_t)k]) blk.push_back(k);
    const int longest = runs.empty() ? 0 : runs[order[0]].b - runs[order[0]].a + 1;
    for (size_t i = 0; i < order.size(); i++) {
        const Run &r = runs[order[i]];
        if (col0[(size_t)order[i]] < 0) continue;
        const int64_t len = r.b - r.a + 1;
        const int prio = (4 * len >= 3 * (int64_t)longest) ? 3 : (2 * len >= longest) ? 2 : (4 * len >= longest) ? 1 : 0;
        for (size_t k = 0; k < blk.size(); k += FEED_G) {
            FeedItem f{r.chr, r.a, r.b, prio, {-1, -1, -1, -1}, col0[(size_t)order[i]], {0, 0, 0}};
            for (size_t w = 0; w < FEED_G && k + w < blk.size(); w++) f.ind0[w] = blk[k + w] * WAVE;
            items.push_back(f);
        }
    }
}

// How many persistent workgroups of lod_feed_kernel per CU.  Not "as many as stay resident": the items are whole runs (a
// chain cannot be cut), a workgroup's pace depends on how many share its CU (measured, 5M x 5k and 2M x 10k: 52 cycles per
// window and wave alone, 80 with one neighbour, 109 with two -- a SIMD gives two chains 1.3 x and three 1.43 x the rate of
// one), and with about as many items as slots the last slots' long items finish alone on an idle chip.  C3 (880 items): three
// per CU 30.8 ms for the four sizes, two per CU 25.6; 2M x 10k (1760 shorter items): three 18.5, two 20.0.  So the launch
// is simulated -- the queue in its order, every CU sharing its pace among the workgroups it holds -- for each count
// that fits, and the shortest one taken.
static double feed_makespan(const std::vector<int32_t> &len, int n_cu, int per_cu)
{
    static const double pace[5] = {0.0, 52.0, 79.6, 109.0, 150.0};       // cycles per window and wave, k workgroups on the CU
    struct Cu { double t; int k; double rem[4]; };
    std::vector<Cu> cus((size_t)n_cu, Cu{0.0, 0, {0, 0, 0, 0}});
    size_t q = 0;
    for (int s = 0; s < per_cu; s++)
        for (int c = 0; c < n_cu && q < len.size(); c++) cus[(size_t)c].rem[cus[(size_t)c].k++] = (double)len[q++];
    typedef std::pair<double, int> Ev;     // (time of the CU's next completion, CU)
    std::priority_queue<Ev, std::vector<Ev>, std::greater<Ev>> heap;
    auto next_of = [&](const Cu &u) {
        double m = u.rem[0];
        for (int i = 1; i < u.k; i++) m = std::min(m, u.rem[i]);
        return u.t + m * pace[u.k];
    };
    for (int c = 0; c < n_cu; c++)
        if (cus[(size_t)c].k) heap.push(Ev(next_of(cus[(size_t)c]), c));
    double end = 0.0;
    while (!heap.empty()) {
        const Ev ev = heap.top();
        heap.pop();
        Cu &u = cus[(size_t)ev.second];
        const double adv = (ev.first - u.t) / pace[u.k];
        u.t = ev.first;
        end = std::max(end, u.t);
        int k = 0;
        for (int i = 0; i < u.k; i++) {
            const double r = u.rem[i] - adv;
            if (r > 0.5) u.rem[k++] = r;
            else if (q < len.size()) u.rem[k++] = (double)len[q++];     // the workgroup pulls the next item
        }
        u.k = k;
        if (k) heap.push(Ev(next_of(u), ev.second));
    }
    return end;
}

int feed_grid(garlic_ctx *ctx, const std::vector<FeedItem> &items, int *grid, int *per_cu_out)
{
    int per_cu = 0;
    HIP_TRY(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, (const void *)lod_feed_kernel, FEED_G * WAVE, 0));
    per_cu = std::max(1, std::min(per_cu, 16 / FEED_G));
    const size_t n_items = items.size();
    if (const char *e = getenv("GARLIC_FEED_PER_CU")) per_cu = std::max(1, atoi(e));
    else if (n_items > (size_t)ctx->n_cu && n_items <= (size_t)64 * ctx->n_cu * per_cu) {
        // (fewer items than CUs: one each; very many: whatever order they finish in, the chip stays full)
        std::vector<int32_t> len(n_items);
        for (size_t i = 0; i < n_items; i++) len[i] = items[i].b - items[i].a + 1 + 64;      // (+ an item's fixed costs)
        int best = per_cu;
        double best_t = feed_makespan(len, ctx->n_cu, per_cu);
        for (int k = per_cu - 1; k >= 1; k--) {
            const double t = feed_makespan(len, ctx->n_cu, k);
            if (t < 0.98 * best_t) { best_t = t; best = k; }
        }
        per_cu = best;
    }
    if (per_cu_out) *per_cu_out = per_cu;
    *grid = (int)std::min<size_t>(n_items, (size_t)ctx->n_cu * per_cu);
    return GARLIC_OK;
}

// The reference tests "previous window has no score" by value (garlic-roh.cpp:79); the tuned chains by
// position.  They agree unless a scored window sums to exactly -9999.0, which needs W terms that can add
// up to it: impossible while W * (most negative term) stays above -9999 (a margin covers the rounding of
// the sums).  Otherwise the exact kernel runs (lod_chain_exact_kernel).  Tables / terms must be current.
// 16-bit dictionary: a lower bound of every finite term that is known BEFORE any term is built -- under term slabs the chain
// kind is decided before the first slab exists.  With every table value e in (0, 1] and every frequency f in [0, 1]
// (f = 0, 1: term +0.0) the homozygous quotients are (1 - e) / (1 - f) + e >= 1 and (1 - e) / f + e >= 1 up to a few roundings
// (terms >= about -1e-15), and the heterozygous quotient is (e * non) / non = e up to one rounding: term = log10(e) within
// an ulp or two.  So: the host's log10 of the smallest table value, minus 1e-6 (a million times the rounding at stake, and
// at most 0.004 over the widest window).  Any value outside (0, 1], any frequency outside {0} and [1e-150, 1] (reachable through
// --freq-file; below 1e-150 the genotype probabilities f * f and 2 f (1 - f) can be subnormal, where e * non rounds in units of
// 2^-1074 and the quotient is no longer e), a NaN among either: no bound -- the scan always runs.  It errs towards kind 1 only.  Where a whole raw matrix
// has been built its measured minimum is taken in as well (it can only lower the bound).
double wide_term_bound(const garlic_panel *p)
{
    if (!p->wide_bound_known) {      // set_freq and every change of the value table clear the flag
        double vmin = 1.0;
        bool bounded = true;
        for (double v : p->gl_values) {
            if (!(v > 0.0 && v <= 1.0)) bounded = false;
            vmin = std::min(vmin, v);
        }
        for (double f : p->freq)
            if (!(f == 0.0 || (f >= 1e-150 && f <= 1.0))) bounded = false;
        p->wide_bound_cached = bounded ? log10(vmin) - 1e-6 : -HUGE_VAL;
        p->wide_bound_known = true;
    }
    double bound = p->wide_bound_cached;
    if (p->glterms_valid && p->d_glterms.p && p->gl_terms_by) bound = std::min(bound, p->glterms_min);
    return bound;
}

bool lod_exact_needed(const garlic_panel *p, Mode mode, int32_t W)
{
    if (getenv("GARLIC_EXACT_CHAIN") || getenv("GARLIC_EXACT_CHAIN_ONLY")) return true;
    const double tmin = mode == MODE_LOD ? p->tab_min : p->gl_wide ? wide_term_bound(p) : (p->gl_cont ? p->glterms_min : p->tabgl_min);
    return (double)W * tmin <= -9990.0;
}

// ---- TGLS: term table per (SNP, error code, genotype), host libm
int ensure_gl_table(garlic_panel *p)
{
    const int ncodes = (int)p->gl_values.size();
    if (ncodes < 1) return fail(GARLIC_ERR_STATE, "use_gl set but no genotype likelihoods were given");
    if (p->tabgl_valid && p->tabgl_ncodes == ncodes) return GARLIC_OK;
    const int64_t rows = GOFF + p->nloci + GPAD_BACK;
    std::vector<double> tab((size_t)rows * ncodes * 4, 0.0);
    const double *freq = p->freq.data();
    const double *val = p->gl_values.data();
    double *t = tab.data() + (size_t)GOFF * ncodes * 4;
    parallel_for(p->nloci, 1 << 12, [=](int64_t lo, int64_t hi) {
        for (int64_t l = lo; l < hi; l++)
            for (int c = 0; c < ncodes; c++) {
                double *e = t + ((size_t)l * ncodes + c) * 4;
                e[0] = host_lod(0, freq[l], val[c]);
                e[1] = host_lod(1, freq[l], val[c]);
                e[2] = host_lod(2, freq[l], val[c]);
                e[3] = host_lod(-9, freq[l], val[c]);
            }
    });
    if (int rc = p->d_tabgl.put(tab, p->ctx->stream)) return rc;
    HIP_TRY(hipStreamSynchronize(p->ctx->stream));
    p->tabgl_valid = true;
    p->tabgl_ncodes = ncodes;
    p->tabgl_min = min_finite(tab.data(), tab.size());
    p->glterms_valid = false;
    return GARLIC_OK;
}

// ---- TGLS with continuous likelihoods: glibc's log table on the device, checked against the host
// Probes: both binades __ieee754_log10 hands to log (random mantissas), a dense band around 1 (the
// polynomial branch and its borders), every table cell's ends, random exponents, subnormals and the
// special values.  One kernel, ~2e5 values; the verdict is kept with the context.
int ensure_log10(garlic_ctx *ctx)
{
    if (ctx->log10_state != 0) return GARLIC_OK;
    static const double tab[256] = GLIBC_LOG_TAB;
    int rc;
    if ((rc = ctx->d_logtab.reserve(256))) return rc;
    HIP_TRY(hipMemcpyAsync(ctx->d_logtab.p, tab, sizeof tab, hipMemcpyHostToDevice, ctx->stream));
    std::vector<double> in;
    uint64_t st = 0x9E3779B97F4A7C15ull;
    auto next = [&]() { st ^= st << 13; st ^= st >> 7; st ^= st << 17; return st; };
    auto bits = [](uint64_t u) { double d; memcpy(&d, &u, sizeof d); return d; };
    for (double x : {0.0, -0.0, 1.0, -1.0, (double)INFINITY, -(double)INFINITY, (double)NAN, 5e-324, 2.2250738585072014e-308,
                     1.7976931348623157e308, 0.5, 2.0, 10.0, 1e-16})
        in.push_back(x);
    in.push_back(bits(0xFFF8000000000000ull));
    in.push_back(bits(0x7FF0000000000001ull));
    for (uint64_t c : {0x3FEE000000000000ull, 0x3FF1090000000000ull, 0x3FF0000000000000ull, 0x3FE6000000000000ull,
                       0x3FF6000000000000ull, 0x0010000000000000ull})
        for (int d = -16; d <= 16; d++) in.push_back(bits(c + (uint64_t)(int64_t)d));
    for (int cell = 0; cell < 128; cell++)
        for (uint64_t top : {0x3FE0000000000000ull, 0x3FF0000000000000ull})
            for (int d = -2; d <= 2; d++) in.push_back(bits(top + ((uint64_t)cell << 45) + (uint64_t)(int64_t)d));
    for (int k = 0; k < 40000; k++) {
        const uint64_t m = next() & 0x000FFFFFFFFFFFFFull;
        in.push_back(bits(0x3FE0000000000000ull | m));
        in.push_back(bits(0x3FF0000000000000ull | m));
        in.push_back(bits((0x3FF0000000000000ull - (1ull << 49)) + (next() % (3ull << 49))));
        in.push_back(bits(((next() % 2046 + 1) << 52) | m));
        if ((k & 63) == 0) in.push_back(bits(m));
    }
    const int64_t n = (int64_t)in.size();
    DevBuf<double> d_in, d_out;
    if ((rc = d_in.reserve((size_t)n)) || (rc = d_out.reserve((size_t)n))) return rc;
    std::vector<double> out((size_t)n);
    hipError_t e = hipMemcpyAsync(d_in.p, in.data(), sizeof(double) * n, hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(log10_probe_kernel, dim3(256), dim3(256), 0, ctx->stream, d_in.p, ctx->d_logtab.p, n, d_out.p);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(out.data(), d_out.p, sizeof(double) * n, hipMemcpyDeviceToHost, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess) return fail(GARLIC_ERR_HIP, "log10 probe: %s", hipGetErrorString(e));
    int64_t bad = 0;
    for (int64_t i = 0; i < n; i++) {
        const double want = log10(in[(size_t)i]);
        if (memcmp(&want, &out[(size_t)i], sizeof want) != 0) bad++;
    }
    ctx->log10_state = bad == 0 ? 1 : -1;
    if (bad)
        fprintf(stderr, "libgarlic_hip: the host's log10 is not the glibc 2.35 FMA variant the device restates "
                        "(%lld of %lld probes differ); continuous TGLS terms will be computed on the host\n",
                (long long)bad, (long long)n);
    return GARLIC_OK;
}

// allele frequencies on the device, in padded row order (pad rows 0 -> term +0.0)
int ensure_dfreq(garlic_panel *p)
{
    if (p->dfreq_valid) return GARLIC_OK;
    const int64_t rows = GOFF + p->nloci + GPAD_BACK;
    std::vector<double> f((size_t)rows, 0.0);
    memcpy(f.data() + GOFF, p->freq.data(), sizeof(double) * (size_t)p->nloci);
    if (int rc = p->d_freq.put(f, p->ctx->stream)) return rc;
    HIP_TRY(hipStreamSynchronize(p->ctx->stream));
    p->dfreq_valid = true;
    return GARLIC_OK;
}

void release_tgls_slabs(garlic_panel *p);
void dict_clear(garlic_panel *p);     // the likelihood dictionary, emptied (with the other uploads' shared steps, below)

// ---- 16-bit dictionary.  The value table on the device (its unused tail 0.0)
int ensure_values16(garlic_panel *p)
{
    if (p->values16_valid) return GARLIC_OK;
    int rc;
    if ((rc = p->d_values16.reserve(GL_WIDE_MAX))) return rc;
    std::vector<double> v(GL_WIDE_MAX, 0.0);
    std::copy(p->gl_values.begin(), p->gl_values.end(), v.begin());
    HIP_TRY(hipMemcpyAsync(p->d_values16.p, v.data(), sizeof(double) * GL_WIDE_MAX, hipMemcpyHostToDevice, p->ctx->stream));
    HIP_TRY(hipStreamSynchronize(p->ctx->stream));
    p->values16_valid = true;
    return GARLIC_OK;
}

// A panel without likelihoods, or one with one-byte codes, takes 16-bit codes from here on: what has been coded is widened
// (the code numbers stay), the per-SNP term table and the terms made from it go.
int switch_to_wide(garlic_panel *p)
{
    if (p->gl_wide || p->gl_cont) return GARLIC_OK;
    const int64_t rows = GOFF + p->nloci + GPAD_BACK;
    const size_t n = (size_t)rows * p->nind_pad;
    hipStream_t s = p->ctx->stream;
    int rc;
    HIP_TRY(hipStreamSynchronize(s));
    if ((rc = p->d_codes16.reserve(n))) return rc;
    if (p->d_codes.p) {
        hipLaunchKernelGGL(gl_widen_kernel, dim3(4096), dim3(256), 0, s, p->d_codes.p, p->nind_pad, rows, p->d_codes16.p);
        HIP_TRY(hipGetLastError());
    } else
        HIP_TRY(hipMemsetAsync(p->d_codes16.p, 0, sizeof(uint16_t) * n, s));
    HIP_TRY(hipStreamSynchronize(s));
    p->d_codes.release();
    p->d_tabgl.release();
    p->tabgl_valid = false;
    p->d_glterms.release();
    release_tgls_slabs(p);
    p->glterms_valid = false;
    p->values16_valid = false;
    p->gl_wide = true;
    return GARLIC_OK;
}

// The dictionary is full (or the caller's values are continuous from the start): from here on the
// panel keeps the error probabilities themselves.  What has been coded so far is decoded.
int switch_to_continuous(garlic_panel *p)
{
    if (p->gl_cont) return GARLIC_OK;
    const int64_t rows = GOFF + p->nloci + GPAD_BACK;
    const size_t n = (size_t)rows * p->nind_pad;
    hipStream_t s = p->ctx->stream;
    int rc;
    HIP_TRY(hipStreamSynchronize(s));
    p->d_glterms.release();          // terms of the dictionary the panel leaves behind
    p->d_slab[0].release();          // ... and its term slabs (continuous likelihoods have no budget)
    p->d_slab[1].release();
    p->glterms_valid = false;
    if ((rc = p->d_glval.reserve(n))) return rc;
    if (p->gl_wide) {      // 16-bit codes and values share the layout: decoded element for element
        if ((rc = ensure_values16(p))) return rc;
        hipLaunchKernelGGL(gl_decode16_kernel, dim3(4096), dim3(256), 0, s, p->d_codes16.p, p->d_values16.p,
                           (int32_t)p->gl_values.size(), (int64_t)n, p->d_glval.p);
        hipError_t e = hipGetLastError();
        if (e == hipSuccess) e = hipStreamSynchronize(s);
        if (e != hipSuccess) return fail(GARLIC_ERR_HIP, "set_gl: %s", hipGetErrorString(e));
    } else if (p->d_codes.p && !p->gl_values.empty()) {
        std::vector<double> dict(GL_DICT_MAX, 0.0);
        std::copy(p->gl_values.begin(), p->gl_values.end(), dict.begin());
        DevBuf<double> d_dict;
        if ((rc = d_dict.reserve(GL_DICT_MAX))) return rc;
        hipError_t e = hipMemcpyAsync(d_dict.p, dict.data(), sizeof(double) * GL_DICT_MAX, hipMemcpyHostToDevice, s);
        if (e == hipSuccess) {
            hipLaunchKernelGGL(gl_decode_kernel, dim3(4096), dim3(256), 0, s, p->d_codes.p, d_dict.p, p->nind_pad, rows,
                               p->d_glval.p);
            e = hipGetLastError();
        }
        if (e == hipSuccess) e = hipStreamSynchronize(s);
        if (e != hipSuccess) return fail(GARLIC_ERR_HIP, "set_gl: %s", hipGetErrorString(e));
    } else {
        HIP_TRY(hipMemsetAsync(p->d_glval.p, 0, sizeof(double) * n, s));
        HIP_TRY(hipStreamSynchronize(s));
    }
    p->d_codes.release();
    p->d_codes16.release();
    p->d_values16.release();
    p->gl_wide = false;
    p->d_tabgl.release();
    dict_clear(p);
    p->gl_cont = true;
    p->gl_vals_dropped = false;
    p->glterms_valid = false;
    return GARLIC_OK;
}

// A new upload after the values were converted in place: the matrix goes back to holding values, all
// zero, and every locus has to come again before the next computation.
int restart_continuous_upload(garlic_panel *p)
{
    if (!p->gl_cont || !p->gl_vals_dropped) return GARLIC_OK;
    const int64_t rows = GOFF + p->nloci + GPAD_BACK;
    const size_t n = (size_t)rows * p->nind_pad;
    HIP_TRY(hipStreamSynchronize(p->ctx->stream));
    std::swap(p->d_glval.p, p->d_glterms.p);
    std::swap(p->d_glval.cap, p->d_glterms.cap);
    HIP_TRY(hipMemsetAsync(p->d_glval.p, 0, sizeof(double) * n, p->ctx->stream));
    p->gl_vals_dropped = false;
    p->glterms_valid = false;
    p->gl_cover_required = true;
    p->gl_cover.assign((size_t)p->nloci, 0);
    return GARLIC_OK;
}

// ---- uploads (the garlic_panel_set_* doors): what they share
int check_loci(const garlic_panel *p, int64_t locus_begin, int64_t locus_count)
{
    if (locus_begin < 0 || locus_count < 1 || locus_begin + locus_count > p->nloci)
        return fail(GARLIC_ERR_INVALID, "locus range [%lld,+%lld) outside panel of %lld loci",
                    (long long)locus_begin, (long long)locus_count, (long long)p->nloci);
    return GARLIC_OK;
}

// rows of one element per individual
int check_rows(const garlic_panel *p, int64_t ld, int64_t locus_begin, int64_t locus_count)
{
    if (ld < p->nind) return fail(GARLIC_ERR_INVALID, "ld %lld < nind %d", (long long)ld, p->nind);
    return check_loci(p, locus_begin, locus_count);
}

int upload_fail(const char *door, hipError_t e) { return fail(GARLIC_ERR_HIP, "%s: %s", door, hipGetErrorString(e)); }

// what the body of a slab (and encode_until_known) may answer besides GARLIC_OK and an error code
constexpr int SLAB_DRAINED = -1;      // done, and the stream is idle: the body synchronised after its last look at the rows
constexpr int DICT_FULL = -2;         // a value of the slab found no room in the dictionary: the slab's codes are void

// The caller's rows, `pitch` bytes each, a slab at a time.  Host rows travel through `stage`, at most 256 MB and at least 16 rows
// of them; device rows are one slab, read where they are.  body(device rows, first row, number of rows) enqueues the slab's
// work; the stream is synchronised once behind every slab, because the staging buffer is used again (and the caller's rows are
// free when the call returns).  A HIP failure is reported under the door's name.
template <class T, class Body>
int for_each_upload_slab(hipStream_t s, const char *door, const void *rows, int64_t pitch, int64_t locus_count, int32_t where,
                         DevBuf<T> &stage, Body body)
{
    const bool host = where == GARLIC_HOST;
    const int64_t slab_rows = host ? std::max<int64_t>(16, ((int64_t)256 << 20) / pitch) : locus_count;
    for (int64_t at = 0; at < locus_count; at += slab_rows) {
        const int64_t n = std::min(slab_rows, locus_count - at);
        const void *src = (const uint8_t *)rows + at * pitch;
        if (host) {
            if (int rc = stage.reserve((size_t)(n * pitch) / sizeof(T))) return rc;
            hipError_t e = hipMemcpyAsync(stage.p, src, (size_t)(n * pitch), hipMemcpyHostToDevice, s);
            if (e != hipSuccess) return upload_fail(door, e);
            src = stage.p;
        }
        const int rc = body(src, at, n);
        if (rc == SLAB_DRAINED) continue;
        if (rc) return rc;
        hipError_t e = hipGetLastError();
        if (e == hipSuccess) e = hipStreamSynchronize(s);
        if (e != hipSuccess) return upload_fail(door, e);
    }
    return GARLIC_OK;
}

// ---- the likelihood dictionary (gl_values / gl_code): written here and nowhere else
uint64_t value_bits(double v)
{
    uint64_t bits;
    memcpy(&bits, &v, sizeof bits);
    return bits;
}

// The code of a value, a new one if it has none: DICT_FULL when that would be value number cap + 1.  Neither form of the panel
// reads the other's table flag (ensure_gl_table runs on one-byte panels only, ensure_values16 on 16-bit ones only, and
// switch_to_wide clears both), so both go.
int dict_add(garlic_panel *p, uint64_t bits, int cap)
{
    auto it = p->gl_code.find(bits);
    if (it != p->gl_code.end()) return it->second;
    const int code = (int)p->gl_values.size();
    if (code >= cap) return DICT_FULL;
    double v;
    memcpy(&v, &bits, sizeof v);
    p->gl_code.emplace(bits, code);
    p->gl_values.push_back(v);
    p->wide_bound_known = false;
    p->tabgl_valid = p->values16_valid = false;
    return code;
}

void dict_clear(garlic_panel *p)
{
    p->gl_code.clear();
    p->gl_values.clear();
    p->wide_bound_known = false;
    p->tabgl_valid = p->values16_valid = false;
}

// device room for a dictionary of cap values, sorted by bit pattern, and for the values that come back unknown
constexpr int UNK_CAP = 8192;
struct EncodeScratch {
    DevBuf<uint64_t> bits, unk;
    DevBuf<uint8_t> codes;               // cap codes of one or two bytes
    DevBuf<int32_t> nunk;
    std::vector<uint64_t> host_unk;
    int reserve(int cap, size_t code_bytes)
    {
        int rc;
        if ((rc = bits.reserve((size_t)cap)) || (rc = codes.reserve((size_t)cap * code_bytes)) || (rc = unk.reserve(UNK_CAP)) ||
            (rc = nunk.reserve(1)))
            return rc;
        host_unk.resize(UNK_CAP);
        return GARLIC_OK;
    }
};

// A slab of values is coded on the device against the dictionary so far; the values it does not know come back (up to UNK_CAP a
// round), join the dictionary, and the slab is coded again, until none is left: SLAB_DRAINED (every round ends synchronised:
// the counter is read).  launch(codes by sorted position, number of values) starts the door's encode kernel on sc.bits / sc.unk /
// sc.nunk.  (A hash look-up per genotype on the host took minutes at 1e10 genotypes.)
template <class Code, class Launch>
int encode_until_known(garlic_panel *p, const char *door, int cap, EncodeScratch &sc, Launch launch)
{
    hipStream_t s = p->ctx->stream;
    for (;;) {
        std::vector<std::pair<uint64_t, Code>> dict;
        for (auto &kv : p->gl_code) dict.emplace_back(kv.first, (Code)kv.second);
        std::sort(dict.begin(), dict.end());
        std::vector<uint64_t> hb(dict.size());
        std::vector<Code> hc(dict.size());
        for (size_t k = 0; k < dict.size(); k++) { hb[k] = dict[k].first; hc[k] = dict[k].second; }
        hipError_t e = hipSuccess;
        if (!dict.empty()) {
            e = hipMemcpyAsync(sc.bits.p, hb.data(), sizeof(uint64_t) * hb.size(), hipMemcpyHostToDevice, s);
            if (e == hipSuccess) e = hipMemcpyAsync(sc.codes.p, hc.data(), sizeof(Code) * hc.size(), hipMemcpyHostToDevice, s);
        }
        if (e == hipSuccess) e = hipMemsetAsync(sc.nunk.p, 0, sizeof(int32_t), s);
        if (e != hipSuccess) return upload_fail(door, e);
        launch((const Code *)sc.codes.p, (int)dict.size());
        int32_t nunk = 0;
        e = hipGetLastError();
        if (e == hipSuccess) e = hipMemcpyAsync(&nunk, sc.nunk.p, sizeof nunk, hipMemcpyDeviceToHost, s);
        if (e == hipSuccess) e = hipStreamSynchronize(s);          // also: hb / hc are free again
        if (e != hipSuccess) return upload_fail(door, e);
        if (nunk == 0) return SLAB_DRAINED;
        const int got = std::min<int32_t>(nunk, UNK_CAP);
        e = hipMemcpy(sc.host_unk.data(), sc.unk.p, sizeof(uint64_t) * got, hipMemcpyDeviceToHost);
        if (e != hipSuccess) return upload_fail(door, e);
        for (int k = 0; k < got; k++)
            if (dict_add(p, sc.host_unk[k], cap) == DICT_FULL) return DICT_FULL;
    }
}

// what every likelihood door does first ...
int begin_gl_upload(garlic_panel *p)
{
    int rc;
    if ((rc = set_device(p->ctx)) || (rc = restart_continuous_upload(p))) return rc;
    if (!p->gl_cont && getenv("GARLIC_TGLS_CONTINUOUS") && (rc = switch_to_continuous(p))) return rc;
    return GARLIC_OK;
}

// ... and last
int end_gl_upload(garlic_panel *p, int64_t locus_begin, int64_t locus_count)
{
    if (p->gl_cont && !p->gl_cover.empty()) memset(p->gl_cover.data() + locus_begin, 1, (size_t)locus_count);
    p->have_gl = true;
    p->glterms_valid = false;
    return GARLIC_OK;
}

// the one-byte code matrix of a panel that keeps such codes, all zero when it is new
int ensure_byte_codes(garlic_panel *p)
{
    if (p->gl_cont || p->gl_wide || p->d_codes.p) return GARLIC_OK;
    const size_t n = (size_t)((GOFF + p->nloci + GPAD_BACK) * p->nind_pad);
    if (int rc = p->d_codes.reserve(n)) return rc;
    HIP_TRY(hipMemsetAsync(p->d_codes.p, 0, n, p->ctx->stream));
    return GARLIC_OK;
}

// terms from values on the host, with the host's own log10: the fallback when the device's restatement
// of glibc's log10 does not reproduce this host's libm (ensure_log10), or GARLIC_TGLS_HOST_TERMS is set
int build_terms_on_host(garlic_panel *p, const double *vals, double *terms)
{
    const int64_t rows = GOFF + p->nloci + GPAD_BACK;
    const int nblk = (int)(p->nind_pad / WAVE);
    const int64_t chunk = std::max<int64_t>(16, (((int64_t)128 << 20) / (8 * WAVE * nblk)) & ~(int64_t)15);
    std::vector<double> hv((size_t)chunk * WAVE * nblk);
    std::vector<uint32_t> hw((size_t)(chunk / 16 + 2) * WAVE * nblk);
    hipStream_t s = p->ctx->stream;
    const double *freq = p->freq.data();
    for (int64_t G0 = GOFF; G0 < GOFF + p->nloci; G0 += chunk) {
        const int64_t G1 = std::min<int64_t>(GOFF + p->nloci, G0 + chunk), nr = G1 - G0;
        const int64_t w0 = G0 >> 4, nw = ((G1 - 1) >> 4) - w0 + 1;
        for (int b = 0; b < nblk; b++) {
            HIP_TRY(hipMemcpyAsync(hv.data() + (size_t)b * chunk * WAVE, vals + ((int64_t)b * rows + G0) * WAVE,
                                   sizeof(double) * nr * WAVE, hipMemcpyDeviceToHost, s));
            HIP_TRY(hipMemcpyAsync(hw.data() + (size_t)b * (chunk / 16 + 2) * WAVE,
                                   p->d_packed.p + ((int64_t)b * p->nwordrows + w0) * WAVE, sizeof(uint32_t) * nw * WAVE,
                                   hipMemcpyDeviceToHost, s));
        }
        HIP_TRY(hipStreamSynchronize(s));
        double *hvp = hv.data();
        const uint32_t *hwp = hw.data();
        parallel_for(nr * nblk, 256, [=](int64_t lo, int64_t hi) {
            for (int64_t k = lo; k < hi; k++) {
                const int64_t b = k / nr, r = k % nr, G = G0 + r;
                double *v = hvp + ((size_t)b * chunk + r) * WAVE;
                const uint32_t *w = hwp + ((size_t)b * (chunk / 16 + 2) + ((G >> 4) - w0)) * WAVE;
                const double f = freq[G - GOFF];
                for (int lane = 0; lane < WAVE; lane++) {
                    const uint32_t code = (w[lane] >> (2 * (int)(G & 15))) & 3u;
                    v[lane] = host_lod(code == 3u ? -9 : (int)code, f, v[lane]);
                }
            }
        });
        for (int b = 0; b < nblk; b++)
            HIP_TRY(hipMemcpyAsync(terms + ((int64_t)b * rows + G0) * WAVE, hv.data() + (size_t)b * chunk * WAVE,
                                   sizeof(double) * nr * WAVE, hipMemcpyHostToDevice, s));
        HIP_TRY(hipStreamSynchronize(s));
    }
    return GARLIC_OK;
}

// The same for a panel of 16-bit codes: the terms of the blocks [b0, b1) into the slab-local matrix dst[blk - b0][rows][64]
// (the whole matrix: b0 = 0), on stream s.  The codes are downloaded chunk by chunk (no host copy is kept: the fall-back is
// rare, a second copy of 2 B per genotype on the host is not).  decay: NULL, or the host's {nomut, norec} rows for the
// scaled slab, (term * nomut) * norec.  *tmin: the most negative finite raw term met, 0.0 when none is negative.
int build_wide_terms_on_host(garlic_panel *p, int b0, int b1, const double *decay, double *dst, hipStream_t s, double *tmin)
{
    const int64_t rows = GOFF + p->nloci + GPAD_BACK;
    const int nb = b1 - b0;
    const int64_t chunk = std::max<int64_t>(16, (((int64_t)128 << 20) / (8 * WAVE * nb)) & ~(int64_t)15);
    std::vector<double> hv((size_t)chunk * WAVE * nb);
    std::vector<uint16_t> hc((size_t)chunk * WAVE * nb);
    std::vector<uint32_t> hw((size_t)(chunk / 16 + 2) * WAVE * nb);
    const double *freq = p->freq.data(), *val = p->gl_values.data();
    const int nval = (int)p->gl_values.size();
    std::mutex mu;
    double best = 0.0;
    HIP_TRY(hipMemsetAsync(dst, 0, sizeof(double) * (size_t)nb * rows * WAVE, s));      // pad rows: +0.0
    for (int64_t G0 = GOFF; G0 < GOFF + p->nloci; G0 += chunk) {
        const int64_t G1 = std::min<int64_t>(GOFF + p->nloci, G0 + chunk), nr = G1 - G0;
        const int64_t w0 = G0 >> 4, nw = ((G1 - 1) >> 4) - w0 + 1;
        for (int b = 0; b < nb; b++) {
            HIP_TRY(hipMemcpyAsync(hc.data() + (size_t)b * chunk * WAVE, p->d_codes16.p + ((int64_t)(b0 + b) * rows + G0) * WAVE,
                                   sizeof(uint16_t) * nr * WAVE, hipMemcpyDeviceToHost, s));
            HIP_TRY(hipMemcpyAsync(hw.data() + (size_t)b * (chunk / 16 + 2) * WAVE,
                                   p->d_packed.p + ((int64_t)(b0 + b) * p->nwordrows + w0) * WAVE, sizeof(uint32_t) * nw * WAVE,
                                   hipMemcpyDeviceToHost, s));
        }
        HIP_TRY(hipStreamSynchronize(s));
        double *hvp = hv.data();
        const uint16_t *hcp = hc.data();
        const uint32_t *hwp = hw.data();
        double *bestp = &best;
        std::mutex *mup = &mu;
        parallel_for(nr * nb, 256, [=](int64_t lo, int64_t hi) {
            double m = 0.0;
            for (int64_t k = lo; k < hi; k++) {
                const int64_t b = k / nr, r = k % nr, G = G0 + r;
                double *v = hvp + ((size_t)b * chunk + r) * WAVE;
                const uint16_t *c = hcp + ((size_t)b * chunk + r) * WAVE;
                const uint32_t *w = hwp + ((size_t)b * (chunk / 16 + 2) + ((G >> 4) - w0)) * WAVE;
                const double f = freq[G - GOFF];
                for (int lane = 0; lane < WAVE; lane++) {
                    const uint32_t code = (w[lane] >> (2 * (int)(G & 15))) & 3u;
                    double t = host_lod(code == 3u ? -9 : (int)code, f, val[c[lane] < nval ? c[lane] : 0]);
                    if (t < m && t > -1.7976931348623157e308) m = t;
                    if (decay) t = (t * decay[2 * G]) * decay[2 * G + 1];
                    v[lane] = t;
                }
            }
            if (m < 0.0) {
                std::lock_guard<std::mutex> lock(*mup);
                if (m < *bestp) *bestp = m;
            }
        });
        for (int b = 0; b < nb; b++)
            HIP_TRY(hipMemcpyAsync(dst + ((int64_t)b * rows + G0) * WAVE, hv.data() + (size_t)b * chunk * WAVE,
                                   sizeof(double) * nr * WAVE, hipMemcpyHostToDevice, s));
        HIP_TRY(hipStreamSynchronize(s));
    }
    if (tmin) *tmin = best;
    return GARLIC_OK;
}

// who builds the terms of lod() on values: the device once its log10 has reproduced the host's, else the host
bool tgls_terms_on_host(const garlic_panel *p) { return p->ctx->log10_state < 0 || getenv("GARLIC_TGLS_HOST_TERMS"); }

// gl_terms_wide_kernel for the blocks [b0, b1) into the slab-local dst, on stream s (values, frequencies and log table are in place)
void launch_wide_terms(garlic_panel *p, int b0, int b1, const double *d_decay, double *dst, unsigned long long *d_minbits, hipStream_t s)
{
    const int64_t rows = GOFF + p->nloci + GPAD_BACK;
    hipLaunchKernelGGL(gl_terms_wide_kernel, dim3((unsigned)((rows + 63) / 64), (unsigned)std::min(b1 - b0, 65535)), dim3(256), 0, s,
                       p->d_packed.p, p->nwordrows, p->d_freq.p, p->ctx->d_logtab.p, p->d_codes16.p, p->d_values16.p,
                       (int32_t)p->gl_values.size(), d_decay, rows, b0, b1, dst, d_minbits);
}

// ---- TGLS pass 1: every (SNP, individual) term, once per panel (window-size independent).
// Dictionary-coded likelihoods: returns GARLIC_OK with glterms_valid unset when the matrix does not
// fit -- the caller then keeps the look-up-in-the-chain kernel.  Continuous likelihoods always end
// with a valid matrix (converted in place when a second buffer does not fit) or an error.
// scaled = multiplied in place by the decay factors of (M, mu) for the weighted tile kernel
// (ensure_decay_table first).  Switching between the two forms rebuilds / rescales.
int ensure_gl_terms(garlic_panel *p, bool scaled = false, int32_t M = 0, double mu = 0.0)
{
    const bool same_scale = p->glterms_scaled && p->glterms_M == M && memcmp(&p->glterms_mu, &mu, sizeof mu) == 0;
    if (p->glterms_valid && (scaled ? same_scale : !p->glterms_scaled)) return GARLIC_OK;
    if (!p->gl_cont && getenv("GARLIC_GL_NO_TERMS")) return GARLIC_OK;
    const int64_t rows = GOFF + p->nloci + GPAD_BACK;
    const size_t n = (size_t)rows * p->nind_pad;
    hipStream_t s = p->ctx->stream;
    int rc;
    const bool rebuild = !p->glterms_valid || p->glterms_scaled;   // the raw terms have to be made (again)
    bool fused_scale = false;                                       // ... and were scaled in the same pass
    if (p->gl_cont && rebuild) {
        if (p->gl_vals_dropped)
            return fail(GARLIC_ERR_STATE, "the likelihoods of this panel were converted to terms in place (no room for "
                                          "both); after changing genotypes, frequencies or the weighting they "
                                          "have to be uploaded again (garlic_panel_set_gl over all loci)");
        if (p->gl_cover_required) {
            for (int64_t l = 0; l < p->nloci; l++)
                if (!p->gl_cover[(size_t)l])
                    return fail(GARLIC_ERR_STATE, "likelihood upload restarted: locus %lld has not been uploaded again",
                                (long long)l);
            p->gl_cover_required = false;
        }
        if ((rc = ensure_log10(p->ctx)) || (rc = ensure_dfreq(p))) return rc;
        size_t free_b = 0, total_b = 0;
        HIP_TRY(hipMemGetInfo(&free_b, &total_b));
        if (p->d_glterms.cap < n && (free_b < n * sizeof(double) || free_b - n * sizeof(double) < (size_t)(0.45 * (double)total_b))) {
            HIP_TRY(hipStreamSynchronize(s));      // idle pooled score buffers are not a reason to give the values up
            (void)score_pool_trim();
            HIP_TRY(hipMemGetInfo(&free_b, &total_b));
        }
        // a second matrix only while it leaves plenty of room for the scores (it is what lets the panel
        // switch between raw and weighted terms later); otherwise the values become the terms
        bool separate = p->d_glterms.cap >= n ||
                        (free_b >= n * sizeof(double) && free_b - n * sizeof(double) >= (size_t)(0.45 * (double)total_b));
        if (const char *e = getenv("GARLIC_TGLS_INPLACE")) separate = atoi(e) == 0;
        if (separate && (rc = p->d_glterms.reserve(n))) return rc;
        double *dst = separate ? p->d_glterms.p : p->d_glval.p;
        p->glterms_valid = false;
        const bool on_host = p->ctx->log10_state < 0 || getenv("GARLIC_TGLS_HOST_TERMS");
        DevBuf<unsigned long long> d_minbits;
        if (on_host) {
            if (separate)   // pad rows of the term matrix: +0.0
                HIP_TRY(hipMemsetAsync(dst, 0, sizeof(double) * n, s));
            if ((rc = build_terms_on_host(p, p->d_glval.p, dst))) return rc;
        } else {
            // all rows, pad rows included: their frequency is 0 and their genotypes code 3 -> +0.0; the most negative
            // finite term (lod_exact_needed) is collected along the way
            if ((rc = d_minbits.reserve(GL_MIN_SLOTS))) return rc;
            HIP_TRY(hipMemsetAsync(d_minbits.p, 0, sizeof(unsigned long long) * GL_MIN_SLOTS, s));
            hipLaunchKernelGGL(gl_terms_cont_kernel, dim3((unsigned)((rows + 63) / 64), (unsigned)(p->nind_pad / WAVE)),
                               dim3(256), 0, s, p->d_packed.p, p->nwordrows, p->d_freq.p, p->ctx->d_logtab.p, p->d_glval.p,
                               (int64_t)0, rows, rows, dst, d_minbits.p);
            HIP_TRY(hipGetLastError());
        }
        if (!separate) {   // the term matrix takes the buffer over
            HIP_TRY(hipStreamSynchronize(s));
            p->d_glterms.release();
            std::swap(p->d_glterms.p, p->d_glval.p);
            std::swap(p->d_glterms.cap, p->d_glval.cap);
            p->gl_vals_dropped = true;
        }
        p->gl_terms_by = on_host ? 2 : 1;
        p->glterms_scaled = false;
        if (!on_host) {
            unsigned long long bits[GL_MIN_SLOTS], best = 0;
            hipError_t e = hipMemcpyAsync(bits, d_minbits.p, sizeof bits, hipMemcpyDeviceToHost, s);
            if (e == hipSuccess) e = hipStreamSynchronize(s);
            d_minbits.release();
            if (e != hipSuccess) return fail(GARLIC_ERR_HIP, "term minimum: %s", hipGetErrorString(e));
            for (unsigned long long b : bits) best = std::max(best, b);
            p->glterms_min = best ? f64_from_bits(best) : 0.0;
        } else {   // most negative finite term, for lod_exact_needed
            constexpr int NB = 1024;
            DevBuf<double> d_part;
            if ((rc = d_part.reserve(NB))) return rc;
            double part[NB];
            hipLaunchKernelGGL(min_finite_kernel, dim3(NB), dim3(256), 0, s, p->d_glterms.p, (int64_t)n, d_part.p);
            hipError_t e = hipMemcpyAsync(part, d_part.p, sizeof part, hipMemcpyDeviceToHost, s);
            if (e == hipSuccess) e = hipStreamSynchronize(s);
            if (e != hipSuccess) return fail(GARLIC_ERR_HIP, "term minimum: %s", hipGetErrorString(e));
            p->glterms_min = min_finite(part, NB);
        }
    } else if (rebuild && p->gl_wide) {
        // 16-bit codes: lod() on the device as for continuous values (or on the host), the weighted kernels' scaling in the same
        // pass.  Room is judged as for a one-byte panel; declined (glterms_valid unset) the caller goes on to slabs.
        if ((rc = ensure_log10(p->ctx)) || (rc = ensure_dfreq(p)) || (rc = ensure_values16(p))) return rc;
        size_t free_b = 0, total_b = 0;
        if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) return GARLIC_OK;
        if (p->d_glterms.cap < n && n * sizeof(double) + ((size_t)8 << 30) > free_b) {
            HIP_TRY(hipStreamSynchronize(s));
            (void)score_pool_trim();
            p->lds.release();
            if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) return GARLIC_OK;
            if (n * sizeof(double) + ((size_t)8 << 30) > free_b) return GARLIC_OK;
        }
        if ((rc = p->d_glterms.reserve(n))) return rc;
        p->glterms_valid = false;
        const int nblk = (int)(p->nind_pad / WAVE);
        if (tgls_terms_on_host(p)) {
            if ((rc = build_wide_terms_on_host(p, 0, nblk, scaled ? p->h_decay.data() : nullptr, p->d_glterms.p, s, &p->glterms_min))) return rc;
            p->gl_terms_by = 2;
        } else {
            DevBuf<unsigned long long> d_minbits;
            if ((rc = d_minbits.reserve(GL_MIN_SLOTS))) return rc;
            HIP_TRY(hipMemsetAsync(d_minbits.p, 0, sizeof(unsigned long long) * GL_MIN_SLOTS, s));
            launch_wide_terms(p, 0, nblk, scaled ? p->d_decay.p : nullptr, p->d_glterms.p, d_minbits.p, s);
            HIP_TRY(hipGetLastError());
            unsigned long long bits[GL_MIN_SLOTS], best = 0;
            hipError_t e = hipMemcpyAsync(bits, d_minbits.p, sizeof bits, hipMemcpyDeviceToHost, s);
            if (e == hipSuccess) e = hipStreamSynchronize(s);
            if (e != hipSuccess) return fail(GARLIC_ERR_HIP, "term minimum: %s", hipGetErrorString(e));
            for (unsigned long long b : bits) best = std::max(best, b);
            p->glterms_min = best ? f64_from_bits(best) : 0.0;
            p->gl_terms_by = 1;
        }
        p->glterms_scaled = false;
        fused_scale = scaled;
    } else if (rebuild) {
        size_t free_b = 0, total_b = 0;
        if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) return GARLIC_OK;
        if (p->d_glterms.cap < n && n * sizeof(double) + ((size_t)8 << 30) > free_b) {
            // score buffers idle in the pool (candidates of an earlier placement probe, freed score matrices) are worth
            // nothing next to the term matrix: give them back first.  (Round 4: 70 GB of them left the 10M x 1250 shard
            // without its term matrix -- the chain then looks its terms up, 4.4 x slower, the weighted strip kernel 60 x.)
            HIP_TRY(hipStreamSynchronize(s));
            (void)score_pool_trim();
            if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) return GARLIC_OK;
        }
        if (p->d_glterms.cap < n && n * sizeof(double) + ((size_t)8 << 30) > free_b) {
            // not enough room: the LD scratch the panel keeps for the next window size is worth less
            // than the term matrix (the look-up-in-the-chain kernel is 10x slower)
            HIP_TRY(hipStreamSynchronize(s));
            p->lds.release();
            if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) return GARLIC_OK;
            if (n * sizeof(double) + ((size_t)8 << 30) > free_b) return GARLIC_OK;
        }
        if ((rc = p->d_glterms.reserve(n))) return rc;
        p->glterms_valid = false;
        // pad rows in front of and behind each block's SNPs: 0.0, the term of a missing genotype (the kernel writes the rest)
        for (int64_t b = 0; b < p->nind_pad / WAVE; b++) {
            HIP_TRY(hipMemsetAsync(p->d_glterms.p + (size_t)b * rows * WAVE, 0, sizeof(double) * GOFF * WAVE, s));
            HIP_TRY(hipMemsetAsync(p->d_glterms.p + ((size_t)b * rows + GOFF + p->nloci) * WAVE, 0,
                                   sizeof(double) * (size_t)(rows - GOFF - p->nloci) * WAVE, s));
        }
        VariantArgs a{p->d_packed.p, nullptr, p->d_tabgl.p, p->d_codes.p, nullptr, nullptr, nullptr, nullptr, nullptr,
                      p->nind_pad, p->nwordrows, 0, 0, 0, (int32_t)p->gl_values.size(), 1, nullptr, 0};
        const size_t terms_lds = sizeof(double) * GL_TERMS_S * 4 * (size_t)a.ncodes;      // <= 64 KB (256 codes)
        if (!getenv("GARLIC_GL_TERMS_GATHER")) {
            if (terms_lds > LDS_DEFAULT_MAX)
                HIP_TRY(hipFuncSetAttribute((const void *)gl_terms_lds_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)terms_lds));
            // (the weighted kernel's scores in the same pass when that is what is asked for)
            hipLaunchKernelGGL(gl_terms_lds_kernel, dim3((unsigned)((p->nloci + GL_TERMS_S - 1) / GL_TERMS_S)), dim3(256), terms_lds, s,
                               a, p->nloci, rows, (int)(p->nind_pad / WAVE), scaled ? p->d_decay.p : (const double *)nullptr,
                               p->d_glterms.p);
            fused_scale = scaled;
        } else
        hipLaunchKernelGGL(gl_terms_kernel, dim3((unsigned)((p->nloci + 63) / 64), (unsigned)(p->nind_pad / WAVE)),
                           dim3(256), 0, s, a, p->nloci, rows, p->d_glterms.p);
        HIP_TRY(hipGetLastError());
        p->glterms_scaled = false;
        p->gl_terms_by = 0;
    }
    if (scaled && fused_scale) {
        p->glterms_scaled = true;
        p->glterms_M = M;
        p->glterms_mu = mu;
    } else if (scaled) {
        hipLaunchKernelGGL(gl_scale_kernel, dim3(4096), dim3(256), 0, s, p->d_glterms.p, p->d_decay.p, rows,
                           (int64_t)(p->nind_pad / WAVE));
        HIP_TRY(hipGetLastError());
        p->glterms_scaled = true;
        p->glterms_M = M;
        p->glterms_mu = mu;
    }
    p->glterms_valid = true;
    return GARLIC_OK;
}

// ---- TGLS term slabs (garlic_panel_set_tgls_term_budget).  A 64-individual block of the matrix and what the panel holds of it:
size_t tgls_block_bytes(const garlic_panel *p) { return sizeof(double) * (size_t)(GOFF + p->nloci + GPAD_BACK) * WAVE; }

// Slab size under a bound of `bytes`: the largest number of blocks s whose buffers fit -- the slabs of a call alternate between
// two buffers, so the first needs s blocks and the second what the second slab holds, min(s, nblk - s), of the nblk blocks that
// hold individuals (the whole matrix has nind_pad / 64 of them, a pad block more when nind leaves less than one free).  0: none fits.
int32_t tgls_slab_blocks_for(const garlic_panel *p, size_t bytes)
{
    const int64_t nblk = (p->nind + WAVE - 1) / WAVE;
    int32_t best = 0;
    for (int64_t s = 1; s <= nblk; s++)
        if ((size_t)(s + std::min(s, nblk - s)) * tgls_block_bytes(p) <= bytes) best = (int32_t)s;
    return best;
}

void release_tgls_slabs(garlic_panel *p)
{
    p->d_slab[0].release();
    p->d_slab[1].release();
}

// What holds the terms of the use_gl call at hand -- raw ones for the unweighted chains, scaled by the decay factors of (M, mu)
// for the weighted kernels (ensure_decay_table first): *slab_blocks > 0 when they are to come slab by slab; 0 when the whole
// matrix serves it as before or, declined, nothing does (glterms_valid / glterms_scaled tell: the caller then looks its terms
// up).  Dictionary-coded panels only; GARLIC_GL_NO_TERMS keeps its meaning.
int tgls_terms_or_slabs(garlic_panel *p, int32_t *slab_blocks, bool scaled = false, int32_t M = 0, double mu = 0.0)
{
    *slab_blocks = 0;
    const size_t block = tgls_block_bytes(p), whole = block * (size_t)(p->nind_pad / WAVE);
    int rc;
    // (16-bit codes have no look-up chain to fall back to: where budget 0 finds no room for the whole matrix they go on as under -1)
    const bool wide_auto = p->gl_wide && (p->terms_budget == 0 || getenv("GARLIC_GL_NO_TERMS"));
    if (!wide_auto && (p->gl_cont || p->terms_budget == 0 || getenv("GARLIC_GL_NO_TERMS") || (p->terms_budget > 0 && whole <= (size_t)p->terms_budget))) {
        if (!p->gl_cont && p->d_slab[0].p) {       // (a budget that now admits the whole matrix: not both)
            HIP_TRY(hipStreamSynchronize(p->ctx->stream));
            release_tgls_slabs(p);
        }
        return ensure_gl_terms(p, scaled, M, mu);
    }
    size_t bytes = (size_t)p->terms_budget;
    if (p->terms_budget < 0 || wide_auto) {
        // the whole matrix when today's test lets it in; otherwise two slab buffers in half of what is free now
        if ((rc = ensure_gl_terms(p, scaled, M, mu))) return rc;
        if (p->glterms_valid && p->glterms_scaled == scaled) {
            if (wide_auto && p->d_slab[0].p) {
                HIP_TRY(hipStreamSynchronize(p->ctx->stream));
                release_tgls_slabs(p);
            }
            return GARLIC_OK;
        }
        size_t free_b = 0, total_b = 0;
        if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) return GARLIC_OK;
        bytes = (free_b + (p->d_slab[0].cap + p->d_slab[1].cap) * sizeof(double)) / 2;
        if (!tgls_slab_blocks_for(p, bytes)) return GARLIC_OK;     // not even one-block slabs: the look-up chain
    } else if (p->d_glterms.cap) {
        // a whole matrix, raw or scaled, from before the budget
        HIP_TRY(hipStreamSynchronize(p->ctx->stream));
        p->d_glterms.release();
        p->glterms_valid = false;
    }
    *slab_blocks = tgls_slab_blocks_for(p, bytes);
    return GARLIC_OK;
}

// ---- wLOD: per-SNP {nomut, norec} (garlic-roh.cpp:134-140, 246-249), host libm exp
int ensure_decay_table(garlic_panel *p, int32_t M, double mu)
{
    if (!p->have_gpos) return fail(GARLIC_ERR_STATE, "wLOD needs genetic positions (set_map with gpos)");
    if (p->decay_valid && p->decay_M == M && memcmp(&p->decay_mu, &mu, sizeof mu) == 0) return GARLIC_OK;
    const int64_t rows = GOFF + p->nloci + GPAD_BACK;
    std::vector<double> dec((size_t)rows * 2, 0.0);
    for (int c = 0; c < p->nchr; c++)
        for (int64_t l = p->chr_off[c]; l < p->chr_off[c + 1]; l++) {
            const bool first = (l == p->chr_off[c]); // locus 0 of a chromosome: absolute position
            const double dP = first ? (double)p->pos[l] : (double)(p->pos[l] - p->pos[l - 1]);
            const double dG = first ? p->gpos[l] : (p->gpos[l] - p->gpos[l - 1]);
            const double Md = M; // the reference passes the int M as a double parameter
            dec[(GOFF + l) * 2 + 0] = exp(-2.0 * Md * mu * dP);
            dec[(GOFF + l) * 2 + 1] = exp(-2.0 * Md * 1 * dG);
        }
    if (int rc = p->d_decay.put(dec, p->ctx->stream)) return rc;
    HIP_TRY(hipStreamSynchronize(p->ctx->stream));
    p->decay_valid = true;
    p->decay_M = M;
    p->decay_mu = mu;
    p->h_decay.swap(dec);
    p->wtab_valid = false;
    return GARLIC_OK;
}

// ---- wLOD, tuned path: score of every genotype per SNP, (lod * nomut) * norec in the reference's
// order (garlic-roh.cpp:249) -- the same three doubles the per-individual expression multiplies
int ensure_score_rows(garlic_panel *p, double error, int32_t M, double mu, int32_t W)
{
    const int64_t rows = GOFF + p->nloci + std::max<int64_t>(GPAD_BACK, W + 64);
    if (p->wtab_valid && rows <= p->wtab_rows && p->wtab_M == M &&
        memcmp(&p->wtab_error, &error, sizeof error) == 0 && memcmp(&p->wtab_mu, &mu, sizeof mu) == 0)
        return GARLIC_OK;
    std::vector<double> w((size_t)rows * 4, 0.0);
    const double *t = p->h_tab.data(), *d = p->h_decay.data();
    const int64_t have = std::min<int64_t>(rows, GOFF + p->nloci + GPAD_BACK);
    double *wp = w.data();
    parallel_for(have, 1 << 16, [=](int64_t lo, int64_t hi) {
        for (int64_t G = lo; G < hi; G++)
            for (int g = 0; g < 4; g++) wp[G * 4 + g] = (t[G * 4 + g] * d[2 * G]) * d[2 * G + 1];
    });
    if (int rc = p->d_wtab.put(w, p->ctx->stream)) return rc;
    HIP_TRY(hipStreamSynchronize(p->ctx->stream));
    p->wtab_valid = true;
    p->wtab_error = error; p->wtab_M = M; p->wtab_mu = mu; p->wtab_rows = rows;
    return GARLIC_OK;
}

// ---- A score call, step by step: arguments (LodCall) -> kernel form (LodForm) -> work lists (LodWork, counted in the
// panel's plan) -> score buffer -> launches (enqueue_lod) -> by-value -9999 rescan -> copy out -> statistics.
struct LodCall {
    Mode mode;
    int32_t W, max_gap, M, ind_begin, ind_count, pitch_align, thin_step, where, host_pitch_align;     // pitch_align: of the device layout
    double error, mu, *out;
    const std::vector<uint8_t> *blocks;
};

// Which kernel takes the call and what that needs: filled once by decide_form, then by finish_form with what depends on the
// score buffer.  Everything after reads it: no later code looks at W, the mode or the environment to pick a kernel.
enum class Family { chain, feed, exact, tgls_ring, tgls_feed, tgls_terms, tgls_lookup, wlod_tile, wlod_tile2, wlod_tile_gl, wlod_glring,
                    wlod_small_tiles, wlod_stream, wlod_strip, wlod_generic, wlod_feed };

struct LodForm {
    Family family = Family::chain;
    bool use_gl = false;
    bool exact_possible = false;   // a window can sum to exactly -9999.0: rescan, and Family::exact if one did
    bool cov_bits = false;         // coverage bits instead of scores (garlic_panel::cov_pending); `out` is no score buffer then
    bool writes_bits = false;      // ... and this family can write them
    bool wlod_tuned = false;       // a tuned wLOD kernel: reads the plan's valid mask, tiles, segments; writes MISSING itself
    bool wlod_gl = false;          // ... with its scores from the scaled term matrix
    int strip_waves = 0;           // wlod_strip: compute waves per workgroup
    bool use_patch = false, no_prefetch = false, feed_asm = true, strip_force_rerun = false;
    size_t tile_lds = 0;           // dynamic LDS of the tile kernels
    bool aligned16 = false;        // finish_form: every score row 16-byte aligned
    bool strip_three = false;      // finish_form: the 80-VGPR strip kernel, three workgroups per CU
    int32_t slab_blocks = 0;       // tgls_ring / tgls_feed, and with wlod_gl the tuned wLOD kernels and wlod_feed: the term matrix
                                   // comes slab by slab, this many blocks each
};

int check_lod_args(const garlic_panel *p, const LodCall &c)
{
    if (c.W <= 1) return fail(GARLIC_ERR_INVALID, "SNP window size must be > 1 (got %d)", c.W);
    if (!p->have_map || !p->have_freq || !p->have_geno)
        return fail(GARLIC_ERR_STATE, "panel needs map, freq and genotypes before computing LOD");
    if (c.ind_begin < 0 || c.ind_count < 1 || (int64_t)c.ind_begin + c.ind_count > p->nind)
        return fail(GARLIC_ERR_INVALID, "individual range [%d,+%d) outside panel of %d", c.ind_begin,
                    c.ind_count, p->nind);
    if (!c.out) return fail(GARLIC_ERR_INVALID, "out is NULL");
    if (c.host_pitch_align < 1) return fail(GARLIC_ERR_INVALID, "pitch_align must be >= 1");
    if (c.thin_step > 0 && (c.where != GARLIC_DEVICE || c.host_pitch_align != 32 || c.ind_begin != 0))
        return fail(GARLIC_ERR_INVALID, "internal: thinned output is for device scores of the whole panel, pitch_align 32");
    return GARLIC_OK;
}

// Shape from the arguments and the switches -> the ensure_* that shape asks for -> the form from what the panel now holds.
int decide_form(garlic_panel *p, const LodCall &c, LodForm &f)
{
    const Mode mode = c.mode;
    const int32_t W = c.W;
    int rc;
    f.use_gl = (mode == MODE_LOD_GL) || (mode == MODE_WLOD && p->wlod_use_gl);
    if ((rc = ensure_segments(p, c.max_gap))) return rc;
    if (f.use_gl) {
        if (!p->have_gl) return fail(GARLIC_ERR_STATE, "use_gl set but no genotype likelihoods were given");
        if (!p->gl_cont && !p->gl_wide && (rc = ensure_gl_table(p))) return rc;
        if (mode == MODE_LOD_GL && (rc = tgls_terms_or_slabs(p, &f.slab_blocks))) return rc;
        if (mode == MODE_LOD_GL && p->gl_wide && !f.slab_blocks && !(p->glterms_valid && !p->glterms_scaled))
            return fail(GARLIC_ERR_NOMEM, "16-bit likelihood codes: no room for the term matrix, nor for one-block term slabs");
    } else if ((rc = ensure_term_table(p, c.error))) return rc;
    if (mode == MODE_WLOD) {
        if (!select_ld(p, W))
            return fail(GARLIC_ERR_STATE, "wLOD needs LD weights for winsize %d (garlic_panel_set_ld)", W);
        if ((rc = ensure_decay_table(p, c.M, c.mu))) return rc;
    }
    // A window sum of exactly -9999.0 is possible (lod_exact_needed): the tuned chain runs first, its scored windows
    // are scanned for that value, and only if one is there the chain that follows the reference to the letter
    // (11-17 x slower) runs instead.  GARLIC_EXACT_CHAIN_ONLY: that chain straight away.
    f.exact_possible = mode != MODE_WLOD && lod_exact_needed(p, mode, W);
    if (f.exact_possible && c.thin_step > 0) {      // the rescan and the exact chain need the full matrix
        if (mode == MODE_LOD_GL) return GARLIC_INTERNAL_NO_SAMPLED;
        return fail(GARLIC_ERR_INVALID, "internal: thinned output with the exact chain");
    }
    // coverage bits instead of scores (garlic_roh_coverage_fused): only the kernels that know how; nothing else may touch
    // `out` (it is not a score buffer then)
    f.cov_bits = p->cov_pending.bits != nullptr;
    if (f.cov_bits && mode == MODE_LOD)
        return fail(GARLIC_ERR_STATE, "internal: coverage bits of the unweighted --error scores come from lod_bits_kernel");
    const bool tgls_ring_shape = (c.ind_begin & (WAVE - 1)) == 0 && !getenv("GARLIC_TGLS_NO_RING");
    if (f.cov_bits && mode == MODE_LOD_GL && (f.exact_possible || c.where != GARLIC_DEVICE || !tgls_ring_shape))
        return GARLIC_INTERNAL_NO_BITS;      // the TGLS ring chain / the tuned wLOD kernels do not take this shape
    if (mode != MODE_WLOD) {
        f.feed_asm = !getenv("GARLIC_FEED_NO_ASM");
        if (mode == MODE_LOD) f.family = c.thin_step > 0 ? Family::feed : Family::chain;   // thinned output: every wave a chain of its own (feed_kernel.hpp)
        else if (f.slab_blocks && tgls_ring_shape) f.family = Family::tgls_ring;      // (launch_tgls_slabs; only the ring chains read slabs)
        else if (!p->glterms_valid || p->glterms_scaled) f.family = Family::tgls_lookup;
        else f.family = tgls_ring_shape ? Family::tgls_ring : Family::tgls_terms;
        f.writes_bits = f.family == Family::tgls_ring;
        if (f.exact_possible && getenv("GARLIC_EXACT_CHAIN_ONLY")) f.family = Family::exact;
        // 16-bit codes have no look-up chain: what only that chain covers under slabs is refused
        if (mode == MODE_LOD_GL && p->gl_wide && f.slab_blocks && f.family != Family::tgls_ring)
            return fail(GARLIC_ERR_NOMEM, "16-bit likelihood codes: this call is not covered by term slabs (an ind_begin that is no "
                                          "multiple of 64, GARLIC_TGLS_NO_RING or the by-value chain) and the whole term matrix has no room");
        if (f.family != Family::tgls_ring) f.slab_blocks = 0;
        // TGLS, thinned output: the ring chain that stores the sampled windows only (tgls_feed_kernel.hpp); the other TGLS
        // chains write full scores.  GARLIC_TGLS_FEED_FULL: never.
        if (mode == MODE_LOD_GL && c.thin_step > 0) {
            if (f.cov_bits) return fail(GARLIC_ERR_STATE, "internal: coverage bits with thinned output");
            if (f.family != Family::tgls_ring || getenv("GARLIC_TGLS_FEED_FULL")) return GARLIC_INTERNAL_NO_SAMPLED;
            f.family = Family::tgls_feed;
            f.writes_bits = false;
        }
        return GARLIC_OK;
    }
    // wLOD, thinned output: only the sampled windows (wlod_feed_kernel.hpp), from the score rows or the scaled term matrix
    if (c.thin_step > 0) {
        if (f.cov_bits) return fail(GARLIC_ERR_STATE, "internal: coverage bits with thinned output");
        if (W + 64 > GPAD_BACK) return GARLIC_INTERNAL_NO_SAMPLED;
        if (f.use_gl) {
            if ((rc = tgls_terms_or_slabs(p, &f.slab_blocks, true, c.M, c.mu))) return rc;
            if (!f.slab_blocks && !(p->glterms_valid && p->glterms_scaled)) return GARLIC_INTERNAL_NO_SAMPLED;   // (the term matrix was declined)
        } else if ((rc = ensure_score_rows(p, c.error, c.M, c.mu, W))) return rc;
        f.wlod_gl = f.use_gl;
        f.family = Family::wlod_feed;
        return GARLIC_OK;
    }
    // wLOD.  Tuned kernels: 16 window accumulators per lane; scores from one LDS row per SNP (plain --error) or from the TGLS
    // score matrix (use_gl); very narrow / very wide windows keep the generic kernel.
    const bool use_gl = f.use_gl;
    const bool wlod_shape_ok = W + 64 <= GPAD_BACK && !getenv("GARLIC_WLOD_GENERIC") &&
                               (W >= WLOD_R || !getenv("GARLIC_WLOD_SMALL_GENERIC"));
    const bool wlod_small = W < WLOD_R;      // narrower than a window group: wlod_group_small (compiler-scheduled)
    if (wlod_shape_ok && use_gl && (rc = tgls_terms_or_slabs(p, &f.slab_blocks, true, c.M, c.mu))) return rc;
    // a slab launch starts at a block of the matrix: a sub-range that does not, and every shape that keeps the generic
    // kernel, looks its terms up in the code table under a budget (nothing is built past the bound)
    if (p->gl_wide && use_gl && f.slab_blocks && (c.ind_begin & (WAVE - 1)) != 0)
        return fail(GARLIC_ERR_NOMEM, "16-bit likelihood codes: a weighted call whose ind_begin is no multiple of 64 is not covered by "
                                      "term slabs and the whole term matrix has no room");
    if ((c.ind_begin & (WAVE - 1)) != 0) f.slab_blocks = 0;
    f.wlod_gl = wlod_shape_ok && use_gl && (f.slab_blocks || (p->glterms_valid && p->glterms_scaled));   // (the term matrix may have been declined)
    f.wlod_tuned = (wlod_shape_ok && !use_gl) || f.wlod_gl;
    if (f.wlod_tuned && !f.wlod_gl && sizeof(double) * (size_t)(W + TILE) * 4 + 16 > LDS_STAGING_MAX) f.wlod_tuned = false;
    if (f.wlod_tuned && !f.wlod_gl && (rc = ensure_score_rows(p, c.error, c.M, c.mu, W))) return rc;
    if (!f.wlod_tuned && (rc = ensure_rld(p))) return rc;
    // narrow windows, plain scores: the streaming kernel (wlod_small_kernel.hpp) reads the plain reciprocals, a window's
    // W weights contiguous
    const bool wlod_stream = f.wlod_tuned && wlod_small && !f.cov_bits && !getenv("GARLIC_WLOD_SMALL_TILES");
    if (f.cov_bits && !f.wlod_tuned) return GARLIC_INTERNAL_NO_BITS;
    if (wlod_stream && (rc = ensure_rld(p))) return rc;
    // continuous likelihoods have no code table: the generic kernel takes its terms from the raw matrix
    if (use_gl && p->gl_cont && !f.wlod_tuned && (rc = ensure_gl_terms(p))) return rc;
    // ... nor have 16-bit codes: the same, where the whole raw matrix may be held
    if (use_gl && p->gl_wide && !f.wlod_tuned) {
        const size_t whole = tgls_block_bytes(p) * (size_t)(p->nind_pad / WAVE);
        if (p->terms_budget > 0 && whole > (size_t)p->terms_budget)
            return fail(GARLIC_ERR_NOMEM, "16-bit likelihood codes: the generic weighted kernel is not covered by term slabs and the "
                                          "term budget does not admit the whole matrix");
        if (p->d_slab[0].p || p->d_slab[1].p) {
            HIP_TRY(hipStreamSynchronize(p->ctx->stream));
            release_tgls_slabs(p);
        }
        if ((rc = ensure_gl_terms(p))) return rc;
        if (!(p->glterms_valid && !p->glterms_scaled))
            return fail(GARLIC_ERR_NOMEM, "16-bit likelihood codes: the generic weighted kernel needs the whole term matrix, which has no room");
    }
    if (!f.wlod_tuned) {
        f.family = Family::wlod_generic;
        f.slab_blocks = 0;
        return GARLIC_OK;
    }
    f.writes_bits = true;
    f.no_prefetch = getenv("GARLIC_WLOD_NO_PF") != nullptr;
    // transposed write-out patch only while rows + patch keep 8 workgroups (32 waves) on a CU
    const size_t wlod_rows = f.wlod_gl ? 0 : sizeof(double) * (size_t)(W + TILE) * 4;
    const size_t wlod_patch = sizeof(double) * (size_t)WAVE * WT_PITCH;
    const bool wlod_use_patch = wlod_rows + 16 + wlod_patch <= 160 * 1024 / 8 && !getenv("GARLIC_WLOD_NO_PATCH");
    // term-matrix variant: the hand-scheduled loop stages the block's term rows through one LDS ring
    // per wave; it needs a block-aligned shard (a wave's 64 lanes = one block of the matrix)
    const bool wlod_gl_ring = f.wlod_gl && !wlod_small && (c.ind_begin & (WAVE - 1)) == 0 && !getenv("GARLIC_WLOD_GL_NO_RING");
    const bool ring_patch = !getenv("GARLIC_WLOD_GL_NO_PATCH");
    // ... and with windows narrow enough for WS_WAVES (W <= 113) or WS_WAVES_WIDE (W <= 241) compute waves per workgroup the strip form: the
    // blocks' term rows enter a CU once per strip (wlod_strip_kernel.hpp)
    const int strip_waves = (W + 15 - 16 * WS_WAVES <= 16 || getenv("GARLIC_WLOD_STRIP_NARROW_ONLY")) ? WS_WAVES : WS_WAVES_WIDE;
    const bool wlod_gl_strip = wlod_gl_ring && W + 15 - 16 * strip_waves <= 16 && !getenv("GARLIC_WLOD_GL_NO_STRIP");
    f.strip_waves = strip_waves;
    f.use_patch = wlod_gl_ring ? ring_patch : wlod_use_patch;
    f.tile_lds = wlod_gl_ring ? WLOD_GL_RING_OFF + (size_t)WLOD_WAVES * GARLIC_WLOD_GL_RING_ROWS * WAVE * 8
                              : wlod_rows + 16 + (wlod_use_patch ? wlod_patch : 0);   // 16: the patch lock
    f.strip_force_rerun = wlod_gl_strip && getenv("GARLIC_WLOD_STRIP_FORCE_RERUN") != nullptr;
    // plain --error scores: two blocks per wave (every scalar-loaded weight used twice); the per-genotype
    // variants keep one block per wave (their term rows, not the weights, set their pace)
    f.family = wlod_stream                            ? Family::wlod_stream      // (finish_form: 16-byte aligned rows only)
               : wlod_small                           ? Family::wlod_small_tiles
               : wlod_gl_strip                        ? Family::wlod_strip
               : wlod_gl_ring                         ? Family::wlod_glring
               : f.wlod_gl                            ? Family::wlod_tile_gl
               : !getenv("GARLIC_WLOD_ONE_BLOCK")     ? Family::wlod_tile2
                                                      : Family::wlod_tile;
    return GARLIC_OK;
}

// ... and what is known only once the score buffer is: the rows' alignment, and with it the last two choices
void finish_form(const garlic_panel *p, const LodCall &c, const Layout &L, const double *d_out, LodForm &f)
{
    f.aligned16 = (c.pitch_align % 2 == 0) && ((reinterpret_cast<uintptr_t>(d_out) & 15) == 0);
    if (f.family == Family::wlod_stream && !f.aligned16) f.family = Family::wlod_small_tiles;
    // scores into 16-B aligned rows at W <= 113: the 80-VGPR form, three workgroups per CU (wlod_strip_kernel.hpp)
    f.strip_three = f.family == Family::wlod_strip && f.strip_waves != WS_WAVES_WIDE && f.aligned16 && !f.cov_bits &&
                    !getenv("GARLIC_WLOD_STRIP_TWO_PER_CU");
    for (int k = 0; f.strip_three && k < p->nchr; k++) f.strip_three = L.pitch[k] * 8 < ((int64_t)1 << 32);
}

using Plan = garlic_panel::Plan;

// host side of a new plan, uploaded by enqueue_lod (a reused plan is on the device already)
struct LodWork {
    std::vector<Run> runs;
    std::vector<FillItem> fill;
    std::vector<ChainItem> items;
    std::vector<FeedItem> feed_items;
    std::vector<ChrDev> chrs;
    std::vector<uint8_t> valid;                    // tuned wLOD kernels: window mask, tiles, segments, strips
    std::vector<int2> tiles, segs;
    std::vector<WlodStrip> strips;
    std::vector<int32_t> feed_blocks;              // wlod_feed_kernel: the blocks in play (its column groups: tiles)
};

// persistent workgroups of lod_chain_kernel: one per CU (GARLIC_WORKERS: another count), no more than there are items
int chain_workers(const garlic_ctx *ctx, size_t n_items)
{
    int workers = ctx->n_cu;
    if (const char *e = getenv("GARLIC_WORKERS")) workers = std::max(1, atoi(e));
    return std::min<int>(workers, (int)n_items);
}

// Runs, chain / feed items, the wLOD kernels' tiles, segments and strips, the ChrDev table; room for them on the device.
int plan_lod(garlic_panel *p, const LodCall &c, const LodForm &form, const Layout &L, const garlic_panel::PlanKey &key, LodWork &w, Plan &plan)
{
    plan = Plan{false, key};
    const int nblk = (c.ind_count + WAVE - 1) / WAVE;
    int rc;
    p->plan.valid = false;
    plan_runs(p, c.W, w.runs, w.fill, plan.n_valid);
    // Work list: (run, 64-individual block) items, longest runs first (LPT); the persistent
    // workgroups of lod_chain_kernel pull them from a device counter.
    const std::vector<int> order = longest_first(w.runs);
    w.items.reserve(w.runs.size() * nblk);
    // TGLS term slabs: one list per slab, the lists one behind the other -- a slab begins at the next block in play and
    // spans slab_blocks consecutive blocks (the subset feed's skipped blocks get no items, a slab of nothing else no launch);
    // a chain launch sees its own slab's list and queue only, longest runs first inside it.  Otherwise one list over all blocks.
    // (The weighted kernels write MISSING themselves: their slabs are cut with no run to score too.)
    const bool wlod_slabs = form.slab_blocks && (form.wlod_tuned || form.family == Family::wlod_feed);
    const int per_list = form.slab_blocks ? form.slab_blocks : std::max(nblk, 1);
    for (int k0 = 0; k0 < nblk && (!w.runs.empty() || wlod_slabs); ) {
        if (c.blocks && !(*c.blocks)[(size_t)k0]) { k0++; continue; }
        const int k1 = std::min(nblk, k0 + per_list);
        const size_t item0 = w.items.size();
        for (size_t i = 0; i < order.size(); i++) {
            const Run &r = w.runs[order[i]];
            for (int k = k0; k < k1; k++)
                if (!c.blocks || (*c.blocks)[(size_t)k]) w.items.push_back(ChainItem{r.chr, r.a, r.b, k * WAVE});
        }
        if (form.slab_blocks) plan.slabs.push_back(Plan::Slab{c.ind_begin / WAVE + k0, c.ind_begin / WAVE + k1, item0, w.items.size() - item0});
        k0 = k1;
    }
    if (form.family == Family::chain && !form.slab_blocks) {
        // lod_chain_kernel's list: the order a simulated pass ends soonest in (host/chain_order.hpp; longest first unless
        // packing the items is simulated more than 1 % shorter) -- a function of the plan alone
        std::vector<int32_t> len(w.items.size());
        for (size_t i = 0; i < len.size(); i++) len[i] = w.items[i].b - w.items[i].a + 1;
        const std::vector<int> at = garlic_host::chainOrder(len, chain_workers(p->ctx, len.size()));
        std::vector<ChainItem> sorted(w.items.size());
        for (size_t i = 0; i < at.size(); i++) sorted[i] = w.items[(size_t)at[i]];
        w.items.swap(sorted);
    }
    if (form.family == Family::feed) {
        // the thinned score matrix: row = individual, column = locus / step
        std::vector<int32_t> col0(w.runs.size());
        for (size_t i = 0; i < w.runs.size(); i++) {
            const int32_t s = (w.runs[i].a + c.thin_step - 1) / c.thin_step;
            col0[i] = (int64_t)s * c.thin_step <= w.runs[i].b ? s : -1;
        }
        build_feed_items(w.runs, order, c.blocks, nblk, col0, w.feed_items);
        plan.n_feed_items = w.feed_items.size();
    }
    w.chrs.resize(p->nchr);
    for (int k = 0; k < p->nchr; k++)
        w.chrs[k] = ChrDev{p->chr_off[k], L.base[k], L.pitch[k], p->chr_nloci[k],
                           (c.pitch_align >= 2 && 64 * L.pitch[k] * 8 + 512 < ((int64_t)1 << 32)) ? 1 : 0};
    plan.n_items = w.items.size();
    plan.n_fill = w.fill.size();
    plan.n_runs = (int64_t)w.runs.size();
    // [0], [1]: the chain kernel's queue; [2]: sentinel_scan_kernel's flag; [3]: the strip kernel's stall flag;
    // [4]: strip launches repaired by the tile form since the panel was made (garlic_call_stats::n_stall_reruns)
    if (!p->d_counter.p) {
        if ((rc = p->d_counter.reserve(8))) return rc;
        HIP_TRY(hipMemsetAsync(p->d_counter.p, 0, 8 * sizeof(int32_t), p->ctx->stream));
    }
    if (form.wlod_tuned || form.family == Family::wlod_feed) {
        w.valid.assign((size_t)p->nloci, 0);
        for (const Run &r : w.runs)
            memset(w.valid.data() + p->chr_off[r.chr] + r.a, 1, (size_t)(r.b - r.a + 1));
    }
    if (form.family == Family::wlod_feed) {
        // WFD_COLS columns of the thinned matrix x the blocks in play
        for (int k = 0; k < p->nchr; k++) {
            const int32_t cols = (int32_t)(((int64_t)p->chr_nloci[k] + c.thin_step - 1) / c.thin_step);
            for (int32_t c0 = 0; c0 < cols; c0 += WFD_COLS) w.tiles.push_back(make_int2(k, c0));
        }
        plan.n_tiles = (int32_t)w.tiles.size();
        for (int k = 0; k < nblk; k++)
            if (!c.blocks || (*c.blocks)[(size_t)k]) w.feed_blocks.push_back(k);
        plan.n_feed_blocks = (int32_t)w.feed_blocks.size();
        // term slabs: the list is ascending, so a slab's blocks in play are one stretch of it (ind_begin is 0 here)
        size_t at = 0;
        for (Plan::Slab &sl : plan.slabs) {
            sl.fb0 = (int32_t)at;
            while (at < w.feed_blocks.size() && w.feed_blocks[at] < sl.b1) at++;
            sl.n_fb = (int32_t)at - sl.fb0;
        }
    }
    if (form.wlod_tuned) {
        for (int k = 0; k < p->nchr; k++)
            for (int s0 = 0; s0 < p->chr_nloci[k]; s0 += TILE) w.tiles.push_back(make_int2(k, s0));
        plan.n_tiles = (int32_t)w.tiles.size();
        for (int k = 0; k < p->nchr; k++)
            for (int s0 = 0; s0 < p->chr_nloci[k]; s0 += WSM_T) w.segs.push_back(make_int2(k, s0));
        plan.n_segs = (int32_t)w.segs.size();
    }
    if (form.family == Family::wlod_strip) {
        // strips of 16-window groups: long enough that filling and draining the workgroup's pipeline (~ 8 groups)
        // stays a few percent, short enough for a few thousand work items
        int64_t total_groups = 0;
        for (int k = 0; k < p->nchr; k++) total_groups += (p->chr_nloci[k] + WLOD_R - 1) / WLOD_R;
        const int64_t pairs = (nblk + 1) / 2;
        int64_t per = total_groups * pairs / 8192;
        per = std::min<int64_t>(256, std::max<int64_t>(64, per)) & ~(int64_t)1;
        if (const char *e = getenv("GARLIC_WLOD_STRIP_GROUPS")) per = std::max<int64_t>(1, atol(e));   // tests: many short strips
        for (int k = 0; k < p->nchr; k++) {
            const int ng = (p->chr_nloci[k] + WLOD_R - 1) / WLOD_R;
            for (int g0 = 0; g0 < ng; g0 += (int)per)
                w.strips.push_back(WlodStrip{k, g0 * WLOD_R, std::min<int>((int)per, ng - g0), 0});
        }
        plan.n_strips = (int32_t)w.strips.size();
    }
    return GARLIC_OK;
}

// Where the kernels write: the caller's device buffer, or the panel's scratch (host output).  A big unweighted scratch is placed first:
// candidates, the real kernel timed into each, the fastest kept (1.36 or 1.62 ms at 1M x 1000 by where the scores sit: DESIGN.md section 4).
int score_buffer(garlic_panel *p, const LodCall &c, const Layout &L, double **d_out)
{
    *d_out = c.out;
    if (c.where != GARLIC_HOST) return GARLIC_OK;
    int rc;
    if (p->d_out.cap < (size_t)L.total && c.mode == MODE_LOD && c.thin_step == 0 && !p->placing &&
        (size_t)L.total * sizeof(double) >= ((size_t)1 << 30) && !getenv("GARLIC_NO_PLACEMENT")) {
        p->placing = true;
        void *best = nullptr;
        rc = garlic_panel_alloc_scores(p, c.pitch_align, c.ind_count, c.W, c.error, c.max_gap, 0, &best, nullptr);
        p->placing = false;
        if (rc) return rc;
        p->d_out.adopt(p->ctx, best, (size_t)L.total);
    }
    if ((rc = p->d_out.reserve(p->ctx, (size_t)L.total))) return rc;
    *d_out = p->d_out.p;
    return GARLIC_OK;
}

// GARLIC_TRACE=<file>, a debugging aid: the per-item time stamps (cols each) a persistent kernel leaves are written there
struct ItemTrace {
    DevBuf<int64_t> d;
    const char *path = nullptr;
    const char *eol = "\n";
    size_t cols = 0, n = 0;
    int64_t *begin(size_t cols_, size_t n_, const char *eol_, hipStream_t s)     // NULL: no trace
    {
        path = getenv("GARLIC_TRACE");
        if (!path || d.reserve(cols_ * n_) != GARLIC_OK) return nullptr;
        cols = cols_;
        n = n_;
        eol = eol_;
        (void)hipMemsetAsync(d.p, 0, sizeof(int64_t) * cols * n, s);
        return d.p;
    }
    void write(hipStream_t s)      // after the launch
    {
        if (!n) return;
        std::vector<int64_t> tr(cols * n);
        (void)hipMemcpyAsync(tr.data(), d.p, sizeof(int64_t) * tr.size(), hipMemcpyDeviceToHost, s);
        (void)hipStreamSynchronize(s);
        if (FILE *fo = fopen(path, "w")) {
            for (size_t i = 0; i < n; i++) {
                fprintf(fo, "%zu", i);
                for (size_t q = 0; q < cols; q++) fprintf(fo, " %lld", (long long)tr[cols * i + q]);
                fputs(eol, fo);
            }
            fclose(fo);
        }
        d.release();
    }
};

// the context's event pair around a call's dominant kernels (garlic_recent_kernel_ms): its first event, or its second and on to the next pair
hipError_t hist_mark(garlic_ctx *ctx, bool end)
{
    const int slot = (int)(ctx->n_calls % garlic_ctx::HIST);
    if (end) ctx->n_calls++;
    return hipEventRecord(end ? ctx->hist1[slot] : ctx->hist0[slot], ctx->stream);
}

VariantArgs variant_args(const garlic_panel *p, const LodCall &c, const LodForm &form, double *d_out)
{
    return VariantArgs{p->d_packed.p, p->d_tab.p,  p->d_tabgl.p, p->d_codes.p, p->d_decay.p, p->d_rld.p,
                       p->d_items.p,  p->d_chrs.p, d_out,        p->nind_pad,  p->nwordrows, c.ind_begin,  c.ind_count,
                       c.W,           (int32_t)p->gl_values.size(), form.use_gl ? 1 : 0,
                       (form.use_gl && (p->gl_cont || p->gl_wide)) ? p->d_glterms.p : nullptr, (int64_t)(GOFF + p->nloci + GPAD_BACK)};
}

// the tile kernel of a family (the strip form's is the one that repairs it)
const void *wlod_tile_fn(Family family, bool gl, bool aligned16)
{
#define WLOD_FN(kernel) (aligned16 ? (const void *)kernel<WLOD_R, true> : (const void *)kernel<WLOD_R, false>)
    switch (family) {
    case Family::wlod_tile2: return WLOD_FN(wlod_tile2_kernel);
    case Family::wlod_tile_gl: return WLOD_FN(wlod_tile_gl_kernel);
    case Family::wlod_glring:
    case Family::wlod_strip: return WLOD_FN(wlod_tile_glring_kernel);
    case Family::wlod_small_tiles: return gl ? WLOD_FN(wlod_tile_small_gl_kernel) : WLOD_FN(wlod_tile_small_kernel);
    default: return WLOD_FN(wlod_tile_kernel);
    }
#undef WLOD_FN
}

// What a weighted launch reads its per-genotype scores from, and the individuals it covers: the whole scaled matrix and the
// whole call, or one slab [b0, b1) of it (blk0 = b0: the kernels count blocks from there, variant_kernels.hpp wlod_slab_first_block)
struct WlodTerms {
    const double *terms;
    int32_t blk0, ind_end, nblk;       // ind_end: one past the launch's last individual, counted from the call's ind_begin
};

WlodTerms wlod_terms_whole(const garlic_panel *p, const LodCall &c)
{
    return WlodTerms{p->d_glterms.p, 0, c.ind_count, (c.ind_count + WAVE - 1) / WAVE};
}

WlodTerms wlod_terms_slab(const LodCall &c, const Plan::Slab &sl, const double *terms)
{
    return WlodTerms{terms, sl.b0, std::min<int32_t>(c.ind_count, sl.b1 * WAVE - c.ind_begin), sl.b1 - sl.b0};
}

int launch_wlod(garlic_panel *p, const LodCall &c, const LodForm &form, const Plan &plan, double *d_out, const WlodTerms &t)
{
    hipStream_t s = p->ctx->stream;
    const int nblk = t.nblk;
    const int per_wg = form.family == Family::wlod_tile2 ? WLOD2_BLOCKS : WLOD_WAVES;
    const int nquad = (nblk + per_wg - 1) / per_wg;
    const bool gl_ring = form.family == Family::wlod_glring || form.family == Family::wlod_strip;
    const int64_t score_rows = GOFF + p->nloci + GPAD_BACK;
    WlodArgs a{p->d_valid.p, p->d_chrs.p, p->d_tiles.p, p->nwordrows, p->nchr, c.ind_begin, t.ind_end, c.W, nquad,
               (uint32_t)((int64_t)plan.n_tiles * nquad), (form.use_patch ? 1 : 0) | (form.no_prefetch ? 2 : 0),
               score_rows, gl_ring ? 1 : 0, p->cov_pending, nullptr, nullptr, t.blk0};
    const uint32_t *a_packed = p->d_packed.p;
    const double *a_wtab = form.wlod_gl ? t.terms : p->d_wtab.p, *a_skew = p->d_skew.p + SKEW_FRONT;
    const dim3 wl_block(WLOD_WAVES * WAVE);
    if (form.family == Family::wlod_stream) {
        // segments of WSM_T windows x eight blocks per workgroup, everything the window loop reads staged in LDS
        a.tiles = p->d_segs.p;
        a.nquad = (nblk + WLOD2_BLOCKS - 1) / WLOD2_BLOCKS;
        a.n_work = (uint32_t)((int64_t)plan.n_segs * a.nquad);
        a.use_patch = 1;
        const void *fn = form.wlod_gl ? wlod_stream_small_gl_fn(c.W) : wlod_stream_small_fn(c.W);
        const size_t lds = wlod_small_lds_bytes(c.W);
        if (lds > LDS_DEFAULT_MAX) HIP_TRY(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        const double *a_rld = p->d_rld.p;
        void *kargs[] = {(void *)&a_packed, (void *)&a_wtab, (void *)&a_rld, (void *)&d_out, (void *)&a};
        HIP_TRY(hipLaunchKernel(fn, dim3((a.n_work + 7u) / 8u * 8u), wl_block, kargs, lds, s));
        return GARLIC_OK;
    }
    if (form.family == Family::wlod_strip) {
        const int n_pairs = (nblk + 1) / 2;
        WlodStripArgs sa{p->d_valid.p, p->d_chrs.p, p->d_strips.p, t.terms, a_skew, d_out,
                         score_rows, c.ind_begin, t.ind_end, c.W, form.strip_waves, n_pairs,
                         form.use_patch ? 1 : 0, (uint32_t)((int64_t)plan.n_strips * n_pairs), p->d_counter.p + 3, p->cov_pending, t.blk0};
        HIP_TRY(hipMemsetAsync(p->d_counter.p + 3, 0, sizeof(int32_t), s));
        const void *fn = form.strip_three ? (const void *)wlod_strip_gl3_kernel
                         : form.strip_waves == WS_WAVES_WIDE ? (form.aligned16 ? (const void *)wlod_strip_gl_kernel<true, WS_WAVES_WIDE>
                                                  : (const void *)wlod_strip_gl_kernel<false, WS_WAVES_WIDE>)
                                : (form.aligned16 ? (const void *)wlod_strip_gl_kernel<true, WS_WAVES>
                                                  : (const void *)wlod_strip_gl_kernel<false, WS_WAVES>);
        const uint32_t strip_lds = form.strip_three ? WF_LDS_BYTES : WS_LDS_BYTES;
        HIP_TRY(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)strip_lds));
        void *kargs[] = {(void *)&sa};
        HIP_TRY(hipLaunchKernel(fn, dim3((sa.n_work + 7u) / 8u * 8u), dim3((form.strip_waves + 1) * WAVE), kargs, strip_lds, s));
        // A wave of the strip kernel that ran out of its poll budget flags the launch (its scores are wrong).  The tile
        // form, which computes the same values without waits between waves, is enqueued behind it (below) and runs only if
        // the flag is set -- on the device: no copy back, no synchronisation, the call stays asynchronous -- and
        // counts itself (garlic_call_stats::n_stall_reruns: expected 0; a liveness bug shows there, not as a slow call).
        // Over term slabs every slab's strip launch has its own reset of the flag and its own repair behind it, reading the
        // same slab: the buffer is released (for_each_tgls_slab) only behind both.
        if (form.strip_force_rerun) HIP_TRY(hipMemsetAsync(p->d_counter.p + 3, 1, sizeof(int32_t), s));
        a.run_if = p->d_counter.p + 3;
        a.rerun_count = p->d_counter.p + 4;
        p->reruns_stale = true;
    }
    const void *fn = wlod_tile_fn(form.family, form.wlod_gl, form.aligned16);
    if (form.tile_lds > LDS_DEFAULT_MAX) HIP_TRY(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)form.tile_lds));
    void *kargs[] = {(void *)&a_packed, (void *)&a_wtab, (void *)&a_skew, (void *)&d_out, (void *)&a};
    HIP_TRY(hipLaunchKernel(fn, dim3((a.n_work + 7u) / 8u * 8u), wl_block, kargs, form.tile_lds, s));
    return GARLIC_OK;
}

// the launch of lod_chain_kernel writes the plan's MISSING stretches itself: full scores of the unweighted chain with a run to
// score.  Every other family, and a plan with nothing to score (no chain launch), leaves them to fill_missing_kernel.
bool chain_takes_fill(const LodForm &form, const Plan &plan, Family family)
{
    return family == Family::chain && plan.n_items && plan.n_fill && !form.wlod_tuned && !form.cov_bits;
}

// unweighted --error scores: the persistent chain kernel, or for thinned output the feed kernel (its grid is chosen from a fresh plan)
int launch_chain(garlic_panel *p, const LodCall &c, const LodForm &form, Plan &plan, const LodWork *fresh, int workers, double *d_out)
{
    garlic_ctx *ctx = p->ctx;
    ItemTrace trace;
    if (form.family == Family::feed && plan.n_feed_items) {
        FeedArgs f{p->d_packed.p, p->d_tab.p, p->d_feed_items.p, p->d_chrs.p, d_out, nullptr, p->nwordrows, c.ind_begin, c.ind_count, c.W,
                   (int32_t)plan.n_feed_items, c.thin_step, form.feed_asm ? 1 : 0, p->d_counter.p, nullptr};
        f.trace = trace.begin(8, plan.n_feed_items, "\n", ctx->stream);
        int grid = (int)std::min<size_t>(plan.n_feed_items, (size_t)ctx->n_cu * std::max(1, plan.feed_per_cu)), rc;
        if (fresh && (rc = feed_grid(ctx, fresh->feed_items, &grid, &plan.feed_per_cu))) return rc;
        void *kargs[] = {(void *)&f};
        HIP_TRY(hipLaunchKernel((const void *)lod_feed_kernel, dim3((unsigned)grid), dim3(FEED_G * WAVE), kargs, 0, ctx->stream));
    } else {
        ChainArgs a{p->d_packed.p, p->d_tab.p, p->d_items.p,     p->d_chrs.p,          d_out, p->nind_pad, p->nwordrows,
                    c.ind_begin,   c.ind_count, c.W,             (int32_t)plan.n_items, p->d_counter.p, nullptr,
                    nullptr,       0};
        if (chain_takes_fill(form, plan, form.family)) {
            a.fill = p->d_fill.p;
            a.n_fill = (int32_t)plan.n_fill;
        }
        a.trace = trace.begin(4, plan.n_items, " 0\n", ctx->stream);      // (a fifth column of zeros: the readers of the chain trace expect it)
        if (form.aligned16)
            hipLaunchKernelGGL((lod_chain_kernel<true>), dim3((unsigned)workers), dim3(CHAIN_THREADS), 0, ctx->stream, a);
        else
            hipLaunchKernelGGL((lod_chain_kernel<false>), dim3((unsigned)workers), dim3(CHAIN_THREADS), 0, ctx->stream, a);
    }
    trace.write(ctx->stream);
    return GARLIC_OK;
}

// The ring chains over a term matrix that is never whole (garlic_panel_set_tgls_term_budget): per slab of the plan
// gl_terms_slab_kernel into one of two buffers on the panel's second stream, then the chain of that slab's items on the
// context's stream.  Events alone order them -- a chain waits for its slab's terms, a buffer is rebuilt once the chain
// that read it (two slabs back) has finished -- so the terms of slab k + 1 are built while the chain of slab k runs and
// every kernel can finish on its own.  Same kernels, same doubles as over the whole matrix.
//
// `chains(k, terms)` enqueues on the context's stream every chain that reads slab k (one per call of the single-size paths; one
// per group of window sizes for garlic_lod_feed_multi_tgls: a slab is built once and every group runs over it before its
// buffer is reused).
// scaled: the slabs hold (term * nomut) * norec of the panel's decay table (ensure_decay_table uploads it on the context's
// stream and waits; the term pass reads it on the second stream behind ev_slab_begin).
template <class Chains>
int for_each_tgls_slab(garlic_panel *p, const std::vector<Plan::Slab> &slabs, int32_t slab_blocks, Chains chains, bool scaled = false)
{
    garlic_ctx *ctx = p->ctx;
    hipStream_t s = ctx->stream;
    const int64_t rows = GOFF + p->nloci + GPAD_BACK;
    const size_t n_slabs = slabs.size();
    int rc;
    p->last_slab_blocks = slab_blocks;
    p->last_n_slabs = (int32_t)n_slabs;
    if (!n_slabs) return GARLIC_OK;
    if (!p->slab_stream) {
        HIP_TRY(hipStreamCreateWithFlags(&p->slab_stream, hipStreamNonBlocking));
        for (hipEvent_t *ev : {&p->ev_slab_begin, &p->ev_slab_built[0], &p->ev_slab_built[1], &p->ev_slab_read[0], &p->ev_slab_read[1]})
            HIP_TRY(hipEventCreateWithFlags(ev, hipEventDisableTiming));
    }
    // buffer q serves the slabs q, q + 2, ..: room for the largest of them (a change of plan that needs more waits for the stream first)
    for (int q = 0; q < 2; q++) {
        size_t blocks = 0;
        for (size_t k = (size_t)q; k < n_slabs; k += 2) blocks = std::max(blocks, (size_t)(slabs[k].b1 - slabs[k].b0));
        const size_t need = blocks * (size_t)rows * WAVE;
        if (need > p->d_slab[q].cap || (!need && p->d_slab[q].cap)) {
            HIP_TRY(hipStreamSynchronize(s));
            p->d_slab[q].release();
            if (need && (rc = p->d_slab[q].reserve(need))) return rc;
        }
    }
    // 16-bit codes: the slab's terms come from lod() on the table values (gl_terms_wide_kernel; the host where the device's
    // log10 is not the host's)
    const bool wide = p->gl_wide, wide_host = wide && tgls_terms_on_host(p);
    if (wide) {
        if ((rc = ensure_log10(p->ctx)) || (rc = ensure_dfreq(p)) || (rc = ensure_values16(p))) return rc;
        p->gl_terms_by = p->slab_terms_by = tgls_terms_on_host(p) ? 2 : 1;
    }
    // what the term pass reads (tables, codes, genotypes) was put on the context's stream
    HIP_TRY(hipEventRecord(p->ev_slab_begin, s));
    HIP_TRY(hipStreamWaitEvent(p->slab_stream, p->ev_slab_begin, 0));
    VariantArgs a{p->d_packed.p, nullptr, p->d_tabgl.p, p->d_codes.p, nullptr, nullptr, nullptr, nullptr, nullptr,
                  p->nind_pad, p->nwordrows, 0, 0, 0, (int32_t)p->gl_values.size(), 1, nullptr, 0};
    const size_t terms_lds = sizeof(double) * GL_TERMS_S * 4 * (size_t)a.ncodes;      // <= 64 KB (256 codes)
    if (!wide && terms_lds > LDS_DEFAULT_MAX)
        HIP_TRY(hipFuncSetAttribute((const void *)gl_terms_slab_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)terms_lds));
    const unsigned terms_grid = (unsigned)((p->nloci + GL_TERMS_S - 1) / GL_TERMS_S + (GL_PAD_ROWS + GL_TERMS_S - 1) / GL_TERMS_S);
    for (size_t k = 0; k < n_slabs; k++) {
        const Plan::Slab &sl = slabs[k];
        const int q = (int)(k & 1);
        if (k >= 2) HIP_TRY(hipStreamWaitEvent(p->slab_stream, p->ev_slab_read[q], 0));
        if (wide_host) {
            if ((rc = build_wide_terms_on_host(p, sl.b0, sl.b1, scaled ? p->h_decay.data() : nullptr, p->d_slab[q].p, p->slab_stream, nullptr)))
                return rc;
        } else if (wide)
            launch_wide_terms(p, sl.b0, sl.b1, scaled ? p->d_decay.p : nullptr, p->d_slab[q].p, nullptr, p->slab_stream);
        else
        hipLaunchKernelGGL(gl_terms_slab_kernel, dim3(terms_grid), dim3(256), terms_lds, p->slab_stream, a, p->nloci, rows, sl.b0, sl.b1,
                           scaled ? p->d_decay.p : (const double *)nullptr, p->d_slab[q].p);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipEventRecord(p->ev_slab_built[q], p->slab_stream));
        HIP_TRY(hipStreamWaitEvent(s, p->ev_slab_built[q], 0));
        if ((rc = chains(k, (const double *)p->d_slab[q].p))) return rc;
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipEventRecord(p->ev_slab_read[q], s));
    }
    return GARLIC_OK;
}

// persistent workgroups of a ring chain: one per CU (GARLIC_WORKERS: another count), no more than there are items
int tgls_workers(const garlic_ctx *ctx, size_t n_items)
{
    int workers = ctx->n_cu;
    if (const char *e = getenv("GARLIC_WORKERS")) workers = std::max(1, atoi(e));
    return std::min<int>(workers, (int)n_items);
}

int launch_tgls_slabs(garlic_panel *p, const LodCall &c, const LodForm &form, const Plan &plan, double *d_out)
{
    hipStream_t s = p->ctx->stream;
    const int64_t rows = GOFF + p->nloci + GPAD_BACK;
    const size_t n_slabs = plan.slabs.size();
    int rc;
    if (n_slabs) {
        if ((rc = p->d_slab_queues.reserve(2 * n_slabs))) return rc;
        HIP_TRY(hipMemsetAsync(p->d_slab_queues.p, 0, 2 * n_slabs * sizeof(int32_t), s));
        if (form.cov_bits) p->cov_written = true;
    }
    return for_each_tgls_slab(p, plan.slabs, form.slab_blocks, [&](size_t k, const double *terms) {
        const Plan::Slab &sl = plan.slabs[k];
        const int workers = tgls_workers(p->ctx, sl.n_items);
        if (form.family == Family::tgls_feed) {
            TglsFeedArgs t{terms, rows, p->d_items.p + sl.item0, p->d_chrs.p, d_out,
                           c.ind_begin, c.ind_count, c.W, (int32_t)sl.n_items, c.thin_step, sl.b0, p->d_slab_queues.p + 2 * k};
            hipLaunchKernelGGL(tgls_feed_kernel, dim3((unsigned)workers), dim3(TGF_THREADS), 0, s, t);
        } else {
            TglsArgs t{terms, rows, p->d_items.p + sl.item0, p->d_chrs.p, d_out,
                       c.ind_begin, c.ind_count, c.W, (int32_t)sl.n_items, sl.b0, p->d_slab_queues.p + 2 * k, p->cov_pending};
            hipLaunchKernelGGL(lod_chain_ring_kernel, dim3((unsigned)workers), dim3(TG_THREADS), 0, s, t);
        }
        return (int)GARLIC_OK;
    });
}

int launch_tgls(garlic_panel *p, const LodCall &c, const LodForm &form, const Plan &plan, int workers, double *d_out)
{
    hipStream_t s = p->ctx->stream;
    const int64_t rows = GOFF + p->nloci + GPAD_BACK;
    if (form.cov_bits && !form.writes_bits) return GARLIC_INTERNAL_NO_BITS;      // only the ring chain takes this shape
    p->last_slab_blocks = p->last_n_slabs = 0;
    if (form.slab_blocks && (form.family == Family::tgls_feed || form.family == Family::tgls_ring))
        return launch_tgls_slabs(p, c, form, plan, d_out);
    if (form.family == Family::tgls_feed) {
        // the same ring chain storing the sampled windows only, into the thinned matrix (tgls_feed_kernel.hpp)
        TglsFeedArgs t{p->d_glterms.p, rows, p->d_items.p, p->d_chrs.p, d_out,
                       c.ind_begin, c.ind_count, c.W, (int32_t)plan.n_items, c.thin_step, 0, p->d_counter.p};
        hipLaunchKernelGGL(tgls_feed_kernel, dim3((unsigned)workers), dim3(TGF_THREADS), 0, s, t);
        return GARLIC_OK;
    }
    if (form.family == Family::tgls_ring) {
        // persistent workgroups, every term row through an LDS ring once (tgls_ring_kernel.hpp)
        TglsArgs t{p->d_glterms.p, rows, p->d_items.p, p->d_chrs.p, d_out,
                   c.ind_begin, c.ind_count, c.W, (int32_t)plan.n_items, 0, p->d_counter.p, p->cov_pending};
        if (form.cov_bits) p->cov_written = true;
        hipLaunchKernelGGL(lod_chain_ring_kernel, dim3((unsigned)workers), dim3(TG_THREADS), 0, s, t);
        return GARLIC_OK;
    }
    const VariantArgs a = variant_args(p, c, form, d_out);
    if (form.family == Family::tgls_terms)
        hipLaunchKernelGGL(lod_chain_terms_kernel, dim3((unsigned)plan.n_items), dim3(2 * WAVE), 0, s, a, (int)plan.n_items, rows, p->d_glterms.p);
    else
        hipLaunchKernelGGL(lod_chain_gl_kernel, dim3((unsigned)((plan.n_items + GL_WAVES - 1) / GL_WAVES)), dim3(GL_WAVES * WAVE), 0, s, a,
                           (int)plan.n_items);
    return GARLIC_OK;
}

int launch_generic_wlod(garlic_panel *p, const LodCall &c, const LodForm &form, const Plan &plan, double *d_out)
{
    const int ring = c.W + TILE;
    const size_t lds = sizeof(double) * ((size_t)ring * WAVE + ((c.W + 1) & ~1) + (size_t)WAVE * TPITCH);
    if (lds > 160 * 1024)
        return fail(GARLIC_ERR_INVALID, "wLOD with winsize %d: this build supports 2..240 and 16..4096", c.W);
    HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(wlod_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(wlod_kernel, dim3((unsigned)plan.n_items), dim3(WAVE), lds, p->ctx->stream, variant_args(p, c, form, d_out), ring);
    return GARLIC_OK;
}

// weighted scores, thinned output: the sampled windows only (wlod_feed_kernel.hpp)
// fb0, n_fb: the launch's stretch of the plan's blocks in play (all of them, or those of the slab t)
int launch_wlod_feed(garlic_panel *p, const LodCall &c, const LodForm &form, const Plan &plan, double *d_out, const WlodTerms &t,
                     int32_t fb0, int32_t n_fb)
{
    const int nquad = (n_fb + WFD_WAVES - 1) / WFD_WAVES;
    WlodFeedArgs a{p->d_packed.p, form.wlod_gl ? t.terms : p->d_wtab.p, p->d_skew.p + SKEW_FRONT, p->d_valid.p, p->d_chrs.p,
                   p->d_tiles.p, p->d_feed_blocks.p + fb0, d_out, p->nwordrows, GOFF + p->nloci + GPAD_BACK, c.ind_count, c.W, c.thin_step,
                   n_fb, nquad, (uint32_t)((int64_t)plan.n_tiles * nquad), t.blk0};
    if (!a.n_work) return GARLIC_OK;
    if (form.wlod_gl) hipLaunchKernelGGL(wlod_feed_kernel<true>, dim3(a.n_work), dim3(WFD_WAVES * WAVE), 0, p->ctx->stream, a);
    else hipLaunchKernelGGL(wlod_feed_kernel<false>, dim3(a.n_work), dim3(WFD_WAVES * WAVE), 0, p->ctx->stream, a);
    return GARLIC_OK;
}

// The weighted kernels over a term matrix that is never whole: per slab of the plan a scaled slab (for_each_tgls_slab), then the
// call's kernel over that slab's individuals -- for the strip form with the tile form that repairs it behind it
int launch_wlod_slabs(garlic_panel *p, const LodCall &c, const LodForm &form, const Plan &plan, double *d_out)
{
    return for_each_tgls_slab(p, plan.slabs, form.slab_blocks, [&](size_t k, const double *terms) {
        const Plan::Slab &sl = plan.slabs[k];
        const WlodTerms t = wlod_terms_slab(c, sl, terms);
        if (form.family == Family::wlod_feed) return launch_wlod_feed(p, c, form, plan, d_out, t, sl.fb0, sl.n_fb);
        return launch_wlod(p, c, form, plan, d_out, t);
    }, /*scaled=*/true);
}

// Everything a call puts on the stream (a second time, as Family::exact, when the rescan found a -9999.0).  (Replaying a repeated
// asynchronous pass as one HIP graph -- counter reset, MISSING fill, chain kernel, events -- was measured: no difference, the
// 1.6 ms kernel hides the launch gaps of the small operations once passes are enqueued back to back.)
// one_kernel: the pass is the chain kernel and nothing else (launch_lod); the event pair around it times the call too
int enqueue_lod(garlic_panel *p, const LodCall &c, const LodForm &form, const Layout &L, Plan &plan, const LodWork *fresh,
                double *d_out, Family family, bool one_kernel = false)
{
    garlic_ctx *ctx = p->ctx;
    hipStream_t s = ctx->stream;
    int rc = GARLIC_OK;
    if (!one_kernel) HIP_TRY(hipEventRecord(ctx->ev_begin, s));
    if (fresh && ((rc = p->d_chrs.put(fresh->chrs, s)) || (rc = p->d_items.put(fresh->items, s)) || (rc = p->d_fill.put(fresh->fill, s)) ||
                  (rc = p->d_feed_items.put(fresh->feed_items, s)) || (rc = p->d_valid.put(fresh->valid, s)) ||
                  (rc = p->d_tiles.put(fresh->tiles, s)) || (rc = p->d_segs.put(fresh->segs, s)) || (rc = p->d_strips.put(fresh->strips, s)) ||
                  (rc = p->d_feed_blocks.put(fresh->feed_blocks, s))))
        return rc;
    if (family == Family::feed || family == Family::tgls_feed) {          // small matrix: MISSING everywhere, the chain kernel overwrites the scored samples
        hipLaunchKernelGGL(fill_value_kernel, dim3(1024), dim3(256), 0, s, d_out, L.total, MISSING_D);
    } else if (plan.n_fill && !form.wlod_tuned && family != Family::wlod_feed && !form.cov_bits &&
               !chain_takes_fill(form, plan, family)) {   // the tuned and the sampled wLOD kernels and the chain kernel write MISSING themselves
        dim3 grid((unsigned)plan.n_fill, (unsigned)((c.ind_count + FILL_ROWS - 1) / FILL_ROWS));
        hipLaunchKernelGGL(fill_missing_kernel, grid, dim3(256), 0, s, p->d_fill.p, p->d_chrs.p, c.ind_count, d_out);
    }
    // queue head and exit count of the persistent chain kernel: its last workgroup leaves both at
    // zero, so only a new plan (or a first call) clears them
    if (plan.n_items && (fresh || c.mode != MODE_LOD)) HIP_TRY(hipMemsetAsync(p->d_counter.p, 0, 2 * sizeof(int32_t), s));
    p->stats_slot = (int)(ctx->n_calls % garlic_ctx::HIST);
    HIP_TRY(hist_mark(ctx, false));
    // Persistent workgroups (4 waves each: CHAIN, POST, PRE, COMB), one per CU; items are pulled longest
    // first, so the short runs pack behind the long ones instead of competing with them for HBM
    // bandwidth.
    const int workers = chain_workers(ctx, plan.n_items);
    if (form.wlod_tuned || plan.n_items || family == Family::wlod_feed)
        switch (family) {
        case Family::chain:
        case Family::feed: rc = launch_chain(p, c, form, plan, fresh, workers, d_out); break;
        case Family::exact:
            hipLaunchKernelGGL(lod_chain_exact_kernel, dim3((unsigned)plan.n_items), dim3(WAVE), 0, s, variant_args(p, c, form, d_out),
                               (int)plan.n_items);
            break;
        case Family::tgls_ring:
        case Family::tgls_feed:
        case Family::tgls_terms:
        case Family::tgls_lookup: rc = launch_tgls(p, c, form, plan, workers, d_out); break;
        case Family::wlod_generic: rc = launch_generic_wlod(p, c, form, plan, d_out); break;
        case Family::wlod_feed:
            rc = form.slab_blocks ? launch_wlod_slabs(p, c, form, plan, d_out)
                                  : launch_wlod_feed(p, c, form, plan, d_out, wlod_terms_whole(p, c), 0, plan.n_feed_blocks);
            break;
        default:
            rc = form.slab_blocks ? launch_wlod_slabs(p, c, form, plan, d_out) : launch_wlod(p, c, form, plan, d_out, wlod_terms_whole(p, c));
        }
    if (rc) return rc;
    HIP_TRY(hist_mark(ctx, true));
    HIP_TRY(hipGetLastError());
    return GARLIC_OK;
}

// thin_step > 0 (device output of the whole panel, pitch_align 32 only): `out` is the thinned matrix
// of make_layout(p, 32, ind_count, thin_step) -- the feed kernels store only the windows at loci
// 0, thin_step, 2 * thin_step, .. of each chromosome, everything else of that matrix is MISSING.  A weighted or TGLS call
// that no kernel with thinned output takes returns GARLIC_INTERNAL_NO_SAMPLED with nothing written.
// blocks (chain and feed kernels only): per 64-individual block of the call, 1 = score it; rows of the other
// blocks are left unwritten (the subset feed never reads them)
int launch_lod(garlic_panel *p, Mode mode, int32_t W, double error, int32_t max_gap, int32_t M, double mu,
               int32_t ind_begin, int32_t ind_count, int32_t pitch_align, double *out, int32_t where,
               int32_t thin_step = 0, const std::vector<uint8_t> *blocks = nullptr)
{
    garlic_ctx *ctx = p->ctx;
    int rc;
    ++*p->scratch_gen;
    if ((rc = set_device(ctx))) return rc;
    // Host output: the device always computes into the padded layout the tuned kernels need; the
    // rows are copied out into the caller's (possibly dense) layout by strided D2H copies.
    const LodCall c{mode, W, max_gap, M, ind_begin, ind_count, where == GARLIC_HOST ? std::max(pitch_align, 32) : pitch_align,
                    thin_step, where, pitch_align, error, mu, out, blocks};
    LodForm form;
    if ((rc = check_lod_args(p, c)) || (rc = decide_form(p, c, form))) return rc;
    if (form.use_gl) p->last_slab_blocks = p->last_n_slabs = 0;      // (for_each_tgls_slab sets them)
    const Layout Lhost = make_layout(p, pitch_align, ind_count), L = make_layout(p, c.pitch_align, ind_count, thin_step);
    for (int k = 0; k < p->nchr; k++)
        if (3 * L.pitch[k] * 8 + 512 >= (int64_t)1 << 32)
            return fail(GARLIC_ERR_INVALID, "chromosome %d too long for 32-bit row offsets", k);
    double *d_out = nullptr;
    if ((rc = score_buffer(p, c, L, &d_out))) return rc;
    finish_form(p, c, L, d_out, form);

    garlic_panel::PlanKey key{(int)mode, W, max_gap, ind_begin, ind_count, c.pitch_align, thin_step, 0, form.wlod_tuned,
                form.family == Family::wlod_strip, thin_step > 0, form.slab_blocks};
    if (blocks) {
        key.blocks_hash = 0xCBF29CE484222325ull;
        for (uint8_t b : *blocks) key.blocks_hash = (key.blocks_hash ^ (b ? 1u : 2u)) * 0x100000001B3ull;
        key.blocks_hash |= 1;
    }
    const bool reuse = p->plan.valid && p->plan.key == key;
    Plan plan = p->plan;
    LodWork work;
    if (!reuse && (rc = plan_lod(p, c, form, L, key, work, plan))) return rc;

    // A repeated asynchronous pass of the unweighted chain is one kernel between one pair of events: no fill launch (the chain
    // kernel writes the MISSING stretches), no counter reset, no rescan -- and the call's own pair of events, which would
    // bracket the same kernel, is not recorded (garlic_last_call_stats reads both times from the one pair)
    const bool one_kernel = ctx->async_device && where == GARLIC_DEVICE && reuse && mode == MODE_LOD && form.family == Family::chain &&
                            plan.n_items && (!plan.n_fill || chain_takes_fill(form, plan, form.family)) && !form.exact_possible;
    if ((rc = enqueue_lod(p, c, form, L, plan, reuse ? nullptr : &work, d_out, form.family, one_kernel))) return rc;
    p->last_chain_kind = form.family == Family::exact ? 2 : 0;
    if (form.exact_possible && form.family != Family::exact && plan.n_items) {
        // the reference tests "no score" by value: did a scored window of the tuned chain come out as exactly -9999.0?
        int32_t found = 0;
        HIP_TRY(hipMemsetAsync(p->d_counter.p + 2, 0, sizeof(int32_t), ctx->stream));
        hipLaunchKernelGGL(sentinel_scan_kernel, dim3((unsigned)plan.n_items), dim3(256), 0, ctx->stream, p->d_items.p, p->d_chrs.p,
                           d_out, ind_count, p->d_counter.p + 2);
        HIP_TRY(hipMemcpyAsync(&found, p->d_counter.p + 2, sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(hipStreamSynchronize(ctx->stream));
        p->last_chain_kind = found ? 2 : 1;
        if (found && form.use_gl && p->gl_wide && !(p->glterms_valid && !p->glterms_scaled && p->d_glterms.p))
            return fail(GARLIC_ERR_NOMEM, "16-bit likelihood codes: a window sums to exactly -9999.0 and the by-value chain needs the "
                                          "whole term matrix, which the term budget does not admit");
        if (found && (rc = enqueue_lod(p, c, form, L, plan, reuse ? nullptr : &work, d_out, Family::exact))) return rc;
    }
    if (where == GARLIC_HOST)
        for (int k = 0; k < p->nchr; k++)
            HIP_TRY(hipMemcpy2DAsync(out + Lhost.base[k], sizeof(double) * Lhost.pitch[k], d_out + L.base[k],
                                     sizeof(double) * L.pitch[k], sizeof(double) * p->chr_nloci[k],
                                     (size_t)ind_count, hipMemcpyDeviceToHost, ctx->stream));
    if (!one_kernel) HIP_TRY(hipEventRecord(ctx->ev_end, ctx->stream));
    // The work list lives in host vectors and per-panel device scratch: finish before returning --
    // unless the context is asynchronous, the output stays on the device and the plan (already
    // resident) is being reused: then nothing on the host is needed again and the call only enqueues.
    const bool enqueue_only = ctx->async_device && where == GARLIC_DEVICE && reuse;
    if (!enqueue_only) HIP_TRY(hipStreamSynchronize(ctx->stream));
    p->stats_pending = true;
    p->stats_one_kernel = one_kernel;
    plan.valid = true;
    p->plan = plan;

    garlic_call_stats &st = p->stats;
    st.n_segments = (int64_t)p->boundaries.size();
    st.n_runs = plan.n_runs;
    st.n_chain_items = (int64_t)plan.n_items;
    st.n_valid_windows = plan.n_valid;
    st.n_missing = p->nloci - plan.n_valid;
    return GARLIC_OK;
}

} // namespace

// =================================================================================== C ABI
extern "C" {

int garlic_hip_abi_version(void) { return GARLIC_HIP_ABI_VERSION; }

const char *garlic_hip_last_error(void) { return g_last_error.c_str(); }

int garlic_hip_device_count(int32_t *count)
{
    if (!count) return fail(GARLIC_ERR_INVALID, "count is NULL");
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess) {
        *count = 0;
        return fail(GARLIC_ERR_HIP, "hipGetDeviceCount: %s", hipGetErrorString(e));
    }
    *count = n;
    return GARLIC_OK;
}

int garlic_ctx_create(int32_t device, void *hip_stream, garlic_ctx **out)
{
    if (!out) return fail(GARLIC_ERR_INVALID, "ctx out pointer is NULL");
    *out = nullptr;
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n < 1)
        return fail(GARLIC_ERR_HIP, "no HIP device available (%s); libgarlic_hip has no CPU path",
                    e == hipSuccess ? "device count 0" : hipGetErrorString(e));
    if (device < 0 || device >= n)
        return fail(GARLIC_ERR_INVALID, "device %d out of range (have %d)", device, n);
    HIP_TRY(hipSetDevice(device));
    hipDeviceProp_t prop;
    HIP_TRY(hipGetDeviceProperties(&prop, device));
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return fail(GARLIC_ERR_HIP, "device %d is %s; this library is built for gfx950 only", device,
                    prop.gcnArchName);
    garlic_ctx *ctx = new garlic_ctx;
    ctx->device = device;
    ctx->n_cu = std::max(1, prop.multiProcessorCount);   // a partitioned device (CPX / DPX) shows 32-128 of the 256
    if (hip_stream) {
        ctx->stream = reinterpret_cast<hipStream_t>(hip_stream);
    } else {
        hipError_t se = hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking);
        if (se != hipSuccess) {
            delete ctx;
            return fail(GARLIC_ERR_HIP, "hipStreamCreate: %s", hipGetErrorString(se));
        }
        ctx->own_stream = true;
    }
    hipEvent_t *evs[2] = {&ctx->ev_begin, &ctx->ev_end};
    for (auto ev : evs) {
        hipError_t ee = hipEventCreate(ev);
        if (ee != hipSuccess) {
            delete ctx;
            return fail(GARLIC_ERR_HIP, "hipEventCreate: %s", hipGetErrorString(ee));
        }
    }
    for (int i = 0; i < garlic_ctx::HIST; i++)
        if (hipEventCreate(&ctx->hist0[i]) != hipSuccess || hipEventCreate(&ctx->hist1[i]) != hipSuccess) {
            (void)garlic_ctx_destroy(ctx);
            return fail(GARLIC_ERR_HIP, "hipEventCreate failed");
        }
    *out = ctx;
    return GARLIC_OK;
}

int garlic_ctx_destroy(garlic_ctx *ctx)
{
    if (!ctx) return GARLIC_OK;
    (void)hipSetDevice(ctx->device);
    (void)hipStreamSynchronize(ctx->stream);
    for (hipEvent_t ev : {ctx->ev_begin, ctx->ev_end})
        if (ev) (void)hipEventDestroy(ev);
    for (int i = 0; i < garlic_ctx::HIST; i++) {
        if (ctx->hist0[i]) (void)hipEventDestroy(ctx->hist0[i]);
        if (ctx->hist1[i]) (void)hipEventDestroy(ctx->hist1[i]);
    }
    ctx->d_logtab.release();
    if (ctx->own_stream) (void)hipStreamDestroy(ctx->stream);
    delete ctx;
    return GARLIC_OK;
}

int garlic_ctx_synchronize(garlic_ctx *ctx)
{
    if (!ctx) return fail(GARLIC_ERR_INVALID, "ctx is NULL");
    HIP_TRY(hipSetDevice(ctx->device));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return GARLIC_OK;
}

int garlic_panel_create(garlic_ctx *ctx, int32_t nchr, const int32_t *chr_nloci, int32_t nind,
                        garlic_panel **out)
{
    if (!out) return fail(GARLIC_ERR_INVALID, "panel out pointer is NULL");
    *out = nullptr;
    if (!ctx) return fail(GARLIC_ERR_INVALID, "ctx is NULL");
    // initWinData refuses nind < 1 or nloci < 1 (src/garlic-data.cpp:1610-1620)
    if (nchr < 1 || !chr_nloci || nind < 1)
        return fail(GARLIC_ERR_INVALID, "need nchr >= 1, chr_nloci and nind >= 1");
    int rc;
    if ((rc = set_device(ctx))) return rc;
    garlic_panel *p = new garlic_panel;
    p->ctx = ctx;
    p->nchr = nchr;
    p->nind = nind;
    p->chr_nloci.assign(chr_nloci, chr_nloci + nchr);
    p->chr_off.resize(nchr + 1);
    p->chr_off[0] = 0;
    for (int c = 0; c < nchr; c++) {
        if (chr_nloci[c] < 1) {
            delete p;
            return fail(GARLIC_ERR_INVALID, "chromosome %d has %d loci; must be positive", c,
                        chr_nloci[c]);
        }
        p->chr_off[c + 1] = p->chr_off[c] + chr_nloci[c];
    }
    p->nloci = p->chr_off[nchr];
    p->nind_pad = ((int64_t)nind + 63 + 63) / 64 * 64;
    p->nwordrows = ((((GOFF + p->nloci + GPAD_BACK) >> 4) + 2) + 15) & ~(int64_t)15; // whole 4 KB chunks
    auto cleanup = [&](int code) { garlic_panel_destroy(p); return code; };
    if ((rc = p->d_packed.reserve((size_t)(p->nwordrows * p->nind_pad)))) return cleanup(rc);
    if ((rc = p->d_chr_off.reserve(nchr + 1))) return cleanup(rc);
    // every 2-bit code starts out "missing" (3): pad rows/columns contribute +0.0 and are never stored
    hipLaunchKernelGGL(fill_u32_kernel, dim3(2048), dim3(256), 0, ctx->stream, p->d_packed.p,
                       p->nwordrows * p->nind_pad, 0xFFFFFFFFu);
    hipError_t e = hipMemcpyAsync(p->d_chr_off.p, p->chr_off.data(), sizeof(int64_t) * (nchr + 1),
                                  hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess)
        return cleanup(fail(GARLIC_ERR_HIP, "panel init: %s", hipGetErrorString(e)));
    *out = p;
    return GARLIC_OK;
}

static void release_feed_slots(garlic_panel *p)
{
    for (auto *sl : p->feed_slots) {
        if (sl->stream) { (void)hipStreamSynchronize(sl->stream); (void)hipStreamDestroy(sl->stream); }
        if (sl->ev0) (void)hipEventDestroy(sl->ev0);
        if (sl->ev1) (void)hipEventDestroy(sl->ev1);
        delete sl;
    }
    p->feed_slots.clear();
}

int garlic_panel_destroy(garlic_panel *p)
{
    if (!p) return GARLIC_OK;
    (void)hipSetDevice(p->ctx->device);
    (void)hipStreamSynchronize(p->ctx->stream);
    ++*p->scratch_gen;
    p->d_out.release();
    release_feed_slots(p);
    if (p->slab_stream) {
        (void)hipStreamSynchronize(p->slab_stream);
        for (hipEvent_t ev : {p->ev_slab_begin, p->ev_slab_built[0], p->ev_slab_built[1], p->ev_slab_read[0], p->ev_slab_read[1]})
            if (ev) (void)hipEventDestroy(ev);
        (void)hipStreamDestroy(p->slab_stream);
    }
    delete p;      // (its DevBuf members free themselves: the device is set and the stream idle)
    return GARLIC_OK;
}

int garlic_panel_set_map(garlic_panel *p, const int32_t *pos, const double *gpos,
                         const int32_t *centro_start, const int32_t *centro_end)
{
    if (!p || !pos || !centro_start || !centro_end)
        return fail(GARLIC_ERR_INVALID, "panel, pos, centro_start and centro_end are required");
    int rc;
    if ((rc = set_device(p->ctx))) return rc;
    p->pos.assign(pos, pos + p->nloci);
    p->cs.assign(centro_start, centro_start + p->nchr);
    p->ce.assign(centro_end, centro_end + p->nchr);
    p->have_gpos = gpos != nullptr;
    if (gpos) p->gpos.assign(gpos, gpos + p->nloci);
    if ((rc = p->d_pos.reserve((size_t)p->nloci))) return rc;
    if ((rc = p->d_cs.reserve(p->nchr))) return rc;
    if ((rc = p->d_ce.reserve(p->nchr))) return rc;
    hipStream_t s = p->ctx->stream;
    HIP_TRY(hipMemcpyAsync(p->d_pos.p, pos, sizeof(int32_t) * p->nloci, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(p->d_cs.p, centro_start, sizeof(int32_t) * p->nchr, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(p->d_ce.p, centro_end, sizeof(int32_t) * p->nchr, hipMemcpyHostToDevice, s));
    HIP_TRY(hipStreamSynchronize(s));
    p->have_map = true;
    p->seg_valid = false;
    p->decay_valid = false;
    p->plan.valid = false;
    if (p->glterms_scaled) p->glterms_valid = false;   // (term * nomut) * norec of the old positions
    return GARLIC_OK;
}

int garlic_panel_set_freq(garlic_panel *p, const double *freq)
{
    if (!p || !freq) return fail(GARLIC_ERR_INVALID, "panel and freq are required");
    p->freq.assign(freq, freq + p->nloci);
    p->wide_bound_known = false;
    p->have_freq = true;
    p->tab_valid = false;
    p->tabgl_valid = false;
    p->glterms_valid = false;
    p->dfreq_valid = false;
    return GARLIC_OK;
}

int garlic_panel_set_genotypes(garlic_panel *p, const int16_t *geno, int64_t ld, int64_t locus_begin,
                               int64_t locus_count, int32_t where)
{
    if (!p || !geno) return fail(GARLIC_ERR_INVALID, "panel and geno are required");
    int rc;
    if ((rc = check_rows(p, ld, locus_begin, locus_count)) || (rc = set_device(p->ctx))) return rc;
    hipStream_t s = p->ctx->stream;
    // (the staging buffer stays with the panel until garlic_panel_release_scratch)
    rc = for_each_upload_slab(s, "set_genotypes", geno, 2 * ld, locus_count, where, p->d_stage16, [&](const void *rows, int64_t at, int64_t n) {
        const int64_t l0 = locus_begin + at;
        const int64_t w_lo = (GOFF + l0) >> 4;
        const int64_t w_hi = ((GOFF + l0 + n - 1) >> 4) + 1;
        for (int64_t w = w_lo; w < w_hi; w += 65535) {
            const int64_t wn = std::min<int64_t>(65535, w_hi - w);
            dim3 grid((unsigned)((p->nind_pad + 255) / 256), (unsigned)wn);
            hipLaunchKernelGGL(pack_genotypes_kernel, grid, dim3(256), 0, s, (const int16_t *)rows, ld, l0, n, p->nind,
                               p->nind_pad, p->nwordrows, p->d_packed.p, w, w + wn);
        }
        return GARLIC_OK;
    });
    if (rc) return rc;
    p->have_geno = true;
    p->geno_epoch++;
    p->glterms_valid = false;
    return GARLIC_OK;
}

int garlic_panel_set_genotypes_2bit(garlic_panel *p, const uint8_t *rows, int64_t row_bytes, int64_t ind_offset,
                                    int64_t locus_begin, int64_t locus_count, int32_t where)
{
    if (!p || !rows) return fail(GARLIC_ERR_INVALID, "panel and rows are required");
    if (ind_offset < 0 || row_bytes < (ind_offset + p->nind + 3) / 4)
        return fail(GARLIC_ERR_INVALID, "row_bytes %lld too small for individuals [%lld,+%d)", (long long)row_bytes,
                    (long long)ind_offset, p->nind);
    int rc;
    if ((rc = check_loci(p, locus_begin, locus_count)) || (rc = set_device(p->ctx))) return rc;
    hipStream_t s = p->ctx->stream;
    DevBuf<uint8_t> stage;
    rc = for_each_upload_slab(s, "set_genotypes_2bit", rows, row_bytes, locus_count, where, stage, [&](const void *src, int64_t at, int64_t n) {
        const int64_t l0 = locus_begin + at;
        const int64_t w_lo = (GOFF + l0) >> 4;
        const int64_t w_hi = ((GOFF + l0 + n - 1) >> 4) + 1;
        for (int64_t w = w_lo; w < w_hi; w += 65535) {
            const int64_t wn = std::min<int64_t>(65535, w_hi - w);
            dim3 grid((unsigned)((p->nind_pad + 255) / 256), (unsigned)wn);
            hipLaunchKernelGGL(pack_genotypes_2bit_kernel, grid, dim3(256), 0, s, (const uint8_t *)src, row_bytes, ind_offset, l0, n,
                               p->nind, p->nind_pad, p->nwordrows, p->d_packed.p, w, w + wn);
        }
        return GARLIC_OK;
    });
    if (rc) return rc;
    p->have_geno = true;
    p->geno_epoch++;
    p->glterms_valid = false;
    return GARLIC_OK;
}

// ---- What the text doors share (text_line.hpp): garlic_bed_set_rows_vcf, garlic_bed_set_rows_tped, garlic_tgls_set_rows_text
// and garlic_tgls_set_rows_vcf take a slab of text and line_begin[row_count + 1] and answer with a status pair per line.
struct TextStage {
    DevBuf<uint8_t> text;                                   // staging, kept until the object's destroy: a host slab,
    DevBuf<int64_t> lines;                                  // its line offsets,
    DevBuf<int32_t> status;                                 // the status pairs
};

static int text_rows_check(int64_t text_bytes, const int64_t *line_begin, int64_t row_count)
{
    for (int64_t r = 0; r <= row_count; r++)
        if (line_begin[r] < 0 || line_begin[r] > text_bytes || (r && line_begin[r] < line_begin[r - 1]))
            return fail(GARLIC_ERR_INVALID, "line_begin[%lld] = %lld: the offsets must ascend inside the slab of %lld bytes", (long long)r,
                        (long long)line_begin[r], (long long)text_bytes);
    return GARLIC_OK;
}

// the slab (uploaded when it is the host's) and its offsets onto the device, room for the status pairs; *d_text: the slab there
static int text_rows_stage(TextStage &st, const char *text, int64_t text_bytes, const int64_t *line_begin, int64_t row_count,
                           int32_t where, hipStream_t s, const uint8_t **d_text)
{
    int rc;
    *d_text = reinterpret_cast<const uint8_t *>(text);
    if (where == GARLIC_HOST) {
        if ((rc = st.text.reserve((size_t)text_bytes + 16))) return rc;          // (its last piece lies inside the buffer)
        HIP_TRY(hipMemcpyAsync(st.text.p, text, (size_t)text_bytes, hipMemcpyHostToDevice, s));
        *d_text = st.text.p;
    }
    if ((rc = st.lines.reserve((size_t)row_count + 1)) || (rc = st.status.reserve((size_t)(2 * row_count)))) return rc;
    HIP_TRY(hipMemcpyAsync(st.lines.p, line_begin, sizeof(int64_t) * (size_t)(row_count + 1), hipMemcpyHostToDevice, s));
    return GARLIC_OK;
}

// Behind the door's launch: the status pairs to the host (the stream is idle when this returns) and into row_status.
// *bad = the first row whose code is above `benign` (0, or the highest code that is no refusal), -1 for none.
static int text_rows_status(TextStage &st, int64_t row_count, int32_t *row_status, int benign, hipStream_t s,
                            std::vector<int32_t> &status, int64_t *bad)
{
    HIP_TRY(hipGetLastError());
    status.resize((size_t)(2 * row_count));
    HIP_TRY(hipMemcpyAsync(status.data(), st.status.p, sizeof(int32_t) * status.size(), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    if (row_status) memcpy(row_status, status.data(), sizeof(int32_t) * status.size());
    *bad = -1;
    for (int64_t r = 0; r < row_count && *bad < 0; r++)
        if (status[(size_t)(2 * r)] > benign) *bad = r;
    return GARLIC_OK;
}

// ---- PLINK .bed rows (bed_kernels.hpp): the image, its census, and the door into a panel
struct garlic_bed {
    garlic_ctx *ctx = nullptr;
    int64_t nrows = 0, row_bytes = 0, image_bytes = 0;      // image_bytes: rows + pad, a multiple of 16
    int32_t nind = 0;
    DevBuf<uint8_t> d_image, d_counted, stage;
    DevBuf<int32_t> d_counts;
    std::vector<uint64_t> row_set;                          // one bit per row that has been set
    int64_t n_set = 0;
    bool census_valid = false;
    std::vector<int32_t> counts;                            // the census, cached with the image
    std::vector<uint8_t> counted;
    // the order plane (vcf_kernels.hpp): one bit per genotype, "its first allele is A2"; absent until the first order or VCF call
    int64_t order_row_bytes = 0;                            // (nind + 7) / 8
    DevBuf<uint8_t> d_order;
    bool have_order = false;
    TextStage text;                                         // garlic_bed_set_rows_vcf, garlic_bed_set_rows_tped
    // where the rows came from: an image filled by garlic_bed_set_rows_tped carries the census its parse wrote (tped_kernels.hpp),
    // which the image rule cannot recompute, so the two kinds of source do not mix on one image
    enum Source { SOURCE_NONE = 0, SOURCE_ROWS = 1, SOURCE_TPED = 2 };
    int source = SOURCE_NONE;
    DevBuf<uint8_t> tped_allele;                            // garlic_bed_set_rows_tped: `one` per row of the call
};

// the first call that fills an image decides its kind
static int bed_claim_source(garlic_bed *b, int source, const char *what)
{
    if (b->source != garlic_bed::SOURCE_NONE && b->source != source)
        return fail(GARLIC_ERR_STATE, "%s: the image holds rows %s; the two sources do not mix on one image", what,
                    b->source == garlic_bed::SOURCE_TPED ? "parsed from TPED text, with the census of that parse" : "set as image rows or parsed from a VCF");
    b->source = source;
    return GARLIC_OK;
}

int garlic_bed_create(garlic_ctx *ctx, int64_t nrows, int32_t nind_total, garlic_bed **out)
{
    if (!out) return fail(GARLIC_ERR_INVALID, "bed out pointer is NULL");
    *out = nullptr;
    if (!ctx) return fail(GARLIC_ERR_INVALID, "ctx is NULL");
    if (nrows < 1 || nrows > 0x7FFFFFFF || nind_total < 1 || nind_total >= (1 << 30))
        return fail(GARLIC_ERR_INVALID, "need 1 <= nrows < 2^31 and 1 <= nind_total < 2^30");    // total = 2 * #non-missing is an int32
    int rc;
    if ((rc = set_device(ctx))) return rc;
    std::unique_ptr<garlic_bed> b(new garlic_bed);
    b->ctx = ctx;
    b->nrows = nrows;
    b->nind = nind_total;
    b->row_bytes = ((int64_t)nind_total + 3) / 4;
    b->order_row_bytes = ((int64_t)nind_total + 7) / 8;
    b->image_bytes = ((nrows * b->row_bytes + 15) & ~(int64_t)15) + BED_IMAGE_PAD;
    if ((rc = b->d_image.reserve((size_t)b->image_bytes)) || (rc = b->d_counts.reserve((size_t)(2 * nrows))) ||
        (rc = b->d_counted.reserve((size_t)nrows)))
        return rc;
    HIP_TRY(hipMemsetAsync(b->d_image.p + b->image_bytes - BED_IMAGE_PAD, 0, BED_IMAGE_PAD, ctx->stream));   // (masked anyway)
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    b->row_set.assign((size_t)((nrows + 63) / 64), 0);
    *out = b.release();
    return GARLIC_OK;
}

int garlic_bed_destroy(garlic_bed *b)
{
    if (!b) return GARLIC_OK;
    (void)hipSetDevice(b->ctx->device);
    (void)hipStreamSynchronize(b->ctx->stream);
    delete b;
    return GARLIC_OK;
}

int garlic_bed_set_rows(garlic_bed *b, const uint8_t *rows, int64_t row_bytes, int64_t row_begin, int64_t row_count, int32_t where)
{
    if (!b || !rows) return fail(GARLIC_ERR_INVALID, "bed and rows are required");
    if (where != GARLIC_HOST && where != GARLIC_DEVICE) return fail(GARLIC_ERR_INVALID, "where must be GARLIC_HOST or GARLIC_DEVICE");
    if (row_bytes < b->row_bytes)
        return fail(GARLIC_ERR_INVALID, "row_bytes %lld too small for %d individuals (%lld)", (long long)row_bytes, b->nind,
                    (long long)b->row_bytes);
    if (row_begin < 0 || row_count < 1 || row_begin + row_count > b->nrows)
        return fail(GARLIC_ERR_INVALID, "row range [%lld,+%lld) outside image of %lld rows", (long long)row_begin,
                    (long long)row_count, (long long)b->nrows);
    int rc;
    if ((rc = bed_claim_source(b, garlic_bed::SOURCE_ROWS, "bed_set_rows")) || (rc = set_device(b->ctx))) return rc;
    hipStream_t s = b->ctx->stream;
    b->census_valid = false;
    rc = for_each_upload_slab(s, "bed_set_rows", rows, row_bytes, row_count, where, b->stage, [&](const void *src, int64_t at, int64_t n) {
        uint8_t *dst = b->d_image.p + (row_begin + at) * b->row_bytes;
        const hipError_t e = row_bytes == b->row_bytes
            ? hipMemcpyAsync(dst, src, (size_t)(n * row_bytes), hipMemcpyDeviceToDevice, s)
            : hipMemcpy2DAsync(dst, (size_t)b->row_bytes, src, (size_t)row_bytes, (size_t)b->row_bytes, (size_t)n, hipMemcpyDeviceToDevice, s);
        return e == hipSuccess ? GARLIC_OK : upload_fail("bed_set_rows", e);
    });
    if (rc) return rc;
    for (int64_t r = row_begin; r < row_begin + row_count; r++) {
        uint64_t &word = b->row_set[(size_t)(r >> 6)];
        const uint64_t bit = 1ull << (r & 63);
        if (!(word & bit)) { word |= bit; b->n_set++; }
    }
    return GARLIC_OK;
}

// the census of the image as it stands, on the device and in the host cache
static int bed_ensure_census(garlic_bed *b)
{
    if (b->n_set != b->nrows)
        return fail(GARLIC_ERR_STATE, "bed census needs every row: %lld of %lld set", (long long)b->n_set, (long long)b->nrows);
    if (b->census_valid) return GARLIC_OK;
    int rc;
    if ((rc = set_device(b->ctx))) return rc;
    hipStream_t s = b->ctx->stream;
    if (b->source == garlic_bed::SOURCE_TPED) {      // the parse wrote it, row by row: only the host's copy is missing
        b->counts.resize((size_t)(2 * b->nrows));
        b->counted.resize((size_t)b->nrows);
        HIP_TRY(hipMemcpyAsync(b->counts.data(), b->d_counts.p, sizeof(int32_t) * 2 * b->nrows, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipMemcpyAsync(b->counted.data(), b->d_counted.p, (size_t)b->nrows, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        b->census_valid = true;
        return GARLIC_OK;
    }
    // lanes per row: the pieces a row can touch (it starts at any byte), as a power of two; narrower rows share a wave
    const int64_t pieces = (b->row_bytes + 30) >> 4;
    int group = 1;
    while (group < 64 && group < pieces) group <<= 1;
    const int64_t rows_per_block = 4 * (64 / group);
    const unsigned grid = (unsigned)std::min<int64_t>((b->nrows + rows_per_block - 1) / rows_per_block, 8 * (int64_t)b->ctx->n_cu);
    hipLaunchKernelGGL(bed_census_kernel, dim3(grid), dim3(256), 0, s, b->d_image.p, b->nrows, b->nind, b->row_bytes, group,
                       b->d_counts.p, b->d_counted.p, b->have_order ? (const uint8_t *)b->d_order.p : (const uint8_t *)nullptr,
                       b->order_row_bytes);
    HIP_TRY(hipGetLastError());
    b->counts.resize((size_t)(2 * b->nrows));
    b->counted.resize((size_t)b->nrows);
    HIP_TRY(hipMemcpyAsync(b->counts.data(), b->d_counts.p, sizeof(int32_t) * 2 * b->nrows, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(b->counted.data(), b->d_counted.p, (size_t)b->nrows, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    b->census_valid = true;
    return GARLIC_OK;
}

int garlic_bed_census(garlic_bed *b, int32_t *counts, uint8_t *counted, int32_t where)
{
    if (!b) return fail(GARLIC_ERR_INVALID, "bed is NULL");
    if (where != GARLIC_HOST && where != GARLIC_DEVICE) return fail(GARLIC_ERR_INVALID, "where must be GARLIC_HOST or GARLIC_DEVICE");
    int rc;
    if ((rc = bed_ensure_census(b))) return rc;
    if (where == GARLIC_HOST) {
        if (counts) memcpy(counts, b->counts.data(), sizeof(int32_t) * b->counts.size());
        if (counted) memcpy(counted, b->counted.data(), b->counted.size());
        return GARLIC_OK;
    }
    hipStream_t s = b->ctx->stream;
    if (counts) HIP_TRY(hipMemcpyAsync(counts, b->d_counts.p, sizeof(int32_t) * 2 * b->nrows, hipMemcpyDeviceToDevice, s));
    if (counted) HIP_TRY(hipMemcpyAsync(counted, b->d_counted.p, (size_t)b->nrows, hipMemcpyDeviceToDevice, s));
    HIP_TRY(hipStreamSynchronize(s));
    return GARLIC_OK;
}

// what the doors from an image into a panel ask of their arguments; first / last: the smallest and largest destination
static int bed_check_dest(const garlic_panel *p, const garlic_bed *b, int64_t ind_offset, const int64_t *dest_locus, int64_t &first,
                          int64_t &last)
{
    if (b->ctx->device != p->ctx->device)
        return fail(GARLIC_ERR_INVALID, "the bed image is on device %d, the panel on device %d", b->ctx->device, p->ctx->device);
    if (ind_offset < 0 || ind_offset + p->nind > b->nind)
        return fail(GARLIC_ERR_INVALID, "individuals [%lld,+%d) outside the image's %d", (long long)ind_offset, p->nind, b->nind);
    int64_t prev = -1;
    first = -1;
    for (int64_t r = 0; r < b->nrows; r++) {
        const int64_t l = dest_locus[r];
        if (l == -1) continue;
        if (l < 0 || l >= p->nloci)
            return fail(GARLIC_ERR_INVALID, "dest_locus[%lld] = %lld outside panel of %lld loci", (long long)r, (long long)l, (long long)p->nloci);
        if (l <= prev)
            return fail(GARLIC_ERR_INVALID, "dest_locus must ascend over the kept rows: row %lld maps to %lld after %lld", (long long)r,
                        (long long)l, (long long)prev);
        if (first < 0) first = l;
        prev = l;
    }
    if (first < 0) return fail(GARLIC_ERR_INVALID, "dest_locus keeps no row");
    last = prev;
    return GARLIC_OK;
}

int garlic_panel_set_genotypes_bed(garlic_panel *p, garlic_bed *b, int64_t ind_offset, const int64_t *dest_locus)
{
    if (!p || !b || !dest_locus) return fail(GARLIC_ERR_INVALID, "panel, bed and dest_locus are required");
    int64_t first, prev;
    if (int rc = bed_check_dest(p, b, ind_offset, dest_locus, first, prev)) return rc;
    int rc;
    if ((rc = bed_ensure_census(b)) || (rc = set_device(p->ctx))) return rc;
    // the rows of every 16-locus word the call touches
    const int64_t w_lo = (GOFF + first) >> 4, w_hi = ((GOFF + prev) >> 4) + 1;
    std::vector<int32_t> word_rows((size_t)((w_hi - w_lo) * 16), -1);
    for (int64_t r = 0; r < b->nrows; r++)
        if (dest_locus[r] >= 0) word_rows[(size_t)(GOFF + dest_locus[r] - 16 * w_lo)] = (int32_t)r;
    hipStream_t s = p->ctx->stream;
    if ((rc = p->d_bed_word_rows.put(word_rows, s))) return rc;
    const int64_t nblk = p->nind_pad / 64;
    const dim3 grid((unsigned)(w_hi - w_lo), (unsigned)((nblk + BED_SPAN_BLOCKS - 1) / BED_SPAN_BLOCKS));
    hipLaunchKernelGGL(bed_pack_kernel, grid, dim3(256), 0, s, b->d_image.p, b->image_bytes, b->row_bytes, b->d_counted.p,
                       p->d_bed_word_rows.p, ind_offset, p->nind, p->nind_pad, p->nwordrows, p->d_packed.p, w_lo);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipStreamSynchronize(s);       // also: word_rows is free again
    if (e != hipSuccess) return upload_fail("set_genotypes_bed", e);
    p->have_geno = true;
    p->geno_epoch++;
    p->glterms_valid = false;
    return GARLIC_OK;
}

int garlic_bed_extract(garlic_bed *src, const int32_t *ind_idx, int32_t n_idx, garlic_bed **out)
{
    if (!src || !ind_idx || !out) return fail(GARLIC_ERR_INVALID, "bed extract: src, ind_idx and out are required");
    if (n_idx < 1 || n_idx >= (1 << 30)) return fail(GARLIC_ERR_INVALID, "bed extract: need 1 <= n_idx < 2^30, got %d", n_idx);
    if (src->have_order)
        return fail(GARLIC_ERR_INVALID, "bed extract: a column subset of an image with an order plane (VCF input) is not built");
    if (src->n_set != src->nrows)
        return fail(GARLIC_ERR_STATE, "bed extract needs every row of the source: %lld of %lld set", (long long)src->n_set, (long long)src->nrows);
    for (int32_t i = 0; i < n_idx; i++)
        if (ind_idx[i] < 0 || ind_idx[i] >= src->nind)
            return fail(GARLIC_ERR_INVALID, "bed extract: ind_idx[%d] = %d outside the source's %d individuals", i, ind_idx[i], src->nind);
    int rc;
    if ((rc = set_device(src->ctx))) return rc;
    hipStream_t s = src->ctx->stream;
    // per span of 8192 subset individuals: the first source byte it needs and the pieces of a row in LDS (0: global form)
    const int64_t nwords = ((int64_t)n_idx + 31) / 32;
    const int64_t nspans = (nwords + BED_EXTRACT_SPAN_WORDS - 1) / BED_EXTRACT_SPAN_WORDS;
    std::vector<BedSpan> spans((size_t)nspans);
    for (int64_t sp = 0; sp < nspans; sp++) {
        const int64_t i0 = sp * BED_EXTRACT_SPAN_WORDS * 32, i1 = std::min<int64_t>(n_idx, i0 + BED_EXTRACT_SPAN_WORDS * 32);
        int32_t lo = ind_idx[i0], hi = ind_idx[i0];
        for (int64_t i = i0; i < i1; i++) { lo = std::min(lo, ind_idx[i]); hi = std::max(hi, ind_idx[i]); }
        const int32_t range = (hi >> 2) - (lo >> 2) + 1;
        spans[(size_t)sp] = {lo >> 2, range > BED_EXTRACT_MAX_RANGE ? 0 : ((range + 14) >> 4) + 1};
    }
    std::unique_ptr<garlic_bed> b(new garlic_bed);      // (a failure below frees what it holds; *out is written last)
    b->ctx = src->ctx;
    b->nrows = src->nrows;
    b->nind = n_idx;
    b->row_bytes = ((int64_t)n_idx + 3) / 4;
    b->order_row_bytes = ((int64_t)n_idx + 7) / 8;
    b->image_bytes = ((b->nrows * b->row_bytes + 15) & ~(int64_t)15) + BED_IMAGE_PAD;
    DevBuf<int32_t> d_idx;
    DevBuf<BedSpan> d_spans;
    if ((rc = b->d_image.reserve((size_t)b->image_bytes)) || (rc = b->d_counts.reserve((size_t)(2 * b->nrows))) ||
        (rc = b->d_counted.reserve((size_t)b->nrows)) || (rc = d_idx.reserve((size_t)n_idx)) || (rc = d_spans.put(spans, s)))
        return rc;
    HIP_TRY(hipMemcpyAsync(d_idx.p, ind_idx, sizeof(int32_t) * (size_t)n_idx, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemsetAsync(b->d_image.p + b->image_bytes - BED_IMAGE_PAD - 16, 0, BED_IMAGE_PAD + 16, s));
    const int64_t want = std::max<int64_t>(1, (8 * (int64_t)src->ctx->n_cu + nspans - 1) / nspans);
    const dim3 grid((unsigned)nspans, (unsigned)std::min<int64_t>(std::min<int64_t>(b->nrows, 65535), want));
    hipLaunchKernelGGL(bed_extract_kernel, grid, dim3(256), 0, s, src->d_image.p, src->image_bytes, src->nrows, src->row_bytes,
                       d_idx.p, n_idx, d_spans.p, b->d_image.p, b->row_bytes);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(s));                   // the index lists are free again; `src` may go
    b->row_set.assign((size_t)((b->nrows + 63) / 64), ~0ull);
    b->n_set = b->nrows;
    b->source = garlic_bed::SOURCE_ROWS;
    *out = b.release();
    return GARLIC_OK;
}

int garlic_bed_get_rows(garlic_bed *b, int64_t row_begin, int64_t row_count, uint8_t *rows, int64_t row_bytes, int32_t where)
{
    if (!b || !rows) return fail(GARLIC_ERR_INVALID, "bed and rows are required");
    if (where != GARLIC_HOST && where != GARLIC_DEVICE) return fail(GARLIC_ERR_INVALID, "where must be GARLIC_HOST or GARLIC_DEVICE");
    if (row_bytes < b->row_bytes)
        return fail(GARLIC_ERR_INVALID, "row_bytes %lld too small for %d individuals (%lld)", (long long)row_bytes, b->nind,
                    (long long)b->row_bytes);
    if (row_begin < 0 || row_count < 1 || row_begin + row_count > b->nrows)
        return fail(GARLIC_ERR_INVALID, "row range [%lld,+%lld) outside image of %lld rows", (long long)row_begin,
                    (long long)row_count, (long long)b->nrows);
    int rc;
    if ((rc = set_device(b->ctx))) return rc;
    hipStream_t s = b->ctx->stream;
    const uint8_t *from = b->d_image.p + row_begin * b->row_bytes;
    const hipMemcpyKind kind = where == GARLIC_HOST ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice;
    if (row_bytes == b->row_bytes)
        HIP_TRY(hipMemcpyAsync(rows, from, (size_t)(row_count * row_bytes), kind, s));
    else
        HIP_TRY(hipMemcpy2DAsync(rows, (size_t)row_bytes, from, (size_t)b->row_bytes, (size_t)b->row_bytes, (size_t)row_count, kind, s));
    HIP_TRY(hipStreamSynchronize(s));
    return GARLIC_OK;
}

// ---- the order plane of an image and the VCF door (vcf_kernels.hpp)
// the plane of an image that gets its first order bits, all zero (padded as the image is)
static int bed_ensure_order(garlic_bed *b)
{
    if (b->have_order) return GARLIC_OK;
    const size_t bytes = (size_t)(((b->nrows * b->order_row_bytes + 15) & ~(int64_t)15) + BED_IMAGE_PAD);
    if (int rc = b->d_order.reserve(bytes)) return rc;
    HIP_TRY(hipMemsetAsync(b->d_order.p, 0, bytes, b->ctx->stream));
    HIP_TRY(hipStreamSynchronize(b->ctx->stream));
    b->have_order = true;
    b->census_valid = false;          // the counted allele now follows the plane
    return GARLIC_OK;
}

static int bed_check_order_args(const garlic_bed *b, const void *rows, int64_t row_bytes, int64_t row_begin, int64_t row_count, int32_t where)
{
    if (!b || !rows) return fail(GARLIC_ERR_INVALID, "bed and rows are required");
    if (where != GARLIC_HOST && where != GARLIC_DEVICE) return fail(GARLIC_ERR_INVALID, "where must be GARLIC_HOST or GARLIC_DEVICE");
    if (row_bytes < b->order_row_bytes)
        return fail(GARLIC_ERR_INVALID, "row_bytes %lld too small for the order bits of %d individuals (%lld)", (long long)row_bytes,
                    b->nind, (long long)b->order_row_bytes);
    if (row_begin < 0 || row_count < 1 || row_begin + row_count > b->nrows)
        return fail(GARLIC_ERR_INVALID, "row range [%lld,+%lld) outside image of %lld rows", (long long)row_begin,
                    (long long)row_count, (long long)b->nrows);
    return GARLIC_OK;
}

int garlic_bed_set_order_rows(garlic_bed *b, const uint8_t *rows, int64_t row_bytes, int64_t row_begin, int64_t row_count, int32_t where)
{
    int rc;
    if ((rc = bed_check_order_args(b, rows, row_bytes, row_begin, row_count, where)) ||
        (rc = bed_claim_source(b, garlic_bed::SOURCE_ROWS, "bed_set_order_rows")) || (rc = set_device(b->ctx)) || (rc = bed_ensure_order(b)))
        return rc;
    hipStream_t s = b->ctx->stream;
    b->census_valid = false;
    return for_each_upload_slab(s, "bed_set_order_rows", rows, row_bytes, row_count, where, b->stage, [&](const void *src, int64_t at, int64_t n) {
        uint8_t *dst = b->d_order.p + (row_begin + at) * b->order_row_bytes;
        const hipError_t e = row_bytes == b->order_row_bytes
            ? hipMemcpyAsync(dst, src, (size_t)(n * row_bytes), hipMemcpyDeviceToDevice, s)
            : hipMemcpy2DAsync(dst, (size_t)b->order_row_bytes, src, (size_t)row_bytes, (size_t)b->order_row_bytes, (size_t)n,
                               hipMemcpyDeviceToDevice, s);
        return e == hipSuccess ? GARLIC_OK : upload_fail("bed_set_order_rows", e);
    });
}

int garlic_bed_get_order_rows(garlic_bed *b, int64_t row_begin, int64_t row_count, uint8_t *rows, int64_t row_bytes, int32_t where)
{
    int rc;
    if ((rc = bed_check_order_args(b, rows, row_bytes, row_begin, row_count, where))) return rc;
    if (!b->have_order) return fail(GARLIC_ERR_STATE, "the image has no order plane");
    if ((rc = set_device(b->ctx))) return rc;
    hipStream_t s = b->ctx->stream;
    const uint8_t *from = b->d_order.p + row_begin * b->order_row_bytes;
    const hipMemcpyKind kind = where == GARLIC_HOST ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice;
    if (row_bytes == b->order_row_bytes)
        HIP_TRY(hipMemcpyAsync(rows, from, (size_t)(row_count * row_bytes), kind, s));
    else
        HIP_TRY(hipMemcpy2DAsync(rows, (size_t)row_bytes, from, (size_t)b->order_row_bytes, (size_t)b->order_row_bytes, (size_t)row_count, kind, s));
    HIP_TRY(hipStreamSynchronize(s));
    return GARLIC_OK;
}

static const char *vcf_offence_name(int code)
{
    switch (code) {
    case VCF_BAD_BYTE: return "a byte that is no part of a genotype `a sep b`";
    case VCF_HALF_MISSING: return "a half-missing genotype";
    case VCF_HAPLOID: return "a haploid genotype";
    case VCF_ALLELE_INDEX: return "an allele index of 2 or more";
    case VCF_FEW_COLUMNS: return "too few sample columns";
    case VCF_MANY_COLUMNS: return "too many sample columns";
    }
    return "an unknown offence";
}

int garlic_bed_set_rows_vcf(garlic_bed *b, const char *text, int64_t text_bytes, const int64_t *line_begin, int64_t row_begin,
                            int64_t row_count, int32_t *row_status, int32_t where)
{
    if (!b || !text || !line_begin) return fail(GARLIC_ERR_INVALID, "bed, text and line_begin are required");
    if (where != GARLIC_HOST && where != GARLIC_DEVICE) return fail(GARLIC_ERR_INVALID, "where must be GARLIC_HOST or GARLIC_DEVICE");
    if (text_bytes < 1) return fail(GARLIC_ERR_INVALID, "text_bytes %lld: the slab is empty", (long long)text_bytes);
    if (row_begin < 0 || row_count < 1 || row_begin + row_count > b->nrows)
        return fail(GARLIC_ERR_INVALID, "row range [%lld,+%lld) outside image of %lld rows", (long long)row_begin,
                    (long long)row_count, (long long)b->nrows);
    int rc;
    if ((rc = text_rows_check(text_bytes, line_begin, row_count))) return rc;
    if ((rc = bed_claim_source(b, garlic_bed::SOURCE_ROWS, "bed_set_rows_vcf")) || (rc = set_device(b->ctx)) || (rc = bed_ensure_order(b))) return rc;
    hipStream_t s = b->ctx->stream;
    b->census_valid = false;
    const uint8_t *d_text;
    if ((rc = text_rows_stage(b->text, text, text_bytes, line_begin, row_count, where, s, &d_text))) return rc;
    hipLaunchKernelGGL(vcf_parse_kernel, dim3((unsigned)row_count), dim3(256), 0, s, d_text, text_bytes, b->text.lines.p, row_begin,
                       b->nind, b->d_image.p, b->row_bytes, b->d_order.p, b->order_row_bytes, b->text.status.p);
    std::vector<int32_t> status;
    int64_t bad;
    if ((rc = text_rows_status(b->text, row_count, row_status, VCF_OK, s, status, &bad))) return rc;
    for (int64_t r = 0; r < row_count; r++) {
        if (status[(size_t)(2 * r)]) continue;                 // its bits are unspecified: the row does not count as set
        uint64_t &word = b->row_set[(size_t)((row_begin + r) >> 6)];
        const uint64_t bit = 1ull << ((row_begin + r) & 63);
        if (!(word & bit)) { word |= bit; b->n_set++; }
    }
    if (bad >= 0)
        return fail(GARLIC_ERR_INVALID, "VCF row %lld (line %lld of the call): %s at sample column %d", (long long)(row_begin + bad),
                    (long long)bad, vcf_offence_name(status[(size_t)(2 * bad)]), status[(size_t)(2 * bad + 1)]);
    return GARLIC_OK;
}

// ---- the TPED door (tped_kernels.hpp) and the census a source hands over
static const char *tped_offence_name(int code)
{
    switch (code) {
    case TPED_LONG_ALLELE: return "an allele longer than one character";
    case TPED_BAD_BYTE: return "a vertical tab, form feed or NUL byte";
    case TPED_FEW_COLUMNS: return "too few allele columns";
    case TPED_MANY_COLUMNS: return "too many allele columns";
    }
    return "an unknown offence";
}

int garlic_bed_set_rows_tped(garlic_bed *b, const char *text, int64_t text_bytes, const int64_t *line_begin, int64_t row_begin,
                             int64_t row_count, uint8_t missing, uint8_t *row_allele, int32_t *row_status, int32_t where)
{
    if (!b || !text || !line_begin) return fail(GARLIC_ERR_INVALID, "bed, text and line_begin are required");
    if (where != GARLIC_HOST && where != GARLIC_DEVICE) return fail(GARLIC_ERR_INVALID, "where must be GARLIC_HOST or GARLIC_DEVICE");
    if (text_bytes < 1) return fail(GARLIC_ERR_INVALID, "text_bytes %lld: the slab is empty", (long long)text_bytes);
    if (missing == ' ' || missing == '\t' || missing == '\r' || missing == '\n')
        return fail(GARLIC_ERR_INVALID, "the missing character (byte %d) is a blank or a newline", (int)missing);
    if (row_begin < 0 || row_count < 1 || row_begin + row_count > b->nrows)
        return fail(GARLIC_ERR_INVALID, "row range [%lld,+%lld) outside image of %lld rows", (long long)row_begin,
                    (long long)row_count, (long long)b->nrows);
    int rc;
    if ((rc = text_rows_check(text_bytes, line_begin, row_count))) return rc;
    if ((rc = bed_claim_source(b, garlic_bed::SOURCE_TPED, "bed_set_rows_tped")) || (rc = set_device(b->ctx)) || (rc = bed_ensure_order(b)))
        return rc;
    hipStream_t s = b->ctx->stream;
    b->census_valid = false;
    const uint8_t *d_text;
    if ((rc = text_rows_stage(b->text, text, text_bytes, line_begin, row_count, where, s, &d_text)) ||
        (rc = b->tped_allele.reserve((size_t)row_count)))
        return rc;
    hipLaunchKernelGGL(tped_parse_kernel, dim3((unsigned)row_count), dim3(256), 0, s, d_text, text_bytes, b->text.lines.p, row_begin, b->nind,
                       (uint32_t)missing, b->d_image.p, b->row_bytes, b->d_order.p, b->order_row_bytes, b->d_counts.p, b->d_counted.p,
                       b->tped_allele.p, b->text.status.p);
    std::vector<int32_t> status;
    std::vector<uint8_t> one((size_t)row_count);
    HIP_TRY(hipMemcpyAsync(one.data(), b->tped_allele.p, one.size(), hipMemcpyDeviceToHost, s));      // (waited for with the status)
    int64_t bad;
    if ((rc = text_rows_status(b->text, row_count, row_status, TPED_OK, s, status, &bad))) return rc;
    if (row_allele) memcpy(row_allele, one.data(), one.size());
    for (int64_t r = 0; r < row_count; r++) {
        uint64_t &word = b->row_set[(size_t)((row_begin + r) >> 6)];
        const uint64_t bit = 1ull << ((row_begin + r) & 63);
        if (status[(size_t)(2 * r)]) {
            if (word & bit) { word &= ~bit; b->n_set--; }      // its bits and its census are unspecified now
            continue;
        }
        if (!(word & bit)) { word |= bit; b->n_set++; }
    }
    if (bad >= 0)
        return fail(GARLIC_ERR_INVALID, "TPED row %lld (line %lld of the call): %s at individual %d", (long long)(row_begin + bad),
                    (long long)bad, tped_offence_name(status[(size_t)(2 * bad)]), status[(size_t)(2 * bad + 1)]);
    return GARLIC_OK;
}

int garlic_bed_set_census(garlic_bed *b, const int32_t *counts, const uint8_t *counted, int32_t where)
{
    if (!b || !counts || !counted) return fail(GARLIC_ERR_INVALID, "bed, counts and counted are required");
    if (where != GARLIC_HOST && where != GARLIC_DEVICE) return fail(GARLIC_ERR_INVALID, "where must be GARLIC_HOST or GARLIC_DEVICE");
    if (b->n_set != b->nrows)
        return fail(GARLIC_ERR_STATE, "bed set_census needs every row: %lld of %lld set", (long long)b->n_set, (long long)b->nrows);
    int rc;
    if ((rc = set_device(b->ctx))) return rc;
    hipStream_t s = b->ctx->stream;
    std::vector<int32_t> c((size_t)(2 * b->nrows));
    std::vector<uint8_t> k((size_t)b->nrows);
    if (where == GARLIC_HOST) {
        memcpy(c.data(), counts, sizeof(int32_t) * c.size());
        memcpy(k.data(), counted, k.size());
    } else {
        HIP_TRY(hipMemcpyAsync(c.data(), counts, sizeof(int32_t) * c.size(), hipMemcpyDeviceToHost, s));
        HIP_TRY(hipMemcpyAsync(k.data(), counted, k.size(), hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
    }
    for (int64_t r = 0; r < b->nrows; r++) {
        if (k[(size_t)r] > 2) return fail(GARLIC_ERR_INVALID, "set_census: counted[%lld] = %d is none of 0 (A1), 1 (A2), 2 (none)", (long long)r, (int)k[(size_t)r]);
        const int32_t na = c[(size_t)(2 * r)], tot = c[(size_t)(2 * r + 1)];
        if (na < 0 || tot < 0 || na > tot)
            return fail(GARLIC_ERR_INVALID, "set_census: counts[%lld] = {%d, %d} are no {nalleles, total}", (long long)r, na, tot);
    }
    HIP_TRY(hipMemcpyAsync(b->d_counts.p, c.data(), sizeof(int32_t) * c.size(), hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(b->d_counted.p, k.data(), k.size(), hipMemcpyHostToDevice, s));
    HIP_TRY(hipStreamSynchronize(s));
    b->counts.swap(c);
    b->counted.swap(k);
    b->census_valid = true;
    return GARLIC_OK;
}

// ---- uploads into a panel of 16-bit codes.
// The caller's table joins the panel's (by bit pattern, first seen first): remap[caller code] = panel code.  When the merged
// table would pass 65,536 values the panel goes on with the values themselves (gl_wide unset on return; remap is void then).
static int merge_wide_table(garlic_panel *p, const double *values, int32_t nvalues, std::vector<uint16_t> &remap)
{
    remap.assign((size_t)nvalues, 0);
    size_t fresh = 0;
    for (int k = 0; k < nvalues; k++)
        fresh += p->gl_code.count(value_bits(values[k])) == 0;      // (a value twice in the caller's table counts twice: an upper bound is enough)
    if (p->gl_values.size() + fresh > (size_t)GL_WIDE_MAX) {
        std::unordered_map<uint64_t, int> probe = p->gl_code;      // exact count before giving the codes up
        for (int k = 0; k < nvalues; k++) probe.emplace(value_bits(values[k]), 0);
        if (probe.size() > (size_t)GL_WIDE_MAX) return switch_to_continuous(p);
    }
    for (int k = 0; k < nvalues; k++) remap[(size_t)k] = (uint16_t)dict_add(p, value_bits(values[k]), GL_WIDE_MAX);      // (there is room: counted)
    return GARLIC_OK;
}

// caller rows of codes of code_bytes (1 or 2) each, translated by remap into the panel's codes
static int upload_wide_codes(garlic_panel *p, const void *codes, size_t code_bytes, int64_t ld, int64_t locus_begin,
                             int64_t locus_count, const std::vector<uint16_t> &remap, int32_t where)
{
    hipStream_t s = p->ctx->stream;
    const int64_t rows_total = GOFF + p->nloci + GPAD_BACK;
    DevBuf<uint8_t> stage;
    DevBuf<uint16_t> d_remap;
    int rc;
    if ((rc = d_remap.reserve(remap.size()))) return rc;
    hipError_t e = hipMemcpy(d_remap.p, remap.data(), sizeof(uint16_t) * remap.size(), hipMemcpyHostToDevice);
    if (e != hipSuccess) return upload_fail("set_gl_codes16", e);
    rc = for_each_upload_slab(s, "set_gl_codes16", codes, (int64_t)code_bytes * ld, locus_count, where, stage, [&](const void *rows, int64_t at, int64_t n) {
        if (code_bytes == 1)
            hipLaunchKernelGGL(gl_recode8to16_kernel, dim3(2048), dim3(256), 0, s, (const uint8_t *)rows, ld, locus_begin + at, n, p->nind,
                               d_remap.p, rows_total, p->d_codes16.p);
        else
            hipLaunchKernelGGL(gl_recode16_kernel, dim3(2048), dim3(256), 0, s, (const uint16_t *)rows, ld, locus_begin + at, n, p->nind,
                               d_remap.p, (int32_t)remap.size(), rows_total, p->d_codes16.p);
        return GARLIC_OK;
    });
    return rc ? rc : end_gl_upload(p, locus_begin, locus_count);
}

int garlic_panel_set_gl(garlic_panel *p, const double *gl, int64_t ld, int64_t locus_begin,
                        int64_t locus_count, int32_t where)
{
    if (!p || !gl) return fail(GARLIC_ERR_INVALID, "panel and gl are required");
    int rc;
    if ((rc = check_rows(p, ld, locus_begin, locus_count)) || (rc = begin_gl_upload(p)) || (rc = ensure_byte_codes(p))) return rc;
    hipStream_t s = p->ctx->stream;
    const int64_t rows_total = GOFF + p->nloci + GPAD_BACK;
    // Few distinct error probabilities (GQ / PL integers) -> one-byte codes: the term table per (SNP,
    // code, genotype) comes from the host libm and the panel keeps 1 B instead of 8 B per genotype.  A
    // panel of 16-bit codes (garlic_panel_set_gl_codes16) codes the values against its table of up to
    // 65,536.  Either way a slab is coded on the device (encode_until_known); when the dictionary is full
    // (--gl-type GL, continuous inputs) the panel switches to keeping the values themselves and evaluates
    // lod() on the device: what was coded is decoded, this slab and every later one is stored as it is.
    EncodeScratch sc;
    if (!p->gl_cont && (rc = sc.reserve(p->gl_wide ? GL_WIDE_MAX : GL_DICT_MAX, p->gl_wide ? 2 : 1))) return rc;
    DevBuf<double> stage;
    rc = for_each_upload_slab(s, "set_gl", gl, 8 * ld, locus_count, where, stage, [&](const void *rows, int64_t at, int64_t n) {
        const double *src = (const double *)rows;
        const int64_t l0 = locus_begin + at;
        if (!p->gl_cont) {
            const int coded =
                p->gl_wide ? encode_until_known<uint16_t>(p, "set_gl", GL_WIDE_MAX, sc, [&](const uint16_t *dcode, int ndict) {
                    hipLaunchKernelGGL(gl_encode16_kernel, dim3(2048), dim3(256), 0, s, src, ld, l0, n, p->nind, sc.bits.p, dcode, ndict,
                                       rows_total, p->d_codes16.p, sc.unk.p, sc.nunk.p, UNK_CAP);
                })
                           : encode_until_known<uint8_t>(p, "set_gl", GL_DICT_MAX, sc, [&](const uint8_t *dcode, int ndict) {
                                 hipLaunchKernelGGL(gl_encode_kernel, dim3(2048), dim3(256), 0, s, src, ld, n, p->nind, p->nind_pad, sc.bits.p,
                                                    dcode, ndict, p->d_codes.p + (GOFF + l0) * p->nind_pad, sc.unk.p, sc.nunk.p, UNK_CAP);
                             });
            if (coded != DICT_FULL) return coded;
            if (int full_rc = switch_to_continuous(p)) return full_rc;
        }
        hipLaunchKernelGGL(gl_store_kernel, dim3(2048), dim3(256), 0, s, src, ld, l0, n, p->nind, rows_total, p->d_glval.p);
        return GARLIC_OK;
    });
    return rc ? rc : end_gl_upload(p, locus_begin, locus_count);
}

int garlic_panel_set_gl_codes(garlic_panel *p, const uint8_t *codes, int64_t ld, int64_t locus_begin,
                              int64_t locus_count, const double *values, int32_t nvalues, int32_t where)
{
    if (!p || !codes || !values) return fail(GARLIC_ERR_INVALID, "panel, codes and values are required");
    if (nvalues < 1 || nvalues > GL_DICT_MAX) return fail(GARLIC_ERR_INVALID, "nvalues must be 1..256 (got %d)", nvalues);
    int rc;
    if ((rc = check_rows(p, ld, locus_begin, locus_count)) || (rc = begin_gl_upload(p))) return rc;
    hipStream_t s = p->ctx->stream;
    const int64_t rows_total = GOFF + p->nloci + GPAD_BACK;
    // the caller's table joins the panel's dictionary; its codes are translated on the device.  A
    // panel whose tables add up to more than 256 values keeps the values themselves from then on.
    if (p->gl_wide) {
        std::vector<uint16_t> remap16;
        if ((rc = merge_wide_table(p, values, nvalues, remap16))) return rc;
        if (p->gl_wide) {
            remap16.resize(256, 0);
            return upload_wide_codes(p, codes, 1, ld, locus_begin, locus_count, remap16, where);
        }
    }
    uint8_t remap[256] = {0};
    for (int k = 0; k < nvalues && !p->gl_cont; k++) {
        const int code = dict_add(p, value_bits(values[k]), GL_DICT_MAX);
        if (code == DICT_FULL) {
            if (!p->d_codes.p) dict_clear(p);      // nothing coded yet: start from an empty value matrix
            if ((rc = switch_to_continuous(p))) return rc;
            break;
        }
        remap[k] = (uint8_t)code;
    }
    if ((rc = ensure_byte_codes(p))) return rc;
    DevBuf<uint8_t> stage, d_remap;
    DevBuf<double> d_dict;
    hipError_t e;
    if (p->gl_cont) {
        std::vector<double> dict(GL_DICT_MAX, 0.0);
        std::copy(values, values + nvalues, dict.begin());
        if ((rc = d_dict.reserve(GL_DICT_MAX))) return rc;
        e = hipMemcpy(d_dict.p, dict.data(), sizeof(double) * GL_DICT_MAX, hipMemcpyHostToDevice);
    } else {
        if ((rc = d_remap.reserve(256))) return rc;
        e = hipMemcpy(d_remap.p, remap, 256, hipMemcpyHostToDevice);
    }
    if (e != hipSuccess) return upload_fail("set_gl_codes", e);
    rc = for_each_upload_slab(s, "set_gl_codes", codes, ld, locus_count, where, stage, [&](const void *rows, int64_t at, int64_t n) {
        if (p->gl_cont)
            hipLaunchKernelGGL(gl_store_codes_kernel, dim3(2048), dim3(256), 0, s, (const uint8_t *)rows, ld, locus_begin + at, n, p->nind,
                               d_dict.p, rows_total, p->d_glval.p);
        else
            hipLaunchKernelGGL(gl_recode_kernel, dim3(2048), dim3(256), 0, s, (const uint8_t *)rows, ld, n, p->nind, p->nind_pad, d_remap.p,
                               p->d_codes.p + (GOFF + locus_begin + at) * p->nind_pad);
        return GARLIC_OK;
    });
    return rc ? rc : end_gl_upload(p, locus_begin, locus_count);
}

int garlic_panel_set_gl_codes16(garlic_panel *p, const uint16_t *codes, int64_t ld, int64_t locus_begin,
                                int64_t locus_count, const double *values, int32_t nvalues, int32_t where)
{
    if (!p || !codes || !values) return fail(GARLIC_ERR_INVALID, "panel, codes and values are required");
    if (nvalues < 1 || nvalues > GL_WIDE_MAX) return fail(GARLIC_ERR_INVALID, "nvalues must be 1..65536 (got %d)", nvalues);
    int rc;
    if ((rc = check_rows(p, ld, locus_begin, locus_count)) || (rc = begin_gl_upload(p))) return rc;
    hipStream_t s = p->ctx->stream;
    const int64_t rows_total = GOFF + p->nloci + GPAD_BACK;
    if (!p->gl_cont) {
        std::vector<uint16_t> remap;
        if ((rc = switch_to_wide(p)) || (rc = merge_wide_table(p, values, nvalues, remap))) return rc;
        if (p->gl_wide) return upload_wide_codes(p, codes, 2, ld, locus_begin, locus_count, remap, where);
    }
    // a continuous panel: the caller's codes become values straight away
    DevBuf<uint16_t> stage;
    DevBuf<double> d_dict;
    if ((rc = d_dict.reserve((size_t)nvalues))) return rc;
    hipError_t e = hipMemcpy(d_dict.p, values, sizeof(double) * (size_t)nvalues, hipMemcpyHostToDevice);
    if (e != hipSuccess) return upload_fail("set_gl_codes16", e);
    rc = for_each_upload_slab(s, "set_gl_codes16", codes, 2 * ld, locus_count, where, stage, [&](const void *rows, int64_t at, int64_t n) {
        hipLaunchKernelGGL(gl_store_codes16_kernel, dim3(2048), dim3(256), 0, s, (const uint16_t *)rows, ld, locus_begin + at, n, p->nind,
                           d_dict.p, nvalues, rows_total, p->d_glval.p);
        return GARLIC_OK;
    });
    return rc ? rc : end_gl_upload(p, locus_begin, locus_count);
}

// ---- --tgls text (tgls_kernels.hpp): rows of 16-bit codes into a dictionary of the RAW values, and the door into a panel
// leaves its scope with the stream idle: declared behind the host lists and device buffers whose copies and readers may be pending
struct StreamDrain {
    hipStream_t s;
    ~StreamDrain() { (void)hipStreamSynchronize(s); }
};

struct garlic_tgls {
    garlic_ctx *ctx = nullptr;
    int64_t nrows = 0;
    int32_t ncols = 0, n_kept = 0;
    bool dead = false;                                      // a 65,537th raw value arrived: the file needs the host reader
    DevBuf<uint16_t> d_codes;                               // [nrows][n_kept]
    DevBuf<int32_t> d_col_dest, d_k_src;                    // column -> staged column or -1; kept column -> staged column
    std::vector<uint64_t> raw_bits;                         // the dictionary: code -> bit pattern, in the order the codes were issued
    std::vector<std::pair<uint64_t, uint16_t>> sorted;      // the same, sorted by bit pattern
    DevBuf<uint64_t> d_bits;                                // `sorted` on the device, TGLS_DICT_MAX entries of room
    DevBuf<uint16_t> d_code;
    DevBuf<unsigned long long> d_set;                       // the unknown values of an encode round
    DevBuf<int32_t> d_flags;                                // 3 words (tgls_encode_kernel)
    std::vector<uint64_t> row_set, row_deferred;            // one bit per row
    int64_t n_set = 0, n_deferred = 0;
    TextStage text;                                         // garlic_tgls_set_rows_text, garlic_tgls_set_rows_vcf
    DevBuf<double> raw;                                     // the parsed doubles [row_count][n_kept] (and the rows of set_rows_values),
    DevBuf<double> d_table, d_out;                          // and what get_rows decodes with and into
};

int garlic_tgls_create(garlic_ctx *ctx, int64_t nrows, int32_t ncols_total, const int32_t *col_idx, int32_t n_idx, garlic_tgls **out)
{
    if (!out) return fail(GARLIC_ERR_INVALID, "tgls out pointer is NULL");
    *out = nullptr;
    if (!ctx) return fail(GARLIC_ERR_INVALID, "ctx is NULL");
    if (nrows < 1 || nrows > 0x7FFFFFFF || ncols_total < 1 || ncols_total >= (1 << 28))
        return fail(GARLIC_ERR_INVALID, "need 1 <= nrows < 2^31 and 1 <= ncols_total < 2^28");
    if (col_idx && (n_idx < 1 || n_idx >= (1 << 28))) return fail(GARLIC_ERR_INVALID, "need 1 <= n_idx < 2^28, got %d", n_idx);
    const int32_t n_kept = col_idx ? n_idx : ncols_total;
    for (int32_t k = 0; col_idx && k < n_idx; k++)
        if (col_idx[k] < 0 || col_idx[k] >= ncols_total)
            return fail(GARLIC_ERR_INVALID, "col_idx[%d] = %d outside the file's %d columns", k, col_idx[k], ncols_total);
    int rc;
    if ((rc = set_device(ctx))) return rc;
    std::unique_ptr<garlic_tgls> t(new garlic_tgls);
    t->ctx = ctx;
    t->nrows = nrows;
    t->ncols = ncols_total;
    t->n_kept = n_kept;
    // a column is staged where its first kept position is; a position that names it again reads it from there
    std::vector<int32_t> dest((size_t)ncols_total, -1), src((size_t)n_kept);
    for (int32_t k = 0; k < n_kept; k++) {
        const int32_t c = col_idx ? col_idx[k] : k;
        if (dest[(size_t)c] < 0) dest[(size_t)c] = k;
        src[(size_t)k] = dest[(size_t)c];
    }
    hipStream_t s = ctx->stream;
    if ((rc = t->d_codes.reserve((size_t)(nrows * n_kept))) || (rc = t->d_col_dest.put(dest, s)) || (rc = t->d_k_src.put(src, s)) ||
        (rc = t->d_bits.reserve(TGLS_DICT_MAX)) || (rc = t->d_code.reserve(TGLS_DICT_MAX)) || (rc = t->d_set.reserve(TGLS_SET_SLOTS)) ||
        (rc = t->d_flags.reserve(3)))
        return rc;
    HIP_TRY(hipStreamSynchronize(s));                   // dest / src may go
    t->row_set.assign((size_t)((nrows + 63) / 64), 0);
    t->row_deferred.assign((size_t)((nrows + 63) / 64), 0);
    *out = t.release();
    return GARLIC_OK;
}

int garlic_tgls_destroy(garlic_tgls *t)
{
    if (!t) return GARLIC_OK;
    (void)hipSetDevice(t->ctx->device);
    (void)hipStreamSynchronize(t->ctx->stream);
    delete t;
    return GARLIC_OK;
}

static int tgls_check_rows(const garlic_tgls *t, int64_t row_begin, int64_t row_count, int32_t where)
{
    if (where != GARLIC_HOST && where != GARLIC_DEVICE) return fail(GARLIC_ERR_INVALID, "where must be GARLIC_HOST or GARLIC_DEVICE");
    if (row_begin < 0 || row_count < 1 || row_begin + row_count > t->nrows)
        return fail(GARLIC_ERR_INVALID, "row range [%lld,+%lld) outside the object's %lld rows", (long long)row_begin, (long long)row_count,
                    (long long)t->nrows);
    if (t->dead)
        return fail(GARLIC_ERR_STATE, "the object met more than %d distinct raw values and is unusable: the file needs the host reader", TGLS_DICT_MAX);
    return GARLIC_OK;
}

static void tgls_mark(garlic_tgls *t, int64_t row, bool set)
{
    uint64_t &ws = t->row_set[(size_t)(row >> 6)], &wd = t->row_deferred[(size_t)(row >> 6)];
    const uint64_t bit = 1ull << (row & 63);
    if (set) {
        if (!(ws & bit)) { ws |= bit; t->n_set++; }
        if (wd & bit) { wd &= ~bit; t->n_deferred--; }
    } else {                                                // deferred: not set until set_rows_values brings it
        if (ws & bit) { ws &= ~bit; t->n_set--; }
        if (!(wd & bit)) { wd |= bit; t->n_deferred++; }
    }
}

// Staged rows -> codes, the dictionary growing by the SORTED set of the values it does not hold, until it holds all (two
// rounds at most).  d_status: the rows' status pairs on the device, or NULL when every row is to be coded.
static int tgls_encode_rows(garlic_tgls *t, const double *d_raw, int64_t ld, const int32_t *d_status, const int32_t *d_k_src,
                            int64_t row_begin, int64_t row_count)
{
    hipStream_t s = t->ctx->stream;
    const unsigned grid = (unsigned)std::max<int64_t>(1, std::min<int64_t>((row_count * t->n_kept + 255) / 256, 2048));
    for (int round = 0;; round++) {
        HIP_TRY(hipMemsetAsync(t->d_set.p, 0xFF, sizeof(unsigned long long) * TGLS_SET_SLOTS, s));
        HIP_TRY(hipMemsetAsync(t->d_flags.p, 0, 3 * sizeof(int32_t), s));
        hipLaunchKernelGGL(tgls_encode_kernel, dim3(grid), dim3(256), 0, s, d_raw, ld, d_status, row_count, t->n_kept, d_k_src,
                           t->d_bits.p, t->d_code.p, (int)t->sorted.size(), t->d_codes.p + row_begin * t->n_kept, t->d_set.p,
                           (int32_t)(TGLS_DICT_MAX - (int)t->sorted.size()), t->d_flags.p);
        HIP_TRY(hipGetLastError());
        int32_t flags[3] = {0, 0, 0};
        HIP_TRY(hipMemcpyAsync(flags, t->d_flags.p, sizeof flags, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        if (!flags[0] && !flags[1] && !flags[2]) return GARLIC_OK;
        if (round >= 2) return fail(GARLIC_ERR_HIP, "tgls encode: values still unknown after the dictionary was extended");
        if ((int64_t)t->sorted.size() + flags[0] + (flags[1] ? 1 : 0) > TGLS_DICT_MAX) {
            t->dead = true;
            return fail(GARLIC_ERR_RANGE, "the likelihood file holds more than %d distinct raw values: it needs the host reader "
                        "(the object is unusable from here on)", TGLS_DICT_MAX);
        }
        if (flags[2]) return fail(GARLIC_ERR_HIP, "tgls encode: a value found no slot in a set that is at most half full");
        std::vector<uint64_t> set(TGLS_SET_SLOTS), fresh;
        HIP_TRY(hipMemcpy(set.data(), t->d_set.p, sizeof(uint64_t) * set.size(), hipMemcpyDeviceToHost));
        for (uint64_t b : set)
            if (b != TGLS_SET_EMPTY) fresh.push_back(b);
        if (flags[1]) fresh.push_back(TGLS_SET_EMPTY);
        std::sort(fresh.begin(), fresh.end());
        for (uint64_t b : fresh) {
            t->sorted.emplace_back(b, (uint16_t)t->raw_bits.size());
            t->raw_bits.push_back(b);
        }
        std::sort(t->sorted.begin(), t->sorted.end());
        std::vector<uint64_t> hb(t->sorted.size());
        std::vector<uint16_t> hc(t->sorted.size());
        for (size_t k = 0; k < hb.size(); k++) { hb[k] = t->sorted[k].first; hc[k] = t->sorted[k].second; }
        HIP_TRY(hipMemcpy(t->d_bits.p, hb.data(), sizeof(uint64_t) * hb.size(), hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(t->d_code.p, hc.data(), sizeof(uint16_t) * hc.size(), hipMemcpyHostToDevice));
    }
}

static const char *tgls_offence_name(int code)
{
    switch (code) {
    case TGLS_FEW_COLUMNS: return "too few sample columns";
    case TGLS_MANY_COLUMNS: return "too many sample columns";
    case TGLS_VCF_NO_KEY: return "FORMAT does not name the key";
    case TGLS_VCF_NO_VALUE: return "a called genotype without a value and no missing value given, at sample column";
    }
    return "a deferred token";
}

// What garlic_tgls_set_rows_text and garlic_tgls_set_rows_vcf share: the slab and its offsets onto the device, `parse` (the
// launch of the door's kernel: device text -> t->raw and t->text.status), the encode, the rows' bookkeeping and the refusal.
static int tgls_set_rows_parsed(garlic_tgls *t, const char *what, const char *text, int64_t text_bytes, const int64_t *line_begin,
                                int64_t row_begin, int64_t row_count, int32_t *row_status, int32_t where,
                                const std::function<void(const uint8_t *, hipStream_t)> &parse)
{
    if (text_bytes < 1) return fail(GARLIC_ERR_INVALID, "text_bytes %lld: the slab is empty", (long long)text_bytes);
    int rc;
    if ((rc = tgls_check_rows(t, row_begin, row_count, where))) return rc;
    if ((rc = text_rows_check(text_bytes, line_begin, row_count)) || (rc = set_device(t->ctx))) return rc;
    hipStream_t s = t->ctx->stream;
    const uint8_t *d_text;
    if ((rc = text_rows_stage(t->text, text, text_bytes, line_begin, row_count, where, s, &d_text)) ||
        (rc = t->raw.reserve((size_t)(row_count * t->n_kept))))
        return rc;
    parse(d_text, s);
    std::vector<int32_t> status;
    int64_t bad;
    if ((rc = text_rows_status(t->text, row_count, row_status, TGLS_DEFERRED, s, status, &bad))) return rc;
    if ((rc = tgls_encode_rows(t, t->raw.p, t->n_kept, t->text.status.p, t->d_k_src.p, row_begin, row_count))) return rc;
    for (int64_t r = 0; r < row_count; r++) {
        const int code = status[(size_t)(2 * r)];
        if (code == TGLS_OK) tgls_mark(t, row_begin + r, true);
        else if (code == TGLS_DEFERRED) tgls_mark(t, row_begin + r, false);      // (any other: its codes are unspecified, the row keeps the state it had)
    }
    if (bad >= 0)
        return fail(GARLIC_ERR_INVALID, "%s row %lld (line %lld of the call): %s (%d)", what, (long long)(row_begin + bad), (long long)bad,
                    tgls_offence_name(status[(size_t)(2 * bad)]), status[(size_t)(2 * bad + 1)]);
    return GARLIC_OK;
}

int garlic_tgls_set_rows_text(garlic_tgls *t, const char *text, int64_t text_bytes, const int64_t *line_begin, int64_t row_begin,
                              int64_t row_count, int32_t *row_status, int32_t where)
{
    if (!t || !text || !line_begin) return fail(GARLIC_ERR_INVALID, "tgls, text and line_begin are required");
    return tgls_set_rows_parsed(t, "TGLS", text, text_bytes, line_begin, row_begin, row_count, row_status, where,
                                [&](const uint8_t *d_text, hipStream_t s) {
        hipLaunchKernelGGL(tgls_parse_kernel, dim3((unsigned)row_count), dim3(256), 0, s, d_text, text_bytes, t->text.lines.p, t->ncols,
                           t->d_col_dest.p, t->raw.p, (int64_t)t->n_kept, t->text.status.p);
    });
}

int garlic_tgls_set_rows_vcf(garlic_tgls *t, const char *text, int64_t text_bytes, const int64_t *line_begin, int64_t row_begin,
                             int64_t row_count, const char *key, const double *missing_raw, int32_t *row_status, int32_t where)
{
    if (!t || !text || !line_begin || !key) return fail(GARLIC_ERR_INVALID, "tgls, text, line_begin and key are required");
    const size_t key_len = strnlen(key, VGL_KEY_MAX + 1);
    bool key_ok = key_len >= 1 && key_len <= (size_t)VGL_KEY_MAX && strcmp(key, "GT") != 0;
    for (size_t i = 0; key_ok && i < key_len; i++) {
        const char c = key[i];
        key_ok = (c >= 'A' && c <= 'Z') || (c >= 'a' && c <= 'z') || (c >= '0' && c <= '9') || c == '_' || c == '.';
    }
    if (!key_ok) return fail(GARLIC_ERR_INVALID, "key must be 1 to %d bytes of [A-Za-z0-9_.] and not GT", VGL_KEY_MAX);
    uint64_t kw[2] = {0, 0};
    memcpy(kw, key, key_len);
    return tgls_set_rows_parsed(t, "VCF likelihood", text, text_bytes, line_begin, row_begin, row_count, row_status, where,
                                [&](const uint8_t *d_text, hipStream_t s) {
        hipLaunchKernelGGL(tgls_vcf_parse_kernel, dim3((unsigned)row_count), dim3(256), 0, s, d_text, text_bytes, t->text.lines.p, t->ncols,
                           t->d_col_dest.p, kw[0], kw[1], (int32_t)key_len, missing_raw ? *missing_raw : 0.0, missing_raw ? 1 : 0,
                           t->raw.p, (int64_t)t->n_kept, t->text.status.p);
    });
}

int garlic_tgls_set_rows_values(garlic_tgls *t, const double *raw, int64_t ld, int64_t row_begin, int64_t row_count, int32_t where)
{
    if (!t || !raw) return fail(GARLIC_ERR_INVALID, "tgls and raw are required");
    int rc;
    if ((rc = tgls_check_rows(t, row_begin, row_count, where))) return rc;
    if (ld < t->n_kept) return fail(GARLIC_ERR_INVALID, "ld %lld < the object's %d kept columns", (long long)ld, t->n_kept);
    if ((rc = set_device(t->ctx))) return rc;
    hipStream_t s = t->ctx->stream;
    int64_t at_row = row_begin;
    rc = for_each_upload_slab(s, "tgls_set_rows_values", raw, 8 * ld, row_count, where, t->raw, [&](const void *rows, int64_t at, int64_t n) {
        at_row = row_begin + at;
        const int enc = tgls_encode_rows(t, (const double *)rows, ld, nullptr, nullptr, at_row, n);
        return enc ? enc : SLAB_DRAINED;
    });
    if (rc) return rc;
    for (int64_t r = 0; r < row_count; r++) tgls_mark(t, row_begin + r, true);
    return GARLIC_OK;
}

// garlic-data.cpp:1557-1576, operation for operation, with the host libm
static double tgls_convert(double gl, int32_t gl_type)
{
    if (gl_type == GARLIC_GL_GQ) { gl /= (-10.0); gl = (gl > -10) ? gl : -10; gl = pow(10, gl); }
    else if (gl_type == GARLIC_GL_GL) { gl = (gl > -10) ? gl : -10; gl = 1 - pow(10, gl); }
    else { gl /= (-10.0); gl = (gl > -10) ? gl : -10; gl = 1 - pow(10, gl); }
    if (gl <= 0) gl = 0.0000000000000001;
    if (gl > 1) gl = 1;
    return gl;
}

static bool tgls_gl_type_ok(int32_t gl_type, bool raw_too)
{
    return gl_type == GARLIC_GL_GQ || gl_type == GARLIC_GL_GL || gl_type == GARLIC_GL_PL || (raw_too && gl_type == GARLIC_TGLS_RAW);
}

// the object's table, code -> value: raw (GARLIC_TGLS_RAW) or converted
static std::vector<double> tgls_table(const garlic_tgls *t, int32_t gl_type)
{
    std::vector<double> table(t->raw_bits.size());
    for (size_t c = 0; c < table.size(); c++) {
        double v;
        memcpy(&v, &t->raw_bits[c], sizeof v);
        table[c] = gl_type == GARLIC_TGLS_RAW ? v : tgls_convert(v, gl_type);
    }
    return table;
}

int garlic_tgls_get_rows(garlic_tgls *t, int32_t gl_type, int64_t row_begin, int64_t row_count, double *out, int64_t ld, int32_t where)
{
    if (!t || !out) return fail(GARLIC_ERR_INVALID, "tgls and out are required");
    if (!tgls_gl_type_ok(gl_type, true)) return fail(GARLIC_ERR_INVALID, "gl_type must be GARLIC_TGLS_RAW or GARLIC_GL_GQ / _GL / _PL (got %d)", gl_type);
    int rc;
    if ((rc = tgls_check_rows(t, row_begin, row_count, where))) return rc;
    if (ld < t->n_kept) return fail(GARLIC_ERR_INVALID, "ld %lld < the object's %d kept columns", (long long)ld, t->n_kept);
    for (int64_t r = row_begin; r < row_begin + row_count; r++)
        if (!((t->row_set[(size_t)(r >> 6)] >> (r & 63)) & 1))
            return fail(GARLIC_ERR_STATE, "tgls row %lld is not set%s", (long long)r,
                        ((t->row_deferred[(size_t)(r >> 6)] >> (r & 63)) & 1) ? " (deferred: it waits for garlic_tgls_set_rows_values)" : "");
    if ((rc = set_device(t->ctx))) return rc;
    hipStream_t s = t->ctx->stream;
    const std::vector<double> table = tgls_table(t, gl_type);
    StreamDrain drain{s};                                   // (the table's copy may be pending at any return from here on)
    if ((rc = t->d_table.put(table, s))) return rc;
    // host rows go through a staging buffer a slab at a time, device rows are written where they are
    const int64_t slab = where == GARLIC_HOST ? std::max<int64_t>(16, ((int64_t)64 << 20) / (8 * (int64_t)t->n_kept)) : row_count;
    for (int64_t at = 0; at < row_count; at += slab) {
        const int64_t n = std::min(slab, row_count - at);
        double *dst = out + at * ld;
        int64_t dst_ld = ld;
        if (where == GARLIC_HOST) {
            if ((rc = t->d_out.reserve((size_t)(n * t->n_kept)))) return rc;
            dst = t->d_out.p;
            dst_ld = t->n_kept;
        }
        const unsigned grid = (unsigned)std::max<int64_t>(1, std::min<int64_t>((n * t->n_kept + 255) / 256, 2048));
        hipLaunchKernelGGL(tgls_decode_kernel, dim3(grid), dim3(256), 0, s, t->d_codes.p + (row_begin + at) * t->n_kept, n, t->n_kept,
                           t->d_table.p, dst, dst_ld);
        HIP_TRY(hipGetLastError());
        if (where == GARLIC_HOST)
            HIP_TRY(hipMemcpy2DAsync(out + at * ld, (size_t)(8 * ld), dst, (size_t)(8 * dst_ld), (size_t)(8 * t->n_kept), (size_t)n,
                                     hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
    }
    return GARLIC_OK;
}

int garlic_tgls_info(garlic_tgls *t, int32_t *n_raw_values, int64_t *rows_set, int64_t *rows_deferred)
{
    if (!t) return fail(GARLIC_ERR_INVALID, "tgls is NULL");
    if (n_raw_values) *n_raw_values = (int32_t)t->raw_bits.size();
    if (rows_set) *rows_set = t->n_set;
    if (rows_deferred) *rows_deferred = t->n_deferred;
    return GARLIC_OK;
}

int garlic_tgls_count_values(garlic_tgls *t, int32_t gl_type, int64_t row_begin, int64_t row_count, int32_t *n_values)
{
    if (!t || !n_values) return fail(GARLIC_ERR_INVALID, "tgls and n_values are required");
    if (!tgls_gl_type_ok(gl_type, true)) return fail(GARLIC_ERR_INVALID, "gl_type must be GARLIC_TGLS_RAW or GARLIC_GL_GQ / _GL / _PL (got %d)", gl_type);
    int rc;
    if ((rc = tgls_check_rows(t, row_begin, row_count, GARLIC_HOST))) return rc;
    for (int64_t r = row_begin; r < row_begin + row_count; r++)
        if (!((t->row_set[(size_t)(r >> 6)] >> (r & 63)) & 1)) return fail(GARLIC_ERR_STATE, "tgls row %lld is not set", (long long)r);
    if ((rc = set_device(t->ctx))) return rc;
    hipStream_t s = t->ctx->stream;
    DevBuf<uint8_t> d_used;
    if ((rc = d_used.reserve(TGLS_DICT_MAX))) return rc;
    StreamDrain drain{s};
    HIP_TRY(hipMemsetAsync(d_used.p, 0, TGLS_DICT_MAX, s));
    const int64_t n = row_count * t->n_kept;
    hipLaunchKernelGGL(tgls_mark_kernel, dim3((unsigned)std::max<int64_t>(1, std::min<int64_t>((n + 255) / 256, 2048))), dim3(256), 0, s,
                       t->d_codes.p + row_begin * t->n_kept, n, d_used.p);
    HIP_TRY(hipGetLastError());
    std::vector<uint8_t> used(TGLS_DICT_MAX);
    HIP_TRY(hipMemcpyAsync(used.data(), d_used.p, used.size(), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    const std::vector<double> table = tgls_table(t, gl_type);
    std::unordered_map<uint64_t, int> seen;
    for (size_t c = 0; c < table.size(); c++)
        if (used[c]) seen.emplace(value_bits(table[c]), 0);
    *n_values = (int32_t)seen.size();
    return GARLIC_OK;
}

int garlic_tgls_get_values(garlic_tgls *t, int32_t gl_type, double *values, int32_t n)
{
    if (!t || !values) return fail(GARLIC_ERR_INVALID, "tgls and values are required");
    if (!tgls_gl_type_ok(gl_type, true)) return fail(GARLIC_ERR_INVALID, "gl_type must be GARLIC_TGLS_RAW or GARLIC_GL_GQ / _GL / _PL (got %d)", gl_type);
    if (n < 0 || (size_t)n > t->raw_bits.size()) return fail(GARLIC_ERR_INVALID, "n = %d outside the dictionary's %zu values", n, t->raw_bits.size());
    const std::vector<double> table = tgls_table(t, gl_type);
    std::copy(table.begin(), table.begin() + n, values);
    return GARLIC_OK;
}

int garlic_panel_set_gl_tgls(garlic_panel *p, garlic_tgls *t, int32_t gl_type, int64_t ind_offset, const int64_t *dest_locus)
{
    if (!p || !t || !dest_locus) return fail(GARLIC_ERR_INVALID, "panel, tgls and dest_locus are required");
    if (!tgls_gl_type_ok(gl_type, false)) return fail(GARLIC_ERR_INVALID, "gl_type must be GARLIC_GL_GQ / _GL / _PL (got %d)", gl_type);
    if (t->ctx->device != p->ctx->device)
        return fail(GARLIC_ERR_INVALID, "the tgls object is on device %d, the panel on device %d", t->ctx->device, p->ctx->device);
    if (t->dead)
        return fail(GARLIC_ERR_STATE, "the object met more than %d distinct raw values and is unusable: the file needs the host reader", TGLS_DICT_MAX);
    if (t->n_set != t->nrows)
        return fail(GARLIC_ERR_STATE, "set_gl_tgls needs every row of the object: %lld of %lld set, %lld deferred", (long long)t->n_set,
                    (long long)t->nrows, (long long)t->n_deferred);
    if (ind_offset < 0 || ind_offset + p->nind > t->n_kept)
        return fail(GARLIC_ERR_INVALID, "individuals [%lld,+%d) outside the object's %d kept columns", (long long)ind_offset, p->nind, t->n_kept);
    // the kept rows, and the runs of consecutive destinations they form
    std::vector<int64_t> src_row;
    struct Run { int64_t first_kept, locus, count; };
    std::vector<Run> runs;
    int64_t prev = -1;
    for (int64_t r = 0; r < t->nrows; r++) {
        const int64_t l = dest_locus[r];
        if (l == -1) continue;
        if (l < 0 || l >= p->nloci) return fail(GARLIC_ERR_INVALID, "dest_locus[%lld] = %lld outside the panel's %lld loci", (long long)r, (long long)l, (long long)p->nloci);
        if (!src_row.empty() && l <= prev)
            return fail(GARLIC_ERR_INVALID, "dest_locus[%lld] = %lld: the destinations of the kept rows must be strictly ascending", (long long)r, (long long)l);
        if (!runs.empty() && l == prev + 1) runs.back().count++;
        else runs.push_back(Run{(int64_t)src_row.size(), l, 1});
        src_row.push_back(r);
        prev = l;
    }
    if (src_row.empty()) return fail(GARLIC_ERR_INVALID, "dest_locus keeps no row");
    // the dictionary converted on the host; the distinct converted values, first code first, are the table the panel gets
    const std::vector<double> conv = tgls_table(t, gl_type);
    std::vector<double> values;
    std::vector<uint16_t> map(conv.size());
    {
        std::unordered_map<uint64_t, int> seen;
        seen.reserve(2 * conv.size());
        for (size_t c = 0; c < conv.size(); c++) {
            auto ins = seen.emplace(value_bits(conv[c]), (int)values.size());
            if (ins.second) values.push_back(conv[c]);
            map[c] = (uint16_t)ins.first->second;
        }
    }
    int rc;
    if ((rc = set_device(p->ctx))) return rc;
    hipStream_t s = p->ctx->stream;
    const bool narrow = !p->gl_wide && !p->gl_cont && values.size() <= (size_t)GL_DICT_MAX;      // the one-byte door, as the host reader's codes take it
    const size_t code_bytes = narrow ? 1 : 2;
    DevBuf<int64_t> d_src;
    DevBuf<uint16_t> d_map;
    DevBuf<uint8_t> d_out;
    StreamDrain drain{s};                                   // (the lists' copies and the kernels that read the buffers: idle before they go)
    const int64_t slab = std::max<int64_t>(16, ((int64_t)64 << 20) / ((int64_t)code_bytes * p->nind));
    if ((rc = d_src.put(src_row, s)) || (rc = d_map.put(map, s)) ||
        (rc = d_out.reserve((size_t)(std::min<int64_t>(slab, (int64_t)src_row.size()) * p->nind) * code_bytes)))
        return rc;
    for (const Run &run : runs)
        for (int64_t at = 0; at < run.count; at += slab) {
            const int64_t n = std::min(slab, run.count - at);
            const unsigned grid = (unsigned)std::max<int64_t>(1, std::min<int64_t>((n * p->nind + 255) / 256, 2048));
            const int64_t *src = d_src.p + run.first_kept + at;
            if (narrow)
                hipLaunchKernelGGL(tgls_compact_kernel<uint8_t>, dim3(grid), dim3(256), 0, s, t->d_codes.p, t->n_kept, src, n, ind_offset,
                                   p->nind, d_map.p, d_out.p);
            else
                hipLaunchKernelGGL(tgls_compact_kernel<uint16_t>, dim3(grid), dim3(256), 0, s, t->d_codes.p, t->n_kept, src, n, ind_offset,
                                   p->nind, d_map.p, reinterpret_cast<uint16_t *>(d_out.p));
            HIP_TRY(hipGetLastError());
            rc = narrow ? garlic_panel_set_gl_codes(p, d_out.p, p->nind, run.locus + at, n, values.data(), (int32_t)values.size(), GARLIC_DEVICE)
                        : garlic_panel_set_gl_codes16(p, reinterpret_cast<const uint16_t *>(d_out.p), p->nind, run.locus + at, n, values.data(),
                                                      (int32_t)values.size(), GARLIC_DEVICE);
            if (rc) return rc;                              // (the doors synchronise behind their slab: d_out is free again)
        }
    HIP_TRY(hipStreamSynchronize(s));
    return GARLIC_OK;
}

// the phase planes of a panel that gets its first phase, all zero
static int ensure_phase_planes(garlic_panel *p, int nblk)
{
    if (p->d_phase.p) return GARLIC_OK;
    if (int rc = p->d_phase.reserve((size_t)nblk * p->nloci)) return rc;
    HIP_TRY(hipMemsetAsync(p->d_phase.p, 0, sizeof(uint64_t) * nblk * p->nloci, p->ctx->stream));
    return GARLIC_OK;
}

int garlic_panel_set_phase(garlic_panel *p, const uint8_t *first_copy, int64_t ld, int64_t locus_begin,
                           int64_t locus_count, int32_t where)
{
    if (!p || !first_copy) return fail(GARLIC_ERR_INVALID, "panel and first_copy are required");
    const int nblk = (int)(p->nind_pad / WAVE);
    int rc;
    if ((rc = check_rows(p, ld, locus_begin, locus_count)) || (rc = set_device(p->ctx)) || (rc = ensure_phase_planes(p, nblk))) return rc;
    hipStream_t s = p->ctx->stream;
    DevBuf<uint8_t> stage;
    rc = for_each_upload_slab(s, "set_phase", first_copy, ld, locus_count, where, stage, [&](const void *rows, int64_t at, int64_t n) {
        const int64_t waves = n * nblk;
        hipLaunchKernelGGL(phase_planes_kernel, dim3((unsigned)((waves + 3) / 4)), dim3(256), 0, s, (const uint8_t *)rows,
                           ld, locus_begin + at, n, p->nind, nblk, p->nloci, p->d_phase.p);
        return GARLIC_OK;
    });
    if (rc) return rc;
    p->have_phase = true;
    return GARLIC_OK;
}

int garlic_panel_set_phase_bits(garlic_panel *p, const uint8_t *rows, int64_t row_bytes, int64_t locus_begin, int64_t locus_count,
                                int32_t where)
{
    if (!p || !rows) return fail(GARLIC_ERR_INVALID, "panel and rows are required");
    if (row_bytes < ((int64_t)p->nind + 7) / 8) return fail(GARLIC_ERR_INVALID, "row_bytes %lld < %d bits", (long long)row_bytes, p->nind);
    const int nblk = (int)(p->nind_pad / WAVE);
    int rc;
    if ((rc = check_loci(p, locus_begin, locus_count)) || (rc = set_device(p->ctx)) || (rc = ensure_phase_planes(p, nblk))) return rc;
    hipStream_t s = p->ctx->stream;
    DevBuf<uint8_t> stage;
    rc = for_each_upload_slab(s, "set_phase_bits", rows, row_bytes, locus_count, where, stage, [&](const void *src, int64_t at, int64_t n) {
        hipLaunchKernelGGL(phase_bits_planes_kernel, dim3((unsigned)((n + WAVE - 1) / WAVE)), dim3(256), 0, s, (const uint8_t *)src,
                           row_bytes, locus_begin + at, n, p->nind, nblk, p->nloci, p->d_phase.p);
        return GARLIC_OK;
    });
    if (rc) return rc;
    p->have_phase = true;
    return GARLIC_OK;
}

int garlic_panel_set_phase_bed(garlic_panel *p, garlic_bed *b, int64_t ind_offset, const int64_t *dest_locus)
{
    if (!p || !b || !dest_locus) return fail(GARLIC_ERR_INVALID, "panel, bed and dest_locus are required");
    if (!b->have_order) return fail(GARLIC_ERR_STATE, "set_phase_bed: the image has no order plane (it carries no phase)");
    int64_t first, last;
    const int nblk = (int)(p->nind_pad / WAVE);
    int rc;
    if ((rc = bed_check_dest(p, b, ind_offset, dest_locus, first, last)) || (rc = bed_ensure_census(b)) || (rc = set_device(p->ctx)) ||
        (rc = ensure_phase_planes(p, nblk)))
        return rc;
    hipStream_t s = p->ctx->stream;
    DevBuf<int64_t> d_dest;      // (freed behind the synchronise below)
    if ((rc = d_dest.reserve((size_t)b->nrows))) return rc;
    HIP_TRY(hipMemcpyAsync(d_dest.p, dest_locus, sizeof(int64_t) * (size_t)b->nrows, hipMemcpyHostToDevice, s));
    const int64_t blocks = (b->nrows * nblk + 3) / 4;
    hipLaunchKernelGGL(bed_phase_planes_kernel, dim3((unsigned)std::min<int64_t>(blocks, 64 * (int64_t)p->ctx->n_cu)), dim3(256), 0, s,
                       b->d_image.p, b->row_bytes, b->d_order.p, b->order_row_bytes, b->d_counted.p, d_dest.p, b->nrows, ind_offset,
                       p->nind, nblk, p->nloci, p->d_phase.p);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipStreamSynchronize(s);       // also: dest_locus is free again
    if (e != hipSuccess) return upload_fail("set_phase_bed", e);
    p->have_phase = true;
    return GARLIC_OK;
}

// reciprocals of device-resident LD weights, plain and skewed (what the wLOD kernels read)
// the skewed reciprocals D[l][j] = 1 / LD[l - j][j]: the weights SNP l has in the windows that contain it as one
// contiguous row (tuned wLOD kernels); rows past the panel stay 0 (SKEW_FRONT doubles of zero padding in front:
// the kernels' first steps read up to 15 elements before a row)
// zero: clear it (skew_reciprocal_kernel's caller).  ld_sum_col_kernel writes every weight a scored window reads; what it
// leaves alone only ever reaches windows that have no score (they are computed along and written as MISSING), so its
// caller clears just the padding behind the panel, which the last windows' loads run into.
static int reserve_skew_buf(garlic_panel *p, DevBuf<double> &buf, int32_t winsize, bool zero)
{
    int rc;
    const size_t nskew = SKEW_FRONT + ((size_t)p->nloci + winsize + 64) * winsize;
    if ((rc = buf.reserve(nskew))) return rc;
    if (zero) {
        HIP_TRY(hipMemsetAsync(buf.p, 0, sizeof(double) * nskew, p->ctx->stream));
    } else {
        HIP_TRY(hipMemsetAsync(buf.p, 0, sizeof(double) * SKEW_FRONT, p->ctx->stream));
        const size_t body = SKEW_FRONT + (size_t)p->nloci * winsize;
        HIP_TRY(hipMemsetAsync(buf.p + body, 0, sizeof(double) * (nskew - body), p->ctx->stream));
    }
    return GARLIC_OK;
}
static int reserve_skew(garlic_panel *p, int32_t winsize, bool zero = true)
{
    return reserve_skew_buf(p, p->d_skew, winsize, zero);
}

// The panel's sets of LD weights: the one in use (d_skew, ld_winsize) and, after a multi call, the others.
static void drop_ld_sets(garlic_panel *p) { p->ld_sets.clear(); }
static bool select_ld(garlic_panel *p, int32_t winsize)
{
    if (p->have_ld && p->ld_winsize == winsize) return true;
    for (size_t i = 0; i < p->ld_sets.size(); i++) {
        garlic_panel::LdSet &set = *p->ld_sets[i];
        if (set.W != winsize) continue;
        std::swap(set.skew.p, p->d_skew.p);
        std::swap(set.skew.cap, p->d_skew.cap);
        std::swap(set.group, p->ld_group);
        if (p->have_ld) set.W = p->ld_winsize;
        else p->ld_sets.erase(p->ld_sets.begin() + (ptrdiff_t)i);
        p->ld_winsize = winsize;
        p->have_ld = true;
        p->rld_valid = false;          // the plain reciprocals follow the size in use (ensure_rld)
        return true;
    }
    return false;
}
// the set in use joins the others (a multi call goes on to the next size)
static void stash_ld(garlic_panel *p, int32_t group)
{
    if (!p->have_ld) return;
    std::unique_ptr<garlic_panel::LdSet> set(new garlic_panel::LdSet);
    set->W = p->ld_winsize;
    set->group = group;
    std::swap(set->skew.p, p->d_skew.p);
    std::swap(set->skew.cap, p->d_skew.cap);
    p->ld_sets.push_back(std::move(set));
    p->have_ld = false;
    p->rld_valid = false;
    p->ld_winsize = 0;
    p->ld_group = -1;
}
static void drop_all_ld(garlic_panel *p)
{
    drop_ld_sets(p);
    p->d_skew.release();
    p->d_rld.release();
    p->have_ld = p->rld_valid = false;
    p->ld_winsize = 0;
    p->ld_group = -1;
}

// skew_done: the LD kernels have written D themselves (ld_sum_col_kernel); keep_sets: inside a multi call, the other sets stay
static int install_ld(garlic_panel *p, int32_t winsize, const double *src, bool skew_done = false, bool keep_sets = false)
{
    int rc;
    hipStream_t s = p->ctx->stream;
    if (!skew_done) {
        if ((rc = reserve_skew(p, winsize))) return rc;
        for (int c = 0; c < p->nchr; c++)
            hipLaunchKernelGGL(skew_reciprocal_kernel, dim3(1024), dim3(256), 0, s, src,
                               p->d_skew.p + SKEW_FRONT, p->chr_off[c], p->chr_off[c + 1], winsize);
    }
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(s));
    p->d_rld.release();          // the plain reciprocals (generic wLOD kernel) are made from D when they are asked for
    p->rld_valid = false;
    p->have_ld = true;
    p->ld_winsize = winsize;
    p->ld_group = -1;
    if (!keep_sets) {   // a single-size call leaves exactly the one set it installs
        drop_ld_sets(p);
        p->ld_pair_passes = p->ld_sum_passes = 0;
    }
    return GARLIC_OK;
}

static int ensure_rld(garlic_panel *p)
{
    if (p->rld_valid) return GARLIC_OK;
    int rc;
    const int32_t W = p->ld_winsize;
    if ((rc = p->d_rld.reserve((size_t)p->nloci * W))) return rc;
    for (int c = 0; c < p->nchr; c++)
        hipLaunchKernelGGL(unskew_kernel, dim3(1024), dim3(256), 0, p->ctx->stream, p->d_skew.p + SKEW_FRONT, p->d_rld.p,
                           p->chr_off[c], p->chr_off[c + 1], W);
    HIP_TRY(hipGetLastError());
    p->rld_valid = true;
    return GARLIC_OK;
}

int garlic_panel_set_ld(garlic_panel *p, int32_t winsize, const double *ld, int32_t where)
{
    if (!p || !ld) return fail(GARLIC_ERR_INVALID, "panel and ld are required");
    if (winsize <= 1) return fail(GARLIC_ERR_INVALID, "winsize must be > 1");
    int rc;
    if ((rc = set_device(p->ctx))) return rc;
    const size_t n = (size_t)p->nloci * winsize;
    const double *src = ld;
    if (where == GARLIC_HOST) {
        if ((rc = p->d_stage64.reserve(n))) return rc;
        HIP_TRY(hipMemcpyAsync(p->d_stage64.p, ld, sizeof(double) * n, hipMemcpyHostToDevice,
                               p->ctx->stream));
        src = p->d_stage64.p;
    }
    rc = install_ld(p, winsize, src);
    p->d_stage64.release();
    return rc;
}

// ---- LD weights on the device (ld_kernels.hpp, ld_multi_kernel.hpp).  An LD call, step by step: arguments (ld_check) -> kernel
// form (LdForm) -> the subsample as a bitmap -> counts (ld_counts_run: bit planes and per-SNP counts, kept per subsample -> grid
// table -> one pair kernel) -> weights (ld_finish_run: zero fill -> hf -> hr2 table -> ordered sums -> install_ld) -> copy out.
// garlic_ld_counts and garlic_ld_finish are the two halves with the integer counts in between (a sharded panel adds them up over
// its shards); garlic_panel_compute_ld runs both on the panel's scratch and, where the form allows it, fused: the pair kernel goes
// on to the hr2 table and no pair table is made.  The multi-size calls run the same steps at the widest shared size, then one sum
// pass per group of sizes.
enum class LdPair { mfma, lane, tiled, flat, plain };
enum class LdSum { flat, col, tiled, plain };

// Which kernels take a call of (panel, W, phased) under the switches of the moment, and what they need.  ld_form fills it, once
// per call; everything after reads it: no later code looks at W, the phasing or the environment to pick a kernel.
struct LdForm {
    int32_t W = 0, nblk = 0;       // nblk: 64-individual blocks of the panel
    bool phased = false;
    // pair counts.  mfma: banded Gram matrices on the matrix cores (16 < W <= 129; phased: three products per block, while the
    // haplotype counts, up to 2 * nind_pad, stay below 2^22 and exact in the f32 accumulators); lane: a lane per SNP while the
    // tile's plane words fit LDS; tiled: a thread per distance (W - 1 <= 256); flat: a thread per pair (a switch); plain: a
    // workgroup per SNP, streamed from L2 -- the only one that adds into a zeroed table instead of writing every entry
    LdPair pair = LdPair::plain;
    int pair_tile = 0;             // mfma, lane, tiled: SNPs per workgroup, all chromosomes in one grid (LdPairChr)
    int mfma_nj = 0;               // mfma: 32-SNP tiles per row of the band
    int lane_stage = 0, lane_dc = 0;   // lane: blocks staged at a time, distances per pass
    size_t pair_lds = 0;           // dynamic LDS of the pair kernel (mfma: without the fused form's transposition tiles)
    bool plane_cache = true;       // the bit planes of an unchanged (genotypes, subsample) are not made again
    // ordered sums.  flat: hr2 evaluated in place, a thread per (window start, column) (W <= 16: GARLIC's default --winsize is
    // 10); col: a thread per SNP of the window over the combined hr2 table, writes the wLOD weights too (32 < W <= 512); tiled: a
    // thread per column of the LD row over two hr2 tables (W <= 256); plain: that streamed from L2, chromosome by chromosome
    LdSum sum = LdSum::plain;
    int col_threads = 0;           // col, and ld_sum_multi_kernel at this W: W + 16 SNPs in whole waves
    int sum_threads = 0;           // tiled: a thread per column, in whole waves
    int sum_b = 0;                 // col, tiled: window starts per workgroup (col: thread W + B - 1 reads one element further on odd steps)
    int pieces = 0;                // col: 1-KB requests per row of the table
    bool hr2_tile = false;         // col: the table from LDS tiles of the pair counts (ld_hr2_tile_kernel), hr2_lds bytes each
    size_t hr2_lds = 0;
    // every individual's counts in one place: the pair kernel can write the hr2 table itself (GARLIC_LD_UNFUSED: the two steps of
    // garlic_ld_counts / garlic_ld_finish, which a sharded panel needs)
    bool fusable = false;
};

constexpr size_t LD_HR2_TILE_LDS_MAX = 64 * 1024;       // ld_hr2_tile_kernel's tile

static LdForm ld_form(const garlic_panel *p, int32_t W, int32_t phased)
{
    LdForm f;
    f.W = W;
    f.nblk = (int)(p->nind_pad / WAVE);
    f.phased = phased != 0;
    const size_t planes = phased ? 4 : 2;      // plane words per (SNP, block) that a pair kernel stages
    const bool no_stage = getenv("GARLIC_LD_PAIR_L2"), no_lane = getenv("GARLIC_LD_PAIR_TILED") || no_stage;
    const bool flat = getenv("GARLIC_LD_PAIR_FLAT") && W <= 32;
    f.mfma_nj = 1 + (30 + W) / 32;
    f.lane_stage = std::min(f.nblk, getenv("GARLIC_LD_LANE_STAGE") ? atoi(getenv("GARLIC_LD_LANE_STAGE")) : 4);
    f.lane_dc = W - 1 <= 16 ? 16 : 32;
    const size_t lane_lds = sizeof(uint64_t) * planes * (size_t)f.lane_stage * (LD_LANE_T + W - 1);
    const bool counts_fit = !phased || 2 * (int64_t)p->nind_pad < LDM_COUNT_MAX;      // (wider panels keep the lane kernel)
    if (counts_fit && !flat && W > LD_SMALL_MAX_W && f.mfma_nj <= 5 && !getenv("GARLIC_LD_PAIR_NO_MFMA") && !no_lane) {
        f.pair = LdPair::mfma;
        f.pair_tile = LDM_TI;
        f.pair_lds = (size_t)2 * (phased ? 3 : 2) * (4 + f.mfma_nj - 1) * WAVE * 16;      // two buffers of {M, H} or {M, A, B}
    } else if (flat) {
        f.pair = LdPair::flat;
    } else if (W - 1 <= 256 && lane_lds <= LDS_STAGING_MAX && !no_lane) {
        f.pair = LdPair::lane;
        f.pair_tile = LD_LANE_T;
        f.pair_lds = lane_lds;
    } else if (W - 1 <= 256 && !no_stage) {
        f.pair = LdPair::tiled;
        f.pair_tile = LD_PAIR_T;
        f.pair_lds = sizeof(uint64_t) * planes * LD_PAIR_BLK * (LD_PAIR_T + W - 1);
    }
    f.plane_cache = !getenv("GARLIC_LD_NO_PLANE_CACHE");
    f.col_threads = (W + 16 + WAVE - 1) / WAVE * WAVE;
    if (W <= LD_SMALL_MAX_W && !getenv("GARLIC_LD_NO_FLAT")) {
        f.sum = LdSum::flat;
    } else if (W > LD_COL_B && W <= 512 && f.col_threads <= LD_COL_MAX_THREADS && !getenv("GARLIC_LD_SUM_BY_COLUMN") &&
               !getenv("GARLIC_LD_SUM_L2")) {
        f.sum = LdSum::col;
        f.sum_b = std::min(LD_COL_B, f.col_threads - W);
        f.pieces = (f.col_threads * 8 + 1023) / 1024;
        f.hr2_lds = sizeof(double) * (LD_HR2_T + W + (size_t)LD_HR2_T * (W + 1));
        f.hr2_tile = f.hr2_lds <= LD_HR2_TILE_LDS_MAX && !getenv("GARLIC_LD_HR2_PLAIN");
    } else if (W <= LD_SUM_MAX_W && !getenv("GARLIC_LD_SUM_L2")) {
        f.sum = LdSum::tiled;
        f.sum_threads = (W + WAVE - 1) / WAVE * WAVE;
        f.sum_b = LD_SUM_B;
    }
    f.fusable = f.pair == LdPair::mfma && f.sum == LdSum::col && !getenv("GARLIC_LD_UNFUSED");
    return f;
}

// what garlic_panel_ld_form_info reports: the form an LD call ran (fused: its pair kernel wrote the hr2 table itself)
static void ld_note_form(garlic_panel *p, const LdForm &f, bool fused)
{
    static_assert((int)LdPair::mfma == 0 && (int)LdPair::plain == 4 && (int)LdSum::flat == 0 && (int)LdSum::plain == 3, "the maps below");
    const int32_t pair_code[] = {GARLIC_LD_PAIR_MFMA, GARLIC_LD_PAIR_LANE, GARLIC_LD_PAIR_TILED, GARLIC_LD_PAIR_FLAT, GARLIC_LD_PAIR_PLAIN};
    const int32_t sum_code[] = {GARLIC_LD_SUM_FLAT, GARLIC_LD_SUM_COL, GARLIC_LD_SUM_TILED, GARLIC_LD_SUM_PLAIN};
    p->ld_last.pair = pair_code[(int)f.pair];
    p->ld_last.sum = sum_code[(int)f.sum];
    p->ld_last.fused = fused;
    p->ld_last.phased = f.phased;
}

int garlic_panel_ld_form_info(garlic_panel *p, int32_t *pair_kernel, int32_t *sum_kernel, int32_t *fused, int32_t *phased)
{
    if (!p) return fail(GARLIC_ERR_INVALID, "panel is NULL");
    if (p->ld_last.pair < 0) return fail(GARLIC_ERR_STATE, "no LD call on this panel yet");
    if (pair_kernel) *pair_kernel = p->ld_last.pair;
    if (sum_kernel) *sum_kernel = p->ld_last.sum;
    if (fused) *fused = p->ld_last.fused;
    if (phased) *phased = p->ld_last.phased;
    return GARLIC_OK;
}

static int ld_check(garlic_panel *p, int32_t winsize, int32_t phased)
{
    if (!p) return fail(GARLIC_ERR_INVALID, "panel is NULL");
    if (!p->have_geno) return fail(GARLIC_ERR_STATE, "panel needs genotypes before LD weights");
    if (phased && !p->have_phase) return fail(GARLIC_ERR_STATE, "phased LD weights need garlic_panel_set_phase first");
    if (phased && !p->have_freq) return fail(GARLIC_ERR_STATE, "phased LD weights need the allele frequencies (garlic_panel_set_freq)");
    if (winsize <= 1) return fail(GARLIC_ERR_INVALID, "winsize must be > 1");
    if ((int64_t)p->nloci * winsize * 2 >= ((int64_t)1 << 40))
        return fail(GARLIC_ERR_INVALID, "LD table of %lld x %d too large", (long long)p->nloci, winsize);
    return set_device(p->ctx);
}

// The LD subsample as one bit per individual (order and repeats do not matter for counts of a set; the reference draws distinct
// indices, garlic-data.cpp:361-362).  sub_idx == NULL: every individual; otherwise exactly the n_sub listed ones -- none when
// n_sub is 0 (a shard that holds no member of a panel-wide subsample)
static int ld_sub_bitmap(const garlic_panel *p, const int32_t *sub_idx, int32_t n_sub, std::vector<uint64_t> &sub)
{
    if (n_sub < 0 || (n_sub > 0 && !sub_idx)) return fail(GARLIC_ERR_INVALID, "bad LD subsample");
    sub.assign((size_t)(p->nind_pad / WAVE), 0);
    for (int i = 0; !sub_idx && i < p->nind; i++) sub[i >> 6] |= (uint64_t)1 << (i & 63);
    for (int k = 0; sub_idx && k < n_sub; k++) {
        const int i = sub_idx[k];
        if (i < 0 || i >= p->nind) return fail(GARLIC_ERR_INVALID, "LD subsample index %d outside panel of %d", i, p->nind);
        if (sub[i >> 6] & ((uint64_t)1 << (i & 63))) return fail(GARLIC_ERR_INVALID, "LD subsample index %d given twice", i);
        sub[i >> 6] |= (uint64_t)1 << (i & 63);
    }
    return GARLIC_OK;
}

// The subsample's bit planes (lds.m, h, o) and the per-SNP counts made with them (lds.loc_planes).  They depend on the genotypes
// and the subsample only, not on the window size: kept across calls, under a key of both.
static int ld_planes(garlic_panel *p, const LdForm &f, const std::vector<uint64_t> &sub)
{
    int rc;
    hipStream_t s = p->ctx->stream;
    auto &L = p->lds;
    const size_t npl = (size_t)f.nblk * p->nloci;
    if ((rc = L.sub.put(sub, s)) || (rc = L.m.reserve(npl)) || (rc = L.h.reserve(npl)) || (f.phased && (rc = L.o.reserve(npl))) ||
        (rc = L.loc_planes.reserve((size_t)p->nloci * 2)))
        return rc;
    uint64_t key = 0xCBF29CE484222325ull;
    for (uint64_t w : sub) key = (key ^ w) * 0x100000001B3ull;
    key = (key ^ (uint64_t)(f.phased ? 2 : 1)) * 0x100000001B3ull;
    key = (key ^ p->geno_epoch) * 0x100000001B3ull;
    key = (key ^ (uint64_t)f.nblk) * 0x100000001B3ull;
    if (L.planes_valid && L.planes_key == key && f.plane_cache) return GARLIC_OK;
    L.planes_valid = false;
    hipLaunchKernelGGL(f.phased ? ld_planes_kernel<true> : ld_planes_kernel<false>, dim3((unsigned)p->nwordrows), dim3(256), 0, s,
                       p->d_packed.p, p->nwordrows, f.nblk, L.sub.p, p->nloci, L.m.p, L.h.p, f.phased ? L.o.p : nullptr, L.loc_planes.p);
    HIP_TRY(hipGetLastError());
    L.planes_key = key;
    L.planes_valid = true;
    return GARLIC_OK;
}

// All chromosomes in one grid, `tile` SNPs per workgroup: the table on its way to lds.pair_chrs, the workgroups in *blocks.  pc
// is the host copy that the upload reads: the caller keeps it until it has synchronised.
static int ld_pair_table(garlic_panel *p, int tile, std::vector<LdPairChr> &pc, unsigned *blocks)
{
    int64_t n = 0;
    for (int c = 0; c < p->nchr; c++) {
        pc.push_back(LdPairChr{p->chr_off[c], p->chr_off[c + 1], n});
        n += (p->chr_nloci[c] + tile - 1) / tile;
    }
    *blocks = (unsigned)n;
    return p->lds.pair_chrs.put(pc, p->ctx->stream);
}

// The per-SNP frequency of the hr2 / r2 formula in lds.hf: homFreq from the per-SNP counts; phased: r2 takes FreqData::freq
// where hr2 takes homFreq (garlic-data.cpp:587-588)
static int ld_hf(garlic_panel *p, const LdForm &f, const int32_t *loc)
{
    hipStream_t s = p->ctx->stream;
    if (int rc = p->lds.hf.reserve(p->nloci)) return rc;
    if (f.phased)
        HIP_TRY(hipMemcpyAsync(p->lds.hf.p, p->freq.data(), sizeof(double) * p->nloci, hipMemcpyHostToDevice, s));
    else
        hipLaunchKernelGGL(ld_homfreq_kernel, dim3((unsigned)((p->nloci + 255) / 256)), dim3(256), 0, s, loc, p->nloci, p->lds.hf.p);
    return GARLIC_OK;
}

// room for the combined hr2 table C of ld_sum_col_kernel, 2 W doubles per SNP (+ 1 KB: the last row's last request may run over)
static int ld_reserve_table(garlic_panel *p, int32_t W) { return p->lds.fwd.reserve(2 * (size_t)p->nloci * W + 256); }
// the phased kernels' two further planes (heterozygous-or-missing, firstCopy); NULL for the unphased ones
static const uint64_t *ld_plane_o(const garlic_panel *p, const LdForm &f) { return f.phased ? p->lds.o.p : nullptr; }
static const uint64_t *ld_plane_fc(const garlic_panel *p, const LdForm &f) { return f.phased ? p->d_phase.p : nullptr; }

// fuse: the kernel goes on from the counts to the hr2 values and writes the table C (lds.fwd); pair is a token then
static int ld_pair_mfma(garlic_panel *p, const LdForm &f, unsigned blocks, int32_t *pair, bool fuse)
{
    int rc;
    decltype(&ld_pair_mfma_kernel<2, false>) const fns[2][2][4] = {
        {{ld_pair_mfma_kernel<2, false>, ld_pair_mfma_kernel<3, false>, ld_pair_mfma_kernel<4, false>, ld_pair_mfma_kernel<5, false>},
         {ld_pair_mfma_kernel<2, true>, ld_pair_mfma_kernel<3, true>, ld_pair_mfma_kernel<4, true>, ld_pair_mfma_kernel<5, true>}},
        {{ld_pair_mfma_kernel<2, false, true>, ld_pair_mfma_kernel<3, false, true>, ld_pair_mfma_kernel<4, false, true>,
          ld_pair_mfma_kernel<5, false, true>},
         {ld_pair_mfma_kernel<2, true, true>, ld_pair_mfma_kernel<3, true, true>, ld_pair_mfma_kernel<4, true, true>,
          ld_pair_mfma_kernel<5, true, true>}}};
    const auto fn = fns[f.phased][fuse][f.mfma_nj - 2];          // (16 < W: two tiles at least)
    const size_t lds = std::max(f.pair_lds, fuse ? LDM_XT_BYTES : (size_t)0);
    if (fuse && ((rc = ld_hf(p, f, p->lds.loc_planes.p)) || (rc = ld_reserve_table(p, f.W)))) return rc;
    if (lds > LDS_DEFAULT_MAX) HIP_TRY(hipFuncSetAttribute((const void *)fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(fn, dim3(blocks), dim3(256), lds, p->ctx->stream, p->lds.m.p, p->lds.h.p, f.nblk, p->nloci, p->lds.pair_chrs.p,
                       p->nchr, f.W, pair, fuse ? p->lds.hf.p : nullptr, fuse ? p->lds.fwd.p : nullptr, ld_plane_o(p, f), ld_plane_fc(p, f));
    return GARLIC_OK;
}

static int ld_pair_lane(garlic_panel *p, const LdForm &f, unsigned blocks, int32_t *pair)
{
    const auto fn = f.lane_dc == 16 ? (f.phased ? ld_pair_lane_kernel<true, 16> : ld_pair_lane_kernel<false, 16>)
                                    : (f.phased ? ld_pair_lane_kernel<true, 32> : ld_pair_lane_kernel<false, 32>);
    if (f.pair_lds > LDS_DEFAULT_MAX) HIP_TRY(hipFuncSetAttribute((const void *)fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)f.pair_lds));
    hipLaunchKernelGGL(fn, dim3(blocks), dim3(LD_LANE_T), f.pair_lds, p->ctx->stream, p->lds.m.p, p->lds.h.p, ld_plane_o(p, f),
                       ld_plane_fc(p, f), f.nblk, p->nloci, p->lds.pair_chrs.p, p->nchr, f.W, f.lane_stage, pair);
    return GARLIC_OK;
}

static int ld_pair_tiled(garlic_panel *p, const LdForm &f, unsigned blocks, int32_t *pair)
{
    const int threads = (f.W - 1 + WAVE - 1) / WAVE * WAVE;
    const auto fn = f.phased ? ld_pair_tiled_kernel<true> : ld_pair_tiled_kernel<false>;
    if (f.pair_lds > LDS_DEFAULT_MAX) HIP_TRY(hipFuncSetAttribute((const void *)fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)f.pair_lds));
    hipLaunchKernelGGL(fn, dim3(blocks), dim3(threads), f.pair_lds, p->ctx->stream, p->lds.m.p, p->lds.h.p, ld_plane_o(p, f),
                       ld_plane_fc(p, f), f.nblk, p->nloci, p->lds.pair_chrs.p, p->nchr, f.W, pair);
    return GARLIC_OK;
}

static int ld_pair_flat(garlic_panel *p, const LdForm &f, int32_t *pair)
{
    hipLaunchKernelGGL(f.phased ? ld_pair_flat_kernel<true> : ld_pair_flat_kernel<false>, dim3((unsigned)(((int64_t)p->nloci * f.W + 255) / 256)),
                       dim3(256), 0, p->ctx->stream, p->lds.m.p, p->lds.h.p, ld_plane_o(p, f), ld_plane_fc(p, f), f.nblk, p->nloci,
                       p->d_chr_off.p, p->nchr, f.W, pair);
    return GARLIC_OK;
}

// a workgroup per SNP, chromosome by chromosome; adds into a zeroed table
static int ld_pair_plain(garlic_panel *p, const LdForm &f, int32_t *pair)
{
    hipStream_t s = p->ctx->stream;
    HIP_TRY(hipMemsetAsync(pair, 0, sizeof(int32_t) * (size_t)p->nloci * f.W * 2, s));
    for (int c = 0; c < p->nchr; c++) {
        if (f.phased)
            hipLaunchKernelGGL(ld_pair_phased_kernel, dim3((unsigned)p->chr_nloci[c]), dim3(256), 0, s, p->lds.m.p, p->lds.h.p, p->lds.o.p,
                               p->d_phase.p, f.nblk, p->nloci, p->chr_off[c], p->chr_off[c + 1], f.W, pair);
        else
            hipLaunchKernelGGL(ld_pair_kernel, dim3((unsigned)p->chr_nloci[c]), dim3(256), 0, s, p->lds.m.p, p->lds.h.p, f.nblk, p->nloci,
                               p->chr_off[c], p->chr_off[c + 1], f.W, pair);
    }
    return GARLIC_OK;
}

// The integer counts of the subsample `sub` into the device tables loc [nloci][2] and pair [nloci][W][2], and from there into
// host_loc / host_pair where given.  fuse (only where f.fusable): the hr2 table of ld_finish_run is made instead, in lds.fwd, and
// pair needs no more than a token allocation.
static int ld_counts_run(garlic_panel *p, const LdForm &f, const std::vector<uint64_t> &sub, int32_t *loc, int32_t *pair, bool fuse,
                         int32_t *host_loc = nullptr, int32_t *host_pair = nullptr)
{
    int rc;
    hipStream_t s = p->ctx->stream;
    if ((rc = ld_planes(p, f, sub))) return rc;
    HIP_TRY(hipMemcpyAsync(loc, p->lds.loc_planes.p, sizeof(int32_t) * p->nloci * 2, hipMemcpyDeviceToDevice, s));
    std::vector<LdPairChr> pc;          // read by its upload; a call that succeeds has synchronised before it goes
    unsigned blocks = 0;
    if (f.pair_tile && (rc = ld_pair_table(p, f.pair_tile, pc, &blocks))) return rc;
    switch (f.pair) {
    case LdPair::mfma: rc = ld_pair_mfma(p, f, blocks, pair, fuse); break;
    case LdPair::lane: rc = ld_pair_lane(p, f, blocks, pair); break;
    case LdPair::tiled: rc = ld_pair_tiled(p, f, blocks, pair); break;
    case LdPair::flat: rc = ld_pair_flat(p, f, pair); break;
    case LdPair::plain: rc = ld_pair_plain(p, f, pair); break;
    }
    if (rc) return rc;
    HIP_TRY(hipGetLastError());
    if (host_loc) HIP_TRY(hipMemcpyAsync(host_loc, loc, sizeof(int32_t) * p->nloci * 2, hipMemcpyDeviceToHost, s));
    if (host_pair) HIP_TRY(hipMemcpyAsync(host_pair, pair, sizeof(int32_t) * (size_t)p->nloci * f.W * 2, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    return GARLIC_OK;
}

int garlic_ld_counts(garlic_panel *p, int32_t winsize, int32_t phased, const int32_t *sub_idx, int32_t n_sub,
                     int32_t *locus_counts, int32_t *pair_counts, int32_t where)
{
    int rc;
    if ((rc = ld_check(p, winsize, phased))) return rc;
    if (!locus_counts || !pair_counts) return fail(GARLIC_ERR_INVALID, "count buffers are required");
    std::vector<uint64_t> sub;
    if ((rc = ld_sub_bitmap(p, sub_idx, n_sub, sub))) return rc;
    const LdForm f = ld_form(p, winsize, phased);
    ld_note_form(p, f, false);
    if (where != GARLIC_HOST) return ld_counts_run(p, f, sub, locus_counts, pair_counts, false);
    DevBuf<int32_t> &d_loc = p->lds.loc, &d_pair = p->lds.pair;
    if ((rc = d_loc.reserve((size_t)p->nloci * 2)) || (rc = d_pair.reserve((size_t)p->nloci * winsize * 2))) return rc;
    return ld_counts_run(p, f, sub, d_loc.p, d_pair.p, false, locus_counts, pair_counts);
}

// The combined table C at pitch 2 W in lds.fwd, from pair counts at pitch W and lds.hf: what ld_sum_col_kernel and
// ld_sum_multi_kernel read (and the fused pair kernel writes itself)
static int ld_build_table(garlic_panel *p, const LdForm &f, const int32_t *pair)
{
    hipStream_t s = p->ctx->stream;
    if (int rc = ld_reserve_table(p, f.W)) return rc;
    for (int c = 0; c < p->nchr; c++) {
        const int64_t lo = p->chr_off[c], hi = p->chr_off[c + 1];
        if (f.hr2_tile)
            hipLaunchKernelGGL(ld_hr2_tile_kernel, dim3((unsigned)((hi - lo + LD_HR2_T - 1) / LD_HR2_T)), dim3(256), f.hr2_lds, s, pair,
                               p->lds.hf.p, lo, hi, f.W, p->lds.fwd.p);
        else
            hipLaunchKernelGGL(ld_hr2_kernel<true>, dim3((unsigned)(hi - lo)), dim3(128), 0, s, pair, p->lds.hf.p, lo, hi, f.W,
                               p->lds.fwd.p, (double *)nullptr);
    }
    HIP_TRY(hipGetLastError());
    return GARLIC_OK;
}

// initLDData zero-fills, and the kernels with a thread per SNP of the window write every entry of the window starts that have a
// full window: that leaves the last W - 1 rows of each chromosome
static int ld_zero_short_rows(garlic_panel *p, int32_t W, double *ld)
{
    for (int c = 0; c < p->nchr; c++) {
        const int64_t lo = p->chr_off[c], hi = p->chr_off[c + 1], from = std::max<int64_t>(lo, hi - W + 1);
        if (hi > from) HIP_TRY(hipMemsetAsync(ld + from * W, 0, sizeof(double) * (size_t)(hi - from) * W, p->ctx->stream));
    }
    return GARLIC_OK;
}

// The launch of ld_sum_col_kernel (n_small == 0) or ld_sum_multi_kernel at f.W: the instantiation for the row's 1-KB requests,
// its LDS, the grid in eights (the kernels deal their workgroups over the 8 XCDs).  The call's dominant kernel: its HIP-event
// time is what garlic_recent_kernel_ms reports for an LD call.
extern "C++" template <class K, class... A>
int ld_launch_col(garlic_panel *p, const LdForm &f, K *const (&fns)[LD_COL_MAX_PIECES], int n_small, unsigned nwork, A... args)
{
    static_assert(LD_COL_MAX_THREADS <= 128 * LD_COL_MAX_PIECES, "one instantiation per request count");
    K *const fn = fns[f.pieces - 1];
    const size_t lds = ldms_lds_bytes(f.col_threads, n_small);
    if (lds > LDS_DEFAULT_MAX) HIP_TRY(hipFuncSetAttribute((const void *)fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    (void)hist_mark(p->ctx, false);
    hipLaunchKernelGGL(fn, dim3((nwork + 7u) / 8u * 8u), dim3(f.col_threads), lds, p->ctx->stream, args..., nwork);
    (void)hist_mark(p->ctx, true);
    HIP_TRY(hipGetLastError());
    return GARLIC_OK;
}
#define LD_COL_FNS(kernel) {kernel<1>, kernel<2>, kernel<3>, kernel<4>, kernel<5>}

// the window starts of a sum kernel's grid, b per workgroup, over all chromosomes that have one; chrs is the host copy that the
// upload to lds.sum_chrs reads
static int ld_sum_table(garlic_panel *p, const LdForm &f, std::vector<LdSumChr> &chrs, unsigned *blocks)
{
    int64_t n = 0;
    for (int c = 0; c < p->nchr; c++) {
        const int64_t nstarts = p->chr_off[c + 1] - p->chr_off[c] - f.W + 1;
        if (nstarts < 1) continue;
        chrs.push_back(LdSumChr{p->chr_off[c], nstarts, n});
        n += (nstarts + f.sum_b - 1) / f.sum_b;
    }
    *blocks = (unsigned)n;
    return p->lds.sum_chrs.put(chrs, p->ctx->stream);
}

// LdSum::col, from the table in lds.fwd: the LD matrix (ld may be NULL) and the wLOD weights, which this kernel writes as well
static int ld_sum_col(garlic_panel *p, const LdForm &f, double *ld, std::vector<LdSumChr> &chrs)
{
    int rc;
    unsigned nwork = 0;
    if ((rc = ld_sum_table(p, f, chrs, &nwork)) || (rc = reserve_skew(p, f.W, false))) return rc;
    if (chrs.empty()) return GARLIC_OK;
    decltype(&ld_sum_col_kernel<1>) const fns[] = LD_COL_FNS(ld_sum_col_kernel);
    return ld_launch_col(p, f, fns, 0, nwork, p->lds.fwd.p, p->lds.sum_chrs.p, (int)chrs.size(), f.W, f.sum_b, ld, p->d_skew.p + SKEW_FRONT);
}

// LdSum::tiled and LdSum::plain: hr2 forwards and backwards in two tables (lds.fwd, lds.bwd), then the sums -- tiled: all
// chromosomes in one grid, after every hr2 value exists; plain: chromosome by chromosome
static int ld_sum_two_tables(garlic_panel *p, const LdForm &f, const int32_t *pair, double *ld, std::vector<LdSumChr> &chrs)
{
    int rc;
    hipStream_t s = p->ctx->stream;
    const int32_t W = f.W;
    const size_t n = (size_t)p->nloci * W;
    if ((rc = p->lds.fwd.reserve(n)) || (rc = p->lds.bwd.reserve(n))) return rc;
    for (int c = 0; c < p->nchr; c++) {
        const int64_t lo = p->chr_off[c], hi = p->chr_off[c + 1];
        hipLaunchKernelGGL(ld_hr2_kernel<false>, dim3((unsigned)(hi - lo)), dim3(256), 0, s, pair, p->lds.hf.p, lo, hi, W, p->lds.fwd.p,
                           p->lds.bwd.p);
        if (f.sum == LdSum::plain && hi - lo >= W)
            hipLaunchKernelGGL(ld_sum_kernel, dim3((unsigned)(hi - lo - W + 1)), dim3(256), 0, s, p->lds.fwd.p, p->lds.bwd.p, lo, W, ld);
    }
    if (f.sum == LdSum::plain) return GARLIC_OK;
    unsigned blocks = 0;
    if ((rc = ld_sum_table(p, f, chrs, &blocks))) return rc;
    if (chrs.empty()) return GARLIC_OK;
    const size_t lds = sizeof(double) * 2 * (2 * (size_t)W - 1 + 128 + f.sum_threads);
    (void)hist_mark(p->ctx, false);
    hipLaunchKernelGGL(ld_sum_tiled_kernel, dim3(blocks), dim3(f.sum_threads), lds, s, p->lds.fwd.p, p->lds.bwd.p, p->lds.sum_chrs.p,
                       (int)chrs.size(), W, ld);
    (void)hist_mark(p->ctx, true);
    return GARLIC_OK;
}

// From the counts (device tables) to the installed wLOD weights and, in ld (device, [nloci][W]), the LD matrix.  ld may be
// NULL only where the sum kernel writes the weights itself (LdSum::col): the matrix is not made at all then.  have_table: the
// pair kernel has left the hr2 table in lds.fwd (ld_counts_run with fuse) and pair is not read.
static int ld_finish_run(garlic_panel *p, const LdForm &f, const int32_t *loc, const int32_t *pair, double *ld, bool have_table,
                         bool keep_sets)
{
    int rc;
    const bool col = f.sum == LdSum::col;
    if (ld && !col) HIP_TRY(hipMemsetAsync(ld, 0, sizeof(double) * (size_t)p->nloci * f.W, p->ctx->stream));      // initLDData zero-fills
    if ((ld && col && (rc = ld_zero_short_rows(p, f.W, ld))) || (rc = ld_hf(p, f, loc))) return rc;
    std::vector<LdSumChr> chrs;         // read by its upload; a call that succeeds has synchronised (install_ld) before it goes
    switch (f.sum) {
    case LdSum::flat:
        (void)hist_mark(p->ctx, false);
        hipLaunchKernelGGL(ld_sum_flat_kernel, dim3((unsigned)(((size_t)p->nloci * f.W + 255) / 256)), dim3(256), 0, p->ctx->stream, pair,
                           p->lds.hf.p, p->d_chr_off.p, p->nchr, p->nloci, f.W, ld);
        (void)hist_mark(p->ctx, true);
        break;
    case LdSum::col:
        if (!have_table) rc = ld_build_table(p, f, pair);
        if (!rc) rc = ld_sum_col(p, f, ld, chrs);
        break;
    case LdSum::tiled:
    case LdSum::plain: rc = ld_sum_two_tables(p, f, pair, ld, chrs); break;
    }
    if (rc) return rc;
    HIP_TRY(hipGetLastError());
    return install_ld(p, f.W, ld, col, keep_sets);
}

static int ld_copy_out(double *dst, const double *src, size_t n, int32_t where)
{
    HIP_TRY(hipMemcpy(dst, src, sizeof(double) * n, where == GARLIC_HOST ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice));
    return GARLIC_OK;
}

// ld_finish_run into the device matrix the call needs (the caller's; scratch when it wants a host copy or the weights are made
// from the matrix; none when nobody asked for it and the sum kernel writes the weights itself), then the copy out
static int ld_finish_to(garlic_panel *p, const LdForm &f, const int32_t *loc, const int32_t *pair, bool have_table, double *ld_out,
                        bool host_out, bool keep_sets)
{
    int rc;
    const size_t n = (size_t)p->nloci * f.W;
    double *ld = host_out ? nullptr : ld_out;
    if (!ld && (ld_out || f.sum != LdSum::col)) {
        if ((rc = p->lds.ld.reserve(n))) return rc;
        ld = p->lds.ld.p;
    }
    if ((rc = ld_finish_run(p, f, loc, pair, ld, have_table, keep_sets))) return rc;
    return ld_out && ld != ld_out ? ld_copy_out(ld_out, ld, n, GARLIC_HOST) : GARLIC_OK;
}

int garlic_ld_finish(garlic_panel *p, int32_t winsize, int32_t phased, const int32_t *locus_counts,
                     const int32_t *pair_counts, double *ld_out, int32_t where)
{
    int rc;
    if ((rc = ld_check(p, winsize, phased))) return rc;
    if (!locus_counts || !pair_counts) return fail(GARLIC_ERR_INVALID, "count buffers are required");
    hipStream_t s = p->ctx->stream;
    if (where == GARLIC_HOST) {
        DevBuf<int32_t> &d_loc = p->lds.loc, &d_pair = p->lds.pair;
        const size_t npair = (size_t)p->nloci * winsize * 2;
        if ((rc = d_loc.reserve((size_t)p->nloci * 2)) || (rc = d_pair.reserve(npair))) return rc;
        HIP_TRY(hipMemcpyAsync(d_loc.p, locus_counts, sizeof(int32_t) * p->nloci * 2, hipMemcpyHostToDevice, s));
        HIP_TRY(hipMemcpyAsync(d_pair.p, pair_counts, sizeof(int32_t) * npair, hipMemcpyHostToDevice, s));
        locus_counts = d_loc.p; pair_counts = d_pair.p;
    }
    const LdForm f = ld_form(p, winsize, phased);
    ld_note_form(p, f, false);
    return ld_finish_to(p, f, locus_counts, pair_counts, false, ld_out, where == GARLIC_HOST, false);
}

// counts and finish on the panel's scratch (kept with the panel, as all LD scratch), fused where the form allows
static int ld_compute(garlic_panel *p, const LdForm &f, const std::vector<uint64_t> &sub, double *ld_out, bool host_out, bool keep_sets)
{
    int rc;
    DevBuf<int32_t> &d_loc = p->lds.loc, &d_pair = p->lds.pair;
    ld_note_form(p, f, f.fusable);
    if ((rc = d_loc.reserve((size_t)p->nloci * 2)) || (rc = d_pair.reserve(f.fusable ? 2 : (size_t)p->nloci * f.W * 2))) return rc;
    if ((rc = ld_counts_run(p, f, sub, d_loc.p, d_pair.p, f.fusable))) return rc;
    return ld_finish_to(p, f, d_loc.p, d_pair.p, f.fusable, ld_out, host_out, keep_sets);
}

int garlic_panel_compute_ld(garlic_panel *p, int32_t winsize, int32_t phased, const int32_t *sub_idx,
                            int32_t n_sub, double *ld_out, int32_t where)
{
    int rc;
    if ((rc = ld_check(p, winsize, phased))) return rc;
    std::vector<uint64_t> sub;
    if ((rc = ld_sub_bitmap(p, sub_idx, n_sub, sub))) return rc;
    return ld_compute(p, ld_form(p, winsize, phased), sub, ld_out, where != GARLIC_DEVICE, false);
}

// ---- LD weights of several window sizes from shared passes (ld_multi_kernel.hpp; the rule is stated in garlic_hip.h)
struct LdMultiPlan {
    std::vector<int32_t> uniq;                     // the distinct sizes, ascending
    std::vector<std::vector<int32_t>> groups;      // the shared passes (ascending), then the sizes on their own (ascending)
    size_t n_shared = 0;                           // groups [0, n_shared) go through ld_sum_multi_kernel
    int32_t wtab = 0;                              // the widest shared size: the pitch of their one pair table
};
static LdMultiPlan ld_multi_plan(const garlic_panel *p, const int32_t *winsizes, int32_t n_sizes, int32_t phased)
{
    LdMultiPlan plan;
    plan.uniq.assign(winsizes, winsizes + n_sizes);
    std::sort(plan.uniq.begin(), plan.uniq.end());
    plan.uniq.erase(std::unique(plan.uniq.begin(), plan.uniq.end()), plan.uniq.end());
    const char *solo_env = getenv("GARLIC_LD_MULTI_SOLO");
    const bool solo = solo_env && atoi(solo_env) != 0;
    std::vector<LdForm> sharing;                   // the sizes whose sums go by SNP, with their forms
    std::vector<int32_t> alone;
    for (int32_t w : plan.uniq) {
        const LdForm f = ld_form(p, w, phased);
        if (!solo && f.sum == LdSum::col) sharing.push_back(f);
        else alone.push_back(w);
    }
    if (sharing.size() < 2) { alone = plan.uniq; sharing.clear(); }      // nothing to share a pass with
    for (const LdForm &f : sharing) {
        const bool fits = !plan.groups.empty() && plan.groups.back().size() < (size_t)LDM_MAX_SIZES &&
                          ldms_lds_bytes(f.col_threads, (int)plan.groups.back().size()) <= LDMS_LDS_MAX;
        if (!fits) plan.groups.emplace_back();
        plan.groups.back().push_back(f.W);
    }
    plan.n_shared = plan.groups.size();
    plan.wtab = sharing.empty() ? 0 : sharing.back().W;
    for (int32_t w : alone) plan.groups.push_back(std::vector<int32_t>{w});
    return plan;
}

typedef std::vector<std::unique_ptr<garlic_panel::LdSet>> LdSetPool;
// a weight buffer for winsize: the one the panel held for that size before the call, or a new one
static std::unique_ptr<garlic_panel::LdSet> ld_pool_take(LdSetPool &pool, int32_t winsize)
{
    for (size_t i = 0; i < pool.size(); i++)
        if (pool[i]->W == winsize) {
            std::unique_ptr<garlic_panel::LdSet> set = std::move(pool[i]);
            pool.erase(pool.begin() + (ptrdiff_t)i);
            return set;
        }
    std::unique_ptr<garlic_panel::LdSet> set(new garlic_panel::LdSet);
    set->W = winsize;
    return set;
}

// one shared pass: the sizes g (ascending, distinct; f: the form of the widest) from the table of pitch 2 wtab in lds.fwd;
// dev_ld[i]: LD matrix of g[i] or NULL
static int ld_multi_group(garlic_panel *p, const LdForm &f, const std::vector<int32_t> &g, int32_t gid, int32_t wtab, double *const *dev_ld,
                          LdSetPool &pool)
{
    int rc;
    hipStream_t s = p->ctx->stream;
    const int32_t W = g.back(), wmin = g.front();
    std::vector<LdMultiChr> chrs;
    int64_t blocks = 0;
    for (int c = 0; c < p->nchr; c++) {
        const int64_t lo = p->chr_off[c], hi = p->chr_off[c + 1], nstarts = hi - lo - wmin + 1;
        if (nstarts < 1) continue;
        chrs.push_back(LdMultiChr{lo, hi, nstarts, blocks});
        blocks += (nstarts + f.sum_b - 1) / f.sum_b;
    }
    std::vector<std::unique_ptr<garlic_panel::LdSet>> sets;
    LdMultiSmall small{};
    small.n = (int32_t)g.size() - 1;
    for (size_t i = 0; i < g.size(); i++) {
        sets.push_back(ld_pool_take(pool, g[i]));
        sets.back()->group = gid;
        if ((rc = reserve_skew_buf(p, sets.back()->skew, g[i], false))) return rc;
        if (dev_ld[i] && (rc = ld_zero_short_rows(p, g[i], dev_ld[i]))) return rc;
        if (i + 1 < g.size()) {
            small.w[i] = g[i];
            small.ld[i] = dev_ld[i];
            small.d[i] = sets.back()->skew.p + SKEW_FRONT;
        }
    }
    if (!chrs.empty()) {
        if ((rc = p->lds.multi_chrs.put(chrs, s))) return rc;
        decltype(&ld_sum_multi_kernel<1>) const fns[] = LD_COL_FNS(ld_sum_multi_kernel);
        if ((rc = ld_launch_col(p, f, fns, small.n, (unsigned)blocks, p->lds.fwd.p, p->lds.multi_chrs.p, (int)chrs.size(), wtab, W, f.sum_b, small,
                                dev_ld[g.size() - 1], sets.back()->skew.p + SKEW_FRONT)))
            return rc;
        HIP_TRY(hipStreamSynchronize(s));          // chrs (host) is read by the copy above
    }
    p->ld_sum_passes++;
    for (auto &set : sets) p->ld_sets.push_back(std::move(set));
    return GARLIC_OK;
}

// counts == false: garlic_panel_compute_ld_multi (sub: the subsample's bitmap); counts == true: garlic_ld_finish_multi (loc, pair_all:
// device pointers, the pair counts at pitch wall)
static int ld_multi_run(garlic_panel *p, const LdMultiPlan &plan, int32_t phased, bool counts, const std::vector<uint64_t> &sub,
                        const int32_t *loc, const int32_t *pair_all, int32_t wall, double *const *dev_ld /* per plan.uniq */)
{
    int rc;
    hipStream_t s = p->ctx->stream;
    auto out_of = [&](int32_t w) { return dev_ld[std::lower_bound(plan.uniq.begin(), plan.uniq.end(), w) - plan.uniq.begin()]; };
    // what the panel held becomes the pool the new sets take their buffers from (a sweep repeats its sizes)
    LdSetPool pool;
    stash_ld(p, -1);
    pool.swap(p->ld_sets);
    p->ld_pair_passes = p->ld_sum_passes = 0;
    DevBuf<int32_t> &d_loc = p->lds.loc, &d_pair = p->lds.pair;
    // the pair counts at the pitch of w (finish): the caller's table or its first w columns
    auto pair_at = [&](int32_t w, const int32_t **out) -> int {
        if (w == wall) { *out = pair_all; return GARLIC_OK; }
        int r = d_pair.reserve((size_t)p->nloci * w * 2);
        if (r) return r;
        hipLaunchKernelGGL(ld_pair_repitch_kernel, dim3((unsigned)(((int64_t)p->nloci * w + 255) / 256)), dim3(256), 0, s, pair_all, wall,
                           p->nloci, w, d_pair.p);
        HIP_TRY(hipGetLastError());
        *out = d_pair.p;
        return GARLIC_OK;
    };
    if (plan.n_shared > 0) {             // one table at the widest shared size, in lds.fwd across all the shared groups
        const LdForm ftab = ld_form(p, plan.wtab, phased);
        const bool fuse = !counts && ftab.fusable;
        const int32_t *pair = nullptr;
        if (!counts) {
            if ((rc = d_loc.reserve((size_t)p->nloci * 2)) || (rc = d_pair.reserve(fuse ? 2 : (size_t)p->nloci * plan.wtab * 2))) return rc;
            if ((rc = ld_counts_run(p, ftab, sub, d_loc.p, d_pair.p, fuse))) return rc;
            loc = d_loc.p;
            pair = d_pair.p;
        } else if ((rc = pair_at(plan.wtab, &pair))) {
            return rc;
        }
        p->ld_pair_passes++;
        if (!fuse && ((rc = ld_hf(p, ftab, loc)) || (rc = ld_build_table(p, ftab, pair)))) return rc;
        for (size_t g = 0; g < plan.n_shared; g++) {
            std::vector<double *> outs;
            for (int32_t w : plan.groups[g]) outs.push_back(out_of(w));
            if ((rc = ld_multi_group(p, ld_form(p, plan.groups[g].back(), phased), plan.groups[g], (int32_t)g, plan.wtab, outs.data(), pool)))
                return rc;
        }
    }
    // the sizes on their own, as single-size calls; after the shared groups, whose table and counts they overwrite.  Each set
    // then joins the others
    for (size_t g = plan.n_shared; g < plan.groups.size(); g++) {
        const int32_t w = plan.groups[g][0];
        const LdForm f = ld_form(p, w, phased);
        std::unique_ptr<garlic_panel::LdSet> set = ld_pool_take(pool, w);
        std::swap(set->skew.p, p->d_skew.p);
        std::swap(set->skew.cap, p->d_skew.cap);
        set.reset();
        if (!counts) {
            rc = ld_compute(p, f, sub, out_of(w), false, true);
        } else {
            const int32_t *pair = nullptr;
            if ((rc = pair_at(w, &pair))) return rc;
            rc = ld_finish_to(p, f, loc, pair, false, out_of(w), false, true);
        }
        if (rc) return rc;
        p->ld_pair_passes++;
        p->ld_sum_passes++;
        stash_ld(p, (int32_t)g);
    }
    if (plan.n_shared > 0) {                        // the call's form: the widest sharing size's pair stage
        const LdForm ftab = ld_form(p, plan.wtab, phased);
        ld_note_form(p, ftab, !counts && ftab.fusable);
    } else if (counts) {
        ld_note_form(p, ld_form(p, plan.groups.back()[0], phased), false);
    }
    HIP_TRY(hipStreamSynchronize(s));               // the pool's leftovers are freed on return
    return GARLIC_OK;
}

static int ld_multi_call(garlic_panel *p, const int32_t *winsizes, int32_t n_sizes, int32_t phased, bool counts, const int32_t *sub_idx,
                         int32_t n_sub, const int32_t *locus_counts, const int32_t *pair_counts, double *const *ld_out, int32_t where)
{
    int rc;
    if (!p) return fail(GARLIC_ERR_INVALID, "panel is NULL");
    if (!winsizes || n_sizes < 1) return fail(GARLIC_ERR_INVALID, "at least one window size is required");
    for (int i = 0; i < n_sizes; i++)
        if ((rc = ld_check(p, winsizes[i], phased))) return rc;
    if (counts && (!locus_counts || !pair_counts)) return fail(GARLIC_ERR_INVALID, "count buffers are required");
    if (!counts && (n_sub < 0 || (n_sub > 0 && !sub_idx))) return fail(GARLIC_ERR_INVALID, "bad LD subsample");
    hipStream_t s = p->ctx->stream;
    const LdMultiPlan plan = ld_multi_plan(p, winsizes, n_sizes, phased);
    const int32_t wall = plan.uniq.back();
    // one device LD matrix per distinct size somebody wants: the caller's (device) or a temporary (host)
    std::vector<std::unique_ptr<DevBuf<double>>> tmp;
    std::vector<double *> dev_ld(plan.uniq.size(), nullptr);
    for (int i = 0; ld_out && i < n_sizes; i++) {
        if (!ld_out[i]) continue;
        const size_t u = std::lower_bound(plan.uniq.begin(), plan.uniq.end(), winsizes[i]) - plan.uniq.begin();
        if (dev_ld[u]) continue;
        if (where == GARLIC_DEVICE) { dev_ld[u] = ld_out[i]; continue; }
        tmp.emplace_back(new DevBuf<double>);
        if ((rc = tmp.back()->reserve((size_t)p->nloci * winsizes[i]))) { drop_all_ld(p); return rc; }
        dev_ld[u] = tmp.back()->p;
    }
    DevBuf<int32_t> in_loc, in_pair;                // the caller's host counts on the device (the panel's scratch is in use)
    if (counts && where == GARLIC_HOST) {
        const size_t npair = (size_t)p->nloci * wall * 2;
        if ((rc = in_loc.reserve((size_t)p->nloci * 2)) || (rc = in_pair.reserve(npair))) { drop_all_ld(p); return rc; }
        hipError_t e = hipMemcpyAsync(in_loc.p, locus_counts, sizeof(int32_t) * p->nloci * 2, hipMemcpyHostToDevice, s);
        if (e == hipSuccess) e = hipMemcpyAsync(in_pair.p, pair_counts, sizeof(int32_t) * npair, hipMemcpyHostToDevice, s);
        if (e != hipSuccess) { drop_all_ld(p); return fail(GARLIC_ERR_HIP, "LD finish: %s", hipGetErrorString(e)); }
        locus_counts = in_loc.p;
        pair_counts = in_pair.p;
    }
    std::vector<uint64_t> sub;
    rc = counts ? GARLIC_OK : ld_sub_bitmap(p, sub_idx, n_sub, sub);
    if (!rc) rc = ld_multi_run(p, plan, phased, counts, sub, locus_counts, pair_counts, wall, dev_ld.data());
    (void)hipStreamSynchronize(s);
    if (rc) {                                       // no LD weights stay installed
        drop_all_ld(p);
        return rc;
    }
    for (int i = 0; ld_out && i < n_sizes; i++) {
        if (!ld_out[i]) continue;
        const size_t u = std::lower_bound(plan.uniq.begin(), plan.uniq.end(), winsizes[i]) - plan.uniq.begin();
        if (ld_out[i] == dev_ld[u]) continue;
        if ((rc = ld_copy_out(ld_out[i], dev_ld[u], (size_t)p->nloci * winsizes[i], where))) { drop_all_ld(p); return rc; }
    }
    select_ld(p, winsizes[0]);
    return GARLIC_OK;
}

int garlic_panel_compute_ld_multi(garlic_panel *p, const int32_t *winsizes, int32_t n_sizes, int32_t phased, const int32_t *sub_idx,
                                  int32_t n_sub, double *const *ld_out, int32_t where)
{
    return ld_multi_call(p, winsizes, n_sizes, phased, false, sub_idx, n_sub, nullptr, nullptr, ld_out, where);
}

int garlic_ld_finish_multi(garlic_panel *p, const int32_t *winsizes, int32_t n_sizes, int32_t phased, const int32_t *locus_counts,
                           const int32_t *pair_counts, double *const *ld_out, int32_t where)
{
    return ld_multi_call(p, winsizes, n_sizes, phased, true, nullptr, 0, locus_counts, pair_counts, ld_out, where);
}

int garlic_panel_ld_info(garlic_panel *p, int32_t cap, int32_t *winsizes, int32_t *groups, int32_t *n_installed, int64_t *weight_bytes,
                         int32_t *n_pair_passes, int32_t *n_sum_passes)
{
    if (!p) return fail(GARLIC_ERR_INVALID, "panel is NULL");
    std::vector<std::pair<int32_t, int32_t>> sets;
    if (p->have_ld) sets.emplace_back(p->ld_winsize, p->ld_group);
    for (const auto &set : p->ld_sets) sets.emplace_back(set->W, set->group);
    std::sort(sets.begin(), sets.end());
    int64_t bytes = 0;
    for (size_t i = 0; i < sets.size(); i++) {
        bytes += (int64_t)sizeof(double) * (SKEW_FRONT + ((int64_t)p->nloci + sets[i].first + 64) * sets[i].first);
        if ((int32_t)i < cap && winsizes) winsizes[i] = sets[i].first;
        if ((int32_t)i < cap && groups) groups[i] = sets[i].second;
    }
    if (n_installed) *n_installed = (int32_t)sets.size();
    if (weight_bytes) *weight_bytes = bytes;
    if (n_pair_passes) *n_pair_passes = p->ld_pair_passes;
    if (n_sum_passes) *n_sum_passes = p->ld_sum_passes;
    return GARLIC_OK;
}

// Drops everything the panel keeps only to make the next call cheaper: LD scratch, the score and
// feed scratch of host-output / feed calls, staging buffers.  Inputs, tables, LD weights and the
// TGLS term matrix stay.
int garlic_panel_release_scratch(garlic_panel *p)
{
    if (!p) return fail(GARLIC_ERR_INVALID, "panel is NULL");
    int rc;
    if ((rc = set_device(p->ctx))) return rc;
    HIP_TRY(hipStreamSynchronize(p->ctx->stream));
    ++*p->scratch_gen;
    p->lds.release();
    p->d_out.release(); p->d_feed.release();
    p->d_stage16.release(); p->d_stage64.release(); p->d_bed_word_rows.release();
    p->fs.release(); p->ctx->fs.release(); p->ctx->kdem.release(); p->ctx->gmm.release();
    for (auto *sl : p->feed_slots) {
        HIP_TRY(hipStreamSynchronize(sl->stream));
        sl->fs.release();
    }
    return GARLIC_OK;
}

int garlic_lod_out_layout(garlic_panel *p, int32_t pitch_align, int32_t nind_out, int64_t *chr_base,
                          int64_t *chr_pitch, int64_t *total)
{
    if (!p) return fail(GARLIC_ERR_INVALID, "panel is NULL");
    if (pitch_align < 1 || nind_out < 1)
        return fail(GARLIC_ERR_INVALID, "pitch_align and nind_out must be >= 1");
    Layout L = make_layout(p, pitch_align, nind_out);
    for (int c = 0; c < p->nchr; c++) {
        if (chr_base) chr_base[c] = L.base[c];
        if (chr_pitch) chr_pitch[c] = L.pitch[c];
    }
    if (total) *total = L.total;
    return GARLIC_OK;
}

int garlic_lod_windows(garlic_panel *p, int32_t winsize, double error, int32_t max_gap,
                       int32_t use_gl, int32_t ind_begin, int32_t ind_count, int32_t pitch_align,
                       double *out, int32_t where)
{
    if (!p) return fail(GARLIC_ERR_INVALID, "panel is NULL");
    return launch_lod(p, use_gl ? MODE_LOD_GL : MODE_LOD, winsize, error, max_gap, 0, 0.0, ind_begin,
                      ind_count, pitch_align, out, where);
}

int garlic_lod_windows_multi(garlic_panel *p, const int32_t *winsizes, int32_t n_winsizes, double error,
                             int32_t max_gap, int32_t use_gl, int32_t ind_begin, int32_t ind_count,
                             int32_t pitch_align, double *out, int64_t out_stride, int32_t where)
{
    if (!p || !winsizes) return fail(GARLIC_ERR_INVALID, "panel and winsizes are required");
    if (n_winsizes < 1) return fail(GARLIC_ERR_INVALID, "n_winsizes must be >= 1");
    if (!out) return fail(GARLIC_ERR_INVALID, "out is NULL");
    const Layout L = make_layout(p, pitch_align, ind_count);
    if (out_stride < L.total)
        return fail(GARLIC_ERR_INVALID, "out_stride %lld smaller than one window size's scores (%lld doubles)",
                    (long long)out_stride, (long long)L.total);
    for (int32_t k = 0; k < n_winsizes; k++) {   // the panel stays resident: only the work list changes
        const int rc = launch_lod(p, use_gl ? MODE_LOD_GL : MODE_LOD, winsizes[k], error, max_gap, 0, 0.0, ind_begin,
                                  ind_count, pitch_align, out + (int64_t)k * out_stride, where);
        if (rc) return rc;
    }
    return GARLIC_OK;
}

int garlic_wlod_windows(garlic_panel *p, int32_t winsize, double error, int32_t max_gap, int32_t use_gl,
                        int32_t M, double mu, int32_t ind_begin, int32_t ind_count, int32_t pitch_align,
                        double *out, int32_t where)
{
    if (!p) return fail(GARLIC_ERR_INVALID, "panel is NULL");
    p->wlod_use_gl = use_gl != 0;
    return launch_lod(p, MODE_WLOD, winsize, error, max_gap, M, mu, ind_begin, ind_count, pitch_align,
                      out, where);
}

// ---- The feed in ascending order (feed_sort_kernel.hpp): nrd0's gsl_sort, src/garlic-kde.cpp:132.
// sort_reserve: everything the sort of n keys needs, before anything is enqueued (out of memory: nothing was touched).
static int sort_reserve(FeedSortScratch &fs, int64_t n)
{
    const int64_t n_tiles = (n + FS_TILE - 1) / FS_TILE;
    if (n_tiles > 0x7fffffff) return fail(GARLIC_ERR_INVALID, "feed sort: %lld keys are more tiles than one launch holds", (long long)n);
    int rc;
    if ((rc = fs.keys.reserve((size_t)n)) || (rc = fs.tiles.reserve((size_t)n_tiles * 256)) || (rc = fs.table.reserve(1))) return rc;
    return GARLIC_OK;
}

// The one sort step: `buf` (device, n > 1 doubles) sorted on stream s, every kernel enqueued at once -- the passes decide on
// the device which of them run.  copy_back: the result always ends in buf (a device copy when an odd number of passes
// ran); else it ends where sort_result says.
static int sort_feed(garlic_ctx *ctx, hipStream_t s, double *buf, int64_t n, FeedSortScratch &fs, bool copy_back)
{
    int rc;
    if ((rc = sort_reserve(fs, n))) return rc;
    const int64_t n_tiles = (n + FS_TILE - 1) / FS_TILE;
    FsTable *tab = fs.table.p;
    HIP_TRY(hipMemsetAsync(tab, 0, sizeof(FsTable), s));
    const int64_t rounds = (n + FS_HIST_KEYS - 1) / FS_HIST_KEYS;
    hipLaunchKernelGGL(fs_hist_kernel, dim3((unsigned)std::min<int64_t>(rounds, 8 * (int64_t)ctx->n_cu)), dim3(FS_THREADS), 0, s, buf, n, tab);
    hipLaunchKernelGGL(fs_plan_kernel, dim3(1), dim3(256), 0, s, tab, n);
    for (int pass = 0; pass < 8; pass++) {
        hipLaunchKernelGGL(fs_count_kernel, dim3((unsigned)n_tiles), dim3(FS_THREADS), 0, s, buf, fs.keys.p, n, n_tiles, pass, tab, fs.tiles.p);
        hipLaunchKernelGGL(fs_scan_kernel, dim3(256), dim3(FS_SCAN_THREADS), 0, s, n_tiles, pass, tab, fs.tiles.p);
        hipLaunchKernelGGL(fs_scatter_kernel, dim3((unsigned)n_tiles), dim3(FS_THREADS), 0, s, buf, fs.keys.p, n, n_tiles, pass, tab, fs.tiles.p);
    }
    if (copy_back)
        hipLaunchKernelGGL(fs_copy_back_kernel, dim3((unsigned)std::min<int64_t>((n + FS_THREADS - 1) / FS_THREADS, 16 * (int64_t)ctx->n_cu)),
                           dim3(FS_THREADS), 0, s, buf, fs.keys.p, n, tab);
    HIP_TRY(hipGetLastError());
    ctx->fs_scratch_bytes = (int64_t)fs.bytes();
    return GARLIC_OK;
}

// Waits for the sort on stream s; *from: the buffer that holds the sorted keys (buf or the scratch).  Notes the pass
// counts for garlic_feed_sort_info.
static int sort_result(garlic_ctx *ctx, hipStream_t s, double *buf, FeedSortScratch &fs, const double **from)
{
    int32_t tail[2] = {0, 0};       // FsTable::n_run, in_scratch
    HIP_TRY(hipMemcpyAsync(tail, &fs.table.p->n_run, sizeof tail, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    ctx->fs_run = tail[0];
    ctx->fs_skipped = 8 - tail[0];
    if (from) *from = tail[1] ? fs.keys.p : buf;
    return GARLIC_OK;
}

// thinned > 0: `scores` is already the thinned matrix of make_layout(.., thinned) (every column is a
// sample); else the full score matrix, sampled every `step` loci
static int flatten_impl(garlic_panel *p, const double *scores, int32_t pitch_align, int32_t nind_out,
                        int32_t step, double *feed, int64_t feed_capacity, int64_t *count, int64_t *chr_counts,
                        int32_t thinned = 0, const int32_t *d_ind_list = nullptr, int32_t n_list = 0)
{   // d_ind_list (device): the rows of the feed, in this order inside every chromosome; NULL: 0 .. nind_out-1
    if (!p || !scores || !count) return fail(GARLIC_ERR_INVALID, "panel, scores and count are required");
    if (step < 1 || pitch_align < 1 || nind_out < 1)
        return fail(GARLIC_ERR_INVALID, "step, pitch_align and nind_out must be >= 1");
    int rc;
    if ((rc = set_device(p->ctx))) return rc;
    hipStream_t s = p->ctx->stream;
    Layout L = make_layout(p, pitch_align, nind_out, thinned);
    std::vector<ChrDev> chrs(p->nchr);
    for (int c = 0; c < p->nchr; c++) {
        const int32_t cols = thinned > 0 ? (p->chr_nloci[c] + thinned - 1) / thinned : p->chr_nloci[c];
        chrs[c] = ChrDev{p->chr_off[c], L.base[c], L.pitch[c], cols, 0};
    }
    if (thinned > 0) step = 1;
    const int per_chr = d_ind_list ? n_list : nind_out;
    const int nrows = p->nchr * per_chr;
    if ((rc = p->d_chrs.reserve(chrs.size()))) return rc;
    if ((rc = p->d_row_counts.reserve((size_t)nrows))) return rc;
    p->plan.valid = false; // d_chrs is shared with the work plan
    HIP_TRY(hipMemcpyAsync(p->d_chrs.p, chrs.data(), sizeof(ChrDev) * chrs.size(), hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(feed_count_kernel, dim3((unsigned)nrows), dim3(WAVE), 0, s, scores, p->d_chrs.p, p->nchr,
                       per_chr, d_ind_list, step, p->d_row_counts.p);
    std::vector<int64_t> counts((size_t)nrows);
    HIP_TRY(hipMemcpyAsync(counts.data(), p->d_row_counts.p, sizeof(int64_t) * nrows, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    int64_t total = 0; // exclusive scan over (chromosome, individual) rows: tiny, done on the host
    if (chr_counts)
        for (int c = 0; c < p->nchr; c++) {
            chr_counts[c] = 0;
            for (int i = 0; i < per_chr; i++) chr_counts[c] += counts[(size_t)c * per_chr + i];
        }
    for (auto &c : counts) { const int64_t n = c; c = total; total += n; }
    *count = total;
    if (total > feed_capacity || total == 0) return GARLIC_OK;
    if (!feed) return fail(GARLIC_ERR_INVALID, "feed is NULL");
    HIP_TRY(hipMemcpyAsync(p->d_row_counts.p, counts.data(), sizeof(int64_t) * nrows, hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(feed_write_kernel, dim3((unsigned)nrows), dim3(WAVE), 0, s, scores, p->d_chrs.p, p->nchr,
                       per_chr, d_ind_list, step, p->d_row_counts.p, feed);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(s));
    return GARLIC_OK;
}

int garlic_lod_flatten(garlic_panel *p, const double *scores, int32_t pitch_align, int32_t nind_out,
                       int32_t step, double *feed, int64_t feed_capacity, int64_t *count)
{
    return flatten_impl(p, scores, pitch_align, nind_out, step, feed, feed_capacity, count, nullptr);
}

// LOD / wLOD scores and their thinned KDE feed in one call: the scores never leave the device.  The general form:
// the scores (full, or the chain kernel's thinned matrix) into device scratch, then garlic_lod_flatten's two passes.
static int feed_single(garlic_panel *p, int32_t winsize, double error, int32_t max_gap, int32_t use_gl,
                       int32_t weighted, int32_t M, double mu, int32_t step, const int32_t *ind_idx, int32_t n_idx,
                       double *feed, int64_t feed_capacity, int64_t *count, int64_t *chr_counts)
{
    if (!p || !count) return fail(GARLIC_ERR_INVALID, "panel and count are required");
    if (step < 1) return fail(GARLIC_ERR_INVALID, "step must be >= 1");
    if (ind_idx && n_idx < 1) return fail(GARLIC_ERR_INVALID, "an individual list needs at least one entry");
    int rc;
    ++*p->scratch_gen;
    if ((rc = set_device(p->ctx))) return rc;
    // the listed individuals (convertSubsetWinData2DoubleData's randInd[]) and the blocks that hold them
    const int nblk = (p->nind + WAVE - 1) / WAVE;
    std::vector<uint8_t> blocks;
    DevBuf<int32_t> d_list;
    if (ind_idx) {
        blocks.assign((size_t)nblk, 0);
        std::vector<uint8_t> seen((size_t)p->nind, 0);
        for (int k = 0; k < n_idx; k++) {
            const int i = ind_idx[k];
            if (i < 0 || i >= p->nind) return fail(GARLIC_ERR_INVALID, "feed individual %d outside panel of %d", i, p->nind);
            if (seen[(size_t)i]) return fail(GARLIC_ERR_INVALID, "feed individual %d listed twice", i);
            seen[(size_t)i] = 1;
            blocks[(size_t)(i >> 6)] = 1;
        }
        if ((rc = d_list.reserve((size_t)n_idx))) return rc;
        hipError_t e = hipMemcpy(d_list.p, ind_idx, sizeof(int32_t) * (size_t)n_idx, hipMemcpyHostToDevice);
        if (e != hipSuccess) return fail(GARLIC_ERR_HIP, "feed: %s", hipGetErrorString(e));
    }
    const int32_t n_rows = ind_idx ? n_idx : p->nind;
    // Unweighted --error scores with a real thinning step: the chain kernel stores only the sampled
    // windows (8/step B per window instead of 8 B, no full-size scratch).  Otherwise the full scores
    // go to the panel's device scratch (the one host-output calls use; it stays allocated, hipMalloc
    // of 8 GB per call would cost more than the kernels) and are sampled from there.
    // Weighted scores sampled at most once per window length (the reference thins with step = winsize): every
    // window is a sum of its own, so wlod_feed_kernel computes the sampled ones only, into the same thinned matrix.
    // (step < winsize: the sampled windows overlap and that kernel would do winsize / step times the per-SNP work;
    // not measured against the tuned kernels, so such steps keep the full scores.)  GARLIC_WLOD_FEED_FULL: never.
    // Unweighted scores from per-genotype likelihoods, step >= 4 as for --error: the ring chain stores the sampled windows
    // only (tgls_feed_kernel.hpp) unless decide_form says the call is not the ring chain's (exact chain possible, term
    // matrix declined or looked up, GARLIC_TGLS_NO_RING, GARLIC_TGLS_FEED_FULL): full scores then.
    int32_t thinned = (!weighted && step >= 4) ? step : 0;
    if (weighted && step >= winsize && !getenv("GARLIC_WLOD_FEED_FULL")) thinned = step;
    if (thinned && !weighted && !use_gl) {   // the exact chain (lod_exact_needed) writes full scores only
        if (!p->have_freq) return fail(GARLIC_ERR_STATE, "panel needs map, freq and genotypes before computing LOD");
        if ((rc = ensure_term_table(p, error))) return rc;
        if (lod_exact_needed(p, MODE_LOD, winsize)) thinned = 0;
    }
    garlic_panel::ScoreBuf &scores = p->d_out;
    DevBuf<double> &d_feed = p->d_feed;            // kept with the panel: window-size sweeps call this repeatedly
    if (weighted) p->wlod_use_gl = use_gl != 0;
    for (;;) {
        const Layout L = make_layout(p, 32, p->nind, thinned);
        if ((rc = scores.reserve(p->ctx, (size_t)L.total))) return rc;
        rc = launch_lod(p, weighted ? MODE_WLOD : (use_gl ? MODE_LOD_GL : MODE_LOD), winsize, error, max_gap, M, mu, 0,
                        p->nind, 32, scores.p, GARLIC_DEVICE, thinned, ind_idx ? &blocks : nullptr);
        if (rc != GARLIC_INTERNAL_NO_SAMPLED) {
            p->last_feed_form = !thinned ? GARLIC_FEED_FROM_SCORES : weighted ? GARLIC_FEED_SAMPLED_WLOD : use_gl ? GARLIC_FEED_TGLS_CHAIN : GARLIC_FEED_CHAIN;
            p->last_feed_doubles = L.total;
            break;
        }
        thinned = 0;      // the sampled-window kernel does not take this call: full scores
    }
    if (rc) return rc;
    // at most ceil(nloci_c / step) values per (chromosome, individual)
    int64_t cap = 0;
    for (int c = 0; c < p->nchr; c++) cap += ((int64_t)p->chr_nloci[c] + step - 1) / step * n_rows;
    if ((rc = d_feed.reserve((size_t)std::max<int64_t>(cap, 1)))) return rc;
    if ((rc = flatten_impl(p, scores.p, 32, p->nind, step, d_feed.p, cap, count, chr_counts, thinned,
                           ind_idx ? d_list.p : nullptr, n_idx)))
        return rc;
    if (*count > feed_capacity || *count == 0) return GARLIC_OK;
    if (!feed && !p->feed_sink) return fail(GARLIC_ERR_INVALID, "feed is NULL");
    const double *from = d_feed.p;
    if ((p->feed_order == GARLIC_FEED_ORDER_SORTED || p->feed_sink) && *count > 1) {
        if ((rc = sort_feed(p->ctx, p->ctx->stream, d_feed.p, *count, p->fs, false))) return rc;
        if ((rc = sort_result(p->ctx, p->ctx->stream, d_feed.p, p->fs, &from))) return rc;
    }
    if (p->feed_sink) {                            // garlic_lod_kde reads it where it lies
        garlic_panel::FeedSink &sink = *p->feed_sink;
        if (sink.to_slot) {                        // one size of several: out of the panel's scratch before the next size runs
            garlic_panel::FeedSlot &sl = *p->feed_slots[(size_t)sink.at];
            if ((rc = sl.feed.reserve((size_t)*count))) return rc;
            HIP_TRY(hipMemcpyAsync(sl.feed.p, from, sizeof(double) * (size_t)*count, hipMemcpyDeviceToDevice, p->ctx->stream));
            from = sl.feed.p;
        }
        sink.size[(size_t)sink.at] = garlic_panel::FeedSink::Entry{from, *count};
        return GARLIC_OK;
    }
    hipError_t e = hipMemcpy(feed, from, sizeof(double) * (size_t)*count, hipMemcpyDeviceToHost);
    if (e != hipSuccess) return fail(GARLIC_ERR_HIP, "feed copy-out: %s", hipGetErrorString(e));
    return GARLIC_OK;
}

int garlic_lod_feed_subset(garlic_panel *p, int32_t winsize, double error, int32_t max_gap, int32_t use_gl,
                           int32_t weighted, int32_t M, double mu, int32_t step, const int32_t *ind_idx, int32_t n_idx,
                           double *feed, int64_t feed_capacity, int64_t *count, int64_t *chr_counts)
{
    if (!p || !count) return fail(GARLIC_ERR_INVALID, "panel and count are required");
    // unweighted --error scores with a real thinning step: the chain kernel writes the feed itself (garlic_lod_feed_multi)
    if (!weighted && !use_gl && step >= 4)
        return garlic_lod_feed_multi(p, &winsize, &step, 1, error, max_gap, ind_idx, n_idx, &feed, &feed_capacity, count, chr_counts);
    return feed_single(p, winsize, error, max_gap, use_gl, weighted, M, mu, step, ind_idx, n_idx, feed, feed_capacity, count,
                       chr_counts);
}

int garlic_lod_feed(garlic_panel *p, int32_t winsize, double error, int32_t max_gap, int32_t use_gl,
                    int32_t weighted, int32_t M, double mu, int32_t step, double *feed,
                    int64_t feed_capacity, int64_t *count, int64_t *chr_counts)
{
    return garlic_lod_feed_subset(p, winsize, error, max_gap, use_gl, weighted, M, mu, step, nullptr, 0, feed,
                                  feed_capacity, count, chr_counts);
}

// one FeedSlot (stream, events, scratch) per window size of a multi-size feed call, kept with the panel
static int ensure_feed_slots(garlic_panel *p, int32_t n_sizes)
{
    while ((int)p->feed_slots.size() < n_sizes) {
        auto *sl = new garlic_panel::FeedSlot;            // (joins the panel's slots only once it is complete)
        bool ok = hipStreamCreateWithFlags(&sl->stream, hipStreamNonBlocking) == hipSuccess;
        const bool ok0 = ok && hipEventCreate(&sl->ev0) == hipSuccess;
        const bool ok1 = ok0 && hipEventCreate(&sl->ev1) == hipSuccess;
        if (!ok1) {
            if (ok0) (void)hipEventDestroy(sl->ev0);
            if (ok) (void)hipStreamDestroy(sl->stream);
            delete sl;
            return fail(GARLIC_ERR_HIP, "feed: stream / event creation failed");
        }
        p->feed_slots.push_back(sl);
    }
    return GARLIC_OK;
}

// The KDE feeds of several window sizes in one call (exploreWinsizes / selectWinsizeFromList run the same panel
// through every size of --winsize-multi, src/garlic-roh.cpp:726-751, 881-920).
//
// The window mask depends on positions only (the same for every individual), so which sampled loci hold a score --
// and the place of every sample in convertWinData2DoubleData's chromosome -> individual -> locus order -- is known
// before anything is computed: lod_feed_kernel stores every sample straight into the feed (row = position in the
// individual list, column = rank among the chromosome's scored samples).  No thinned score matrix, no compaction
// pass.  (That needs every scored window to be a finite number other than -9999, i.e. finite terms and
// !lod_exact_needed; otherwise, and for steps below 4, the single-size path runs: scores, then garlic_lod_flatten.)
// Each size has a stream and a feed buffer of its own and every size's kernel is enqueued before the first feed is
// fetched: the tail of one size's chain kernel (its longest runs, a few waves per CU) runs beside the bulk of the
// next size's, and a feed crosses PCIe while the following sizes are computed.
int garlic_lod_feed_multi(garlic_panel *p, const int32_t *winsizes, const int32_t *steps, int32_t n_sizes, double error,
                          int32_t max_gap, const int32_t *ind_idx, int32_t n_idx, double *const *feeds,
                          const int64_t *feed_capacity, int64_t *counts, int64_t *chr_counts)
{
    if (!p || !winsizes || !steps || !feeds || !feed_capacity || !counts)
        return fail(GARLIC_ERR_INVALID, "panel, winsizes, steps, feeds, feed_capacity and counts are required");
    if (n_sizes < 1) return fail(GARLIC_ERR_INVALID, "n_sizes must be >= 1");
    if (ind_idx && n_idx < 1) return fail(GARLIC_ERR_INVALID, "an individual list needs at least one entry");
    for (int i = 0; i < n_sizes; i++) {
        if (winsizes[i] <= 1) return fail(GARLIC_ERR_INVALID, "SNP window size must be > 1 (got %d)", winsizes[i]);
        if (steps[i] < 1) return fail(GARLIC_ERR_INVALID, "step must be >= 1");
    }
    garlic_ctx *ctx = p->ctx;
    int rc;
    ++*p->scratch_gen;
    if ((rc = set_device(ctx))) return rc;
    if (!p->have_map || !p->have_freq || !p->have_geno)
        return fail(GARLIC_ERR_STATE, "panel needs map, freq and genotypes before computing LOD");
    bool direct = !getenv("GARLIC_FEED_SERIAL");
    for (int i = 0; i < n_sizes && direct; i++) direct = steps[i] >= 4;
    if (direct) {
        if ((rc = ensure_segments(p, max_gap))) return rc;
        if ((rc = ensure_term_table(p, error))) return rc;
        direct = p->tab_all_finite;
        for (int i = 0; i < n_sizes && direct; i++) direct = !lod_exact_needed(p, MODE_LOD, winsizes[i]);
    }
    if (!direct) {
        for (int i = 0; i < n_sizes; i++) {
            if (p->feed_sink) p->feed_sink->at = i;
            if ((rc = feed_single(p, winsizes[i], error, max_gap, 0, 0, 0, 0.0, steps[i], ind_idx, n_idx, feeds[i],
                                  feed_capacity[i], &counts[i], chr_counts ? chr_counts + (size_t)i * p->nchr : nullptr)))
                return rc;
        }
        return GARLIC_OK;
    }
    p->last_feed_form = GARLIC_FEED_CHAIN;      // the samples go straight into the feeds: no score matrix of any kind
    p->last_feed_doubles = 0;
    // rows of the feed: the listed individuals in list order, or everyone
    const int nblk = (p->nind + WAVE - 1) / WAVE;
    const int nrows = ind_idx ? n_idx : p->nind;
    std::vector<uint8_t> blocks;
    std::vector<int32_t> row_map;
    DevBuf<int32_t> d_rowmap;
    // one way out: whatever was enqueued on the sizes' streams has finished (the next call reuses their scratch) and the
    // row map is released
    auto done = [&](int code) {
        if (code != GARLIC_OK)
            for (auto *sl : p->feed_slots) (void)hipStreamSynchronize(sl->stream);
        d_rowmap.release();
        return code;
    };
#define FEED_TRY(expr)                                                                              \
    do {                                                                                            \
        hipError_t e_ = (expr);                                                                     \
        if (e_ != hipSuccess) return done(fail(GARLIC_ERR_HIP, "feed: %s: %s", #expr, hipGetErrorString(e_))); \
    } while (0)
    const bool sorted = p->feed_order == GARLIC_FEED_ORDER_SORTED || p->feed_sink;
    if (ind_idx) {
        blocks.assign((size_t)nblk, 0);
        row_map.assign((size_t)p->nind, -1);
        for (int k = 0; k < n_idx; k++) {
            const int i = ind_idx[k];
            if (i < 0 || i >= p->nind) return fail(GARLIC_ERR_INVALID, "feed individual %d outside panel of %d", i, p->nind);
            if (row_map[(size_t)i] >= 0) return fail(GARLIC_ERR_INVALID, "feed individual %d listed twice", i);
            row_map[(size_t)i] = k;
            blocks[(size_t)(i >> 6)] = 1;
        }
        if ((rc = d_rowmap.reserve((size_t)p->nind))) return done(rc);
        hipError_t e = hipMemcpy(d_rowmap.p, row_map.data(), sizeof(int32_t) * (size_t)p->nind, hipMemcpyHostToDevice);
        if (e != hipSuccess) return done(fail(GARLIC_ERR_HIP, "feed: %s", hipGetErrorString(e)));
    }
    if ((rc = ensure_feed_slots(p, n_sizes))) return done(rc);
    FEED_TRY(hipStreamSynchronize(ctx->stream));          // uploads and earlier calls on the context's stream
    // ---- plans and their uploads, all sizes, before any kernel is enqueued (an upload from pageable memory waits
    //      for the device to take it: behind a running chain kernel it would hold back the sizes that follow)
    std::vector<size_t> n_items((size_t)n_sizes, 0);
    std::vector<int> grids((size_t)n_sizes, 1);      // workgroups each size's kernel is launched with (feed_grid)
    std::vector<int64_t> total((size_t)n_sizes, 0);
    for (int i = 0; i < n_sizes; i++) {
        garlic_panel::FeedSlot &sl = *p->feed_slots[(size_t)i];
        const int32_t W = winsizes[i], step = steps[i];
        std::vector<Run> runs;
        std::vector<FillItem> fill;
        int64_t n_valid = 0;
        plan_runs(p, W, runs, fill, n_valid);             // in chromosome and position order
        // rank of every run's first sample among its chromosome's scored samples; samples per chromosome
        std::vector<int32_t> col0(runs.size(), -1);
        std::vector<int64_t> nkeep((size_t)p->nchr, 0);
        for (size_t r = 0; r < runs.size(); r++) {
            const int64_t s = ((int64_t)runs[r].a + step - 1) / step * step;
            if (s > runs[r].b) continue;
            col0[r] = (int32_t)nkeep[(size_t)runs[r].chr];
            nkeep[(size_t)runs[r].chr] += (runs[r].b - s) / step + 1;
        }
        std::vector<FeedItem> items;
        build_feed_items(runs, longest_first(runs), ind_idx ? &blocks : nullptr, nblk, col0, items);
        std::vector<ChrDev> chrs((size_t)p->nchr);
        int64_t off = 0;
        for (int c = 0; c < p->nchr; c++) {
            chrs[(size_t)c] = ChrDev{p->chr_off[c], off, nkeep[(size_t)c], p->chr_nloci[c], 1};
            if (chr_counts) chr_counts[(size_t)i * p->nchr + c] = nkeep[(size_t)c] * nrows;
            if (nkeep[(size_t)c] * 8 * (int64_t)nrows >= (int64_t)1 << 32)
                return done(fail(GARLIC_ERR_INVALID, "chromosome %d: feed rows beyond 32-bit offsets", c));
            off += nkeep[(size_t)c] * nrows;
        }
        total[(size_t)i] = off;
        counts[i] = off;
        n_items[(size_t)i] = items.size();
        if (off > feed_capacity[i] || off == 0) { n_items[(size_t)i] = 0; continue; }
        if (!items.empty() && (rc = feed_grid(ctx, items, &grids[(size_t)i], nullptr))) return done(rc);
        if (!feeds[i] && !p->feed_sink) return done(fail(GARLIC_ERR_INVALID, "feed %d is NULL", i));
        if ((rc = sl.items.reserve(std::max<size_t>(items.size(), 1)))) return done(rc);
        if ((rc = sl.chrs.reserve((size_t)p->nchr))) return done(rc);
        if ((rc = sl.counter.reserve(4))) return done(rc);
        if ((rc = sl.feed.reserve((size_t)off))) return done(rc);
        if (sorted && off > 1 && (rc = sort_reserve(sl.fs, off))) return done(rc);
        FEED_TRY(hipMemcpy(sl.chrs.p, chrs.data(), sizeof(ChrDev) * (size_t)p->nchr, hipMemcpyHostToDevice));
        if (!items.empty()) FEED_TRY(hipMemcpy(sl.items.p, items.data(), sizeof(FeedItem) * items.size(), hipMemcpyHostToDevice));
        FEED_TRY(hipMemset(sl.counter.p, 0, 2 * sizeof(int32_t)));
    }
    p->plan.valid = false;
    // ---- every size's chain kernel, each on its own stream; every element of a feed is written by its kernel
    for (int i = 0; i < n_sizes; i++) {
        garlic_panel::FeedSlot &sl = *p->feed_slots[(size_t)i];
        FEED_TRY(hipEventRecord(sl.ev0, sl.stream));
        if (n_items[(size_t)i]) {
            FeedArgs f{p->d_packed.p, p->d_tab.p, sl.items.p, sl.chrs.p, sl.feed.p, ind_idx ? d_rowmap.p : nullptr, p->nwordrows, 0,
                       p->nind, winsizes[i], (int32_t)n_items[(size_t)i], steps[i], getenv("GARLIC_FEED_NO_ASM") ? 0 : 1,
                       sl.counter.p, nullptr};
            void *kargs[] = {(void *)&f};
            FEED_TRY(hipLaunchKernel((const void *)lod_feed_kernel, dim3((unsigned)grids[(size_t)i]), dim3(FEED_G * WAVE), kargs, 0, sl.stream));
        }
        FEED_TRY(hipEventRecord(sl.ev1, sl.stream));
        FEED_TRY(hipGetLastError());
        // ascending order: the sort follows the chain on the size's own stream, nothing is waited for here
        if (sorted && n_items[(size_t)i] && total[(size_t)i] > 1 && (rc = sort_feed(ctx, sl.stream, sl.feed.p, total[(size_t)i], sl.fs, false)))
            return done(rc);
    }
    // ---- the feeds, in order
    for (int i = 0; i < n_sizes; i++) {
        garlic_panel::FeedSlot &sl = *p->feed_slots[(size_t)i];
        if (!n_items[(size_t)i]) continue;
        const double *from = sl.feed.p;
        if (sorted && total[(size_t)i] > 1 && (rc = sort_result(ctx, sl.stream, sl.feed.p, sl.fs, &from))) return done(rc);
        if (p->feed_sink) {                        // garlic_lod_kde, garlic_lod_kde_multi: the feed stays in the slot's buffers
            p->feed_sink->size[(size_t)i] = garlic_panel::FeedSink::Entry{from, total[(size_t)i]};
            continue;
        }
        FEED_TRY(hipMemcpyAsync(feeds[i], from, sizeof(double) * (size_t)total[(size_t)i], hipMemcpyDeviceToHost, sl.stream));
    }
    float ms_sum = 0.f;
    for (int i = 0; i < n_sizes; i++) {
        garlic_panel::FeedSlot &sl = *p->feed_slots[(size_t)i];
        FEED_TRY(hipStreamSynchronize(sl.stream));
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, sl.ev0, sl.ev1) == hipSuccess) ms_sum += ms;
    }
    p->stats = garlic_call_stats{};
    p->stats.chain_kernel_ms = ms_sum;    // (the sizes overlap: the sum of their spans, not wall time)
    p->stats_pending = false;
    return done(GARLIC_OK);
#undef FEED_TRY
}

// Which sizes of a garlic_lod_feed_multi_tgls call share a chain launch (include/garlic_hip.h states the rule): `shared[i]`
// says whether size i can take the thinned ring form at all.  Returns the number of groups.
static int32_t tgls_multi_groups(const int32_t *winsizes, int32_t n, const std::vector<uint8_t> &ring_ok, bool solo,
                                 std::vector<int32_t> &group)
{
    std::vector<int32_t> order((size_t)n);
    for (int i = 0; i < n; i++) order[(size_t)i] = i;
    std::stable_sort(order.begin(), order.end(), [&](int x, int y) { return winsizes[x] < winsizes[y]; });
    group.assign((size_t)n, -1);
    int32_t n_groups = 0, in_group = 0;
    for (int i : order)       // ascending: the sizes one ring serves, cut every TGM_MAX_SIZES
        if (ring_ok[(size_t)i] && winsizes[i] <= TG_SINGLE_MAX_W) {
            if (in_group == 0 || in_group == TGM_MAX_SIZES || solo) { n_groups++; in_group = 0; }
            group[(size_t)i] = n_groups - 1;
            in_group++;
        }
    for (int i : order)       // then, ascending again, every other size on its own
        if (group[(size_t)i] < 0) group[(size_t)i] = n_groups++;
    return n_groups;
}

// The TGLS KDE feeds of several window sizes in one call: garlic_lod_feed_multi's counterpart for per-genotype likelihoods
// (the reference's sweeps run with USE_GL as they do with --error).  The sizes that take the thinned ring form are chained
// group by group over one pass of the term matrix (tgls_feed_multi_kernel.hpp; a group of one: tgls_feed_kernel) -- under
// a term budget every slab is built once for the whole call -- each size into a thinned matrix of its own, which is then
// flattened per size on the size's own stream.  Every other size goes through feed_single, after the groups.
int garlic_lod_feed_multi_tgls(garlic_panel *p, const int32_t *winsizes, const int32_t *steps, int32_t n_sizes, int32_t max_gap,
                               const int32_t *ind_idx, int32_t n_idx, double *const *feeds, const int64_t *feed_capacity,
                               int64_t *counts, int64_t *chr_counts)
{
    if (!p || !winsizes || !steps || !feeds || !feed_capacity || !counts)
        return fail(GARLIC_ERR_INVALID, "panel, winsizes, steps, feeds, feed_capacity and counts are required");
    if (n_sizes < 1) return fail(GARLIC_ERR_INVALID, "n_sizes must be >= 1");
    if (ind_idx && n_idx < 1) return fail(GARLIC_ERR_INVALID, "an individual list needs at least one entry");
    for (int i = 0; i < n_sizes; i++) {
        if (winsizes[i] <= 1) return fail(GARLIC_ERR_INVALID, "SNP window size must be > 1 (got %d)", winsizes[i]);
        if (steps[i] < 1) return fail(GARLIC_ERR_INVALID, "step must be >= 1");
    }
    garlic_ctx *ctx = p->ctx;
    hipStream_t s = ctx->stream;
    int rc;
    ++*p->scratch_gen;
    if ((rc = set_device(ctx))) return rc;
    const int nblk = (p->nind + WAVE - 1) / WAVE;
    const int nrows = ind_idx ? n_idx : p->nind;
    std::vector<uint8_t> blocks;
    DevBuf<int32_t> d_list;
    if (ind_idx) {
        blocks.assign((size_t)nblk, 0);
        std::vector<uint8_t> seen((size_t)p->nind, 0);
        for (int k = 0; k < n_idx; k++) {
            const int i = ind_idx[k];
            if (i < 0 || i >= p->nind) return fail(GARLIC_ERR_INVALID, "feed individual %d outside panel of %d", i, p->nind);
            if (seen[(size_t)i]) return fail(GARLIC_ERR_INVALID, "feed individual %d listed twice", i);
            seen[(size_t)i] = 1;
            blocks[(size_t)(i >> 6)] = 1;
        }
    }
    // ---- which sizes the thinned ring chain takes (decide_form, as for a single call), and with what term matrix
    double dummy = 0.0;
    std::vector<uint8_t> ring_ok((size_t)n_sizes, 0);
    int32_t slab_blocks = 0;
    bool have_form = false;
    for (int i = 0; i < n_sizes; i++) {
        if (steps[i] < 4) continue;
        const LodCall c{MODE_LOD_GL, winsizes[i], max_gap, 0, 0, p->nind, 32, steps[i], GARLIC_DEVICE, 32, 0.0, 0.0, &dummy,
                        ind_idx ? &blocks : nullptr};
        LodForm form;
        if ((rc = check_lod_args(p, c))) return rc;
        rc = decide_form(p, c, form);
        if (rc == GARLIC_INTERNAL_NO_SAMPLED) continue;
        if (rc) return rc;
        if (form.family != Family::tgls_feed) continue;
        if (!have_form) slab_blocks = form.slab_blocks;
        have_form = true;
        ring_ok[(size_t)i] = 1;
    }
    std::vector<int32_t> group;
    const int32_t n_groups = tgls_multi_groups(winsizes, n_sizes, ring_ok, getenv("GARLIC_TGLS_FEED_MULTI_SOLO") != nullptr, group);
    p->multi_forms.assign((size_t)n_sizes, GARLIC_FEED_FROM_SCORES);
    p->multi_groups = group;
    p->multi_chain_launches = p->multi_term_builds = 0;
    // the ring groups: their sizes in ascending order
    struct Group { std::vector<int> sizes; std::vector<size_t> item0, n_items; };     // item ranges per slab (one range: whole matrix)
    std::vector<Group> G;
    {
        std::vector<int32_t> order((size_t)n_sizes);
        for (int i = 0; i < n_sizes; i++) order[(size_t)i] = i;
        std::stable_sort(order.begin(), order.end(), [&](int x, int y) { return winsizes[x] < winsizes[y]; });
        std::vector<int> slot((size_t)n_groups, -1);
        for (int i : order) {
            if (!ring_ok[(size_t)i]) continue;
            int &g = slot[(size_t)group[(size_t)i]];
            if (g < 0) { g = (int)G.size(); G.emplace_back(); }
            G[(size_t)g].sizes.push_back(i);
        }
    }
    for (const Group &g : G)
        for (int i : g.sizes) p->multi_forms[(size_t)i] = g.sizes.size() >= 2 ? GARLIC_FEED_TGLS_CHAIN_SHARED : GARLIC_FEED_TGLS_CHAIN;

    // one way out of the part that enqueues: every stream used has finished (the next call reuses the scratch)
    auto done = [&](int code) {
        if (code != GARLIC_OK) {
            (void)hipStreamSynchronize(s);
            if (p->slab_stream) (void)hipStreamSynchronize(p->slab_stream);
            for (auto *sl : p->feed_slots) (void)hipStreamSynchronize(sl->stream);
        }
        d_list.release();
        return code;
    };
#define FEED_TRY(expr)                                                                              \
    do {                                                                                            \
        hipError_t e_ = (expr);                                                                     \
        if (e_ != hipSuccess) return done(fail(GARLIC_ERR_HIP, "feed: %s: %s", #expr, hipGetErrorString(e_))); \
    } while (0)
    if (!G.empty()) {
        if ((rc = ensure_feed_slots(p, n_sizes))) return rc;
        FEED_TRY(hipStreamSynchronize(s));          // uploads and earlier calls on the context's stream
        if (ind_idx) {
            if ((rc = d_list.reserve((size_t)n_idx))) return done(rc);
            FEED_TRY(hipMemcpy(d_list.p, ind_idx, sizeof(int32_t) * (size_t)n_idx, hipMemcpyHostToDevice));
        }
        // ---- slabs of the call (as plan_lod cuts them: a slab begins at the next block in play), or one range of all blocks
        std::vector<Plan::Slab> slabs;
        const int per_list = slab_blocks ? slab_blocks : std::max(nblk, 1);
        for (int k0 = 0; k0 < nblk;) {
            if (ind_idx && !blocks[(size_t)k0]) { k0++; continue; }
            const int k1 = std::min(nblk, k0 + per_list);
            slabs.push_back(Plan::Slab{k0, k1, 0, 0});
            k0 = k1;
        }
        // ---- work lists: per group the stretches that hold its smallest size, longest first, x the blocks in play of each slab
        std::vector<ChainItem> items;
        bool any_items = false;
        for (Group &g : G) {
            const int32_t Wmin = winsizes[g.sizes[0]];
            std::vector<Run> runs;
            std::vector<FillItem> fill;
            int64_t n_valid = 0;
            plan_runs(p, Wmin, runs, fill, n_valid);
            const std::vector<int> order = longest_first(runs);
            // (tgls_feed_kernel: b is the run's last window; tgls_feed_multi_kernel: the stretch's last SNP)
            const int32_t b_add = g.sizes.size() >= 2 ? Wmin - 1 : 0;
            for (const Plan::Slab &sl : slabs) {
                g.item0.push_back(items.size());
                for (size_t r = 0; r < order.size(); r++) {
                    const Run &run = runs[(size_t)order[r]];
                    for (int k = sl.b0; k < sl.b1; k++)
                        if (!ind_idx || blocks[(size_t)k]) items.push_back(ChainItem{run.chr, run.a, run.b + b_add, k * WAVE});
                }
                g.n_items.push_back(items.size() - g.item0.back());
                any_items = any_items || g.n_items.back();
            }
        }
        if (!any_items) slabs.clear();      // (no stretch holds a window of any size: nothing to build or chain)
        // ---- per size: the thinned matrix, its table, MISSING everywhere
        std::vector<ChrDev> chrs((size_t)n_sizes * p->nchr);
        std::vector<Layout> layouts((size_t)n_sizes);
        for (const Group &g : G)
            for (int i : g.sizes) {
                Layout &L = layouts[(size_t)i] = make_layout(p, 32, p->nind, steps[i]);
                for (int c = 0; c < p->nchr; c++) {
                    if (3 * L.pitch[c] * 8 + 512 >= (int64_t)1 << 32)
                        return done(fail(GARLIC_ERR_INVALID, "chromosome %d too long for 32-bit row offsets", c));
                    const int32_t cols = (int32_t)(((int64_t)p->chr_nloci[c] + steps[i] - 1) / steps[i]);
                    chrs[(size_t)i * p->nchr + c] = ChrDev{p->chr_off[c], L.base[c], L.pitch[c], cols, 0};
                }
                garlic_panel::FeedSlot &sl = *p->feed_slots[(size_t)i];
                if ((rc = sl.out.reserve((size_t)std::max<int64_t>(L.total, 1)))) return done(rc);
                if ((rc = sl.row_counts.reserve((size_t)p->nchr * nrows))) return done(rc);
            }
        const size_t n_launch = G.size() * std::max<size_t>(slabs.size(), 1);
        if ((rc = p->d_multi_items.put(items, s)) || (rc = p->d_multi_chrs.put(chrs, s)) || (rc = p->d_multi_queues.reserve(2 * n_launch)))
            return done(rc);
        FEED_TRY(hipMemsetAsync(p->d_multi_queues.p, 0, 2 * n_launch * sizeof(int32_t), s));
        for (const Group &g : G)
            for (int i : g.sizes)
                hipLaunchKernelGGL(fill_value_kernel, dim3(1024), dim3(256), 0, s, p->feed_slots[(size_t)i]->out.p, layouts[(size_t)i].total,
                                   MISSING_D);
        FEED_TRY(hipGetLastError());
        // ---- the chains: every group over the whole matrix, or over every slab before that slab's buffer is rebuilt
        const int64_t rows = GOFF + p->nloci + GPAD_BACK;
        FEED_TRY(hipEventRecord(p->feed_slots[0]->ev0, s));
        auto chains = [&](size_t k, const double *terms) -> int {
            for (size_t gi = 0; gi < G.size(); gi++) {
                const Group &g = G[gi];
                const size_t n = g.n_items[k];
                if (!n) continue;
                const int32_t blk0 = slab_blocks ? slabs[k].b0 : 0;
                int32_t *queue = p->d_multi_queues.p + 2 * (k * G.size() + gi);
                const int workers = tgls_workers(ctx, n);
                if (g.sizes.size() == 1) {
                    const int i = g.sizes[0];
                    TglsFeedArgs t{terms, rows, p->d_multi_items.p + g.item0[k], p->d_multi_chrs.p + (size_t)i * p->nchr,
                                   p->feed_slots[(size_t)i]->out.p, 0, p->nind, winsizes[i], (int32_t)n, steps[i], blk0, queue};
                    hipLaunchKernelGGL(tgls_feed_kernel, dim3((unsigned)workers), dim3(TGF_THREADS), 0, s, t);
                } else {
                    // (the group's tables are consecutive only when its sizes are: a table of its own, in the group's order)
                    TglsFeedMultiArgs t{};
                    t.terms = terms; t.term_rows = rows; t.items = p->d_multi_items.p + g.item0[k];
                    t.chrs = p->d_multi_gchrs.p + gi * (size_t)TGM_MAX_SIZES * p->nchr;
                    for (size_t j = 0; j < g.sizes.size(); j++) {
                        const int i = g.sizes[j];
                        t.out[j] = p->feed_slots[(size_t)i]->out.p;
                        t.winsize[j] = winsizes[i];
                        t.thin_step[j] = steps[i];
                    }
                    t.n_sizes = (int32_t)g.sizes.size(); t.nchr = p->nchr; t.ind_begin = 0; t.ind_count = p->nind;
                    t.n_items = (int32_t)n; t.blk0 = blk0; t.next_item = queue;
                    hipLaunchKernelGGL(tgls_feed_multi_kernel, dim3((unsigned)workers), dim3(TGF_THREADS), 0, s, t);
                }
                p->multi_chain_launches++;
            }
            return GARLIC_OK;
        };
        // the shared groups' tables, in group order
        {
            std::vector<ChrDev> gchrs(G.size() * (size_t)TGM_MAX_SIZES * p->nchr);
            for (size_t gi = 0; gi < G.size(); gi++)
                for (size_t j = 0; j < G[gi].sizes.size(); j++)
                    for (int c = 0; c < p->nchr; c++)
                        gchrs[(gi * TGM_MAX_SIZES + j) * p->nchr + c] = chrs[(size_t)G[gi].sizes[j] * p->nchr + c];
            if ((rc = p->d_multi_gchrs.put(gchrs, s))) return done(rc);
            FEED_TRY(hipStreamSynchronize(s));      // (the host lists go out of use here)
        }
        if (slab_blocks) {
            if ((rc = for_each_tgls_slab(p, slabs, slab_blocks, chains))) return done(rc);
            p->multi_term_builds = (int32_t)slabs.size();
        } else {
            p->last_slab_blocks = p->last_n_slabs = 0;
            if (!slabs.empty() && (rc = chains(0, p->d_glterms.p))) return done(rc);
        }
        FEED_TRY(hipGetLastError());
        FEED_TRY(hipEventRecord(p->feed_slots[0]->ev1, s));
        // ---- per size, on its own stream: the samples of every (chromosome, listed individual) counted
        std::vector<std::vector<int64_t>> row_counts((size_t)n_sizes);
        std::vector<int64_t> sort_n((size_t)n_sizes, 0);     // sizes whose feed is being sorted: its length
        const int n_flat = p->nchr * nrows;
        for (const Group &g : G)
            for (int i : g.sizes) {
                garlic_panel::FeedSlot &sl = *p->feed_slots[(size_t)i];
                FEED_TRY(hipStreamWaitEvent(sl.stream, p->feed_slots[0]->ev1, 0));
                hipLaunchKernelGGL(feed_count_kernel, dim3((unsigned)n_flat), dim3(WAVE), 0, sl.stream, sl.out.p,
                                   p->d_multi_chrs.p + (size_t)i * p->nchr, p->nchr, nrows, ind_idx ? d_list.p : nullptr, 1, sl.row_counts.p);
                row_counts[(size_t)i].resize((size_t)n_flat);
                FEED_TRY(hipMemcpyAsync(row_counts[(size_t)i].data(), sl.row_counts.p, sizeof(int64_t) * n_flat, hipMemcpyDeviceToHost, sl.stream));
            }
        // ---- the feeds, in order: offsets (a tiny scan on the host), the compaction, the copy out -- every size's
        //      chain and count kernels were enqueued above, before the first feed is fetched
        for (const Group &g : G)
            for (int i : g.sizes) {
                garlic_panel::FeedSlot &sl = *p->feed_slots[(size_t)i];
                std::vector<int64_t> &rcnt = row_counts[(size_t)i];
                FEED_TRY(hipStreamSynchronize(sl.stream));
                int64_t total = 0;
                if (chr_counts)
                    for (int c = 0; c < p->nchr; c++) {
                        int64_t &cc = chr_counts[(size_t)i * p->nchr + c] = 0;
                        for (int r = 0; r < nrows; r++) cc += rcnt[(size_t)c * nrows + r];
                    }
                for (auto &c : rcnt) { const int64_t n = c; c = total; total += n; }
                counts[i] = total;
                if (total > feed_capacity[i] || total == 0) continue;
                if (!feeds[i] && !p->feed_sink) return done(fail(GARLIC_ERR_INVALID, "feed %d is NULL", i));
                if ((rc = sl.feed.reserve((size_t)total))) return done(rc);
                FEED_TRY(hipMemcpyAsync(sl.row_counts.p, rcnt.data(), sizeof(int64_t) * n_flat, hipMemcpyHostToDevice, sl.stream));
                hipLaunchKernelGGL(feed_write_kernel, dim3((unsigned)n_flat), dim3(WAVE), 0, sl.stream, sl.out.p,
                                   p->d_multi_chrs.p + (size_t)i * p->nchr, p->nchr, nrows, ind_idx ? d_list.p : nullptr, 1, sl.row_counts.p,
                                   sl.feed.p);
                if ((p->feed_order == GARLIC_FEED_ORDER_SORTED || p->feed_sink) && total > 1) {      // fetched below, once every size's sort is enqueued
                    if ((rc = sort_feed(ctx, sl.stream, sl.feed.p, total, sl.fs, false))) return done(rc);
                    sort_n[(size_t)i] = total;
                    continue;
                }
                if (p->feed_sink) {                    // garlic_lod_kde_multi: (one value) stays in the slot's buffer
                    p->feed_sink->size[(size_t)i] = garlic_panel::FeedSink::Entry{sl.feed.p, total};
                    continue;
                }
                FEED_TRY(hipMemcpyAsync(feeds[i], sl.feed.p, sizeof(double) * (size_t)total, hipMemcpyDeviceToHost, sl.stream));
            }
        for (const Group &g : G)
            for (int i : g.sizes) {
                if (!sort_n[(size_t)i]) continue;
                garlic_panel::FeedSlot &sl = *p->feed_slots[(size_t)i];
                const double *from = sl.feed.p;
                if ((rc = sort_result(ctx, sl.stream, sl.feed.p, sl.fs, &from))) return done(rc);
                if (p->feed_sink) {                    // garlic_lod_kde_multi: stays in the slot's buffers
                    p->feed_sink->size[(size_t)i] = garlic_panel::FeedSink::Entry{from, sort_n[(size_t)i]};
                    continue;
                }
                FEED_TRY(hipMemcpyAsync(feeds[i], from, sizeof(double) * (size_t)sort_n[(size_t)i], hipMemcpyDeviceToHost, sl.stream));
            }
        for (const Group &g : G)
            for (int i : g.sizes) FEED_TRY(hipStreamSynchronize(p->feed_slots[(size_t)i]->stream));
        FEED_TRY(hipGetLastError());
        float ms = 0.f;
        p->stats = garlic_call_stats{};
        if (hipEventElapsedTime(&ms, p->feed_slots[0]->ev0, p->feed_slots[0]->ev1) == hipSuccess) p->stats.chain_kernel_ms = ms;
        p->stats_pending = false;
        p->last_feed_form = p->multi_forms[(size_t)G.back().sizes.back()];      // garlic_lod_feed_info: the last size processed
        p->last_feed_doubles = layouts[(size_t)G.back().sizes.back()].total;
    }
#undef FEED_TRY
    d_list.release();
    // ---- every other size on its own: full scores (or whatever form feed_single finds), after the groups
    {
        std::vector<int32_t> order((size_t)n_sizes);
        for (int i = 0; i < n_sizes; i++) order[(size_t)i] = i;
        std::stable_sort(order.begin(), order.end(), [&](int x, int y) { return group[(size_t)x] < group[(size_t)y]; });
        for (int i : order) {
            if (ring_ok[(size_t)i]) continue;
            if (p->feed_sink) p->feed_sink->at = i;
            if ((rc = feed_single(p, winsizes[i], 0.0, max_gap, 1, 0, 0, 0.0, steps[i], ind_idx, n_idx, feeds[i], feed_capacity[i],
                                  &counts[i], chr_counts ? chr_counts + (size_t)i * p->nchr : nullptr)))
                return rc;
            p->multi_forms[(size_t)i] = p->last_feed_form;
            p->multi_chain_launches++;
            p->multi_term_builds += p->last_n_slabs;
        }
    }
    return GARLIC_OK;
}

int garlic_lod_feed_multi_info(garlic_panel *p, int32_t n, int32_t *forms, int32_t *groups, int32_t *n_chain_launches,
                               int32_t *n_term_builds)
{
    if (!p) return fail(GARLIC_ERR_INVALID, "panel is required");
    if (n < 0 || (size_t)n > p->multi_forms.size())
        return fail(GARLIC_ERR_INVALID, "the last garlic_lod_feed_multi_tgls call had %d sizes (asked for %d)", (int)p->multi_forms.size(), n);
    for (int i = 0; i < n; i++) {
        if (forms) forms[i] = p->multi_forms[(size_t)i];
        if (groups) groups[i] = p->multi_groups[(size_t)i];
    }
    if (n_chain_launches) *n_chain_launches = p->multi_chain_launches;
    if (n_term_builds) *n_term_builds = p->multi_term_builds;
    return GARLIC_OK;
}

// Coverage counts of the unweighted --error scores without the scores: chain + compare + sliding count in one kernel
// (coverage_kernel.hpp).  Where that kernel does not apply -- a cutoff at or below MISSING, terms that are not all
// finite, a window sum that can be -9999.0, W > COVF_MAX_W -- the scores are computed into the panel's scratch and
// counted by garlic_roh_coverage.

// The window bits, one per window and individual: [chromosome][individual][word] on the device, with the two tables the
// kernels that write and read them take (bchrs: out_base / out_pitch in dwords; word_base: words before each chromosome).
struct BitMatrix {
    std::vector<ChrDev> bchrs;
    std::vector<int32_t> word_base;
    int64_t total = 0;             // dwords
    PoolBuf<uint32_t> d_bits;
    DevBuf<ChrDev> d_bchrs;
    DevBuf<int32_t> d_wbase;
    // row_align: rows padded to a multiple of that many dwords (8 for lod_bits_kernel, which stores eight tiles' dwords as
    // one aligned 32-byte piece; 1 for everything else).  Then room for the bits and the tables on their way.
    int make(garlic_panel *p, int row_align)
    {
        bchrs.assign((size_t)p->nchr, ChrDev{});
        word_base.assign((size_t)p->nchr + 1, 0);
        for (int c = 0; c < p->nchr; c++) {
            const int64_t words = (p->chr_nloci[c] + 31) / 32;
            const int64_t row_words = (words + row_align - 1) / row_align * row_align;
            bchrs[(size_t)c] = ChrDev{p->chr_off[c], total, row_words, p->chr_nloci[c], 0};
            total += row_words * p->nind;
            word_base[(size_t)c + 1] = word_base[(size_t)c] + (int32_t)words;
            if (row_words * 4 * (int64_t)p->nind >= (int64_t)1 << 32) return fail(GARLIC_ERR_INVALID, "chromosome %d: bit rows beyond 32-bit offsets", c);
        }
        int rc;
        if ((rc = d_bits.reserve(p->ctx, zeroed_words())) || (rc = d_bchrs.put(bchrs, p->ctx->stream))) return rc;
        return d_wbase.put(word_base, p->ctx->stream);
    }
    // (never fewer than four dwords.  Zeroing is for kernels that set bits: one that writes every word needs none, a memset is traffic.)
    size_t zeroed_words() const { return (size_t)std::max<int64_t>(total, 4); }
    hipError_t zero(hipStream_t s) { return hipMemsetAsync(d_bits.p, 0, sizeof(uint32_t) * zeroed_words(), s); }
};

// The arguments of garlic_roh_coverage_fused / garlic_roh_segments: what becomes of the window bits, counts or segments
struct CovSink {
    int32_t W, max_gap, use_gl, weighted, M;
    double error, mu, cutoff;
    int16_t *inwin = nullptr;            // counts
    int32_t inwin_pitch_align = 8, where = GARLIC_DEVICE;
    bool segments = false;               // segments
    double overlap_frac = 0.0;
    garlic_roh_segment *segs = nullptr;
    int64_t cap = 0, *n_out = nullptr;
};

// a layout as the kernels take it
static std::vector<ChrDev> chr_table(const garlic_panel *p, const Layout &L)
{
    std::vector<ChrDev> chrs((size_t)p->nchr);
    for (int c = 0; c < p->nchr; c++) chrs[(size_t)c] = ChrDev{p->chr_off[c], L.base[c], L.pitch[c], p->chr_nloci[c], 0};
    return chrs;
}

// eight counts per store: every row of the count matrix 16-B aligned
static bool cov_vec_ok(const garlic_panel *p, const Layout &Lo, const int16_t *dst)
{
    bool vec_ok = (reinterpret_cast<uintptr_t>(dst) & 15) == 0;
    for (int c = 0; c < p->nchr; c++) vec_ok = vec_ok && Lo.base[c] % 8 == 0 && Lo.pitch[c] % 8 == 0;
    return vec_ok;
}

// where the counts are written: the caller's device matrix, or scratch that finish_counts copies to the caller's host matrix
static int counts_target(int16_t *inwin, int32_t where, const Layout &Lo, DevBuf<int16_t> &d_cov, int16_t **dst)
{
    *dst = inwin;
    if (where != GARLIC_HOST) return GARLIC_OK;
    const int rc = d_cov.reserve((size_t)Lo.total);
    *dst = d_cov.p;
    return rc;
}

// the sliding counts from the window bits (d_ochrs: the count matrix's table on the device)
static void launch_counts_from_bits(garlic_panel *p, const BitMatrix &bm, const CovSink &c, const Layout &Lo, const ChrDev *d_ochrs, int16_t *dst)
{
    hipLaunchKernelGGL(cov_counts_from_bits_kernel, dim3((unsigned)((bm.word_base[(size_t)p->nchr] + 255) / 256),
                                                         (unsigned)((p->nind + COV_ITEM_ROWS - 1) / COV_ITEM_ROWS)),
                       dim3(256), 0, p->ctx->stream, bm.d_bits.p, bm.d_bchrs.p, d_ochrs, bm.d_wbase.p, p->nchr, c.W, p->nind,
                       cov_vec_ok(p, Lo, dst) ? 1 : 0, dst);
}

// the counts to the caller and the end of the call (d_timed_out: the flag of count items that rode in the chain kernel's queue)
static int finish_counts(garlic_panel *p, int16_t *inwin, int32_t where, const Layout &Lo, const int16_t *dst, const int32_t *d_timed_out)
{
    hipStream_t s = p->ctx->stream;
    hipError_t e = hipGetLastError();
    if (e == hipSuccess && where == GARLIC_HOST)
        e = hipMemcpyAsync(inwin, dst, sizeof(int16_t) * (size_t)Lo.total, hipMemcpyDeviceToHost, s);
    int32_t timed_out = 0;
    if (e == hipSuccess && d_timed_out) e = hipMemcpyAsync(&timed_out, d_timed_out, sizeof(int32_t), hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) return fail(GARLIC_ERR_HIP, "coverage: %s", hipGetErrorString(e));
    if (!timed_out) return GARLIC_OK;
    p->n_count_timeouts++;
    return fail(GARLIC_ERR_HIP, "coverage: a count item gave up waiting for its chromosome's chains");
}

// ROH segments from the window bits (roh_segments_kernel.hpp): r bits, break bits, the list; sorted on the host into
// the reference's order.
static int segments_from_bits(garlic_panel *p, const BitMatrix &bm, const CovSink &sink)
{
    const int32_t W = sink.W;
    garlic_ctx *ctx = p->ctx;
    hipStream_t s = ctx->stream;
    double T = sink.overlap_frac * W;              // src/garlic-roh.cpp:421-423
    T = (T >= 1) ? T : 1;
    T = (T <= W) ? T : W;
    const int thr = (int)std::ceil(T);             // counts are integers: cnt >= T  <=>  cnt >= ceil(T)
    const size_t nchr = (size_t)p->nchr;
    const int64_t total_words = bm.word_base[nchr];
    int64_t bit_words = 0;
    for (size_t c = 0; c < nchr; c++) bit_words = std::max<int64_t>(bit_words, bm.bchrs[c].out_base + bm.bchrs[c].out_pitch * p->nind);
    PoolBuf<uint32_t> d_mask;
    PoolBuf<garlic_roh_segment> d_segs;
    DevBuf<uint32_t> d_brk;
    DevBuf<unsigned long long> d_count;
    DevBuf<int32_t> d_w0, d_wedge_chr;             // chromosomes whose first SNP is at position 0 (roh_segments_kernel.hpp)
    std::vector<int32_t> wedge_chr;
    for (int c = 0; c < p->nchr; c++)
        if (p->chr_nloci[c] > 0 && p->pos[(size_t)p->chr_off[c]] == 0) wedge_chr.push_back(c);
    int rc;
    const int64_t cap = std::max<int64_t>(sink.cap, 0);
    if ((rc = d_mask.reserve(ctx, (size_t)std::max<int64_t>(bit_words, 1))) || (rc = d_brk.reserve((size_t)std::max<int64_t>(total_words, 1))) ||
        (rc = d_segs.reserve(ctx, (size_t)std::max<int64_t>(cap, 1))) || (rc = d_count.reserve(1)))
        return rc;
    hipError_t e = hipMemsetAsync(d_brk.p, 0, sizeof(uint32_t) * (size_t)std::max<int64_t>(total_words, 1), s);
    if (e == hipSuccess) e = hipMemsetAsync(d_count.p, 0, sizeof(unsigned long long), s);
    if (e != hipSuccess) return fail(GARLIC_ERR_HIP, "roh segments: %s", hipGetErrorString(e));
    unsigned long long found = 0;
    if (total_words > 0) {
        const int nb = (int)p->boundaries.size();
        if (nb > 0)
            hipLaunchKernelGGL(roh_break_bits_kernel, dim3((unsigned)((nb + 255) / 256)), dim3(256), 0, s, p->d_boundaries.p, nb,
                               p->d_chr_off.p, bm.d_wbase.p, p->nchr, d_brk.p);
        const dim3 grid((unsigned)((total_words + 255) / 256), (unsigned)((p->nind + ROH_ROWS - 1) / ROH_ROWS));
        hipLaunchKernelGGL(roh_mask_from_bits_kernel, grid, dim3(256), 0, s, bm.d_bits.p, bm.d_bchrs.p, bm.d_wbase.p, p->nchr, p->nind, W, thr, d_mask.p);
        const int32_t *a_w0 = nullptr;
        if (!wedge_chr.empty()) {
            const size_t n_w0 = nchr * (size_t)p->nind;
            if ((rc = d_w0.reserve(n_w0)) || (rc = d_wedge_chr.reserve(wedge_chr.size()))) return rc;
            e = hipMemsetAsync(d_w0.p, 0xff, sizeof(int32_t) * n_w0, s);            // -1: an ordinary row
            if (e == hipSuccess)
                e = hipMemcpyAsync(d_wedge_chr.p, wedge_chr.data(), sizeof(int32_t) * wedge_chr.size(), hipMemcpyHostToDevice, s);
            if (e != hipSuccess) return fail(GARLIC_ERR_HIP, "roh segments: %s", hipGetErrorString(e));
            const int n_threads = (int)wedge_chr.size() * p->nind;
            hipLaunchKernelGGL(roh_wedge_kernel, dim3((unsigned)((n_threads + 63) / 64)), dim3(64), 0, s, d_mask.p, bm.d_bchrs.p, d_brk.p, bm.d_wbase.p,
                               d_wedge_chr.p, (int)wedge_chr.size(), p->nind, T, d_w0.p, d_segs.p, (long long)cap, d_count.p);
            a_w0 = d_w0.p;
        }
        hipLaunchKernelGGL(roh_segments_from_mask_kernel, grid, dim3(256), 0, s, d_mask.p, bm.d_bchrs.p, d_brk.p, bm.d_wbase.p, p->nchr, p->nind, T,
                           d_segs.p, (long long)cap, d_count.p, a_w0);
        e = hipGetLastError();
        if (e == hipSuccess) e = hipMemcpyAsync(&found, d_count.p, sizeof found, hipMemcpyDeviceToHost, s);
        if (e == hipSuccess) e = hipStreamSynchronize(s);
        if (e != hipSuccess) return fail(GARLIC_ERR_HIP, "roh segments: %s", hipGetErrorString(e));
    }
    if (sink.n_out) *sink.n_out = (int64_t)found;
    if ((int64_t)found <= cap && found > 0) {
        e = hipMemcpyAsync(sink.segs, d_segs.p, sizeof(garlic_roh_segment) * found, hipMemcpyDeviceToHost, s);
        if (e == hipSuccess) e = hipStreamSynchronize(s);
        if (e != hipSuccess) return fail(GARLIC_ERR_HIP, "roh segments: %s", hipGetErrorString(e));
        std::sort(sink.segs, sink.segs + found, [](const garlic_roh_segment &x, const garlic_roh_segment &y) {
            return x.ind != y.ind ? x.ind < y.ind : x.chr != y.chr ? x.chr < y.chr : x.start < y.start;
        });
    }
    return GARLIC_OK;
}

// scores into the panel's scratch, then garlic_roh_coverage; for segments the scores' bits, then as from the chains' bits
static int coverage_unfused(garlic_panel *p, const CovSink &c)
{
    hipStream_t s = p->ctx->stream;
    const Layout L = make_layout(p, 32, p->nind);
    int rc;
    if ((rc = p->d_out.reserve(p->ctx, (size_t)L.total))) return rc;
    if (c.weighted) rc = garlic_wlod_windows(p, c.W, c.error, c.max_gap, c.use_gl, c.M, c.mu, 0, p->nind, 32, p->d_out.p, GARLIC_DEVICE);
    else rc = garlic_lod_windows(p, c.W, c.error, c.max_gap, c.use_gl, 0, p->nind, 32, p->d_out.p, GARLIC_DEVICE);
    if (rc) return rc;
    if (!c.segments) return garlic_roh_coverage(p, p->d_out.p, 32, p->nind, c.W, c.cutoff, c.inwin, c.inwin_pitch_align, c.where);
    // (score >= cutoff, MISSING compared like any score; the kernel writes every word of the matrix)
    const std::vector<ChrDev> schrs = chr_table(p, L);
    BitMatrix bm;
    DevBuf<ChrDev> d_schrs;
    if ((rc = bm.make(p, 1)) || (rc = d_schrs.put(schrs, s))) return rc;
    if (bm.word_base[(size_t)p->nchr] > 0)
        hipLaunchKernelGGL(roh_bits_from_scores_kernel, dim3((unsigned)((bm.word_base[(size_t)p->nchr] + 255) / 256), (unsigned)p->nind),
                           dim3(256), 0, s, p->d_out.p, d_schrs.p, bm.d_bchrs.p, bm.d_wbase.p, p->nchr, c.W, c.cutoff, bm.d_bits.p);
    const hipError_t e = hipStreamSynchronize(s);      // (the host vectors above)
    if (e != hipSuccess) return fail(GARLIC_ERR_HIP, "roh segments: %s", hipGetErrorString(e));
    return segments_from_bits(p, bm, c);
}

// --weighted (with or without likelihoods), or unweighted scores with likelihoods: the tuned wLOD kernels leave 16 bits per
// individual and group instead of 16 scores (wlod_write_group), the TGLS ring chain a dword of bits per lane and tile; the
// counts come from the bits as for the unweighted scores
static int coverage_from_score_kernels(garlic_panel *p, const CovSink &c)
{
    hipStream_t s = p->ctx->stream;
    const Layout Lo = make_layout(p, c.inwin_pitch_align, p->nind);
    const std::vector<ChrDev> ochrs = chr_table(p, Lo);
    BitMatrix bm;
    DevBuf<ChrDev> d_ochrs;
    DevBuf<int16_t> d_cov;
    int16_t *dst;
    int rc;
    if ((rc = bm.make(p, 1)) || (rc = d_ochrs.put(ochrs, s)) || (rc = counts_target(c.inwin, c.where, Lo, d_cov, &dst))) return rc;
    hipError_t e = bm.zero(s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);      // (the host vectors above)
    if (e != hipSuccess) return fail(GARLIC_ERR_HIP, "coverage: %s", hipGetErrorString(e));
    p->cov_pending = CovBits{bm.d_bits.p, bm.d_bchrs.p, c.cutoff};
    p->cov_written = false;
    double *bits_as_out = reinterpret_cast<double *>(bm.d_bits.p);
    if (c.weighted) rc = garlic_wlod_windows(p, c.W, c.error, c.max_gap, c.use_gl, c.M, c.mu, 0, p->nind, 32, bits_as_out, GARLIC_DEVICE);
    else rc = garlic_lod_windows(p, c.W, c.error, c.max_gap, 1, 0, p->nind, 32, bits_as_out, GARLIC_DEVICE);
    const bool written = c.weighted || p->cov_written;
    p->cov_pending = CovBits{nullptr, nullptr, 0.0};
    if (rc == GARLIC_INTERNAL_NO_BITS) return coverage_unfused(p, c);
    if (rc) return rc;
    if (!written) return coverage_unfused(p, c);       // (no scored window at all: nothing was launched)
    if (c.segments) return segments_from_bits(p, bm, c);
    launch_counts_from_bits(p, bm, c, Lo, d_ochrs.p, dst);
    return finish_counts(p, c.inwin, c.where, Lo, dst, nullptr);
}

// unweighted --error scores.  Two kernels: one bit per window and individual from the hand-scheduled chain
// (lod_bits_kernel), then the sliding counts from the bits (cov_counts_from_bits_kernel): a 64th of the score bytes in between
static int coverage_lod_bits(garlic_panel *p, const CovSink &c)
{
    garlic_ctx *ctx = p->ctx;
    hipStream_t s = ctx->stream;
    const int32_t W = c.W;
    const size_t nchr = (size_t)p->nchr;
    std::vector<Run> runs;
    std::vector<FillItem> fill;
    int64_t n_valid = 0;
    plan_runs(p, W, runs, fill, n_valid);              // in chromosome and position order
    std::vector<int32_t> col0(runs.size(), 0);
    std::vector<FeedItem> items;
    build_feed_items(runs, longest_first(runs), nullptr, (p->nind + WAVE - 1) / WAVE, col0, items);
    const Layout Lo = make_layout(p, c.inwin_pitch_align, p->nind);
    const std::vector<ChrDev> chrs = chr_table(p, Lo);
    BitMatrix bm;
    DevBuf<FeedItem> d_items;
    DevBuf<ChrDev> d_chrs;
    DevBuf<int32_t> d_counter, d_cnt;      // d_cnt: chr_done[nchr] | timeout | chr_need[nchr] | cnt_order[nchr] | cnt_base[nchr + 1]
    DevBuf<int16_t> d_cov;
    int16_t *dst;
    int rc;
    if ((rc = d_items.put(items, s)) || (rc = d_chrs.put(chrs, s)) || (rc = d_counter.reserve(4)) || (rc = counts_target(c.inwin, c.where, Lo, d_cov, &dst)))
        return rc;
    hipError_t e = hipMemsetAsync(d_counter.p, 0, 4 * sizeof(int32_t), s);
    if (e != hipSuccess) return fail(GARLIC_ERR_HIP, "coverage: %s", hipGetErrorString(e));
    const bool vec_ok = cov_vec_ok(p, Lo, dst);
    if ((rc = bm.make(p, 8))) return rc;
    (void)hist_mark(ctx, false);
    if ((e = bm.zero(s)) != hipSuccess) return fail(GARLIC_ERR_HIP, "coverage: %s", hipGetErrorString(e));
    // GARLIC_COVERAGE_OVERLAP=1: the counts ride in the chain kernel's queue (FeedArgs::cnt_order) instead of a launch of
    // their own behind it -- the longest runs' chains are that kernel's critical path and leave most of the chip idle,
    // the counts of every finished chromosome could fill it.  Built and measured ("Coverage
    // counts without the scores"): the chains are latency-bound and the counts' traffic slows the longest one from
    // 22.8 to 36.5 ns per window, 19.5 ms against 17.6 ms for the two launches at 10M x 1250.  Off by default.
    const bool overlap = !items.empty() && !c.segments && getenv("GARLIC_COVERAGE_OVERLAP");
    int64_t n_cnt_items = 0;
    if (overlap) {
        std::vector<int32_t> h(4 * nchr + 2, 0);
        int32_t *need = h.data() + nchr + 1, *corder = need + nchr, *cbase = corder + nchr;
        std::vector<int32_t> longest(nchr, 0);
        for (const FeedItem &it : items) need[it.chr]++;
        for (const Run &r : runs) longest[(size_t)r.chr] = std::max(longest[(size_t)r.chr], r.b - r.a + 1);
        for (size_t k = 0; k < nchr; k++) corder[k] = (int32_t)k;
        std::stable_sort(corder, corder + nchr, [&](int32_t x, int32_t y) { return longest[(size_t)x] < longest[(size_t)y]; });
        const int64_t nrg = (p->nind + COV_ITEM_ROWS - 1) / COV_ITEM_ROWS;
        for (size_t k = 0; k < nchr; k++) {
            cbase[k] = (int32_t)n_cnt_items;
            const int64_t words = (p->chr_nloci[corder[k]] + 31) / 32;
            n_cnt_items += (words + COV_ITEM_WORDS - 1) / COV_ITEM_WORDS * nrg;
        }
        cbase[nchr] = (int32_t)n_cnt_items;
        if (n_cnt_items + (int64_t)items.size() >= ((int64_t)1 << 31)) return fail(GARLIC_ERR_INVALID, "coverage: more than 2^31 work items");
        if ((rc = d_cnt.put(h, s))) return rc;
        if ((e = hipStreamSynchronize(s)) != hipSuccess) return fail(GARLIC_ERR_HIP, "coverage: %s", hipGetErrorString(e));      // (h leaves scope)
    }
    if (!items.empty()) {
        FeedArgs f{p->d_packed.p, p->d_tab.p, d_items.p, bm.d_bchrs.p, reinterpret_cast<double *>(bm.d_bits.p), nullptr, p->nwordrows, 0,
                   p->nind, W, (int32_t)items.size(), 1, getenv("GARLIC_FEED_NO_ASM") ? 0 : 1, d_counter.p, nullptr, c.cutoff};
        if (overlap) {
            f.chr_done = d_cnt.p;
            f.cnt_timeout = d_cnt.p + nchr;
            f.chr_need = d_cnt.p + nchr + 1;
            f.cnt_order = d_cnt.p + 2 * nchr + 1;
            f.cnt_base = d_cnt.p + 3 * nchr + 1;
            f.cnt_chrs = d_chrs.p;
            f.cnt_out = dst;
            f.n_cnt_items = (int32_t)n_cnt_items;
            f.n_cnt_chr = p->nchr;
            f.cnt_vec_ok = vec_ok ? 1 : 0;
        }
        ItemTrace trace;
        f.trace = trace.begin(8, items.size(), "\n", s);
        // workgroups per CU as the chains want them (feed_grid: the same chains, the same paces); the count items behind
        // them in the queue are short and fill whatever is idle.  (Persistent workgroups, all resident: a count item
        // that waits must not keep a chain item from starting.)
        int per_cu = 1, chain_grid = 1;
        if ((rc = feed_grid(ctx, items, &chain_grid, &per_cu))) return rc;
        const int grid = (int)std::min<size_t>(items.size() + (size_t)n_cnt_items, (size_t)ctx->n_cu * per_cu);
        void *kargs[] = {(void *)&f};
        e = hipLaunchKernel((const void *)lod_bits_kernel, dim3((unsigned)grid), dim3(FEED_G * WAVE), kargs, 0, s);
        if (e != hipSuccess) return fail(GARLIC_ERR_HIP, "coverage: %s", hipGetErrorString(e));
        trace.write(s);
    }
    if (!c.segments && !overlap) launch_counts_from_bits(p, bm, c, Lo, d_chrs.p, dst);
    (void)hist_mark(ctx, true);
    if (c.segments) return segments_from_bits(p, bm, c);
    return finish_counts(p, c.inwin, c.where, Lo, dst, overlap ? d_cnt.p + nchr : nullptr);
}

static int coverage_impl(garlic_panel *p, const CovSink &c)
{
    const int32_t W = c.W, weighted = c.weighted, use_gl = c.use_gl;
    int rc;
    if ((rc = set_device(p->ctx))) return rc;
    if (!p->have_map || !p->have_freq || !p->have_geno)
        return fail(GARLIC_ERR_STATE, "panel needs map, freq and genotypes before computing LOD");
    if ((rc = ensure_segments(p, c.max_gap))) return rc;
    if ((rc = ensure_term_table(p, c.error))) return rc;
    if ((weighted || use_gl) && c.cutoff > MISSING_D && !getenv("GARLIC_COVERAGE_UNFUSED")) return coverage_from_score_kernels(p, c);
    const bool fused = !weighted && !use_gl && W <= COVF_MAX_W && c.cutoff > MISSING_D && p->tab_all_finite &&
                       !lod_exact_needed(p, MODE_LOD, W) && !getenv("GARLIC_COVERAGE_UNFUSED");
    return fused ? coverage_lod_bits(p, c) : coverage_unfused(p, c);
}

int garlic_roh_coverage_fused(garlic_panel *p, int32_t winsize, double error, int32_t max_gap, int32_t use_gl,
                              int32_t weighted, int32_t M, double mu, double cutoff, int16_t *inwin,
                              int32_t inwin_pitch_align, int32_t where)
{
    if (!p || !inwin) return fail(GARLIC_ERR_INVALID, "panel and inwin are required");
    if (winsize <= 1 || inwin_pitch_align < 1) return fail(GARLIC_ERR_INVALID, "winsize must be > 1, inwin_pitch_align >= 1");
    if (winsize > 32767) return fail(GARLIC_ERR_INVALID, "coverage counts are 16-bit: winsize <= 32767");
    if (p->nind > 65535) return fail(GARLIC_ERR_INVALID, "coverage: at most 65535 individuals per call");
    const CovSink sink{winsize, max_gap, use_gl, weighted, M, error, mu, cutoff, inwin, inwin_pitch_align, where};
    return coverage_impl(p, sink);
}

int garlic_roh_segments(garlic_panel *p, int32_t winsize, double error, int32_t max_gap, int32_t use_gl, int32_t weighted,
                        int32_t M, double mu, double cutoff, double overlap_frac, garlic_roh_segment *segments,
                        int64_t capacity, int64_t *n_segments)
{
    if (!p || !n_segments) return fail(GARLIC_ERR_INVALID, "panel and n_segments are required");
    if (capacity < 0 || (capacity > 0 && !segments)) return fail(GARLIC_ERR_INVALID, "segments: capacity without a buffer");
    if (winsize <= 1) return fail(GARLIC_ERR_INVALID, "winsize must be > 1");
    if (winsize > 32767) return fail(GARLIC_ERR_INVALID, "coverage counts are 16-bit: winsize <= 32767");
    if (p->nind > 65535) return fail(GARLIC_ERR_INVALID, "coverage: at most 65535 individuals per call");
    if (!(overlap_frac == overlap_frac)) return fail(GARLIC_ERR_INVALID, "overlap_frac is not a number");
    *n_segments = 0;
    // (the reference tells "a segment is open" by its first position being > 0 and "none" by < 0, src/garlic-roh.cpp:456, 493,
    // 514: a chromosome that starts at 0 takes the device's restatement of what that does; a negative position has no meaning)
    if (p->have_map)
        for (int c = 0; c < p->nchr; c++)
            if (p->chr_nloci[c] > 0 && p->pos[(size_t)p->chr_off[c]] < 0)
                return fail(GARLIC_ERR_INVALID, "chromosome %d starts at position %d: ROH segments need positions >= 0", c,
                            (int)p->pos[(size_t)p->chr_off[c]]);
    CovSink sink{winsize, max_gap, use_gl, weighted, M, error, mu, cutoff};
    sink.segments = true;
    sink.overlap_frac = overlap_frac;
    sink.segs = segments;
    sink.cap = capacity;
    sink.n_out = n_segments;
    return coverage_impl(p, sink);
}

int garlic_panel_tgls_mode(garlic_panel *p, int32_t *mode, int32_t *terms_by)
{
    if (!p || !mode) return fail(GARLIC_ERR_INVALID, "panel and mode are required");
    *mode = !p->have_gl ? 0 : p->gl_cont ? GARLIC_TGLS_CONTINUOUS : p->gl_wide ? GARLIC_TGLS_DICTIONARY16 : GARLIC_TGLS_DICTIONARY;
    // 16-bit codes under term slabs: there is no resident matrix, the answer is who built the slabs of the last call
    if (terms_by) *terms_by = p->glterms_valid ? p->gl_terms_by : (p->gl_wide && p->last_n_slabs > 0) ? p->slab_terms_by : 0;
    return GARLIC_OK;
}

int garlic_panel_set_tgls_term_budget(garlic_panel *p, int64_t bytes)
{
    if (!p) return fail(GARLIC_ERR_INVALID, "panel is NULL");
    if (bytes < -1) return fail(GARLIC_ERR_INVALID, "term budget %lld: 0, -1 or a number of bytes", (long long)bytes);
    if (bytes > 0 && !tgls_slab_blocks_for(p, (size_t)bytes))
        return fail(GARLIC_ERR_INVALID, "term budget of %lld bytes: the buffers of one-block slabs of this panel need %lld",
                    (long long)bytes, (long long)(tgls_block_bytes(p) * (p->nind > WAVE ? 2 : 1)));
    int rc;
    if ((rc = set_device(p->ctx))) return rc;
    HIP_TRY(hipStreamSynchronize(p->ctx->stream));
    p->terms_budget = bytes;
    if (p->gl_cont) return GARLIC_OK;            // (8 bytes per genotype are the panel's data there: no budget)
    // what the new bound does not allow goes now; the next call builds what it needs
    if (bytes == 0 || (bytes > 0 && (p->d_slab[0].cap + p->d_slab[1].cap) * sizeof(double) > (size_t)bytes)) release_tgls_slabs(p);
    if (bytes > 0 && p->d_glterms.cap * sizeof(double) > (size_t)bytes) {
        p->d_glterms.release();
        p->glterms_valid = false;
    }
    return GARLIC_OK;
}

int garlic_panel_tgls_terms_info(garlic_panel *p, int64_t *whole_bytes, int64_t *resident_bytes, int32_t *slab_blocks, int32_t *n_slabs)
{
    if (!p) return fail(GARLIC_ERR_INVALID, "panel is NULL");
    if (whole_bytes) *whole_bytes = (int64_t)(tgls_block_bytes(p) * (size_t)(p->nind_pad / WAVE));
    if (resident_bytes) *resident_bytes = (int64_t)((p->d_glterms.cap + p->d_slab[0].cap + p->d_slab[1].cap) * sizeof(double));
    if (slab_blocks) *slab_blocks = p->last_slab_blocks;
    if (n_slabs) *n_slabs = p->last_n_slabs;
    return GARLIC_OK;
}

int garlic_roh_coverage(garlic_panel *p, const double *scores, int32_t pitch_align, int32_t nind_out,
                        int32_t winsize, double cutoff, int16_t *inwin, int32_t inwin_pitch_align,
                        int32_t where)
{
    if (!p || !scores || !inwin) return fail(GARLIC_ERR_INVALID, "panel, scores and inwin are required");
    if (winsize <= 1 || pitch_align < 1 || inwin_pitch_align < 1 || nind_out < 1)
        return fail(GARLIC_ERR_INVALID, "winsize must be > 1; pitch_align, inwin_pitch_align and nind_out >= 1");
    if (winsize > 32767) return fail(GARLIC_ERR_INVALID, "coverage counts are 16-bit: winsize <= 32767");
    if (nind_out > 65535) return fail(GARLIC_ERR_INVALID, "coverage: at most 65535 individuals per call");
    int rc;
    if ((rc = set_device(p->ctx))) return rc;
    hipStream_t s = p->ctx->stream;
    const Layout L = make_layout(p, pitch_align, nind_out), Lo = make_layout(p, inwin_pitch_align, nind_out);
    std::vector<ChrDev> chrs = chr_table(p, L);
    const std::vector<ChrDev> ochrs = chr_table(p, Lo);
    chrs.insert(chrs.end(), ochrs.begin(), ochrs.end());
    std::vector<int32_t> seg_base(p->nchr + 1, 0);
    for (int c = 0; c < p->nchr; c++) seg_base[c + 1] = seg_base[c] + (p->chr_nloci[c] + COV_SEG - 1) / COV_SEG;
    DevBuf<ChrDev> d_chrs;
    DevBuf<int32_t> d_seg;
    DevBuf<int16_t> d_cov;
    int16_t *dst;
    if ((rc = d_chrs.put(chrs, s)) || (rc = d_seg.put(seg_base, s)) || (rc = counts_target(inwin, where, Lo, d_cov, &dst))) return rc;
    const size_t lds = sizeof(uint16_t) * ((size_t)winsize + COV_SEG + 2);      // (counts <= COV_SEG + W - 1: 16 bits, W < 57000)
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(roh_coverage_kernel),
                            hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return fail(GARLIC_ERR_HIP, "coverage: %s", hipGetErrorString(e));
    hipLaunchKernelGGL(roh_coverage_kernel, dim3((unsigned)seg_base[p->nchr], (unsigned)nind_out),
                       dim3(COV_THREADS), lds, s, scores, d_chrs.p, d_chrs.p + p->nchr, d_seg.p, p->nchr, nind_out,
                       winsize, cutoff, dst, cov_vec_ok(p, Lo, dst) ? 1 : 0);
    return finish_counts(p, inwin, where, Lo, dst, nullptr);
}

int garlic_last_call_stats(garlic_panel *p, garlic_call_stats *stats)
{
    if (!p || !stats) return fail(GARLIC_ERR_INVALID, "panel and stats are required");
    if (p->stats_pending) {   // the event times of the last call (waits for it if it is still running)
        int rc;
        if ((rc = set_device(p->ctx))) return rc;
        // (a one-kernel pass recorded only the pair around its kernel: the call's time is the kernel's)
        HIP_TRY(hipEventSynchronize(p->stats_one_kernel ? p->ctx->hist1[p->stats_slot] : p->ctx->ev_end));
        (void)hipEventElapsedTime(&p->stats.chain_kernel_ms, p->ctx->hist0[p->stats_slot], p->ctx->hist1[p->stats_slot]);
        if (p->stats_one_kernel) p->stats.total_ms = p->stats.chain_kernel_ms;
        else (void)hipEventElapsedTime(&p->stats.total_ms, p->ctx->ev_begin, p->ctx->ev_end);
        p->stats_pending = false;
    }
    // Strip launches the tile form had to repair, counted on the device: read once after a call that launched the strip
    // kernel (that call has been waited for by now), not on every poll -- the copy waits for whatever the stream holds.
    if (p->reruns_stale && p->d_counter.p) {
        int32_t n = 0;
        int rc;
        if ((rc = set_device(p->ctx))) return rc;
        HIP_TRY(hipMemcpyAsync(&n, p->d_counter.p + 4, sizeof(int32_t), hipMemcpyDeviceToHost, p->ctx->stream));
        HIP_TRY(hipStreamSynchronize(p->ctx->stream));
        p->n_stall_reruns = n;
        p->reruns_stale = false;
    }
    p->stats.n_stall_reruns = p->n_stall_reruns;
    p->stats.n_count_timeouts = p->n_count_timeouts;
    *stats = p->stats;
    return GARLIC_OK;
}

int garlic_recent_kernel_ms(garlic_ctx *ctx, float *ms, int32_t n, int32_t *got)
{
    if (!ctx || !ms || !got || n < 1) return fail(GARLIC_ERR_INVALID, "ctx, ms, got are required; n >= 1");
    HIP_TRY(hipSetDevice(ctx->device));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    const int64_t have = std::min<int64_t>(std::min<int64_t>(n, garlic_ctx::HIST), ctx->n_calls);
    for (int64_t k = 0; k < have; k++) {       // oldest of the requested ones first
        const int64_t call = ctx->n_calls - have + k;
        ms[k] = 0.f;
        (void)hipEventElapsedTime(&ms[k], ctx->hist0[call % garlic_ctx::HIST], ctx->hist1[call % garlic_ctx::HIST]);
    }
    *got = (int32_t)have;
    return GARLIC_OK;
}

int garlic_device_alloc(garlic_ctx *ctx, int64_t bytes, void **out)
{
    if (!ctx || !out || bytes < 1) return fail(GARLIC_ERR_INVALID, "context, size and result pointer are required");
    int rc;
    if ((rc = set_device(ctx))) return rc;
    return score_alloc(ctx, (size_t)bytes, out);
}

int garlic_device_free(garlic_ctx *ctx, void *ptr)
{
    if (!ctx) return fail(GARLIC_ERR_INVALID, "context is required");
    if (!ptr) return GARLIC_OK;
    int rc;
    if ((rc = set_device(ctx))) return rc;
    return score_free(ctx, ptr);
}

int garlic_device_upload(garlic_ctx *ctx, void *dst, const void *src, int64_t bytes)
{
    if (!ctx || !dst || !src) return fail(GARLIC_ERR_INVALID, "context, dst and src are required");
    if (bytes < 0) return fail(GARLIC_ERR_INVALID, "bytes %lld is negative", (long long)bytes);
    int rc;
    if ((rc = set_device(ctx))) return rc;
    if (!bytes) return GARLIC_OK;
    HIP_TRY(hipMemcpyAsync(dst, src, (size_t)bytes, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return GARLIC_OK;
}

int garlic_device_download(garlic_ctx *ctx, void *dst, const void *src, int64_t bytes)
{
    if (!ctx || !dst || !src) return fail(GARLIC_ERR_INVALID, "context, dst and src are required");
    if (bytes < 0) return fail(GARLIC_ERR_INVALID, "bytes %lld is negative", (long long)bytes);
    int rc;
    if ((rc = set_device(ctx))) return rc;
    if (!bytes) return GARLIC_OK;
    HIP_TRY(hipMemcpyAsync(dst, src, (size_t)bytes, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return GARLIC_OK;
}

int garlic_device_copy(garlic_ctx *ctx, void *dst, const void *src, int64_t bytes)
{
    if (!ctx || !dst || !src) return fail(GARLIC_ERR_INVALID, "context, dst and src are required");
    if (bytes < 0) return fail(GARLIC_ERR_INVALID, "bytes %lld is negative", (long long)bytes);
    const uintptr_t d = (uintptr_t)dst, f = (uintptr_t)src;
    if (d < f + (uintptr_t)bytes && f < d + (uintptr_t)bytes && bytes) return fail(GARLIC_ERR_INVALID, "the ranges overlap");
    int rc;
    if ((rc = set_device(ctx))) return rc;
    if (!bytes) return GARLIC_OK;
    HIP_TRY(hipMemcpyAsync(dst, src, (size_t)bytes, hipMemcpyDeviceToDevice, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return GARLIC_OK;
}

// ---- BGZF text on the device (bgzf_kernels.hpp)
int garlic_bgzf_inflate(garlic_ctx *ctx, const void *comp, int64_t comp_bytes, const int64_t *block_begin, int64_t nblocks, void *out,
                        const int64_t *out_begin, int32_t *block_status, int32_t where)
{
    if (!ctx || !block_begin || !out_begin) return fail(GARLIC_ERR_INVALID, "context, block_begin and out_begin are required");
    if (where != GARLIC_HOST && where != GARLIC_DEVICE) return fail(GARLIC_ERR_INVALID, "where must be GARLIC_HOST or GARLIC_DEVICE");
    if (nblocks < 0 || nblocks >= (1ll << 31) * BGZF_WAVES || comp_bytes < 0)
        return fail(GARLIC_ERR_INVALID, "nblocks %lld, comp_bytes %lld", (long long)nblocks, (long long)comp_bytes);
    if (!nblocks) return GARLIC_OK;
    if (!comp || !out) return fail(GARLIC_ERR_INVALID, "comp and out are required");
    if (block_begin[0] < 0 || block_begin[nblocks] > comp_bytes || out_begin[0] < 0)
        return fail(GARLIC_ERR_INVALID, "the blocks must lie inside comp_bytes = %lld, the output ranges at or behind 0", (long long)comp_bytes);
    for (int64_t b = 0; b < nblocks; b++) {
        const int64_t m = block_begin[b + 1] - block_begin[b], o = out_begin[b + 1] - out_begin[b];
        if (m < BGZF_MEMBER_MIN || m > BGZF_MEMBER_MAX || o < 0 || o > BGZF_MEMBER_MAX)
            return fail(GARLIC_ERR_INVALID, "block %lld: %lld bytes to %lld: a BGZF block has %lld to %lld bytes and inflates to at most %lld",
                        (long long)b, (long long)m, (long long)o, (long long)BGZF_MEMBER_MIN, (long long)BGZF_MEMBER_MAX, (long long)BGZF_MEMBER_MAX);
    }
    int rc;
    if ((rc = set_device(ctx))) return rc;
    BgzfScratch &sc = ctx->bgzf;
    hipStream_t s = ctx->stream;
    const uint8_t *d_comp = reinterpret_cast<const uint8_t *>(comp);
    if (where == GARLIC_HOST) {
        if ((rc = sc.comp.reserve((size_t)comp_bytes))) return rc;
        HIP_TRY(hipMemcpyAsync(sc.comp.p, comp, (size_t)comp_bytes, hipMemcpyHostToDevice, s));
        d_comp = sc.comp.p;
    }
    const size_t n1 = (size_t)nblocks + 1;
    if ((rc = sc.offsets.reserve(2 * n1)) || (rc = sc.status.reserve((size_t)nblocks))) return rc;
    HIP_TRY(hipMemcpyAsync(sc.offsets.p, block_begin, sizeof(int64_t) * n1, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(sc.offsets.p + n1, out_begin, sizeof(int64_t) * n1, hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(bgzf_inflate_kernel, dim3((unsigned)((nblocks + BGZF_WAVES - 1) / BGZF_WAVES)), dim3(WAVE * BGZF_WAVES), 0, s, d_comp,
                       sc.offsets.p, nblocks, reinterpret_cast<uint8_t *>(out), sc.offsets.p + n1, sc.status.p);
    HIP_TRY(hipGetLastError());
    std::vector<int32_t> own;                                 // only a caller without block_status needs it
    if (!block_status) own.resize((size_t)nblocks);
    int32_t *status = block_status ? block_status : own.data();
    HIP_TRY(hipMemcpyAsync(status, sc.status.p, sizeof(int32_t) * (size_t)nblocks, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    for (int64_t b = 0; b < nblocks; b++)
        if (status[(size_t)b]) {
            static const char *const what[] = {"", "bad block type or header", "bad code lengths", "bad symbol", "bad distance", "input ended",
                                               "output full", "output short", "bad CRC32"};
            const int32_t c = status[(size_t)b];
            return fail(GARLIC_ERR_INVALID, "BGZF block %lld (at byte %lld): status %d (%s)", (long long)b, (long long)block_begin[b], (int)c,
                        c > 0 && c < 9 ? what[c] : "?");
        }
    return GARLIC_OK;
}

int garlic_text_lines(garlic_ctx *ctx, const void *text, int64_t text_bytes, int32_t last, int64_t seen, int64_t head_bytes,
                      int64_t capacity, int64_t *begin, int64_t *end, int64_t *number, void *heads, int64_t *n_lines,
                      int64_t *consumed, int64_t *seen_out)
{
    if (!ctx || !n_lines || !consumed || !seen_out) return fail(GARLIC_ERR_INVALID, "context, n_lines, consumed and seen_out are required");
    if (text_bytes < 0 || text_bytes >= (1ll << 31) || capacity < 0 || (capacity > 0 && (!begin || !end || !number)))
        return fail(GARLIC_ERR_INVALID, "text_bytes %lld must be below 2^31; begin, end and number need room for capacity %lld",
                    (long long)text_bytes, (long long)capacity);
    if (heads && (head_bytes < 1 || head_bytes > (1 << 20))) return fail(GARLIC_ERR_INVALID, "head_bytes %lld: 1 to 2^20", (long long)head_bytes);
    *n_lines = 0;
    *consumed = 0;
    *seen_out = seen;
    if (!text_bytes) return GARLIC_OK;
    if (!text) return fail(GARLIC_ERR_INVALID, "text is required");
    int rc;
    if ((rc = set_device(ctx))) return rc;
    BgzfScratch &sc = ctx->bgzf;
    hipStream_t s = ctx->stream;
    const uint8_t *d_text = reinterpret_cast<const uint8_t *>(text);
    const int64_t tiles = (text_bytes + (int64_t)((uintptr_t)text & 15) + TEXT_LINES_TILE - 1) / TEXT_LINES_TILE;
    if ((rc = sc.tiles.reserve((size_t)(2 * tiles))) || (rc = sc.res.reserve(1))) return rc;
    int32_t *t_newlines = sc.tiles.p, *t_full = sc.tiles.p + tiles;
    hipLaunchKernelGGL(text_lines_count_kernel, dim3((unsigned)tiles), dim3(TEXT_PASS_PIECES), 0, s, d_text, text_bytes, t_newlines, t_full);
    hipLaunchKernelGGL(text_lines_scan_kernel, dim3(1), dim3(TEXT_PASS_PIECES), 0, s, t_newlines, t_full, tiles, sc.res.p);
    HIP_TRY(hipGetLastError());
    TextLinesResult res = {};
    HIP_TRY(hipMemcpyAsync(&res, sc.res.p, sizeof res, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    const int64_t cap = res.lines + 1;                        // the lines that end at a '\n', and a last one that does not
    if ((rc = sc.lines.reserve((size_t)(3 * cap)))) return rc;
    int64_t *d_begin = sc.lines.p, *d_end = d_begin + cap, *d_number = d_end + cap;
    hipLaunchKernelGGL(text_lines_write_kernel, dim3((unsigned)tiles), dim3(TEXT_PASS_PIECES), 0, s, d_text, text_bytes, (int)(last != 0), seen,
                       t_newlines, t_full, res.newlines, cap, d_begin, d_end, d_number, sc.res.p);
    const bool want_heads = heads && cap <= capacity + 1;
    if (want_heads) {
        if ((rc = sc.heads.reserve((size_t)(cap * head_bytes)))) return rc;
        const int64_t blocks = std::min<int64_t>((cap * head_bytes + 255) / 256, 8 * (int64_t)ctx->n_cu);
        hipLaunchKernelGGL(text_heads_kernel, dim3((unsigned)blocks), dim3(256), 0, s, d_text, d_begin, d_end, cap, sc.res.p, head_bytes,
                           text_bytes, sc.heads.p);
    }
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(&res, sc.res.p, sizeof res, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    *n_lines = res.lines;
    *consumed = res.consumed;
    *seen_out = seen + res.taken;
    if (res.lines > capacity) return fail(GARLIC_ERR_RANGE, "the slab holds %lld lines, the arrays %lld", (long long)res.lines, (long long)capacity);
    if (res.lines) {
        const size_t nb = sizeof(int64_t) * (size_t)res.lines;
        HIP_TRY(hipMemcpyAsync(begin, d_begin, nb, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipMemcpyAsync(end, d_end, nb, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipMemcpyAsync(number, d_number, nb, hipMemcpyDeviceToHost, s));
        if (heads) HIP_TRY(hipMemcpyAsync(heads, sc.heads.p, (size_t)(res.lines * head_bytes), hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
    }
    return GARLIC_OK;
}

int garlic_device_trim(garlic_ctx *ctx)
{
    if (!ctx) return fail(GARLIC_ERR_INVALID, "context is required");
    int rc;
    if ((rc = set_device(ctx))) return rc;
    return score_pool_trim();
}

int garlic_device_alloc_stats(garlic_ctx *ctx, int64_t *live_bytes, int64_t *pooled_bytes, int64_t *reserved_bytes)
{
    if (!ctx) return fail(GARLIC_ERR_INVALID, "context is required");
    std::lock_guard<std::mutex> lock(g_score_mutex);
    int64_t live = 0, pooled = 0;
    for (const ScoreAlloc &a : g_score_allocs)
        if (a.device == ctx->device) (a.pooled ? pooled : live) += (int64_t)a.size;
    if (live_bytes) *live_bytes = live;
    if (pooled_bytes) *pooled_bytes = pooled;
    if (reserved_bytes) *reserved_bytes = live + pooled + g_score_retired[ctx->device < 16 ? ctx->device : 15];
    return GARLIC_OK;
}

// Score memory in the chain kernel's fast placement: `candidates` buffers side by side, the real
// kernel for `winsize` timed into each (one pass that builds the plan, four in a row, the last three timed), the
// fastest kept, the others returned to the pool.
int garlic_panel_alloc_scores(garlic_panel *p, int32_t pitch_align, int32_t nind_out, int32_t winsize, double error,
                              int32_t max_gap, int32_t candidates, void **out, float *candidate_ms)
{
    if (!p || !out) return fail(GARLIC_ERR_INVALID, "panel and result pointer are required");
    if (nind_out < 1 || nind_out > p->nind) return fail(GARLIC_ERR_INVALID, "nind_out outside the panel");
    int rc;
    if ((rc = set_device(p->ctx))) return rc;
    *out = nullptr;
    if (candidates <= 0) candidates = 4;
    candidates = std::min(candidates, 16);
    const Layout L = make_layout(p, pitch_align, nind_out);
    // Candidates come in rounds.  Buffers of one round are cut from neighbouring physical memory and can ALL land on
    // the slow side (profiles/r03_bench_plain_all_candidates_slow.json: eight candidates at 1.65 ms on a fresh device, 1.35 ms
    // one process later), and the times are not two clean classes either (BENCH_r03: 1.44 kept / 1.50 median / 1.54 worst
    // in one round, 1.34-1.40 on other leases), so a relative spread inside a round says little.  The criterion is the
    // kernel's own bound: a round whose best candidate takes its score bytes at >= 0.74 of the HBM peak (1.39 ms at 1M SNPs
    // x 1000 individuals) has found the fast placement; otherwise another round is taken from fresh memory while the
    // earlier ones are still held (so that the allocator cannot hand the same pages back) -- three rounds at most
    // (GARLIC_ALLOC_ROUNDS), 2 s at most, memory permitting.  The best of all rounds is kept; how many were drawn and what
    // they timed: garlic_panel_alloc_scores_info.
    int max_rounds = 3;
    if (const char *e = getenv("GARLIC_ALLOC_ROUNDS")) max_rounds = std::max(1, std::min(atoi(e), 4));
    const size_t bytes = sizeof(double) * (size_t)L.total;
    const float target_ms = (float)((double)bytes / (0.74 * 8.0e12) * 1e3);
    std::vector<void *> cand;
    std::vector<float> ms;
    std::vector<size_t> round_start;
    auto cleanup = [&](int keep) {
        for (int k = 0; k < (int)cand.size(); k++)
            if (k != keep && cand[(size_t)k]) (void)score_free(p->ctx, cand[(size_t)k]);
    };
    garlic_ctx *ctx = p->ctx;
    const bool was_async = ctx->async_device;
    const auto t_begin = std::chrono::steady_clock::now();
    int best = -1, best_round = 0;
    for (int round = 0; round < max_rounds; round++) {
        const size_t base = cand.size();
        round_start.push_back(base);
        for (int k = 0; k < candidates; k++) {
            void *q = nullptr;
            if ((rc = score_alloc(ctx, bytes, &q))) break;
            cand.push_back(q);
            ms.push_back(0.f);
        }
        const bool short_round = rc != 0;
        if (short_round) {
            if (round == 0 && cand.empty()) return rc;
            g_last_error.clear();   // no room for (all of) another round: what there is stands
            rc = 0;
        }
        // passes enqueued back to back, as a caller that keeps the scores on the device issues them (a pass that is waited
        // for runs ~5 % faster than one in a queue: DESIGN.md section 4): one pass to build the plan, then four in a row,
        // the last three timed by their HIP events
        for (size_t k = base; k < cand.size(); k++) {
            ctx->async_device = false;
            rc = launch_lod(p, MODE_LOD, winsize, error, max_gap, 0, 0.0, 0, nind_out, pitch_align, (double *)cand[k], GARLIC_DEVICE);
            ctx->async_device = true;
            for (int pass = 0; pass < 4 && !rc; pass++)
                rc = launch_lod(p, MODE_LOD, winsize, error, max_gap, 0, 0.0, 0, nind_out, pitch_align, (double *)cand[k], GARLIC_DEVICE);
            ctx->async_device = was_async;
            if (rc) { cleanup(-1); return rc; }
            hipError_t e = hipStreamSynchronize(ctx->stream);
            if (e != hipSuccess) { cleanup(-1); return fail(GARLIC_ERR_HIP, "alloc_scores: %s", hipGetErrorString(e)); }
            float acc = 0.f;
            for (int q = 1; q <= 3; q++) {
                const int slot = (int)((ctx->n_calls - q) % garlic_ctx::HIST);
                float t = 0.f;
                (void)hipEventElapsedTime(&t, ctx->hist0[slot], ctx->hist1[slot]);
                acc += t;
            }
            ms[k] = acc / 3;
            if (best < 0 || ms[k] < ms[(size_t)best]) { best = (int)k; best_round = round; }
        }
        const double elapsed = std::chrono::duration<double>(std::chrono::steady_clock::now() - t_begin).count();
        if (short_round || ms[(size_t)best] <= target_ms || elapsed > 2.0) break;
    }
    if (candidate_ms) {
        memset(candidate_ms, 0, sizeof(float) * (size_t)candidates);
        const size_t r0 = round_start[(size_t)best_round];
        const size_t r1 = (size_t)best_round + 1 < round_start.size() ? round_start[(size_t)best_round + 1] : ms.size();
        memcpy(candidate_ms, ms.data() + r0, sizeof(float) * std::min((size_t)candidates, r1 - r0));
    }
    {
        std::vector<float> sorted(ms);
        std::sort(sorted.begin(), sorted.end());
        p->placement = garlic_panel::Placement{(int32_t)ms.size(), (int32_t)round_start.size(), sorted.front(),
                                               sorted[sorted.size() / 2], sorted.back(), target_ms,
                                               sorted.front() <= target_ms ? 1 : 0};
    }
    cleanup(best);
    *out = cand[(size_t)best];
    return GARLIC_OK;
}

int garlic_panel_alloc_scores_info(garlic_panel *p, int32_t *drawn, int32_t *rounds, float *best_ms, float *median_ms,
                                   float *worst_ms, float *target_ms, int32_t *reached_target)
{
    if (!p) return fail(GARLIC_ERR_INVALID, "panel is NULL");
    if (p->placement.drawn == 0) return fail(GARLIC_ERR_STATE, "garlic_panel_alloc_scores has not run on this panel");
    if (drawn) *drawn = p->placement.drawn;
    if (rounds) *rounds = p->placement.rounds;
    if (best_ms) *best_ms = p->placement.best_ms;
    if (median_ms) *median_ms = p->placement.median_ms;
    if (worst_ms) *worst_ms = p->placement.worst_ms;
    if (target_ms) *target_ms = p->placement.target_ms;
    if (reached_target) *reached_target = p->placement.reached;
    return GARLIC_OK;
}

int garlic_panel_set_feed_order(garlic_panel *p, int32_t order)
{
    if (!p) return fail(GARLIC_ERR_INVALID, "panel is NULL");
    if (order != GARLIC_FEED_ORDER_REFERENCE && order != GARLIC_FEED_ORDER_SORTED)
        return fail(GARLIC_ERR_INVALID, "feed order must be GARLIC_FEED_ORDER_REFERENCE or GARLIC_FEED_ORDER_SORTED (got %d)", order);
    p->feed_order = order;
    return GARLIC_OK;
}

int garlic_feed_sort(garlic_ctx *ctx, double *values, int64_t n, int32_t where)
{
    if (!ctx) return fail(GARLIC_ERR_INVALID, "context is NULL");
    if (n < 0) return fail(GARLIC_ERR_INVALID, "feed sort: n must be >= 0 (got %lld)", (long long)n);
    if (n > 0 && !values) return fail(GARLIC_ERR_INVALID, "feed sort: values is NULL");
    if (where != GARLIC_HOST && where != GARLIC_DEVICE) return fail(GARLIC_ERR_INVALID, "feed sort: where must be GARLIC_HOST or GARLIC_DEVICE");
    int rc;
    if ((rc = set_device(ctx))) return rc;
    if (n <= 1) {                                    // nothing to order
        ctx->fs_run = 0;
        ctx->fs_skipped = 8;
        ctx->fs_scratch_bytes = (int64_t)ctx->fs.bytes();
        return GARLIC_OK;
    }
    hipStream_t s = ctx->stream;
    if ((rc = sort_reserve(ctx->fs, n))) return rc;   // before the caller's data is touched
    if (where == GARLIC_DEVICE) {
        if ((rc = sort_feed(ctx, s, values, n, ctx->fs, true))) return rc;
        return sort_result(ctx, s, values, ctx->fs, nullptr);
    }
    if ((rc = ctx->fs.stage.reserve((size_t)n))) return rc;
    HIP_TRY(hipMemcpyAsync(ctx->fs.stage.p, values, sizeof(double) * (size_t)n, hipMemcpyHostToDevice, s));
    if ((rc = sort_feed(ctx, s, ctx->fs.stage.p, n, ctx->fs, false))) return rc;
    const double *from = nullptr;
    if ((rc = sort_result(ctx, s, ctx->fs.stage.p, ctx->fs, &from))) return rc;
    HIP_TRY(hipMemcpy(values, from, sizeof(double) * (size_t)n, hipMemcpyDeviceToHost));
    return GARLIC_OK;
}

int garlic_feed_sort_info(garlic_ctx *ctx, int32_t *passes_run, int32_t *passes_skipped, int64_t *scratch_bytes)
{
    if (!ctx) return fail(GARLIC_ERR_INVALID, "context is NULL");
    if (passes_run) *passes_run = ctx->fs_run;
    if (passes_skipped) *passes_skipped = ctx->fs_skipped;
    if (scratch_bytes) *scratch_bytes = ctx->fs_scratch_bytes;
    return GARLIC_OK;
}

// ---- computeKDE on the device (kde_kernels.hpp, kde_multi_kernels.hpp; host arithmetic: host/kde_select.hpp; the plan:
// host/kde_multi_plan.hpp).  One driver for one feed and for several: the single calls are its batch of one.

// where the six order statistics of n values lie, and the weights of the two quartile mixes
static void kde_stat_index(int64_t n, KdeIdx &idx, double &delta25, double &delta75)
{
    namespace gh = garlic_host;
    idx.at[0] = 0;
    idx.at[1] = n - 1;
    gh::kdeQuantileIndex(n, 0.25, &idx.at[2], &delta25);
    gh::kdeQuantileIndex(n, 0.75, &idx.at[4], &delta75);
    idx.at[3] = idx.at[2] + 1;
    idx.at[5] = idx.at[4] + 1;
}

// what the moments say of a feed: refused (the cause in the error text), or n, lo, hi, sd, the quartiles, h and the targets
// in r, with 1 / h^2 for the sums (garlic_feed_kde and garlic_feed_kde_multi run these lines)
static int kde_from_moments(const KdeMoments &mom, int64_t n, const KdeIdx &idx, double delta25, double delta75, garlic_kde &r,
                            double &inv_h2)
{
    namespace gh = garlic_host;
    if (mom.flags & KDE_FLAG_NOT_FINITE) return fail(GARLIC_ERR_INVALID, "feed KDE: the values hold a NaN or an infinity");
    if (mom.flags & KDE_FLAG_NOT_ASCENDING) return fail(GARLIC_ERR_INVALID, "feed KDE: the values are not in ascending order (garlic_feed_sort)");
    r.n = n;
    r.lo = mom.stat[0];
    r.hi = mom.stat[1];
    r.sd = sqrt(mom.ssq / (double)(n - 1));
    r.q25 = idx.at[2] >= n - 1 ? mom.stat[2] : gh::kdeQuantileMix(mom.stat[2], mom.stat[3], delta25);
    r.q75 = idx.at[4] >= n - 1 ? mom.stat[4] : gh::kdeQuantileMix(mom.stat[4], mom.stat[5], delta75);
    r.h = gh::kdeBandwidth(r.sd, r.q25, r.q75, n);
    if (!(r.h > 0) || !std::isfinite(r.h))
        return fail(GARLIC_ERR_INVALID, "feed KDE: bandwidth %g (sd %g, quartiles %g and %g): all values equal, or no spread between the quartiles",
                    r.h, r.sd, r.q25, r.q75);
    gh::kdeTargets(r.lo, r.hi, r.h, r.x);
    inv_h2 = 1.0 / (r.h * r.h);
    if (!std::isfinite(inv_h2)) return fail(GARLIC_ERR_INVALID, "feed KDE: bandwidth %g is too small to square", r.h);
    return GARLIC_OK;
}

// what a KDE driver refuses of one feed: the code and the bare words (garlic_feed_kde's), and on a split feed the set whose
// part caused it (-1: the union as a whole).  Only the public calls add "feed i: " and "set p: ", or nothing.
struct KdeRefusal {
    int32_t code = GARLIC_OK;
    int set = -1;
    std::string why;
    std::string last;                      // where several parts refuse one feed: the words of the last of them (else empty)
};

static bool kde_any_refused(const KdeRefusal *refused, int n_feeds)
{
    return std::any_of(refused, refused + n_feeds, [](const KdeRefusal &r) { return r.code != GARLIC_OK; });
}

// a single-feed call's refusal, in its own words.  Where several parts of the feed are refused, the code is the first
// part's and the text the last part's: garlic_kde_parts waits for every part, and each refusal leaves its sentence.
static int kde_report_one(const KdeRefusal &refused)
{
    if (!refused.code) return GARLIC_OK;
    return fail(refused.code, "%s", (refused.last.empty() ? refused.why : refused.last).c_str());
}

// a multi-feed call's refusals: the one of the lowest index as the call's error text; status NULL: as the call's code too
static int kde_report_feeds(const KdeRefusal *refused, int n_feeds, int32_t *status)
{
    int rc = GARLIC_OK;
    for (int i = n_feeds - 1; i >= 0; i--) {
        const KdeRefusal &r = refused[i];
        if (status) status[i] = r.code;
        if (!r.code) continue;
        rc = r.set < 0 ? fail(r.code, "feed %d: %s", i, r.why.c_str()) : fail(r.code, "feed %d: set %d: %s", i, r.set, r.why.c_str());
    }
    return status ? (int)GARLIC_OK : rc;
}

// The two launches of a step over a table of n_feeds descriptors (h: the host's copy, d: the device's).  The batched
// kernels serve any number of feeds.  Where the table holds ONE feed, the single-feed kernels of kde_kernels.hpp run
// on that feed's fields of the table instead: the same __device__ bodies, so the same bits, but x, n and the partition
// arrive as kernel arguments -- the batched kernels fetch them from the table, which costs every workgroup a dependent
// scalar load and turns the reads of x into flat loads (measured: profiles/kde_one_driver_ab.txt).
static void kde_launch_moments(hipStream_t s, const KdeFeedDesc *h, KdeFeedDesc *d, int n_feeds, const garlic_host::KdeMultiPlan &plan, int pass,
                               double *partial, int32_t *flags)
{
    if (n_feeds == 1 && h[0].n_chunks > 0) {
        hipLaunchKernelGGL(kde_moment_kernel, dim3((unsigned)h[0].n_chunks), dim3(KDE_THREADS), 0, s, h[0].x, h[0].n, pass, &d[0].mom, partial, flags);
        hipLaunchKernelGGL(kde_tree_kernel, dim3(1), dim3(KDE_THREADS), 0, s, h[0].x, h[0].n, h[0].n_chunks, pass, partial, flags, h[0].idx, &d[0].mom);
        return;
    }
    hipLaunchKernelGGL(kde_moment_multi_kernel, dim3((unsigned)plan.total_chunks), dim3(KDE_THREADS), 0, s, d, n_feeds, plan.chunk_first, pass,
                       partial, flags);
    hipLaunchKernelGGL(kde_tree_multi_kernel, dim3((unsigned)n_feeds), dim3(KDE_THREADS), 0, s, d, pass, partial, flags);
}

// divided: raw = the sums / n (a whole feed); not: the sums themselves (a part of a split feed)
static void kde_launch_sums(hipStream_t s, const KdeFeedDesc *h, KdeFeedDesc *d, int n_feeds, const garlic_host::KdeMultiPlan &plan, bool divided,
                            double *slices)
{
    if (n_feeds == 1 && h[0].active && h[0].n_slices > 0) {
        hipLaunchKernelGGL(kde_sum_kernel, dim3((unsigned)h[0].n_slices), dim3(KDE_THREADS), 0, s, h[0].x, h[0].n, h[0].n_chunks,
                           h[0].chunks_per_slice, d[0].targets, h[0].inv_h2, slices, &d[0].skipped);
        if (divided)
            hipLaunchKernelGGL(kde_slice_kernel, dim3(KDE_POINTS), dim3(KDE_THREADS), 0, s, slices, h[0].n_slices, h[0].n, d[0].raw);
        else
            hipLaunchKernelGGL(kde_slice_sum_kernel, dim3(KDE_POINTS), dim3(KDE_THREADS), 0, s, slices, h[0].n_slices, d[0].raw);
        return;
    }
    hipLaunchKernelGGL(kde_sum_multi_kernel, dim3((unsigned)plan.total_slices), dim3(KDE_THREADS), 0, s, d, n_feeds, plan.slice_first, slices);
    if (divided)
        hipLaunchKernelGGL(kde_slice_multi_kernel, dim3((unsigned)n_feeds * KDE_POINTS), dim3(KDE_THREADS), 0, s, d, slices);
    else
        hipLaunchKernelGGL(kde_slice_sum_multi_kernel, dim3((unsigned)n_feeds * KDE_POINTS), dim3(KDE_THREADS), 0, s, d, slices);
}

// The KDE of n_feeds whole feeds in one set of launches.  d_x[i]: n[i] device doubles, ascending (anything, NULL included,
// where n[i] < 2).  Six launches and two waits on the context's stream whatever n_feeds is; four and one when no feed is
// left after the moments.  few_fmt: the wording of the "at least 2 values" refusal of the caller (one %lld).  A nonzero
// return is a failure of the call; otherwise refused[i] says what became of feed i.  strict: the first refusal ends the
// call.  outs[i] is written for the feeds that were not refused, and `info`, after everything else has succeeded.
static int kde_multi_device(garlic_ctx *ctx, const double *const *d_x, const int64_t *n, int32_t n_feeds, const char *few_fmt,
                            bool strict, garlic_kde *outs, KdeRefusal *refused, KdeInfo &info)
{
    namespace gh = garlic_host;
    static_assert(GARLIC_KDE_MAX_FEEDS == gh::KDE_MULTI_MAX_FEEDS, "one limit");
    static_assert(KDE_POINTS == GARLIC_KDE_POINTS && gh::KDE_POINTS == GARLIC_KDE_POINTS, "one M");
    gh::KdeMultiPlan plan;
    if (!gh::kdeMultiPlan(n, n_feeds, &plan))
        return fail(GARLIC_ERR_INVALID, "feed KDE: the %d feeds are more chunks than one launch holds", (int)n_feeds);
    KdeMultiScratch &k = ctx->kdem;
    hipStream_t s = ctx->stream;
    int rc;
    if ((rc = k.partial.reserve((size_t)std::max<int64_t>(plan.total_chunks, 1))) ||
        (rc = k.flags.reserve((size_t)std::max<int64_t>(plan.total_chunks, 1))) ||
        (rc = k.slices.reserve((size_t)std::max<int64_t>(plan.total_slices, 1) * KDE_POINTS)) ||
        (rc = k.table.reserve(GARLIC_KDE_MAX_FEEDS)))
        return rc;
    for (auto &e : k.ev)
        if (!e) HIP_TRY(hipEventCreate(&e));
    // per feed: what the moments gave
    std::vector<garlic_kde> res((size_t)n_feeds);
    std::vector<KdeFeedDesc> table((size_t)n_feeds);
    std::vector<double> delta25((size_t)n_feeds, 0.0), delta75((size_t)n_feeds, 0.0);
    auto refuse = [&](int i, int c) { refused[i].code = c; refused[i].why = g_last_error; };
    auto stop = [&]() { return strict && kde_any_refused(refused, n_feeds); };
    memset(table.data(), 0, sizeof(KdeFeedDesc) * table.size());
    for (int i = 0; i < n_feeds; i++) {
        const gh::KdeMultiFeedPlan &f = plan.feed[i];
        KdeFeedDesc &d = table[(size_t)i];
        if (n[i] < 2) { refuse(i, fail(GARLIC_ERR_INVALID, few_fmt, (long long)n[i])); continue; }
        d.x = d_x[i];
        d.n = f.n;
        d.n_chunks = f.n_chunks;
        d.chunks_per_slice = f.chunks_per_slice;
        d.n_slices = f.n_slices;
        d.chunk_off = plan.chunk_first.at[i];
        d.slice_off = plan.slice_first.at[i];
        kde_stat_index(f.n, d.idx, delta25[(size_t)i], delta75[(size_t)i]);
    }
    int32_t launches = 0, waits = 0;
    const size_t table_bytes = sizeof(KdeFeedDesc) * (size_t)n_feeds;
    if (plan.total_chunks > 0 && !stop()) {
        HIP_TRY(hipMemcpyAsync(k.table.p, table.data(), table_bytes, hipMemcpyHostToDevice, s));
        HIP_TRY(hipEventRecord(k.ev[0], s));
        for (int pass = 0; pass < 2; pass++) {
            kde_launch_moments(s, table.data(), k.table.p, n_feeds, plan, pass, k.partial.p, k.flags.p);
            launches += 2;
        }
        HIP_TRY(hipEventRecord(k.ev[1], s));
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(table.data(), k.table.p, table_bytes, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        waits++;
    }
    // every h and every target set, then one upload
    int n_active = 0;
    for (int i = 0; i < n_feeds && waits; i++) {
        KdeFeedDesc &d = table[(size_t)i];
        if (refused[i].code) continue;
        if ((rc = kde_from_moments(d.mom, d.n, d.idx, delta25[(size_t)i], delta75[(size_t)i], res[(size_t)i], d.inv_h2))) {
            refuse(i, rc);
            continue;
        }
        memcpy(d.targets, res[(size_t)i].x, sizeof d.targets);
        d.skipped = 0;
        d.active = 1;
        n_active++;
    }
    if (stop()) return GARLIC_OK;
    if (n_active) {
        HIP_TRY(hipMemcpyAsync(k.table.p, table.data(), table_bytes, hipMemcpyHostToDevice, s));
        HIP_TRY(hipEventRecord(k.ev[2], s));
        kde_launch_sums(s, table.data(), k.table.p, n_feeds, plan, true, k.slices.p);
        launches += 2;
        HIP_TRY(hipEventRecord(k.ev[3], s));
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(table.data(), k.table.p, table_bytes, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        waits++;
    }
    info.chunks.assign((size_t)n_feeds, 0);
    info.skipped.assign((size_t)n_feeds, 0);
    for (int i = 0; i < n_feeds; i++) {
        const KdeFeedDesc &d = table[(size_t)i];
        info.chunks[(size_t)i] = d.n_chunks;
        if (refused[i].code) continue;
        garlic_kde &r = res[(size_t)i];
        memcpy(r.raw, d.raw, sizeof r.raw);
        gh::kdeNormalise(r.raw, r.x, r.y);
        info.skipped[(size_t)i] = (int64_t)d.skipped;
        outs[i] = r;
    }
    info.launches = launches;
    info.waits = waits;
    info.moments_ms = info.sums_ms = 0.f;
    if (waits && hipEventElapsedTime(&info.moments_ms, k.ev[0], k.ev[1]) != hipSuccess) info.moments_ms = 0.f;
    if (n_active && hipEventElapsedTime(&info.sums_ms, k.ev[2], k.ev[3]) != hipSuccess) info.sums_ms = 0.f;
    return GARLIC_OK;
}

// one feed: the batch of one, refused in garlic_feed_kde's words ("feed KDE: ..." and no more)
static int kde_one_device(garlic_ctx *ctx, const double *d_x, int64_t n, garlic_kde *out)
{
    if ((n + KDE_CHUNK - 1) / KDE_CHUNK > 0x7fffffff)
        return fail(GARLIC_ERR_INVALID, "feed KDE: %lld values are more chunks than one launch holds", (long long)n);
    KdeRefusal refused;
    const int rc = kde_multi_device(ctx, &d_x, &n, 1, "feed KDE: needs at least 2 values (got %lld)", true, out, &refused, ctx->kde_info);
    return rc ? rc : kde_report_one(refused);
}

int garlic_feed_kde(garlic_ctx *ctx, const double *sorted, int64_t n, int32_t where, garlic_kde *out)
{
    if (!ctx || !out) return fail(GARLIC_ERR_INVALID, "feed KDE: context and out are required");
    if (where != GARLIC_HOST && where != GARLIC_DEVICE) return fail(GARLIC_ERR_INVALID, "feed KDE: where must be GARLIC_HOST or GARLIC_DEVICE");
    if (n < 2) return fail(GARLIC_ERR_INVALID, "feed KDE: needs at least 2 values (got %lld)", (long long)n);
    if (!sorted) return fail(GARLIC_ERR_INVALID, "feed KDE: values is NULL");
    int rc;
    if ((rc = set_device(ctx))) return rc;
    if (where == GARLIC_DEVICE) return kde_one_device(ctx, sorted, n, out);
    if ((rc = ctx->kdem.stage.reserve((size_t)n))) return rc;
    HIP_TRY(hipMemcpyAsync(ctx->kdem.stage.p, sorted, sizeof(double) * (size_t)n, hipMemcpyHostToDevice, ctx->stream));
    return kde_one_device(ctx, ctx->kdem.stage.p, n, out);
}

int garlic_feed_kde_info(garlic_ctx *ctx, int64_t *chunks, int64_t *pairs_skipped, int64_t *scratch_bytes)
{
    if (!ctx) return fail(GARLIC_ERR_INVALID, "context is NULL");
    const KdeInfo &info = ctx->kde_info;
    if (chunks) *chunks = info.chunks.empty() ? 0 : info.chunks[0];
    if (pairs_skipped) *pairs_skipped = info.skipped.empty() ? 0 : info.skipped[0];
    if (scratch_bytes) *scratch_bytes = (int64_t)ctx->kdem.bytes();
    return GARLIC_OK;
}

int garlic_feed_kde_times(garlic_ctx *ctx, float *moments_ms, float *sums_ms)
{
    if (!ctx) return fail(GARLIC_ERR_INVALID, "context is NULL");
    if (moments_ms) *moments_ms = ctx->kde_info.moments_ms;
    if (sums_ms) *sums_ms = ctx->kde_info.sums_ms;
    return GARLIC_OK;
}

int garlic_lod_kde(garlic_panel *p, int32_t winsize, double error, int32_t max_gap, int32_t use_gl, int32_t weighted, int32_t M,
                   double mu, int32_t step, const int32_t *ind_idx, int32_t n_idx, garlic_kde *out, int64_t *chr_counts)
{
    if (!p || !out) return fail(GARLIC_ERR_INVALID, "panel and out are required");
    garlic_panel::FeedSink sink;
    int64_t count = 0;
    p->feed_sink = &sink;                  // the feed call sorts and leaves the values on the device; the order setting is not touched
    const int rc = garlic_lod_feed_subset(p, winsize, error, max_gap, use_gl, weighted, M, mu, step, ind_idx, n_idx, nullptr,
                                          INT64_MAX, &count, chr_counts);
    p->feed_sink = nullptr;
    if (rc) return rc;
    if (count < 2 || sink.size[0].n != count) return fail(GARLIC_ERR_INVALID, "feed KDE: needs at least 2 values (the feed holds %lld)", (long long)count);
    return kde_one_device(p->ctx, sink.size[0].data, sink.size[0].n, out);
}

// several feeds: "feed i: " in front of a refusal's words; status NULL: any refused feed fails the call
static int kde_feeds_device(garlic_ctx *ctx, const double *const *d_x, const int64_t *n, int32_t n_feeds, const char *few_fmt,
                            garlic_kde *outs, int32_t *status)
{
    KdeRefusal refused[GARLIC_KDE_MAX_FEEDS];
    const int rc = kde_multi_device(ctx, d_x, n, n_feeds, few_fmt, status == nullptr, outs, refused, ctx->kdem_info);
    return rc ? rc : kde_report_feeds(refused, n_feeds, status);
}

int garlic_feed_kde_multi(garlic_ctx *ctx, const double *const *sorted, const int64_t *n, int32_t n_feeds, int32_t where,
                          garlic_kde *outs, int32_t *status)
{
    if (!ctx || !sorted || !n || !outs) return fail(GARLIC_ERR_INVALID, "feed KDE: context, feeds, lengths and outs are required");
    if (n_feeds < 1 || n_feeds > GARLIC_KDE_MAX_FEEDS)
        return fail(GARLIC_ERR_INVALID, "feed KDE: %d feeds (1 to %d)", (int)n_feeds, GARLIC_KDE_MAX_FEEDS);
    if (where != GARLIC_HOST && where != GARLIC_DEVICE) return fail(GARLIC_ERR_INVALID, "feed KDE: where must be GARLIC_HOST or GARLIC_DEVICE");
    for (int i = 0; i < n_feeds; i++)
        if (n[i] > 0 && !sorted[i]) return fail(GARLIC_ERR_INVALID, "feed KDE: values of feed %d is NULL", i);
    int rc;
    if ((rc = set_device(ctx))) return rc;
    const char *few = "feed KDE: needs at least 2 values (got %lld)";
    if (where == GARLIC_DEVICE) return kde_feeds_device(ctx, sorted, n, n_feeds, few, outs, status);
    // host buffers: the feeds that can take part, one after the other in the context's scratch
    const double *d_x[GARLIC_KDE_MAX_FEEDS] = {};
    int64_t total = 0;
    for (int i = 0; i < n_feeds; i++)
        if (n[i] >= 2) {
            if (n[i] > INT64_MAX / 16 - total) return fail(GARLIC_ERR_INVALID, "feed KDE: the %d feeds are more chunks than one launch holds", (int)n_feeds);
            total += n[i];
        }
    if ((rc = ctx->kdem.stage.reserve((size_t)std::max<int64_t>(total, 1)))) return rc;
    int64_t at = 0;
    for (int i = 0; i < n_feeds; i++) {
        if (n[i] < 2) continue;
        HIP_TRY(hipMemcpyAsync(ctx->kdem.stage.p + at, sorted[i], sizeof(double) * (size_t)n[i], hipMemcpyHostToDevice, ctx->stream));
        d_x[i] = ctx->kdem.stage.p + at;
        at += n[i];
    }
    return kde_feeds_device(ctx, d_x, n, n_feeds, few, outs, status);
}

int garlic_feed_kde_multi_info(garlic_ctx *ctx, int32_t n, int64_t *chunks, int64_t *pairs_skipped, int32_t *kernel_launches,
                               int32_t *host_waits, int64_t *scratch_bytes, float *moments_ms, float *sums_ms)
{
    if (!ctx) return fail(GARLIC_ERR_INVALID, "context is NULL");
    if (n < 0 || (size_t)n > ctx->kdem_info.chunks.size())
        return fail(GARLIC_ERR_INVALID, "the last multi-feed KDE on the context had %d feeds (asked for %d)", (int)ctx->kdem_info.chunks.size(), (int)n);
    for (int i = 0; i < n; i++) {
        if (chunks) chunks[i] = ctx->kdem_info.chunks[(size_t)i];
        if (pairs_skipped) pairs_skipped[i] = ctx->kdem_info.skipped[(size_t)i];
    }
    if (kernel_launches) *kernel_launches = ctx->kdem_info.launches;
    if (host_waits) *host_waits = ctx->kdem_info.waits;
    if (scratch_bytes) *scratch_bytes = (int64_t)ctx->kdem.bytes();
    if (moments_ms) *moments_ms = ctx->kdem_info.moments_ms;
    if (sums_ms) *sums_ms = ctx->kdem_info.sums_ms;
    return GARLIC_OK;
}

int garlic_lod_kde_multi(garlic_panel *p, const int32_t *winsizes, const int32_t *steps, int32_t n_sizes, double error,
                         int32_t max_gap, int32_t use_gl, const int32_t *ind_idx, int32_t n_idx, garlic_kde *outs, int32_t *status,
                         int64_t *chr_counts)
{
    if (!p || !outs) return fail(GARLIC_ERR_INVALID, "panel and outs are required");
    if (!winsizes || !steps) return fail(GARLIC_ERR_INVALID, "panel, winsizes, steps, feeds, feed_capacity and counts are required");
    if (n_sizes < 1) return fail(GARLIC_ERR_INVALID, "n_sizes must be >= 1");
    if (n_sizes > GARLIC_KDE_MAX_FEEDS) return fail(GARLIC_ERR_INVALID, "feed KDE: %d window sizes (1 to %d)", (int)n_sizes, GARLIC_KDE_MAX_FEEDS);
    garlic_ctx *ctx = p->ctx;
    int rc;
    if ((rc = set_device(ctx)) || (rc = ensure_feed_slots(p, n_sizes))) return rc;
    // the feed call sorts every size and leaves it in that size's slot; the order setting is not touched
    garlic_panel::FeedSink sink(n_sizes);
    sink.to_slot = true;
    std::vector<double *> feeds((size_t)n_sizes, nullptr);
    std::vector<int64_t> cap((size_t)n_sizes, INT64_MAX), counts((size_t)n_sizes, 0);
    p->feed_sink = &sink;
    rc = use_gl ? garlic_lod_feed_multi_tgls(p, winsizes, steps, n_sizes, max_gap, ind_idx, n_idx, feeds.data(), cap.data(), counts.data(), chr_counts)
                : garlic_lod_feed_multi(p, winsizes, steps, n_sizes, error, max_gap, ind_idx, n_idx, feeds.data(), cap.data(), counts.data(),
                                        chr_counts);
    p->feed_sink = nullptr;
    if (rc) return rc;
    // the KDE on the context's stream, behind whatever the sizes' streams still hold
    const double *d_x[GARLIC_KDE_MAX_FEEDS] = {};
    int64_t n[GARLIC_KDE_MAX_FEEDS] = {};
    for (int i = 0; i < n_sizes; i++) {
        garlic_panel::FeedSlot &sl = *p->feed_slots[(size_t)i];
        HIP_TRY(hipEventRecord(sl.ev1, sl.stream));
        HIP_TRY(hipStreamWaitEvent(ctx->stream, sl.ev1, 0));
        const bool held = counts[(size_t)i] >= 2 && sink.size[(size_t)i].n == counts[(size_t)i];
        d_x[i] = held ? sink.size[(size_t)i].data : nullptr;
        n[i] = held ? counts[(size_t)i] : std::min<int64_t>(counts[(size_t)i], 1);
    }
    return kde_feeds_device(ctx, d_x, n, n_sizes, "feed KDE: needs at least 2 values (the feed holds %lld)", outs, status);
}

// ---- The KDE of feeds that are split into sorted parts (a sharded panel: one part of every feed per shard, on the
// shard's device).  n, the sums and the 512 Gaussian sums add over the parts, lo / hi are a min and a max, and the four
// order statistics come from rank queries (host/kde_parts.hpp).  A set holds one shard's part of every feed of a
// window-size sweep, and every step runs once per set for all its feeds (kde_part_set_kernels.hpp); a garlic_kde_part
// (below) is a set of one feed.  A set owns its scratch, so every step is enqueued on every set's stream before any is
// waited for.  The set's table of KdeFeedDesc lives in pinned memory and is mirrored on the device: the host writes
// what a step needs (who is active, the unions' means, the targets), the step uploads it, runs, and copies it back.
struct garlic_kde_part_set {
    garlic_ctx *ctx = nullptr;
    int32_t n_feeds = 0;
    garlic_host::KdeMultiPlan plan;
    int64_t n[GARLIC_KDE_MAX_FEEDS] = {};
    DevBuf<double> own;                            // host buffers' uploads, one after the other
    std::shared_ptr<uint64_t> gen;                 // a set borrowed from a panel: the panel's scratch count, and its value at creation
    uint64_t gen_at = 0;
    DevBuf<double> partial, slices;
    DevBuf<int32_t> flags;
    DevBuf<KdeFeedDesc> table;
    DevBuf<unsigned long long> keys;
    DevBuf<long long> below;
    void *pinned = nullptr;                        // h_table[n_feeds], h_keys and h_below [n_feeds][KDE_RANK_MAX]
    KdeFeedDesc *h_table = nullptr;
    unsigned long long *h_keys = nullptr;
    long long *h_below = nullptr;
    hipEvent_t ev[4] = {};                         // around the moment part and around the sums part
    int32_t rank_m = 0;
    int32_t launches = 0, waits = 0, rank_rounds = 0;   // garlic_kde_parts_multi_info
    float moments_ms = 0.f, sums_ms = 0.f;
    bool moments_timed = false;
    size_t table_bytes() const { return sizeof(KdeFeedDesc) * (size_t)n_feeds; }
    bool has_values() const { return plan.total_chunks > 0; }
};

static int kde_set_usable(const garlic_kde_part_set *set)
{
    if (!set) return fail(GARLIC_ERR_INVALID, "KDE part set is NULL");
    if (set->gen && *set->gen != set->gen_at)
        return fail(GARLIC_ERR_STATE, "KDE part set is stale: its panel has computed scores or a feed, or released its scratch, since the set was made");
    return GARLIC_OK;
}

static void kde_set_free(garlic_kde_part_set *set)
{
    for (auto &e : set->ev)
        if (e) (void)hipEventDestroy(e);
    if (set->pinned) (void)hipHostFree(set->pinned);
    delete set;
}

// everything a set's steps need, before anything is enqueued; d_x[i] may be filled in by the caller afterwards (h_table[i].x)
static int kde_set_new(garlic_ctx *ctx, const int64_t *n, int32_t n_feeds, garlic_kde_part_set **out)
{
    namespace gh = garlic_host;
    int rc;
    if ((rc = set_device(ctx))) return rc;
    std::unique_ptr<garlic_kde_part_set, void (*)(garlic_kde_part_set *)> set(new garlic_kde_part_set, kde_set_free);
    set->ctx = ctx;
    set->n_feeds = n_feeds;
    if (!gh::kdePartSetPlan(n, n_feeds, &set->plan))
        return fail(GARLIC_ERR_INVALID, "KDE part set: the %d feeds are more chunks than one launch holds", (int)n_feeds);
    const size_t probes = (size_t)n_feeds * KDE_RANK_MAX;
    if ((rc = set->partial.reserve((size_t)std::max<int64_t>(set->plan.total_chunks, 1))) ||
        (rc = set->flags.reserve((size_t)std::max<int64_t>(set->plan.total_chunks, 1))) ||
        (rc = set->slices.reserve((size_t)std::max<int64_t>(set->plan.total_slices, 1) * KDE_POINTS)) ||
        (rc = set->table.reserve((size_t)n_feeds)) || (rc = set->keys.reserve(probes)) || (rc = set->below.reserve(probes)))
        return rc;
    const size_t bytes = set->table_bytes() + probes * (sizeof(unsigned long long) + sizeof(long long));
    HIP_TRY(hipHostMalloc(&set->pinned, bytes, hipHostMallocDefault));
    memset(set->pinned, 0, bytes);
    set->h_table = static_cast<KdeFeedDesc *>(set->pinned);
    set->h_keys = reinterpret_cast<unsigned long long *>(set->h_table + n_feeds);
    set->h_below = reinterpret_cast<long long *>(set->h_keys + probes);
    for (auto &e : set->ev) HIP_TRY(hipEventCreate(&e));
    for (int i = 0; i < n_feeds; i++) {
        const gh::KdeMultiFeedPlan &f = set->plan.feed[i];
        KdeFeedDesc &d = set->h_table[i];
        set->n[i] = n[i];
        d.n = f.n;
        d.n_chunks = f.n_chunks;
        d.chunks_per_slice = f.chunks_per_slice;
        d.n_slices = f.n_slices;
        d.chunk_off = set->plan.chunk_first.at[i];
        d.slice_off = set->plan.slice_first.at[i];
        d.active = 1;
    }
    *out = set.release();
    return GARLIC_OK;
}

int garlic_kde_part_set_create(garlic_ctx *ctx, const double *const *sorted, const int64_t *n, int32_t n_feeds, int32_t where,
                               garlic_kde_part_set **out)
{
    if (!ctx || !sorted || !n || !out) return fail(GARLIC_ERR_INVALID, "KDE part set: context, feeds, lengths and set are required");
    if (n_feeds < 1 || n_feeds > GARLIC_KDE_MAX_FEEDS)
        return fail(GARLIC_ERR_INVALID, "KDE part set: %d feeds (1 to %d)", (int)n_feeds, GARLIC_KDE_MAX_FEEDS);
    if (where != GARLIC_HOST && where != GARLIC_DEVICE) return fail(GARLIC_ERR_INVALID, "KDE part set: where must be GARLIC_HOST or GARLIC_DEVICE");
    int64_t total = 0;
    for (int i = 0; i < n_feeds; i++) {
        if (n[i] < 0) return fail(GARLIC_ERR_INVALID, "KDE part set: n of feed %d must be >= 0 (got %lld)", i, (long long)n[i]);
        if (n[i] > 0 && !sorted[i]) return fail(GARLIC_ERR_INVALID, "KDE part set: values of feed %d is NULL", i);
        if (n[i] > INT64_MAX / 16 - total) return fail(GARLIC_ERR_INVALID, "KDE part set: the %d feeds are more chunks than one launch holds", (int)n_feeds);
        total += n[i];
    }
    garlic_kde_part_set *set = nullptr;
    int rc;
    if ((rc = kde_set_new(ctx, n, n_feeds, &set))) return rc;
    if (where == GARLIC_HOST && total > 0) {
        hipError_t e = hipSuccess;
        rc = set->own.reserve((size_t)total);
        int64_t at = 0;
        for (int i = 0; i < n_feeds && !rc && e == hipSuccess; i++) {
            if (n[i] == 0) continue;
            e = hipMemcpyAsync(set->own.p + at, sorted[i], sizeof(double) * (size_t)n[i], hipMemcpyHostToDevice, ctx->stream);
            set->h_table[i].x = set->own.p + at;
            at += n[i];
        }
        if (!rc && e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
        if (rc || e != hipSuccess) {
            kde_set_free(set);
            return rc ? rc : fail(GARLIC_ERR_HIP, "KDE part set upload: %s", hipGetErrorString(e));
        }
    } else {
        for (int i = 0; i < n_feeds; i++) set->h_table[i].x = n[i] > 0 ? sorted[i] : nullptr;
    }
    *out = set;
    return GARLIC_OK;
}

int garlic_lod_kde_part_set(garlic_panel *p, const int32_t *winsizes, const int32_t *steps, int32_t n_sizes, double error,
                            int32_t max_gap, int32_t use_gl, const int32_t *ind_idx, int32_t n_idx, garlic_kde_part_set **out,
                            int64_t *chr_counts)
{
    if (!p || !out) return fail(GARLIC_ERR_INVALID, "panel and set are required");
    if (!winsizes || !steps) return fail(GARLIC_ERR_INVALID, "panel, winsizes, steps, feeds, feed_capacity and counts are required");
    if (n_sizes < 1) return fail(GARLIC_ERR_INVALID, "n_sizes must be >= 1");
    if (n_sizes > GARLIC_KDE_MAX_FEEDS) return fail(GARLIC_ERR_INVALID, "feed KDE: %d window sizes (1 to %d)", (int)n_sizes, GARLIC_KDE_MAX_FEEDS);
    garlic_ctx *ctx = p->ctx;
    int rc;
    if ((rc = set_device(ctx)) || (rc = ensure_feed_slots(p, n_sizes))) return rc;
    // as garlic_lod_kde_multi: every size sorted and left in its slot
    garlic_panel::FeedSink sink(n_sizes);
    sink.to_slot = true;
    std::vector<double *> feeds((size_t)n_sizes, nullptr);
    std::vector<int64_t> cap((size_t)n_sizes, INT64_MAX), counts((size_t)n_sizes, 0);
    p->feed_sink = &sink;
    rc = use_gl ? garlic_lod_feed_multi_tgls(p, winsizes, steps, n_sizes, max_gap, ind_idx, n_idx, feeds.data(), cap.data(), counts.data(), chr_counts)
                : garlic_lod_feed_multi(p, winsizes, steps, n_sizes, error, max_gap, ind_idx, n_idx, feeds.data(), cap.data(), counts.data(),
                                        chr_counts);
    p->feed_sink = nullptr;
    if (rc) return rc;
    for (int i = 0; i < n_sizes; i++)
        if (counts[(size_t)i] > 0 && sink.size[(size_t)i].n != counts[(size_t)i])
            return fail(GARLIC_ERR_STATE, "KDE part set: the feed of size %d (%lld values) was not left on the device", i, (long long)counts[(size_t)i]);
    garlic_kde_part_set *set = nullptr;
    if ((rc = kde_set_new(ctx, counts.data(), n_sizes, &set))) return rc;
    // the set's steps run on the context's stream, behind whatever the sizes' streams still hold
    for (int i = 0; i < n_sizes; i++) {
        garlic_panel::FeedSlot &sl = *p->feed_slots[(size_t)i];
        hipError_t e = hipEventRecord(sl.ev1, sl.stream);
        if (e == hipSuccess) e = hipStreamWaitEvent(ctx->stream, sl.ev1, 0);
        if (e != hipSuccess) {
            kde_set_free(set);
            return fail(GARLIC_ERR_HIP, "KDE part set: %s", hipGetErrorString(e));
        }
        set->h_table[i].x = counts[(size_t)i] > 0 ? sink.size[(size_t)i].data : nullptr;
    }
    set->gen = p->scratch_gen;
    set->gen_at = *p->scratch_gen;
    *out = set;
    return GARLIC_OK;
}

int garlic_kde_part_set_destroy(garlic_kde_part_set *set)
{
    if (!set) return GARLIC_OK;
    (void)hipSetDevice(set->ctx->device);
    (void)hipStreamSynchronize(set->ctx->stream);
    kde_set_free(set);
    return GARLIC_OK;
}

int garlic_kde_part_set_counts(garlic_kde_part_set *set, int64_t *n)
{
    int rc;
    if ((rc = kde_set_usable(set))) return rc;
    if (!n) return fail(GARLIC_ERR_INVALID, "KDE part set: n is NULL");
    for (int i = 0; i < set->n_feeds; i++) n[i] = set->n[i];
    return GARLIC_OK;
}

// The steps in two halves: *_enqueue puts the work and the copy back on the set's stream, *_wait waits for that stream
// and reads the pinned table.  active[i] == 0 switches feed i off for this and every later step of the
// set, up to the next pass 0 (NULL: as it stands).  A set without a value enqueues nothing, the ranks excepted (they read
// no value, and upload the table themselves: a rank call may be a set's first).
static void kde_set_activate(garlic_kde_part_set *set, const int32_t *active)
{
    for (int i = 0; i < set->n_feeds && active; i++)
        if (!active[i]) set->h_table[i].active = 0;
}

// every feed on again without a pass 0 (a garlic_kde_part's step calls: each runs whatever an earlier step refused)
static void kde_set_reactivate(garlic_kde_part_set *set)
{
    for (int i = 0; i < set->n_feeds; i++) set->h_table[i].active = 1;
}

static int kde_set_moment_enqueue(garlic_kde_part_set *set, int pass, const double *means, const int32_t *active)
{
    int rc;
    if ((rc = set_device(set->ctx))) return rc;
    if (pass == 0) {                               // a new KDE: every feed takes part again, the counts of _info start over
        for (int i = 0; i < set->n_feeds; i++) set->h_table[i].active = 1;
        set->launches = set->waits = set->rank_rounds = 0;
    }
    kde_set_activate(set, active);
    if (!set->has_values()) return GARLIC_OK;
    hipStream_t s = set->ctx->stream;
    for (int i = 0; i < set->n_feeds && pass; i++) set->h_table[i].mom.mean = means[i];
    HIP_TRY(hipMemcpyAsync(set->table.p, set->h_table, set->table_bytes(), hipMemcpyHostToDevice, s));
    if (pass == 0) HIP_TRY(hipEventRecord(set->ev[0], s));
    hipLaunchKernelGGL(kde_moment_set_kernel, dim3((unsigned)set->plan.total_chunks), dim3(KDE_THREADS), 0, s, set->table.p, (int)set->n_feeds,
                       set->plan.chunk_first, pass, set->partial.p, set->flags.p);
    hipLaunchKernelGGL(kde_tree_set_kernel, dim3((unsigned)set->n_feeds), dim3(KDE_THREADS), 0, s, set->table.p, pass, set->partial.p, set->flags.p);
    set->launches += 2;
    if (pass == 1) HIP_TRY(hipEventRecord(set->ev[1], s));
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(set->h_table, set->table.p, set->table_bytes(), hipMemcpyDeviceToHost, s));
    return GARLIC_OK;
}

// values[i]: the sum (pass 0) or the squared deviations of feed i's part, 0.0 for an empty part; pass 0: lo / hi its ends and
// code[i], why[i] what its flags refuse (such a feed is switched off).  A feed that is not active is passed over.
static int kde_set_moment_wait(garlic_kde_part_set *set, int pass, double *values, double *lo, double *hi, int32_t *code, std::string *why)
{
    int rc;
    if ((rc = set_device(set->ctx))) return rc;
    if (set->has_values()) {
        HIP_TRY(hipStreamSynchronize(set->ctx->stream));
        set->waits++;
        set->moments_timed = pass == 1;
    }
    for (int i = 0; i < set->n_feeds; i++) {
        KdeFeedDesc &d = set->h_table[i];
        if (!d.active) continue;
        if (d.n == 0) {
            values[i] = 0.0;
            continue;
        }
        if (pass == 0 && (d.mom.flags & (KDE_FLAG_NOT_FINITE | KDE_FLAG_NOT_ASCENDING))) {
            const int c = d.mom.flags & KDE_FLAG_NOT_FINITE ? fail(GARLIC_ERR_INVALID, "feed KDE: the values hold a NaN or an infinity")
                                                            : fail(GARLIC_ERR_INVALID, "feed KDE: the values are not in ascending order (garlic_feed_sort)");
            d.active = 0;
            if (code) code[i] = c;
            if (why) why[i] = g_last_error;
            continue;
        }
        values[i] = pass == 0 ? d.mom.sum : d.mom.ssq;
        if (pass == 0 && lo) lo[i] = d.mom.stat[0];
        if (pass == 0 && hi) hi[i] = d.mom.stat[1];
    }
    return GARLIC_OK;
}

// keys: [n_feeds][m]
static int kde_set_rank_enqueue(garlic_kde_part_set *set, const uint64_t *keys, int32_t m)
{
    int rc;
    if ((rc = set_device(set->ctx))) return rc;
    hipStream_t s = set->ctx->stream;
    const size_t total = (size_t)set->n_feeds * (size_t)m;
    for (size_t i = 0; i < total; i++) set->h_keys[i] = keys[i];
    set->rank_m = m;
    HIP_TRY(hipMemcpyAsync(set->table.p, set->h_table, set->table_bytes(), hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(set->keys.p, set->h_keys, sizeof(unsigned long long) * total, hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(kde_rank_multi_kernel, dim3((unsigned)((total + KDE_RANK_SET_THREADS - 1) / KDE_RANK_SET_THREADS)), dim3(KDE_RANK_SET_THREADS),
                       0, s, set->table.p, (int)set->n_feeds, set->keys.p, (int)m, set->below.p);
    set->launches++;
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(set->h_below, set->below.p, sizeof(long long) * total, hipMemcpyDeviceToHost, s));
    return GARLIC_OK;
}

static int kde_set_rank_wait(garlic_kde_part_set *set)      // the counts of the active feeds are in h_below[i * rank_m ..]
{
    int rc;
    if ((rc = set_device(set->ctx))) return rc;
    HIP_TRY(hipStreamSynchronize(set->ctx->stream));
    set->waits++;
    set->rank_rounds++;
    return GARLIC_OK;
}

// targets: [n_feeds][512]; inv_h2: [n_feeds] (what an inactive feed's entries hold is not read)
static int kde_set_sums_enqueue(garlic_kde_part_set *set, const double *targets, const double *inv_h2, const int32_t *active)
{
    int rc;
    if ((rc = set_device(set->ctx))) return rc;
    kde_set_activate(set, active);
    if (!set->has_values()) return GARLIC_OK;
    hipStream_t s = set->ctx->stream;
    for (int i = 0; i < set->n_feeds; i++) {
        KdeFeedDesc &d = set->h_table[i];
        d.skipped = 0;
        if (!d.active) continue;
        memcpy(d.targets, targets + (size_t)i * KDE_POINTS, sizeof d.targets);
        d.inv_h2 = inv_h2[i];
    }
    HIP_TRY(hipMemcpyAsync(set->table.p, set->h_table, set->table_bytes(), hipMemcpyHostToDevice, s));
    HIP_TRY(hipEventRecord(set->ev[2], s));
    kde_launch_sums(s, set->h_table, set->table.p, set->n_feeds, set->plan, false, set->slices.p);
    set->launches += 2;
    HIP_TRY(hipEventRecord(set->ev[3], s));
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(set->h_table, set->table.p, set->table_bytes(), hipMemcpyDeviceToHost, s));
    return GARLIC_OK;
}

static int kde_set_sums_wait(garlic_kde_part_set *set)      // feed i's undivided sums are in h_table[i].raw (zeros for an empty part)
{
    int rc;
    if ((rc = set_device(set->ctx))) return rc;
    set->moments_ms = set->sums_ms = 0.f;
    if (set->has_values()) {
        HIP_TRY(hipStreamSynchronize(set->ctx->stream));
        set->waits++;
        if (set->moments_timed && hipEventElapsedTime(&set->moments_ms, set->ev[0], set->ev[1]) != hipSuccess) set->moments_ms = 0.f;
        if (hipEventElapsedTime(&set->sums_ms, set->ev[2], set->ev[3]) != hipSuccess) set->sums_ms = 0.f;
    }
    for (int i = 0; i < set->n_feeds; i++) {
        KdeFeedDesc &d = set->h_table[i];
        if (d.active && d.n == 0) memset(d.raw, 0, sizeof d.raw);
    }
    return GARLIC_OK;
}

// status of a step call: on entry a nonzero status[i] switches feed i off, on return it holds what this set refuses of it
static void kde_set_status_in(const garlic_kde_part_set *set, const int32_t *status, int32_t *active)
{
    for (int i = 0; i < set->n_feeds; i++) active[i] = !(status && status[i]);
}

int garlic_kde_part_set_moment(garlic_kde_part_set *set, int32_t pass, const double *means, double *values, double *lo, double *hi,
                               int32_t *status)
{
    int rc;
    if ((rc = kde_set_usable(set))) return rc;
    if (pass != 0 && pass != 1) return fail(GARLIC_ERR_INVALID, "KDE part set: pass must be 0 (sums) or 1 (squared deviations), got %d", (int)pass);
    if (!values || (pass == 1 && !means)) return fail(GARLIC_ERR_INVALID, "KDE part set: values and, for pass 1, means are required");
    int32_t active[GARLIC_KDE_MAX_FEEDS], code[GARLIC_KDE_MAX_FEEDS] = {};
    std::string why[GARLIC_KDE_MAX_FEEDS];
    kde_set_status_in(set, status, active);
    if ((rc = kde_set_moment_enqueue(set, pass, means, active)) || (rc = kde_set_moment_wait(set, pass, values, lo, hi, code, why))) return rc;
    for (int i = 0; i < set->n_feeds; i++) {
        if (!code[i]) continue;
        if (!status) return fail(code[i], "feed %d: %s", i, why[i].c_str());
        status[i] = code[i];
    }
    for (int i = set->n_feeds - 1; i >= 0; i--)
        if (code[i]) (void)fail(code[i], "feed %d: %s", i, why[i].c_str());      // (the text names the lowest refused feed)
    return GARLIC_OK;
}

int garlic_kde_part_set_rank(garlic_kde_part_set *set, const uint64_t *keys, int32_t m, int64_t *below)
{
    int rc;
    if ((rc = kde_set_usable(set))) return rc;
    if (m < 1 || m > KDE_RANK_MAX) return fail(GARLIC_ERR_INVALID, "KDE part set: %d probe keys per feed (1 to %d)", (int)m, KDE_RANK_MAX);
    if (!keys || !below) return fail(GARLIC_ERR_INVALID, "KDE part set: keys and below are required");
    if ((rc = kde_set_rank_enqueue(set, keys, m)) || (rc = kde_set_rank_wait(set))) return rc;
    for (int i = 0; i < set->n_feeds; i++) {
        if (!set->h_table[i].active) continue;
        for (int j = 0; j < m; j++) below[(size_t)i * m + j] = set->h_below[(size_t)i * m + j];
    }
    return GARLIC_OK;
}

int garlic_kde_part_set_sums(garlic_kde_part_set *set, const double *targets, const double *h, const int32_t *active, double *sums,
                             int64_t *pairs_skipped)
{
    int rc;
    if ((rc = kde_set_usable(set))) return rc;
    if (!targets || !h || !sums) return fail(GARLIC_ERR_INVALID, "KDE part set: targets, h and sums are required");
    kde_set_activate(set, active);
    double inv_h2[GARLIC_KDE_MAX_FEEDS] = {};
    for (int i = 0; i < set->n_feeds; i++) {
        if (!set->h_table[i].active) continue;
        inv_h2[i] = 1.0 / (h[i] * h[i]);
        if (!(h[i] > 0) || !std::isfinite(inv_h2[i]))
            return fail(GARLIC_ERR_INVALID, "feed %d: feed KDE: bandwidth %g cannot be used (zero, negative, not finite or too small to square)", i, h[i]);
    }
    if ((rc = kde_set_sums_enqueue(set, targets, inv_h2, nullptr)) || (rc = kde_set_sums_wait(set))) return rc;
    for (int i = 0; i < set->n_feeds; i++) {
        const KdeFeedDesc &d = set->h_table[i];
        if (!d.active) continue;
        memcpy(sums + (size_t)i * KDE_POINTS, d.raw, sizeof d.raw);
        if (pairs_skipped) pairs_skipped[i] = (int64_t)d.skipped;
    }
    return GARLIC_OK;
}

// The KDEs of the F unions whose parts lie in n_sets usable sets of F feeds each (garlic_kde_parts_multi; garlic_kde_parts
// with F = 1).  A nonzero return is a failure of the call; otherwise refused[i] says what became of union i.  strict: the
// first refusal ends the call.  outs[i] is written for the unions that were not refused, after everything has succeeded.
static int kde_parts_reduce(garlic_kde_part_set *const *sets, int32_t n_sets, bool strict, garlic_kde *outs, KdeRefusal *refused)
{
    namespace gh = garlic_host;
    static_assert(GARLIC_KDE_MAX_PARTS <= KDE_THREADS && gh::KDE_DESCENT_PROBES == KDE_RANK_MAX, "one descent round is one rank launch");
    int rc;
    const int F = sets[0]->n_feeds;
    const size_t nF = (size_t)F, nP = (size_t)n_sets;
    // per feed: what the steps gave
    std::vector<int32_t> active(nF, 1);
    std::vector<garlic_kde> res(nF);
    std::vector<int64_t> n(nF, 0);
    auto stop = [&]() { return strict && kde_any_refused(refused, F); };
    auto refuse = [&](int i, int c, int set, const std::string &words) {
        refused[i].code = c;
        refused[i].set = set;
        refused[i].why = words;
        active[(size_t)i] = 0;
    };
    for (int i = 0; i < F; i++) {
        for (int p = 0; p < n_sets; p++) n[(size_t)i] += sets[p]->n[i];
        if (n[(size_t)i] < 2) {
            const int c = fail(GARLIC_ERR_INVALID, "feed KDE: needs at least 2 values (the parts hold %lld)", (long long)n[(size_t)i]);
            refuse(i, c, -1, g_last_error);
        }
    }
    if (stop()) return GARLIC_OK;
    // a step on every set: all enqueued, then all waited for (the first error is the one returned)
    auto each = [&](auto enqueue, auto wait) {
        int first = GARLIC_OK;
        int enqueued = 0;
        for (; enqueued < n_sets && !first; enqueued++) first = enqueue(sets[enqueued], enqueued);
        for (int p = 0; p < (first ? enqueued - 1 : enqueued); p++) {
            const int r = wait(sets[p], p);
            if (r && !first) first = r;
        }
        return first;
    };
    // pass 0: the parts' sums, ends and flags
    std::vector<double> value(nP * nF, 0.0), lo(nF, 0.0), hi(nF, 0.0), mean(nF, 0.0);
    std::vector<uint64_t> lo_key(nF, 0), hi_key(nF, 0);
    std::vector<char> have_ends(nF, 0);
    if ((rc = each([&](garlic_kde_part_set *set, int) { return kde_set_moment_enqueue(set, 0, nullptr, active.data()); },
                   [&](garlic_kde_part_set *set, int p) {
                       std::vector<int32_t> c(nF, GARLIC_OK);
                       std::vector<std::string> w(nF);
                       const int r2 = kde_set_moment_wait(set, 0, &value[(size_t)p * nF], lo.data(), hi.data(), c.data(), w.data());
                       for (int i = 0; i < F && !r2; i++) {
                           if (c[(size_t)i] && !refused[i].code) refused[i] = KdeRefusal{c[(size_t)i], p, w[(size_t)i]};
                           if (c[(size_t)i]) refused[i].last = w[(size_t)i];
                           if (c[(size_t)i] || !set->h_table[i].active || set->n[i] == 0) continue;
                           const uint64_t kl = gh::kdeKey(lo[(size_t)i]), kh = gh::kdeKey(hi[(size_t)i]);
                           if (!have_ends[(size_t)i] || kl < lo_key[(size_t)i]) lo_key[(size_t)i] = kl;
                           if (!have_ends[(size_t)i] || kh > hi_key[(size_t)i]) hi_key[(size_t)i] = kh;
                           have_ends[(size_t)i] = 1;
                       }
                       return r2;
                   })))
        return rc;
    for (int i = 0; i < F; i++)
        if (refused[i].code) active[(size_t)i] = 0;
    if (stop()) return GARLIC_OK;
    std::vector<double> of_feed(nP);
    auto combine = [&](int i) {
        for (int p = 0; p < n_sets; p++) of_feed[(size_t)p] = value[(size_t)p * nF + (size_t)i];
        return gh::kdeCombine(of_feed.data(), n_sets);
    };
    for (int i = 0; i < F; i++) {
        if (!active[(size_t)i]) continue;
        garlic_kde &r = res[(size_t)i];
        r.n = n[(size_t)i];
        r.lo = gh::kdeKeyValue(lo_key[(size_t)i]);
        r.hi = gh::kdeKeyValue(hi_key[(size_t)i]);
        mean[(size_t)i] = combine(i) / (double)r.n;
    }
    // pass 1 about the unions' means
    if ((rc = each([&](garlic_kde_part_set *set, int) { return kde_set_moment_enqueue(set, 1, mean.data(), active.data()); },
                   [&](garlic_kde_part_set *set, int p) {
                       return kde_set_moment_wait(set, 1, &value[(size_t)p * nF], nullptr, nullptr, nullptr, nullptr);
                   })))
        return rc;
    // the four order statistics of every union: one descent, eight rounds
    std::vector<int64_t> rank(nF * 4, 0), k25(nF, 0), k75(nF, 0);
    std::vector<double> delta25(nF, 0.0), delta75(nF, 0.0), stat(nF * 4, 0.0);
    std::vector<uint8_t> descend(nF, 0);
    for (int i = 0; i < F; i++) {
        if (!active[(size_t)i]) continue;
        garlic_kde &r = res[(size_t)i];
        r.sd = sqrt(combine(i) / (double)(r.n - 1));
        gh::kdeQuantileIndex(r.n, 0.25, &k25[(size_t)i], &delta25[(size_t)i]);
        gh::kdeQuantileIndex(r.n, 0.75, &k75[(size_t)i], &delta75[(size_t)i]);
        const int64_t at[4] = {k25[(size_t)i], k25[(size_t)i] + 1, k75[(size_t)i], k75[(size_t)i] + 1};
        for (int q = 0; q < 4; q++) rank[(size_t)i * 4 + q] = at[q] < 0 ? 0 : (at[q] >= r.n ? r.n - 1 : at[q]);
        descend[(size_t)i] = 1;
    }
    int rounds = 0;
    const bool any_active = std::find(active.begin(), active.end(), 1) != active.end();
    if (any_active) {
        rc = gh::kdeSelectRanksMulti(F, rank.data(), descend.data(), [&](const uint64_t *probes, int m, int64_t *below) {
            for (size_t i = 0; i < nF * (size_t)m; i++) below[i] = 0;
            return each([&](garlic_kde_part_set *set, int) { return kde_set_rank_enqueue(set, probes, m); },
                        [&](garlic_kde_part_set *set, int) {
                            const int r2 = kde_set_rank_wait(set);
                            for (int i = 0; i < F && !r2; i++) {
                                if (!active[(size_t)i]) continue;
                                for (int j = 0; j < m; j++) below[(size_t)i * m + j] += set->h_below[(size_t)i * m + j];
                            }
                            return r2;
                        });
        }, stat.data(), &rounds);
        if (rc) return rc;
    }
    // every h and every target set
    std::vector<double> targets(nF * KDE_POINTS, 0.0), inv_h2(nF, 0.0);
    for (int i = 0; i < F; i++) {
        if (!active[(size_t)i]) continue;
        garlic_kde &r = res[(size_t)i];
        const double *st = &stat[(size_t)i * 4];
        r.q25 = k25[(size_t)i] >= r.n - 1 ? st[0] : gh::kdeQuantileMix(st[0], st[1], delta25[(size_t)i]);
        r.q75 = k75[(size_t)i] >= r.n - 1 ? st[2] : gh::kdeQuantileMix(st[2], st[3], delta75[(size_t)i]);
        r.h = gh::kdeBandwidth(r.sd, r.q25, r.q75, r.n);
        if (!(r.h > 0) || !std::isfinite(r.h)) {
            const int c = fail(GARLIC_ERR_INVALID, "feed KDE: bandwidth %g (sd %g, quartiles %g and %g): all values equal, or no spread between the quartiles",
                               r.h, r.sd, r.q25, r.q75);
            refuse(i, c, -1, g_last_error);
            continue;
        }
        gh::kdeTargets(r.lo, r.hi, r.h, r.x);
        inv_h2[(size_t)i] = 1.0 / (r.h * r.h);
        if (!std::isfinite(inv_h2[(size_t)i])) {
            const int c = fail(GARLIC_ERR_INVALID, "feed KDE: bandwidth %g is too small to square", r.h);
            refuse(i, c, -1, g_last_error);
            continue;
        }
        memcpy(&targets[(size_t)i * KDE_POINTS], r.x, sizeof r.x);
    }
    if (stop()) return GARLIC_OK;
    if (std::find(active.begin(), active.end(), 1) != active.end()) {
        if ((rc = each([&](garlic_kde_part_set *set, int) { return kde_set_sums_enqueue(set, targets.data(), inv_h2.data(), active.data()); },
                       [&](garlic_kde_part_set *set, int) { return kde_set_sums_wait(set); })))
            return rc;
    }
    std::vector<const double *> sums(nP);
    for (int i = 0; i < F; i++) {
        if (refused[i].code) continue;
        garlic_kde &r = res[(size_t)i];
        for (int p = 0; p < n_sets; p++) sums[(size_t)p] = sets[p]->h_table[i].raw;
        gh::kdeCombineSums(sums.data(), n_sets, KDE_POINTS, r.n, r.raw);
        gh::kdeNormalise(r.raw, r.x, r.y);
        outs[i] = r;
    }
    return GARLIC_OK;
}

int garlic_kde_parts_multi(garlic_kde_part_set *const *sets, int32_t n_sets, garlic_kde *outs, int32_t *status)
{
    if (!sets || !outs) return fail(GARLIC_ERR_INVALID, "KDE parts: sets and outs are required");
    if (n_sets < 1 || n_sets > GARLIC_KDE_MAX_PARTS) return fail(GARLIC_ERR_INVALID, "KDE parts: %d sets (1 to %d)", (int)n_sets, GARLIC_KDE_MAX_PARTS);
    int rc;
    for (int p = 0; p < n_sets; p++) {
        if (!sets[p]) return fail(GARLIC_ERR_INVALID, "KDE parts: set %d is NULL", p);
        for (int q = 0; q < p; q++)
            if (sets[q] == sets[p]) return fail(GARLIC_ERR_INVALID, "KDE parts: set %d is set %d again", p, q);
        if ((rc = kde_set_usable(sets[p]))) return rc;
        if (sets[p]->n_feeds != sets[0]->n_feeds)
            return fail(GARLIC_ERR_INVALID, "KDE parts: set %d holds %d feeds, set 0 holds %d", p, (int)sets[p]->n_feeds, (int)sets[0]->n_feeds);
    }
    KdeRefusal refused[GARLIC_KDE_MAX_FEEDS];
    if ((rc = kde_parts_reduce(sets, n_sets, status == nullptr, outs, refused))) return rc;
    return kde_report_feeds(refused, sets[0]->n_feeds, status);
}

int garlic_kde_parts_multi_info(garlic_kde_part_set *const *sets, int32_t n_sets, int64_t *chunks, int64_t *pairs_skipped,
                                int32_t *kernel_launches, int32_t *host_waits, int32_t *rank_rounds, float *moments_ms, float *sums_ms)
{
    if (!sets) return fail(GARLIC_ERR_INVALID, "KDE parts: sets is NULL");
    if (n_sets < 1 || n_sets > GARLIC_KDE_MAX_PARTS) return fail(GARLIC_ERR_INVALID, "KDE parts: %d sets (1 to %d)", (int)n_sets, GARLIC_KDE_MAX_PARTS);
    for (int p = 0; p < n_sets; p++) {
        if (!sets[p]) return fail(GARLIC_ERR_INVALID, "KDE parts: set %d is NULL", p);
        const int rc = kde_set_usable(sets[p]);
        if (rc) return rc;
        if (sets[p]->n_feeds != sets[0]->n_feeds)
            return fail(GARLIC_ERR_INVALID, "KDE parts: set %d holds %d feeds, set 0 holds %d", p, (int)sets[p]->n_feeds, (int)sets[0]->n_feeds);
        const size_t row = (size_t)p * (size_t)sets[0]->n_feeds;
        for (int i = 0; i < sets[p]->n_feeds; i++) {
            const KdeFeedDesc &d = sets[p]->h_table[i];
            if (chunks) chunks[row + (size_t)i] = d.n_chunks;
            if (pairs_skipped) pairs_skipped[row + (size_t)i] = d.active ? (int64_t)d.skipped : 0;
        }
        if (kernel_launches) kernel_launches[p] = sets[p]->launches;
        if (host_waits) host_waits[p] = sets[p]->waits;
        if (rank_rounds) rank_rounds[p] = sets[p]->rank_rounds;
        if (moments_ms) moments_ms[p] = sets[p]->moments_ms;
        if (sums_ms) sums_ms[p] = sets[p]->sums_ms;
    }
    return GARLIC_OK;
}

// ---- One feed split into parts: a garlic_kde_part is a part set of one feed behind a handle of its own, with its own
// wording for what the handle refuses.  Its step calls run the set's halves on the one feed, and garlic_kde_parts is the
// reduction of garlic_kde_parts_multi with F = 1, a refusal in garlic_feed_kde's bare words.
struct garlic_kde_part {
    garlic_kde_part_set *set = nullptr;
    int64_t chunks = 0, pairs_skipped = 0;         // garlic_kde_parts_info: of the part's last sums ...
    float sums_ms = 0.f;
    int32_t rank_rounds = 0;                       // ... and of the last garlic_kde_parts it took part in
};

// what the sums that have just been waited for leave for garlic_kde_parts_info
static void kde_part_note_sums(garlic_kde_part *part)
{
    part->chunks = part->set->h_table[0].n_chunks;
    part->pairs_skipped = (int64_t)part->set->h_table[0].skipped;
    part->sums_ms = part->set->sums_ms;
}

static int kde_part_usable(const garlic_kde_part *part)
{
    if (!part) return fail(GARLIC_ERR_INVALID, "KDE part is NULL");
    if (part->set->gen && *part->set->gen != part->set->gen_at)
        return fail(GARLIC_ERR_STATE, "KDE part is stale: its panel has computed scores or a feed, or released its scratch, since the part was made");
    return GARLIC_OK;
}

static void kde_part_free(garlic_kde_part *part)
{
    kde_set_free(part->set);
    delete part;
}

static int kde_part_new(garlic_ctx *ctx, int64_t n, garlic_kde_part **out)
{
    if (n > (int64_t)0x7fffffff * KDE_CHUNK) return fail(GARLIC_ERR_INVALID, "feed KDE: %lld values are more chunks than one launch holds", (long long)n);
    garlic_kde_part_set *set = nullptr;
    const int rc = kde_set_new(ctx, &n, 1, &set);
    if (rc) return rc;
    *out = new garlic_kde_part;
    (*out)->set = set;
    return GARLIC_OK;
}

int garlic_kde_part_create(garlic_ctx *ctx, const double *sorted, int64_t n, int32_t where, garlic_kde_part **out)
{
    if (!ctx || !out) return fail(GARLIC_ERR_INVALID, "KDE part: context and part are required");
    if (where != GARLIC_HOST && where != GARLIC_DEVICE) return fail(GARLIC_ERR_INVALID, "KDE part: where must be GARLIC_HOST or GARLIC_DEVICE");
    if (n < 0) return fail(GARLIC_ERR_INVALID, "KDE part: n must be >= 0 (got %lld)", (long long)n);
    if (n > 0 && !sorted) return fail(GARLIC_ERR_INVALID, "KDE part: values is NULL");
    garlic_kde_part *part = nullptr;
    int rc;
    if ((rc = kde_part_new(ctx, n, &part))) return rc;
    garlic_kde_part_set *set = part->set;
    set->h_table[0].x = n > 0 ? sorted : nullptr;
    if (where == GARLIC_HOST && n > 0) {
        hipError_t e = hipSuccess;
        if ((rc = set->own.reserve((size_t)n)) ||
            (e = hipMemcpyAsync(set->own.p, sorted, sizeof(double) * (size_t)n, hipMemcpyHostToDevice, ctx->stream)) != hipSuccess ||
            (e = hipStreamSynchronize(ctx->stream)) != hipSuccess) {
            kde_part_free(part);
            return rc ? rc : fail(GARLIC_ERR_HIP, "KDE part upload: %s", hipGetErrorString(e));
        }
        set->h_table[0].x = set->own.p;
    }
    *out = part;
    return GARLIC_OK;
}

int garlic_lod_kde_part(garlic_panel *p, int32_t winsize, double error, int32_t max_gap, int32_t use_gl, int32_t weighted, int32_t M,
                        double mu, int32_t step, const int32_t *ind_idx, int32_t n_idx, garlic_kde_part **out, int64_t *chr_counts)
{
    if (!p || !out) return fail(GARLIC_ERR_INVALID, "panel and part are required");
    garlic_panel::FeedSink sink;
    int64_t count = 0;
    p->feed_sink = &sink;                  // as garlic_lod_kde: sorted, left on the device
    int rc = garlic_lod_feed_subset(p, winsize, error, max_gap, use_gl, weighted, M, mu, step, ind_idx, n_idx, nullptr,
                                    INT64_MAX, &count, chr_counts);
    p->feed_sink = nullptr;
    if (rc) return rc;
    if (count > 0 && sink.size[0].n != count) return fail(GARLIC_ERR_STATE, "KDE part: the feed of %lld values was not left on the device", (long long)count);
    garlic_kde_part *part = nullptr;
    if ((rc = kde_part_new(p->ctx, count, &part))) return rc;
    part->set->h_table[0].x = count > 0 ? sink.size[0].data : nullptr;
    part->set->gen = p->scratch_gen;
    part->set->gen_at = *p->scratch_gen;
    *out = part;
    return GARLIC_OK;
}

int garlic_kde_part_destroy(garlic_kde_part *part)
{
    if (!part) return GARLIC_OK;
    (void)hipSetDevice(part->set->ctx->device);
    (void)hipStreamSynchronize(part->set->ctx->stream);
    kde_part_free(part);
    return GARLIC_OK;
}

int garlic_kde_part_count(garlic_kde_part *part, int64_t *n)
{
    int rc;
    if ((rc = kde_part_usable(part))) return rc;
    if (n) *n = part->set->n[0];
    return GARLIC_OK;
}

int garlic_kde_part_moment(garlic_kde_part *part, int32_t pass, double mean, double *value, double *lo, double *hi)
{
    int rc;
    if ((rc = kde_part_usable(part))) return rc;
    if (pass != 0 && pass != 1) return fail(GARLIC_ERR_INVALID, "KDE part: pass must be 0 (sum) or 1 (squared deviations), got %d", (int)pass);
    if (!value) return fail(GARLIC_ERR_INVALID, "KDE part: value is NULL");
    garlic_kde_part_set *set = part->set;
    kde_set_reactivate(set);
    KdeRefusal refused;
    if ((rc = kde_set_moment_enqueue(set, pass, &mean, nullptr)) || (rc = kde_set_moment_wait(set, pass, value, lo, hi, &refused.code, &refused.why)))
        return rc;
    return kde_report_one(refused);
}

int garlic_kde_part_rank(garlic_kde_part *part, const uint64_t *keys, int32_t m, int64_t *below)
{
    int rc;
    if ((rc = kde_part_usable(part))) return rc;
    if (m < 1 || m > KDE_RANK_MAX) return fail(GARLIC_ERR_INVALID, "KDE part: %d probe keys (1 to %d)", (int)m, KDE_RANK_MAX);
    if (!keys || !below) return fail(GARLIC_ERR_INVALID, "KDE part: keys and below are required");
    garlic_kde_part_set *set = part->set;
    kde_set_reactivate(set);
    if ((rc = kde_set_rank_enqueue(set, keys, m)) || (rc = kde_set_rank_wait(set))) return rc;
    for (int i = 0; i < m; i++) below[i] = set->h_below[i];
    return GARLIC_OK;
}

int garlic_kde_part_sums(garlic_kde_part *part, const double *targets, double h, double *sums)
{
    int rc;
    if ((rc = kde_part_usable(part))) return rc;
    if (!targets || !sums) return fail(GARLIC_ERR_INVALID, "KDE part: targets and sums are required");
    const double inv_h2 = 1.0 / (h * h);
    if (!(h > 0) || !std::isfinite(inv_h2)) return fail(GARLIC_ERR_INVALID, "feed KDE: bandwidth %g cannot be used (zero, negative, not finite or too small to square)", h);
    garlic_kde_part_set *set = part->set;
    kde_set_reactivate(set);
    if ((rc = kde_set_sums_enqueue(set, targets, &inv_h2, nullptr)) || (rc = kde_set_sums_wait(set))) return rc;
    kde_part_note_sums(part);
    memcpy(sums, set->h_table[0].raw, sizeof(double) * KDE_POINTS);
    return GARLIC_OK;
}

int garlic_kde_parts(garlic_kde_part *const *parts, int32_t n_parts, garlic_kde *out)
{
    if (!parts || !out) return fail(GARLIC_ERR_INVALID, "KDE parts: parts and out are required");
    if (n_parts < 1 || n_parts > GARLIC_KDE_MAX_PARTS) return fail(GARLIC_ERR_INVALID, "KDE parts: %d parts (1 to %d)", (int)n_parts, GARLIC_KDE_MAX_PARTS);
    int rc;
    garlic_kde_part_set *sets[GARLIC_KDE_MAX_PARTS];
    for (int p = 0; p < n_parts; p++) {
        if (!parts[p]) return fail(GARLIC_ERR_INVALID, "KDE parts: part %d is NULL", p);
        for (int q = 0; q < p; q++)
            if (parts[q] == parts[p]) return fail(GARLIC_ERR_INVALID, "KDE parts: part %d is part %d again", p, q);
        if ((rc = kde_part_usable(parts[p]))) return rc;
        sets[p] = parts[p]->set;
    }
    KdeRefusal refused;
    if ((rc = kde_parts_reduce(sets, n_parts, true, out, &refused))) return rc;
    if (refused.code) return kde_report_one(refused);
    for (int p = 0; p < n_parts; p++) {
        kde_part_note_sums(parts[p]);
        parts[p]->rank_rounds = sets[p]->rank_rounds;
    }
    return GARLIC_OK;
}

int garlic_kde_parts_info(garlic_kde_part *const *parts, int32_t n_parts, int64_t *chunks, int64_t *pairs_skipped, int32_t *rank_rounds,
                          float *sums_ms)
{
    if (!parts) return fail(GARLIC_ERR_INVALID, "KDE parts: parts is NULL");
    if (n_parts < 1 || n_parts > GARLIC_KDE_MAX_PARTS) return fail(GARLIC_ERR_INVALID, "KDE parts: %d parts (1 to %d)", (int)n_parts, GARLIC_KDE_MAX_PARTS);
    for (int p = 0; p < n_parts; p++) {
        if (!parts[p]) return fail(GARLIC_ERR_INVALID, "KDE parts: part %d is NULL", p);
        const int rc = kde_part_usable(parts[p]);
        if (rc) return rc;
        if (chunks) chunks[p] = parts[p]->chunks;
        if (pairs_skipped) pairs_skipped[p] = parts[p]->pairs_skipped;
        if (sums_ms) sums_ms[p] = parts[p]->sums_ms;
    }
    if (rank_rounds) *rank_rounds = parts[0]->rank_rounds;
    return GARLIC_OK;
}

// ---- GMM::estimate on the device (gmm_kernels.hpp).  One update is a pass over the points and the finish that turns the
// blocks' partial sums into the next parameters (one launch when the pass is a single workgroup).  The host enqueues
// GMM_BATCH updates at a time and reads the state once per batch: every kernel behind the update that met the stop rule
// returns at once, so a batch costs no blocking round trip per iteration and at most GMM_BATCH - 1 empty updates.
int garlic_gmm_fit(garlic_ctx *ctx, const double *x, int64_t n, int32_t where, int32_t k, const double *a0, const double *mean0,
                   const double *var0, int32_t max_iter, double precision, garlic_gmm *out)
{
    static_assert(GMM_MAX_K == GARLIC_GMM_MAX_K, "one K limit");
    if (!ctx || !out || !x || !a0 || !mean0 || !var0) return fail(GARLIC_ERR_INVALID, "GMM fit: context, values, initial parameters and out are required");
    if (where != GARLIC_HOST && where != GARLIC_DEVICE) return fail(GARLIC_ERR_INVALID, "GMM fit: where must be GARLIC_HOST or GARLIC_DEVICE");
    if (n < 1) return fail(GARLIC_ERR_INVALID, "GMM fit: needs at least 1 value (got %lld)", (long long)n);
    if (k < 1 || k > GARLIC_GMM_MAX_K) return fail(GARLIC_ERR_INVALID, "GMM fit: %d Gaussians (1 to %d)", (int)k, GARLIC_GMM_MAX_K);
    if (max_iter < 1) return fail(GARLIC_ERR_INVALID, "GMM fit: max_iter must be at least 1 (got %d)", (int)max_iter);
    const int64_t n_blocks = (n + GMM_BLOCK_POINTS - 1) / GMM_BLOCK_POINTS;
    if (n_blocks > 0x7fffffff) return fail(GARLIC_ERR_INVALID, "GMM fit: %lld values are more blocks than one launch holds", (long long)n);
    int rc;
    if ((rc = set_device(ctx))) return rc;
    GmmScratch &g = ctx->gmm;
    if ((where == GARLIC_HOST && (rc = g.stage.reserve((size_t)n))) || (rc = g.partial.reserve((size_t)n_blocks * 2 * (3 * (size_t)k + 1))) ||
        (rc = g.state.reserve(1)))
        return rc;
    for (auto &e : g.ev)
        if (!e) HIP_TRY(hipEventCreate(&e));
    hipStream_t s = ctx->stream;
    const double *d_x = x;
    if (where == GARLIC_HOST) {
        HIP_TRY(hipMemcpyAsync(g.stage.p, x, sizeof(double) * (size_t)n, hipMemcpyHostToDevice, s));
        d_x = g.stage.p;
    }
    GmmState st;
    memset(&st, 0, sizeof st);
    for (int i = 0; i < k; i++) {
        st.a[i] = a0[i];
        st.mean[i] = mean0[i];
        st.var[i] = var0[i];
    }
    st.loglik = st.prev = -std::numeric_limits<double>::max();   // GMM::GMM, src/gmm.cpp:201-202
    st.bic = std::numeric_limits<double>::max();
    HIP_TRY(hipMemcpyAsync(g.state.p, &st, sizeof st, hipMemcpyHostToDevice, s));
    HIP_TRY(hipStreamSynchronize(s));              // st is written below
    const double log_n = log((double)n);
    HIP_TRY(hipEventRecord(g.ev[0], s));
    for (int done = 0; done < max_iter && !st.converged;) {
        const int updates = std::min<int>(GMM_BATCH, max_iter - done);
        switch (k) {
        case 1: gmm_enqueue<1>(s, d_x, n, n_blocks, log_n, precision, g.state.p, g.partial.p, updates); break;
        case 2: gmm_enqueue<2>(s, d_x, n, n_blocks, log_n, precision, g.state.p, g.partial.p, updates); break;
        case 3: gmm_enqueue<3>(s, d_x, n, n_blocks, log_n, precision, g.state.p, g.partial.p, updates); break;
        case 4: gmm_enqueue<4>(s, d_x, n, n_blocks, log_n, precision, g.state.p, g.partial.p, updates); break;
        case 5: gmm_enqueue<5>(s, d_x, n, n_blocks, log_n, precision, g.state.p, g.partial.p, updates); break;
        case 6: gmm_enqueue<6>(s, d_x, n, n_blocks, log_n, precision, g.state.p, g.partial.p, updates); break;
        case 7: gmm_enqueue<7>(s, d_x, n, n_blocks, log_n, precision, g.state.p, g.partial.p, updates); break;
        default: gmm_enqueue<8>(s, d_x, n, n_blocks, log_n, precision, g.state.p, g.partial.p, updates); break;
        }
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(&st, g.state.p, sizeof st, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        done += updates;
    }
    HIP_TRY(hipEventRecord(g.ev[1], s));
    HIP_TRY(hipEventSynchronize(g.ev[1]));
    garlic_gmm r;
    memset(&r, 0, sizeof r);
    r.k = k;
    r.iterations = st.iterations;
    r.converged = st.converged;
    for (int i = 0; i < k; i++) {
        r.a[i] = st.a[i];
        r.mean[i] = st.mean[i];
        r.var[i] = st.var[i];
    }
    r.loglik = st.loglik;
    r.bic = st.bic;
    ctx->gmm_blocks = n_blocks;
    if (hipEventElapsedTime(&ctx->gmm_em_ms, g.ev[0], g.ev[1]) != hipSuccess) ctx->gmm_em_ms = 0.f;
    *out = r;
    return GARLIC_OK;
}

int garlic_gmm_fit_info(garlic_ctx *ctx, int64_t *blocks, int64_t *scratch_bytes, float *em_ms)
{
    if (!ctx) return fail(GARLIC_ERR_INVALID, "context is NULL");
    if (blocks) *blocks = ctx->gmm_blocks;
    if (scratch_bytes) *scratch_bytes = (int64_t)ctx->gmm.bytes();
    if (em_ms) *em_ms = ctx->gmm_em_ms;
    return GARLIC_OK;
}

// ---- count_features_in_roh.pl on the device (feature_kernels.hpp).  A feature set holds the hom rows of the annotated
// alleles block-major, with the rows' chromosome, position and effect; a call brings one list of classified intervals and
// counts.  The intervals and their per-individual offsets travel through a pinned block of the set's, so the call enqueues
// and returns: the only wait is for the previous call's upload out of that block (an event), never for the stream.
struct garlic_feature_set {
    garlic_ctx *ctx = nullptr;
    int64_t nrows = 0;
    int32_t nind = 0, nblk = 0;
    bool have_sites = false;
    int32_t max_effect = -1;
    DevBuf<uint64_t> bits;                         // [blk][row]
    DevBuf<int32_t> chr, pos, eff;
    DevBuf<FeatInterval> iv;
    DevBuf<int32_t> off;
    DevBuf<unsigned long long> counts, skipped;
    void *pinned = nullptr;                        // intervals, then offsets
    size_t pinned_bytes = 0;
    hipEvent_t uploaded = nullptr, ev[2] = {};
    bool upload_pending = false, timed = false;
    int64_t blocks = 0, chunks = 0, launches = 0;
};

static void feature_set_free(garlic_feature_set *fs)
{
    if (fs->uploaded) (void)hipEventDestroy(fs->uploaded);
    for (auto &e : fs->ev)
        if (e) (void)hipEventDestroy(e);
    if (fs->pinned) (void)hipHostFree(fs->pinned);
    delete fs;
}

int garlic_feature_set_create(garlic_ctx *ctx, int64_t nrows, int32_t nind, garlic_feature_set **out)
{
    static_assert(sizeof(FeatInterval) == sizeof(garlic_roh_interval) && FEAT_MAX_EFFECTS == GARLIC_FEATURE_MAX_EFFECTS &&
                  FEAT_MAX_CLASSES == GARLIC_GMM_MAX_K, "one interval, one set of limits");
    if (!ctx || !out) return fail(GARLIC_ERR_INVALID, "feature set: context and set are required");
    if (nrows < 0 || nind < 1) return fail(GARLIC_ERR_INVALID, "feature set: %lld rows, %d individuals (>= 0 and >= 1)", (long long)nrows, (int)nind);
    const int64_t nblk = ((int64_t)nind + WAVE - 1) / WAVE, n_chunks = (nrows + FEAT_CHUNK_ROWS - 1) / FEAT_CHUNK_ROWS;
    if (nblk * n_chunks > 0x7fffffff) return fail(GARLIC_ERR_INVALID, "feature set: %lld rows x %d individuals are more wavefronts than one launch holds", (long long)nrows, (int)nind);
    int rc;
    if ((rc = set_device(ctx))) return rc;
    std::unique_ptr<garlic_feature_set, void (*)(garlic_feature_set *)> fs(new garlic_feature_set, feature_set_free);
    fs->ctx = ctx;
    fs->nrows = nrows;
    fs->nind = nind;
    fs->nblk = (int32_t)nblk;
    const size_t rows = (size_t)std::max<int64_t>(nrows, 1);
    if ((rc = fs->bits.reserve(rows * (size_t)nblk)) || (rc = fs->chr.reserve(rows)) || (rc = fs->pos.reserve(rows)) || (rc = fs->eff.reserve(rows)) ||
        (rc = fs->off.reserve((size_t)nind + 1)) || (rc = fs->skipped.reserve(1)))
        return rc;
    HIP_TRY(hipEventCreateWithFlags(&fs->uploaded, hipEventDisableTiming));
    for (auto &e : fs->ev) HIP_TRY(hipEventCreate(&e));
    HIP_TRY(hipMemsetAsync(fs->bits.p, 0, sizeof(uint64_t) * rows * (size_t)nblk, ctx->stream));    // rows never set hold no homozygote
    *out = fs.release();
    return GARLIC_OK;
}

int garlic_feature_set_destroy(garlic_feature_set *fs)
{
    if (!fs) return GARLIC_OK;
    (void)hipSetDevice(fs->ctx->device);
    (void)hipStreamSynchronize(fs->ctx->stream);
    feature_set_free(fs);
    return GARLIC_OK;
}

int garlic_feature_set_rows(garlic_feature_set *fs, const uint8_t *bits, int64_t row_bytes, int64_t row_begin, int64_t row_count)
{
    if (!fs || !bits) return fail(GARLIC_ERR_INVALID, "feature set and rows are required");
    if (row_bytes < ((int64_t)fs->nind + 7) / 8) return fail(GARLIC_ERR_INVALID, "row_bytes %lld < %d bits", (long long)row_bytes, fs->nind);
    if (row_begin < 0 || row_count < 1 || row_begin + row_count > fs->nrows)
        return fail(GARLIC_ERR_INVALID, "row range [%lld,+%lld) outside feature set of %lld rows", (long long)row_begin, (long long)row_count, (long long)fs->nrows);
    int rc;
    if ((rc = set_device(fs->ctx))) return rc;
    hipStream_t s = fs->ctx->stream;
    DevBuf<uint8_t> stage;
    return for_each_upload_slab(s, "feature_set_rows", bits, row_bytes, row_count, GARLIC_HOST, stage, [&](const void *src, int64_t at, int64_t n) {
        hipLaunchKernelGGL(phase_bits_planes_kernel, dim3((unsigned)((n + WAVE - 1) / WAVE)), dim3(256), 0, s, (const uint8_t *)src, row_bytes,
                           row_begin + at, n, fs->nind, fs->nblk, fs->nrows, fs->bits.p);
        return GARLIC_OK;
    });
}

// the same rows from a .bed image on the set's device (bed_hom_rows_kernel): the plan's two lists are the only host bytes
int garlic_feature_set_rows_bed(garlic_feature_set *fs, garlic_bed *b, const int64_t *file_row, const uint8_t *allele, int64_t row_begin,
                                int64_t row_count)
{
    if (!fs || !b) return fail(GARLIC_ERR_INVALID, "feature set rows from a bed image: set and image are required");
    if (row_count > 0 && (!file_row || !allele)) return fail(GARLIC_ERR_INVALID, "feature set rows from a bed image: file_row and allele are required");
    if (fs->nind != b->nind)
        return fail(GARLIC_ERR_INVALID, "the feature set has %d individuals, the bed image %d", fs->nind, b->nind);
    if (b->ctx->device != fs->ctx->device)
        return fail(GARLIC_ERR_INVALID, "the bed image is on device %d, the feature set on device %d", b->ctx->device, fs->ctx->device);
    if (row_begin < 0 || row_count < 0 || row_begin + row_count > fs->nrows)
        return fail(GARLIC_ERR_INVALID, "row range [%lld,+%lld) outside feature set of %lld rows", (long long)row_begin, (long long)row_count, (long long)fs->nrows);
    if (b->n_set != b->nrows)
        return fail(GARLIC_ERR_STATE, "feature set rows need every row of the bed image: %lld of %lld set", (long long)b->n_set, (long long)b->nrows);
    for (int64_t k = 0; k < row_count; k++) {
        if (file_row[k] < 0 || file_row[k] >= b->nrows)
            return fail(GARLIC_ERR_INVALID, "file_row[%lld] = %lld outside the image's %lld rows", (long long)k, (long long)file_row[k], (long long)b->nrows);
        if (allele[k] > 2) return fail(GARLIC_ERR_INVALID, "allele[%lld] = %d (0 = hom A1, 1 = hom A2, 2 = none)", (long long)k, (int)allele[k]);
    }
    if (row_count == 0) return GARLIC_OK;
    int rc;
    if ((rc = set_device(fs->ctx))) return rc;
    hipStream_t s = fs->ctx->stream;      // (every call that writes the image has waited for its own stream before it returned)
    DevBuf<int64_t> d_row;
    DevBuf<uint8_t> d_allele;
    if ((rc = d_row.reserve((size_t)row_count)) || (rc = d_allele.reserve((size_t)row_count))) return rc;
    HIP_TRY(hipMemcpyAsync(d_row.p, file_row, sizeof(int64_t) * (size_t)row_count, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(d_allele.p, allele, (size_t)row_count, hipMemcpyHostToDevice, s));
    const int64_t ngroups = ((int64_t)fs->nblk + BED_HOM_BLOCKS - 1) / BED_HOM_BLOCKS;
    const int64_t nitems = ((row_count + WAVE - 1) / WAVE) * ngroups;
    const unsigned grid = (unsigned)std::min<int64_t>((nitems + 3) / 4, 8 * (int64_t)fs->ctx->n_cu);
    hipLaunchKernelGGL(bed_hom_rows_kernel, dim3(grid), dim3(256), 0, s, b->d_image.p, b->image_bytes, b->row_bytes, b->nind, d_row.p,
                       d_allele.p, row_begin, row_count, fs->nrows, fs->nblk, fs->bits.p);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(s));      // the two lists are free again; the image may go
    return GARLIC_OK;
}

int garlic_feature_set_get_rows(garlic_feature_set *fs, int64_t row_begin, int64_t row_count, uint8_t *bits, int64_t row_bytes)
{
    if (!fs) return fail(GARLIC_ERR_INVALID, "feature set is NULL");
    if (row_count > 0 && !bits) return fail(GARLIC_ERR_INVALID, "feature set get_rows: bits is NULL");
    const int64_t own = ((int64_t)fs->nind + 7) / 8;
    if (row_bytes < own) return fail(GARLIC_ERR_INVALID, "row_bytes %lld < %d bits", (long long)row_bytes, fs->nind);
    if (row_begin < 0 || row_count < 0 || row_begin + row_count > fs->nrows)
        return fail(GARLIC_ERR_INVALID, "row range [%lld,+%lld) outside feature set of %lld rows", (long long)row_begin, (long long)row_count, (long long)fs->nrows);
    int rc;
    if ((rc = set_device(fs->ctx))) return rc;
    hipStream_t s = fs->ctx->stream;
    if (row_count == 0) {
        HIP_TRY(hipStreamSynchronize(s));
        return GARLIC_OK;
    }
    // the words [blk][row] of the range, then the transpose into byte rows on the host (a door for checks, not a hot path)
    std::vector<uint64_t> words((size_t)fs->nblk * (size_t)row_count);
    HIP_TRY(hipMemcpy2DAsync(words.data(), sizeof(uint64_t) * (size_t)row_count, fs->bits.p + row_begin, sizeof(uint64_t) * (size_t)fs->nrows,
                             sizeof(uint64_t) * (size_t)row_count, (size_t)fs->nblk, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    for (int64_t r = 0; r < row_count; r++)
        for (int64_t blk = 0; blk < fs->nblk; blk++) {
            const uint64_t w = words[(size_t)(blk * row_count + r)];
            const int64_t n = std::min<int64_t>(8, own - 8 * blk);
            for (int64_t t = 0; t < n; t++) bits[r * row_bytes + 8 * blk + t] = (uint8_t)(w >> (8 * t));
        }
    return GARLIC_OK;
}

int garlic_feature_set_sites(garlic_feature_set *fs, const int32_t *chr, const int32_t *pos, const int32_t *effect)
{
    if (!fs) return fail(GARLIC_ERR_INVALID, "feature set is NULL");
    if (fs->nrows > 0 && (!chr || !pos || !effect)) return fail(GARLIC_ERR_INVALID, "feature set: chr, pos and effect are required");
    int32_t max_effect = -1;
    for (int64_t r = 0; r < fs->nrows; r++) {
        if (chr[r] < 0 || effect[r] < 0 || effect[r] >= GARLIC_FEATURE_MAX_EFFECTS)
            return fail(GARLIC_ERR_INVALID, "feature set: row %lld has chromosome %d, effect %d (chromosome >= 0, effect in [0, %d))", (long long)r,
                        (int)chr[r], (int)effect[r], GARLIC_FEATURE_MAX_EFFECTS);
        if (r && (chr[r] < chr[r - 1] || (chr[r] == chr[r - 1] && pos[r] < pos[r - 1])))
            return fail(GARLIC_ERR_INVALID, "feature set: rows are not sorted by (chromosome, position) at row %lld", (long long)r);
        max_effect = std::max(max_effect, effect[r]);
    }
    int rc;
    if ((rc = set_device(fs->ctx))) return rc;
    hipStream_t s = fs->ctx->stream;
    if (fs->nrows > 0) {
        const size_t bytes = sizeof(int32_t) * (size_t)fs->nrows;
        HIP_TRY(hipMemcpyAsync(fs->chr.p, chr, bytes, hipMemcpyHostToDevice, s));
        HIP_TRY(hipMemcpyAsync(fs->pos.p, pos, bytes, hipMemcpyHostToDevice, s));
        HIP_TRY(hipMemcpyAsync(fs->eff.p, effect, bytes, hipMemcpyHostToDevice, s));
        HIP_TRY(hipStreamSynchronize(s));          // the caller's arrays are free on return
    }
    fs->max_effect = max_effect;
    fs->have_sites = true;
    return GARLIC_OK;
}

int garlic_feature_counts(garlic_feature_set *fs, const garlic_roh_interval *intervals, int64_t n_intervals, int32_t n_classes,
                          int32_t n_effects, int64_t *counts, int32_t where)
{
    if (!fs || !counts) return fail(GARLIC_ERR_INVALID, "feature counts: set and counts are required");
    if (where != GARLIC_HOST && where != GARLIC_DEVICE) return fail(GARLIC_ERR_INVALID, "feature counts: where must be GARLIC_HOST or GARLIC_DEVICE");
    if (n_intervals < 0 || n_intervals > 0x7fffffff || (n_intervals > 0 && !intervals))
        return fail(GARLIC_ERR_INVALID, "feature counts: %lld intervals (0 to 2^31 - 1, with a list)", (long long)n_intervals);
    if (n_classes < 1 || n_classes > GARLIC_GMM_MAX_K) return fail(GARLIC_ERR_INVALID, "feature counts: %d classes (1 to %d)", (int)n_classes, GARLIC_GMM_MAX_K);
    if (n_effects < 1 || n_effects > GARLIC_FEATURE_MAX_EFFECTS)
        return fail(GARLIC_ERR_INVALID, "feature counts: %d effects (1 to %d)", (int)n_effects, GARLIC_FEATURE_MAX_EFFECTS);
    if (!fs->have_sites) return fail(GARLIC_ERR_STATE, "feature counts: the set needs garlic_feature_set_sites first");
    if (fs->max_effect >= n_effects) return fail(GARLIC_ERR_INVALID, "feature counts: a row has effect %d, n_effects is %d", (int)fs->max_effect, (int)n_effects);
    for (int64_t i = 0; i < n_intervals; i++) {
        const garlic_roh_interval &v = intervals[i];
        if (v.ind < 0 || v.ind >= fs->nind) return fail(GARLIC_ERR_INVALID, "feature counts: interval %lld has individual %d (0 to %d)", (long long)i, (int)v.ind, fs->nind - 1);
        if (v.cls < 0 || v.cls >= n_classes) return fail(GARLIC_ERR_INVALID, "feature counts: interval %lld has class %d (0 to %d)", (long long)i, (int)v.cls, n_classes - 1);
        if (v.chr < 0 || v.stop < v.start) return fail(GARLIC_ERR_INVALID, "feature counts: interval %lld has chromosome %d, [%d, %d)", (long long)i, (int)v.chr, (int)v.start, (int)v.stop);
        if (!i) continue;
        const garlic_roh_interval &u = intervals[i - 1];
        if (v.ind < u.ind || (v.ind == u.ind && (v.chr < u.chr || (v.chr == u.chr && v.start < u.start))))
            return fail(GARLIC_ERR_INVALID, "feature counts: intervals are not ordered by (individual, chromosome, start) at interval %lld", (long long)i);
        if (v.ind == u.ind && v.chr == u.chr && v.start < u.stop)
            return fail(GARLIC_ERR_INVALID, "feature counts: interval %lld overlaps the one before it", (long long)i);
    }
    int rc;
    if ((rc = set_device(fs->ctx))) return rc;
    hipStream_t s = fs->ctx->stream;
    // the pinned block: free again once the previous call's copies out of it have run
    if (fs->upload_pending) HIP_TRY(hipEventSynchronize(fs->uploaded));
    fs->upload_pending = false;
    const size_t iv_bytes = sizeof(FeatInterval) * (size_t)n_intervals, off_bytes = sizeof(int32_t) * ((size_t)fs->nind + 1);
    const size_t off_at = (iv_bytes + 15) & ~(size_t)15, need = off_at + off_bytes;
    if (need > fs->pinned_bytes) {
        if (fs->pinned) HIP_TRY(hipHostFree(fs->pinned));
        fs->pinned = nullptr;
        fs->pinned_bytes = 0;
        HIP_TRY(hipHostMalloc(&fs->pinned, need + need / 2, hipHostMallocDefault));
        fs->pinned_bytes = need + need / 2;
    }
    const size_t n_counts = (size_t)fs->nind * (size_t)(n_classes + 1) * (size_t)n_effects;
    if ((rc = fs->iv.reserve(std::max<size_t>((size_t)n_intervals, 1))) || (where == GARLIC_HOST && (rc = fs->counts.reserve(n_counts)))) return rc;
    uint8_t *pin = (uint8_t *)fs->pinned;
    if (n_intervals) memcpy(pin, intervals, iv_bytes);
    int32_t *off = (int32_t *)(pin + off_at);
    {
        int64_t i = 0;
        for (int32_t ind = 0; ind <= fs->nind; ind++) {
            while (i < n_intervals && intervals[i].ind < ind) i++;
            off[ind] = (int32_t)i;
        }
    }
    if (n_intervals) HIP_TRY(hipMemcpyAsync(fs->iv.p, pin, iv_bytes, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(fs->off.p, off, off_bytes, hipMemcpyHostToDevice, s));
    HIP_TRY(hipEventRecord(fs->uploaded, s));
    fs->upload_pending = true;
    unsigned long long *d_counts = where == GARLIC_HOST ? fs->counts.p : (unsigned long long *)counts;
    HIP_TRY(hipMemsetAsync(d_counts, 0, sizeof(unsigned long long) * n_counts, s));
    HIP_TRY(hipMemsetAsync(fs->skipped.p, 0, sizeof(unsigned long long), s));
    const int64_t n_chunks = (fs->nrows + FEAT_CHUNK_ROWS - 1) / FEAT_CHUNK_ROWS;
    int64_t launches = 0;
    HIP_TRY(hipEventRecord(fs->ev[0], s));
    if (n_chunks > 0)
        for (int e0 = 0; e0 <= fs->max_effect; e0 += FEAT_GROUP_EFFECTS, launches++) {
            const int ge = std::min<int>(FEAT_GROUP_EFFECTS, n_effects - e0);
            const size_t lds = feature_counts_lds(n_classes, ge);
            if (lds > LDS_DEFAULT_MAX) HIP_TRY(hipFuncSetAttribute((const void *)feature_counts_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
            hipLaunchKernelGGL(feature_counts_kernel, dim3((unsigned)(n_chunks * fs->nblk)), dim3(WAVE), lds, s, fs->bits.p, fs->chr.p, fs->pos.p,
                               fs->eff.p, fs->nrows, fs->nind, n_chunks, fs->iv.p, fs->off.p, (int)n_classes, (int)n_effects, e0, ge, d_counts,
                               e0 == 0 ? fs->skipped.p : nullptr);        // zero words are counted once, not once per launch
            HIP_TRY(hipGetLastError());
        }
    HIP_TRY(hipEventRecord(fs->ev[1], s));
    fs->timed = true;
    fs->blocks = fs->nblk;
    fs->chunks = n_chunks;
    fs->launches = launches;
    if (where == GARLIC_HOST) {
        HIP_TRY(hipMemcpyAsync(counts, fs->counts.p, sizeof(int64_t) * n_counts, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
    }
    return GARLIC_OK;
}

int garlic_feature_counts_info(garlic_feature_set *fs, int64_t *blocks, int64_t *chunks, int64_t *words_skipped, float *kernel_ms)
{
    if (!fs) return fail(GARLIC_ERR_INVALID, "feature set is NULL");
    if (blocks) *blocks = fs->blocks;
    if (chunks) *chunks = fs->chunks;
    if (!words_skipped && !kernel_ms) return GARLIC_OK;
    int rc;
    if ((rc = set_device(fs->ctx))) return rc;
    unsigned long long skipped = 0;
    float ms = 0.f;
    if (fs->timed) {                               // waits for the last call's kernels
        HIP_TRY(hipMemcpyAsync(&skipped, fs->skipped.p, sizeof skipped, hipMemcpyDeviceToHost, fs->ctx->stream));
        HIP_TRY(hipStreamSynchronize(fs->ctx->stream));
        if (hipEventElapsedTime(&ms, fs->ev[0], fs->ev[1]) != hipSuccess) ms = 0.f;
    }
    if (words_skipped) *words_skipped = (int64_t)skipped;
    if (kernel_ms) *kernel_ms = ms;
    return GARLIC_OK;
}

int garlic_lod_feed_info(garlic_panel *p, int32_t *form, int64_t *score_doubles)
{
    if (!p || !form) return fail(GARLIC_ERR_INVALID, "panel and form are required");
    *form = p->last_feed_form;
    if (score_doubles) *score_doubles = p->last_feed_doubles;
    return GARLIC_OK;
}

int garlic_panel_chain_kind(garlic_panel *p, int32_t *kind)
{
    if (!p || !kind) return fail(GARLIC_ERR_INVALID, "panel and kind are required");
    *kind = p->last_chain_kind;
    return GARLIC_OK;
}

int garlic_ctx_set_async(garlic_ctx *ctx, int32_t on)
{
    if (!ctx) return fail(GARLIC_ERR_INVALID, "ctx is NULL");
    ctx->async_device = on != 0;
    return GARLIC_OK;
}

} // extern "C"
