"""GPU: every kernel form at the window widths and term values that select it, bit for bit against the oracle.

The dispatcher (garlic_amd/csrc/garlic_hip.hip) switches kernel forms at fixed widths, several of them at widths
the other files do not reach; tests/test_window_regimes_cpu.py reads the switch points from the headers and
checks that each one is tested here on both sides:

  * TGLS chain (lod_chain_ring_kernel): one stream up to TG_SINGLE_MAX_W = 144, the two-stream form above
    (two 120-row ring halves: the wrapping read runs), for scores and for coverage bits; an individual range
    that is not block-aligned takes lod_chain_terms_kernel;
  * unweighted coverage bits (lod_bits_kernel) up to COVF_MAX_W = 1024, scores + counts above;
  * weighted bits and scores: the strip kernels up to 113 / 241 (WS_WAVES / WS_WAVES_WIDE compute waves), the GL
    ring form of the tile kernel above, the plain two-block tile kernel at every width;
  * terms that are not all finite (--error 0, a NaN frequency): the feed's and the coverage's fall-backs, and
    the chains carrying -inf / NaN (x86's NaN, sign bit set) through their rolling sums.
"""
import numpy as np
import pytest

import oracle_lib as ol
from garlic_amd import abi

pytestmark = pytest.mark.gpu
MG = 200000

# the widths each form is tested at (tests/test_window_regimes_cpu.py pins them to the source's switch points)
TGLS_WIDTHS = [143, 144, 145, 146, 200, 240, 241, 500, 1500]
TGLS_BITS_WIDTHS = [144, 145, 200, 500]
UNWEIGHTED_BITS_WIDTHS = [300, 513, 1000, 1024, 1025, 1100]
WEIGHTED_WIDTHS = [113, 114, 200, 241, 242, 300, 1000]
NONFINITE_WIDTHS = [5, 60, 300]


def chrom_sizes(W, big=None):
    """1, W-1, W, W+1, W+33, one of a few thousand SNPs (gaps and a centromere), one not a multiple of 32"""
    odd = W + 777 if (W + 777) % 32 else W + 778
    return [1, W - 1, W, W + 1, W + 33, big or max(3000, 3 * W), odd]


def make_chroms(rng, sizes, nind, big_idx=5):
    """gaps and a centromere in the big chromosome, a centromere in the ones behind it, the short ones whole"""
    return [ol.random_panel(rng, n, nind, max_gap=MG, gaps=3 if k == big_idx else 0, centro=k >= big_idx)
            for k, n in enumerate(sizes)]


def open_panel(ctx, chroms, nind, gpos=None):
    panel = abi.Panel(ctx, [c[0].shape[0] for c in chroms], nind)
    panel.set_map(np.concatenate([c[2] for c in chroms]), [c[3] for c in chroms], [c[4] for c in chroms],
                  gpos=None if gpos is None else np.concatenate(gpos))
    panel.set_freq(np.concatenate([c[1] for c in chroms]))
    panel.set_genotypes(np.concatenate([c[0] for c in chroms], axis=0))
    return panel


def device_rows(panel, sizes, nind, pitch_align, launch):
    """launch(out_ptr) writes scores into a device buffer of out_layout(pitch_align, nind): per-chromosome rows"""
    import torch
    base, pitch, total = panel.out_layout(pitch_align, nind)
    out = torch.full((int(total),), 12345.0, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    launch(out.data_ptr())
    panel.ctx.synchronize()
    host = out.cpu().numpy()
    return [host[base[c]: base[c] + nind * pitch[c]].reshape(nind, pitch[c])[:, :n] for c, n in enumerate(sizes)]


def assert_scores(got, want, what):
    for c in range(len(want)):
        g = np.ascontiguousarray(got[c])
        assert ol.bits_equal(g, want[c]), (what, c, ol.count_mismatch(g, want[c]) if g.shape == want[c].shape else g.shape)


def cutoffs_of(scores, qs=(0.1, 0.5, 0.9)):
    """cutoffs equal to scores that occur (the >= at its edge): low ones make long ROH, high ones short ones"""
    v = np.concatenate([s.ravel() for s in scores])
    v = np.sort(v[np.isfinite(v) & (v != ol.MISSING)])
    if v.shape[0] == 0:
        return [0.0] * len(qs)
    return [float(v[int(q * (v.shape[0] - 1))]) for q in qs]


def oracle_segments(chroms, scores, W, cutoff, frac):
    """the oracle's scores through the oracle's inWin[] loop and segment walk -> [(individual, chromosome, first, last)]"""
    out = []
    for c, (g, f, p, cs, ce) in enumerate(chroms):
        cov = ol.oracle_roh_coverage(np.ascontiguousarray(scores[c]), W, cutoff)
        out += [(i, c, a, b) for i, a, b in ol.oracle_roh_segments(cov, p, cs, ce, W, MG, frac)]
    return sorted(out)


def check_coverage(panel, chroms, scores, W, cutoff, pitch_align, what, **kw):
    got = panel.roh_coverage_fused(W, kw.pop("error", 0.001), MG, cutoff, pitch_align=pitch_align, **kw)
    covered = 0
    for c, (g, f, p, cs, ce) in enumerate(chroms):
        n = g.shape[0]
        want = ol.oracle_roh_coverage(np.ascontiguousarray(scores[c]), W, cutoff)
        assert np.array_equal(got[c][:, :n], want), (what, W, cutoff, pitch_align, c)
        covered += int(np.count_nonzero(want))
    return covered


def check_segments(panel, chroms, scores, W, cutoff, frac, what, **kw):
    want = oracle_segments(chroms, scores, W, cutoff, frac)
    got = panel.roh_segments(W, kw.pop("error", 0.001), MG, cutoff, frac, **kw)
    assert [tuple(int(v) for v in r) for r in got] == want, (what, W, cutoff, frac, len(got), len(want))
    return len(want)


# ------------------------------------------------------------------------------------------------ TGLS scores

@pytest.mark.parametrize("W", TGLS_WIDTHS)
def test_tgls_scores_across_the_two_stream_switch(gpu_ctx, W):
    """unweighted scores with likelihoods (dictionary and continuous): host and device output, dense and padded rows,
    an aligned sub-range (the ring chain) and an unaligned one (lod_chain_terms_kernel)"""
    rng = np.random.default_rng(3000 + W)
    nind = 130 if W % 2 else 70
    sizes = chrom_sizes(W)
    chroms = make_chroms(rng, sizes, nind)
    for kind in ("dictionary", "continuous"):
        err = [rng.choice([1e-16, 1e-3, 0.01, 0.2, 1.0], size=c[0].shape) if kind == "dictionary"
               else rng.uniform(1e-4, 0.5, size=c[0].shape) for c in chroms]
        want = [ol.oracle_calc_lod(g, f, p, cs, ce, W, 0.001, MG, gl=err[c], threads=8)
                for c, (g, f, p, cs, ce) in enumerate(chroms)]
        assert sum(int(np.count_nonzero(w != ol.MISSING)) for w in want) > 1000
        with open_panel(gpu_ctx, chroms, nind) as panel:
            allerr = np.concatenate(err, axis=0)
            if W == 200:                                  # uploaded in slabs that cut chromosomes
                for l0 in range(0, allerr.shape[0], 700):
                    panel.set_gl(allerr[l0:l0 + 700], locus_begin=l0)
            else:
                panel.set_gl(allerr)
            assert panel.tgls_mode()[0] == (1 if kind == "dictionary" else 2)
            for pa in (1, 32):
                assert_scores(panel.lod_windows(W, 0.001, MG, use_gl=True, pitch_align=pa), want, (kind, "host", pa))
                got = device_rows(panel, sizes, nind, pa,
                                  lambda ptr: panel.lod_windows_device(ptr, W, 0.001, MG, pitch_align=pa, use_gl=True))
                assert_scores(got, want, (kind, "device", pa))
            for i0, cnt in ((64, nind - 64), (37, min(70, nind - 37))):
                got = panel.lod_windows(W, 0.001, MG, use_gl=True, ind_begin=i0, ind_count=cnt, pitch_align=32)
                assert_scores(got, [w[i0:i0 + cnt] for w in want], (kind, "sub-range", i0))


# ------------------------------------------------------------------------------------------------ TGLS bits

@pytest.mark.parametrize("W", TGLS_BITS_WIDTHS)
def test_tgls_coverage_and_segments_across_the_two_stream_switch(gpu_ctx, W):
    """roh_coverage_fused / roh_segments with likelihoods: the ring chain's chain wave stores the bits itself"""
    rng = np.random.default_rng(3100 + W)
    nind = 130 if W % 2 else 70
    chroms = make_chroms(rng, chrom_sizes(W), nind)
    err = [rng.choice([1e-3, 0.01, 0.05, 0.2], size=c[0].shape) if W % 2
           else rng.uniform(1e-3, 0.3, size=c[0].shape) for c in chroms]
    scores = [ol.oracle_calc_lod(g, f, p, cs, ce, W, 0.001, MG, gl=err[c], threads=8) for c, (g, f, p, cs, ce) in enumerate(chroms)]
    cuts = cutoffs_of(scores)
    with open_panel(gpu_ctx, chroms, nind) as panel:
        panel.set_gl(np.concatenate(err, axis=0))
        covered = segs = 0
        for cutoff, pa in zip(cuts, (1, 8, 32)):
            covered += check_coverage(panel, chroms, scores, W, cutoff, pa, "tgls", use_gl=True)
        for cutoff in cuts[:2]:
            for frac in (1e-9, 0.25, 0.6, 1.0):
                segs += check_segments(panel, chroms, scores, W, cutoff, frac, "tgls", use_gl=True)
        assert covered > 0 and segs > 0


# ------------------------------------------------------------------------------------------------ unweighted bits

@pytest.mark.parametrize("W", UNWEIGHTED_BITS_WIDTHS)
def test_unweighted_coverage_and_segments_around_covf_max_w(gpu_ctx, W):
    """lod_bits_kernel up to COVF_MAX_W, scores + counts above; at W = 1024 also a chromosome whose runs span
    hundreds of tiles"""
    rng = np.random.default_rng(3200 + W)
    nind = 130 if W % 2 else 70
    sizes = chrom_sizes(W) + ([9000] if W == 1024 else [])
    chroms = make_chroms(rng, sizes, nind)
    if W == 1024:                                          # the long one without gaps or a centromere
        chroms[-1] = ol.random_panel(rng, 9000, nind, max_gap=MG, gaps=0, centro=False)
    scores = [ol.oracle_calc_lod(g, f, p, cs, ce, W, 0.001, MG, threads=8) for (g, f, p, cs, ce) in chroms]
    cuts = cutoffs_of(scores)
    with open_panel(gpu_ctx, chroms, nind) as panel:
        covered = segs = 0
        for cutoff in cuts:
            for pa in (1, 8):
                covered += check_coverage(panel, chroms, scores, W, cutoff, pa, "unweighted")
        for cutoff in cuts[:2]:
            for frac in (1e-9, 0.25, 1.0):
                segs += check_segments(panel, chroms, scores, W, cutoff, frac, "unweighted")
        assert covered > 0 and segs > 0


# ------------------------------------------------------------------------------------------------ weighted

@pytest.mark.parametrize("W", WEIGHTED_WIDTHS)
def test_weighted_bits_and_scores_at_wide_windows(gpu_ctx, W):
    """--weighted coverage and segments, plain (two-block tile kernel) and with likelihoods (strip kernels up to
    241, the GL ring form above); GL-weighted scores, host and device, aligned and unaligned sub-ranges"""
    rng = np.random.default_rng(3300 + W)
    nind = 130 if W % 2 else 70
    sizes = chrom_sizes(W, big=3000)
    chroms = make_chroms(rng, sizes, nind)
    gpos = [np.cumsum(np.diff(c[2], prepend=0) * 1e-6 * rng.uniform(0.8, 1.2, size=c[2].shape[0])) for c in chroms]
    lds = [rng.uniform(1.0, max(2.0, W / 4.0), size=(n, W)) for n in sizes]
    gl = [rng.choice([1e-16, 1e-3, 0.01, 0.2, 1.0], size=c[0].shape) for c in chroms]
    with open_panel(gpu_ctx, chroms, nind, gpos) as panel:
        panel.set_ld(W, np.concatenate(lds, axis=0))
        panel.set_gl(np.concatenate(gl, axis=0))
        for use_gl in (False, True):
            scores = [ol.oracle_calc_wlod(g, f, p, gpos[c], lds[c], cs, ce, W, 0.001, MG, 1e-9, 7,
                                          gl=gl[c] if use_gl else None, threads=8)
                      for c, (g, f, p, cs, ce) in enumerate(chroms)]
            cuts = cutoffs_of(scores)
            covered = segs = 0
            for cutoff, pa in zip(cuts, (1, 8, 8)):
                covered += check_coverage(panel, chroms, scores, W, cutoff, pa, ("weighted", use_gl),
                                          use_gl=use_gl, weighted=True)
            for frac in (1e-9, 0.25, 1.0):
                segs += check_segments(panel, chroms, scores, W, cuts[0], frac, ("weighted", use_gl),
                                       use_gl=use_gl, weighted=True)
            assert covered > 0 and segs > 0
            if not use_gl:
                continue
            for pa in (1, 32):
                assert_scores(panel.wlod_windows(W, 0.001, MG, 7, 1e-9, use_gl=True, pitch_align=pa), scores, ("gl", "host", pa))
                got = device_rows(panel, sizes, nind, pa,
                                  lambda ptr: panel.wlod_windows_device(ptr, W, 0.001, MG, 7, 1e-9, pitch_align=pa, use_gl=True))
                assert_scores(got, scores, ("gl", "device", pa))
            for i0, cnt in ((64, nind - 64), (37, min(70, nind - 37))):
                got = panel.wlod_windows(W, 0.001, MG, 7, 1e-9, use_gl=True, ind_begin=i0, ind_count=cnt, pitch_align=32)
                assert_scores(got, [s[i0:i0 + cnt] for s in scores], ("gl", "sub-range", i0))


# ------------------------------------------------------------------------------------------------ non-finite terms

@pytest.mark.parametrize("W", NONFINITE_WIDTHS)
def test_nonfinite_unweighted_terms(gpu_ctx, W):
    """--error 0 (-inf het terms: -inf - -inf in the rolling sums) and, in a chromosome of its own, a NaN frequency at
    one locus: scores, feeds, coverage and segments (their fall-backs) and wLOD scores carry the reference's
    infinities and NaNs, NaN sign included"""
    rng = np.random.default_rng(3400 + W)
    nind = 70 if W % 2 else 130
    sizes = chrom_sizes(W, big=3000) + [2 * W + 100]
    chroms = make_chroms(rng, sizes, nind)
    chroms[-1][1][W + 7] = np.nan                          # the NaN chromosome: one special only (a NaN never leaves a run)
    gpos = [np.cumsum(np.diff(c[2], prepend=0) * 1e-6 * rng.uniform(0.8, 1.2, size=c[2].shape[0])) for c in chroms]
    lds = [rng.uniform(1.0, max(2.0, W / 4.0), size=(n, W)) for n in sizes]
    idx = np.array([nind - 1, 3, 64, 65, 0])
    with open_panel(gpu_ctx, chroms, nind, gpos) as panel:
        panel.set_ld(W, np.concatenate(lds, axis=0))
        covered = segs = 0
        for error in (0.0, 0.001):
            want = [ol.oracle_calc_lod(g, f, p, cs, ce, W, error, MG, threads=8) for (g, f, p, cs, ce) in chroms]
            allw = np.concatenate([w.ravel() for w in want])
            assert np.isnan(want[-1]).any()
            if error == 0.0:        # inf - inf: x86's NaN, sign bit set
                assert np.isinf(allw).any() and np.signbit(allw[np.isnan(allw)]).any()
                assert np.isnan(want[4]).any() and np.isnan(want[5]).any()
            what = ("error", error)
            for pa in (1, 32):
                assert_scores(panel.lod_windows(W, error, MG, pitch_align=pa), want, what + ("host", pa))
            got = device_rows(panel, sizes, nind, 32, lambda ptr: panel.lod_windows_device(ptr, W, error, MG, pitch_align=32))
            assert_scores(got, want, what + ("device", 32))
            got = device_rows(panel, sizes, nind, 1, lambda ptr: panel.lod_windows_device(ptr, W, error, MG, pitch_align=1))
            assert_scores(got, want, what + ("device", 1))
            # feeds: a thinned size, a subset, several sizes in one call
            step = max(4, W)
            feed, per_chr = panel.lod_feed(W, error, MG, step)
            flat = [ol.oracle_flatten(w, step) for w in want]
            assert [len(x) for x in flat] == list(per_chr), what
            assert ol.bits_equal(feed, np.concatenate(flat)), what + ("feed",)
            if error == 0.0:        # (the feed drops NaN and MISSING, keeps the infinities)
                assert np.isinf(np.concatenate(flat)).any()
            feed, per_chr = panel.lod_feed(W, error, MG, 7, ind_idx=idx)
            flat = [ol.oracle_flatten_subset(w, 7, idx) for w in want]
            assert [len(x) for x in flat] == list(per_chr), what
            assert ol.bits_equal(feed, np.concatenate(flat)), what + ("feed subset",)
            cuts = cutoffs_of(want) + [0.0]
            for cutoff, pa in zip(cuts, (1, 8, 8, 1)):
                covered += check_coverage(panel, chroms, want, W, cutoff, pa, what, error=error)
            for frac in (1e-9, 0.25, 1.0):
                segs += check_segments(panel, chroms, want, W, cuts[0], frac, what, error=error)
            wwant = [ol.oracle_calc_wlod(g, f, p, gpos[c], lds[c], cs, ce, W, error, MG, 1e-9, 7, threads=8)
                     for c, (g, f, p, cs, ce) in enumerate(chroms)]
            assert not np.isfinite(np.concatenate([w.ravel() for w in wwant])).all()
            for pa in (1, 32):
                assert_scores(panel.wlod_windows(W, error, MG, 7, 1e-9, pitch_align=pa), wwant, what + ("wlod", pa))
        assert covered > 0 and segs > 0
        wants = {V: [ol.oracle_calc_lod(g, f, p, cs, ce, V, 0.0, MG, threads=8) for (g, f, p, cs, ce) in chroms]
                 for V in NONFINITE_WIDTHS}
    # lod_feed_multi: every width on one panel that holds all of them
    with open_panel(gpu_ctx, chroms, nind) as panel:
        feeds, per_chr = panel.lod_feed_multi(NONFINITE_WIDTHS, 0.0, MG)
        for i, V in enumerate(NONFINITE_WIDTHS):
            flat = [ol.oracle_flatten(w, V) for w in wants[V]]
            assert [len(x) for x in flat] == list(per_chr[i]), V
            assert ol.bits_equal(feeds[i], np.concatenate(flat)), ("feed multi", V)
