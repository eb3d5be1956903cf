"""GPU: every kernel that walks runs, on the dense-run panels of tests/run_cases.py, bit for bit against the oracle.

A run is a maximal stretch of SNPs that no max_gap hole or centromere cuts.  The other GPU files meet run edges where a
run is a whole chromosome, or at a handful of random places; here a chromosome has hundreds of runs of 1, W-1, W, W+1,
.. W+65, 3W+7 SNPs (1, 2, 31 .. 33, 63 .. 65 valid windows) that start at arbitrary columns, so for W <= 31 one 32-bit
word of a bit row holds windows of two, three or more runs written by different work items, MISSING fills of exactly
W-1 columns sit between other items' stores, and thinned feeds step through runs shorter than the step
(tests/test_runs_cpu.py asserts that the panels hold these shapes and pins the oracle to the reference on them).

Every comparison is exact and against the oracle; the only comparison between two GPU runs is the explicit repeat
check of the segment list.  max_gap = 5000.  Each panel carries one ordinary random_panel chromosome and one of W-1
SNPs behind the dense ones, so no chromosome's output base, bit-row words or break words are trivial.  Where the
library tells which form ran (chain_kind, tgls_mode, tgls_terms_info, feed_info, feed_multi_info, stats) the test
asserts it: the unweighted chain at every width incl. 250; the TGLS ring chain on both sides of TG_SINGLE_MAX_W = 144
and in slabs; the wLOD stream / small-tile forms below WLOD_R = 16 and the tile / strip forms above (113, 241 are the
strip switches; 150 lies between them); COVF_MAX_W = 1024 is not reached, so unweighted bits come from lod_bits_kernel."""
import ctypes as C
import functools

import numpy as np
import pytest

import oracle_lib as ol
import run_cases as rc
import tgls_slab_cases as slabs
from garlic_amd import abi
from test_gpu_window_regimes import assert_scores, open_panel

pytestmark = pytest.mark.gpu
MG, ERR, M, MU = rc.MAX_GAP, 0.001, 7, 1e-9
WS = [2, 5, 10, 16, 30, 33, 100, 150]
VARIANTS = ["dense", "centromere", "borders", "from_zero"]
GL_VALUES = np.array([1e-16, 1e-3, 0.01, 0.2, 1.0])
FLAG_SETS = [(False, False), (False, True), (True, False), (True, True)]      # (weighted, use_gl)
CUTOFFS = (0.0, -2.5, -10000.0)
FRACS = (1e-9, 0.25, 1.0)


class Data:
    """the chromosomes of one case ("all": the four variants behind one another) plus a random_panel chromosome and one of
    W-1 SNPs; genetic positions, LD weights and likelihood codes for them; the oracle's scores, computed once per mode"""

    def __init__(self, name, W, nind):
        if name == "all":
            chroms = [c for v in VARIANTS for c in rc.CASES[v](W, nind)[0]]
        elif name == "many_blocks":
            chroms = rc.many_blocks(W, nind)[0]
        else:
            chroms = rc.CASES[name](W, nind)[0]
        rng = np.random.default_rng([W, nind, len(name)])
        if name != "all_breaks":
            chroms = list(chroms) + [ol.random_panel(rng, 700, nind, max_gap=MG)]
        chroms = list(chroms) + [ol.random_panel(rng, max(1, W - 1), nind, max_gap=MG, gaps=0)]
        self.name, self.W, self.nind, self.chroms = name, W, nind, chroms
        self.sizes = [c[0].shape[0] for c in chroms]
        self.nloci = sum(self.sizes)
        self.gpos = [c[2] * 1e-6 for c in chroms]
        self.ld = [rng.uniform(1.0, max(2.0, W / 4.0), size=(n, W)) for n in self.sizes]
        self.codes = [rng.integers(0, len(GL_VALUES), size=c[0].shape).astype(np.uint8) for c in chroms]
        self.gl = [GL_VALUES[k] for k in self.codes]
        self._scores = {}

    def scores(self, weighted=False, use_gl=False, W=None, gl=None, max_gap=MG):
        W = self.W if W is None else W
        key = (weighted, use_gl, W, max_gap)
        if gl is not None or key not in self._scores:      # (a caller's own likelihoods: not kept)
            out = []
            for c, (g, f, p, cs, ce) in enumerate(self.chroms):
                e = (self.gl[c] if gl is None else gl[c]) if use_gl else None
                if weighted:
                    assert W == self.W
                    out.append(ol.oracle_calc_wlod(g, f, p, self.gpos[c], self.ld[c], cs, ce, W, ERR, max_gap, MU, M, gl=e, threads=8))
                else:
                    out.append(ol.oracle_calc_lod(g, f, p, cs, ce, W, ERR, max_gap, gl=e, threads=8))
            if gl is not None:
                return out
            self._scores[key] = out
        return self._scores[key]

    def open(self, ctx, ld=False, gl=False):
        panel = open_panel(ctx, self.chroms, self.nind, self.gpos)
        if ld:
            panel.set_ld(self.W, np.concatenate(self.ld, axis=0))
        if gl:
            panel.set_gl_codes(np.concatenate(self.codes, axis=0), GL_VALUES)
        return panel

    def longest_run(self):
        return max(int(np.diff(np.append(np.flatnonzero(rc.breaks_of(c[2], c[3], c[4], MG)), c[2].shape[0])).max()) for c in self.chroms)


@functools.lru_cache(maxsize=2)
def data(name, W, nind=70):
    return Data(name, W, nind)


def flat(scores, step, idx=None):
    return [ol.oracle_flatten(s, step) if idx is None else ol.oracle_flatten_subset(s, step, idx) for s in scores]


def feed_form(weighted, use_gl, W, step):
    if weighted:
        return abi.FEED_SAMPLED_WLOD if step >= W else abi.FEED_FROM_SCORES
    if step < 4:
        return abi.FEED_FROM_SCORES
    return abi.FEED_TGLS_CHAIN if use_gl else abi.FEED_CHAIN


def check_feed(panel, scores, W, step, weighted, use_gl, what, idx=None, order=abi.FEED_ORDER_REFERENCE):
    want = flat(scores, step, idx)
    feed, per_chr = panel.lod_feed(W, ERR, MG, step, use_gl=use_gl, weighted=weighted, M=M, mu=MU, ind_idx=idx)
    assert [len(x) for x in want] == list(per_chr), (what, step)
    allw = np.concatenate(want)
    assert ol.bits_equal(feed, allw if order == abi.FEED_ORDER_REFERENCE else np.sort(allw)), (what, step)
    if order == abi.FEED_ORDER_REFERENCE:
        assert panel.feed_info()[0] == feed_form(weighted, use_gl, W, step), (what, step, panel.feed_info())
    return allw.shape[0]


def oracle_counts(scores, W, cutoff):
    """the oracle's inWin[] loop over the oracle's scores, per chromosome (computed once per cutoff: the counts are
    compared themselves and feed the oracle's segment walk)"""
    return [ol.oracle_roh_coverage(np.ascontiguousarray(s), W, cutoff) for s in scores]


def segments_of_counts(d, counts, W, frac):
    """rc.oracle_segments from counts already at hand -> [(individual, chromosome, first SNP, last SNP)], sorted"""
    out = []
    for c, (g, f, p, cs, ce) in enumerate(d.chroms):
        out += [(i, c, a, b) for i, a, b in ol.oracle_roh_segments(counts[c], p, cs, ce, W, MG, frac)]
    return sorted(out)


def check_coverage(panel, d, scores, W, cutoff, pa, what, counts=None, **kw):
    counts = oracle_counts(scores, W, cutoff) if counts is None else counts
    got = panel.roh_coverage_fused(W, ERR, MG, cutoff, pitch_align=pa, M=M, mu=MU, **kw)
    for c, n in enumerate(d.sizes):
        assert np.array_equal(got[c][:, :n], counts[c]), (what, W, cutoff, pa, c)
    return sum(int(np.count_nonzero(x)) for x in counts)


def check_segments(panel, d, scores, W, cutoff, frac, what, repeats=1, counts=None, **kw):
    want = segments_of_counts(d, oracle_counts(scores, W, cutoff) if counts is None else counts, W, frac)
    for _ in range(repeats):      # the list leaves the kernel through an atomic counter: the same every time
        got = [tuple(int(v) for v in r) for r in panel.roh_segments(W, ERR, MG, cutoff, frac, M=M, mu=MU, **kw)]
        assert sorted(got) == want and got == want, (what, W, cutoff, frac, len(got), len(want))
    return want


# ------------------------------------------------------------------------------------------------ 1. boundaries

def check_w2(panel, chroms, mg, what):
    """W = 2: a window is valid exactly where its two SNPs are in one run, so the mask pins every single boundary"""
    out = panel.lod_windows(2, ERR, mg)
    assert panel.stats()["n_segments"] == rc.n_boundaries(chroms, mg), (what, mg)
    assert panel.chain_kind() == 0
    scored = 0
    for c, (g, f, p, cs, ce) in enumerate(chroms):
        mask = ol.oracle_mask(p, cs, ce, 2, mg).astype(bool)
        assert np.array_equal(out[c] != ol.MISSING, np.broadcast_to(mask, out[c].shape)), (what, mg, c)
        assert ol.bits_equal(np.ascontiguousarray(out[c]), ol.oracle_calc_lod(g, f, p, cs, ce, 2, ERR, mg, threads=8)), (what, mg, c)
        scored += int(mask.sum())
    return scored


@pytest.mark.parametrize("name", VARIANTS + ["all_breaks"])
def test_boundaries_of_every_variant(gpu_ctx, name):
    """garlic_call_stats.n_segments against the boundary count from positions, centromeres and chromosome offsets in
    numpy, and the W = 2 mask; `borders` at two further max_gap values (every other pair a break, nearly every pair
    one) and back: the boundary cache is keyed by max_gap"""
    d = data(name, 2, 37)
    with d.open(gpu_ctx) as panel:
        first = check_w2(panel, d.chroms, MG, name)
        assert (first == 0) == (name == "all_breaks")
        if name == "borders":
            for mg in (100, 1, MG):
                check_w2(panel, d.chroms, mg, name)


def test_boundaries_over_69_scan_workgroups(gpu_ctx):
    """many_blocks: 140,000 SNPs, about 9,000 runs: the boundary scan's carry loop takes a second round"""
    d = data("many_blocks", 2, 8)
    assert -(-d.nloci // 2048) >= 69
    with d.open(gpu_ctx) as panel:
        assert check_w2(panel, d.chroms, MG, "many_blocks") > 100000
        scores = d.scores()
        want = check_segments(panel, d, scores, 2, 0.0, 0.25, "many_blocks")
        assert want == rc.oracle_segments(d.chroms, scores, 2, 0.0, MG, 0.25) and len(want) > 1000
        check_feed(panel, scores, 2, 5, False, False, "many_blocks")


# ------------------------------------------------------------------------------------------------ 2. unweighted scores

NAN_PATTERN = np.uint64(0x7FF8DEADBEEF0001)


def device_prefilled(panel, nind, pa, launch):
    """the raw words of a device score buffer that held a NaN pattern before launch(ptr) wrote into it"""
    import torch
    base, pitch, total = panel.out_layout(pa, nind)
    out = torch.from_numpy(np.full(int(total), NAN_PATTERN, dtype=np.uint64).view(np.float64)).cuda()
    torch.cuda.synchronize()
    launch(out.data_ptr())
    panel.ctx.synchronize()
    return out.cpu().numpy().view(np.uint64), base, pitch


@pytest.mark.parametrize("W", WS + [250])
def test_unweighted_scores(gpu_ctx, W):
    """lod_chain_kernel and its MISSING fills: dense rows and rows padded to 8 and 32, 1 / 37 / 130 individuals, a
    sub-range of them; every variant in one panel; pad columns of a prefilled buffer untouched (fills next to chain
    stores write each element exactly once, and nothing else)"""
    for nind in (1, 37, 130):
        d = data("dense", W, nind)
        want = d.scores()
        with d.open(gpu_ctx) as panel:
            for pa in (1, 8, 32):
                assert_scores(panel.lod_windows(W, ERR, MG, pitch_align=pa), want, ("dense", nind, pa))
                assert panel.chain_kind() == 0
            if nind == 130:
                got = panel.lod_windows(W, ERR, MG, ind_begin=37, ind_count=70, pitch_align=32)
                assert_scores(got, [w[37:107] for w in want], ("dense", "sub-range"))
            if nind == 37:
                words, base, pitch = device_prefilled(panel, nind, 32, lambda ptr: panel.lod_windows_device(ptr, W, ERR, MG, pitch_align=32))
                pads = 0
                for c, n in enumerate(d.sizes):
                    rows = words[base[c]: base[c] + nind * pitch[c]].reshape(nind, pitch[c])
                    assert np.array_equal(rows[:, :n], np.ascontiguousarray(want[c]).view(np.uint64)), ("prefilled", c)
                    assert (rows[:, n:] == NAN_PATTERN).all(), ("pad columns written", c)
                    pads += rows[:, n:].size
                assert pads > 0
    d = data("all", W)
    with d.open(gpu_ctx) as panel:
        assert_scores(panel.lod_windows(W, ERR, MG, pitch_align=32), d.scores(), "all variants")
        assert panel.chain_kind() == 0


@pytest.mark.parametrize("W", [10, 33])
def test_unweighted_scores_of_several_sizes_in_one_call(gpu_ctx, W):
    d = data("dense", W)
    sizes = (5, 10, 33, 100)
    with d.open(gpu_ctx) as panel:
        got = panel.lod_windows_multi(sizes, ERR, MG, pitch_align=32)
        for V in sizes:
            assert_scores(got[V], d.scores(W=V), ("multi", V))


# ------------------------------------------------------------------------------------------------ 3. TGLS

@pytest.mark.parametrize("W", [5, 10, 33, 100, 144, 145, 150])
def test_tgls_scores(gpu_ctx, W):
    """the ring chain (one stream up to 144, two above) from dictionary codes and from continuous likelihoods"""
    d = data("dense", W)
    rng = np.random.default_rng(W)
    with d.open(gpu_ctx, gl=True) as panel:
        for pa in (1, 32):
            assert_scores(panel.lod_windows(W, ERR, MG, use_gl=True, pitch_align=pa), d.scores(use_gl=True), ("codes", pa))
        assert panel.tgls_mode()[0] == abi.TGLS_DICTIONARY and panel.chain_kind() == 0
    cont = [rng.uniform(1e-4, 0.5, size=c[0].shape) for c in d.chroms]
    with d.open(gpu_ctx) as panel:
        panel.set_gl(np.concatenate(cont, axis=0))
        assert_scores(panel.lod_windows(W, ERR, MG, use_gl=True, pitch_align=32), d.scores(use_gl=True, gl=cont), "continuous")
        assert panel.tgls_mode()[0] == abi.TGLS_CONTINUOUS and panel.chain_kind() == 0


@pytest.mark.parametrize("W", [10, 145])
def test_tgls_scores_in_term_slabs(gpu_ctx, W):
    """a term budget of two blocks: three slabs of one 64-individual block each, every one walking every run"""
    d = data("dense", W, 130)
    with d.open(gpu_ctx, gl=True) as panel:
        panel.set_tgls_term_budget(slabs.budget_for(d.nloci, 1, d.nind))
        assert_scores(panel.lod_windows(W, ERR, MG, use_gl=True, pitch_align=32), d.scores(use_gl=True), "slabs")
        info = panel.tgls_terms_info()
        assert info["slab_blocks"] == 1 and info["n_slabs"] == 3, info
        check_feed(panel, d.scores(use_gl=True), W, max(4, W), False, True, "slabs")
        assert panel.tgls_terms_info()["n_slabs"] == 3


# ------------------------------------------------------------------------------------------------ 4. wLOD

@pytest.mark.parametrize("W", [5, 10, 16, 33, 100])
def test_wlod_scores(gpu_ctx, W):
    """the stream / small-tile forms (W < 16) and the tile / strip forms, plain and with likelihoods: every variant"""
    d = data("all", W)
    with d.open(gpu_ctx, ld=True, gl=True) as panel:
        for use_gl in (False, True):
            want = d.scores(weighted=True, use_gl=use_gl)
            for pa in (32, 1):
                got = panel.wlod_windows(W, ERR, MG, M, MU, use_gl=use_gl, pitch_align=pa)
                assert_scores(got, want, ("wlod", use_gl, pa))
                assert panel.stats()["n_stall_reruns"] == 0


# ------------------------------------------------------------------------------------------------ 5. feeds

@pytest.mark.parametrize("W", WS)
def test_feeds(gpu_ctx, W):
    """lod_feed unweighted, TGLS and weighted: steps 1, 4, W, W + 7 and one beyond every run; a subsample; sorted order"""
    d = data("all", W)
    steps = sorted({1, 4, W, W + 7, d.longest_run() + 1})
    idx = np.array([69, 3, 64, 0, 40])
    with d.open(gpu_ctx, ld=True, gl=True) as panel:
        for weighted, use_gl in FLAG_SETS[:3]:
            scores = d.scores(weighted=weighted, use_gl=use_gl)
            what = ("feed", weighted, use_gl)
            n = [check_feed(panel, scores, W, step, weighted, use_gl, what) for step in steps]
            assert n[0] > 1000 and n[-1] > 0
            for step in (max(4, W), W + 7):
                check_feed(panel, scores, W, step, weighted, use_gl, what + ("subsample",), idx=idx)
            panel.set_feed_order(abi.FEED_ORDER_SORTED)
            check_feed(panel, scores, W, max(4, W), weighted, use_gl, what + ("sorted",), order=abi.FEED_ORDER_SORTED)
            panel.set_feed_order(abi.FEED_ORDER_REFERENCE)


def test_feeds_of_several_sizes_in_one_call(gpu_ctx):
    d = data("all", 10)
    sizes = (5, 10, 33)
    with d.open(gpu_ctx, gl=True) as panel:
        feeds, per_chr = panel.lod_feed_multi(sizes, ERR, MG)
        assert panel.feed_info()[0] == abi.FEED_CHAIN
        for i, V in enumerate(sizes):
            want = flat(d.scores(W=V), V)
            assert [len(x) for x in want] == list(per_chr[i]), V
            assert ol.bits_equal(feeds[i], np.concatenate(want)), V
        feeds, per_chr = panel.lod_feed_multi_tgls(sizes, MG)
        assert set(panel.feed_multi_info(3)["forms"]) <= {abi.FEED_TGLS_CHAIN, abi.FEED_TGLS_CHAIN_SHARED}
        for i, V in enumerate(sizes):
            want = flat(d.scores(use_gl=True, W=V), V)
            assert [len(x) for x in want] == list(per_chr[i]), ("tgls", V)
            assert ol.bits_equal(feeds[i], np.concatenate(want)), ("tgls", V)


@pytest.mark.parametrize("W", [2, 10, 33])
def test_a_panel_without_a_valid_window(gpu_ctx, W):
    """all_breaks: every score MISSING, every feed empty (the KDE entry refuses it and leaves its output alone), every
    count zero, no segment"""
    d = data("all_breaks", W, 37)
    with d.open(gpu_ctx, ld=True, gl=True) as panel:
        for weighted, use_gl in FLAG_SETS:
            if weighted:
                got = panel.wlod_windows(W, ERR, MG, M, MU, use_gl=use_gl, pitch_align=32)
            else:
                got = panel.lod_windows(W, ERR, MG, use_gl=use_gl, pitch_align=32)
            assert all((np.ascontiguousarray(g).view(np.uint64) == np.float64(ol.MISSING).view(np.uint64)).all() for g in got)
            for step in (1, max(4, W)):
                feed, per_chr = panel.lod_feed(W, ERR, MG, step, use_gl=use_gl, weighted=weighted, M=M, mu=MU)
                assert feed.shape[0] == 0 and not per_chr.any()
            out = abi.Kde()
            C.memset(C.byref(out), 0x5A, C.sizeof(out))
            before = bytes(out)
            rcode = abi.lib().garlic_lod_kde(panel.handle, W, ERR, MG, int(use_gl), int(weighted), M, MU, max(4, W), None, 0,
                                             C.byref(out), None)
            assert rcode == abi.ERR_INVALID and bytes(out) == before
            for pa in (1, 8):
                cov = panel.roh_coverage_fused(W, ERR, MG, 0.0, pitch_align=pa, use_gl=use_gl, weighted=weighted, M=M, mu=MU)
                assert all(not c[:, :n].any() for c, n in zip(cov, d.sizes))
            assert len(panel.roh_segments(W, ERR, MG, 0.0, 0.25, use_gl=use_gl, weighted=weighted, M=M, mu=MU)) == 0
        feeds, per_chr = panel.lod_feed_multi((W, W + 3, 2 * W + 1), ERR, MG)     # (no narrower: the last chromosome has W-1 SNPs)
        assert all(f.shape[0] == 0 for f in feeds) and not per_chr.any()
        # a cutoff below MISSING counts every window, scored or not: the oracle's counts and segments
        scores = d.scores()
        check_coverage(panel, d, scores, W, -10000.0, 8, "all_breaks")
        check_segments(panel, d, scores, W, -10000.0, 1e-9, "all_breaks")


# ------------------------------------------------------------------------------------------------ 6. coverage, segments

@pytest.mark.parametrize("W", WS)
def test_coverage_and_segments(gpu_ctx, W):
    """roh_coverage_fused and roh_segments, unweighted / with likelihoods / weighted / both, on every variant in one
    panel: bit words shared between runs, several break bits in a word, breaks at bit 0 and 31, breaks inside covered
    stretches (cutoff -10000: one stretch per chromosome cut into every run), a chromosome from position 0"""
    import torch
    d = data("all", W, 40 if W in (2, 100, 150) else 70)      # (fewer rows where the segment lists or the oracle's sums are long)
    with d.open(gpu_ctx, ld=True, gl=True) as panel:
        for weighted, use_gl in FLAG_SETS:
            scores = d.scores(weighted=weighted, use_gl=use_gl)
            kw = dict(weighted=weighted, use_gl=use_gl)
            what = ("weighted" if weighted else "unweighted", "gl" if use_gl else "error")
            covered = n_segs = 0
            ref = None
            for cutoff in CUTOFFS:
                counts = oracle_counts(scores, W, cutoff)
                for pa in (1, 8):
                    covered += check_coverage(panel, d, scores, W, cutoff, pa, what, counts=counts, **kw)
                for frac in FRACS:
                    want = check_segments(panel, d, scores, W, cutoff, frac, what, repeats=3 if (cutoff, frac) == (0.0, 0.25) else 1,
                                          counts=counts, **kw)
                    n_segs += len(want)
                    if (cutoff, frac) == (0.0, 0.25):
                        ref = want
            assert covered > 0 and n_segs > 200 and len(ref) > 1
            if weighted or use_gl:
                continue
            with pytest.raises(abi.GarlicError):
                panel.roh_segments(W, ERR, MG, 0.0, 0.25, capacity=len(ref) - 1)
            # the counts of a device score matrix (roh_bits_from_scores_kernel)
            base, pitch, total = panel.out_layout(32, d.nind)
            dev = torch.empty(int(total), dtype=torch.float64, device="cuda")
            torch.cuda.synchronize()
            panel.lod_windows_device(dev.data_ptr(), W, ERR, MG, pitch_align=32)
            for cutoff in CUTOFFS:
                counts = oracle_counts(scores, W, cutoff)
                for ipa in (1, 8):
                    got = panel.roh_coverage(dev.data_ptr(), W, cutoff, pitch_align=32, inwin_pitch_align=ipa)
                    for c, n in enumerate(d.sizes):
                        assert np.array_equal(got[c][:, :n], counts[c]), (W, cutoff, ipa, c)


@pytest.mark.parametrize("W", [5, 30, 100])
def test_coverage_and_segments_by_individual_count(gpu_ctx, W):
    """1, 37 and 130 individuals: a lone row, a ragged block, two blocks and a ragged third"""
    for nind in (1, 37, 130):
        d = data("dense", W, nind)
        scores = d.scores()
        with d.open(gpu_ctx) as panel:
            for cutoff, pa in ((0.0, 1), (-2.5, 8)):
                check_coverage(panel, d, scores, W, cutoff, pa, nind)
                check_segments(panel, d, scores, W, cutoff, 0.25, nind)


# ------------------------------------------------------------------------------------------------ 7. fallback forms

@pytest.mark.parametrize("W", [5, 10])
@pytest.mark.parametrize("switch", ["GARLIC_COVERAGE_UNFUSED", "GARLIC_FEED_NO_ASM"])
def test_fallback_forms_on_shared_words(gpu_ctx, monkeypatch, switch, W):
    """counts from a score matrix, and the feed / bits chains through the compiler-generated tiles, where a bit word
    holds the windows of several runs"""
    d = data("dense", W)
    monkeypatch.setenv(switch, "1")
    with d.open(gpu_ctx, ld=True, gl=True) as panel:
        for weighted, use_gl in FLAG_SETS:
            scores = d.scores(weighted=weighted, use_gl=use_gl)
            kw = dict(weighted=weighted, use_gl=use_gl)
            assert check_coverage(panel, d, scores, W, 0.0, 8, switch, **kw) > 0
            assert len(check_segments(panel, d, scores, W, 0.0, 0.25, switch, **kw)) > 100
        for step in (4, W + 7):
            check_feed(panel, d.scores(), W, step, False, False, switch)
