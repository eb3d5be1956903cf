"""GPU: the KDE feed of unweighted scores with per-genotype likelihoods from the ring chain that stores only the sampled
windows (tgls_feed_kernel), through the C ABI, bit for bit against the oracle's full TGLS scores thinned by the oracle's
convertWinData2DoubleData / convertSubsetWinData2DoubleData; counts and per-chromosome counts equal.  No tolerance.

garlic_lod_feed_info tells which path a call took: every TGLS call with step >= 4 whose windows cannot sum to -9999.0
must report GARLIC_FEED_TGLS_CHAIN and a score scratch of the thinned layout's size; the fallbacks (steps below 4, the
exact chain possible, GARLIC_TGLS_FEED_FULL=1, GARLIC_TGLS_NO_RING=1) report GARLIC_FEED_FROM_SCORES and the full
layout.  Every case is a non-empty feed (tests/test_tgls_feed_cpu.py checks the shape cases with the oracle alone; all
assert it here per call)."""
import os
import re

import numpy as np
import pytest

import oracle_lib as ol
import tgls_feed_cases as cases
import wlod_feed_cases as wcases
from garlic_amd import abi

pytestmark = pytest.mark.gpu
MG, ERROR = cases.MG, cases.ERROR
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TGLS_CHAIN = getattr(abi, "FEED_TGLS_CHAIN", 3)      # (a library without the form fails on the value it reports)


def open_panel(ctx, chroms, nind, gl=None, gpos=None):
    panel = abi.Panel(ctx, [c[0].shape[0] for c in chroms], nind)
    panel.set_map(np.concatenate([c[2] for c in chroms]), [c[3] for c in chroms], [c[4] for c in chroms],
                  gpos=None if gpos is None else np.concatenate(gpos))
    panel.set_freq(np.concatenate([c[1] for c in chroms]))
    panel.set_genotypes(np.concatenate([c[0] for c in chroms], axis=0))
    if gl is not None:
        panel.set_gl(np.concatenate(gl, axis=0))
    return panel


def check_feed(panel, scores, W, step, what, *, idx=None, form=TGLS_CHAIN):
    """one TGLS feed call against the oracle; returns the feed"""
    want = cases.flat(scores, step, idx)
    assert sum(len(x) for x in want) > 0, ("empty case", what)
    feed, per_chr = panel.lod_feed(W, ERROR, MG, step, use_gl=True, ind_idx=idx)
    got_form, doubles = panel.feed_info()
    print(what, "form", got_form, "score doubles", doubles, "values", len(feed))
    assert [len(x) for x in want] == list(per_chr), (what, list(per_chr))
    flat = np.concatenate(want)
    assert feed.shape == flat.shape, what
    assert ol.bits_equal(feed, flat), (what, ol.count_mismatch(feed, flat))
    assert got_form == form, (what, got_form)
    sizes = [s.shape[1] for s in scores]
    if form == TGLS_CHAIN:
        assert doubles == cases.thinned_doubles(sizes, panel.nind, step), what
    elif form == abi.FEED_FROM_SCORES:
        assert doubles == panel.out_layout(32, panel.nind)[2], what
    return feed


def check_full_scores(panel, scores, W, what):
    """garlic_lod_windows(use_gl) against the oracle; the tuned chain alone took it (a -9999.0 sum is impossible)"""
    got = panel.lod_windows(W, ERROR, MG, use_gl=True, pitch_align=32)
    for c in range(len(scores)):
        assert ol.bits_equal(np.ascontiguousarray(got[c]), scores[c]), (what, c)
    assert panel.chain_kind() == 0, what


# ------------------------------------------------------------------------------------------------ 1. shapes

@pytest.mark.parametrize("W", cases.widths())
def test_shapes(gpu_ctx, W):
    """both sides of every boundary of the kernel (the tile, the one-stream / two-stream switch); chromosomes of 1, W-1,
    W, W+1, W+33 SNPs, gaps and a centromere; 1 .. 200 individuals; steps W, W+7, 2W, 4 and one beyond every chromosome"""
    nind, chroms, gl = cases.shape_case(W)
    sizes = [c[0].shape[0] for c in chroms]
    scores = cases.tgls_scores(chroms, gl, W)
    with open_panel(gpu_ctx, chroms, nind, gl) as panel:
        for step in cases.steps_of(W, sizes):
            check_feed(panel, scores, W, step, ("shape", W, step, nind))
        check_full_scores(panel, scores, W, ("shape", W))      # ... so no case above fell back for another reason


# ------------------------------------------------------------------------------------------------ 2. likelihoods

@pytest.mark.parametrize("kind", ["codes", "continuous"])
@pytest.mark.parametrize("W", cases.GL_WIDTHS)
def test_likelihoods(gpu_ctx, W, kind):
    """dictionary codes and continuous values, the clamp values 1e-16 and 1.0 among them (300 x -16 stays above -9990)"""
    nind, chroms, gl, steps = cases.likelihood_case(W, kind)
    scores = cases.tgls_scores(chroms, gl, W)
    with open_panel(gpu_ctx, chroms, nind, gl) as panel:
        assert panel.tgls_mode()[0] == (1 if kind == "codes" else 2)
        for step in steps:
            check_feed(panel, scores, W, step, ("gl", kind, W, step))
        check_full_scores(panel, scores, W, ("gl", kind, W))


def test_panel_fed_by_codes(gpu_ctx):
    W, nind, chroms, codes, values, gl, steps = cases.codes_case()
    scores = cases.tgls_scores(chroms, gl, W)
    with open_panel(gpu_ctx, chroms, nind) as panel:
        panel.set_gl_codes(np.concatenate(codes, axis=0), values)
        assert panel.tgls_mode()[0] == 1
        for step in steps:
            check_feed(panel, scores, W, step, ("set_gl_codes", W, step))


# ------------------------------------------------------------------------------------------------ 3. subsets

@pytest.mark.parametrize("W", [10, 100])
def test_subsets(gpu_ctx, W):
    """unordered lists that leave whole 64-individual blocks out (one, two and three of four), a list of one, then
    everyone"""
    nind, chroms, gl = cases.subset_case(W)
    scores = cases.tgls_scores(chroms, gl, W)
    with open_panel(gpu_ctx, chroms, nind, gl) as panel:
        left_out = set()
        for idx in (np.array(x) for x in cases.SUBSETS):
            left_out.add(4 - len({int(i) >> 6 for i in idx}))
            check_feed(panel, scores, W, W, ("subset", W, list(idx)), idx=idx)
        assert {1, 3} <= left_out
        check_feed(panel, scores, W, W, ("everyone after subsets", W))


# ------------------------------------------------------------------------------------------------ 4. dropped by value

@pytest.mark.parametrize("W", [5, 60, 300])
def test_nonfinite_terms(gpu_ctx, W):
    """a NaN frequency and likelihoods of 0 and infinity (infinite terms): the chain carries the reference's NaN /
    infinity to the end of the run, the feed drops NaN by value"""
    nind, chroms, gl, steps = cases.nonfinite_case(W)
    scores = cases.tgls_scores(chroms, gl, W)
    allw = np.concatenate([s.ravel() for s in scores])
    assert np.isnan(allw).any()
    with open_panel(gpu_ctx, chroms, nind, gl) as panel:
        for step in steps:
            feed = check_feed(panel, scores, W, step, ("non-finite terms", W, step))
            assert not np.isnan(feed).any()


# ------------------------------------------------------------------------------------------------ 5. fallbacks

def test_fallbacks_tell_the_truth(gpu_ctx, monkeypatch):
    W, nind, chroms, gl, _ = cases.fallback_case()
    sizes = [c[0].shape[0] for c in chroms]
    scores = cases.tgls_scores(chroms, gl, W)
    with open_panel(gpu_ctx, chroms, nind, gl) as panel:
        full = panel.out_layout(32, nind)[2]
        check_feed(panel, scores, W, W, "thinned")
        assert panel.feed_info() == (TGLS_CHAIN, cases.thinned_doubles(sizes, nind, W))
        assert panel.feed_info()[1] < full // 8          # (every chromosome's columns are padded to 32: not W times smaller here)
        for step in (1, 3):
            check_feed(panel, scores, W, step, ("step", step), form=abi.FEED_FROM_SCORES)
            assert panel.feed_info() == (abi.FEED_FROM_SCORES, full)
        for switch in ("GARLIC_TGLS_FEED_FULL", "GARLIC_TGLS_NO_RING"):
            monkeypatch.setenv(switch, "1")
            check_feed(panel, scores, W, W, switch, form=abi.FEED_FROM_SCORES)
            assert panel.feed_info() == (abi.FEED_FROM_SCORES, full)
            monkeypatch.delenv(switch)
            check_feed(panel, scores, W, W, ("after", switch))


def test_exact_chain_possible_keeps_the_full_scores(gpu_ctx):
    """W = 1000 with likelihoods of 1e-16: W times the most negative term passes -9999, the rescan needs the full matrix"""
    W, narrow, nind, chroms, gl = cases.exact_case()
    scores = cases.tgls_scores(chroms, gl, W)
    with open_panel(gpu_ctx, chroms, nind, gl) as panel:
        check_feed(panel, scores, W, W, "exact possible", form=abi.FEED_FROM_SCORES)
        assert panel.chain_kind() in (1, 2)
        # ... and a width at which it is not possible takes the thinned form on the same panel
        check_feed(panel, cases.tgls_scores(chroms, gl, narrow), narrow, narrow, "narrow again")


# ------------------------------------------------------------------------------------------------ 6. neighbours

@pytest.mark.parametrize("W", [20, 200])
def test_neighbours_on_one_panel(gpu_ctx, W):
    """full scores, the weighted feed (scales the term matrix), the thinned feed again (plain terms back), the --error
    feed and the ROH segments after a thinned TGLS feed of the same width: every one against the oracle"""
    M, MU = wcases.M, wcases.MU
    nind, chroms, gpos, lds, gl, _ = cases.neighbour_case(W)
    scores = cases.tgls_scores(chroms, gl, W)
    with open_panel(gpu_ctx, chroms, nind, gl, gpos) as panel:
        panel.set_ld(W, np.concatenate(lds, axis=0))
        check_feed(panel, scores, W, W, "thinned")
        check_full_scores(panel, scores, W, "full scores after the thinned feed")
        wscores = wcases.wlod_scores(chroms, gpos, lds, W, gl=gl)
        wwant = np.concatenate(cases.flat(wscores, W))
        wfeed, _ = panel.lod_feed(W, ERROR, MG, W, use_gl=True, weighted=True, M=M, mu=MU)
        assert len(wwant) > 0 and ol.bits_equal(wfeed, wwant)
        assert panel.feed_info()[0] == abi.FEED_SAMPLED_WLOD
        check_feed(panel, scores, W, W, "thinned after the weighted feed")
        pwant = np.concatenate([ol.oracle_flatten(ol.oracle_calc_lod(g, f, p, cs, ce, W, ERROR, MG), W) for (g, f, p, cs, ce) in chroms])
        pfeed, _ = panel.lod_feed(W, ERROR, MG, W)
        assert len(pwant) > 0 and ol.bits_equal(pfeed, pwant)
        assert panel.feed_info()[0] == abi.FEED_CHAIN
        check_feed(panel, scores, W, W + 7, "thinned after the --error feed")
        scored = np.concatenate([x[np.isfinite(x) & (x != -9999.0)] for x in scores])
        cutoff, frac = float(np.quantile(scored, 0.7)), 0.25       # (a cutoff that leaves segments to compare)
        segs = panel.roh_segments(W, ERROR, MG, cutoff, frac, use_gl=True)
        n_checked = 0
        for c, (g, f, p, cs, ce) in enumerate(chroms):
            want_segs = ol.oracle_roh_segments(ol.oracle_roh_coverage(scores[c], W, cutoff), p, cs, ce, W, MG, frac)
            got = sorted((int(i), int(a), int(b)) for i, cc, a, b in segs if cc == c)
            assert got == sorted(want_segs), ("roh segments", c)
            n_checked += len(got)
        assert n_checked > 0
        check_feed(panel, scores, W, 2 * W, "thinned after the segments")


# ------------------------------------------------------------------------------------------------ 7. switch, repeats

@pytest.mark.parametrize("seed", [1, 2, 3])
def test_same_bytes_with_and_without_the_switch(gpu_ctx, seed, monkeypatch):
    """random panels (window, step, individuals, likelihoods drawn): GARLIC_TGLS_FEED_FULL=1 and the thinned path give
    the oracle's bytes both"""
    W, step, nind, chroms, gl, idx = cases.random_case(seed)
    scores = cases.tgls_scores(chroms, gl, W)
    with open_panel(gpu_ctx, chroms, nind, gl) as panel:
        a = check_feed(panel, scores, W, step, ("thinned", seed))
        a_sub = check_feed(panel, scores, W, step, ("thinned subset", seed), idx=idx)
        monkeypatch.setenv("GARLIC_TGLS_FEED_FULL", "1")
        b = check_feed(panel, scores, W, step, ("full", seed), form=abi.FEED_FROM_SCORES)
        b_sub = check_feed(panel, scores, W, step, ("full subset", seed), idx=idx, form=abi.FEED_FROM_SCORES)
        assert ol.bits_equal(a, b) and ol.bits_equal(a_sub, b_sub)


def test_twenty_launches_identical(gpu_ctx):
    W, nind, chroms, gl = cases.repeat_case()
    scores = cases.tgls_scores(chroms, gl, W)
    with open_panel(gpu_ctx, chroms, nind, gl) as panel:
        first = check_feed(panel, scores, W, W, "first")
        for k in range(20):
            feed, _ = panel.lod_feed(W, ERROR, MG, W, use_gl=True)
            assert ol.bits_equal(feed, first), k
            assert panel.feed_info()[0] == TGLS_CHAIN


# ------------------------------------------------------------------------------------------------ 8. memory

def score_chunk_bytes():
    """the size of the physical chunks score memory is made of, from the allocator's source"""
    src = open(os.path.join(ROOT, "garlic_amd", "csrc", "garlic_hip.hip")).read()
    m = re.search(r"const size_t chunk = \(\(\(size_t\)1 << (\d+)\) \+ gran - 1\) / gran \* gran;", src)
    assert m, "score_alloc's chunk size not found"
    return 1 << int(m.group(1))


def test_score_memory_is_the_thinned_matrix(gpu_ctx, monkeypatch):
    """A panel whose full score matrix (1.2 GB) is larger than one chunk of the score allocator: after release_scratch
    and trim the TGLS step = W feed may raise live + pooled score memory by the thinned matrix rounded up to the chunk
    size and no more -- the full matrix does not fit in that -- and under GARLIC_TGLS_FEED_FULL=1 the same call takes at
    least the full matrix (so the bound above is a real one).  The bound comes from the layout and the chunk size."""
    W, nloci, nind = 100, 60000, 2500
    rng = np.random.default_rng(8500)
    geno = rng.integers(0, 3, size=(nloci, nind), dtype=np.int16)
    geno[rng.random(nloci) < 0.01, :] = -9
    geno[::97, ::13] = -9
    pos = np.cumsum(rng.integers(1, 4000, size=nloci)).astype(np.int32)
    freq = rng.uniform(0.05, 0.95, size=nloci)
    gl = rng.choice([1e-6, 1e-3, 0.01, 0.2], size=(nloci, nind))
    chunk = score_chunk_bytes()
    with abi.Panel(gpu_ctx, [nloci], nind) as panel:
        panel.set_map(pos, [0], [0])
        panel.set_freq(freq)
        panel.set_genotypes(geno)
        panel.set_gl(gl)
        full = panel.out_layout(32, nind)[2] * 8
        thin = cases.thinned_doubles([nloci], nind, W) * 8
        assert full > chunk and thin < full // 50
        bound = (thin + chunk - 1) // chunk * chunk
        panel.release_scratch()
        gpu_ctx.trim()
        live0, pooled0, _ = gpu_ctx.alloc_stats()
        feed, per_chr = panel.lod_feed(W, ERROR, MG, W, use_gl=True)
        assert len(feed) > 0 and len(feed) == per_chr[0]
        live1, pooled1, _ = gpu_ctx.alloc_stats()
        print("score memory: before %d, after the thinned feed %d (thinned matrix %d, full %d, chunk %d)"
              % (live0 + pooled0, live1 + pooled1, thin, full, chunk))
        assert panel.feed_info() == (TGLS_CHAIN, thin // 8)
        assert live1 + pooled1 - (live0 + pooled0) <= bound
        # the sampled windows against the oracle, for a few individuals
        some = np.array([0, 1, 777, nind - 1])
        want = ol.oracle_calc_lod(geno[:, some], freq, pos, 0, 0, W, ERROR, MG, gl=np.ascontiguousarray(gl[:, some]), threads=8)
        got, _ = panel.lod_feed(W, ERROR, MG, W, use_gl=True, ind_idx=some)
        flat = ol.oracle_flatten(want, W)
        assert len(flat) > 0 and ol.bits_equal(got, flat)
        monkeypatch.setenv("GARLIC_TGLS_FEED_FULL", "1")
        panel.release_scratch()
        gpu_ctx.trim()
        live0, pooled0, _ = gpu_ctx.alloc_stats()
        feed_full, _ = panel.lod_feed(W, ERROR, MG, W, use_gl=True)
        live2, pooled2, _ = gpu_ctx.alloc_stats()
        print("score memory under GARLIC_TGLS_FEED_FULL=1: before %d, after %d" % (live0 + pooled0, live2 + pooled2))
        assert live2 + pooled2 - (live0 + pooled0) >= full
        assert ol.bits_equal(feed, feed_full)
        assert panel.stats()["n_stall_reruns"] == 0
        panel.release_scratch()
    gpu_ctx.trim()
