"""GPU: the weighted KDE feed from the sampled windows only (wlod_feed_kernel), through the C ABI, bit for bit against the
oracle's full wLOD scores thinned by the oracle's convertWinData2DoubleData; counts and per-chromosome counts equal.

garlic_lod_feed_info tells which path a call took: every weighted call with step >= W here must report
GARLIC_FEED_SAMPLED_WLOD and a score scratch of the thinned layout's size.  Every case is a non-empty feed
(tests/test_wlod_feed_cpu.py checks the shape cases with the oracle alone; the others assert it here)."""
import re
import os

import numpy as np
import pytest

import oracle_lib as ol
import wlod_feed_cases as cases
from garlic_amd import abi

pytestmark = pytest.mark.gpu
MG, ERROR, M, MU = cases.MG, cases.ERROR, cases.M, cases.MU
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def open_panel(ctx, chroms, nind, gpos, W, lds):
    panel = abi.Panel(ctx, [c[0].shape[0] for c in chroms], nind)
    panel.set_map(np.concatenate([c[2] for c in chroms]), [c[3] for c in chroms], [c[4] for c in chroms], gpos=np.concatenate(gpos))
    panel.set_freq(np.concatenate([c[1] for c in chroms]))
    panel.set_genotypes(np.concatenate([c[0] for c in chroms], axis=0))
    panel.set_ld(W, np.concatenate(lds, axis=0))
    return panel


def check_feed(panel, scores, W, step, what, *, error=ERROR, use_gl=False, idx=None, form=abi.FEED_SAMPLED_WLOD):
    """one weighted feed call against the oracle; returns the feed"""
    want = cases.flat(scores, step, idx)
    assert sum(len(x) for x in want) > 0, ("empty case", what)
    feed, per_chr = panel.lod_feed(W, error, MG, step, use_gl=use_gl, weighted=True, M=M, mu=MU, ind_idx=idx)
    assert [len(x) for x in want] == list(per_chr), (what, list(per_chr))
    flat = np.concatenate(want)
    assert feed.shape == flat.shape, what
    assert ol.bits_equal(feed, flat), (what, ol.count_mismatch(feed, flat))
    got_form, doubles = panel.feed_info()
    assert got_form == form, (what, got_form)
    sizes = [s.shape[1] for s in scores]
    if form == abi.FEED_SAMPLED_WLOD:
        assert doubles == cases.thinned_doubles(sizes, panel.nind, step), what
    elif form == abi.FEED_FROM_SCORES:
        assert doubles == panel.out_layout(32, panel.nind)[2], what
    return feed


# ------------------------------------------------------------------------------------------------ 1. shapes

@pytest.mark.parametrize("W", cases.WIDTHS)
def test_shapes(gpu_ctx, W):
    """chromosomes of 1, W-1, W, W+1, W+33 SNPs, gaps and a centromere; 1 .. 200 individuals; step = W and beyond"""
    nind = cases.nind_of(W)
    sizes = cases.chrom_sizes(W)
    chroms, gpos, lds = cases.make_case(W, nind, 5100 + W)
    scores = cases.wlod_scores(chroms, gpos, lds, W)
    with open_panel(gpu_ctx, chroms, nind, gpos, W, lds) as panel:
        for step in cases.steps_of(W, sizes):
            check_feed(panel, scores, W, step, ("shape", W, step, nind))


# ------------------------------------------------------------------------------------------------ 2. likelihoods

@pytest.mark.parametrize("kind", ["codes", "continuous"])
@pytest.mark.parametrize("W", cases.GL_WIDTHS)
def test_likelihoods(gpu_ctx, W, kind):
    """dictionary codes and continuous values: the scaled term matrix instead of the score rows; then without"""
    nind = 130 if W % 4 else 65
    sizes = cases.chrom_sizes(W)
    chroms, gpos, lds = cases.make_case(W, nind, 5300 + W)
    gl = cases.likelihoods(np.random.default_rng(5400 + W), chroms, kind)
    with open_panel(gpu_ctx, chroms, nind, gpos, W, lds) as panel:
        panel.set_gl(np.concatenate(gl, axis=0))
        assert panel.tgls_mode()[0] == (1 if kind == "codes" else 2)
        scores = cases.wlod_scores(chroms, gpos, lds, W, gl=gl)
        for step in (W, W + 7):
            check_feed(panel, scores, W, step, ("gl", kind, W, step), use_gl=True)
        plain = cases.wlod_scores(chroms, gpos, lds, W)
        check_feed(panel, plain, W, W, ("gl panel, plain scores", kind, W))
        check_feed(panel, scores, W, W, ("gl again", kind, W), use_gl=True)


# ------------------------------------------------------------------------------------------------ 3. subsets

@pytest.mark.parametrize("W", [10, 100])
def test_subsets(gpu_ctx, W):
    """an unordered list that leaves whole 64-individual blocks out (1 and 3 of four), and a list of one"""
    nind = 200
    sizes = cases.chrom_sizes(W)
    chroms, gpos, lds = cases.make_case(W, nind, 5500 + W)
    gl = cases.likelihoods(np.random.default_rng(5600 + W), chroms, "codes")
    with open_panel(gpu_ctx, chroms, nind, gpos, W, lds) as panel:
        panel.set_gl(np.concatenate(gl, axis=0))
        for use_gl in (False, True):
            scores = cases.wlod_scores(chroms, gpos, lds, W, gl=gl if use_gl else None)
            for idx in (np.array([130, 3, 190, 129, 0]), np.array([77]), np.array([199, 64])):
                check_feed(panel, scores, W, W, ("subset", W, use_gl, list(idx)), use_gl=use_gl, idx=idx)
            check_feed(panel, scores, W, W, ("everyone after subsets", W, use_gl), use_gl=use_gl)


# ------------------------------------------------------------------------------------------------ 4. dropped by value

@pytest.mark.parametrize("W", [5, 60, 300])
def test_nonfinite_terms_and_weights(gpu_ctx, W):
    """--error 0 and a NaN frequency (infinite and NaN terms), LD weights of 0 and inf (weights inf and 0): the sums
    are the reference's infinities and NaNs, and the feed drops NaN and -9999 by value"""
    nind = 70 if W % 2 else 130
    sizes = cases.chrom_sizes(W) + [2 * W + 100]
    chroms, gpos, lds = cases.make_case(W, nind, 5700 + W, sizes=sizes)
    chroms[-1][1][W + 7] = np.nan
    rng = np.random.default_rng(5800 + W)
    with open_panel(gpu_ctx, chroms, nind, gpos, W, lds) as panel:
        for error in (0.0, ERROR):
            scores = cases.wlod_scores(chroms, gpos, lds, W, error=error)
            allw = np.concatenate([s.ravel() for s in scores])
            assert np.isnan(allw).any()
            feed = check_feed(panel, scores, W, W, ("non-finite terms", W, error), error=error)
            assert not np.isnan(feed).any()
        special = [ld.copy() for ld in lds]
        for ld in special:                               # a zero and an infinity in every few rows
            n = ld.shape[0]
            ld[rng.integers(0, n, size=max(1, n // 5)), rng.integers(0, W, size=max(1, n // 5))] = 0.0
            ld[rng.integers(0, n, size=max(1, n // 5)), rng.integers(0, W, size=max(1, n // 5))] = np.inf
        special[4][0, 0] = 0.0                           # ... and in sampled windows for certain
        special[5][0, 1] = np.inf
        panel.set_ld(W, np.concatenate(special, axis=0))
        scores = cases.wlod_scores(chroms, gpos, special, W)
        sampled = np.concatenate([s[:, ::W].ravel() for s in scores])
        assert (np.isinf(sampled) | np.isnan(sampled)).any()
        check_feed(panel, scores, W, W, ("weights 0 and inf", W))


# ------------------------------------------------------------------------------------------------ 5. which path

def test_feed_info_tells_the_path(gpu_ctx, monkeypatch):
    W, nind = 60, 65
    sizes = cases.chrom_sizes(W)
    chroms, gpos, lds = cases.make_case(W, nind, 5900)
    scores = cases.wlod_scores(chroms, gpos, lds, W)
    with open_panel(gpu_ctx, chroms, nind, gpos, W, lds) as panel:
        full = panel.out_layout(32, nind)[2]
        check_feed(panel, scores, W, W, "sampled")
        assert panel.feed_info() == (abi.FEED_SAMPLED_WLOD, cases.thinned_doubles(sizes, nind, W))
        assert panel.feed_info()[1] < full // 8          # (every chromosome's columns are padded to 32: not W times smaller here)
        check_feed(panel, scores, W, 1, "step 1", form=abi.FEED_FROM_SCORES)
        assert panel.feed_info() == (abi.FEED_FROM_SCORES, full)
        check_feed(panel, scores, W, W - 1, "overlapping samples", form=abi.FEED_FROM_SCORES)
        monkeypatch.setenv("GARLIC_WLOD_FEED_FULL", "1")
        check_feed(panel, scores, W, W, "forced full", form=abi.FEED_FROM_SCORES)
        assert panel.feed_info() == (abi.FEED_FROM_SCORES, full)
        monkeypatch.delenv("GARLIC_WLOD_FEED_FULL")
        check_feed(panel, scores, W, 2 * W, "sampled again")
        # unweighted, step = W: the chain stores only the samples
        want = [ol.oracle_flatten(ol.oracle_calc_lod(g, f, p, cs, ce, W, ERROR, MG), W) for (g, f, p, cs, ce) in chroms]
        feed, per_chr = panel.lod_feed(W, ERROR, MG, W)
        assert ol.bits_equal(feed, np.concatenate(want)) and len(feed) > 0
        assert panel.feed_info()[0] == abi.FEED_CHAIN
        # ... and the full weighted scores after a thinned call of the same window size are not served by its plan
        got = panel.wlod_windows(W, ERROR, MG, M, MU, pitch_align=32)
        for c in range(len(sizes)):
            assert ol.bits_equal(np.ascontiguousarray(got[c]), scores[c]), c


# ------------------------------------------------------------------------------------------------ 6. switch, repeats

@pytest.mark.parametrize("seed", [1, 2, 3])
def test_same_bytes_with_and_without_the_switch(gpu_ctx, seed, monkeypatch):
    """random panels (window, step, individuals, likelihoods drawn): GARLIC_WLOD_FEED_FULL=1 and the sampled path give
    the oracle's bytes both"""
    rng = np.random.default_rng(20260500 + seed)
    W = int(rng.choice([4, 7, 10, 23, 64, 150]))
    nind = int(rng.integers(1, 260))
    step = W + int(rng.choice([0, 0, 1, 13, W]))
    sizes = [int(rng.integers(W + 40, 2500)) for _ in range(int(rng.integers(1, 5)))] + [int(rng.integers(1, W + 3))]
    use_gl = bool(rng.integers(0, 2))
    rp = np.random.default_rng(int(rng.integers(1 << 30)))
    chroms = [ol.random_panel(rp, n, nind, max_gap=MG, gaps=int(rng.integers(0, 3))) for n in sizes]
    gpos = [np.cumsum(np.diff(c[2], prepend=0) * 1e-6 * rp.uniform(0.8, 1.2, size=c[2].shape[0])) for c in chroms]
    lds = [rp.uniform(1.0, max(2.0, W / 4.0), size=(n, W)) for n in sizes]
    gl = cases.likelihoods(rp, chroms, "codes" if seed % 2 else "continuous") if use_gl else None
    scores = cases.wlod_scores(chroms, gpos, lds, W, gl=gl)
    idx = rp.permutation(nind)[: max(1, nind // 3)]
    with open_panel(gpu_ctx, chroms, nind, gpos, W, lds) as panel:
        if use_gl:
            panel.set_gl(np.concatenate(gl, axis=0))
        a = check_feed(panel, scores, W, step, ("sampled", seed), use_gl=use_gl)
        a_sub = check_feed(panel, scores, W, step, ("sampled subset", seed), use_gl=use_gl, idx=idx)
        monkeypatch.setenv("GARLIC_WLOD_FEED_FULL", "1")
        b = check_feed(panel, scores, W, step, ("full", seed), use_gl=use_gl, form=abi.FEED_FROM_SCORES)
        b_sub = check_feed(panel, scores, W, step, ("full subset", seed), use_gl=use_gl, idx=idx, form=abi.FEED_FROM_SCORES)
        assert ol.bits_equal(a, b) and ol.bits_equal(a_sub, b_sub)


def test_twenty_launches_identical(gpu_ctx):
    W, nind = 100, 200
    chroms, gpos, lds = cases.make_case(W, nind, 6100)
    gl = cases.likelihoods(np.random.default_rng(6101), chroms, "continuous")
    with open_panel(gpu_ctx, chroms, nind, gpos, W, lds) as panel:
        panel.set_gl(np.concatenate(gl, axis=0))
        for use_gl in (False, True):
            scores = cases.wlod_scores(chroms, gpos, lds, W, gl=gl if use_gl else None)
            first = check_feed(panel, scores, W, W, ("first", use_gl), use_gl=use_gl)
            for k in range(20):
                feed, _ = panel.lod_feed(W, ERROR, MG, W, use_gl=use_gl, weighted=True, M=M, mu=MU)
                assert ol.bits_equal(feed, first), (use_gl, k)
                assert panel.feed_info()[0] == abi.FEED_SAMPLED_WLOD


# ------------------------------------------------------------------------------------------------ 7. memory

def score_chunk_bytes():
    """the size of the physical chunks score memory is made of, from the allocator's source"""
    src = open(os.path.join(ROOT, "garlic_amd", "csrc", "garlic_hip.hip")).read()
    m = re.search(r"const size_t chunk = \(\(\(size_t\)1 << (\d+)\) \+ gran - 1\) / gran \* gran;", src)
    assert m, "score_alloc's chunk size not found"
    return 1 << int(m.group(1))


def test_score_memory_is_the_thinned_matrix(gpu_ctx, monkeypatch):
    """A panel whose full score matrix (1.2 GB) is larger than one chunk of the score allocator: after
    release_scratch and trim the weighted step = W feed may raise live + pooled score memory by the thinned matrix
    rounded up to the chunk size and no more -- the full matrix does not fit in that -- and under
    GARLIC_WLOD_FEED_FULL=1 the same call takes at least the full matrix (so the library's score scratch is counted
    by garlic_device_alloc_stats, and the bound above is a real one)."""
    W, nloci, nind = 100, 60000, 2500
    rng = np.random.default_rng(6200)
    geno = rng.integers(0, 3, size=(nloci, nind), dtype=np.int16)
    geno[rng.random(nloci) < 0.01, :] = -9
    geno[::97, ::13] = -9
    pos = np.cumsum(rng.integers(1, 4000, size=nloci)).astype(np.int32)
    gpos = pos * 1e-6
    freq = rng.uniform(0.05, 0.95, size=nloci)
    ld = rng.uniform(1.0, 20.0, size=(nloci, W))
    chunk = score_chunk_bytes()
    with abi.Panel(gpu_ctx, [nloci], nind) as panel:
        panel.set_map(pos, [0], [0], gpos=gpos)
        panel.set_freq(freq)
        panel.set_genotypes(geno)
        panel.set_ld(W, ld)
        full = panel.out_layout(32, nind)[2] * 8
        thin = cases.thinned_doubles([nloci], nind, W) * 8
        assert full > chunk and thin < full // 50
        bound = (thin + chunk - 1) // chunk * chunk
        panel.release_scratch()
        gpu_ctx.trim()
        live0, pooled0, _ = gpu_ctx.alloc_stats()
        feed, per_chr = panel.lod_feed(W, ERROR, MG, W, weighted=True, M=M, mu=MU)
        assert len(feed) > 0 and len(feed) == per_chr[0]
        assert panel.feed_info() == (abi.FEED_SAMPLED_WLOD, thin // 8)
        live1, pooled1, _ = gpu_ctx.alloc_stats()
        print("score memory: before %d, after the sampled feed %d (thinned matrix %d, full %d, chunk %d)"
              % (live0 + pooled0, live1 + pooled1, thin, full, chunk))
        assert live1 + pooled1 - (live0 + pooled0) <= bound
        # the sampled windows against the oracle, for a few individuals
        some = np.array([0, 1, 777, nind - 1])
        want = ol.oracle_calc_wlod(geno[:, some], freq, pos, gpos, ld, 0, 0, W, ERROR, MG, MU, M, threads=8)
        got, _ = panel.lod_feed(W, ERROR, MG, W, weighted=True, M=M, mu=MU, ind_idx=some)
        assert ol.bits_equal(got, ol.oracle_flatten(want, W))
        monkeypatch.setenv("GARLIC_WLOD_FEED_FULL", "1")
        panel.release_scratch()
        gpu_ctx.trim()
        live0, pooled0, _ = gpu_ctx.alloc_stats()
        feed_full, _ = panel.lod_feed(W, ERROR, MG, W, weighted=True, M=M, mu=MU)
        live2, pooled2, _ = gpu_ctx.alloc_stats()
        print("score memory under GARLIC_WLOD_FEED_FULL=1: before %d, after %d" % (live0 + pooled0, live2 + pooled2))
        assert live2 + pooled2 - (live0 + pooled0) >= full
        assert ol.bits_equal(feed, feed_full)
        panel.release_scratch()
    gpu_ctx.trim()
