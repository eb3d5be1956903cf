"""GPU: weighted scores from dictionary-coded likelihoods with the scaled term matrix built and read slab by slab
(garlic_panel_set_tgls_term_budget): full scores to host and device, an aligned sub-range, the sampled KDE feed (everyone
and individual lists) and the feed from scores, coverage counts and ROH segments -- bit for bit against the oracle and
against the same calls over the whole scaled matrix (budget 0) on the same panel.  No tolerance.
garlic_panel_tgls_terms_info after every call: the term buffers hold no more than the budget and the call ran the slabs
tests/tgls_slab_cases.py counts (test_wlod_slabs_cpu.py pins those counts: 4, 1, 4, 3 for everyone).

Widths 10, 100, 200, 260: the stream form, the 80-VGPR strip, the wide strip and the ring tile form.  200 individuals under
a budget of two blocks run one-block slabs -- every pair of the strip form and every group of the tile and stream forms
loses its partners --, under four blocks one slab; 456 individuals run slabs of 2 and of 3 (3 + 3 + 2)."""
import numpy as np
import pytest

import oracle_lib as ol
import tgls_feed_cases as fcases
import wlod_slab_cases as cases
from garlic_amd import abi
from test_gpu_window_regimes import device_rows

pytestmark = pytest.mark.gpu
MG, ERROR, FRAC, M, MU = cases.MG, cases.ERROR, cases.FRAC, cases.M, cases.MU


def open_panel(ctx, chroms, nind, gpos, W, lds, codes=None, gl=None):
    panel = abi.Panel(ctx, [c[0].shape[0] for c in chroms], nind)
    panel.set_map(np.concatenate([c[2] for c in chroms]), [c[3] for c in chroms], [c[4] for c in chroms], gpos=np.concatenate(gpos))
    panel.set_freq(np.concatenate([c[1] for c in chroms]))
    panel.set_genotypes(np.concatenate([c[0] for c in chroms], axis=0))
    panel.set_ld(W, np.concatenate(lds, axis=0))
    if codes is not None:
        panel.set_gl_codes(np.concatenate(codes, axis=0), cases.VALUES)
    elif gl is not None:
        panel.set_gl(np.concatenate(gl, axis=0))
    return panel


def check_info(panel, nloci, budget, blocks, what, reruns=0):
    """the slabs of the call that just returned; blocks: the 64-individual blocks it scored, None: its terms are looked up"""
    info = panel.tgls_terms_info()
    whole = (cases.ROWS_PAD + nloci) * cases.nind_pad_of(panel.nind) * 8
    print(what, "budget", budget, info)
    assert info["whole_bytes"] == whole, what
    if budget > 0:
        assert info["resident_bytes"] <= budget, (what, info)
    st = panel.stats()
    assert st["n_stall_reruns"] == reruns and st["n_count_timeouts"] == 0, (what, st["n_stall_reruns"])
    if budget == 0 or budget >= whole:
        assert info["n_slabs"] == 0 and info["resident_bytes"] == whole, (what, info)
        return info
    if blocks is None:
        assert info["n_slabs"] == 0, (what, info)
        return info
    s = info["slab_blocks"]
    assert s == cases.slab_blocks_for(budget, nloci, panel.nind) and s >= 1, (what, info)
    assert info["n_slabs"] == cases.n_slabs_of(blocks, s) >= 1, (what, info, blocks)
    return info


def score_scratch(ctx):
    live, pooled, _ = ctx.alloc_stats()
    return live + pooled


def same(got, want, what):
    for c in range(len(want)):
        g = np.ascontiguousarray(got[c])
        w = np.ascontiguousarray(want[c])
        assert ol.bits_equal(g, w), (what, c, ol.count_mismatch(g, w))


def all_calls(panel, chroms, scores, W, budget, what, subsets, sub_range):
    """every covered call once, each against the oracle; returns their bytes for the comparison between budgets"""
    nind, sizes = panel.nind, [c[0].shape[0] for c in chroms]
    nloci = sum(sizes)
    everyone = cases.blocks_of(nind)
    res = {}

    got = panel.wlod_windows(W, ERROR, MG, M, MU, use_gl=True, pitch_align=1)
    same(got, scores, (what, "host scores"))
    check_info(panel, nloci, budget, everyone, (what, "host scores"))
    res["host"] = np.concatenate([np.ascontiguousarray(g).ravel() for g in got])

    got = device_rows(panel, sizes, nind, 32, lambda ptr: panel.wlod_windows_device(ptr, W, ERROR, MG, M, MU, pitch_align=32, use_gl=True))
    same(got, scores, (what, "device scores"))
    check_info(panel, nloci, budget, everyone, (what, "device scores"))
    res["device"] = np.concatenate([np.ascontiguousarray(g).ravel() for g in got])

    b, n = sub_range
    got = panel.wlod_windows(W, ERROR, MG, M, MU, ind_begin=b, ind_count=n, use_gl=True, pitch_align=32)
    same(got, [s[b: b + n] for s in scores], (what, "sub-range"))
    check_info(panel, nloci, budget, cases.blocks_of(nind, sub=sub_range), (what, "sub-range"))
    res["sub"] = np.concatenate([np.ascontiguousarray(g).ravel() for g in got])

    full = panel.out_layout(32, nind)[2]
    for idx in [None] + [np.array(x) for x in subsets]:
        want = cases.flat(scores, W, idx)
        assert sum(len(x) for x in want) > 0
        feed, per_chr = panel.lod_feed(W, ERROR, MG, W, use_gl=True, weighted=True, M=M, mu=MU, ind_idx=idx)
        tag = ("feed", W, None if idx is None else list(idx))
        assert [len(x) for x in want] == list(per_chr), (what, tag)
        assert ol.bits_equal(feed, np.concatenate(want)), (what, tag)
        assert panel.feed_info() == (abi.FEED_SAMPLED_WLOD, cases.thinned_doubles(sizes, nind, W)), (what, tag, panel.feed_info())
        check_info(panel, nloci, budget, everyone if idx is None else cases.blocks_of(nind, idx=idx), (what, tag))
        res[str(tag)] = (feed, panel.feed_info())
    # ... and from full scores (overlapping samples)
    feed, _ = panel.lod_feed(W, ERROR, MG, 3, use_gl=True, weighted=True, M=M, mu=MU)
    assert len(feed) > 0 and ol.bits_equal(feed, np.concatenate(cases.flat(scores, 3)))
    assert panel.feed_info() == (abi.FEED_FROM_SCORES, full)
    check_info(panel, nloci, budget, everyone, (what, "feed from scores"))
    res["feed3"] = (feed, panel.feed_info())

    # coverage counts and segments from the tuned kernels' bits: the calls draw bit matrices and segment lists from the score
    # pool, a 64th of the scores and less; the generic kernel's fallback would reserve the full score matrix there
    cutoff = cases.cutoff_of(scores)
    panel.release_scratch()
    panel.ctx.trim()
    before = score_scratch(panel.ctx)
    cov = panel.roh_coverage_fused(W, ERROR, MG, cutoff, pitch_align=8, use_gl=True, weighted=True, M=M, mu=MU)
    covered = 0
    for c, n_c in enumerate(sizes):
        want = ol.oracle_roh_coverage(np.ascontiguousarray(scores[c]), W, cutoff)
        assert np.array_equal(cov[c][:, :n_c], want), (what, "coverage", c)
        covered += int(np.count_nonzero(want))
    assert covered > 0
    check_info(panel, nloci, budget, everyone, (what, "coverage"))
    segs = [tuple(int(v) for v in r) for r in panel.roh_segments(W, ERROR, MG, cutoff, FRAC, use_gl=True, weighted=True, M=M, mu=MU)]
    want = cases.oracle_segments(chroms, scores, W, cutoff)
    assert len(want) > 0 and segs == want, (what, "segments", len(segs), len(want))
    check_info(panel, nloci, budget, everyone, (what, "segments"))
    assert score_scratch(panel.ctx) - before < full * 8 // 4, (what, "coverage / segments took a score matrix")
    res["cov scratch"] = np.array([score_scratch(panel.ctx) - before])      # ... and the same with and without slabs
    res["cov"] = np.concatenate([np.ascontiguousarray(x[:, :n_c]).ravel() for x, n_c in zip(cov, sizes)])
    res["segs"] = segs
    return res


def assert_same_results(a, b, what):
    assert a.keys() == b.keys()
    for k in a:
        if isinstance(a[k], tuple):        # (feed, feed_info): same bytes, same form and score scratch
            assert ol.bits_equal(a[k][0], b[k][0]) and a[k][1] == b[k][1], (what, k, a[k][1], b[k][1])
        elif isinstance(a[k], list):
            assert a[k] == b[k], (what, k)
        elif a[k].dtype == np.float64:
            assert ol.bits_equal(a[k], b[k]), (what, k)
        else:
            assert np.array_equal(a[k], b[k]), (what, k)


# ------------------------------------------------------------------------------------------------ 1. every call, every budget

@pytest.mark.parametrize("W", cases.WIDTHS)
def test_every_weighted_call_under_every_budget(gpu_ctx, W):
    """budget 0, then slabs of 1 block, one slab of the 4 blocks, then a budget at whole_bytes"""
    nind = cases.NIND
    chroms, codes, gl, gpos, lds = cases.case(W)
    scores = cases.scores_of(W)
    nloci = sum(c[0].shape[0] for c in chroms)
    with open_panel(gpu_ctx, chroms, nind, gpos, W, lds, codes) as panel:
        assert panel.tgls_mode()[0] == 1
        base = all_calls(panel, chroms, scores, W, 0, (W, "budget 0"), cases.SUBSETS, cases.SUB_RANGE)
        whole = panel.tgls_terms_info()["whole_bytes"]
        for k, budget in cases.budgets_of(nloci, nind) + [(0, whole)]:
            assert budget == whole or (budget < whole and cases.slab_blocks_for(budget, nloci, nind) == k)
            panel.set_tgls_term_budget(budget)
            got = all_calls(panel, chroms, scores, W, budget, (W, k, "blocks per slab"), cases.SUBSETS, cases.SUB_RANGE)
            assert_same_results(base, got, (W, k))


def test_two_and_three_block_slabs_on_eight_blocks(gpu_ctx):
    """456 individuals = 8 blocks under slabs of 2 and of 3 (3 + 3 + 2); the sub-range [64, 64 + 300) = blocks 1 .. 5 runs
    2 + 2 + 1 and 3 + 2"""
    W, nind = cases.WIDE_W, cases.NIND_WIDE
    chroms, codes, gl, gpos, lds = cases.case(W, nind)
    scores = cases.scores_of(W, nind)
    nloci = sum(c[0].shape[0] for c in chroms)
    with open_panel(gpu_ctx, chroms, nind, gpos, W, lds, codes) as panel:
        base = all_calls(panel, chroms, scores, W, 0, (W, "wide, budget 0"), cases.WIDE_SUBSETS, (64, 300))
        for k, budget in cases.budgets_of(nloci, nind):
            panel.set_tgls_term_budget(budget)
            got = all_calls(panel, chroms, scores, W, budget, (W, "wide", k, "blocks per slab"), cases.WIDE_SUBSETS, (64, 300))
            assert_same_results(base, got, (W, "wide", k))
            panel.wlod_windows(W, ERROR, MG, M, MU, use_gl=True)
            info = panel.tgls_terms_info()
            assert (info["slab_blocks"], info["n_slabs"]) == (k, -(-8 // k))


# ------------------------------------------------------------------------------------------------ 2. shapes that look up

GENERIC_MAX_W = 250        # the generic kernel's LDS ring: 8 ((W + 32) 64 + W + 64 * 34) bytes <= 160 KB


@pytest.mark.parametrize("W", cases.WIDTHS)
def test_unaligned_sub_range_looks_its_terms_up(gpu_ctx, W, monkeypatch):
    """a range that begins inside a block, and GARLIC_WLOD_GENERIC: under a budget nothing is built -- no slabs, no whole
    matrix past the bound -- and the scores are the oracle's.  Windows too wide for the generic kernel (W = 260) are refused
    there, as GARLIC_WLOD_GENERIC refuses them without a budget, and the panel stays usable."""
    nind = cases.NIND
    chroms, codes, gl, gpos, lds = cases.case(W)
    scores = cases.scores_of(W)
    nloci = sum(c[0].shape[0] for c in chroms)
    budget = cases.budget_for(nloci, 1, nind)
    b, n = cases.UNALIGNED_RANGE

    def looked_up(what, **kw):
        if W > GENERIC_MAX_W:
            with pytest.raises(abi.GarlicError) as e:
                panel.wlod_windows(W, ERROR, MG, M, MU, use_gl=True, pitch_align=32, **kw)
            assert e.value.code == abi.ERR_INVALID and "winsize" in str(e.value), (W, what)
        else:
            got = panel.wlod_windows(W, ERROR, MG, M, MU, use_gl=True, pitch_align=32, **kw)
            lo, cnt = kw.get("ind_begin", 0), kw.get("ind_count", nind)
            same(got, [s[lo: lo + cnt] for s in scores], (W, what))
        check_info(panel, nloci, budget, None, (W, what))

    with open_panel(gpu_ctx, chroms, nind, gpos, W, lds, codes) as panel:
        panel.wlod_windows(W, ERROR, MG, M, MU, use_gl=True)            # a whole scaled matrix from before the budget
        panel.set_tgls_term_budget(budget)
        looked_up("unaligned", ind_begin=b, ind_count=n)
        got = panel.wlod_windows(W, ERROR, MG, M, MU, use_gl=True, pitch_align=32)          # slabs again
        same(got, scores, (W, "everyone after the unaligned range"))
        check_info(panel, nloci, budget, cases.blocks_of(nind), (W, "everyone after the unaligned range"))
        monkeypatch.setenv("GARLIC_WLOD_GENERIC", "1")
        looked_up("generic")


def test_continuous_panel_ignores_the_budget(gpu_ctx):
    W, nind = 100, cases.NIND
    chroms, _, _, gpos, lds = cases.case(W)
    gl = fcases.bounded_likelihoods(np.random.default_rng(9400), chroms, "continuous")
    assert len(np.unique(np.concatenate([g.ravel() for g in gl]))) > 256
    scores = [ol.oracle_calc_wlod(g, f, p, gpos[c], lds[c], cs, ce, W, ERROR, MG, MU, M, gl=gl[c], threads=8)
              for c, (g, f, p, cs, ce) in enumerate(chroms)]
    nloci = sum(c[0].shape[0] for c in chroms)
    with open_panel(gpu_ctx, chroms, nind, gpos, W, lds, None, gl) as panel:
        assert panel.tgls_mode()[0] == 2
        panel.set_tgls_term_budget(cases.budget_for(nloci, 1, nind))
        got = panel.wlod_windows(W, ERROR, MG, M, MU, use_gl=True)
        same(got, scores, "continuous")
        info = panel.tgls_terms_info()
        assert info["n_slabs"] == 0 and info["whole_bytes"] == (cases.ROWS_PAD + nloci) * cases.nind_pad_of(nind) * 8
        feed, _ = panel.lod_feed(W, ERROR, MG, W, use_gl=True, weighted=True, M=M, mu=MU)
        assert len(feed) > 0 and ol.bits_equal(feed, np.concatenate(cases.flat(scores, W)))
        assert panel.feed_info()[0] == abi.FEED_SAMPLED_WLOD and panel.tgls_terms_info()["n_slabs"] == 0


# ------------------------------------------------------------------------------------------------ 3. sequences on one panel

def test_both_kinds_two_scales_and_the_budget_in_sequence(gpu_ctx):
    """unweighted, weighted (7, 1e-9), weighted (3, 2e-9), unweighted again on the same two slab buffers; then the budget
    raised above the whole matrix and lowered again"""
    W, nind = 100, cases.NIND
    chroms, codes, gl, gpos, lds = cases.case(W)
    nloci = sum(c[0].shape[0] for c in chroms)
    small = cases.budget_for(nloci, 1, nind)
    everyone = cases.blocks_of(nind)
    plain = cases.unweighted_scores_of(W)
    scaled = {(M, MU): cases.scores_of(W), (cases.M2, cases.MU2): cases.scores_of(W, nind, cases.M2, cases.MU2)}

    def unweighted(panel, budget, what):
        same(panel.lod_windows(W, ERROR, MG, use_gl=True), plain, what)
        check_info(panel, nloci, budget, everyone, what)

    def weighted(panel, m, mu, budget, what):
        same(panel.wlod_windows(W, ERROR, MG, m, mu, use_gl=True), scaled[(m, mu)], what)
        check_info(panel, nloci, budget, everyone, what)
        feed, _ = panel.lod_feed(W, ERROR, MG, W, use_gl=True, weighted=True, M=m, mu=mu)
        assert len(feed) > 0 and ol.bits_equal(feed, np.concatenate(cases.flat(scaled[(m, mu)], W))), (what, "feed")
        check_info(panel, nloci, budget, everyone, (what, "feed"))

    with open_panel(gpu_ctx, chroms, nind, gpos, W, lds, codes) as panel:
        whole = panel.tgls_terms_info()["whole_bytes"]
        panel.set_tgls_term_budget(small)
        unweighted(panel, small, "1. unweighted")
        weighted(panel, M, MU, small, "2. weighted (7, 1e-9)")
        weighted(panel, cases.M2, cases.MU2, small, "3. weighted (3, 2e-9)")
        unweighted(panel, small, "4. unweighted again")
        panel.set_tgls_term_budget(whole + 4096)                  # 5. both kinds read a whole matrix
        weighted(panel, M, MU, whole + 4096, "5. weighted, whole matrix")
        unweighted(panel, whole + 4096, "5. unweighted, whole matrix")
        weighted(panel, cases.M2, cases.MU2, whole + 4096, "5. weighted (3, 2e-9), whole matrix")
        panel.set_tgls_term_budget(small)                         # 6. the whole matrix goes, slabs return
        assert panel.tgls_terms_info()["resident_bytes"] <= small
        weighted(panel, M, MU, small, "6. weighted, slabs again")
        unweighted(panel, small, "6. unweighted, slabs again")


def test_forced_rerun_reads_its_own_slab(gpu_ctx, monkeypatch):
    """GARLIC_WLOD_STRIP_FORCE_RERUN under one-block slabs: the tile form behind every strip launch runs, over the slab its
    strip launch read, before that buffer is rebuilt -- the oracle's scores, one rerun per slab"""
    W, nind = 100, cases.NIND
    chroms, codes, gl, gpos, lds = cases.case(W)
    scores = cases.scores_of(W)
    nloci = sum(c[0].shape[0] for c in chroms)
    budget = cases.budget_for(nloci, 1, nind)
    with open_panel(gpu_ctx, chroms, nind, gpos, W, lds, codes) as panel:
        panel.set_tgls_term_budget(budget)
        same(panel.wlod_windows(W, ERROR, MG, M, MU, use_gl=True, pitch_align=32), scores, "strip form")
        n_slabs = check_info(panel, nloci, budget, cases.blocks_of(nind), "strip form")["n_slabs"]
        assert n_slabs == 4
        monkeypatch.setenv("GARLIC_WLOD_STRIP_FORCE_RERUN", "1")
        for k in (1, 2):
            same(panel.wlod_windows(W, ERROR, MG, M, MU, use_gl=True, pitch_align=32), scores, ("forced rerun", k))
            check_info(panel, nloci, budget, cases.blocks_of(nind), ("forced rerun", k), reruns=k * n_slabs)
        monkeypatch.delenv("GARLIC_WLOD_STRIP_FORCE_RERUN")
        same(panel.wlod_windows(W, ERROR, MG, M, MU, use_gl=True, pitch_align=32), scores, "strip form again")
        check_info(panel, nloci, budget, cases.blocks_of(nind), "strip form again", reruns=2 * n_slabs)
