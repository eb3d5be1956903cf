"""GPU: unweighted scores from dictionary-coded likelihoods with the term matrix built and read slab by slab
(garlic_panel_set_tgls_term_budget): full scores to host and device, the KDE feed (sampled ring form and from scores),
coverage counts and ROH segments, bit for bit against the oracle and against the same calls over the whole matrix
(budget 0) on the same panel.  No tolerance.  garlic_panel_tgls_terms_info after every call: the term buffers hold no
more than the budget and the call ran ceil(blocks / slab_blocks) slabs (a subset feed: the slabs that hold a listed
block, tgls_slab_cases.n_slabs_of).

Budgets.  The slabs of a call alternate between two buffers (one is built while the other is read): slabs of k blocks
cost k + min(k, nblk - k) blocks, and the library takes the largest k that fits.  On the 200-individual panel (nblk = 4;
its whole matrix has a pad block, 5) that gives slabs of 1 block (budget 2 blocks) or one slab of all 4 (budget 4 blocks),
never slabs of 2 or 3: 2 + 2 and 3 + 1 cost the same 4 blocks as the single slab, which is what the library then takes.
So slabs of 2 blocks, and of 3 with the uneven splits 3 + 3 + 2 and (a sub-range of five blocks) 3 + 2, run on a panel of
456 individuals (nblk = 8)."""
import numpy as np
import pytest

import oracle_lib as ol
import tgls_feed_cases as fcases
import tgls_slab_cases as cases
from garlic_amd import abi
from test_gpu_window_regimes import device_rows

pytestmark = pytest.mark.gpu
MG, ERROR, FRAC = cases.MG, cases.ERROR, cases.FRAC
TGLS_CHAIN = abi.FEED_TGLS_CHAIN


def open_panel(ctx, chroms, nind, codes=None, gl=None):
    panel = abi.Panel(ctx, [c[0].shape[0] for c in chroms], nind)
    panel.set_map(np.concatenate([c[2] for c in chroms]), [c[3] for c in chroms], [c[4] for c in chroms])
    panel.set_freq(np.concatenate([c[1] for c in chroms]))
    panel.set_genotypes(np.concatenate([c[0] for c in chroms], axis=0))
    if codes is not None:
        panel.set_gl_codes(np.concatenate(codes, axis=0), cases.VALUES)
    elif gl is not None:
        panel.set_gl(np.concatenate(gl, axis=0))
    return panel


def check_info(panel, nloci, budget, blocks, what):
    """the slabs of the call that just returned; blocks: the 64-individual blocks it scored"""
    info = panel.tgls_terms_info()
    nind_pad = cases.nind_pad_of(panel.nind)
    whole = (cases.ROWS_PAD + nloci) * nind_pad * 8
    print(what, "budget", budget, info)
    assert info["whole_bytes"] == whole, what
    if budget > 0:
        assert info["resident_bytes"] <= budget, (what, info)
    if budget == 0 or budget >= whole:
        assert info["n_slabs"] == 0 and info["resident_bytes"] == whole, (what, info)
        return
    s = info["slab_blocks"]
    assert s == cases.slab_blocks_for(budget, nloci, panel.nind) and s >= 1, (what, info)
    assert info["n_slabs"] == cases.n_slabs_of(blocks, s) >= 1, (what, info, blocks)
    if blocks == list(range(blocks[0], blocks[-1] + 1)):
        assert info["n_slabs"] == -(-len(blocks) // s), (what, info)
    st = panel.stats()
    assert st["n_stall_reruns"] == 0 and st["n_count_timeouts"] == 0, what


def score_scratch(ctx):
    live, pooled, _ = ctx.alloc_stats()
    return live + pooled


def all_calls(panel, chroms, scores, W, budget, what, subsets=cases.SUBSETS, sub_range=cases.SUB_RANGE):
    """every covered call once, each against the oracle; returns their bytes for the comparison between budgets"""
    nind, sizes = panel.nind, [c[0].shape[0] for c in chroms]
    nloci = sum(sizes)
    everyone = cases.blocks_of(nind)
    res = {}

    def same(got, want, tag):
        for c in range(len(want)):
            g = np.ascontiguousarray(got[c])
            assert ol.bits_equal(g, np.ascontiguousarray(want[c])), (what, tag, c, ol.count_mismatch(g, np.ascontiguousarray(want[c])))

    got = panel.lod_windows(W, ERROR, MG, use_gl=True, pitch_align=1)
    same(got, scores, "host scores")
    check_info(panel, nloci, budget, everyone, (what, "host scores"))
    assert panel.chain_kind() == 0
    res["host"] = np.concatenate([np.ascontiguousarray(g).ravel() for g in got])

    got = device_rows(panel, sizes, nind, 32, lambda ptr: panel.lod_windows_device(ptr, W, ERROR, MG, pitch_align=32, use_gl=True))
    same(got, scores, "device scores")
    check_info(panel, nloci, budget, everyone, (what, "device scores"))
    res["device"] = np.concatenate([np.ascontiguousarray(g).ravel() for g in got])

    b, n = sub_range
    got = panel.lod_windows(W, ERROR, MG, ind_begin=b, ind_count=n, use_gl=True, pitch_align=32)
    same(got, [s[b: b + n] for s in scores], "sub-range")
    check_info(panel, nloci, budget, cases.blocks_of(nind, sub=sub_range), (what, "sub-range"))
    res["sub"] = np.concatenate([np.ascontiguousarray(g).ravel() for g in got])

    full = panel.out_layout(32, nind)[2]
    for step, idx in [(W, None), (4, None)] + [(W, np.array(x)) for x in subsets]:
        want = fcases.flat(scores, step, idx)
        assert sum(len(x) for x in want) > 0
        feed, per_chr = panel.lod_feed(W, ERROR, MG, step, use_gl=True, ind_idx=idx)
        tag = ("feed", step, None if idx is None else list(idx))
        assert [len(x) for x in want] == list(per_chr), (what, tag)
        assert ol.bits_equal(feed, np.concatenate(want)), (what, tag)
        assert panel.feed_info() == (TGLS_CHAIN, fcases.thinned_doubles(sizes, nind, step)), (what, tag, panel.feed_info())
        check_info(panel, nloci, budget, everyone if idx is None else cases.blocks_of(nind, idx=idx), (what, tag))
        res[str(tag)] = (feed, panel.feed_info())
    # ... and from full scores (steps below 4 are sampled from the score scratch)
    feed, _ = panel.lod_feed(W, ERROR, MG, 3, use_gl=True)
    assert len(feed) > 0 and ol.bits_equal(feed, np.concatenate(fcases.flat(scores, 3)))
    assert panel.feed_info() == (abi.FEED_FROM_SCORES, full)
    check_info(panel, nloci, budget, everyone, (what, "feed from scores"))
    res["feed3"] = (feed, panel.feed_info())

    # coverage counts and segments from the chain's bits (the bit form survives the slabs): the calls draw bit matrices and
    # segment lists from the score pool, a 64th of the scores and less; the fallback would reserve the full score matrix there
    cutoff = cases.cutoff_of(scores)
    panel.release_scratch()
    panel.ctx.trim()
    before = score_scratch(panel.ctx)
    cov = panel.roh_coverage_fused(W, ERROR, MG, cutoff, pitch_align=8, use_gl=True)
    covered = 0
    for c, n_c in enumerate(sizes):
        want = ol.oracle_roh_coverage(np.ascontiguousarray(scores[c]), W, cutoff)
        assert np.array_equal(cov[c][:, :n_c], want), (what, "coverage", c)
        covered += int(np.count_nonzero(want))
    assert covered > 0
    check_info(panel, nloci, budget, everyone, (what, "coverage"))
    segs = [tuple(int(v) for v in r) for r in panel.roh_segments(W, ERROR, MG, cutoff, FRAC, use_gl=True)]
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

@pytest.mark.parametrize("feeding", cases.FEEDINGS)
@pytest.mark.parametrize("W", cases.WIDTHS)
def test_every_call_under_every_budget(gpu_ctx, W, feeding):
    """budget 0, then slabs of 1 block, one slab of the 4 blocks, then a budget at whole_bytes"""
    chroms, codes, gl, scores = cases.case(W)
    nloci = sum(c[0].shape[0] for c in chroms)
    with open_panel(gpu_ctx, chroms, cases.NIND, codes if feeding == "set_gl_codes" else None, gl) as panel:
        assert panel.tgls_mode()[0] == 1
        base = all_calls(panel, chroms, scores, W, 0, (W, feeding, "budget 0"))
        whole = panel.tgls_terms_info()["whole_bytes"]
        for k, budget in ((1, cases.budget_for(nloci, 1, cases.NIND)), (4, cases.budget_for(nloci, 4, cases.NIND)), (0, whole)):
            assert budget == whole or (budget < whole and cases.slab_blocks_for(budget, nloci, cases.NIND) == k)
            panel.set_tgls_term_budget(budget)
            got = all_calls(panel, chroms, scores, W, budget, (W, feeding, k, "blocks per slab"))
            assert_same_results(base, got, (W, feeding, k))


@pytest.mark.parametrize("W", cases.WIDTHS)
def test_two_and_three_block_slabs_on_eight_blocks(gpu_ctx, W):
    """456 individuals = 8 blocks under slabs of 2 and of 3 (3 + 3 + 2); the sub-range [64, 64 + 300) = blocks 1 .. 5 runs
    2 + 2 + 1 and 3 + 2"""
    nind = cases.NIND_WIDE
    chroms, codes, gl, scores = cases.case(W, nind)
    nloci = sum(c[0].shape[0] for c in chroms)
    subsets = [[130, 3, 455, 0, 300], [455, 64, 200]]          # blocks {0, 2, 4, 7} and {1, 3, 7}
    with open_panel(gpu_ctx, chroms, nind, codes) as panel:
        base = all_calls(panel, chroms, scores, W, 0, (W, "wide, budget 0"), subsets, (64, 300))
        for k in (2, 3):
            budget = cases.budget_for(nloci, k, nind) + 12345            # (a budget need not be a multiple of anything)
            panel.set_tgls_term_budget(budget)
            got = all_calls(panel, chroms, scores, W, budget, (W, "wide", k, "blocks per slab"), subsets, (64, 300))
            assert_same_results(base, got, (W, "wide", k))
            panel.lod_windows(W, ERROR, MG, use_gl=True)
            info = panel.tgls_terms_info()
            assert (info["slab_blocks"], info["n_slabs"]) == (k, -(-8 // k))


# ------------------------------------------------------------------------------------------------ 2. the budget itself

def test_budget_too_small_is_refused_and_the_panel_stays_usable(gpu_ctx):
    W = 100
    chroms, codes, gl, scores = cases.case(W)
    nloci = sum(c[0].shape[0] for c in chroms)
    with open_panel(gpu_ctx, chroms, cases.NIND, codes) as panel:
        for bad in (1, cases.budget_for(nloci, 1, cases.NIND) - 1):
            with pytest.raises(abi.GarlicError) as e:
                panel.set_tgls_term_budget(bad)
            assert e.value.code == abi.ERR_INVALID and "budget" in str(e.value) and str(cases.budget_for(nloci, 1, cases.NIND)) in str(e.value)
        got = panel.lod_windows(W, ERROR, MG, use_gl=True)
        assert all(ol.bits_equal(np.ascontiguousarray(got[c]), scores[c]) for c in range(len(scores)))
        check_info(panel, nloci, 0, cases.blocks_of(cases.NIND), "after the refused budgets")
        panel.set_tgls_term_budget(cases.budget_for(nloci, 1, cases.NIND))
        got = panel.lod_windows(W, ERROR, MG, use_gl=True)
        assert all(ol.bits_equal(np.ascontiguousarray(got[c]), scores[c]) for c in range(len(scores)))
        check_info(panel, nloci, cases.budget_for(nloci, 1, cases.NIND), cases.blocks_of(cases.NIND), "smallest budget")


def test_continuous_panel_ignores_the_budget(gpu_ctx):
    W = 100
    chroms, _, _, _ = cases.case(W)
    gl = fcases.bounded_likelihoods(np.random.default_rng(9300), chroms, "continuous")
    scores = fcases.tgls_scores(chroms, gl, W)
    nloci = sum(c[0].shape[0] for c in chroms)
    with open_panel(gpu_ctx, chroms, cases.NIND, None, gl) as panel:
        assert panel.tgls_mode()[0] == 2
        panel.set_tgls_term_budget(cases.budget_for(nloci, 1, cases.NIND))
        got = panel.lod_windows(W, ERROR, MG, use_gl=True)
        assert all(ol.bits_equal(np.ascontiguousarray(got[c]), scores[c]) for c in range(len(scores)))
        info = panel.tgls_terms_info()
        assert info["n_slabs"] == 0 and info["whole_bytes"] == (cases.ROWS_PAD + nloci) * cases.nind_pad_of(cases.NIND) * 8


# ------------------------------------------------------------------------------------------------ 3. sequences on one panel

def test_widths_budgets_and_new_genotypes_in_sequence(gpu_ctx):
    nind = cases.NIND
    chroms, codes, gl, _ = cases.case(100)
    nloci = sum(c[0].shape[0] for c in chroms)
    small = cases.budget_for(nloci, 1, nind)
    everyone = cases.blocks_of(nind)

    def scores_match(panel, chroms, gl, W, budget, what):
        want = fcases.tgls_scores(chroms, gl, W)
        got = panel.lod_windows(W, ERROR, MG, use_gl=True)
        for c in range(len(want)):
            assert ol.bits_equal(np.ascontiguousarray(got[c]), want[c]), (what, c)
        check_info(panel, nloci, budget, everyone, what)
        feed, _ = panel.lod_feed(W, ERROR, MG, W, use_gl=True)
        flat = np.concatenate(fcases.flat(want, W))
        assert len(flat) > 0 and ol.bits_equal(feed, flat), what
        assert panel.feed_info()[0] == TGLS_CHAIN
        check_info(panel, nloci, budget, everyone, (what, "feed"))

    with open_panel(gpu_ctx, chroms, nind, codes) as panel:
        panel.set_tgls_term_budget(small)
        for W in (100, 10, 200):                                  # window sizes in turn on the same slabs
            scores_match(panel, chroms, gl, W, small, ("width", W))
        panel.set_tgls_term_budget(0)                             # small -> 0 -> small
        scores_match(panel, chroms, gl, 100, 0, "budget 0 after slabs")
        panel.set_tgls_term_budget(small)
        assert panel.tgls_terms_info()["resident_bytes"] <= small        # the whole matrix went at once
        scores_match(panel, chroms, gl, 100, small, "slabs after budget 0")
        # new genotypes between two calls: the second call's slabs are built from them
        changed = [(np.where(g >= 0, 2 - g, g).astype(g.dtype), f, p, cs, ce) for (g, f, p, cs, ce) in chroms]
        assert not np.array_equal(changed[5][0], chroms[5][0])
        panel.set_genotypes(np.concatenate([c[0] for c in changed], axis=0))
        scores_match(panel, changed, gl, 100, small, "after set_genotypes")
        panel.set_freq(np.concatenate([1.0 - c[1] for c in changed]))
        flipped = [(g, 1.0 - f, p, cs, ce) for (g, f, p, cs, ce) in changed]
        scores_match(panel, flipped, gl, 100, small, "after set_freq")
        other = [cases.VALUES[::-1][k] for k in codes]           # another likelihood for every genotype
        panel.set_gl_codes(np.concatenate(codes, axis=0), cases.VALUES[::-1].copy())
        scores_match(panel, flipped, other, 100, small, "after set_gl_codes")


def test_twenty_launches_identical(gpu_ctx):
    W, nind = 100, cases.NIND_WIDE
    chroms, codes, gl, scores = cases.case(W, nind)
    nloci = sum(c[0].shape[0] for c in chroms)
    cutoff = cases.cutoff_of(scores)
    with open_panel(gpu_ctx, chroms, nind, codes) as panel:
        panel.set_tgls_term_budget(cases.budget_for(nloci, 2, nind))
        first = None
        for k in range(21):
            out = panel.lod_windows(W, ERROR, MG, use_gl=True, pitch_align=32)
            feed, _ = panel.lod_feed(W, ERROR, MG, W, use_gl=True)
            segs = panel.roh_segments(W, ERROR, MG, cutoff, FRAC, use_gl=True)
            now = (np.concatenate([np.ascontiguousarray(x).ravel() for x in out]), feed, np.asarray(segs))
            if first is None:
                first = now
                assert all(ol.bits_equal(np.ascontiguousarray(out[c]), scores[c]) for c in range(len(scores)))
                assert len(feed) > 0 and len(segs) > 0
            assert ol.bits_equal(now[0], first[0]) and ol.bits_equal(now[1], first[1]) and np.array_equal(now[2], first[2]), k
        info = panel.tgls_terms_info()
        assert (info["slab_blocks"], info["n_slabs"]) == (2, 4)
        st = panel.stats()
        assert st["n_stall_reruns"] == 0 and st["n_count_timeouts"] == 0
