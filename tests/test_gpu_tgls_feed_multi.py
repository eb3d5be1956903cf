"""GPU: the TGLS KDE feeds of several window sizes in one call (garlic_lod_feed_multi_tgls: tgls_feed_multi_kernel for the
groups, tgls_feed_kernel for the sizes on their own), through the C ABI, bit for bit against the oracle's full TGLS scores
thinned by the oracle's convertWinData2DoubleData / convertSubsetWinData2DoubleData per size; counts and per-chromosome
counts equal.  No tolerance.  garlic_lod_feed_multi_info tells what every size took: forms, groups, chain launches and
term slabs built are asserted against the rule of include/garlic_hip.h (tests/tgls_feed_multi_cases.groups_of)."""
import numpy as np
import pytest

import oracle_lib as ol
import tgls_feed_cases as cases
import tgls_feed_multi_cases as mcases
import tgls_slab_cases as scases
import wlod_feed_cases as wcases
from garlic_amd import abi
from test_gpu_tgls_feed import check_feed, check_full_scores, open_panel

pytestmark = pytest.mark.gpu
MG, ERROR = cases.MG, cases.ERROR
SHARED, CHAIN, FROM_SCORES = getattr(abi, "FEED_TGLS_CHAIN_SHARED", 4), abi.FEED_TGLS_CHAIN, abi.FEED_FROM_SCORES


def check_multi(panel, scores, ws, steps, what, *, idx=None, ring=None, solo=False, n_slabs=0):
    """one multi call against the oracle, size by size; forms, groups and launch counts against the rule; returns the feeds"""
    want = mcases.expected(scores, ws, steps, idx)
    feeds, per_chr = panel.lod_feed_multi_tgls(ws, MG, steps=steps, ind_idx=idx)
    info = panel.feed_multi_info(len(ws))
    print(what, info, [len(f) for f in feeds])
    ring = [mcases.take_ring(W, s) for W, s in zip(ws, steps)] if ring is None else ring
    groups = mcases.groups_of(ws, ring, solo)
    for k, (W, step) in enumerate(zip(ws, steps)):
        assert sum(len(x) for x in want[k]) > 0, ("empty case", what, W, step)
        assert [len(x) for x in want[k]] == list(per_chr[k]), (what, W, step, list(per_chr[k]))
        flat = np.concatenate(want[k])
        assert feeds[k].shape == flat.shape, (what, W, step)
        assert ol.bits_equal(feeds[k], flat), (what, W, step, ol.count_mismatch(feeds[k], flat))
    assert info["groups"] == groups, (what, info)
    shared = mcases.shared_of(groups)
    assert info["forms"] == [FROM_SCORES if not r else SHARED if s else CHAIN for r, s in zip(ring, shared)], (what, info)
    n_ring_groups = len({g for g, r in zip(groups, ring) if r})
    assert info["n_chain_launches"] == n_ring_groups * max(n_slabs, 1) + ring.count(False), (what, info)
    return feeds


# ------------------------------------------------------------------------------------------------ 1. shapes

@pytest.mark.parametrize("name", sorted(mcases.size_lists()))
def test_shapes(gpu_ctx, name):
    """size lists on both sides of the tile, up to the ring's widest window, a size twice with two steps, more sizes than
    one group holds; chromosomes of 1, Wmin-1, Wmin, between Wmin and Wmax, Wmax, Wmax+1, Wmax+33 SNPs, gaps and a
    centromere; 1 .. 200 individuals; steps 4, W, W+7 and one beyond every chromosome"""
    ws, nind, chroms, gl, scores = mcases.shape_case(name)
    sizes = [c[0].shape[0] for c in chroms]
    with open_panel(gpu_ctx, chroms, nind, gl) as panel:
        for kind in mcases.step_kinds(name):
            check_multi(panel, scores, ws, mcases.steps_of(name, kind, ws, sizes), ("shape", name, kind, nind))
            info = panel.feed_multi_info(len(ws))
            assert all(f == SHARED for f in info["forms"]), info
            assert info["n_chain_launches"] == len(set(info["groups"])) == -(-len(ws) // mcases.max_sizes())
        check_full_scores(panel, scores[ws[0]], ws[0], ("shape", name))      # ... so no case above fell back for another reason


# ------------------------------------------------------------------------------------------------ 2. ring boundary

@pytest.mark.parametrize("k", range(len(mcases.boundary_lists())))
def test_ring_boundary(gpu_ctx, k):
    """sizes above the one-stream ring's widest window run on their own, in the same call; the others are shared"""
    ws, nind, chroms, gl, scores = mcases.boundary_case(k)
    s = cases.single_max_w()
    with open_panel(gpu_ctx, chroms, nind, gl) as panel:
        check_multi(panel, scores, ws, ws, ("boundary", ws))
        forms = panel.feed_multi_info(len(ws))["forms"]
        n_narrow = sum(W <= s for W in ws)
        assert forms == [(SHARED if n_narrow >= 2 else CHAIN) if W <= s else CHAIN for W in ws]
        assert any(W > s for W in ws)


# ------------------------------------------------------------------------------------------------ 3. likelihoods

@pytest.mark.parametrize("kind", ["codes", "continuous"])
def test_likelihoods(gpu_ctx, kind):
    ws, nind, chroms, gl, scores = mcases.likelihood_case(kind)
    with open_panel(gpu_ctx, chroms, nind, gl) as panel:
        assert panel.tgls_mode()[0] == (1 if kind == "codes" else 2)
        check_multi(panel, scores, ws, ws, ("gl", kind))


def test_panel_fed_by_codes(gpu_ctx):
    ws, nind, chroms, codes, values, gl, scores = mcases.codes_case()
    with open_panel(gpu_ctx, chroms, nind) as panel:
        panel.set_gl_codes(np.concatenate(codes, axis=0), values)
        assert panel.tgls_mode()[0] == 1
        check_multi(panel, scores, ws, ws, "set_gl_codes")


# ------------------------------------------------------------------------------------------------ 4. subsets

def test_subsets(gpu_ctx):
    """unordered lists that leave whole 64-individual blocks out, a list of one, then everyone"""
    ws, nind, chroms, gl, scores = mcases.subset_case()
    with open_panel(gpu_ctx, chroms, nind, gl) as panel:
        for idx in (np.array(x) for x in mcases.SUBSETS):
            check_multi(panel, scores, ws, ws, ("subset", list(idx)), idx=idx)
        check_multi(panel, scores, ws, ws, "everyone after subsets")


# ------------------------------------------------------------------------------------------------ 5. slabs

@pytest.mark.parametrize("nind,asked,slab_blocks", mcases.slab_budgets())
def test_slabs_are_built_once_per_call(gpu_ctx, nind, asked, slab_blocks):
    """under a term budget: the bytes of budget 0, every slab built once for the four sizes, the buffers within the budget.
    (On the 200-individual panel the budget of two-block slabs gives one slab of all four blocks: mcases.slab_budgets.)"""
    ws, chroms, codes, scores = mcases.slab_case(nind)
    nloci = sum(c[0].shape[0] for c in chroms)
    budget = scases.budget_for(nloci, asked, nind)
    assert scases.slab_blocks_for(budget, nloci, nind) == slab_blocks
    nblk = (nind + 63) // 64
    with open_panel(gpu_ctx, chroms, nind) as panel:
        panel.set_gl_codes(np.concatenate(codes, axis=0), scases.VALUES)
        whole = check_multi(panel, scores, ws, ws, "whole matrix")
        assert panel.feed_multi_info(len(ws))["n_term_builds"] == 0 and panel.tgls_terms_info()["n_slabs"] == 0
        panel.set_tgls_term_budget(budget)
        n_slabs = -(-nblk // slab_blocks)
        under = check_multi(panel, scores, ws, ws, ("budget", budget), n_slabs=n_slabs)
        for a, b in zip(whole, under):
            assert ol.bits_equal(a, b)
        info, terms = panel.feed_multi_info(len(ws)), panel.tgls_terms_info()
        print(info, terms)
        assert terms["slab_blocks"] == slab_blocks and terms["n_slabs"] == n_slabs
        assert info["n_term_builds"] == terms["n_slabs"]
        assert info["n_term_builds"] < len(ws) * terms["n_slabs"]
        assert terms["resident_bytes"] <= budget
        # a subset: only the slabs that hold a listed block
        idx = np.array(scases.SUBSETS[2])
        check_multi(panel, scores, ws, ws, ("budget, subset", budget), idx=idx,
                    n_slabs=scases.n_slabs_of(scases.blocks_of(nind, idx=idx), slab_blocks))
        assert panel.feed_multi_info(len(ws))["n_term_builds"] == panel.tgls_terms_info()["n_slabs"]
        panel.set_tgls_term_budget(0)
        check_multi(panel, scores, ws, ws, "whole matrix again")


# ------------------------------------------------------------------------------------------------ 6. fallbacks per size

def test_fallbacks_per_size(gpu_ctx):
    """a step-3 size and a size whose windows can sum to exactly -9999.0 among ordinary ones: every size the oracle's
    bytes and its own form, the ordinary sizes still shared"""
    ws, steps, ring, nind, chroms, gl, scores = mcases.fallback_case()
    with open_panel(gpu_ctx, chroms, nind, gl) as panel:
        check_multi(panel, scores, ws, steps, "mixed", ring=ring)
        forms = panel.feed_multi_info(len(ws))["forms"]
        assert forms == [FROM_SCORES, FROM_SCORES, SHARED, SHARED]


# ------------------------------------------------------------------------------------------------ 7. non-finite terms

def test_nonfinite_terms(gpu_ctx):
    """a NaN frequency and likelihoods of 0 and infinity: the NaN runs to the end of each size's own run, the feed drops it"""
    ws, nind, chroms, gl, scores = mcases.nonfinite_case()
    for W in ws:
        assert np.isnan(np.concatenate([s.ravel() for s in scores[W]])).any()
    with open_panel(gpu_ctx, chroms, nind, gl) as panel:
        for steps in (ws, [4] * len(ws)):
            for feed in check_multi(panel, scores, ws, steps, ("non-finite terms", steps)):
                assert not np.isnan(feed).any()


# ------------------------------------------------------------------------------------------------ 8. switch, repeats

def test_same_bytes_in_groups_of_one(gpu_ctx, monkeypatch):
    ws, nind, chroms, gl, scores = mcases.subset_case()
    with open_panel(gpu_ctx, chroms, nind, gl) as panel:
        a = check_multi(panel, scores, ws, ws, "shared")
        monkeypatch.setenv("GARLIC_TGLS_FEED_MULTI_SOLO", "1")
        b = check_multi(panel, scores, ws, ws, "GARLIC_TGLS_FEED_MULTI_SOLO", solo=True)
        assert panel.feed_multi_info(len(ws))["forms"] == [CHAIN] * len(ws)
        monkeypatch.delenv("GARLIC_TGLS_FEED_MULTI_SOLO")
        for x, y in zip(a, b):
            assert ol.bits_equal(x, y)


def test_twenty_launches_identical(gpu_ctx):
    ws, nind, chroms, gl, scores = mcases.subset_case()
    with open_panel(gpu_ctx, chroms, nind, gl) as panel:
        first = check_multi(panel, scores, ws, ws, "first")
        for k in range(20):
            feeds, _ = panel.lod_feed_multi_tgls(ws, MG)
            for x, y in zip(first, feeds):
                assert ol.bits_equal(x, y), k
            assert panel.feed_multi_info(len(ws))["forms"] == [SHARED] * len(ws)


# ------------------------------------------------------------------------------------------------ 9. neighbours

def test_neighbours_on_one_panel(gpu_ctx):
    """after a multi call: a single TGLS feed, full TGLS scores, a weighted feed with likelihoods (rescales the term matrix),
    the --error multi feed; then the multi call again -- every one against the oracle"""
    M, MU = wcases.M, wcases.MU
    ws, nind, chroms, gpos, lds, gl, scores = mcases.neighbour_case()
    W = ws[0]
    with open_panel(gpu_ctx, chroms, nind, gl, gpos) as panel:
        panel.set_ld(W, np.concatenate(lds, axis=0))
        check_multi(panel, scores, ws, ws, "multi")
        check_feed(panel, scores[W], W, W, "single feed after the multi call")
        check_full_scores(panel, scores[W], W, "full scores after the multi call")
        wwant = np.concatenate(cases.flat(wcases.wlod_scores(chroms, gpos, lds, W, gl=gl), W))
        wfeed, _ = panel.lod_feed(W, ERROR, MG, W, use_gl=True, weighted=True, M=M, mu=MU)
        assert len(wwant) > 0 and ol.bits_equal(wfeed, wwant)
        assert panel.feed_info()[0] == abi.FEED_SAMPLED_WLOD
        check_multi(panel, scores, ws, ws, "multi after the weighted feed")
        pfeeds, _ = panel.lod_feed_multi(ws[:2], ERROR, MG)
        for Wp, pf in zip(ws[:2], pfeeds):
            pwant = np.concatenate([ol.oracle_flatten(ol.oracle_calc_lod(g, f, p, cs, ce, Wp, ERROR, MG), Wp) for (g, f, p, cs, ce) in chroms])
            assert len(pwant) > 0 and ol.bits_equal(pf, pwant)
        check_multi(panel, scores, ws, [w + 7 for w in ws], "multi after the --error feeds")
        assert panel.feed_info()[0] == SHARED


# ------------------------------------------------------------------------------------------------ 10. host tool

def test_host_tool_winsize_multi_with_likelihoods(tmp_path):
    """garlic-lod --tgls .. --winsize-multi with three sizes (one multi call) writes the KDE input feeds of three
    single-size runs, byte for byte"""
    import filecmp
    import os
    from test_gpu_host_tool import E2E, run_tool_tgls
    tgls = ["--tgls", os.path.join(E2E, "tiny.tgls.gz"), "--gl-type", "GQ"]
    sizes = ["20", "45", "33"]
    d = tmp_path / "multi"
    d.mkdir()
    multi = run_tool_tgls(d, *tgls, "--winsize-multi", *sizes)
    for W in sizes:
        d = tmp_path / ("single" + W)
        d.mkdir()
        single = run_tool_tgls(d, *tgls, "--winsize", W)
        assert os.path.getsize(f"{single}.{W}SNPs.lod.f64") > 0
        assert filecmp.cmp(f"{multi}.{W}SNPs.lod.f64", f"{single}.{W}SNPs.lod.f64", shallow=False), W
