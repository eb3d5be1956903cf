"""GPU parity of the LD weights on panels wider than six 64-individual blocks (7, 10, 21 and 34 blocks): the integer counts
against plain numpy, the weights against the CPU oracle, bit for bit -- the staging paths of ld_planes_kernel,
ld_pair_lane_kernel, ld_pair_tiled_kernel and ld_pair_mfma_kernel that narrower panels never reach (tests/ld_wide_cases.py;
tests/test_ld_wide_cpu.py checks that the cases reach them).  Every comparison is exact."""
import numpy as np
import pytest

import ld_wide_cases as lw
import oracle_lib as ol
from garlic_amd import abi

pytestmark = pytest.mark.gpu

COUNT_SUBS = ["all", "third", "from_blk4", "last_blk", "one_per_blk", "empty"]
WEIGHT_SUBS = ["all", "third", "one_per_blk"]


def make_panel(ctx, chroms, nind, phase=None):
    panel = abi.Panel(ctx, [c[0].shape[0] for c in chroms], nind)
    pos = np.concatenate([c[2] for c in chroms])
    panel.set_map(pos, [c[3] for c in chroms], [c[4] for c in chroms], gpos=pos * 1e-6)
    panel.set_freq(np.concatenate([c[1] for c in chroms]))
    panel.set_genotypes(np.concatenate([c[0] for c in chroms], axis=0))
    if phase is not None:
        panel.set_phase(phase)
    return panel


def case_panel(ctx, nind, w, phased=True):
    chroms, phase, _ = lw.panel(nind, w)
    return make_panel(ctx, chroms, nind, phase if phased else None)


def ref_counts(nind, w, phased, subname):
    chroms, phase, subs = lw.panel(nind, w)
    return lw.phased_pair_counts(chroms, phase, w, subs[subname]) if phased else lw.pair_counts(chroms, w, subs[subname])


def check_counts(panel, nind, w, phased, subnames, tag=""):
    chroms, _, subs = lw.panel(nind, w)
    want_loc = lw.locus_counts(chroms)
    for name in subnames:
        loc, pair = panel.ld_counts(w, sub_idx=subs[name], phased=phased)
        want = ref_counts(nind, w, phased, name)
        assert np.array_equal(loc, want_loc), (tag, nind, w, phased, name)       # homFreq's counts: every individual
        bad = np.argwhere(pair != want)
        assert bad.shape[0] == 0, (tag, nind, w, phased, name, bad.shape[0], bad[:4].tolist())
        if name == "empty":
            assert not pair.any()


def check_weights(panel, nind, w, phased, subnames, tag=""):
    _, _, subs = lw.panel(nind, w)
    for name in subnames:
        got = panel.compute_ld(w, sub_idx=subs[name], phased=phased)
        assert ol.bits_equal(got, lw.oracle_weights(nind, w, phased, name)), (tag, nind, w, phased, name)


@pytest.mark.parametrize("nind,w,phased", lw.CASES)
def test_counts_match_numpy(gpu_ctx, nind, w, phased):
    """ld_counts against the numpy counts for every kind of subsample: everyone, a random third, members only in blocks 4
    and up, only in the last real block, one per block, nobody"""
    with case_panel(gpu_ctx, nind, w, phased) as panel:
        check_counts(panel, nind, w, phased, COUNT_SUBS)


@pytest.mark.parametrize("nind,w,phased", lw.CASES)
def test_weights_match_oracle(gpu_ctx, nind, w, phased):
    """compute_ld (the fused MFMA -> hr2 form where it applies) against oracle_hr2_ld / oracle_r2_ld"""
    with case_panel(gpu_ctx, nind, w, phased) as panel:
        check_weights(panel, nind, w, phased, WEIGHT_SUBS)


@pytest.mark.parametrize("nind,w", [(n, w) for n, w, ph in lw.CASES if not ph and lw.pair_kernel(w, False, lw.nblk_of(n)) == "mfma"])
def test_mfma_widths_unfused(gpu_ctx, monkeypatch, nind, w):
    """the MFMA pair counts written as a table and finished by ld_finish's kernels"""
    monkeypatch.setenv("GARLIC_LD_UNFUSED", "1")
    with case_panel(gpu_ctx, nind, w, False) as panel:
        check_weights(panel, nind, w, False, WEIGHT_SUBS, "unfused")


SWITCHES = [("GARLIC_LD_PAIR_TILED", "1"), ("GARLIC_LD_PAIR_L2", "1"), ("GARLIC_LD_PAIR_NO_MFMA", "1"),
            ("GARLIC_LD_PAIR_FLAT", "1"), ("GARLIC_LD_LANE_STAGE", "3"), ("GARLIC_LD_NO_PLANE_CACHE", "1")]


SWITCH_CASES = [(s, v, n, w, ph) for s, v in SWITCHES for n, w, ph in lw.CASES
                if n in lw.SWITCH_NINDS and not (s == "GARLIC_LD_PAIR_FLAT" and w > 32)]


@pytest.mark.parametrize("switch,value,nind,w,phased", SWITCH_CASES)
def test_pair_stage_under_switch(gpu_ctx, monkeypatch, switch, value, nind, w, phased):
    """the pair stage of every 577- and 1250-wide case under a kernel-selecting switch: counts against numpy, and the weights
    against the oracle for everyone"""
    monkeypatch.setenv(switch, value)
    with case_panel(gpu_ctx, nind, w, phased) as panel:
        check_counts(panel, nind, w, phased, ["all", "from_blk4", "one_per_blk"], switch)
        check_weights(panel, nind, w, phased, ["all"], switch)


@pytest.mark.parametrize("phased", [False, True])
def test_plane_cache_across_subsamples_and_genotypes(gpu_ctx, phased):
    """1250 individuals: subsample A, then B, then A again, then new genotypes -- the cache key hashes nblk = 21 words, a
    stale plane would show"""
    nind, w = 1250, 40
    chroms, phase, subs = lw.panel(nind, w)
    with make_panel(gpu_ctx, chroms, nind, phase) as panel:
        for name in ("third", "one_per_blk", "third"):
            check_weights(panel, nind, w, phased, [name], "cache")
            check_counts(panel, nind, w, phased, [name], "cache")
        rng = np.random.default_rng(4)
        chroms2 = lw.wide_chroms(rng, [c[0].shape[0] for c in chroms], nind)
        chroms2 = [(c2[0],) + tuple(c[1:]) for c, c2 in zip(chroms, chroms2)]          # same map, new genotypes
        panel.set_genotypes(np.concatenate([c[0] for c in chroms2], axis=0))
        sub = subs["one_per_blk"]
        want = lw.oracle_r2(chroms2, phase, w, sub) if phased else lw.oracle_ld(chroms2, w, sub)
        assert ol.bits_equal(panel.compute_ld(w, sub_idx=sub, phased=phased), want)
        loc, pair = panel.ld_counts(w, sub_idx=subs["third"], phased=phased)
        want = lw.phased_pair_counts(chroms2, phase, w, subs["third"]) if phased else lw.pair_counts(chroms2, w, subs["third"])
        assert np.array_equal(loc, lw.locus_counts(chroms2)) and np.array_equal(pair, want)


def shards_of(ctx, chroms, phase, sub, cuts, phased):
    """[(panel, shard-local subsample)] of the individuals [lo, hi) of every cut"""
    parts = []
    for lo, hi in cuts:
        shard = [(g[:, lo:hi].copy(), f, p, cs, ce) for g, f, p, cs, ce in chroms]          # freq: the whole panel's
        panel = make_panel(ctx, shard, hi - lo, phase[:, lo:hi].copy() if phased else None)
        parts.append((panel, (sub[(sub >= lo) & (sub < hi)] - lo).astype(np.int32)))
    return parts


@pytest.mark.parametrize("phased", [False, True])
def test_sharded_counts_sum_to_the_whole(gpu_ctx, phased):
    """1250 individuals cut at 700 (no multiple of 64) with a panel-wide subsample: the summed counts are the numpy counts of
    the whole panel, and every shard finishes them to the oracle's weights"""
    nind, w = 1250, 40
    chroms, phase, subs = lw.panel(nind, w)
    parts = shards_of(gpu_ctx, chroms, phase, subs["third"], ((0, 700), (700, nind)), phased)
    try:
        counts = [panel.ld_counts(w, sub_idx=s, phased=phased) for panel, s in parts]
        loc, pair = counts[0][0] + counts[1][0], counts[0][1] + counts[1][1]
        assert np.array_equal(loc, lw.locus_counts(chroms))
        assert np.array_equal(pair, ref_counts(nind, w, phased, "third"))
        for panel, _ in parts:
            assert ol.bits_equal(panel.ld_finish(w, loc, pair, phased=phased), lw.oracle_weights(nind, w, phased, "third"))
    finally:
        for panel, _ in parts:
            panel.close()


def test_sharded_counts_on_device(gpu_ctx):
    """the same through ld_counts_device / ld_finish_device: the count tensors stay on the GPU and are summed there"""
    import torch
    nind, w = 1250, 40
    chroms, phase, subs = lw.panel(nind, w)
    nloci = sum(c[0].shape[0] for c in chroms)
    parts = shards_of(gpu_ctx, chroms, phase, subs["third"], ((0, 700), (700, nind)), False)
    try:
        tensors = []
        for panel, s in parts:
            loc = torch.zeros((nloci, 2), dtype=torch.int32, device="cuda")
            pair = torch.zeros((nloci, w, 2), dtype=torch.int32, device="cuda")
            torch.cuda.synchronize()
            panel.ld_counts_device(w, loc.data_ptr(), pair.data_ptr(), sub_idx=s)
            tensors.append((loc, pair))
        loc, pair = tensors[0][0] + tensors[1][0], tensors[0][1] + tensors[1][1]
        torch.cuda.synchronize()
        assert np.array_equal(pair.cpu().numpy(), ref_counts(nind, w, False, "third"))
        for panel, _ in parts:
            ld = torch.empty((nloci, w), dtype=torch.float64, device="cuda")
            torch.cuda.synchronize()
            panel.ld_finish_device(w, loc.data_ptr(), pair.data_ptr(), ld.data_ptr())
            assert ol.bits_equal(ld.cpu().numpy(), lw.oracle_weights(nind, w, False, "third"))
    finally:
        for panel, _ in parts:
            panel.close()


def multi_rows(chroms, w):
    """rows of the chromosomes of at most w + 1 SNPs -- those the oracle is asked for at size w (it takes every pair of a window
    anew: the 300-SNP chromosome at W = 40 alone would cost it 5e8 genotype pairs)"""
    rows, l0 = [], 0
    for c in chroms:
        n = c[0].shape[0]
        if n <= w + 1:
            rows.append((l0, n, c[0]))
        l0 += n
    return rows


_multi_oracle = {}


def check_multi(got, single, chroms, sizes, sub):
    for w, ld in zip(sizes, got):
        assert ol.bits_equal(ld, single[w]), w                  # every row: what compute_ld gives for the size
        for l0, n, g in multi_rows(chroms, w):
            key = (w, l0, sub is None)
            if key not in _multi_oracle:
                _multi_oracle[key] = ol.oracle_hr2_ld(g, w, idx=sub)
            assert ol.bits_equal(ld[l0:l0 + n], _multi_oracle[key]), (w, n)


@pytest.mark.parametrize("subname", ["all", "third"])
def test_several_sizes_in_one_call(gpu_ctx, subname):
    """1250 individuals, compute_ld_multi([40, 100, 200, 300]): per size compute_ld's weights on every row and the oracle's on
    the chromosomes of at most W + 1 SNPs; for everyone and with a subsample"""
    nind, sizes = 1250, lw.MULTI_SIZES
    chroms, subs = lw.multi_panel()
    assert all(any(n >= w for _, n, _ in multi_rows(chroms, w)) for w in sizes)
    sub = subs[subname]
    with make_panel(gpu_ctx, chroms, nind) as panel:
        single = {w: panel.compute_ld(w, sub_idx=sub) for w in sizes}
        check_multi(panel.compute_ld_multi(sizes, sub_idx=sub), single, chroms, sizes, sub)


def test_several_sizes_from_summed_shard_counts(gpu_ctx):
    """ld_finish_multi on both shards of the 1250-wide panel (cut at 700) from the summed counts of the largest size"""
    nind, sizes = 1250, lw.MULTI_SIZES
    chroms, _ = lw.multi_panel()
    with make_panel(gpu_ctx, chroms, nind) as panel:
        single = {w: panel.compute_ld(w) for w in sizes}
    parts = shards_of(gpu_ctx, chroms, None, np.arange(nind), ((0, 700), (700, nind)), False)
    try:
        counts = [panel.ld_counts(max(sizes), sub_idx=s) for panel, s in parts]
        loc, pair = counts[0][0] + counts[1][0], counts[0][1] + counts[1][1]
        assert np.array_equal(pair, lw.pair_counts(chroms, max(sizes)))
        for panel, _ in parts:
            check_multi(panel.ld_finish_multi(sizes, loc, pair), single, chroms, sizes, None)
    finally:
        for panel, _ in parts:
            panel.close()


def test_wide_weights_feed_wlod(gpu_ctx):
    """577 individuals: wLOD from the device-computed weights == the oracle's wLOD from the oracle's weights, for individuals of
    the first, a middle and the last block (which holds one)"""
    nind, w, mg = 577, 40, 200000
    chroms, _, _ = lw.panel(nind, w)
    with make_panel(gpu_ctx, chroms, nind) as panel:
        ld = panel.compute_ld(w)
        out = panel.wlod_windows(w, 0.001, mg, 7, 1e-9, pitch_align=32)
    want_ld = lw.oracle_weights(nind, w, False, "all")
    assert ol.bits_equal(ld, want_ld)
    inds = [0, 63, 64, 300, 511, 575, 576]
    off = 0
    for c, (g, f, p, cs, ce) in enumerate(chroms):
        n = g.shape[0]
        want = ol.oracle_calc_wlod(g, f, p, p * 1e-6, want_ld[off:off + n], cs, ce, w, 0.001, mg, 1e-9, 7)
        off += n
        assert ol.bits_equal(np.ascontiguousarray(out[c][inds]), want[inds]), c
