"""No GPU: the wide-panel LD cases reach the staging paths they are there for, and the plain numpy counts they are compared
with are the oracle's -- by a brute-force triple loop, and through hr2 / r2 and the ordered sums bit for bit."""
import numpy as np

import ld_wide_cases as lw
import oracle_lib as ol


def reached(switches=None, ninds=None):
    """{(kernel, path)} over the case table"""
    out = set()
    for nind, w, phased in lw.CASES:
        if ninds is not None and nind not in ninds:
            continue
        if "GARLIC_LD_PAIR_FLAT" in (switches or {}) and w > 32:
            continue
        nblk = lw.nblk_of(nind)
        k = lw.pair_kernel(w, phased, nblk, switches)
        out |= {(k, p) for p in lw.staging(w, phased, nblk, switches)} | {(k, "any")}
    return out


def test_nblk_of_the_widths():
    assert [lw.nblk_of(n) for n in (385, 577, 1250, 2113)] == [7, 10, 21, 34]
    assert [lw.real_blocks(n) for n in (385, 577, 1250, 2113)] == [7, 10, 20, 34]       # 1250: an all-padding last block
    assert lw.nblk_of(1) == 1 and lw.nblk_of(2) == 2 and lw.nblk_of(66) == 3           # 2 .. 64: a pad block
    assert all(n % 64 == 1 for n in (385, 577, 2113))          # the last real block holds one individual


def test_choice_rule_at_its_boundaries():
    for nblk in (7, 10, 21, 34):
        assert [lw.pair_kernel(w, False, nblk) for w in (10, 16, 17, 40, 100, 129, 130, 257, 258)] == \
            ["lane", "lane", "mfma", "mfma", "mfma", "mfma", "lane", "lane", "plain"]
        assert [lw.pair_kernel(w, True, nblk) for w in (9, 40, 257, 258)] == ["lane", "lane", "lane", "plain_phased"]
        assert lw.pair_kernel(100, False, nblk, {"GARLIC_LD_PAIR_NO_MFMA": "1"}) == "lane"
        assert lw.pair_kernel(100, False, nblk, {"GARLIC_LD_PAIR_TILED": "1"}) == "tiled"
        assert lw.pair_kernel(258, False, nblk, {"GARLIC_LD_PAIR_TILED": "1"}) == "plain"
        assert lw.pair_kernel(100, True, nblk, {"GARLIC_LD_PAIR_L2": "1"}) == "plain_phased"
        assert lw.pair_kernel(32, False, nblk, {"GARLIC_LD_PAIR_FLAT": "1"}) == "flat"
        assert lw.pair_kernel(33, False, nblk, {"GARLIC_LD_PAIR_FLAT": "1"}) == "mfma"
    assert lw.lane_stage_of(10) == 4 and lw.lane_stage_of(3) == 3 and lw.lane_stage_of(10, {"GARLIC_LD_LANE_STAGE": "3"}) == 3


def test_cases_reach_every_staging_path():
    """shrink the list and this fails: every kernel of the table appears with an nblk beyond its staging depth"""
    cases = [(nind, w, ph, lw.nblk_of(nind), lw.pair_kernel(w, ph, lw.nblk_of(nind))) for nind, w, ph in lw.CASES]
    for phased in (False, True):
        assert any(k == "lane" and nblk > 8 and nblk % 4 != 0 for _, _, ph, nblk, k in cases if ph == phased), phased
        assert any(nblk > 32 for _, _, ph, nblk, _ in cases if ph == phased), phased        # planes: second outer trip
        assert any(nblk > 8 for _, _, ph, nblk, _ in cases if ph == phased), phased         # planes: u >= 2
    assert any(k == "mfma" and nblk >= 21 for *_, nblk, k in cases)
    assert any(k == "mfma" and nblk > 32 for *_, nblk, k in cases)
    assert any(k == "plain" and nblk >= 21 for *_, nblk, k in cases)
    assert any(k == "plain_phased" and nblk > 8 for *_, nblk, k in cases)
    default = reached()
    for pair in [("lane", "lane_partial"), ("lane", "lane_stages3"), ("lane", "lane_restaged"), ("lane", "planes_u2"),
                 ("lane", "planes_trip2"), ("mfma", "mfma_steady"), ("mfma", "planes_trip2"),
                 ("plain", "any"), ("plain_phased", "any")]:
        assert pair in default, pair
    # 385: a partial second stage and no third; 577: three stages, the last partial
    assert lw.nblk_of(385) == 4 + 3 and lw.nblk_of(577) == 4 + 4 + 2
    assert any(nind == 385 and k == "lane" for nind, _, _, _, k in cases)
    # under the switches, on the widths the switch tests run at
    tiled = [(nind, w, ph) for nind, w, ph in lw.CASES if nind in lw.SWITCH_NINDS
             and lw.pair_kernel(w, ph, lw.nblk_of(nind), {"GARLIC_LD_PAIR_TILED": "1"}) == "tiled"]
    assert any(lw.nblk_of(nind) > 8 and not ph for nind, _, ph in tiled) and any(lw.nblk_of(nind) > 8 and ph for nind, _, ph in tiled)
    assert ("tiled", "tiled_chunk2") in reached({"GARLIC_LD_PAIR_TILED": "1"}, lw.SWITCH_NINDS)
    assert {k for k, _ in reached({"GARLIC_LD_PAIR_L2": "1"}, lw.SWITCH_NINDS)} == {"plain", "plain_phased"}
    assert "mfma" not in {k for k, _ in reached({"GARLIC_LD_PAIR_NO_MFMA": "1"}, lw.SWITCH_NINDS)}
    assert {k for k, _ in reached({"GARLIC_LD_PAIR_FLAT": "1"}, lw.SWITCH_NINDS)} == {"flat"}
    stage3 = reached({"GARLIC_LD_LANE_STAGE": "3"}, lw.SWITCH_NINDS)
    assert ("lane", "lane_stages3") in stage3 and ("lane", "lane_partial") in stage3        # 10 = 3 + 3 + 3 + 1
    assert set(lw.NINDS) == {385, 577, 1250, 2113}
    # both sides of every boundary
    assert {16, 17, 129, 130, 257, 258} <= set(lw.UNPHASED[577]) and {257, 258} <= set(lw.PHASED[577])


def test_blocks_of_a_wide_panel_differ():
    """missingness and homozygosity differ from block to block, one block is all-missing at a few SNPs: the per-block counts of
    a SNP pair are all different from one another often enough that a swapped or repeated block shows"""
    chroms, _, subs = lw.panel(577, 10)
    g = chroms[0][0]
    nreal = lw.real_blocks(577)
    present = np.stack([(g[:, b * 64:(b + 1) * 64] != -9).sum(axis=0).mean() for b in range(nreal - 1)])
    assert np.all(np.diff(present) < 0)                                                     # missingness rises with the block
    het = np.stack([(g[:, b * 64:(b + 1) * 64] == 1).mean() for b in range(nreal - 1)])
    assert het[0] > het[-1] + 0.1
    dead = nreal // 2
    assert (g[[2, 3, 7], dead * 64:(dead + 1) * 64] == -9).all() and (g[4, dead * 64:(dead + 1) * 64] != -9).any()
    assert subs["all"] is None and subs["empty"].shape[0] == 0
    assert subs["from_blk4"].min() >= 256 and (subs["last_blk"] // 64 == nreal - 1).all()
    assert sorted(subs["one_per_blk"] // 64) == list(range(nreal))
    assert subs["third"].shape[0] == 577 // 3 and np.unique(subs["third"]).shape[0] == 577 // 3


def small_panel():
    rng = np.random.default_rng(77)
    chroms = lw.wide_chroms(rng, [37, 1, 11, 12, 13], 130)
    nloci = sum(c[0].shape[0] for c in chroms)
    phase = rng.integers(0, 2, size=(nloci, 130)).astype(np.uint8)
    sub = np.sort(rng.choice(130, size=43, replace=False)).astype(np.int32)
    return chroms, phase, sub


def test_numpy_counts_against_the_triple_loop():
    chroms, phase, sub = small_panel()
    w = 12
    for s in (None, sub, np.zeros(0, dtype=np.int32)):
        loc = lw.locus_counts(chroms)
        pair = lw.pair_counts(chroms, w, s)
        ppair = lw.phased_pair_counts(chroms, phase, w, s)
        l0 = 0
        for c in chroms:
            n = c[0].shape[0]
            bl, bp = lw.brute_counts(c[0], w, s)
            _, bpp = lw.brute_counts(c[0], w, s, phase[l0:l0 + n])
            assert np.array_equal(loc[l0:l0 + n], bl)
            assert np.array_equal(pair[l0:l0 + n], bp)
            assert np.array_equal(ppair[l0:l0 + n], bpp)
            l0 += n
        assert pair[:, 0].max() == 0 and (s is None or len(s) or not pair.any())
    assert lw.pair_counts(chroms, w)[:, 1:, 0].max() > 100          # (the check is not of an empty table)


def test_numpy_counts_give_the_oracles_weights_bit_for_bit():
    """count convention -- d, the chromosome edges, subsample for the pairs against everyone for homFreq -- tied to the oracle"""
    chroms, phase, sub = small_panel()
    w = 12
    loc = lw.locus_counts(chroms)
    hf = lw.hom_freq(loc)
    for s in (None, sub, np.zeros(0, dtype=np.int32)):        # (nobody: every pair is 0/0, x86's NaN with the sign set)
        pair = lw.pair_counts(chroms, w, s)
        ppair = lw.phased_pair_counts(chroms, phase, w, s)
        l0 = 0
        for c in chroms:
            n = c[0].shape[0]
            got = lw.ld_from_counts(n, w, hf[l0:l0 + n], pair[l0:l0 + n])
            assert ol.bits_equal(got, ol.oracle_hr2_ld(c[0], w, idx=s)), (n, s is None)
            got = lw.ld_from_counts(n, w, c[1], ppair[l0:l0 + n])
            assert ol.bits_equal(got, ol.oracle_r2_ld(c[0], phase[l0:l0 + n], c[1], w, idx=s)), (n, s is None)
            l0 += n
    want = ol.oracle_hr2_ld(chroms[0][0], w)
    assert (want[:37 - w + 1] >= 1).all() and not want[37 - w + 1:].any()
    nobody = ol.oracle_hr2_ld(chroms[0][0], w, idx=np.zeros(0, dtype=np.int32))
    assert np.isnan(nobody).any() and np.signbit(nobody[np.isnan(nobody)]).all()


def test_oracle_cost_of_the_cases_stays_small():
    """the oracle visits starts x W^2 x individuals genotype pairs: every case stays within ORACLE_VISITS, or has the three
    window starts of its W and W+1 chromosomes and no more; every case keeps 1, W-1, W, W+1"""
    for nind, w, _ in lw.CASES:
        sizes = lw.chrom_sizes(nind, w)
        assert {1, w - 1, w, w + 1} <= set(sizes)
        starts = lw.starts_of(sizes, w)
        assert starts == 3 or starts * w * w * nind <= lw.ORACLE_VISITS, (nind, w)
    # the tile edges where they are affordable: MFMA 128-SNP tiles and lane 256-SNP tiles at more than 8 blocks
    assert {127, 128, 129} <= set(lw.chrom_sizes(385, 17)) and {127, 128, 129} <= set(lw.chrom_sizes(577, 17))
    assert {255, 256, 257} <= set(lw.chrom_sizes(577, 10)) and {255, 256, 257} <= set(lw.chrom_sizes(577, 9))
    assert {255, 256, 257} <= set(lw.chrom_sizes(2113, 9))
    for w in lw.MULTI_SIZES:
        assert any(w <= n <= w + 1 for n in lw.MULTI_CHROMS)
