"""No GPU: the rule that sends phased LD calls to the matrix cores at its boundaries, the haplotype identity the phased
ld_pair_mfma_kernel rests on against the definition of x11, and the bit-row phase layout against the byte layout."""
import numpy as np
import pytest

import ld_phased_cases as lp
import ld_wide_cases as lw


@pytest.mark.parametrize("nblk", [1, 2, 4, 21, 34])
def test_rule_at_the_window_boundaries(nblk):
    """W = 16 | 17: lane | mfma (LD_SMALL_MAX_W); W = 129 | 130: mfma | lane (NJ = 5 | 6)"""
    assert lp.pair_kernel_phased(16, nblk) == "lane"
    assert lp.pair_kernel_phased(17, nblk) == "mfma"
    assert lp.pair_kernel_phased(129, nblk) == "mfma"
    assert lp.pair_kernel_phased(130, nblk) == "lane"
    assert lp.mfma_nj(129) == 5 and lp.mfma_nj(130) == 6 and lp.mfma_nj(17) == 2
    assert [lp.mfma_nj(w) for w in lp.WINSIZES] == [2, 3, 5, 5]


@pytest.mark.parametrize("w", [17, 40, 100, 129])
def test_every_switch_that_leaves_the_form(w):
    nblk = 4
    assert lp.pair_kernel_phased(w, nblk, {"GARLIC_LD_PAIR_NO_MFMA": "1"}) == "lane"
    assert lp.pair_kernel_phased(w, nblk, {"GARLIC_LD_PAIR_TILED": "1"}) == "tiled"
    assert lp.pair_kernel_phased(w, nblk, {"GARLIC_LD_PAIR_L2": "1"}) == "plain_phased"
    assert lp.pair_kernel_phased(w, nblk, {"GARLIC_LD_PAIR_FLAT": "1"}) == ("flat" if w <= 32 else "mfma")
    # switches that do not pick the pair kernel leave it alone
    assert lp.pair_kernel_phased(w, nblk, {"GARLIC_LD_LANE_STAGE": "3"}) == "mfma"
    assert lp.pair_kernel_phased(w, nblk, {"GARLIC_LD_NO_PLANE_CACHE": "1"}) == "mfma"
    # off the form, the rule is the one ld_wide_cases states for phased calls
    for sw in ({"GARLIC_LD_PAIR_NO_MFMA": "1"}, {"GARLIC_LD_PAIR_TILED": "1"}, {"GARLIC_LD_PAIR_L2": "1"}):
        assert lp.pair_kernel_phased(w, nblk, sw) == lw.pair_kernel(w, True, nblk, sw)


def test_count_bound():
    """the f32 tiles hold count / 4 exactly below 2^22: 2 * nind_pad = 128 nblk must stay below it"""
    assert lp.pair_kernel_phased(40, (1 << 15) - 1) == "mfma"
    assert lp.pair_kernel_phased(40, 1 << 15) != "mfma"
    assert np.float32((lp.LDM_COUNT_MAX - 1) / 4) * np.float32(4) == lp.LDM_COUNT_MAX - 1


def test_cases_reach_every_nj_and_pipeline_depth():
    assert {lp.pair_kernel_phased(w, lw.nblk_of(n)) for n, w in lp.CASES} == {"mfma"}
    assert sorted({lw.nblk_of(n) for n in lp.NINDS}) == [1, 2, 4, 5]        # no prefetch; prefetch only; steady state
    for nind in lp.NINDS:
        subs = lp.subsamples(np.random.default_rng(0), nind)
        assert subs["third"].shape[0] == nind // 3
        blks = set((subs["one_blk"] // 64).tolist())
        assert len(blks) == 1


@pytest.fixture(scope="module")
def small():
    """one chromosome, 130 individuals (three blocks with somebody), missing genotypes throughout, a dead middle block"""
    rng = np.random.default_rng(31)
    nind, n = 130, 24
    (g, f, p, cs, ce), = lw.wide_chroms(rng, [n], nind)
    phase = rng.integers(0, 2, size=(n, nind)).astype(np.uint8)
    assert (g == -9).any() and (g == 1).any() and (g == 2).any()
    return g, phase, rng


@pytest.mark.parametrize("subname", ["all", "third", "last_blk", "empty"])
def test_haplotype_identity_matches_the_definition(small, subname):
    """|A_i & A_j| + |B_i & B_j| == x11 and 2 |M_i & M_j| == total, against the triple loop of brute_counts(.., phase=..)"""
    g, phase, _ = small
    nind, w = g.shape[1], 9
    sub = {"all": None, "third": np.arange(0, nind, 3), "last_blk": np.arange(128, nind), "empty": np.zeros(0, dtype=np.int64)}[subname]
    _, want = lw.brute_counts(g, w, sub, phase=phase)
    got = lp.haplotype_pair_counts(g, phase, w, sub)
    assert np.array_equal(got, want)
    assert np.array_equal(got, lw.phased_pair_counts([(g,)], phase, w, sub))
    if subname == "empty":
        assert not got.any()
    else:
        assert got[..., 1].any()


def test_haplotype_identity_per_genotype_pair():
    """the table of garlic-data.cpp:598-604, one individual: (2,2) -> 2; (1,2), (2,1) -> 1; (1,1) -> 1 iff firstCopy agrees"""
    for a in (0, 1, 2, -9):
        for b in (0, 1, 2, -9):
            for fa in (0, 1):
                for fb in (0, 1):
                    g = np.array([[a], [b]], dtype=np.int16)
                    ph = np.array([[fa], [fb]], dtype=np.uint8)
                    tot, x11 = lp.haplotype_pair_counts(g, ph, 2)[0, 1]
                    want = 2 if (a, b) == (2, 2) else 1 if a + b == 3 and -9 not in (a, b) else int((a, b) == (1, 1) and fa == fb)
                    assert x11 == want, (a, b, fa, fb)
                    assert tot == (0 if -9 in (a, b) else 2)
                    assert x11 <= tot                                    # a set bit of A or B is a non-missing genotype


@pytest.mark.parametrize("nind", [1, 7, 8, 9, 63, 64, 65, 130])
def test_bit_rows_against_bytes(nind):
    """np.packbits(.., bitorder='little') is the cache's layout; the plane words made from the rows (8 bytes a word, pad bits
    cleared, a row never read past (nind + 7) / 8 bytes) are those made from the bytes -- also with wider rows full of ones"""
    rng = np.random.default_rng(nind)
    phase = rng.integers(0, 2, size=(11, nind)).astype(np.uint8)
    nblk = lw.nblk_of(nind)
    want = lp.plane_words_from_bytes(phase, nblk)
    rows = lp.pack_phase_rows(phase)
    assert rows.shape == (11, (nind + 7) // 8)
    for l in range(11):
        for i in range(nind):
            assert (rows[l, i >> 3] >> (i & 7)) & 1 == phase[l, i]
    assert np.array_equal(lp.plane_words_from_rows(rows, nind, nblk), want)
    wide = lp.pack_phase_rows(phase, row_bytes=rows.shape[1] + 5, fill=0xFF)
    assert np.array_equal(lp.plane_words_from_rows(wide, nind, nblk), want)
    dirty = rows.copy()
    if nind & 7:
        dirty[:, -1] |= np.uint8((0xFF << (nind & 7)) & 0xFF)              # ones behind the last individual
    assert np.array_equal(lp.plane_words_from_rows(dirty, nind, nblk), want)
