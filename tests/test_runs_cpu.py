"""CPU: what the dense-run panels of tests/run_cases.py guarantee, and the oracle against the real reference
(oracle/_ref) on them -- calcLOD's jumps and assembleROHWindows' four-branch machine under hundreds of runs per
chromosome, bit for bit.  The figures each guarantee reached are printed (pytest -s) and quoted in DESIGN.md section 5."""
import numpy as np
import pytest

import oracle_lib as ol
import run_cases as rc

MG = rc.MAX_GAP
needs_ref = pytest.mark.skipif(not ol.have_ref(), reason="oracle/_ref/libgarlic_ref.so not built")


@pytest.fixture(scope="module")
def dense12():
    """W -> (chroms, guarantees with the cutoff-0 share, oracle scores) of the dense panel at 12 individuals"""
    cache = {}

    def get(W):
        if W not in cache:
            chroms, _ = rc.dense(W, 12)
            scores = [ol.oracle_calc_lod(g, f, p, cs, ce, W, 0.001, MG) for g, f, p, cs, ce in chroms]
            cache[W] = (chroms, rc.guarantees(chroms, W, MG, scores=scores, cutoffs=(0.0,)), scores)
        return cache[W]
    return get


@pytest.mark.parametrize("W", [2, 5, 10, 16, 30, 33, 100, 150, 250])
def test_dense_panel_guarantees(dense12, W):
    chroms, g, scores = dense12(W)
    segs = len(rc.oracle_segments(chroms, scores, W, 0.0, MG, 0.25))
    print(f"dense W={W}: snps {g['n_snps']} runs {g['n_runs']} valid share {g['valid_share']:.2f} "
          f"score>=0 share {g['share_at_or_above'][0.0]:.2f} words with >=2 runs {g['words_2runs']} >=3 runs {g['words_3runs']} "
          f">=2 breaks {g['words_2breaks']} runs by valid windows {g['runs_by_valid']} segments {segs}")
    if W in (2, 5, 10):
        assert g["words_2runs"] >= 100
    if W == 2:
        assert g["words_3runs"] >= 10
    if W in (16, 30):
        assert g["words_2runs"] >= 5
    if W >= 33:         # W - 1 >= 32 MISSING windows separate any two runs' valid windows: no word holds two
        assert g["words_2runs"] == 0 and g["words_3runs"] == 0
    for k in rc.VALID_COUNTS:
        assert g["runs_by_valid"][k] >= 5, k
    assert 0.05 <= g["share_at_or_above"][0.0] <= 0.8
    assert segs >= 200
    assert g["words_2breaks"] >= 5


def test_variant_guarantees():
    for W in (2, 10, 33):
        chroms, g = rc.centromere(W, 3)
        # 120 one-SNP runs inside the centromere of chromosome 0, the run behind it, and one break in chromosome 1
        assert g["n_runs"] == 1 + 120 + 1 + 2 + 1, g["n_runs"]
        b0 = rc.breaks_of(*chroms[0][2:5], MG)
        assert np.count_nonzero(b0) == 122 and np.count_nonzero(rc.breaks_of(*chroms[1][2:5], MG)) == 2
        assert g["words_2breaks"] >= 4
        chroms, g = rc.borders(W, 3)
        starts = np.flatnonzero(rc.breaks_of(*chroms[1][2:5], MG)) + 5
        for s in rc.BORDER_LOCI + tuple(range(*rc.BORDER_STRETCH)):
            assert s in starts
        assert g["n_runs"] == 2 + len(set(rc.BORDER_LOCI) | set(range(*rc.BORDER_STRETCH))) and g["n_runs"] >= 302
        chroms, g = rc.all_breaks(W, 3)
        assert g["valid_share"] == 0.0 and g["n_runs"] == g["n_snps"]
        chroms, g = rc.from_zero(W, 3)
        assert g["n_runs"] > 100
        print(f"W={W}: from_zero runs {g['n_runs']} words >=2 runs {g['words_2runs']}")
    chroms, g = rc.many_blocks()
    print(f"many_blocks: snps {g['n_snps']} runs {g['n_runs']} words >=2 runs {g['words_2runs']} >=3 {g['words_3runs']}")
    assert g["n_snps"] == 140000 and -(-g["n_snps"] // 2048) == 69 and 8000 <= g["n_runs"] <= 10000
    assert rc.n_boundaries(chroms, MG) == g["n_runs"]


# ------------------------------------------------------------------------------------------ oracle == reference

def _case(name, W, nind=12):
    return rc.CASES[name](W, nind)[0]


@needs_ref
@pytest.mark.parametrize("W", [2, 10, 33])
@pytest.mark.parametrize("name", ["dense", "centromere", "borders", "all_breaks", "from_zero"])
def test_oracle_equals_reference_on_dense_runs(name, W):
    """calcLOD (plain and with likelihoods), calcwLOD (1 and 4 threads), assembleROHWindows and
    convertWinData2DoubleData of the real reference against the oracle's, on every variant, bit for bit"""
    rng = np.random.default_rng([W, len(name)])
    n_segs = 0
    for c, (g, f, p, cs, ce) in enumerate(_case(name, W)):
        gl = rng.choice([1e-16, 1e-3, 0.01, 0.5, 1.0], size=g.shape)
        win = ol.oracle_calc_lod(g, f, p, cs, ce, W, 0.001, MG)
        assert ol.bits_equal(win, ol.ref_calc_lod(g, f, p, cs, ce, W, 0.001, MG)), (name, W, c)
        assert ((win != ol.MISSING) == ol.oracle_mask(p, cs, ce, W, MG)[None, :].astype(bool)).all()
        assert ol.bits_equal(ol.oracle_calc_lod(g, f, p, cs, ce, W, 0.001, MG, gl=gl),
                             ol.ref_calc_lod(g, f, p, cs, ce, W, 0.001, MG, gl=gl)), (name, W, c, "gl")
        gpos = p * 1e-6
        ld = rng.uniform(1.0, max(2.0, W / 4.0), size=(g.shape[0], W))
        for threads in (1, 4):
            for use_gl in (None, gl):
                a = ol.oracle_calc_wlod(g, f, p, gpos, ld, cs, ce, W, 0.001, MG, 1e-9, 7, gl=use_gl, threads=threads)
                b = ol.ref_calc_wlod(g, f, p, gpos, ld, cs, ce, W, 0.001, MG, 1e-9, 7, gl=use_gl, threads=threads)
                assert ol.bits_equal(a, b), (name, W, c, "wlod", threads, use_gl is not None)
        for step in (1, 7, W):
            assert ol.bits_equal(ol.oracle_flatten(win, step), ol.ref_flatten(win, step)), (name, W, c, step)
        for cutoff in (0.0, -2.5):
            cov = ol.oracle_roh_coverage(win, W, cutoff)
            for frac in (1e-9, 0.25, 1.0):
                want = ol.ref_assemble_roh(win, p, cs, ce, cutoff, W, MG, frac)
                segs = ol.oracle_roh_segments(cov, p, cs, ce, W, MG, frac)
                assert [(i, float(p[a]), float(p[b])) for i, a, b in segs] == want, (name, W, c, cutoff, frac)
                n_segs += len(want)
    assert (n_segs == 0) == (name == "all_breaks" and W >= 2)
