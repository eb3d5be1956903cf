"""GPU: the 16-bit likelihood dictionary (garlic_panel_set_gl_codes16, GARLIC_TGLS_DICTIONARY16).  Every value is compared
bit for bit with the CPU oracle on the doubles the codes stand for (tests/dict16_cases.py); no tolerance.

A panel enters the mode through garlic_panel_set_gl_codes16 only: tests/test_gpu_tgls_continuous.py pins that
garlic_panel_set_gl and garlic_panel_set_gl_codes uploads past 256 values turn a one-byte panel continuous, so those two
doors are checked here as uploads INTO a panel that already holds 16-bit codes (they are then merged into its table)."""
import contextlib
import os

import numpy as np
import pytest

import dict16_cases as cases
import oracle_lib as ol
import tgls_feed_cases as fcases
import tgls_slab_cases as scases
from garlic_amd import abi

pytestmark = pytest.mark.gpu
MG, ERROR, FRAC, M, MU = cases.MG, cases.ERROR, cases.FRAC, cases.M, cases.MU
D16 = abi.TGLS_DICTIONARY16


@contextlib.contextmanager
def env(**kw):
    old = {k: os.environ.get(k) for k in kw}
    os.environ.update({k: str(v) for k, v in kw.items()})
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def open_panel(ctx, chroms=None, gpos=None):
    if chroms is None:
        chroms, gpos = cases.panel()
    panel = abi.Panel(ctx, [c[0].shape[0] for c in chroms], chroms[0][0].shape[1])
    panel.set_map(np.concatenate([c[2] for c in chroms]), [c[3] for c in chroms], [c[4] for c in chroms],
                  gpos=None if gpos is None else np.concatenate(gpos))
    panel.set_freq(np.concatenate([c[1] for c in chroms]))
    panel.set_genotypes(np.concatenate([c[0] for c in chroms], axis=0))
    return panel


def same(got, want, what):
    for c in range(len(want)):
        g, w = np.ascontiguousarray(got[c]), np.ascontiguousarray(want[c])
        assert ol.bits_equal(g, w), (what, c, ol.count_mismatch(g, w))


def check_lod(panel, nvalues, W, what, freq_seed=0, **kw):
    got = panel.lod_windows(W, ERROR, MG, use_gl=True, **kw)
    same(got, cases.lod_scores(nvalues, W, freq_seed), (what, "lod", W))
    return got


def check_wlod(panel, nvalues, W, what, freq_seed=0, **kw):
    """LD weights from garlic_panel_compute_ld; the oracle gets the same weights"""
    lds = cases.split_ld(panel.compute_ld(W))
    got = panel.wlod_windows(W, ERROR, MG, M, MU, use_gl=True, **kw)
    same(got, cases.wlod_scores(nvalues, W, lds, freq_seed), (what, "wlod", W))
    return got


# ------------------------------------------------------------------------------------------------ 1. scores

@pytest.mark.parametrize("nvalues", cases.NVALUES)
def test_scores_match_the_oracle(gpu_ctx, nvalues):
    values, codes, _ = cases.codes_of(nvalues)
    with open_panel(gpu_ctx) as panel:
        panel.set_gl_codes16(np.concatenate(codes, axis=0), values)
        assert panel.tgls_mode()[0] == D16
        for W in cases.WIDTHS:
            check_lod(panel, nvalues, W, nvalues, pitch_align=32)
            assert panel.chain_kind() == 0
            assert panel.tgls_mode() == (D16, 1), "the terms must come from the device's log10 on this host"
            check_wlod(panel, nvalues, W, nvalues, pitch_align=32)
        check_lod(panel, nvalues, 40, (nvalues, "dense rows"), pitch_align=1)
        got = panel.lod_windows(33, ERROR, MG, use_gl=True, ind_begin=37, ind_count=70, pitch_align=32)      # unaligned sub-range
        same(got, [s[37:107] for s in cases.lod_scores(nvalues, 33)], (nvalues, "sub-range"))
        assert panel.tgls_mode()[0] == D16


# ------------------------------------------------------------------------------------------------ 2. same data, three doors

def test_same_data_through_three_doors(gpu_ctx):
    """all of it through set_gl_codes16; or a first chunk through set_gl_codes16 and the rest as doubles through set_gl; or the
    rest through set_gl_codes chunks with one-byte tables of their own that together pass 256 values: identical scores, and
    the panel stays in the 16-bit mode.  Also: one-byte codes first, widened by the first set_gl_codes16 chunk."""
    nvalues, W = 1000, 40
    values, codes, gl = cases.codes_of(nvalues)
    allc, allg = np.concatenate(codes, axis=0), np.concatenate(gl, axis=0)
    n = allc.shape[0]
    results = []

    def chunk_tables(lo, hi):
        """rows [lo, hi) as one-byte codes, every row with a table of its own (130 genotypes: at most 130 values)"""
        for a in range(lo, hi):
            tab, inv = np.unique(allg[a], return_inverse=True)
            yield a, inv.reshape(1, -1).astype(np.uint8), tab

    for door in ("codes16", "codes16 chunks", "set_gl", "set_gl_codes", "one byte first"):
        with open_panel(gpu_ctx) as panel:
            if door == "codes16":
                panel.set_gl_codes16(allc, values)
            elif door == "codes16 chunks":          # every chunk with a table of its own, in its own order
                for a in range(0, n, 97):
                    tab, inv = np.unique(allg[a:a + 97], return_inverse=True)
                    panel.set_gl_codes16(inv.reshape(-1, cases.NIND).astype(np.uint16), tab, locus_begin=a)
            elif door == "set_gl":
                panel.set_gl_codes16(allc[:100], values)
                for a in range(100, n, 250):
                    panel.set_gl(allg[a:a + 250], locus_begin=a)
            elif door == "set_gl_codes":
                panel.set_gl_codes16(allc[:100], values[: int(allc[:100].max()) + 1])
                seen = set()
                for a, c8, tab in chunk_tables(100, n):
                    panel.set_gl_codes(c8, tab, locus_begin=a)
                    seen |= set(tab.tolist())
                assert len(seen) > 256
            else:
                # few values first: a one-byte dictionary; the 16-bit upload widens what is there
                first = np.unique(allg[:20])[:200]
                rows = np.searchsorted(first, np.clip(allg[:20], first[0], first[-1])).clip(0, first.shape[0] - 1).astype(np.uint8)
                panel.set_gl_codes(rows, first)
                assert panel.tgls_mode()[0] == abi.TGLS_DICTIONARY
                panel.set_gl_codes16(allc[20:], values, locus_begin=20)
                assert panel.tgls_mode()[0] == D16
                got = panel.lod_windows(W, ERROR, MG, use_gl=True, pitch_align=32)
                chroms = cases.panel()[0]
                mixed = np.concatenate([first[rows], allg[20:]], axis=0)
                same(got, fcases.tgls_scores(chroms, cases.split_ld(mixed), W), "widened one-byte rows")
                panel.set_gl_codes16(allc[:20], values)          # ... and now the real rows
            assert panel.tgls_mode()[0] == D16, door
            results.append(np.concatenate([np.ascontiguousarray(x).ravel() for x in check_lod(panel, nvalues, W, door, pitch_align=32)]))
            results.append(np.concatenate([np.ascontiguousarray(x).ravel() for x in check_wlod(panel, nvalues, W, door, pitch_align=32)]))
            assert panel.tgls_mode()[0] == D16, door
    for k in range(2, len(results)):
        assert ol.bits_equal(results[k], results[k % 2])


# ------------------------------------------------------------------------------------------------ 3. overflow

def test_table_overflow_turns_the_panel_continuous(gpu_ctx):
    nvalues, W = 65536, 40
    values, codes, gl = cases.codes_of(nvalues)
    allc = np.concatenate(codes, axis=0)
    chroms = cases.panel()[0]
    extra = np.array([0.123456789, 0.987654321])          # two values the full table does not hold
    assert not np.isin(extra, values).any()
    new_rows = np.random.default_rng(5).integers(0, 2, size=(50, cases.NIND)).astype(np.uint16)
    allg = np.concatenate(gl, axis=0).copy()
    allg[300:350] = extra[new_rows]
    want = fcases.tgls_scores(chroms, cases.split_ld(allg), W)
    for door in ("codes16", "set_gl", "set_gl_codes"):
        with open_panel(gpu_ctx) as panel:
            panel.set_gl_codes16(allc, values)
            assert panel.tgls_mode()[0] == D16
            if door == "codes16":
                panel.set_gl_codes16(new_rows, extra, locus_begin=300)
            elif door == "set_gl":
                panel.set_gl(allg[300:350], locus_begin=300)
            else:
                panel.set_gl_codes(new_rows.astype(np.uint8), extra, locus_begin=300)
            assert panel.tgls_mode()[0] == abi.TGLS_CONTINUOUS, door
            same(panel.lod_windows(W, ERROR, MG, use_gl=True, pitch_align=32), want, ("overflow", door))
            panel.set_gl_codes16(allc[300:350], values, locus_begin=300)      # codes into a continuous panel: stored as values
            assert panel.tgls_mode()[0] == abi.TGLS_CONTINUOUS
            check_lod(panel, nvalues, W, ("overflow, rows restored", door), pitch_align=32)


# ------------------------------------------------------------------------------------------------ 4. budget

def every_call(panel, nvalues, budget, what):
    """unweighted and weighted scores, feeds in both orders, the multi-size feed, coverage and segments; each against the oracle"""
    chroms = cases.panel()[0]
    sizes, nloci = cases.SIZES, sum(cases.SIZES)
    whole = (cases.ROWS_PAD + nloci) * scases.nind_pad_of(cases.NIND) * 8
    res = {}

    def info(tag, slabs=True):
        i = panel.tgls_terms_info()
        print(what, tag, i)
        assert i["whole_bytes"] == whole
        if budget:
            assert i["resident_bytes"] <= budget, (what, tag, i)
            if slabs:
                k = scases.slab_blocks_for(budget, nloci, cases.NIND)
                assert (i["slab_blocks"], i["n_slabs"]) == (k, -(-3 // k)), (what, tag, i)
        else:
            assert i["n_slabs"] == 0 and i["resident_bytes"] == whole, (what, tag, i)

    W = 40
    flat = lambda got: np.concatenate([np.ascontiguousarray(x).ravel() for x in got])
    res["lod"] = flat(check_lod(panel, nvalues, W, what, pitch_align=32))
    info("lod")
    res["wlod"] = flat(check_wlod(panel, nvalues, W, what, pitch_align=32))
    info("wlod")
    scores = cases.lod_scores(nvalues, W)
    for order in (abi.FEED_ORDER_REFERENCE, abi.FEED_ORDER_SORTED):
        panel.set_feed_order(order)
        feed, per_chr = panel.lod_feed(W, ERROR, MG, W, use_gl=True)
        want = np.concatenate(fcases.flat(scores, W))
        assert feed.shape[0] > 0 and ol.bits_equal(feed, np.sort(want) if order else want), (what, "feed", order)
        assert panel.feed_info()[0] == abi.FEED_TGLS_CHAIN
        info(("feed", order))
        res["feed %d" % order] = feed
    panel.set_feed_order(abi.FEED_ORDER_REFERENCE)
    feeds, _ = panel.lod_feed_multi_tgls(cases.FEED_SIZES, MG)
    for Wk, feed in zip(cases.FEED_SIZES, feeds):
        want = np.concatenate(fcases.flat(cases.lod_scores(nvalues, Wk), Wk))
        assert feed.shape[0] > 0 and ol.bits_equal(feed, want), (what, "multi feed", Wk)
        res["multi %d" % Wk] = feed.copy()
    mi = panel.feed_multi_info(len(cases.FEED_SIZES))
    assert mi["forms"] == [abi.FEED_TGLS_CHAIN_SHARED] * 3, mi
    info("multi feed")
    cutoff = scases.cutoff_of(scores)
    cov = panel.roh_coverage_fused(W, ERROR, MG, cutoff, pitch_align=8, use_gl=True)
    for c, n_c in enumerate(sizes):
        assert np.array_equal(cov[c][:, :n_c], ol.oracle_roh_coverage(np.ascontiguousarray(scores[c]), W, cutoff)), (what, "coverage", c)
    info("coverage")
    res["cov"] = np.concatenate([np.ascontiguousarray(x[:, :n_c]).ravel() for x, n_c in zip(cov, sizes)])
    segs = [tuple(int(v) for v in r) for r in panel.roh_segments(W, ERROR, MG, cutoff, FRAC, use_gl=True)]
    want = scases.oracle_segments(chroms, scores, W, cutoff)
    assert len(want) > 0 and segs == want, (what, "segments", len(segs), len(want))
    info("segments")
    res["segs"] = np.array(segs)
    return res


def test_every_call_under_the_term_budget(gpu_ctx):
    nvalues = 1000
    values, codes, _ = cases.codes_of(nvalues)
    with open_panel(gpu_ctx) as panel:
        panel.set_gl_codes16(np.concatenate(codes, axis=0), values)
        base = every_call(panel, nvalues, 0, "budget 0")
        for k, budget in cases.budgets():
            panel.set_tgls_term_budget(budget)
            got = every_call(panel, nvalues, budget, "slabs of %d" % k)
            assert got.keys() == base.keys()
            for key in base:
                a, b = base[key], got[key]
                assert (ol.bits_equal(a, b) if a.dtype == np.float64 else np.array_equal(a, b)), (k, key)
        assert panel.tgls_mode()[0] == D16
        # two slabs: the first two blocks under the one-block budget
        panel.set_tgls_term_budget(cases.budgets()[0][1])
        got = panel.lod_windows(40, ERROR, MG, use_gl=True, ind_begin=0, ind_count=128, pitch_align=32)
        same(got, [s[:128] for s in cases.lod_scores(nvalues, 40)], "two slabs")
        assert panel.tgls_terms_info()["n_slabs"] == 2
        lds = cases.split_ld(panel.compute_ld(40))
        got = panel.wlod_windows(40, ERROR, MG, M, MU, use_gl=True, ind_begin=0, ind_count=128, pitch_align=32)
        same(got, [s[:128] for s in cases.wlod_scores(nvalues, 40, lds)], "two slabs, weighted")
        assert panel.tgls_terms_info()["n_slabs"] == 2
        # shapes that slabs do not cover are refused with a message that says so: there is no look-up kernel to fall back to
        with pytest.raises(abi.GarlicError) as e:
            panel.lod_windows(40, ERROR, MG, use_gl=True, ind_begin=37, ind_count=70, pitch_align=32)
        assert e.value.code == abi.ERR_NOMEM and "not covered by term slabs" in str(e.value)
        panel.compute_ld(40, want_output=False)
        with pytest.raises(abi.GarlicError) as e:
            panel.wlod_windows(40, ERROR, MG, M, MU, use_gl=True, ind_begin=37, ind_count=70, pitch_align=32)
        assert e.value.code == abi.ERR_NOMEM and "not covered by term slabs" in str(e.value)
        with env(GARLIC_WLOD_GENERIC=1):                 # the generic weighted kernel reads the whole raw matrix
            with pytest.raises(abi.GarlicError) as e:
                panel.wlod_windows(40, ERROR, MG, M, MU, use_gl=True, pitch_align=32)
            assert e.value.code == abi.ERR_NOMEM and "not covered by term slabs" in str(e.value)
            panel.set_tgls_term_budget(0)
            check_wlod(panel, nvalues, 40, "generic weighted kernel, whole matrix", pitch_align=32)


# ------------------------------------------------------------------------------------------------ 5. no re-upload

def test_no_reupload_when_terms_are_rebuilt(gpu_ctx):
    """unweighted, weighted, new frequencies, unweighted again, under a budget that holds two one-block buffers: raw and scaled
    terms can never both stay.  The codes are never overwritten, so no call answers GARLIC_ERR_STATE."""
    nvalues, W = 257, 40
    values, codes, _ = cases.codes_of(nvalues)
    for budget in (cases.budgets()[0][1], 0):
        with open_panel(gpu_ctx) as panel:
            panel.set_gl_codes16(np.concatenate(codes, axis=0), values)
            panel.set_tgls_term_budget(budget)
            check_lod(panel, nvalues, W, ("first", budget), pitch_align=32)
            check_wlod(panel, nvalues, W, ("weighted", budget), pitch_align=32)
            check_lod(panel, nvalues, W, ("raw again", budget), pitch_align=32)
            panel.set_freq(np.concatenate([c[1] for c in cases.with_freq(1)]))
            check_wlod(panel, nvalues, W, ("weighted, new frequencies", budget), freq_seed=1, pitch_align=32)
            check_lod(panel, nvalues, W, ("new frequencies", budget), freq_seed=1, pitch_align=32)
            panel.set_genotypes(np.concatenate([c[0] for c in cases.panel()[0]], axis=0))      # the same genotypes, uploaded again
            check_lod(panel, nvalues, 100, ("after a genotype upload", budget), freq_seed=1, pitch_align=32)
            if budget:
                assert panel.tgls_terms_info()["resident_bytes"] <= budget
            assert panel.tgls_mode()[0] == D16


# ------------------------------------------------------------------------------------------------ 6. -9999.0

def test_wide_window_over_the_smallest_value_is_scanned(gpu_ctx):
    """640 x log10(1e-16) <= -9990: the chain kind is decided before any term exists and must not be 0"""
    chroms, values, codes, gl, scores = cases.exact_case()
    W = cases.EXACT_W
    for budget in (0, scases.budget_for(700, 1, 70)):
        with open_panel(gpu_ctx, chroms) as panel:
            panel.set_gl_codes16(codes[0], values)
            panel.set_tgls_term_budget(budget)
            same(panel.lod_windows(W, ERROR, MG, use_gl=True, pitch_align=32), scores, ("sentinel", budget))
            assert panel.chain_kind() >= 1
            same(panel.lod_windows(10, ERROR, MG, use_gl=True, pitch_align=32), fcases.tgls_scores(chroms, gl, 10), ("narrow", budget))
            assert panel.chain_kind() == 0
            feed, _ = panel.lod_feed(W, ERROR, MG, W, use_gl=True)      # the sampled ring form is not taken: from full scores
            assert ol.bits_equal(feed, np.concatenate(fcases.flat(scores, W))) and panel.feed_info()[0] == abi.FEED_FROM_SCORES
            # a frequency so small that 2 f (1 - f) is subnormal: the heterozygous term is no longer log10(value), so there is
            # no bound and even a narrow window is scanned
            g, f, p, cs, ce = chroms[0]
            tiny = f.copy()
            tiny[5] = 1e-310
            panel.set_freq(tiny)
            same(panel.lod_windows(10, ERROR, MG, use_gl=True, pitch_align=32), fcases.tgls_scores([(g, tiny, p, cs, ce)], gl, 10),
                 ("subnormal genotype probability", budget))
            assert panel.chain_kind() >= 1


# ------------------------------------------------------------------------------------------------ 7. host fall-back

def test_terms_on_the_host_when_forced(gpu_ctx):
    nvalues, W = 1000, 40
    values, codes, _ = cases.codes_of(nvalues)
    with env(GARLIC_TGLS_HOST_TERMS=1), open_panel(gpu_ctx) as panel:
        panel.set_gl_codes16(np.concatenate(codes, axis=0), values)
        check_lod(panel, nvalues, W, "host terms", pitch_align=32)
        assert panel.tgls_mode() == (D16, 2)
        check_wlod(panel, nvalues, W, "host terms", pitch_align=32)
        assert panel.tgls_mode() == (D16, 2)
        panel.set_tgls_term_budget(cases.budgets()[0][1])
        check_lod(panel, nvalues, W, "host terms, slabs", pitch_align=32)
        assert panel.tgls_terms_info()["n_slabs"] == 3 and panel.tgls_mode() == (D16, 2)      # who built the slabs
        check_wlod(panel, nvalues, W, "host terms, slabs", pitch_align=32)
        assert panel.tgls_terms_info()["n_slabs"] == 3 and panel.tgls_mode() == (D16, 2)
    with open_panel(gpu_ctx) as panel:                   # and without the switch the slabs are the device's
        panel.set_gl_codes16(np.concatenate(codes, axis=0), values)
        panel.set_tgls_term_budget(cases.budgets()[0][1])
        check_lod(panel, nvalues, W, "device terms, slabs", pitch_align=32)
        assert panel.tgls_terms_info()["n_slabs"] == 3 and panel.tgls_mode() == (D16, 1)


# ------------------------------------------------------------------------------------------------ 8. the tool

def test_tool_reads_gl_columns_with_thousands_of_values(tmp_path):
    """garlic-lod --tgls F --gl-type GL --raw-lod on the tool fixture's genotypes (tests/golden/e2e: 6000 SNPs x 24 individuals,
    3 chromosomes, monomorphic SNPs for the filter to drop) with GL columns of three printed decimals written here: about 5000
    distinct values a chromosome.  The raw scores are the oracle's to the six printed digits (the same %g text), the KDE feed is
    oracle_flatten of them bit for bit, and under --tgls-term-gb every file is the same.  Before the 16-bit form the tool
    stopped with "more than 256 distinct genotype likelihood values"."""
    import gzip
    import math
    import re
    import subprocess

    import test_gpu_host_tool as ht                      # its TPED re-parse (tiny_panels) and file names
    import test_gpu_host_tool_slabs as hs                # block_gb, assert_same_files

    W = 30
    rng = np.random.default_rng(20260119)
    tgls = str(tmp_path / "gl.tgls.gz")
    x_rows, keep_rows = [], []
    with gzip.open(os.path.join(ht.E2E, "tiny.tped.gz"), "rt") as f, gzip.open(tgls, "wt") as g:
        for line in f:
            t = line.split()
            k = rng.integers(0, 5000, size=24)
            k[rng.random(24) < 0.01] = 12000             # below the clamp at -10
            g.write(" ".join(t[:4] + ["%.3f" % (-v / 1000.0) for v in k]) + "\n")
            x_rows.append((t[0], [float("%.3f" % (-v / 1000.0)) for v in k]))

    def convert(x):                                      # garlic-data.cpp:1557-1576 for GL, operation for operation
        v = 1 - math.pow(10, x if x > -10 else -10)
        return 1e-16 if v <= 0 else min(v, 1.0)

    per_chr = ht.tiny_panels()
    # the filter of tiny_panels again, for the likelihood rows: same order, same SNPs
    chrom_names, gl_chr = [], []
    with gzip.open(os.path.join(ht.E2E, "tiny.tped.gz"), "rt") as f:
        rows = [line.split() for line in f]
    for c in dict.fromkeys(r[0] for r in rows):
        chrom_names.append(c if c.startswith("chr") else "chr" + c)
        sel = [i for i, r in enumerate(rows) if r[0] == c]
        gl = np.array([[convert(x) for x in x_rows[i][1]] for i in sel])
        freq = []
        for i in sel:
            al = [a for a in rows[i][4:] if a != "0"]
            freq.append(sum(a == al[0] for a in al) / len(al) if al else 0.0)
        freq = np.array(freq)
        gl_chr.append(gl[(freq > 0) & (freq < 1)])
        assert np.unique(gl).shape[0] > 256
    assert [g.shape[0] for g in gl_chr] == [p[0].shape[0] for p in per_chr] and sum(g.shape[0] for g in gl_chr) < len(rows)

    def run(name, *extra):
        out_dir = tmp_path / name
        out_dir.mkdir()
        cmd = [ht.TOOL, "--tped", os.path.join(ht.E2E, "tiny.tped.gz"), "--tfam", os.path.join(ht.E2E, "tiny.tfam"),
               "--centromere", os.path.join(ht.E2E, "tiny.centromeres.txt"), "--out", str(out_dir / "o"), "--kde-subsample", "0",
               "--winsize", str(W), "--raw-lod", "--tgls", tgls, "--gl-type", "GL", "--lod-cutoff", "-11",
               "--size-bounds", "50000", "200000"] + list(extra)
        r = subprocess.run(cmd, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-2000:]
        return str(out_dir), r.stderr

    plain, err = run("plain")
    assert re.search(r"Genotype likelihoods \(GL\): .* as 16-bit codes \(\d{4} values\)", err), err[-800:]
    assert "one-byte" not in err and "as doubles" not in err
    feed = []
    for c, ((g, f, p, (cs, ce)), gl) in enumerate(zip(per_chr, gl_chr)):
        want = ol.oracle_calc_lod(g, f, p, cs, ce, W, 0.001, 200000, gl=np.ascontiguousarray(gl))
        got = ht.read_rows(os.path.join(plain, "o.POP.%s.raw.lod.windows.gz" % chrom_names[c]))
        assert len(got) == 24
        for i in range(24):
            assert got[i] == ["NA" if v == ol.MISSING else "%g" % v for v in want[i]], (c, i)
        feed.append(ol.oracle_flatten(want, W))
    assert ol.bits_equal(np.fromfile(os.path.join(plain, "o.%dSNPs.lod.f64" % W), dtype=np.float64), np.concatenate(feed))
    slabs, err = run("slabs", "--tgls-term-gb", "%.9f" % (hs.block_gb(hs.NLOCI) + 1e-9))
    assert re.search(r"TGLS terms .*: last call in 1 slabs of 1 blocks", err), err[-500:]
    hs.assert_same_files(plain, slabs)
