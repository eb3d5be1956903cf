"""GPU: phased LD weights on the matrix cores (ld_pair_mfma_kernel<.., PHASED>: three Gram products per block, x11 from the
two haplotype planes) against the CPU oracle and the numpy counts, bit for bit; garlic_panel_ld_form_info; the phase uploaded
as bit rows (garlic_panel_set_phase_bits) against the byte upload.  Cases and restatements: tests/ld_phased_cases.py."""
import ctypes as C

import numpy as np
import pytest

import ld_phased_cases as lp
import ld_wide_cases as lw
import oracle_lib as ol
from garlic_amd import abi

pytestmark = pytest.mark.gpu

X86_NAN = 0xFFF8000000000000


def make_panel(ctx, chroms, nind, phase=None, bits=False):
    panel = abi.Panel(ctx, [c[0].shape[0] for c in chroms], nind)
    pos = np.concatenate([c[2] for c in chroms])
    panel.set_map(pos, [c[3] for c in chroms], [c[4] for c in chroms], gpos=pos * 1e-6)
    panel.set_freq(np.concatenate([c[1] for c in chroms]))
    panel.set_genotypes(np.concatenate([c[0] for c in chroms], axis=0))
    if phase is not None and bits:
        panel.set_phase_bits(lp.pack_phase_rows(phase))
    elif phase is not None:
        panel.set_phase(phase)
    return panel


def case_panel(ctx, nind, w):
    chroms, phase, _ = lp.panel(nind, w)
    return make_panel(ctx, chroms, nind, phase)


def form(panel):
    return panel.ld_form_info()


@pytest.mark.parametrize("nind,w", lp.CASES)
def test_fused_weights_match_oracle(gpu_ctx, nind, w):
    """compute_ld(phased) -- the fused form: the pair kernel writes the r2 table -- against oracle_r2_ld for everyone, a third
    and one block only; the form info says matrix cores, fused, phased"""
    _, _, subs = lp.panel(nind, w)
    with case_panel(gpu_ctx, nind, w) as panel:
        with pytest.raises(abi.GarlicError) as e:
            panel.ld_form_info()
        assert e.value.code == abi.ERR_STATE
        for name in lp.SUBS:
            got = panel.compute_ld(w, sub_idx=subs[name], phased=True)
            # 32 < W: the sum kernel that reads the table the pair kernel can write itself; W = 17 sums two tables
            assert form(panel) == (abi.LD_PAIR_MFMA, abi.LD_SUM_COL if w > 32 else abi.LD_SUM_TILED, w > 32, True), (nind, w, name)
            assert ol.bits_equal(got, lp.oracle_weights(nind, w, name)), (nind, w, name)


@pytest.mark.parametrize("nind,w", lp.CASES)
def test_counts_match_numpy_and_finish_to_the_same_weights(gpu_ctx, monkeypatch, nind, w):
    """ld_counts(phased) == {2 tot, x11} of numpy; ld_finish on them == the fused call's weights; and the same call under
    GARLIC_LD_UNFUSED (the kernel's counts epilogue, then ld_finish's kernels)"""
    chroms, phase, subs = lp.panel(nind, w)
    want_loc = lw.locus_counts(chroms)
    with case_panel(gpu_ctx, nind, w) as panel:
        for name in lp.SUBS:
            loc, pair = panel.ld_counts(w, sub_idx=subs[name], phased=True)
            assert form(panel)[0] == abi.LD_PAIR_MFMA and form(panel)[2:] == (False, True)
            want = lw.phased_pair_counts(chroms, phase, w, subs[name])
            assert np.array_equal(loc, want_loc), (nind, w, name)
            bad = np.argwhere(pair != want)
            assert bad.shape[0] == 0, (nind, w, name, bad.shape[0], bad[:4].tolist())
            got = panel.ld_finish(w, loc, pair, phased=True)
            assert form(panel)[2:] == (False, True)
            assert ol.bits_equal(got, lp.oracle_weights(nind, w, name)), (nind, w, name)
        monkeypatch.setenv("GARLIC_LD_UNFUSED", "1")
        for name in lp.SUBS:
            got = panel.compute_ld(w, sub_idx=subs[name], phased=True)
            assert form(panel)[0] == abi.LD_PAIR_MFMA and form(panel)[2:] == (False, True)
            assert ol.bits_equal(got, lp.oracle_weights(nind, w, name)), ("unfused", nind, w, name)


@pytest.mark.parametrize("sizes,pair", [([40, 100], abi.LD_PAIR_MFMA), ([17, 129, 130], abi.LD_PAIR_LANE)])
def test_phased_multi_size_call(gpu_ctx, sizes, pair):
    """compute_ld_multi(phased): every size equals its single call bit for bit; the form is that of the widest sharing size's
    pair stage -- 100: matrix cores, fused; 130 (NJ = 6): the lane kernel"""
    nind = 130
    chroms, phase, subs = lp.panel(nind, 100)
    with make_panel(gpu_ctx, chroms, nind, phase) as panel:
        for name in ("all", "third"):
            single = {w: panel.compute_ld(w, sub_idx=subs[name], phased=True) for w in sizes}
            got = panel.compute_ld_multi(sizes, sub_idx=subs[name], phased=True)
            assert form(panel) == (pair, abi.LD_SUM_COL, pair == abi.LD_PAIR_MFMA, True)
            for w, ld in zip(sizes, got):
                assert ol.bits_equal(ld, single[w]), (w, name)
        if 100 in sizes:                                           # (single: the last subsample's)
            assert ol.bits_equal(single[100], lp.oracle_weights(nind, 100, "third"))


def test_special_values(gpu_ctx):
    """0/0 -> the x86 NaN with the sign set, handed through to the weights; freq 0 and 1 -> r2 = 0; r2 > 1 clamped: the
    oracle's values, and the oracle's table has them where the panel was built to produce them"""
    chroms, phase, w = lp.special_panel()
    g, f = chroms[0][0], chroms[0][1]
    nind = g.shape[1]
    want = lw.oracle_r2(chroms, phase, w)
    bits = want.view(np.uint64)
    # the window starting at 0 holds SNPs 4 and 6 (and 13, which nobody is genotyped at): their columns sum a 0/0 term
    assert bits[0, 4] == X86_NAN and bits[0, 6] == X86_NAN and not (np.isnan(want) & (bits != X86_NAN)).any()
    # column of SNP 10 (freq 0) in the window starting at 10: 1.0 for itself, 0 for every partner
    assert want[10, 0] == 1.0 and want[10, 1] == 1.0
    # the window starting at 20: SNP 21 as SNP 20's partner is clamped to exactly 1
    assert want[20, 0] == 17.0 and want[20, 1] == 17.0            # (every partner of SNPs 20 and 21: 17 terms of exactly 1)
    pairs = lw.phased_pair_counts(chroms, phase, w)
    assert pairs[20, 1, 0] == 2 * nind and pairs[20, 1, 1] == 2 * nind
    one = lw.ld_from_counts(g.shape[0], w, f, pairs)
    assert ol.bits_equal(one, want)                                # the restated formula (with its clamp) is the oracle's
    with make_panel(gpu_ctx, chroms, nind, phase) as panel:
        got = panel.compute_ld(w, phased=True)
        assert form(panel)[0] == abi.LD_PAIR_MFMA
        assert ol.bits_equal(got, want)
        loc, pair = panel.ld_counts(w, phased=True)
        assert np.array_equal(pair, pairs)
        assert pair[4, 2, 0] == 0 and pair[4, 2, 1] == 0           # SNPs 4 and 6: nobody has both
    w2 = 40                                                        # the fused epilogue's NaN, zero and clamp
    want2 = lw.oracle_r2(chroms, phase, w2)
    with make_panel(gpu_ctx, chroms, nind, phase) as panel:
        got = panel.compute_ld(w2, phased=True)
        assert form(panel) == (abi.LD_PAIR_MFMA, abi.LD_SUM_COL, True, True)
        assert (want2.view(np.uint64) == X86_NAN).any()
        assert ol.bits_equal(got, want2)


@pytest.mark.parametrize("switch,code", [("GARLIC_LD_PAIR_NO_MFMA", abi.LD_PAIR_LANE), ("GARLIC_LD_PAIR_TILED", abi.LD_PAIR_TILED),
                                         ("GARLIC_LD_PAIR_L2", abi.LD_PAIR_PLAIN)])
def test_switches_leave_the_form(gpu_ctx, monkeypatch, switch, code):
    """the AND + popcount kernels stay reachable for phased calls, and give the same weights"""
    nind, w = 130, 40
    chroms, phase, subs = lp.panel(nind, w)
    monkeypatch.setenv(switch, "1")
    assert lp.PAIR_CODE[lp.pair_kernel_phased(w, lw.nblk_of(nind), {switch: "1"})] == code
    with make_panel(gpu_ctx, chroms, nind, phase) as panel:
        for name in ("all", "third"):
            got = panel.compute_ld(w, sub_idx=subs[name], phased=True)
            assert form(panel) == (code, abi.LD_SUM_COL, False, True)
            assert ol.bits_equal(got, lp.oracle_weights(nind, w, name)), (switch, name)
            loc, pair = panel.ld_counts(w, sub_idx=subs[name], phased=True)
            assert np.array_equal(pair, lw.phased_pair_counts(chroms, phase, w, subs[name]))


def test_unphased_form_is_reported_too(gpu_ctx):
    nind, w = 65, 40
    chroms, _, _ = lp.panel(nind, w)
    with make_panel(gpu_ctx, chroms, nind) as panel:
        panel.compute_ld(w, want_output=False)
        assert form(panel) == (abi.LD_PAIR_MFMA, abi.LD_SUM_COL, True, False)
        panel.compute_ld(10, want_output=False)
        assert form(panel) == (abi.LD_PAIR_LANE, abi.LD_SUM_FLAT, False, False)
        # any pointer may be NULL
        assert abi.lib().garlic_panel_ld_form_info(panel.handle, None, None, None, None) == abi.OK


# ------------------------------------------------------------------------------------------------------- phase as bit rows
BITS_NINDS = [1, 63, 64, 65, 130]
BITS_W = 17


def bits_panel_data(nind):
    rng = np.random.default_rng(500 + nind)
    chroms = lw.wide_chroms(rng, [40, 23], nind)
    nloci = 63
    phase = rng.integers(0, 2, size=(nloci, nind)).astype(np.uint8)
    phase2 = phase.copy()
    het = np.concatenate([c[0] for c in chroms], axis=0) == 1
    phase2[het] ^= 1                                               # every heterozygote's phase flips ...
    phase2[::2] = phase[::2]                                       # ... at every other SNP: (1, 1) pairs change their agreement
    return chroms, phase, phase2


@pytest.mark.parametrize("nind", BITS_NINDS)
def test_phase_bits_give_the_byte_upload_weights(gpu_ctx, nind):
    """the same weights (so the same planes: F enters every (1, 1) pair) from set_phase_bits as from set_phase -- whole, in two
    pieces, with wider rows full of ones, and from device memory; then a new phase through bits changes the weights to the
    oracle's for it"""
    import torch
    chroms, phase, phase2 = bits_panel_data(nind)
    nloci = phase.shape[0]
    want = lw.oracle_r2(chroms, phase, BITS_W)
    with make_panel(gpu_ctx, chroms, nind, phase) as panel:
        by_bytes = panel.compute_ld(BITS_W, phased=True)
        by_bytes_counts = panel.ld_counts(BITS_W, phased=True)[1]
    assert ol.bits_equal(by_bytes, want)

    def check(panel, tag):
        assert ol.bits_equal(panel.compute_ld(BITS_W, phased=True), by_bytes), (tag, nind)
        assert np.array_equal(panel.ld_counts(BITS_W, phased=True)[1], by_bytes_counts), (tag, nind)

    rows = lp.pack_phase_rows(phase)
    with make_panel(gpu_ctx, chroms, nind, phase, bits=True) as panel:
        check(panel, "whole")
        # a call after a bits upload that changes the phase: different, correct weights
        panel.set_phase_bits(lp.pack_phase_rows(phase2))
        got2 = panel.compute_ld(BITS_W, phased=True)
        assert ol.bits_equal(got2, lw.oracle_r2(chroms, phase2, BITS_W))
        if nind > 1:
            assert not ol.bits_equal(got2, by_bytes)
        panel.set_phase_bits(rows[37:], locus_begin=37)           # back, in two pieces, the second first
        panel.set_phase_bits(rows[:37], locus_begin=0)
        check(panel, "pieces")
    with make_panel(gpu_ctx, chroms, nind) as panel:
        wide = lp.pack_phase_rows(phase, row_bytes=rows.shape[1] + 3, fill=0xFF)
        dirty = wide.copy()
        if nind & 7:
            dirty[:, rows.shape[1] - 1] |= np.uint8((0xFF << (nind & 7)) & 0xFF)
        panel.set_phase_bits(dirty)
        check(panel, "wide rows")
    with make_panel(gpu_ctx, chroms, nind) as panel:
        dev = torch.from_numpy(wide).cuda()
        torch.cuda.synchronize()
        panel.set_phase_bits_device(dev.data_ptr(), wide.shape[1], 0, 40)
        panel.set_phase_bits_device(dev.data_ptr() + 40 * wide.shape[1], wide.shape[1], 40, nloci - 40)
        check(panel, "device")


def test_phase_bits_bad_arguments(gpu_ctx):
    nind = 65
    chroms, phase, _ = bits_panel_data(nind)
    rows = lp.pack_phase_rows(phase)
    L = abi.lib()
    ptr = C.c_void_p(rows.ctypes.data)
    with make_panel(gpu_ctx, chroms, nind) as panel:
        h = panel.handle
        assert L.garlic_panel_set_phase_bits(None, ptr, rows.shape[1], 0, 63, abi.HOST) == abi.ERR_INVALID
        assert L.garlic_panel_set_phase_bits(h, None, rows.shape[1], 0, 63, abi.HOST) == abi.ERR_INVALID
        assert L.garlic_panel_set_phase_bits(h, ptr, rows.shape[1] - 1, 0, 63, abi.HOST) == abi.ERR_INVALID       # 8 bytes < 65 bits
        assert L.garlic_panel_set_phase_bits(h, ptr, rows.shape[1], -1, 10, abi.HOST) == abi.ERR_INVALID
        assert L.garlic_panel_set_phase_bits(h, ptr, rows.shape[1], 0, 0, abi.HOST) == abi.ERR_INVALID
        assert L.garlic_panel_set_phase_bits(h, ptr, rows.shape[1], 60, 4, abi.HOST) == abi.ERR_INVALID
        with pytest.raises(abi.GarlicError) as e:                  # nothing was uploaded: still no phase
            panel.compute_ld(BITS_W, phased=True)
        assert e.value.code == abi.ERR_STATE
        assert L.garlic_panel_set_phase_bits(h, ptr, rows.shape[1], 0, 63, abi.HOST) == abi.OK
        assert ol.bits_equal(panel.compute_ld(BITS_W, phased=True), lw.oracle_r2(chroms, phase, BITS_W))
