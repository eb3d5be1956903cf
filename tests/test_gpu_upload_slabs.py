"""GPU: host uploads that cross the staging-slab boundary.  Host rows go to the device through a staging buffer bounded by
256 MB and by no fewer than 16 rows, a slab of rows at a time; the bound is in bytes, so few rows cross it when the caller's
pitch is wide.  Every array here has a pitch of 16 MB: 33 rows travel as slabs of 16, 16 and 1 rows, through each of the eight
upload doors, and the results are the oracle's bit for bit.  Two transitions between likelihood forms happen in the last slab.

One chromosome of 33 SNPs, 70 individuals (two 64-individual blocks, the second partial), windows of 5 SNPs."""
import functools

import numpy as np
import pytest

import dict16_cases as d16
import ld_phased_cases as lp
import ld_wide_cases as lw
import oracle_lib as ol
from garlic_amd import abi
from test_gpu_parity import pack2bit

pytestmark = pytest.mark.gpu
NLOCI, NIND, W, MG, ERROR = 33, 70, 5, 200000, 0.001
PITCH_BYTES = 1 << 24          # 2^28 / 2^24 = 16 rows a slab


def wide(rows, col0=0):
    """the rows at a pitch of 16 MB (lazily mapped zeros around them), columns from col0"""
    rows = np.asarray(rows)
    out = np.zeros((rows.shape[0], PITCH_BYTES // rows.dtype.itemsize), dtype=rows.dtype)
    out[:, col0:col0 + rows.shape[1]] = rows
    assert out.flags.c_contiguous and out.strides[0] == PITCH_BYTES and rows.shape[0] == NLOCI
    return out


@functools.lru_cache(maxsize=None)
def chrom():
    rng = np.random.default_rng(3316)
    c = ol.random_panel(rng, NLOCI, NIND, max_gap=MG, gaps=0, centro=False)
    c[0].setflags(write=False)
    return c


@functools.lru_cache(maxsize=None)
def scores(gl_key=None):
    """the oracle's scores, once per likelihood matrix (gl_key names one of gl_cases())"""
    g, f, p, cs, ce = chrom()
    want = ol.oracle_calc_lod(g, f, p, cs, ce, W, ERROR, MG, gl=None if gl_key is None else gl_cases()[gl_key][2])
    assert np.count_nonzero(want != ol.MISSING) > NIND * (NLOCI - W) // 2
    want.setflags(write=False)
    return want


@functools.lru_cache(maxsize=None)
def gl_cases():
    """{name: (values, codes [33][70], the doubles they stand for)}
      few      200 values: a one-byte dictionary
      wide     1,000 values: 16-bit codes
      byte257  256 values in rows 0..31, every one of them used, and the 257th in row 32 (the third slab)
      near16   a table of 65,530 values, rows 0..31 from it, and 7 values outside it in row 32: 65,537"""
    rng = np.random.default_rng(3317)
    out = {}
    for name, n in (("few", 200), ("wide", 1000)):
        values = d16.table(n)
        codes = rng.integers(0, n, size=(NLOCI, NIND)).astype(np.uint16)
        out[name] = (values, codes, values[codes])
    values = d16.table(257)
    codes = rng.integers(0, 256, size=(NLOCI, NIND)).astype(np.uint16)
    codes.reshape(-1)[:256] = np.arange(256)                       # rows 0..3
    codes[32, 5::9] = 256
    assert np.unique(codes[:32]).shape[0] == 256 and codes[:32].max() == 255
    out["byte257"] = (values, codes, values[codes])
    values = d16.table(65530)
    extra = 0.123456789 + 1e-3 * np.arange(7)
    assert not np.isin(extra, values).any()
    codes = rng.integers(0, 65530, size=(NLOCI, NIND)).astype(np.uint16)
    gl = values[codes]
    gl[32, 3:3 + 7 * 9:9] = extra
    assert np.unique(np.concatenate([values, gl[32]])).shape[0] == 65537
    out["near16"] = (values, codes, gl)
    for v in out.values():
        for a in v:
            a.setflags(write=False)
    return out


def open_panel(ctx, c=None, genotypes=True):
    g, f, p, cs, ce = c or chrom()
    panel = abi.Panel(ctx, [NLOCI], NIND)
    panel.set_map(p, [cs], [ce], gpos=p * 1e-6)
    panel.set_freq(f)
    if genotypes:
        panel.set_genotypes(g)
    return panel


def check_lod(panel, gl_key=None, what=""):
    got = np.ascontiguousarray(panel.lod_windows(W, ERROR, MG, use_gl=gl_key is not None)[0])
    want = scores(gl_key)
    assert ol.bits_equal(got, want), (what, gl_key, ol.count_mismatch(got, want))


# ---------------------------------------------------------------------------------------------------- one case per door

def test_set_genotypes(gpu_ctx):
    with open_panel(gpu_ctx, genotypes=False) as panel:
        rows = wide(chrom()[0])
        panel.set_genotypes(rows)
        del rows
        check_lod(panel, what="set_genotypes")


def test_set_genotypes_2bit(gpu_ctx):
    lo = 3
    g = chrom()[0]
    everyone = np.full((NLOCI, lo + NIND + 2), -9, dtype=np.int16)      # the data set: 3 individuals in front, 2 behind
    everyone[:, :lo] = 1
    everyone[:, lo:lo + NIND] = g
    with open_panel(gpu_ctx, genotypes=False) as panel:
        rows = wide(pack2bit(everyone))
        panel.set_genotypes_2bit(rows, ind_offset=lo)
        del rows
        check_lod(panel, what="set_genotypes_2bit")


def test_set_gl(gpu_ctx):
    with open_panel(gpu_ctx) as panel:
        rows = wide(gl_cases()["few"][2])
        panel.set_gl(rows)
        del rows
        assert panel.tgls_mode()[0] == abi.TGLS_DICTIONARY
        check_lod(panel, "few", "set_gl")


def test_set_gl_codes(gpu_ctx):
    values, codes, _ = gl_cases()["few"]
    with open_panel(gpu_ctx) as panel:
        rows = wide(codes.astype(np.uint8))
        panel.set_gl_codes(rows, values)
        del rows
        assert panel.tgls_mode()[0] == abi.TGLS_DICTIONARY
        check_lod(panel, "few", "set_gl_codes")


def test_set_gl_codes16(gpu_ctx):
    values, codes, _ = gl_cases()["wide"]
    with open_panel(gpu_ctx) as panel:
        rows = wide(codes)
        panel.set_gl_codes16(rows, values)
        del rows
        assert panel.tgls_mode()[0] == abi.TGLS_DICTIONARY16
        check_lod(panel, "wide", "set_gl_codes16")


@functools.lru_cache(maxsize=None)
def phase_case():
    """(chroms, phase, the oracle's phased weights): ld_phased_cases' kind of panel at this file's shape"""
    rng = np.random.default_rng(3318)
    chroms = lw.wide_chroms(rng, [NLOCI], NIND)
    phase = rng.integers(0, 2, size=(NLOCI, NIND)).astype(np.uint8)
    want = lw.oracle_r2(chroms, phase, W)
    want.setflags(write=False)
    return chroms, phase, want


@pytest.mark.parametrize("bits", [False, True])
def test_set_phase(gpu_ctx, bits):
    """garlic_panel_set_phase (bytes) and garlic_panel_set_phase_bits"""
    chroms, phase, want = phase_case()
    with open_panel(gpu_ctx, chroms[0]) as panel:
        rows = wide(lp.pack_phase_rows(phase) if bits else phase)
        if bits:
            panel.set_phase_bits(rows)
        else:
            panel.set_phase(rows)
        del rows
        got = panel.compute_ld(W, phased=True)
        assert ol.bits_equal(got, want), (bits, ol.count_mismatch(got, want))


# ---------------------------------------------------------------------------- transitions that happen in the third slab

def test_one_byte_dictionary_overflows_in_the_last_slab(gpu_ctx):
    """slabs 1 and 2 are coded against a dictionary that reaches 256 values; the single row of slab 3 brings the 257th: what
    was coded is decoded, and slab 3 is stored as values"""
    with open_panel(gpu_ctx) as panel:
        rows = wide(gl_cases()["byte257"][2])
        panel.set_gl(rows)
        del rows
        assert panel.tgls_mode()[0] == abi.TGLS_CONTINUOUS
        check_lod(panel, "byte257", "one-byte overflow")


def test_16_bit_dictionary_overflows_in_the_last_slab(gpu_ctx):
    """a 16-bit panel with 65,530 values takes all 33 rows again as doubles: slabs 1 and 2 hold table values, the row of slab 3
    has 7 new ones, 65,537 in all: the panel turns continuous and the call goes on from slab 3 with values"""
    values, codes, gl = gl_cases()["near16"]
    with open_panel(gpu_ctx) as panel:
        panel.set_gl_codes16(codes, values)
        assert panel.tgls_mode()[0] == abi.TGLS_DICTIONARY16
        rows = wide(gl)
        panel.set_gl(rows)
        del rows
        assert panel.tgls_mode()[0] == abi.TGLS_CONTINUOUS
        check_lod(panel, "near16", "16-bit overflow")
