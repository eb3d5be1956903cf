"""GPU: garlic_bed_extract -- a column subset of a .bed image as a new image -- byte for byte against numpy
(pack_rows(codes[:, idx], garbage=False) through garlic_bed_get_rows), its census against the restatement on the subset's
columns, and panels filled from it against the int16 door and the oracle, bit for bit.  tests/bed_cases.py holds the cases
and the restatements."""
import ctypes as C

import numpy as np
import pytest

import bed_cases as cases
import oracle_lib as ol
from garlic_amd import abi

pytestmark = pytest.mark.gpu

ERROR, MAX_GAP = 0.001, 200000
N_IDX = [1, 3, 4, 5, 31, 32, 33, 64, 65, 257]


def _fast_census(codes):
    """cases.census vectorised (checked against it on a slice)"""
    nm = codes != cases.MISS
    first = np.argmax(nm, axis=1)
    anyone = nm.any(axis=1)
    c = np.where(anyone, (codes[np.arange(codes.shape[0]), first] == 3).astype(np.uint8), 2).astype(np.uint8)
    hom = np.where(c == 1, (codes == 3).sum(axis=1), (codes == 0).sum(axis=1))
    counts = np.stack([2 * hom + (codes == 2).sum(axis=1), 2 * nm.sum(axis=1)], axis=1).astype(np.int32)
    counts[~anyone] = 0
    a, b = cases.census(codes[:300])
    assert np.array_equal(a, counts[:300]) and np.array_equal(b, c[:300])
    return counts, c


def _check(sub, codes, idx, where, fast=False):
    """the two checks every case makes: the extract's bytes, and its census"""
    want = cases.pack_rows(codes[:, idx], garbage=False)
    got = sub.get_rows()
    assert got.shape == want.shape, where
    assert np.array_equal(got, want), (where, np.argwhere(got != want)[:8])
    counts, counted = sub.census()
    want_counts, want_counted = (_fast_census if fast else cases.census)(codes[:, idx])
    assert np.array_equal(counted, want_counted), (where, np.flatnonzero(counted != want_counted)[:8])
    assert np.array_equal(counts, want_counts), (where, np.flatnonzero((counts != want_counts).any(axis=1))[:8])


def _scattered(rng, n_idx, n):
    """ascending indices into n individuals that include 0 and n - 1 (n_idx 1: individual n - 1; n_idx >= n: everyone)"""
    if n_idx >= n:
        return np.arange(n)
    if n_idx == 1:
        return np.array([n - 1])
    inner = rng.choice(np.arange(1, n - 1), size=n_idx - 2, replace=False)
    return np.sort(np.concatenate([[0, n - 1], inner]))


@pytest.fixture(scope="module")
def file257():
    """257 individuals: 65-byte rows, so every start alignment of a source row occurs; garbage in the source's pad bits"""
    return cases.case_codes(257, np.random.default_rng(257))


@pytest.mark.parametrize("extra_pitch", [0, 3])
def test_bytes_and_census_of_every_subset_size(gpu_ctx, file257, extra_pitch):
    codes = file257
    rng = np.random.default_rng(5 + extra_pitch)
    rows = cases.pack_rows(codes, pitch=65 + extra_pitch, garbage=True)
    with abi.Bed(gpu_ctx, codes.shape[0], 257) as bed:
        bed.set_rows(rows)
        for n_idx in N_IDX:
            asc = _scattered(rng, n_idx, 257)
            repeats = asc.copy()
            repeats[rng.integers(0, n_idx, size=max(1, n_idx // 3))] = asc[rng.integers(0, n_idx)]      # any order, with repeats
            for name, idx in (("ascending", asc), ("reversed", asc[::-1].copy()), ("repeats", repeats)):
                with bed.extract(idx) as sub:
                    assert (sub.nrows, sub.nind_total, sub.row_bytes) == (codes.shape[0], n_idx, (n_idx + 3) // 4)
                    _check(sub, codes, idx, (n_idx, name, extra_pitch))


@pytest.mark.parametrize("n_idx", [8197, 8192])
def test_second_span_and_ragged_rows(gpu_ctx, n_idx):
    """9000 individuals, 27 rows: 8197 subset individuals are a span of 256 words and one of a single ragged word (2050-byte
    rows: odd and even rows start at other alignments); 8192 fill one span exactly"""
    rng = np.random.default_rng(n_idx)
    codes = cases.case_codes(9000, rng, random_rows=13)
    assert codes.shape[0] == 27
    idx = np.sort(rng.choice(9000, size=n_idx, replace=False))
    with abi.Bed(gpu_ctx, codes.shape[0], 9000) as bed:
        bed.set_rows(cases.pack_rows(codes))
        with bed.extract(idx) as sub:
            _check(sub, codes, idx, n_idx)


def test_global_form_and_lds_form_on_one_wide_image(gpu_ctx):
    """140,001 individuals (35,001-byte rows), 9 rows.  70 indices spread from 0 to 140,000: the span's source range is past
    the 32,753 bytes one row may take of the LDS budget -- the global form.  70 indices inside 100,000 .. 130,000 (7,501
    bytes): the LDS form on the same image.  And a range of exactly 32,753 bytes and one byte more: either side of the switch"""
    rng = np.random.default_rng(140001)
    n = 140001
    codes = rng.integers(0, 4, size=(9, n), dtype=np.uint8)
    codes[rng.random(codes.shape) < 0.2] = cases.MISS
    codes[4] = cases.MISS
    wide = np.sort(np.concatenate([[0, n - 1], rng.choice(np.arange(1, n - 1), size=68, replace=False)]))
    narrow = np.sort(rng.choice(np.arange(100000, 130000), size=70, replace=False))
    lo = 4 * 777 + 1
    at_limit = np.array([lo, lo + 5, lo + 4 * 32752 - 1, lo + 4 * 32752 + 2])      # bytes 777 .. 777 + 32752: 32,753 bytes
    past_limit = np.array([lo, lo + 5, lo + 4 * 32753 - 1, lo + 4 * 32753 + 2])    # one byte more
    with abi.Bed(gpu_ctx, 9, n) as bed:
        bed.set_rows(cases.pack_rows(codes))
        for name, idx in (("wide", wide), ("narrow", narrow), ("at_limit", at_limit), ("past_limit", past_limit)):
            with bed.extract(idx) as sub:
                _check(sub, codes, idx, name, fast=True)


def test_more_rows_than_one_trip_of_the_grid(gpu_ctx):
    """70,001 rows of 45 individuals, 20 kept: 16 rows a step, 4,376 steps for a grid capped at 8 workgroups per CU"""
    rng = np.random.default_rng(70001)
    codes = rng.integers(0, 4, size=(70001, 45), dtype=np.uint8)
    codes[rng.random(codes.shape) < 0.3] = cases.MISS
    codes[::97] = cases.MISS
    idx = np.sort(rng.choice(45, size=20, replace=False))
    with abi.Bed(gpu_ctx, codes.shape[0], 45) as bed:
        bed.set_rows(cases.pack_rows(codes))
        with bed.extract(idx) as sub:
            _check(sub, codes, idx, "rows", fast=True)


@pytest.mark.parametrize("which", ["scattered65", "behind70"])
def test_panels_filled_from_an_extract_score_like_the_int16_door_and_the_oracle(gpu_ctx, which):
    """the 257-individual score file; the subset's census recomputed in numpy; panels cut from the extract at ind_offset 0
    (64 individuals) and 1 (the rest) against panels filled with the recoded subset, against the oracle, and their ROH segments"""
    rng = np.random.default_rng(11)
    codes = cases.score_file(rng)
    nloci = sum(cases.SCORE_CHR)
    if which == "scattered65":
        idx = _scattered(np.random.default_rng(65), 65, 257)
    else:
        idx = np.sort(np.random.default_rng(130).choice(np.arange(70, 257), size=130, replace=False))      # the first 70 absent
    sub_codes = np.ascontiguousarray(codes[:, idx])
    _, counted = cases.census(sub_codes)
    m = cases.dest_maps(codes.shape[0], nloci)["scattered"][0]
    geno = np.ascontiguousarray(cases.recode(sub_codes, counted)[cases.final_map([m])])
    pos = np.cumsum(rng.integers(100, 3000, size=nloci)).astype(np.int32)
    freq = rng.uniform(0.05, 0.95, size=nloci)
    off = np.concatenate([[0], np.cumsum(cases.SCORE_CHR)])
    oracle = [ol.oracle_calc_lod(np.ascontiguousarray(geno[off[c]:off[c + 1]]), freq[off[c]:off[c + 1]], pos[off[c]:off[c + 1]], 0, 0,
                                 cases.SCORE_W, ERROR, MAX_GAP) for c in range(3)]

    def panel(nind):
        p = abi.Panel(gpu_ctx, cases.SCORE_CHR, nind)
        p.set_map(pos, [0, 0, 0], [0, 0, 0])
        p.set_freq(freq)
        return p

    with abi.Bed(gpu_ctx, codes.shape[0], 257) as bed:
        bed.set_rows(cases.pack_rows(codes))
        sub = bed.extract(idx)
    with sub:      # (the source is gone)
        for ind_offset, nind in ((0, 64), (1, len(idx) - 1)):
            with panel(nind) as mine, panel(nind) as ref:
                mine.set_genotypes_bed(sub, m, ind_offset)
                ref.set_genotypes(np.ascontiguousarray(geno[:, ind_offset:ind_offset + nind]))
                got, exp = mine.lod_windows(cases.SCORE_W, ERROR, MAX_GAP), ref.lod_windows(cases.SCORE_W, ERROR, MAX_GAP)
                for c in range(3):
                    assert ol.bits_equal(got[c], exp[c]), (which, ind_offset, c)
                    assert ol.bits_equal(got[c], oracle[c][ind_offset:ind_offset + nind]), (which, ind_offset, c)
                seg = mine.roh_segments(cases.SCORE_W, ERROR, MAX_GAP, -1.0, 0.25)
                assert len(seg) > 0 and np.array_equal(seg, ref.roh_segments(cases.SCORE_W, ERROR, MAX_GAP, -1.0, 0.25))


def test_independence_composition_and_refusals(gpu_ctx, file257):
    codes = file257
    nrows = codes.shape[0]
    rng = np.random.default_rng(3)
    rows = cases.pack_rows(codes)
    first = rng.permutation(257)[:100]
    second = rng.integers(0, 100, size=37)
    bed = abi.Bed(gpu_ctx, nrows, 257)
    bed.set_rows(rows)
    sub = bed.extract(first)
    bed.destroy()                                   # the extract does not need its source
    with sub:
        _check(sub, codes, first, "after destroy")
        with sub.extract(second) as subsub:         # an extract of an extract = the extract by composed indices
            _check(subsub, codes, first[second], "composed")
        # get_rows: a part of the rows; past the image refused
        assert np.array_equal(sub.get_rows(3, 5), cases.pack_rows(codes[:, first], garbage=False)[3:8])
        for begin, count in ((0, nrows + 1), (nrows, 1), (-1, 2), (0, 0)):
            with pytest.raises(abi.GarlicError) as e:
                sub.get_rows(begin, count)
            assert e.value.code == abi.ERR_INVALID, (begin, count)
        # pitched destination: the bytes past a row's own stay
        out = np.full((nrows, sub.row_bytes + 3), 0xEE, dtype=np.uint8)
        abi.check(abi.lib().garlic_bed_get_rows(sub.handle, 0, nrows, C.c_void_p(out.ctypes.data), out.shape[1], abi.HOST))
        assert np.array_equal(out[:, :sub.row_bytes], cases.pack_rows(codes[:, first], garbage=False)) and (out[:, sub.row_bytes:] == 0xEE).all()
        with pytest.raises(abi.GarlicError) as e:
            sub.extract([100])                      # nind_total of this image
        assert e.value.code == abi.ERR_INVALID and "100" in str(e.value)
    with abi.Bed(gpu_ctx, nrows, 257) as partial:
        partial.set_rows(rows[:nrows - 1], 0)
        with pytest.raises(abi.GarlicError) as e:
            partial.extract([0, 1])                 # an incomplete source
        assert e.value.code == abi.ERR_STATE
        with pytest.raises(abi.GarlicError) as e:
            partial.extract([257])                  # index nind_total (checked before the state? either way refused)
        assert e.value.code in (abi.ERR_INVALID, abi.ERR_STATE)
        partial.set_rows(rows[nrows - 1:], nrows - 1)
        for bad in (-1, 257):
            with pytest.raises(abi.GarlicError) as e:
                partial.extract([0, bad])
            assert e.value.code == abi.ERR_INVALID, bad
        with pytest.raises(abi.GarlicError) as e:
            partial.extract(np.zeros(0, dtype=np.int32))      # n_idx = 0
        assert e.value.code == abi.ERR_INVALID
