"""GPU: garlic_feature_set_rows_bed -- the hom rows of a feature set built on the device from a .bed image -- bit for bit
against the numpy restatement of tests/feature_bed_cases.py, read back through garlic_feature_set_get_rows: every row
alignment and block tail, zero and all-one pad bits, file_row in any order and with repeats, selector 2, a sub-range of a set
filled through set_rows, an extract as the source, the counts of such a set, and the refusals."""
import ctypes as C

import numpy as np
import pytest

import feature_bed_cases as fb
import feature_cases as fc
from garlic_amd import abi, synth

pytestmark = pytest.mark.gpu


def _bed(ctx, codes, pad_bits=0):
    bed = abi.Bed(ctx, codes.shape[0], codes.shape[1])
    bed.set_rows(synth.bed_rows(codes, pad_bits=pad_bits))
    return bed


def _same(got, hom, where):
    want = fc.pack(hom)
    assert got.shape == want.shape, (where, got.shape, want.shape)
    assert np.array_equal(got, want), (where, np.argwhere(got != want)[:8])


@pytest.mark.parametrize("pad_bits", fb.PADS)
@pytest.mark.parametrize("nind", fb.NINDS)
def test_hom_rows_of_every_shape(gpu_ctx, nind, pad_bits):
    rng = np.random.default_rng(1000 * nind + pad_bits)
    codes = fb.image_codes(nind, rng)
    with _bed(gpu_ctx, codes, pad_bits) as bed:
        for n_out in fb.ROW_COUNTS:
            for name, (file_row, allele) in fb.plans(n_out, codes.shape[0], rng).items():
                if n_out > 1:
                    assert 0 in file_row and codes.shape[0] - 1 in file_row
                with abi.FeatureSet(gpu_ctx, n_out, nind) as fs:
                    fs.set_rows_bed(bed, file_row, allele)
                    got = fs.get_rows()
                hom = fb.hom_rows(codes, file_row, allele)
                assert not hom[allele == 2].any()
                _same(got, hom, (nind, pad_bits, n_out, name))
                # the bits past the last individual are 0 whatever the pad bits hold (pack leaves them 0: stated once more)
                if n_out and nind % 8:
                    assert not (got[:, -1] >> (nind % 8)).any(), (nind, pad_bits, n_out, name)


def test_selector_two_rows_are_zero_and_get_rows_leaves_the_pitch_alone(gpu_ctx):
    rng = np.random.default_rng(2)
    codes = fb.image_codes(130, rng)
    file_row = np.array([0, 0, 0, 69, 69, 69, 5], dtype=np.int64)
    allele = np.array([0, 1, 2, 0, 1, 2, 2], dtype=np.uint8)
    with _bed(gpu_ctx, codes) as bed, abi.FeatureSet(gpu_ctx, 7, 130) as fs:
        fs.set_rows(np.full((7, 17), 0xFF, dtype=np.uint8))          # the call overwrites, it does not OR
        fs.set_rows_bed(bed, file_row, allele)
        got = fs.get_rows()
        assert not got[[2, 5, 6]].any()
        assert got[0, :16].min() == 0xFF and got[0, 16] == 0x03 and not got[1].any()        # image row 0 is all hom A1
        assert got[4, :16].min() == 0xFF and got[4, 16] == 0x03 and not got[3].any()        # the last image row all hom A2
        _same(got, fb.hom_rows(codes, file_row, allele), "selectors")
        # a wider pitch: the bytes past a row's own are untouched
        wide = np.full((3, 20), 0x5A, dtype=np.uint8)
        abi.check(abi.lib().garlic_feature_set_get_rows(fs.handle, 3, 3, C.c_void_p(wide.ctypes.data), 20))
        assert np.array_equal(wide[:, :17], got[3:6]) and (wide[:, 17:] == 0x5A).all()


def test_sub_range_of_a_set_filled_through_set_rows(gpu_ctx):
    rng = np.random.default_rng(3)
    nind, nrows = 257, 200
    codes = fb.image_codes(nind, rng)
    before = rng.random((nrows, nind)) < 0.3
    file_row = rng.integers(0, codes.shape[0], size=77).astype(np.int64)
    allele = rng.integers(0, 3, size=77).astype(np.uint8)
    with _bed(gpu_ctx, codes, 0xFF) as bed, abi.FeatureSet(gpu_ctx, nrows, nind, rows=fc.pack(before)) as fs:
        fs.set_rows_bed(bed, file_row, allele, row_begin=61)
        want = before.copy()
        want[61:61 + 77] = fb.hom_rows(codes, file_row, allele)
        _same(fs.get_rows(), want, "sub-range")
        _same(fs.get_rows(60, 3), want[60:63], "get_rows of a range")
        fs.set_rows(fc.pack(before[100:110]), row_begin=100)         # and back through the other door: the two mix
        want[100:110] = before[100:110]
        _same(fs.get_rows(), want, "mixed doors")


def test_an_extract_as_the_source(gpu_ctx):
    rng = np.random.default_rng(4)
    codes = fb.image_codes(257, rng)
    idx = np.sort(rng.choice(257, size=131, replace=False)).astype(np.int32)
    idx[0], idx[-1] = 0, 256
    file_row, allele = fb.plans(65, codes.shape[0], rng)["repeats"]
    with _bed(gpu_ctx, codes, 0xFF) as bed, bed.extract(idx) as sub, abi.FeatureSet(gpu_ctx, 65, 131) as fs:
        fs.set_rows_bed(sub, file_row, allele)
        _same(fs.get_rows(), fb.hom_rows(codes[:, idx], file_row, allele), "extract")


def test_counts_of_a_set_filled_from_the_image(gpu_ctx):
    nind, nrows, n_classes, n_effects = 130, 300, 3, 5
    _hom, chr_, pos, effect, iv = fc.random_case(11, nind, nrows, n_classes, n_effects)
    rng = np.random.default_rng(5)
    codes = fb.image_codes(nind, rng, nrows=90)
    file_row = rng.integers(0, 90, size=nrows).astype(np.int64)
    allele = rng.integers(0, 3, size=nrows).astype(np.uint8)
    hom = fb.hom_rows(codes, file_row, allele)
    with _bed(gpu_ctx, codes, 0xFF) as bed, abi.FeatureSet(gpu_ctx, nrows, nind, chr=chr_, pos=pos, effect=effect) as fs:
        fs.set_rows_bed(bed, file_row, allele)
        from_image = fs.counts(iv, n_classes, n_effects)
    with abi.FeatureSet(gpu_ctx, nrows, nind, rows=fc.pack(hom), chr=chr_, pos=pos, effect=effect) as fs:
        from_rows = fs.counts(iv, n_classes, n_effects)
    assert np.array_equal(from_image, from_rows)
    assert np.array_equal(from_image, fc.expected_counts(hom, chr_, pos, effect, iv, nind, n_classes, n_effects))
    assert from_image.sum() == hom.sum() > 0


def _rows_bed(fs, bed, file_row, allele, row_begin, row_count):
    p = lambda a: C.c_void_p(a.ctypes.data) if a is not None else None
    return abi.lib().garlic_feature_set_rows_bed(fs, bed, p(file_row), p(allele), row_begin, row_count)


def test_refusals_leave_the_set_as_it_was(gpu_ctx):
    rng = np.random.default_rng(6)
    codes = fb.image_codes(65, rng)
    before = rng.random((10, 65)) < 0.5
    file_row = np.arange(4, dtype=np.int64)
    allele = np.array([0, 1, 2, 0], dtype=np.uint8)
    error = lambda: abi.lib().garlic_hip_last_error().decode()
    with _bed(gpu_ctx, codes) as bed, abi.FeatureSet(gpu_ctx, 10, 65, rows=fc.pack(before)) as fs:
        assert _rows_bed(None, bed.handle, file_row, allele, 0, 4) == abi.ERR_INVALID
        assert _rows_bed(fs.handle, None, file_row, allele, 0, 4) == abi.ERR_INVALID
        assert _rows_bed(fs.handle, bed.handle, None, allele, 0, 4) == abi.ERR_INVALID
        assert _rows_bed(fs.handle, bed.handle, file_row, None, 0, 4) == abi.ERR_INVALID
        for begin, count in ((-1, 4), (7, 4), (0, -1)):
            assert _rows_bed(fs.handle, bed.handle, file_row, allele, begin, count) == abi.ERR_INVALID, (begin, count)
        bad = np.array([0, 69, 70, -1], dtype=np.int64)
        assert _rows_bed(fs.handle, bed.handle, bad, allele, 0, 4) == abi.ERR_INVALID
        assert "file_row[2] = 70" in error()
        assert _rows_bed(fs.handle, bed.handle, np.array([0, -3, 70, 1], dtype=np.int64), allele, 0, 4) == abi.ERR_INVALID
        assert "file_row[1] = -3" in error()
        assert _rows_bed(fs.handle, bed.handle, file_row, np.array([0, 2, 3, 9], dtype=np.uint8), 0, 4) == abi.ERR_INVALID
        assert "allele[2] = 3" in error()
        with abi.Bed(gpu_ctx, 70, 64) as other:                      # another individual count
            other.set_rows(synth.bed_rows(codes[:, :64]))
            assert _rows_bed(fs.handle, other.handle, file_row, allele, 0, 4) == abi.ERR_INVALID
        with abi.Bed(gpu_ctx, 70, 65) as partial:                    # not fully set
            partial.set_rows(synth.bed_rows(codes[:69]))
            assert _rows_bed(fs.handle, partial.handle, file_row, allele, 0, 4) == abi.ERR_STATE
        import torch
        if torch.cuda.device_count() > 1:                            # an image on another device
            with abi.Context(1) as ctx1, _bed(ctx1, codes) as far:
                assert _rows_bed(fs.handle, far.handle, file_row, allele, 0, 4) == abi.ERR_INVALID
                assert "device" in error()
        with pytest.raises(abi.GarlicError):
            fs.get_rows(8, 3)
        _same(fs.get_rows(), before, "after the refusals")
        assert _rows_bed(fs.handle, bed.handle, file_row, allele, 6, 4) == abi.OK        # the last rows of the set
        want = before.copy()
        want[6:] = fb.hom_rows(codes, file_row, allele)
        _same(fs.get_rows(), want, "the accepted call")
