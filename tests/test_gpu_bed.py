"""GPU: the PLINK .bed door of the C ABI -- garlic_bed_census against the numpy restatement element for element, and panels
filled by garlic_panel_set_genotypes_bed against panels filled with the recoded int16 matrix and against the oracle, bit for
bit (tests/bed_cases.py holds the cases and the restatements)."""
import numpy as np
import pytest

import bed_cases as cases
import oracle_lib as ol
from garlic_amd import abi

pytestmark = pytest.mark.gpu

ERROR, MAX_GAP = 0.001, 200000


def _upload(bed, rows, chunk, device):
    nrows = rows.shape[0]
    if device:
        import torch
        t = torch.from_numpy(rows).cuda()
        for r in range(0, nrows, chunk):
            n = min(chunk, nrows - r)
            bed.set_rows_device(t.data_ptr() + r * rows.shape[1], rows.shape[1], r, n)
        torch.cuda.synchronize()
    else:
        for r in range(0, nrows, chunk):
            bed.set_rows(rows[r:r + chunk], r)


@pytest.mark.parametrize("n", cases.CENSUS_N)
def test_census_equals_the_restatement(gpu_ctx, n):
    """every N of the list (a tail inside a byte, a word, a wave and a loop trip; rows shorter than one read), rows of all
    missing, first non-missing genotype hom A1 / het / hom A2 at the first and the last individual and in the last lane's tail,
    garbage in the pad bits; row pitch minimum and minimum + 3; host and device sources; chunks of 1, 7 and all rows"""
    rng = np.random.default_rng(100 + n)
    codes = cases.case_codes(n, rng)
    nrows = codes.shape[0]
    want_counts, want_counted = cases.census(codes)
    rb = (n + 3) // 4
    for pitch in (rb, rb + 3):
        rows = cases.pack_rows(codes, pitch=pitch, garbage=True)
        for device in (False, True):
            for chunk in (1, 7, nrows):
                with abi.Bed(gpu_ctx, nrows, n) as bed:
                    _upload(bed, rows, chunk, device)
                    counts, counted = bed.census()
                    where = (n, pitch, device, chunk)
                    assert np.array_equal(counted, want_counted), (where, np.flatnonzero(counted != want_counted)[:8])
                    assert np.array_equal(counts, want_counts), (where, np.flatnonzero((counts != want_counts).any(axis=1))[:8])
                    counts2, counted2 = bed.census()            # the cached answer
                    assert np.array_equal(counts2, want_counts) and np.array_equal(counted2, want_counted)


@pytest.mark.parametrize("n,nrows", [(45, 300001), (2000, 9001)])
def test_census_over_more_rows_than_one_trip_of_the_grid(gpu_ctx, n, nrows):
    """the grid of bed_census_kernel is capped at 8 workgroups per CU (2048 on a 256-CU device) and strides over the rest.
    45 individuals: 12-byte rows, 2 lanes each, 128 rows per workgroup, one trip = 262,144 rows; 2000 individuals: 500-byte
    rows, a wave each, 4 rows per workgroup, one trip = 8192 rows.  Both cases go round more than once"""
    rng = np.random.default_rng(n)
    codes = rng.integers(0, 4, size=(nrows, n), dtype=np.uint8)
    codes[rng.random(codes.shape) < 0.3] = cases.MISS
    codes[::97] = cases.MISS
    want_counts, want_counted = _fast_census(codes)
    with abi.Bed(gpu_ctx, nrows, n) as bed:
        bed.set_rows(cases.pack_rows(codes))
        counts, counted = bed.census()
    assert np.array_equal(counted, want_counted) and np.array_equal(counts, want_counts)


def test_census_into_device_memory(gpu_ctx):
    """garlic_bed_census with where = GARLIC_DEVICE; any other `where` is refused"""
    import ctypes as C
    import torch
    codes = cases.case_codes(130, np.random.default_rng(5))
    want_counts, want_counted = cases.census(codes)
    d_counts = torch.full((codes.shape[0], 2), -1, dtype=torch.int32, device="cuda")
    d_counted = torch.full((codes.shape[0],), 9, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    with abi.Bed(gpu_ctx, codes.shape[0], 130) as bed:
        bed.set_rows(cases.pack_rows(codes))
        bed.census_device(d_counts.data_ptr(), d_counted.data_ptr())
        assert np.array_equal(d_counts.cpu().numpy(), want_counts) and np.array_equal(d_counted.cpu().numpy(), want_counted)
        assert abi.lib().garlic_bed_census(bed.handle, C.c_void_p(d_counts.data_ptr()), None, 7) == abi.ERR_INVALID
        rows = cases.pack_rows(codes)
        assert abi.lib().garlic_bed_set_rows(bed.handle, C.c_void_p(rows.ctypes.data), rows.shape[1], 0, 1, 7) == abi.ERR_INVALID


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


@pytest.fixture(scope="module")
def score_setup(gpu_ctx):
    """the file, its image on the device, map / freq of the 3-chromosome panel, and the oracle's scores of all 257 individuals
    per final row map (computed once)"""
    rng = np.random.default_rng(11)
    codes = cases.score_file(rng)
    nloci = sum(cases.SCORE_CHR)
    _, counted = cases.census(codes)
    data = cases.recode(codes, counted)
    pos = np.cumsum(rng.integers(100, 3000, size=nloci)).astype(np.int32)
    freq = rng.uniform(0.05, 0.95, size=nloci)
    maps = cases.dest_maps(codes.shape[0], nloci)
    off = np.concatenate([[0], np.cumsum(cases.SCORE_CHR)])
    def scores(geno):
        geno = np.ascontiguousarray(geno)
        return geno, [ol.oracle_calc_lod(np.ascontiguousarray(geno[off[c]:off[c + 1]]), freq[off[c]:off[c + 1]],
                                         pos[off[c]:off[c + 1]], 0, 0, cases.SCORE_W, ERROR, MAX_GAP) for c in range(3)]

    want = {name: scores(data[cases.final_map(maps[name])]) for name in ("scattered", "prefix")}
    want["two_calls"] = want["scattered"]
    bed = abi.Bed(gpu_ctx, codes.shape[0], cases.SCORE_NIND_FILE)
    bed.set_rows(cases.pack_rows(codes))
    # the variant that keeps all: a second file of exactly nloci rows, every row of the image mapped, its last included
    codes_all = cases.keep_all_file(rng)
    assert codes_all.shape[0] == nloci
    bed_all = abi.Bed(gpu_ctx, nloci, cases.SCORE_NIND_FILE)
    bed_all.set_rows(cases.pack_rows(codes_all))
    want["all"] = scores(cases.recode(codes_all, cases.census(codes_all)[1]))
    variants = {name: (bed, calls) for name, calls in maps.items()}
    variants["all"] = (bed_all, [np.arange(nloci, dtype=np.int64)])
    yield dict(codes=codes, data=data, pos=pos, freq=freq, maps=maps, want=want, bed=bed, variants=variants)
    bed.destroy()
    bed_all.destroy()


def _panel(ctx, s, nind):
    p = abi.Panel(ctx, cases.SCORE_CHR, nind)
    p.set_map(s["pos"], [0, 0, 0], [0, 0, 0])
    p.set_freq(s["freq"])
    return p


@pytest.mark.parametrize("ind_offset", cases.SCORE_OFFSETS)
def test_bed_panel_scores_like_the_int16_panel_and_the_oracle(gpu_ctx, score_setup, ind_offset):
    """dest_locus variants: scattered drops (first row, last row, 20 consecutive rows), all rows of a file kept, a prefix of
    the longer file, and two calls that each write half of every word"""
    s = score_setup
    assert set(s["variants"]) == {"scattered", "all", "prefix", "two_calls"}
    for nind in cases.SCORE_NINDS:
        if ind_offset + nind > cases.SCORE_NIND_FILE:
            continue
        for name, (bed, calls) in s["variants"].items():
            geno, oracle = s["want"][name]
            with _panel(gpu_ctx, s, nind) as mine, _panel(gpu_ctx, s, nind) as ref:
                for m in calls:
                    mine.set_genotypes_bed(bed, m, ind_offset)
                ref.set_genotypes(np.ascontiguousarray(geno[:, ind_offset:ind_offset + nind]))
                got = mine.lod_windows(cases.SCORE_W, ERROR, MAX_GAP)
                exp = ref.lod_windows(cases.SCORE_W, ERROR, MAX_GAP)
                for c in range(3):
                    where = (ind_offset, nind, name, c)
                    assert ol.bits_equal(got[c], exp[c]), where
                    assert ol.bits_equal(got[c], oracle[c][ind_offset:ind_offset + nind]), where


def test_unmapped_loci_keep_their_bits(gpu_ctx, score_setup):
    """a panel filled through the int16 door, then half of its loci overwritten from OTHER file rows through the bed door:
    the other half still scores as before"""
    s = score_setup
    nloci = sum(cases.SCORE_CHR)
    geno, _ = s["want"]["prefix"]
    m = np.full(s["codes"].shape[0], -1, dtype=np.int64)
    src = np.arange(30, 30 + nloci // 2)                       # file rows 30 .. go to the even loci
    m[src] = 2 * np.arange(nloci // 2)
    expect = geno[:, 5:70].copy()
    expect[2 * np.arange(nloci // 2)] = s["data"][src, 5:70]
    with _panel(gpu_ctx, s, 65) as mine, _panel(gpu_ctx, s, 65) as ref:
        mine.set_genotypes(np.ascontiguousarray(geno[:, 5:70]))
        mine.set_genotypes_bed(s["bed"], m, 5)
        ref.set_genotypes(np.ascontiguousarray(expect))
        got, exp = mine.lod_windows(cases.SCORE_W, ERROR, MAX_GAP), ref.lod_windows(cases.SCORE_W, ERROR, MAX_GAP)
        assert all(ol.bits_equal(got[c], exp[c]) for c in range(3))


def test_refusals(gpu_ctx, score_setup):
    s = score_setup
    nrows = s["codes"].shape[0]
    good = s["maps"]["prefix"][0]
    with _panel(gpu_ctx, s, 64) as p:
        bad = good.copy()
        bad[[4, 5]] = bad[[5, 4]]                               # not ascending
        with pytest.raises(abi.GarlicError) as e:
            p.set_genotypes_bed(s["bed"], bad, 0)
        assert e.value.code == abi.ERR_INVALID
        same = good.copy()
        same[5] = same[4]                                       # ascending, but not strictly
        with pytest.raises(abi.GarlicError) as e:
            p.set_genotypes_bed(s["bed"], same, 0)
        assert e.value.code == abi.ERR_INVALID
        with pytest.raises(abi.GarlicError) as e:
            p.set_genotypes_bed(s["bed"], good, cases.SCORE_NIND_FILE - 63)      # ind_offset + nind > nind_total
        assert e.value.code == abi.ERR_INVALID
        p.set_genotypes_bed(s["bed"], good, cases.SCORE_NIND_FILE - 64)
    rows = cases.pack_rows(s["codes"])
    with abi.Bed(gpu_ctx, nrows, cases.SCORE_NIND_FILE) as bed:
        bed.set_rows(rows[:nrows - 1], 0)
        with pytest.raises(abi.GarlicError) as e:
            bed.census()                                        # a row is still missing
        assert e.value.code == abi.ERR_STATE
        with pytest.raises(abi.GarlicError) as e:
            bed.set_rows(rows[:2], nrows - 1)                   # past the image
        assert e.value.code == abi.ERR_INVALID
        with pytest.raises(abi.GarlicError) as e:
            bed.set_rows(np.ascontiguousarray(rows[:, :rows.shape[1] - 1]), 0)        # row_bytes too small
        assert e.value.code == abi.ERR_INVALID
        bed.set_rows(rows[nrows - 1:], nrows - 1)
        counts, counted = bed.census()
        want_counts, want_counted = cases.census(s["codes"])
        assert np.array_equal(counts, want_counts) and np.array_equal(counted, want_counted)


def test_two_shards_reproduce_the_single_panel(gpu_ctx, score_setup):
    """the 257 individuals as one panel and as two shards (ind_offset 0 and 129), each shard in a context of its own with its
    own image: same score rows, same ROH segments"""
    s = score_setup
    m = s["maps"]["scattered"][0]
    rows = cases.pack_rows(s["codes"])
    cutoff, overlap = -1.0, 0.25
    with _panel(gpu_ctx, s, 257) as whole:
        whole.set_genotypes_bed(s["bed"], m, 0)
        want = whole.lod_windows(cases.SCORE_W, ERROR, MAX_GAP)
        want_seg = whole.roh_segments(cases.SCORE_W, ERROR, MAX_GAP, cutoff, overlap)
    assert len(want_seg) > 0
    got_rows, got_seg = [[] for _ in range(3)], []
    for ind_offset, nind in ((0, 129), (129, 128)):
        with abi.Context(0) as ctx, abi.Bed(ctx, rows.shape[0], 257) as bed, _panel(ctx, s, nind) as shard:
            bed.set_rows(rows)
            shard.set_genotypes_bed(bed, m, ind_offset)
            out = shard.lod_windows(cases.SCORE_W, ERROR, MAX_GAP)
            seg = shard.roh_segments(cases.SCORE_W, ERROR, MAX_GAP, cutoff, overlap)
            seg[:, 0] += ind_offset
            got_seg.append(seg)
            for c in range(3):
                got_rows[c].append(np.array(out[c]))
    for c in range(3):
        assert ol.bits_equal(np.concatenate(got_rows[c], axis=0), want[c]), c
    assert np.array_equal(np.concatenate(got_seg, axis=0), want_seg)
