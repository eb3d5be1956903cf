"""GPU: garlic_feature_counts (csrc/feature_kernels.hpp) against the numpy restatement of tests/feature_cases.py: exact
equality of every count at every shape -- block tails, chunk edges (one wavefront takes FEAT_CHUNK_ROWS rows), an interval
across a chunk edge, individuals with no, one and many intervals over several chromosomes, empty and adjacent intervals,
two rows at one position, every class count, the effect counts on both sides of a launch's 32 and at the cap, zero-word
skipping, repeated calls, a caller-owned stream with device output, and what the call refuses."""
import functools

import numpy as np
import pytest

import feature_cases as fc
from garlic_amd import abi

pytestmark = pytest.mark.gpu
R = abi.FEATURE_CHUNK_ROWS
NINDS = [1, 63, 64, 65, 130]
NROWS = [0, 1, R - 1, R, R + 1, 2 * R + 3]


@functools.lru_cache(maxsize=None)
def case(nind, nrows, n_classes, n_effects, seed=0):
    """the random case and its expected counts, computed once"""
    straddle = R if nrows > R else None          # individual 1's interval lies across the first chunk edge
    hom, chr_, pos, effect, iv = fc.random_case(100 + seed, nind, nrows, n_classes, n_effects, straddle=straddle)
    want = fc.expected_counts(hom, chr_, pos, effect, iv, nind, n_classes, n_effects)
    for a in (hom, chr_, pos, effect, iv, want):
        a.setflags(write=False)
    if straddle is not None and nind > 1:
        one = iv[iv["ind"] == 1]
        assert one.shape[0] == 1 and one["start"][0] <= pos[R - 1] and pos[R] < one["stop"][0] and one["chr"][0] == chr_[R - 1] == chr_[R]
    return hom, chr_, pos, effect, iv, want


def open_set(ctx, hom, chr_, pos, effect):
    return abi.FeatureSet(ctx, hom.shape[0], hom.shape[1], rows=fc.pack(hom), chr=chr_, pos=pos, effect=effect)


def zero_words(hom):
    nrows, nind = hom.shape
    pad = np.zeros((nrows, -nind % 64), dtype=bool)
    return int((~np.concatenate([hom, pad], axis=1).reshape(nrows, (nind + 63) // 64, 64).any(axis=2)).sum())


@pytest.mark.parametrize("nrows", NROWS)
@pytest.mark.parametrize("nind", NINDS)
def test_counts_at_block_tails_and_chunk_edges(gpu_ctx, nind, nrows):
    hom, chr_, pos, effect, iv, want = case(nind, nrows, 3, 3)
    if nind >= 63 and nrows >= R - 1:      # the case holds what it is meant to hold
        per = np.bincount(iv["ind"], minlength=nind)
        assert per[0] == 0 and per[1] == 1 and per.max() > 10
        assert ((iv["start"] == iv["stop"])).any(), "an empty interval"
        same = (iv["ind"][1:] == iv["ind"][:-1]) & (iv["chr"][1:] == iv["chr"][:-1])
        assert (same & (iv["start"][1:] == iv["stop"][:-1]) & (iv["cls"][1:] != iv["cls"][:-1])).any(), "adjacent, different classes"
        assert ((pos[1:] == pos[:-1]) & (chr_[1:] == chr_[:-1]) & (effect[1:] != effect[:-1])).any(), "two rows at one position"
        assert len(set(chr_) - set(iv["chr"])) == 1 and len(set(iv["chr"]) - set(chr_)) == 1
        assert want[:, :3].sum() > 0 and want[:, 3].sum() > 0
    with open_set(gpu_ctx, hom, chr_, pos, effect) as fs:
        got = fs.counts(iv, 3, 3)
        info = fs.info()
    assert got.dtype == np.int64 and got.shape == want.shape
    assert np.array_equal(got, want), (nind, nrows, int((got != want).sum()), "counts differ")
    assert info["blocks"] == (nind + 63) // 64 and info["chunks"] == (nrows + R - 1) // R
    assert info["words_skipped"] == zero_words(hom)


@pytest.mark.parametrize("n_effects", [1, abi.FEATURE_GROUP_EFFECTS, abi.FEATURE_GROUP_EFFECTS + 1, abi.FEATURE_MAX_EFFECTS])
@pytest.mark.parametrize("n_classes", [1, 3, 8])
def test_every_class_count_and_effects_across_launches(gpu_ctx, n_classes, n_effects):
    hom, chr_, pos, effect, iv, want = case(65, R + 1, n_classes, n_effects, seed=1)
    assert effect.max() == n_effects - 1 and (n_classes == 1 or len(set(iv["cls"])) == n_classes)
    with open_set(gpu_ctx, hom, chr_, pos, effect) as fs:
        got = fs.counts(iv, n_classes, n_effects)
        assert fs.info()["words_skipped"] == zero_words(hom), "zero words are counted once, not once per launch"
    assert np.array_equal(got, want), (n_classes, n_effects, int((got != want).sum()))
    assert got.sum() == hom.sum()


def test_all_ones_and_all_zero_rows(gpu_ctx):
    nind, nrows = 130, R + 70
    rng = np.random.default_rng(5)
    hom = np.zeros((nrows, nind), dtype=bool)
    hom[rng.choice(nrows, 200, replace=False)] = True
    _, chr_, pos, effect, iv, _ = case(nind, nrows, 3, 3, seed=2)
    want = fc.expected_counts(hom, chr_, pos, effect, iv, nind, 3, 3)
    with open_set(gpu_ctx, hom, chr_, pos, effect) as fs:
        got = fs.counts(iv, 3, 3)
        assert fs.info()["words_skipped"] == 3 * (nrows - 200)
    assert np.array_equal(got, want) and got.sum() == 200 * nind     # no padding bit of the last block counts
    # rows that were never uploaded hold no homozygote
    with abi.FeatureSet(gpu_ctx, nrows, nind, chr=chr_, pos=pos, effect=effect) as fs:
        assert fs.counts(iv, 3, 3).sum() == 0
        assert fs.info()["words_skipped"] == 3 * nrows


def test_second_call_with_other_intervals_and_ten_repeats(gpu_ctx):
    hom, chr_, pos, effect, iv, want = case(130, 2 * R + 3, 3, 3)
    _, _, _, _, iv2, _ = case(130, 2 * R + 3, 3, 3, seed=3)
    want2 = fc.expected_counts(hom, chr_, pos, effect, iv2, 130, 3, 3)
    assert not np.array_equal(want, want2)
    with open_set(gpu_ctx, hom, chr_, pos, effect) as fs:
        first = fs.counts(iv, 3, 3)
        assert np.array_equal(fs.counts(iv2, 3, 3), want2), "counts are overwritten, not accumulated"
        assert np.array_equal(fs.counts(iv[:0], 3, 3)[:, 3], want.sum(axis=1)), "no interval: everything is NONE"
        for _ in range(10):
            assert fs.counts(iv, 3, 3).tobytes() == first.tobytes()
    assert np.array_equal(first, want)


def test_caller_stream_and_device_output():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    hom, chr_, pos, effect, iv, want = case(130, 2 * R + 3, 3, 3)
    _, _, _, _, iv2, _ = case(130, 2 * R + 3, 3, 3, seed=3)
    want2 = fc.expected_counts(hom, chr_, pos, effect, iv2, 130, 3, 3)
    s = torch.cuda.Stream()
    assert s.cuda_stream != 0
    ctx = abi.Context(0, stream=s.cuda_stream)
    try:
        with open_set(ctx, hom, chr_, pos, effect) as fs:
            out = torch.full((130, 4, 3), -7, dtype=torch.int64, device="cuda")
            torch.cuda.synchronize()                         # the sentinel is in place
            fs.counts_device(iv, 3, 3, out)
            with torch.cuda.stream(s):
                snap = out.clone()                           # consumed on the caller's stream, no wait in between
            fs.counts_device(iv2, 3, 3, out)                 # the next call's intervals do not disturb the one in flight
            with torch.cuda.stream(s):
                snap2 = out.clone()
            s.synchronize()
            assert np.array_equal(snap.cpu().numpy(), want)
            assert np.array_equal(snap2.cpu().numpy(), want2)
    finally:
        s.synchronize()
        ctx.close()


def test_refusals(gpu_ctx):
    hom, chr_, pos, effect, iv, want = case(65, R + 1, 3, 3)
    with abi.FeatureSet(gpu_ctx, hom.shape[0], 65, rows=fc.pack(hom)) as fs:
        with pytest.raises(abi.GarlicError, match="garlic_feature_set_sites") as e:
            fs.counts(iv, 3, 3)
        assert e.value.code == abi.ERR_STATE
        bad = pos.copy()
        bad[[10, 11]] = bad[[11, 10]] + np.array([1, 0], dtype=np.int32)
        assert chr_[10] == chr_[11] and bad[11] < bad[10]
        with pytest.raises(abi.GarlicError, match="not sorted") as e:
            fs.set_sites(chr_, bad, effect)
        assert e.value.code == abi.ERR_INVALID
        with pytest.raises(abi.GarlicError, match="effect"):
            fs.set_sites(chr_, pos, np.where(np.arange(R + 1) == 5, abi.FEATURE_MAX_EFFECTS, effect))
        fs.set_sites(chr_, pos, effect)
        k = int(np.nonzero((iv["ind"][1:] == iv["ind"][:-1]) & (iv["chr"][1:] == iv["chr"][:-1]))[0][0]) + 1
        for what, change in (("overlaps", lambda v: v["start"].__setitem__(k, v["stop"][k - 1] - 1) if v["stop"][k - 1] > v["start"][k - 1]
                              else (v["stop"].__setitem__(k - 1, v["start"][k] + 1))),
                             ("not ordered", lambda v: v["ind"].__setitem__(0, 64)),
                             ("class", lambda v: v["cls"].__setitem__(3, 3)),
                             ("class", lambda v: v["cls"].__setitem__(3, -1)),
                             ("individual", lambda v: v["ind"].__setitem__(v.shape[0] - 1, 65))):
            v = iv.copy()
            change(v)
            with pytest.raises(abi.GarlicError, match=what) as e:
                fs.counts(v, 3, 3)
            assert e.value.code == abi.ERR_INVALID, what
        for n_classes, n_effects, what in ((3, abi.FEATURE_MAX_EFFECTS + 1, "effects"), (9, 3, "classes"), (0, 3, "classes"),
                                           (3, 2, "n_effects is 2")):
            with pytest.raises(abi.GarlicError, match=what) as e:
                fs.counts(iv, n_classes, n_effects)
            assert e.value.code == abi.ERR_INVALID, what
        assert np.array_equal(fs.counts(iv, 3, 3), want), "a refused call leaves the set usable"
