"""GPU: the KDE of a feed split into sorted parts (garlic_kde_parts: every part a part set of one feed,
csrc/kde_part_set_kernels.hpp, csrc/kde_kernels.hpp: kde_sum_kernel, kde_slice_sum_kernel) against the long-double numpy reference of tests/kde_cases.py evaluated on
the UNION -- never against a second run of the kernels, except where the claim is that two runs agree (one part and
garlic_feed_kde, the same call twice, two contexts, the step calls composed here).  All parts sit on the one device.

Tolerances: those derived at the top of tests/test_gpu_kde.py, restated (none of them from what the kernels give):
  n, q25, q75, lo, hi   bit for bit (the order statistics are exact whatever the split).
  h, sd     relative 1e-13 against the long-double reference: summation trees of depth <= 40 with three roundings per
            term, the mean's error entering squared, give <~ 5e-15 on sd; an order of margin.
  x         bit for bit against the formula evaluated from the returned h, lo, hi.
  raw       |got - want| <= 1e-12 want + 1e-300 against the reference evaluated at the returned h and x: the argument
            carries <= 4 roundings, the sum at most (4 * 746 + 64) * 2^-53 ~ 3.4e-13, rounded up.
  y         bit for bit from the returned raw and x by the sequential rule.
The derivation still holds for parts: combining them is at most 64 further sequential adds of non-negative terms, which
adds 64 * 2^-53 ~ 7e-15 to either sum's relative error -- inside the margin of both bounds.
The long-double sums cost 0.1 us per (source, target) pair, so at BIG one split with several parts (interleaved, two
parts) is checked at all 512 targets and the others at 16 of them (both ends, every thread quarter of the sums kernel
among them): the kernels treat every target alike."""
import ctypes as C
import math

import numpy as np
import pytest

import feed_sort_cases as fcases
import kde_cases as cases
import kde_parts_cases as pcases
import oracle_lib as ol
from garlic_amd import abi

pytestmark = pytest.mark.gpu
MG, ERROR, M, MU = fcases.MG, fcases.ERROR, fcases.M, fcases.MU
FIELDS = ("n", "h", "sd", "q25", "q75", "lo", "hi")
INT_AND_ORDER = ("n", "q25", "q75", "lo", "hi")
FEW = np.array([0, 1, 37, 74, 111, 130, 185, 222, 257, 296, 333, 383, 444, 481, 510, 511])


def same_struct(a, b):
    return all(np.float64(a[k]).tobytes() == np.float64(b[k]).tobytes() for k in FIELDS) and \
        all(ol.bits_equal(a[k], b[k]) for k in ("x", "y", "raw"))


class Parts:
    """the parts of one split on a context, from host or device buffers; closes them on exit"""

    def __init__(self, ctxs, arrays, device=False):
        import torch
        ctxs = ctxs if isinstance(ctxs, (list, tuple)) else [ctxs]
        self.tensors, self.parts = [], []
        for i, a in enumerate(arrays):
            ctx = ctxs[i % len(ctxs)]
            if device:
                t = torch.from_numpy(np.array(a)).cuda()
                self.tensors.append((t, a))
                self.parts.append(ctx.kde_part(t.data_ptr() if a.shape[0] else 0, n=a.shape[0]))
            else:
                self.parts.append(ctx.kde_part(np.ascontiguousarray(a)))

    def __enter__(self):
        return self.parts

    def __exit__(self, *exc):
        import torch
        for p in self.parts:
            p.close()
        torch.cuda.synchronize()
        for t, a in self.tensors:
            assert ol.bits_equal(t.cpu().numpy(), a), "the caller's device buffer was modified"


_raw_cache = {}


def check_kde(got, x, what, at=None):
    """every field of got against the reference of the ascending union x; raw at the targets `at` (default: all)"""
    n = x.shape[0]
    at = np.arange(cases.POINTS) if at is None else at
    ref = cases.reference(x, with_raw=False)
    assert got["n"] == n, what
    want_h = np.longdouble(0.9) * min(ref["sd"], np.longdouble((ref["q75"] - ref["q25"]) / 1.34)) * np.longdouble(float(n)) ** np.longdouble(-0.2)
    print(what, "h rel err %.3g" % abs(float((np.longdouble(got["h"]) - want_h) / want_h)))
    assert abs(np.longdouble(got["h"]) - want_h) <= np.longdouble(1e-13) * want_h, (what, got["h"], want_h)
    assert abs(np.longdouble(got["sd"]) - ref["sd"]) <= np.longdouble(1e-13) * ref["sd"], (what, got["sd"], ref["sd"])
    for k in ("q25", "q75", "lo", "hi"):
        assert np.float64(got[k]).tobytes() == np.float64(ref[k]).tobytes(), (what, k, got[k], ref[k])
    assert ol.bits_equal(got["x"], cases.targets(got["lo"], got["hi"], got["h"])), (what, "x")
    key = (n, x[:64].tobytes(), np.float64(got["h"]).tobytes(), got["x"].tobytes(), at.tobytes())
    if key not in _raw_cache:
        _raw_cache[key] = cases.raw_longdouble(x, got["x"][at], got["h"])
    want = _raw_cache[key]
    err = np.abs(got["raw"][at].astype(np.longdouble) - want)
    bound = np.longdouble(1e-12) * want + np.longdouble(1e-300)
    worst = float(np.max(err / bound))
    print(what, "raw: worst error / bound %.3g" % worst)
    assert (err <= bound).all(), (what, "raw", worst, int(np.argmax(err / bound)))
    assert ol.bits_equal(got["y"], cases.normalise(got["raw"], got["x"])), (what, "y")


# --------------------------------------------------------------------------------------------- 1. every content x every split

@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("n", pcases.totals())
@pytest.mark.parametrize("name", cases.CONTENTS)
def test_parts_every_content_and_split(gpu_ctx, name, n, device):
    x = cases.content(name, n)
    chunk = cases.kde_chunk()
    for i, (label, arrays) in enumerate(pcases.splits(name, n)):
        with Parts(gpu_ctx, arrays, device) as parts:
            got = abi.kde_parts(parts)
            info = abi.kde_parts_info(parts)
            assert [p.count() for p in parts] == [a.shape[0] for a in arrays]
        check_kde(got, x, (name, n, label), at=FEW if n >= cases.BIG and i != 1 else None)
        assert info["rank_rounds"] == 8, (label, info)
        assert list(info["chunks"]) == [(a.shape[0] + chunk - 1) // chunk for a in arrays], (label, info)
        assert all(0 <= s <= c * 512 for s, c in zip(info["pairs_skipped"], info["chunks"]))
        if name == "wide" and label.startswith("ranges") and n >= 3 * chunk + 17:
            # a contiguous part spans a fraction of the range of +-2e4 at h <~ 1: targets far from it contribute exactly 0
            assert all(s > 0 for s, a in zip(info["pairs_skipped"], arrays) if a.shape[0]), (label, info)
        if name == "narrow":
            assert not info["pairs_skipped"].any(), (label, info)


def test_parts_with_signed_zeros_and_ties(gpu_ctx):
    x, arrays = pcases.zero_feed()
    with Parts(gpu_ctx, arrays) as parts:
        got = abi.kde_parts(parts)
    want = gpu_ctx.feed_kde(x)
    for k in INT_AND_ORDER:
        assert np.float64(got[k]).tobytes() == np.float64(want[k]).tobytes(), k
    assert np.float64(got["q25"]).tobytes() == np.float64(cases.quantile(x, 0.25)).tobytes()
    assert np.float64(got["q75"]).tobytes() == np.float64(cases.quantile(x, 0.75)).tobytes()


# --------------------------------------------------------------------------------------------- 2. identities and determinism

@pytest.mark.parametrize("name", ["bimodal", "wide"])
def test_one_part_is_feed_kde_bit_for_bit(gpu_ctx, name):
    for n in (3 * cases.kde_chunk() + 17, cases.BIG):
        x = cases.content(name, n)
        want = gpu_ctx.feed_kde(x)
        want_info = gpu_ctx.feed_kde_info()
        for device in (False, True):
            with Parts(gpu_ctx, [x], device) as parts:
                got = abi.kde_parts(parts)
                again = abi.kde_parts(parts)
                info = abi.kde_parts_info(parts)
            assert same_struct(got, want), (name, n, device)
            assert same_struct(again, got), (name, n, device, "the same call twice")
            assert info["chunks"][0] == want_info["chunks"] and info["pairs_skipped"][0] == want_info["pairs_skipped"]
            assert info["sums_ms"][0] > 0


def test_same_bits_twice_on_two_contexts_and_permuted(gpu_ctx):
    n = 3 * cases.kde_chunk() + 17
    x = cases.content("bimodal", n)
    arrays = pcases.interleaved(x, 3)
    with Parts(gpu_ctx, arrays) as parts:
        first = abi.kde_parts(parts)
        assert same_struct(abi.kde_parts(parts), first), "the same call twice"
        permuted = abi.kde_parts([parts[2], parts[0], parts[1]])
    with abi.Context(0) as other:
        with Parts([gpu_ctx, other], arrays) as parts:
            assert same_struct(abi.kde_parts(parts), first), "parts on two contexts of the device"
    for k in INT_AND_ORDER:
        assert np.float64(permuted[k]).tobytes() == np.float64(first[k]).tobytes(), k
    check_kde(permuted, x, "permuted parts")


def compose(parts):
    """garlic_kde_parts from the step calls, by the rules of include/garlic_hip.h"""
    counts = [p.count() for p in parts]
    n = sum(counts)
    total, lo, hi = 0.0, None, None
    for p in parts:
        s, a, b = p.moment(0)
        total = total + s
        if a is not None:
            lo = a if lo is None or pcases.key([a])[0] < pcases.key([lo])[0] else lo
            hi = b if hi is None or pcases.key([b])[0] > pcases.key([hi])[0] else hi
    mean = total / float(n)
    ssq = 0.0
    for p in parts:
        ssq = ssq + p.moment(1, mean)
    sd = math.sqrt(ssq / float(n - 1))
    stat, rounds = pcases.descent(lambda probes: sum(p.rank(probes) for p in parts), pcases.order_ranks(n))
    assert rounds == 8
    q = []
    for f, (a, b) in ((0.25, stat[:2]), (0.75, stat[2:])):
        idx = f * float(n - 1)
        k = int(idx)
        d = idx - float(k)
        q.append(float(a) if k >= n - 1 else float((1 - d) * float(a) + d * float(b)))
    h = cases.bandwidth(sd, q[0], q[1], n)
    t = cases.targets(lo, hi, h)
    sums = [p.sums(t, h) for p in parts]
    raw = np.zeros(cases.POINTS)
    for j in range(cases.POINTS):
        acc = 0.0
        for s in sums:
            acc = acc + float(s[j])
        raw[j] = acc / float(n)
    return {"n": n, "h": h, "sd": sd, "q25": q[0], "q75": q[1], "lo": lo, "hi": hi, "x": t, "raw": raw, "y": cases.normalise(raw, t)}


@pytest.mark.parametrize("name,n,split", [("bimodal", 3 * 2048 + 17, "interleaved3"), ("wide", 3 * 2048 + 17, "lopsided rest+0+2"),
                                          ("two_values", 65, "interleaved2"), ("uniform", 3, "lopsided 1+rest")])
def test_step_calls_compose_to_kde_parts(gpu_ctx, name, n, split):
    arrays = dict(pcases.splits(name, n))[split]
    with Parts(gpu_ctx, arrays) as parts:
        want = abi.kde_parts(parts)
        got = compose(parts)
    assert same_struct(got, want), (name, n, split)


def test_rank_against_searchsorted(gpu_ctx):
    x = cases.content("two_values", 65)
    big = cases.content("bimodal", cases.BIG)
    rng = np.random.default_rng(5)
    with Parts(gpu_ctx, [x, x[:0], big]) as (small, empty, large):
        for part, v in ((small, x), (empty, x[:0]), (large, big)):
            k = pcases.key(v)
            inside = pcases.key(rng.uniform(-30.0, 15.0, 200))
            on = k[rng.integers(0, len(k), 300)] if len(k) else np.zeros(0, dtype=np.uint64)
            ends = np.array([0, 1, 2 ** 63 - 1, 2 ** 63, 2 ** 64 - 1], dtype=np.uint64)        # below and above every value
            around = np.concatenate([on - np.uint64(1), on + np.uint64(1)])
            probes = np.concatenate([ends, pcases.key([-1e300, 1e300, -1.5, 2.25, 0.0, -0.0]), inside, on, around])[:1024]
            probes = np.concatenate([probes, rng.integers(0, 2 ** 64, 1024 - len(probes), dtype=np.uint64)])
            assert len(probes) == 1024
            assert np.array_equal(part.rank(probes), np.searchsorted(k, probes, side="left")), len(v)
            for one in probes[:8]:
                assert part.rank([one])[0] == np.searchsorted(k, one, side="left")
        L = abi.lib()
        buf = (C.c_uint64 * 1025)()
        out = (C.c_int64 * 1025)()
        for m in (0, 1025, -1):
            assert L.garlic_kde_part_rank(small.handle, buf, m, out) == abi.ERR_INVALID


# --------------------------------------------------------------------------------------------- 3. Panel.lod_kde_part

NIND, CUT, W = 200, 128, 10


def open_panels(ctx):
    chroms, _, _, _, _, _ = fcases.panel(NIND)
    panels = []
    for b, e in ((0, NIND), (0, CUT), (CUT, NIND)):
        p = abi.Panel(ctx, [c[0].shape[0] for c in chroms], e - b)
        p.set_map(np.concatenate([c[2] for c in chroms]), [c[3] for c in chroms], [c[4] for c in chroms])
        p.set_freq(np.concatenate([c[1] for c in chroms]))
        p.set_genotypes(np.ascontiguousarray(np.concatenate([c[0] for c in chroms], axis=0)[:, b:e]))
        panels.append(p)
    return panels


@pytest.mark.parametrize("subset", [False, True], ids=["everyone", "subset"])
def test_lod_kde_part_on_two_panels_that_split_one(gpu_ctx, subset):
    whole, a, b = open_panels(gpu_ctx)
    with whole, a, b:
        idx = sorted(fcases.SUBSET) if subset else None
        split = [None, None] if idx is None else [[i for i in idx if i < CUT], [i - CUT for i in idx if i >= CUT]]
        feed, per_chr = whole.lod_feed(W, ERROR, MG, W, ind_idx=idx)
        union = np.sort(feed)
        pa, chr_a = a.lod_kde_part(W, ERROR, MG, W, ind_idx=split[0])
        pb, chr_b = b.lod_kde_part(W, ERROR, MG, W, ind_idx=split[1])
        with pa, pb:
            assert pa.count() + pb.count() == len(feed) and pa.count() > 0 and pb.count() > 0
            assert list(chr_a + chr_b) == list(per_chr)
            got = abi.kde_parts([pa, pb])
            check_kde(got, union, ("two panels", subset))
            # a part is stale once its panel computes another feed; the other panel's part is not
            a.lod_feed(W, ERROR, MG, W)
            for call in (pa.count, lambda: pa.moment(0), lambda: pa.rank([0]), lambda: abi.kde_parts([pa, pb]),
                         lambda: abi.kde_parts_info([pa, pb])):
                with pytest.raises(abi.GarlicError) as e:
                    call()
                assert e.value.code == abi.ERR_STATE and "stale" in str(e.value)
            assert pb.count() > 0
            b.release_scratch()
            with pytest.raises(abi.GarlicError) as e:
                pb.count()
            assert e.value.code == abi.ERR_STATE
        # an empty feed (a window wider than every chromosome) is a valid, empty part
        pe, _ = a.lod_kde_part(5000, ERROR, MG, 5000)
        with pe:
            assert pe.count() == 0 and pe.moment(0) == (0.0, None, None)


# --------------------------------------------------------------------------------------------- 4. refusals (argument checks)

def refused(parts_or_handles, n_parts=None):
    out = abi.Kde()
    C.memset(C.byref(out), 0x5A, C.sizeof(out))
    before = bytes(out)
    if n_parts is None:
        with pytest.raises(abi.GarlicError) as e:
            abi.kde_parts(parts_or_handles, out=out)
        code, msg = e.value.code, str(e.value)
    else:
        code = abi.lib().garlic_kde_parts(parts_or_handles, n_parts, C.byref(out))
        msg = abi.lib().garlic_hip_last_error().decode()
    assert bytes(out) == before, msg
    return code, msg


def test_parts_refusals_to_the_letter(gpu_ctx):
    """garlic_kde_parts on the bad feeds of tests/test_gpu_kde.py split in two says garlic_feed_kde's sentences, with "the
    parts hold" for the count: nothing of the sets behind the parts ("feed 0: ", "set 1: ") shows"""
    from test_gpu_kde import bad_feeds, refusal_text
    for what, x, _ in bad_feeds():
        half = x.shape[0] // 2
        with Parts(gpu_ctx, [x[:half], x[half:]]) as parts:
            code, msg = refused((C.c_void_p * 2)(parts[0].handle, parts[1].handle), 2)
        assert code == abi.ERR_INVALID and msg == refusal_text(x, "the parts hold"), (what, msg)
    # two parts refused for different reasons: every part is waited for and each refusal leaves its sentence, so the text
    # is the last refused part's (the code is the first's; both are GARLIC_ERR_INVALID)
    feeds = {what: x for what, x, _ in bad_feeds()}
    descending, nan = feeds["swapped inside a chunk"], feeds["NaN in the middle"]
    for arrays, want in (([descending, nan], nan), ([nan, descending], descending)):
        with Parts(gpu_ctx, arrays) as parts:
            code, msg = refused((C.c_void_p * 2)(parts[0].handle, parts[1].handle), 2)
        assert code == abi.ERR_INVALID and msg == refusal_text(want, "the parts hold"), msg


def test_parts_info_is_of_the_last_sums_and_the_last_kde_parts(gpu_ctx):
    """garlic_kde_parts_info answers zeros before anything ran; chunks, pairs_skipped and sums_ms are of a part's last sums
    (garlic_kde_parts or the step call), rank_rounds of the last garlic_kde_parts alone: rank step calls do not count"""
    chunk = cases.kde_chunk()
    x = cases.content("wide", 3 * chunk + 17)
    arrays = [np.ascontiguousarray(x[:chunk + 1]), np.ascontiguousarray(x[chunk + 1:])]
    with Parts(gpu_ctx, arrays) as parts:
        info = abi.kde_parts_info(parts)
        assert list(info["chunks"]) == [0, 0] and not info["pairs_skipped"].any() and info["rank_rounds"] == 0, info
        assert list(info["sums_ms"]) == [0, 0], info
        parts[0].rank([0, 1])
        assert abi.kde_parts_info(parts)["rank_rounds"] == 0
        got = abi.kde_parts(parts)
        parts[0].rank([0, 1])
        info = abi.kde_parts_info(parts)
        assert info["rank_rounds"] == 8 and list(info["chunks"]) == [(a.shape[0] + chunk - 1) // chunk for a in arrays] == [2, 3], info
        assert all(s > 0 for s in info["pairs_skipped"]) and all(ms > 0 for ms in info["sums_ms"]), info
        parts[1].sums(got["x"], 1e4)                       # the step call with a bandwidth at which no argument reaches -746
        after = abi.kde_parts_info(parts)
        assert after["pairs_skipped"][0] == info["pairs_skipped"][0] and after["pairs_skipped"][1] == 0, (info, after)
        assert after["rank_rounds"] == 8


def test_refusals_leave_the_output_untouched(gpu_ctx):
    c = cases.kde_chunk()
    base = np.array(cases.content("bimodal", 3 * c + 17))
    half = len(base) // 2
    nan = base[half:].copy(); nan[len(nan) // 3] = np.nan
    descent = base[half:].copy(); descent[[c + 100, c + 101]] = descent[[c + 101, c + 100]]
    assert descent[c + 100] > descent[c + 101]
    for what, arrays, word in [("n = 0", [base[:0], base[:0]], "at least 2"), ("n = 1", [base[:0], base[:1]], "at least 2"),
                               ("all equal", [np.full(c + 5, -3.25), np.full(7, -3.25)], "bandwidth"),
                               ("a NaN in the second part", [base[:half], nan], "NaN"),
                               ("a descent inside a part", [base[:half], descent], "ascending")]:
        with Parts(gpu_ctx, arrays) as parts:
            code, msg = refused(parts)
            assert code == abi.ERR_INVALID and word in msg, (what, msg)
    with Parts(gpu_ctx, [base[:half], base[half:]]) as parts:
        handles = (C.c_void_p * 65)(*[parts[i % 2].handle for i in range(65)])
        assert refused(handles, 0)[0] == abi.ERR_INVALID and refused(handles, 65)[0] == abi.ERR_INVALID
        assert refused(handles, -1)[0] == abi.ERR_INVALID
        assert refused(None, 2)[0] == abi.ERR_INVALID
        code, msg = refused([parts[0], None])
        assert code == abi.ERR_INVALID and "NULL" in msg
        code, msg = refused([parts[0], parts[1], parts[0]])
        assert code == abi.ERR_INVALID and "again" in msg
        assert abi.lib().garlic_kde_parts(handles, 2, None) == abi.ERR_INVALID
        with pytest.raises(abi.GarlicError) as e:       # the step call names the cause too
            parts[0].moment(2)
        assert e.value.code == abi.ERR_INVALID
        good = abi.kde_parts(parts)                     # and the parts still work
        check_kde(good, base, "after the refusals")
    with Parts(gpu_ctx, [nan]) as parts:
        with pytest.raises(abi.GarlicError) as e:
            parts[0].moment(0)
        assert e.value.code == abi.ERR_INVALID and "NaN" in str(e.value)
    L = abi.lib()
    h = C.c_void_p()
    x = np.array([1.0, 2.0])
    assert L.garlic_kde_part_create(gpu_ctx.handle, C.c_void_p(x.ctypes.data), -1, abi.HOST, C.byref(h)) == abi.ERR_INVALID
    assert L.garlic_kde_part_create(gpu_ctx.handle, None, 2, abi.HOST, C.byref(h)) == abi.ERR_INVALID
    assert L.garlic_kde_part_create(gpu_ctx.handle, C.c_void_p(x.ctypes.data), 2, 7, C.byref(h)) == abi.ERR_INVALID
    assert L.garlic_kde_part_create(gpu_ctx.handle, C.c_void_p(x.ctypes.data), 2, abi.HOST, None) == abi.ERR_INVALID
    assert L.garlic_kde_part_destroy(None) == abi.OK
