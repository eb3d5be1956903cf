"""GPU: the KDEs of several split feeds at once (garlic_kde_parts_multi over garlic_kde_part_set, csrc/kde_part_set_kernels.hpp,
kde_rank_multi_kernel).  The contract is equality, so there are no tolerances here: every struct equals garlic_kde_parts's
for the same parts in every field bit for bit (tests/test_gpu_kde_parts.py holds garlic_kde_parts against the long-double
reference), one set equals garlic_feed_kde_multi's, the step calls compose to the same bits, and the batched rank equals
numpy.searchsorted on keys.  All sets sit on the one device."""
import ctypes as C
import math

import numpy as np
import pytest

import feed_sort_cases as fcases
import kde_cases as cases
import kde_parts_cases as pcases
import kde_parts_multi_cases as mcases
import oracle_lib as ol
from garlic_amd import abi

pytestmark = pytest.mark.gpu
MG, ERROR = fcases.MG, fcases.ERROR
FIELDS = ("n", "h", "sd", "q25", "q75", "lo", "hi")
INT_AND_ORDER = ("n", "q25", "q75", "lo", "hi")


def same_struct(a, b):
    return all(np.float64(a[k]).tobytes() == np.float64(b[k]).tobytes() for k in FIELDS) and \
        all(ol.bits_equal(a[k], b[k]) for k in ("x", "y", "raw"))


class Sets:
    """the sets of a batch [(label, [part of set 0, ...])] on one or several contexts, from host or device buffers"""

    def __init__(self, ctxs, feeds, device=False):
        import torch
        ctxs = ctxs if isinstance(ctxs, (list, tuple)) else [ctxs]
        P = len(feeds[0][1])
        assert all(len(parts) == P for _, parts in feeds)
        self.tensors, self.sets = [], []
        for p, arrays in enumerate(mcases.sets_of(feeds, P)):
            ctx = ctxs[p % len(ctxs)]
            if device:
                ts = [torch.from_numpy(np.array(a)).cuda() for a in arrays]
                self.tensors += list(zip(ts, arrays))
                self.sets.append(ctx.kde_part_set([t.data_ptr() if a.shape[0] else 0 for t, a in zip(ts, arrays)],
                                                  ns=[a.shape[0] for a in arrays]))
            else:
                self.sets.append(ctx.kde_part_set([np.ascontiguousarray(a) for a in arrays]))

    def __enter__(self):
        return self.sets

    def __exit__(self, *exc):
        import torch
        for s in self.sets:
            s.close()
        torch.cuda.synchronize()
        for t, a in self.tensors:
            assert ol.bits_equal(t.cpu().numpy(), a), "the caller's device buffer was modified"


def parts_kde(ctx, arrays):
    """garlic_kde_parts over single parts of the same values: the struct, or the GarlicError it refuses with"""
    parts = [ctx.kde_part(np.ascontiguousarray(a)) for a in arrays]
    try:
        return abi.kde_parts(parts)
    except abi.GarlicError as e:
        return e
    finally:
        for p in parts:
            p.close()


_want = {}


def want_of(ctx, label, arrays):
    """computed once per (label, number of parts), shared and never written to"""
    key = (label, len(arrays))
    if key not in _want:
        _want[key] = parts_kde(ctx, arrays)
    return _want[key]


def check_batch(ctx, feeds, device, what):
    chunk = cases.kde_chunk()
    with Sets(ctx, feeds, device) as sets:
        got, status = abi.kde_parts_multi(sets)
        info = abi.kde_parts_multi_info(sets)
        for p, s in enumerate(sets):
            assert list(s.counts()) == [parts[p].shape[0] for _, parts in feeds]
    for i, (label, parts) in enumerate(feeds):
        want = want_of(ctx, label, parts)
        if isinstance(want, abi.GarlicError):
            assert status[i] == want.code and got[i] is None, (what, i, label)
            continue
        assert status[i] == abi.OK and same_struct(got[i], want), (what, i, label)
        for p, a in enumerate(parts):
            assert info["chunks"][p, i] == (a.shape[0] + chunk - 1) // chunk
            assert 0 <= info["pairs_skipped"][p, i] <= info["chunks"][p, i] * 512
    return info


# --------------------------------------------------------------------------------------------- 1. equality with garlic_kde_parts

@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("F,P,shift", [(1, 1, 0), (1, 2, 4), (2, 2, 1), (2, 3, 3), (4, 1, 2), (4, 3, 0), (4, 8, 1), (2, 8, 2), (32, 2, 0)])
def test_multi_equals_kde_parts_per_feed(gpu_ctx, F, P, shift, device):
    feeds = mcases.batch(F, P, shift)
    info = check_batch(gpu_ctx, feeds, device, (F, P, shift))
    with_values = [p for p in range(P) if any(parts[p].shape[0] for _, parts in feeds)]
    assert all(info["kernel_launches"][p] == 14 and info["host_waits"][p] == 11 and info["rank_rounds"][p] == 8 for p in with_values), info


def test_every_total_and_split_kind_is_in_the_batches():
    seen = set()
    for F, P, shift in [(1, 1, 0), (1, 2, 4), (2, 2, 1), (2, 3, 3), (4, 1, 2), (4, 3, 0), (4, 8, 1), (2, 8, 2), (32, 2, 0)]:
        for label, _ in mcases.batch(F, P, shift):
            name, n, kind = label.split()
            seen.add((int(n), kind if P > 1 else "one"))
    for n in pcases.totals():
        for kind in mcases.KINDS:
            assert (n, kind) in seen, (n, kind)


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_mixed_lengths_and_a_feed_that_is_empty_in_one_set(gpu_ctx, device):
    """unions of 0, 1, 2, 3 and 65 values, ties and zeros crossing the sets, next to feeds of several chunks; set 0 holds
    nothing of "0+all", and nothing at all of the first two feeds"""
    big = cases.content("wide", 3 * cases.kde_chunk() + 17)
    feeds = mcases.small_mixed() + mcases.tied() + [("0+all wide", [mcases.EMPTY, np.ascontiguousarray(big)])] + mcases.batch(2, 2, shift=1)
    check_batch(gpu_ctx, feeds, device, "mixed")
    with Sets(gpu_ctx, feeds, device) as sets:
        got, status = abi.kde_parts_multi(sets)
        msg = abi.lib().garlic_hip_last_error().decode()
    assert status[:2] == [abi.ERR_INVALID, abi.ERR_INVALID] and all(s == abi.OK for s in status[2:]), status
    assert msg.startswith("feed 0:") and "at least 2" in msg, msg


def test_one_set_is_feed_kde_multi_bit_for_bit(gpu_ctx):
    feeds = mcases.batch(4, 1, shift=1) + [("one value", [np.array([2.5])])]
    arrays = [parts[0] for _, parts in feeds]
    want, want_status, _ = gpu_ctx.feed_kde_multi([np.ascontiguousarray(a) for a in arrays])
    with Sets(gpu_ctx, feeds) as sets:
        got, status = abi.kde_parts_multi(sets)
    assert status == want_status and status[-1] == abi.ERR_INVALID
    for g, w in zip(got[:-1], want[:-1]):
        assert same_struct(g, w)
    assert got[-1] is None and want[-1] is None


def test_a_part_is_a_set_of_one_feed(gpu_ctx):
    """garlic_kde_parts over [2 values, the rest, an empty part] and garlic_kde_parts_multi over three sets of one feed made
    of the same values: one struct, and garlic_kde_parts_info still answers per part"""
    chunk = cases.kde_chunk()
    x = cases.content("bimodal", 3 * chunk + 17)
    arrays = [np.ascontiguousarray(x[:2]), np.ascontiguousarray(x[2:]), mcases.EMPTY]
    parts = [gpu_ctx.kde_part(a) for a in arrays]
    try:
        want = abi.kde_parts(parts)
        info = abi.kde_parts_info(parts)
    finally:
        for p in parts:
            p.close()
    with Sets(gpu_ctx, [("2 + rest + 0", arrays)]) as sets:
        got, status = abi.kde_parts_multi(sets)
    assert status == [abi.OK] and same_struct(got[0], want)
    assert info["rank_rounds"] == 8, info
    assert list(info["chunks"]) == [1, 4, 0] == [(a.shape[0] + chunk - 1) // chunk for a in arrays], info
    assert info["pairs_skipped"][2] == 0 and info["sums_ms"][0] > 0 and info["sums_ms"][1] > 0 and info["sums_ms"][2] == 0, info


# --------------------------------------------------------------------------------------------- 2. per-feed refusal

def refusal_feeds():
    c = cases.kde_chunk()
    base = np.array(cases.content("bimodal", 3 * c + 17))
    half = len(base) // 2
    nan = base[half:].copy()
    nan[len(nan) // 3] = np.nan
    good = mcases.batch(3, 2, shift=2)
    return [good[0], ("all equal", [np.full(c + 5, -3.25), np.full(7, -3.25)]), good[1],
            ("union of one value", [mcases.EMPTY, np.array([4.0])]), ("a NaN in set 1", [np.ascontiguousarray(base[:half]), nan]), good[2]]


def test_refused_feeds_leave_their_outputs_and_the_good_feeds_alone(gpu_ctx):
    feeds = refusal_feeds()
    bad = {1: "bandwidth", 3: "at least 2", 4: "NaN"}
    outs = (abi.Kde * len(feeds))()
    C.memset(outs, 0x5A, C.sizeof(outs))
    before = bytes(outs)
    one = C.sizeof(abi.Kde)
    with Sets(gpu_ctx, feeds) as sets:
        got, status = abi.kde_parts_multi(sets, outs=outs)
        msg = abi.lib().garlic_hip_last_error().decode()
        for i, (label, parts) in enumerate(feeds):
            if i in bad:
                assert status[i] == abi.ERR_INVALID and got[i] is None, (i, label)
                assert bytes(outs)[i * one:(i + 1) * one] == before[i * one:(i + 1) * one], (label, "a refused output was written")
                want = want_of(gpu_ctx, label, parts)
                assert isinstance(want, abi.GarlicError) and bad[i] in str(want), (label, str(want))
            else:
                assert status[i] == abi.OK and same_struct(got[i], want_of(gpu_ctx, label, parts)), (i, label)
        assert msg.startswith("feed 1:") and "bandwidth" in msg, msg        # the lowest refused index
        # status NULL: as garlic_feed_kde_multi, the call fails at the first step that refuses a feed (the union of one value
        # is known before anything runs), with that feed's code and text, all outputs untouched
        C.memset(outs, 0x5A, C.sizeof(outs))
        with pytest.raises(abi.GarlicError) as e:
            abi.kde_parts_multi(sets, strict=True, outs=outs)
        assert e.value.code == abi.ERR_INVALID and "feed 3:" in str(e.value) and "at least 2" in str(e.value)
        assert bytes(outs) == before
        again, status2 = abi.kde_parts_multi(sets)                        # and the sets still work
        assert status2 == status and all(same_struct(a, g) for a, g in zip(again, got) if g is not None)
    # a part at fault is named with its set; the lowest refused feed is the NaN one here
    with Sets(gpu_ctx, [feeds[0], feeds[4], feeds[1]]) as sets:
        _, status = abi.kde_parts_multi(sets)
        msg = abi.lib().garlic_hip_last_error().decode()
    assert status == [abi.OK, abi.ERR_INVALID, abi.ERR_INVALID] and msg.startswith("feed 1: set 1:") and "NaN" in msg, msg


def test_argument_refusals(gpu_ctx):
    feeds = mcases.batch(2, 2)
    L = abi.lib()
    with Sets(gpu_ctx, feeds) as sets, Sets(gpu_ctx, mcases.batch(3, 1)) as other:
        outs, st = (abi.Kde * 2)(), (C.c_int32 * 2)()
        handles = (C.c_void_p * 65)(*[sets[i % 2].handle for i in range(65)])
        for n in (0, -1, 65):
            assert L.garlic_kde_parts_multi(handles, n, outs, st) == abi.ERR_INVALID
        assert L.garlic_kde_parts_multi(None, 2, outs, st) == abi.ERR_INVALID
        assert L.garlic_kde_parts_multi(handles, 2, None, st) == abi.ERR_INVALID
        for bad, word in (([sets[0], None], "NULL"), ([sets[0], sets[1], sets[0]], "again"), ([sets[0], other[0]], "feeds")):
            with pytest.raises(abi.GarlicError) as e:
                abi.kde_parts_multi(bad)
            assert e.value.code == abi.ERR_INVALID and word in str(e.value)
        with pytest.raises(abi.GarlicError):
            sets[0].moment(2)
        keys = np.zeros((2, 1025), dtype=np.uint64)
        with pytest.raises(abi.GarlicError):
            sets[0].rank(keys)
    x = np.array([1.0, 2.0])
    ptrs, h = (C.c_void_p * 33)(*[x.ctypes.data] * 33), C.c_void_p()
    ns = np.full(33, 2, dtype=np.int64)
    nsp = ns.ctypes.data_as(C.POINTER(C.c_int64))
    for n_feeds in (0, 33, -1):
        assert L.garlic_kde_part_set_create(gpu_ctx.handle, ptrs, nsp, n_feeds, abi.HOST, C.byref(h)) == abi.ERR_INVALID
    assert L.garlic_kde_part_set_create(gpu_ctx.handle, ptrs, nsp, 2, 7, C.byref(h)) == abi.ERR_INVALID
    ns[1] = -1
    assert L.garlic_kde_part_set_create(gpu_ctx.handle, ptrs, nsp, 2, abi.HOST, C.byref(h)) == abi.ERR_INVALID
    assert L.garlic_kde_part_set_destroy(None) == abi.OK


# --------------------------------------------------------------------------------------------- 3. the step calls

def compose(sets, n_feeds):
    """garlic_kde_parts_multi from the step calls, by the rules of include/garlic_hip.h: what one process per GPU would
    all-reduce is added (or compared by key) over the sets here.  -> ([struct or None], status)"""
    counts = np.array([s.counts() for s in sets])
    n = counts.sum(axis=0)
    status = np.where(n < 2, abi.ERR_INVALID, 0).astype(np.int32)
    part0 = [s.moment(0, status=status) for s in sets]
    for _, _, _, st in part0:
        status = np.maximum(status, st)
    mean, lo, hi = np.zeros(n_feeds), [None] * n_feeds, [None] * n_feeds
    for i in range(n_feeds):
        if status[i]:
            continue
        total = 0.0
        for p, (v, a, b, _) in enumerate(part0):
            total = total + float(v[i])
            if counts[p][i]:
                lo[i] = a[i] if lo[i] is None or pcases.key([a[i]])[0] < pcases.key([lo[i]])[0] else lo[i]
                hi[i] = b[i] if hi[i] is None or pcases.key([b[i]])[0] > pcases.key([hi[i]])[0] else hi[i]
        mean[i] = total / float(n[i])
    part1 = [s.moment(1, means=mean, status=status)[0] for s in sets]
    # the descent of every feed, eight rank calls per set in all
    on = [i for i in range(n_feeds) if not status[i]]
    prefix = np.zeros((n_feeds, 4), dtype=np.uint64)
    digits = np.arange(256, dtype=np.uint64)
    ranks = {i: pcases.order_ranks(int(n[i])) for i in on}
    for byte in range(7, -1, -1):
        shift = np.uint64(8 * byte)
        probes = (prefix[:, :, None] | (digits[None, None, :] << shift)).reshape(n_feeds, 1024)
        below = sum(s.rank(probes) for s in sets).reshape(n_feeds, 4, 256)
        for i in on:
            for q in range(4):
                d = int(np.nonzero(below[i, q] <= ranks[i][q])[0].max())
                prefix[i, q] |= np.uint64(d) << shift
    out, h, targets = [None] * n_feeds, np.ones(n_feeds), np.zeros((n_feeds, cases.POINTS))
    for i in on:
        ssq = 0.0
        for v in part1:
            ssq = ssq + float(v[i])
        sd = math.sqrt(ssq / float(n[i] - 1))
        stat = pcases.key_value(prefix[i])
        q = []
        for f, (a, b) in ((0.25, stat[:2]), (0.75, stat[2:])):
            idx = f * float(n[i] - 1)
            k = int(idx)
            d = idx - float(k)
            q.append(float(a) if k >= n[i] - 1 else float((1 - d) * float(a) + d * float(b)))
        bw = cases.bandwidth(sd, q[0], q[1], int(n[i]))
        if not (bw > 0 and math.isfinite(bw)):
            status[i] = abi.ERR_INVALID
            continue
        h[i] = bw
        targets[i] = cases.targets(lo[i], hi[i], bw)
        out[i] = {"n": int(n[i]), "h": bw, "sd": sd, "q25": q[0], "q75": q[1], "lo": lo[i], "hi": hi[i], "x": targets[i].copy()}
    sums = [s.sums(targets, h, active=(status == 0).astype(np.int32))[0] for s in sets]
    for i in range(n_feeds):
        if status[i]:
            out[i] = None
            continue
        raw = np.zeros(cases.POINTS)
        for j in range(cases.POINTS):
            acc = 0.0
            for s in sums:
                acc = acc + float(s[i, j])
            raw[j] = acc / float(n[i])
        out[i]["raw"] = raw
        out[i]["y"] = cases.normalise(raw, out[i]["x"])
    return out, [int(v) for v in status]


def test_step_calls_compose_to_kde_parts_multi(gpu_ctx):
    feeds = [("two_values 65 interleaved", pcases.interleaved(cases.content("two_values", 65), 3)),
             ("all equal", [np.full(9, -3.25), np.full(7, -3.25), mcases.EMPTY]),
             ("bimodal 3c+17 interleaved", pcases.interleaved(cases.content("bimodal", 3 * cases.kde_chunk() + 17), 3)),
             ("one value", [mcases.EMPTY, np.array([1.0]), mcases.EMPTY]),
             ("wide rest+0+2", dict(pcases.splits("wide", 3 * cases.kde_chunk() + 17))["lopsided rest+0+2"]),
             ("uniform 3", mcases.pad(dict(pcases.splits("uniform", 3))["lopsided 1+rest"], 3))]
    with Sets(gpu_ctx, feeds) as sets:
        want, want_status = abi.kde_parts_multi(sets)
        got, status = compose(sets, len(feeds))
        info = abi.kde_parts_multi_info(sets)
    assert status == want_status == [0, abi.ERR_INVALID, 0, abi.ERR_INVALID, 0, 0]
    for g, w, (label, _) in zip(got, want, feeds):
        assert (g is None and w is None) or same_struct(g, w), label
    assert list(info["kernel_launches"]) == [14] * 3 and list(info["host_waits"]) == [11] * 3 and list(info["rank_rounds"]) == [8] * 3


def test_batched_rank_against_searchsorted(gpu_ctx):
    rng = np.random.default_rng(5)
    values = [cases.content("two_values", 65), mcases.EMPTY, cases.content("bimodal", cases.BIG), np.array([0.0]),
              cases.content("uniform", 3 * cases.kde_chunk() + 17)]
    rows = []
    for v in values:
        k = pcases.key(v)
        on = k[rng.integers(0, len(k), 300)] if len(k) else np.zeros(0, dtype=np.uint64)
        ends = np.array([0, 1, 2 ** 63 - 1, 2 ** 63, 2 ** 64 - 1], dtype=np.uint64)        # below and above every value
        probes = np.concatenate([ends, pcases.key([-1e300, 1e300, -1.5, 2.25, 0.0, -0.0]), pcases.key(rng.uniform(-30.0, 15.0, 200)), on,
                                 on - np.uint64(1), on + np.uint64(1)])[:1024]
        rows.append(np.concatenate([probes, rng.integers(0, 2 ** 64, 1024 - len(probes), dtype=np.uint64)]))
    keys = np.array(rows)
    with gpu_ctx.kde_part_set([np.ascontiguousarray(v) for v in values]) as s:
        for m in (1024, 1, 77):
            got = s.rank(keys[:, :m])                       # (a set's first call may be a rank call)
            for i, v in enumerate(values):
                assert np.array_equal(got[i], np.searchsorted(pcases.key(v), keys[i, :m], side="left")), (i, m)


# --------------------------------------------------------------------------------------------- 4. info, determinism

def test_launches_and_waits_do_not_depend_on_the_number_of_feeds(gpu_ctx):
    per_f = {}
    for F in (1, 4):
        with Sets(gpu_ctx, mcases.batch(F, 2, shift=3)) as sets:
            abi.kde_parts_multi(sets, strict=True)
            info = abi.kde_parts_multi_info(sets)
        per_f[F] = (list(info["kernel_launches"]), list(info["host_waits"]), list(info["rank_rounds"]))
        assert (info["sums_ms"] > 0).all() and (info["moments_ms"] > 0).all()
    assert per_f[1] == per_f[4] == ([14, 14], [11, 11], [8, 8])


def test_same_bits_twice_and_on_two_contexts(gpu_ctx):
    feeds = mcases.batch(4, 3, shift=0)
    with Sets(gpu_ctx, feeds) as sets:
        first, status = abi.kde_parts_multi(sets)
        again, _ = abi.kde_parts_multi(sets)
    with abi.Context(0) as other:
        with Sets([gpu_ctx, other], feeds) as sets:
            split, _ = abi.kde_parts_multi(sets)
    assert status == [abi.OK] * 4
    for a, b, c in zip(first, again, split):
        assert same_struct(a, b) and same_struct(a, c)


# --------------------------------------------------------------------------------------------- 5. Panel.lod_kde_part_set

NIND, CUT, SIZES = 48, 31, [10, 60, 100]


_chroms = []


def open_panels(ctx):
    """3290 SNPs x 48 individuals on three chromosomes (the last one narrower than the widest window): the whole panel, and
    two panels that split its individuals"""
    if not _chroms:
        rng = np.random.default_rng(9911)
        _chroms.extend(ol.random_panel(rng, n, NIND, max_gap=MG) for n in (2000, 1200, 90))
    chroms = _chroms
    panels = []
    for b, e in ((0, NIND), (0, CUT), (CUT, NIND)):
        p = abi.Panel(ctx, [c[0].shape[0] for c in chroms], e - b)
        p.set_map(np.concatenate([c[2] for c in chroms]), [c[3] for c in chroms], [c[4] for c in chroms])
        p.set_freq(np.concatenate([c[1] for c in chroms]))
        p.set_genotypes(np.ascontiguousarray(np.concatenate([c[0] for c in chroms], axis=0)[:, b:e]))
        panels.append(p)
    return panels


@pytest.mark.parametrize("subset", [False, True], ids=["everyone", "subset"])
def test_lod_kde_part_set_on_two_panels_that_split_one(gpu_ctx, subset):
    whole, a, b = open_panels(gpu_ctx)
    with whole, a, b:
        idx = [2, 5, 11, 17, 30, 40] if subset else None            # the subset leaves the second shard one individual
        split = [None, None] if idx is None else [[i for i in idx if i < CUT], [i - CUT for i in idx if i >= CUT]]
        assert idx is None or len(split[1]) == 1
        one, one_status, per_chr = whole.lod_kde_multi(SIZES, ERROR, MG, ind_idx=idx)
        assert one_status == [abi.OK] * 3
        # the per-size loop: garlic_lod_kde_part on either panel + garlic_kde_parts
        loop = []
        for W in SIZES:
            pa, _ = a.lod_kde_part(W, ERROR, MG, W, ind_idx=split[0])
            pb, _ = b.lod_kde_part(W, ERROR, MG, W, ind_idx=split[1])
            with pa, pb:
                loop.append(abi.kde_parts([pa, pb]))
        sa, chr_a = a.lod_kde_part_set(SIZES, ERROR, MG, ind_idx=split[0])
        sb, chr_b = b.lod_kde_part_set(SIZES, ERROR, MG, ind_idx=split[1])
        with sa, sb:
            assert np.array_equal(chr_a + chr_b, per_chr)
            assert list(sa.counts() + sb.counts()) == [k["n"] for k in one] and (sa.counts() > 0).all() and (sb.counts() > 0).all()
            got, status = abi.kde_parts_multi([sa, sb])
            assert status == [abi.OK] * 3
            for g, w, l in zip(got, one, loop):
                assert same_struct(g, l), "the per-size loop of garlic_lod_kde_part + garlic_kde_parts"
                for k in INT_AND_ORDER:
                    assert np.float64(g[k]).tobytes() == np.float64(w[k]).tobytes(), k
            # a set is stale once its panel computes another feed; the other panel's set is not
            a.lod_feed(SIZES[0], ERROR, MG, SIZES[0])
            for call in (sa.counts, lambda: sa.moment(0), lambda: sa.rank(np.zeros((3, 1), dtype=np.uint64)),
                         lambda: abi.kde_parts_multi([sa, sb]), lambda: abi.kde_parts_multi_info([sa, sb])):
                with pytest.raises(abi.GarlicError) as e:
                    call()
                assert e.value.code == abi.ERR_STATE and "stale" in str(e.value)
            assert (sb.counts() > 0).all()


def test_shard_lod_kde_multi_and_on_shards(gpu_ctx):
    from garlic_amd import shard
    whole, a, b = open_panels(gpu_ctx)
    with whole, a, b:
        got, status = shard.lod_kde_multi(gpu_ctx, [a, b], SIZES, ERROR, MG)
        single, single_status = shard.lod_kde_multi(gpu_ctx, [whole], SIZES, ERROR, MG)
        assert status == single_status == [abi.OK] * 3
        for W, g, s in zip(SIZES, got, single):
            on = shard.lod_kde(gpu_ctx, [a, b], W, ERROR, MG, W, on_shards=True)
            assert same_struct(g, on), W
            merged = shard.lod_kde(gpu_ctx, [a, b], W, ERROR, MG, W)
            for k in INT_AND_ORDER:
                assert np.float64(g[k]).tobytes() == np.float64(s[k]).tobytes() == np.float64(merged[k]).tobytes(), (W, k)
